// zd.h -- float64 complex numbers of the device code (the float64 recursions: echo cancellation, RLS, covariance designs).
// Products and sums are spelled with fma, so every file that includes this rounds alike.
// Everything sits in the unnamed namespace, like the kernels that take a zd: each translation unit keeps its own internal copy.
#pragma once
#include <hip/hip_runtime.h>

namespace {

struct zd { double x, y; };
__device__ __forceinline__ zd zmk(double x, double y) { zd r; r.x = x; r.y = y; return r; }
__device__ __forceinline__ zd zadd(zd a, zd b) { return zmk(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ zd zsub(zd a, zd b) { return zmk(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ zd zconj(zd a) { return zmk(a.x, -a.y); }
__device__ __forceinline__ zd zscale(zd a, double s) { return zmk(a.x * s, a.y * s); }
__device__ __forceinline__ zd zmul(zd a, zd b) { return zmk(fma(a.x, b.x, -(a.y * b.y)), fma(a.x, b.y, a.y * b.x)); }
__device__ __forceinline__ double zabs2(zd a) { return fma(a.x, a.x, a.y * a.y); }
__device__ __forceinline__ zd zinv(zd a) { const double d = 1.0 / fma(a.x, a.x, a.y * a.y); return zmk(a.x * d, -a.y * d); }
// c + a b
__device__ __forceinline__ zd zfma(zd a, zd b, zd c)
{
  c.x = fma(a.x, b.x, c.x); c.x = fma(-a.y, b.y, c.x);
  c.y = fma(a.x, b.y, c.y); c.y = fma(a.y, b.x, c.y);
  return c;
}
// c - a b
__device__ __forceinline__ zd zfms(zd a, zd b, zd c) { return zfma(zmk(-a.x, -a.y), b, c); }
// c + a conj(b)
__device__ __forceinline__ zd zfmabc(zd a, zd b, zd c)
{
  c.x = fma(a.x, b.x, c.x); c.x = fma(a.y, b.y, c.x);
  c.y = fma(a.y, b.x, c.y); c.y = fma(-a.x, b.y, c.y);
  return c;
}
// c + conj(a) b
__device__ __forceinline__ zd zfmac(zd a, zd b, zd c)
{
  c.x = fma(a.x, b.x, c.x); c.x = fma(a.y, b.y, c.x);
  c.y = fma(a.x, b.y, c.y); c.y = fma(-a.y, b.x, c.y);
  return c;
}

}  // namespace
