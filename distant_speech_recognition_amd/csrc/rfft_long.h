// rfft_long.h -- the real transform of L = 2 NF points (L = 256 ... 16384) on fft_long.h's NF-point complex transform, for the
// kernels of tdoa_kernels.hip, fe_kernels.hip and conv_kernels.hip: the even / odd samples packed as one complex sequence in
// LDS, a split step behind the forward transform, a pre-twist step in front of the backward one.  How a kernel fills buf and
// what it does with the bins is its own business.  Below the device functions: what a host needs to launch such a kernel
// (fft_long_host.hip holds the tables).
#pragma once
#include <atomic>
#include <type_traits>
#include "btk_internal.h"
#include "fft_long.h"

constexpr int RFFT_MIN_L = 256, RFFT_MAX_L = 16384;

// threads per transform: one radix-4 butterfly each where a workgroup may be that large or small
template <int LOG2NF> constexpr int rfft_threads = (1 << LOG2NF) / 4 < 64 ? 64 : ((1 << LOG2NF) / 4 > 512 ? 512 : (1 << LOG2NF) / 4);

// split step: bins k and m = NF - k (0 <= k <= NF/2) of the L-point real transform whose packed NF-point complex transform lies
// in buf.  Z = E + i O of the even / odd samples, X[k] = E[k] + w^k O[k], X[NF-k] = conj(E[k] - w^k O[k]), w = exp(-i 2 pi / L);
// k == 0 gives the two real bins 0 and L/2, at k == NF/2 x1 is x0's conjugate (not another bin).  The caller hands in its own
// NF - k, the index it stores x1 under: computed in here it is folded to -k before the call is inlined, and the caller's loop
// then carries both
template <int NF>
__device__ __forceinline__ void rfft_split(const float2* __restrict__ buf, const float2* __restrict__ tw, int k, int m, float2& x0,
                                           float2& x1)
{
  constexpr int TS = BTK_LONGFFT_TWN / (2 * NF);   // table entries per step of exp(-i 2 pi / L)
  const float2 A = buf[k], B = cconjf(buf[m & (NF - 1)]);
  const float2 E = make_float2(0.5f * (A.x + B.x), 0.5f * (A.y + B.y));
  const float2 O = make_float2(0.5f * (A.y - B.y), -0.5f * (A.x - B.x));   // (A - B) / (2 i)
  const float2 wO = k == 0 ? O : cmulf(O, tw[k * TS]);
  x0 = caddf(E, wO);
  x1 = cconjf(csubf(E, wO));
}

// the same with the index computed here (folded, see above): the form for a caller that is the faster for it, as the
// convolution kernels are -- conv_spectrum_kernel's machine code is then what it was with its own copy of this function
template <int NF>
__device__ __forceinline__ void rfft_split(const float2* __restrict__ buf, const float2* __restrict__ tw, int k, float2& x0, float2& x1)
{
  rfft_split<NF>(buf, tw, k, NF - k, x0, x1);
}

// pre-twist step: from the bins Gk = G[k], Gm = G[NF-k] (0 <= k <= NF/2) of a real sequence's spectrum the values zk, zm that
// go to buf[k] and buf[NF-k] in front of the backward NF-point transform, which then leaves z[n] = L (g[2n] + i g[2n+1]):
// Z[k] = (G[k] + conj G[NF-k]) + i v^k (G[k] - conj G[NF-k]), v = exp(+i 2 pi / L).  k == 0 takes Gk = G[0], Gm = G[NF], whose
// imaginary parts are ignored as numpy's irfft ignores them, and has no zm; at k == NF/2 (Gk == Gm) zm is not another value
template <int NF>
__device__ __forceinline__ void rfft_pretwist(float2 Gk, float2 Gm, const float2* __restrict__ tw, int k, float2& zk, float2& zm)
{
  constexpr int TS = BTK_LONGFFT_TWN / (2 * NF);
  if (k == 0) {
    zk = zm = make_float2(Gk.x + Gm.x, Gk.x - Gm.x);
  } else {
    const float2 Sm = make_float2(Gk.x + Gm.x, Gk.y - Gm.y), Df = make_float2(Gk.x - Gm.x, Gk.y + Gm.y);
    const float2 Q = cmulf(Df, cconjf(tw[k * TS]));
    zk = make_float2(Sm.x - Q.y, Sm.y + Q.x);
    zm = make_float2(Sm.x + Q.y, Q.x - Sm.y);
  }
}

// ---- host side.  The tables are built in float64 on the host and uploaded at the first use of a device (of a window length),
// whichever module that comes from; they live as long as the process.
#pragma GCC visibility push(hidden)                // the library exports its C ABI and nothing of this
// fft_long.h's twiddle table, one per device
int longfft_twiddles(const float2** out);
// HammingFeature's window of D points in float64, one per (device, D); who: the entry point an error message names
int longfft_hamming(const char* who, int D, const double** out);
// log2 L for a power of two from RFFT_MIN_L to RFFT_MAX_L, else -1
int longfft_log2(int L);
#pragma GCC visibility pop

// f(std::integral_constant<int, LOG2NF>) for the transform length L = 2^lg, lg = longfft_log2(L) >= 0
template <class F> int longfft_dispatch(int lg, F&& f)
{
  switch (lg - 1) {
    case 7: return f(std::integral_constant<int, 7>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 9: return f(std::integral_constant<int, 9>{});
    case 10: return f(std::integral_constant<int, 10>{});
    case 11: return f(std::integral_constant<int, 11>{});
    case 12: return f(std::integral_constant<int, 12>{});
    default: return f(std::integral_constant<int, 13>{});
  }
}

// a workgroup's LDS may exceed the default limit (it does at the largest transform): raised to lds bytes once per kernel
// instantiation and device; every later call is one atomic load
template <auto Kern> int btk_allow_lds(size_t lds)
{
  static std::atomic<unsigned long long> done{0};
  int dev = 0;
  BTK_HIP_CHECK(hipGetDevice(&dev));
  const unsigned long long bit = 1ull << (dev & 63);
  if (done.load(std::memory_order_acquire) & bit) return BTK_OK;
  BTK_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  done.fetch_or(bit, std::memory_order_release);
  return BTK_OK;
}
