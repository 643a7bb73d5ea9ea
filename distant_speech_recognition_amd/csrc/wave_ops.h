// wave_ops.h -- what the kernels do across the 64 lanes of a wavefront, one definition each: DPP moves, quad and wavefront sums,
// lane broadcasts, the DPP schedule of the wave-wide affine scan, and the operand vectors of the matrix cores.
// The DPP control words and row masks are easy to get wrong and invisible when they are; they are written here and nowhere else:
//   quad_perm [a,b,c,d] = a | b << 2 | c << 4 | d << 6      0xB1 = [1,0,3,2]   0x4E = [2,3,0,1]
//   row_shr:n = 0x110 + n (lane i of a 16-lane row reads lane i - n of the same row)
//   row_bcast:15 = 0x142 (lane 15 of each row to the whole next row), row_bcast:31 = 0x143 (lane 31 to rows 2 and 3)
//   row mask: bit r enables the write in row r (lanes 16 r .. 16 r + 15); bank mask 0xF throughout
// Everything sits in the unnamed namespace (see zd.h).
#pragma once
#include <hip/hip_runtime.h>
#include "zd.h"

// accumulator / operand vectors of v_mfma_f32_16x16x4_f32 and v_mfma_f32_32x32x*
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

// a conj(b), plain multiply-adds (the complex Cholesky solvers)
__device__ __forceinline__ float2 cmul_conj_b(float2 a, float2 b) { return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }

// v of the lane that CTRL names; lanes without a source read 0 (bound_ctrl)
template <int CTRL> __device__ __forceinline__ double dpp_d(double v)
{
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
// v of the lane that CTRL names, in the rows of ROW_MASK; lanes without a source and the other rows get `identity`
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_or(float identity, float v)
{
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, identity), __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xF, false));
}

// sum over the four lanes of a quad, in every lane of it
__device__ __forceinline__ double quad_sum(double v)
{
  v += dpp_d<0xB1>(v);                  // quad_perm [1,0,3,2]
  v += dpp_d<0x4E>(v);                  // quad_perm [2,3,0,1]
  return v;
}
__device__ __forceinline__ zd quad_sum(zd v) { return zmk(quad_sum(v.x), quad_sum(v.y)); }

// sum over the 64 lanes, in every lane.  Butterfly: every lane ends with the same bits (each step adds the same two values in
// either order)
template <class T> __device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ zd wave_sum(zd v) { return zmk(wave_sum(v.x), wave_sum(v.y)); }
// the same butterfly over aligned groups of W lanes (W a power of two <= 64), in every lane of the group
template <int W, class T> __device__ __forceinline__ T group_sum(T v)
{
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// largest value over the 64 lanes, in every lane
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// value of a wavefront-uniform lane
__device__ __forceinline__ double lane_d(double v, int lane)
{
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ zd lane_z(zd v, int lane) { return zmk(lane_d(v.x, lane), lane_d(v.y, lane)); }
// value of lane `l` (compile-time) broadcast to the wavefront through an SGPR
__device__ __forceinline__ float lane_value(float x, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), l)); }

// Inclusive wave-wide scan of affine maps v -> a v + b in the DPP network: four row_shr steps inside the 16-lane rows, then the
// row totals travel with row_bcast:15 (into rows 1 and 3) and row_bcast:31 (into rows 2 and 3).  Lanes without a source keep the
// identity map (the `identity` operand of dpp_or), so no lane tests are needed.  The shuffle form of the same scan was 30
// dependent ds_bpermute round trips per 64-frame chunk.
// step(dpp_ctrl<CTRL>, dpp_rows<ROW_MASK>) composes every lane's map with the map of the lane that CTRL names, fetched with
// dpp_or<CTRL, ROW_MASK>; the step bodies differ from file to file on purpose (pf_, ss_, binaural_kernels.hip) and stay there.
template <int CTRL> struct dpp_ctrl { static constexpr int value = CTRL; };
template <int ROW_MASK> struct dpp_rows { static constexpr int value = ROW_MASK; };
template <class Step>
__device__ __forceinline__ void affine_scan_schedule(Step step)
{
  step(dpp_ctrl<0x111>(), dpp_rows<0xF>());      // row_shr:1
  step(dpp_ctrl<0x112>(), dpp_rows<0xF>());      // row_shr:2
  step(dpp_ctrl<0x114>(), dpp_rows<0xF>());      // row_shr:4
  step(dpp_ctrl<0x118>(), dpp_rows<0xF>());      // row_shr:8
  step(dpp_ctrl<0x142>(), dpp_rows<0xA>());      // row_bcast:15 -> rows 1, 3
  step(dpp_ctrl<0x143>(), dpp_rows<0xC>());      // row_bcast:31 -> rows 2, 3
}

}  // namespace
