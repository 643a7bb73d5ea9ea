// stft_tile.h -- the tile of the windowed FFT bank (NormalFFTAnalysisBank::next, reference modulated/modulated.cc:203-227) that
// stft_kernel (fb_pr_kernels.hip) and the fused Itakura-Saito kernel (obj_kernels.hip) share: plan, tile geometry, PCM staging
// and the window multiply + transform.  Both kernels call stft_tile_spectra with the same template arguments, so a frame's
// spectrum is the same bits whichever kernel made it.
#pragma once
#include "btk_internal.h"
#include "fft_lds.h"
#include <cstdint>
#include <type_traits>

struct btk_stft {
  int M, r, R, D, window_type;
  float* d_win;      // [M]
  float2* d_tw;      // [2*M] e^{+j pi j / M}
};

namespace {

constexpr int NT = 256;                       // threads per workgroup (4 wavefronts)
constexpr size_t LDS_MAX = 160 * 1024;

// N-point complex transforms per workgroup tile: the FFT buffer stays at ~32 KB (two workgroups per CU at M2 = 512 and 1024 with
// m = 4) and every pass of fft_lds tiles the workgroup
template <int LOG2N> struct PrCfg {
  static constexpr int N = 1 << LOG2N;
  static constexpr int TT = N >= 64 ? 4096 / N : (N >= 16 ? 64 : 128);
  static constexpr int STRIDE = N + 1;
};

// PCM span -> LDS: local index l <-> global sample g0 + l, zero outside [0, nsamples)
__device__ __forceinline__ void stage_span(float* xs, const float* src, const float* pcm, long pcm_stride, long nsamples, long g0,
                                           int span, int D, int tid)
{
  const bool vec_ok = ((pcm_stride & 3) == 0) && ((reinterpret_cast<uintptr_t>(pcm) & 15) == 0) && ((g0 & 3) == 0) &&
                      ((D & 3) == 0) && ((span & 3) == 0);
  if (vec_ok && g0 >= 0 && g0 + span <= nsamples) {
    for (int l = tid * 4; l < span; l += NT * 4)
      *reinterpret_cast<float4*>(xs + l) = *reinterpret_cast<const float4*>(src + g0 + l);
  } else {
    for (int l = tid; l < span; l += NT) {
      const long g = g0 + l;
      xs[l] = (g >= 0 && g < nsamples) ? src[g] : 0.0f;
    }
  }
}

// STFT frames of a staged span: zbuf[f][kappa] = sum_i win[i] xs[f D + i] e^{-j 2 pi kappa i/M} for the TT frames of a tile.
// The caller has put a barrier after staging xs and tw; the transform ends with one.
template <int LOG2N>
__device__ __forceinline__ void stft_tile_spectra(float2* zbuf, const float2* tw, const float* xs, const float* __restrict__ win,
                                                  int D, int tid)
{
  using C = PrCfg<LOG2N>;
  constexpr int M = C::N, TT = C::TT, STRIDE = C::STRIDE;
  for (int idx = tid; idx < TT * M; idx += NT) {
    const int f = idx / M, i = idx % M;
    zbuf[f * STRIDE + i] = make_float2(win[i] * xs[f * D + i], 0.0f);
  }
  __syncthreads();
  fft_lds<LOG2N, TT, STRIDE, NT, -1>(zbuf, tw, tid);              // gsl_fft_complex_radix2_forward
}

// one launch per power of two: f(std::integral_constant<int, log2 n>), n in [lo, 2048]
template <class F> int for_log2n(int n, int lo, F f)
{
  if (n >= lo) switch (n) {
    case 8:    return f(std::integral_constant<int, 3>{});
    case 16:   return f(std::integral_constant<int, 4>{});
    case 32:   return f(std::integral_constant<int, 5>{});
    case 64:   return f(std::integral_constant<int, 6>{});
    case 128:  return f(std::integral_constant<int, 7>{});
    case 256:  return f(std::integral_constant<int, 8>{});
    case 512:  return f(std::integral_constant<int, 9>{});
    case 1024: return f(std::integral_constant<int, 10>{});
    case 2048: return f(std::integral_constant<int, 11>{});
  }
  return btk_set_error(BTK_ERR_PARAMETER, "unsupported transform length %d", n);
}

}  // namespace
