// fb_pr_kernels.hip -- the cosine-modulated perfect-reconstruction (PR) filter banks and the plain windowed FFT bank for gfx950.
//
// Replaces PerfectReconstructionFFTAnalysisBank::next, PerfectReconstructionFFTSynthesisBank::next and
// NormalFFTAnalysisBank::next (reference modulated/modulated.cc:683-718, :861-898, :203-227) with whole-tile kernels in the
// arrangement of fb_kernels.hip; all M2 = 2 M bins are complex and independent (no Hermitian symmetry), so the transform is the
// full-length complex FFT of fft_lds.h.
//
// Closed forms (M2 = 2 M, R = 2^r, D = M / R, q = r + 2, pd = 2 m - 1; x = 0 outside the recording):
//   analysis frame t: newest sample n_t = (t + 1) D - 1,
//       p[i] = sum_{k<m} (-1)^k h[i + M2 k] x[n_t - q k D - i],  X_t[kappa] = 1/M2 sum_i p[i] e^{-j pi i/M2} e^{+j 2 pi kappa i/M2}
//       (the ring step is q frames, buffer_.sample((r_+2)*k, m) at :695, NOT 2 R: for r >= 1 the taps are not contiguous in time)
//   synthesis block b: newest input frame f = b + pd,
//       v_f[i] = Re(e^{+j pi i/M2} sum_kappa Y_f[kappa] e^{-j 2 pi kappa i/M2})
//       s_b[i] = sum_{k<m} (-1)^{k+m-1} h[i + M2 (m-1-k)] v_{f - q k}[i]      (frames before 0 are zero)
//       out_b[D-1-d] = sum_{sx<2R} s_{b-(2R-1-sx)}[d + sx D] / R              (float32 running sum in this order, blocks before 0 zero)
//   STFT frame t: X_t[kappa] = sum_{i<M} win[i] x[n_t - M + 1 + i] e^{-j 2 pi kappa i/M}
// The signs (-1)^k are folded into the float32 taps when the plan is made.
#include "btk_internal.h"
#include "fft_lds.h"
#include "stft_tile.h"
#include <cmath>
#include <cstdint>
#include <type_traits>
#include <vector>

struct btk_prfb {
  int M, M2, m, r, R, D, q, pd, synthesis;
  float* d_proto;    // [m*M2] signed taps: analysis (-1)^k h[i + M2 k]; synthesis row k = (-1)^{k+m-1} h[i + M2 (m-1-k)]
  float2* d_tw;      // [2*M2] e^{+j pi j / M2}: the transform's twiddles; entries < M2 are the synthesis rotation
  float2* d_rot;     // [M2]   e^{-j pi i / M2} / M2: the analysis rotation with the inverse transform's factor
};

namespace {

// btk_stft, NT, LDS_MAX, PrCfg, stage_span and for_log2n are stft_tile.h's

// XCD-aware mapping as in fb_kernels.hip: consecutive tiles of one channel share an XCD's L2 (PCM halo reuse)
__device__ __forceinline__ bool tile_of_block(int ntiles, int nchan, int* chan, int* tile)
{
  const int b = blockIdx.x;
  const int xcd = b & 7, slot = b >> 3;
  *chan = (slot / ntiles) * 8 + xcd;
  *tile = slot % ntiles;
  return *chan < nchan;
}

// bins of a tile: for each kappa a run of TT frames (TT*8 B contiguous) of X [S][NB][N][T_stride]
template <int NB, int TT, int STRIDE>
__device__ __forceinline__ void store_bins(const float2* zbuf, float2* X, int chan, int N, long T_stride, long tt0, long tcount, int tid)
{
  const int s = chan / N, nch = chan % N;
  float2* xo = X + ((long)s * NB * N + nch) * T_stride + tt0;
  for (int idx = tid; idx < TT * NB; idx += NT) {
    const int f = idx % TT, k = idx / TT;
    if (tt0 + f < tcount) xo[(long)k * N * T_stride + f] = zbuf[f * STRIDE + k];
  }
}

// ------------------------------------------------------------------ PR analysis
// MT > 0: compile-time prototype length factor m (taps in registers); MT == 0: runtime m.
template <int LOG2N, int MT>
__global__ __launch_bounds__(NT)
void pr_analysis_kernel(const float* __restrict__ pcm, long nsamples, long pcm_stride,
                        const float* __restrict__ proto, const float2* __restrict__ twg, const float2* __restrict__ rotg,
                        int m_rt, int D, int q, int N, float2* __restrict__ X, long T_stride, long t0, long tcount,
                        int ntiles, int nchan)
{
  using C = PrCfg<LOG2N>;
  constexpr int M2 = C::N, TT = C::TT, STRIDE = C::STRIDE;
  const int m = MT > 0 ? MT : m_rt;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float2* zbuf = reinterpret_cast<float2*>(smem);                 // [TT][STRIDE]
  float2* tw = zbuf + TT * STRIDE;                                // [2 M2]
  float* xs = reinterpret_cast<float*>(tw + 2 * M2);              // [(TT-1) D + q (m-1) D + M2]

  const int tid = threadIdx.x;
  int chan, tile;
  if (!tile_of_block(ntiles, nchan, &chan, &tile)) return;
  const long tt0 = (long)tile * TT;                               // first frame of tile, relative to t0
  const long tabs0 = t0 + tt0;                                    // absolute frame number

  for (int j = tid; j < 2 * M2; j += NT) tw[j] = twg[j];

  // local index of x[n_t - q k D - i], t = tabs0 + f:  f D + q (m-1-k) D + M2 - 1 - i
  const int hist = q * (m - 1) * D;
  const int span = (TT - 1) * D + hist + M2;
  const long g0 = (tabs0 + 1) * (long)D - hist - M2;
  stage_span(xs, pcm + (long)chan * pcm_stride, pcm, pcm_stride, nsamples, g0, span, D, tid);
  __syncthreads();

  // ---- polyphase sums times the rotation: z[f][i] = p[i] e^{-j pi i/M2} / M2
  constexpr int NOWN = M2 > NT ? M2 / NT : 1;        // indices i owned by a thread
  constexpr int FPT = M2 > NT ? TT : TT * M2 / NT;   // frames handled per owned i
  constexpr int FSTEP = M2 > NT ? 1 : NT / M2;
  constexpr int MTR = MT > 0 ? MT : 1;
  const int f_first = M2 > NT ? 0 : tid / M2;
  const int qD = q * D;
#pragma unroll
  for (int o = 0; o < NOWN; o++) {
    const int i = M2 > NT ? tid + o * NT : tid % M2;
    const float2 rot = rotg[i];
    float hreg[MTR];
    if (MT > 0) {
#pragma unroll
      for (int k = 0; k < MT; k++) hreg[k] = proto[i + M2 * k];
    }
#pragma unroll 4
    for (int fi = 0; fi < FPT; fi++) {
      const int f = f_first + fi * FSTEP;
      const int base = f * D + hist + M2 - 1 - i;
      float p = 0.0f;
      if (MT > 0) {
#pragma unroll
        for (int k = 0; k < MT; k++) p = fmaf(hreg[k], xs[base - qD * k], p);
      } else {
        for (int k = 0; k < m; k++) p = fmaf(proto[i + M2 * k], xs[base - qD * k], p);
      }
      zbuf[f * STRIDE + i] = make_float2(rot.x * p, rot.y * p);
    }
  }
  __syncthreads();

  // ---- M2-point complex FFT, backward sign (gsl_fft_complex_radix2_inverse; its 1/M2 sits in the rotation table)
  fft_lds<LOG2N, TT, STRIDE, NT, +1>(zbuf, tw, tid);
  store_bins<M2, TT, STRIDE>(zbuf, X, chan, N, T_stride, tt0, tcount, tid);
}

// ------------------------------------------------------------------ windowed FFT (NormalFFTAnalysisBank)
template <int LOG2N>
__global__ __launch_bounds__(NT)
void stft_kernel(const float* __restrict__ pcm, long nsamples, long pcm_stride, const float* __restrict__ win,
                 const float2* __restrict__ twg, int D, int N, float2* __restrict__ X, long T_stride, long t0, long tcount,
                 int ntiles, int nchan)
{
  using C = PrCfg<LOG2N>;
  constexpr int M = C::N, TT = C::TT, STRIDE = C::STRIDE;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float2* zbuf = reinterpret_cast<float2*>(smem);                 // [TT][STRIDE]
  float2* tw = zbuf + TT * STRIDE;                                // [2 M]
  float* xs = reinterpret_cast<float*>(tw + 2 * M);               // [(TT-1) D + M]

  const int tid = threadIdx.x;
  int chan, tile;
  if (!tile_of_block(ntiles, nchan, &chan, &tile)) return;
  const long tt0 = (long)tile * TT;
  const long tabs0 = t0 + tt0;

  for (int j = tid; j < 2 * M; j += NT) tw[j] = twg[j];
  // local index of x[n_t - M + 1 + i], t = tabs0 + f:  f D + i
  const int span = (TT - 1) * D + M;
  const long g0 = (tabs0 + 1) * (long)D - M;
  stage_span(xs, pcm + (long)chan * pcm_stride, pcm, pcm_stride, nsamples, g0, span, D, tid);
  __syncthreads();

  stft_tile_spectra<LOG2N>(zbuf, tw, xs, win, D, tid);
  store_bins<M, TT, STRIDE>(zbuf, X, chan, N, T_stride, tt0, tcount, tid);
}

// ------------------------------------------------------------------ PR synthesis
template <int LOG2N> struct PrSynCfg {
  static constexpr int N = 1 << LOG2N;
  static constexpr int FR = N >= 128 ? (N >= 4096 ? 1 : 4096 / N) : 64;           // frames per FFT round
  static constexpr int STRIDE = N + 1;
  static_assert((FR * N) % 256 == 0, "a round's elements tile the workgroup");
};

// One workgroup: stream s, output blocks [bt0, bt0+TB).  Needs v_f for f in [f_lo, f_hi], f_lo = bt0 + pd - (2R-1) - q (m-1),
// f_hi = bt0 + TB - 1 + pd; the rows live in LDS as vbuf[f - f_lo][M2] floats.  Frames before the tile are recomputed.
// MT > 0: compile-time m, the taps of one polyphase sum are loaded together; MT == 0: runtime m.
template <int LOG2N, int MT>
__global__ __launch_bounds__(NT)
void pr_synthesis_kernel(const float2* __restrict__ Y, long nframes, long T_stride, const float* __restrict__ proto,
                         const float2* __restrict__ twg, int m_rt, int R, int D, int q, int pd, int TB,
                         float* __restrict__ out, long out_stride, long b0, long bcount)
{
  const int m = MT > 0 ? MT : m_rt;
  using C = PrSynCfg<LOG2N>;
  constexpr int M2 = C::N, FR = C::FR, STRIDE = C::STRIDE;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float2* zbuf = reinterpret_cast<float2*>(smem);                 // [FR][STRIDE]
  float2* tw = zbuf + FR * STRIDE;                                // [2 M2]
  float* vbuf = reinterpret_cast<float*>(tw + 2 * M2);            // [NV][M2]
  const int R2 = 2 * R;
  const int NV = TB + R2 - 1 + q * (m - 1);                       // frames of v needed

  const int tid = threadIdx.x;
  const int s = blockIdx.y;
  const long bt0 = b0 + (long)blockIdx.x * TB;
  const long f_lo = bt0 + pd - (R2 - 1) - (long)q * (m - 1);
  const float2* Ys = Y + (long)s * M2 * T_stride;

  for (int j = tid; j < 2 * M2; j += NT) tw[j] = twg[j];
  __syncthreads();

  for (int r0 = 0; r0 < NV; r0 += FR) {
    // all loads of the round are issued before the first is stored: a workgroup has few wavefronts to hide their latency behind
    constexpr int NL = FR * M2 / NT;
    float2 zr[NL];
#pragma unroll
    for (int u = 0; u < NL; u++) {
      const int idx = tid + u * NT;
      const int fr = idx % FR, k = idx / FR;                      // frames fastest: coalesced along t
      const long f = f_lo + r0 + fr;
      zr[u] = make_float2(0.f, 0.f);
      if (r0 + fr < NV && f >= 0 && f < nframes) zr[u] = Ys[(long)k * T_stride + f];
    }
#pragma unroll
    for (int u = 0; u < NL; u++) {
      const int idx = tid + u * NT;
      zbuf[(idx % FR) * STRIDE + idx / FR] = zr[u];
    }
    __syncthreads();
    fft_lds<LOG2N, FR, STRIDE, NT, -1>(zbuf, tw, tid);            // gsl_fft_complex_radix2_forward
    // v[i] = Re(e^{+j pi i/M2} Z[i])  (modulated.cc:852-855)
    for (int idx = tid; idx < FR * M2; idx += NT) {
      const int fr = idx / M2, i = idx % M2;
      if (r0 + fr < NV) {
        const float2 z = zbuf[fr * STRIDE + i], w = tw[i];
        vbuf[(long)(r0 + fr) * M2 + i] = fmaf(z.x, w.x, -z.y * w.y);
      }
    }
    __syncthreads();
  }

  // ---- polyphase + overlap-add in the reference's order with a float32 running sum (modulated.cc:879-895).  Row of
  //      v_{jb + pd - q k} in vbuf, jb = bglob - (2R-1-sx):  bb + sx + q (m-1-k)
  const float invR = 1.0f / (float)R;
  float* os = out + (long)s * out_stride;
  for (int idx = tid; idx < TB * D; idx += NT) {
    const int bb = idx / D, d = idx % D;
    const long bglob = bt0 + bb;
    if (bglob - b0 >= bcount) continue;
    float acc = 0.f;
    for (int sx = 0; sx < R2; sx++) {
      // gsi_ only holds s-frames of earlier next() calls: before block 0 the ring is still zero (nothing is pushed while priming)
      if (bglob - (R2 - 1 - sx) < 0) continue;
      const int i = d + sx * D;
      float sv = 0.f;
      if (MT > 0) {
        float hv[MT > 0 ? MT : 1], vv[MT > 0 ? MT : 1];
#pragma unroll
        for (int k = 0; k < MT; k++) {
          hv[k] = proto[i + M2 * k];
          vv[k] = vbuf[(bb + sx + q * (MT - 1 - k)) * M2 + i];
        }
#pragma unroll
        for (int k = 0; k < MT; k++) sv = fmaf(hv[k], vv[k], sv);
      } else {
        for (int k = 0; k < m; k++)
          sv = fmaf(proto[i + M2 * k], vbuf[(long)(bb + sx + q * (m - 1 - k)) * M2 + i], sv);
      }
      acc += sv * invR;
    }
    os[(bglob - b0) * D + (D - 1 - d)] = acc;
  }
}

// ------------------------------------------------------------------ launchers
template <int LOG2N, int MT>
int launch_pr_analysis_mt(const btk_prfb* fb, const float* pcm, long nsamples, long pcm_stride, int S, int N,
                          float2* X, long T_stride, long t0, long tcount, size_t lds, hipStream_t st)
{
  using C = PrCfg<LOG2N>;
  const int nchan = S * N;
  const int ntiles = (int)((tcount + C::TT - 1) / C::TT);
  const long nblocks = (long)((nchan + 7) / 8) * ntiles * 8;
  auto kern = pr_analysis_kernel<LOG2N, MT>;
  if (lds > 64 * 1024)
    BTK_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)nblocks), dim3(NT), lds, st, pcm, nsamples, pcm_stride, fb->d_proto, fb->d_tw, fb->d_rot,
                     fb->m, fb->D, fb->q, N, X, T_stride, t0, tcount, ntiles, nchan);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

template <int LOG2N>
int launch_pr_analysis(const btk_prfb* fb, const float* pcm, long nsamples, long pcm_stride, int S, int N,
                       float2* X, long T_stride, long t0, long tcount, hipStream_t st)
{
  using C = PrCfg<LOG2N>;
  const size_t lds = sizeof(float2) * (C::TT * C::STRIDE + 2 * C::N) +
                     sizeof(float) * ((size_t)(C::TT - 1) * fb->D + (size_t)fb->q * (fb->m - 1) * fb->D + C::N);
  if (lds > LDS_MAX)
    return btk_set_error(BTK_ERR_PARAMETER, "btk_prfb_analysis: tile needs %zu B of LDS (M=%d m=%d r=%d)", lds, fb->M, fb->m, fb->r);
#define BTK_PR_ANA(MT) return launch_pr_analysis_mt<LOG2N, MT>(fb, pcm, nsamples, pcm_stride, S, N, X, T_stride, t0, tcount, lds, st)
  switch (fb->m) {
    case 1: BTK_PR_ANA(1);
    case 2: BTK_PR_ANA(2);
    case 3: BTK_PR_ANA(3);
    case 4: BTK_PR_ANA(4);
    case 5: BTK_PR_ANA(5);
    case 6: BTK_PR_ANA(6);
    case 7: BTK_PR_ANA(7);
    case 8: BTK_PR_ANA(8);
    default: BTK_PR_ANA(0);
  }
#undef BTK_PR_ANA
}

template <int LOG2N>
int launch_pr_synthesis(const btk_prfb* fb, const float2* Y, long nframes, long T_stride, int S,
                        float* out, long out_stride, long b0, long bcount, hipStream_t st)
{
  using C = PrSynCfg<LOG2N>;
  // TB output blocks per workgroup, bounded by LDS: (TB + 2R - 1 + q (m-1)) rows of M2 floats
  const int extra = 2 * fb->R - 1 + fb->q * (fb->m - 1);
  const long fixed = (long)sizeof(float2) * (C::FR * C::STRIDE + 2 * C::N);
  const long lds_cap = C::N <= 512 ? 96 * 1024 : (long)LDS_MAX;
  long TB = (lds_cap - fixed) / (long)(sizeof(float) * C::N) - extra;
  if (TB > 32) TB = 32;
  if (TB > bcount) TB = bcount;
  if (TB < 1)
    return btk_set_error(BTK_ERR_PARAMETER, "btk_prfb_synthesis: tile does not fit LDS (M=%d m=%d r=%d)", fb->M, fb->m, fb->r);
  const size_t lds = (size_t)fixed + sizeof(float) * (size_t)C::N * (size_t)(TB + extra);
  const unsigned gx = (unsigned)((bcount + TB - 1) / TB);
#define BTK_PR_SYN(MT)                                                                                                          \
  do {                                                                                                                          \
    auto kern = pr_synthesis_kernel<LOG2N, MT>;                                                                                 \
    if (lds > 64 * 1024)                                                                                                        \
      BTK_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
    hipLaunchKernelGGL(kern, dim3(gx, (unsigned)S), dim3(NT), lds, st, Y, nframes, T_stride, fb->d_proto, fb->d_tw, fb->m, fb->R, \
                       fb->D, fb->q, fb->pd, (int)TB, out, out_stride, b0, bcount);                                             \
  } while (0)
  switch (fb->m) {
    case 1: BTK_PR_SYN(1); break;
    case 2: BTK_PR_SYN(2); break;
    case 3: BTK_PR_SYN(3); break;
    case 4: BTK_PR_SYN(4); break;
    default: BTK_PR_SYN(0); break;
  }
#undef BTK_PR_SYN
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

template <int LOG2N>
int launch_stft(const btk_stft* fb, const float* pcm, long nsamples, long pcm_stride, int S, int N,
                float2* X, long T_stride, long t0, long tcount, hipStream_t st)
{
  using C = PrCfg<LOG2N>;
  const int nchan = S * N;
  const int ntiles = (int)((tcount + C::TT - 1) / C::TT);
  const long nblocks = (long)((nchan + 7) / 8) * ntiles * 8;
  const size_t lds = sizeof(float2) * (C::TT * C::STRIDE + 2 * C::N) + sizeof(float) * ((size_t)(C::TT - 1) * fb->D + C::N);
  if (lds > LDS_MAX) return btk_set_error(BTK_ERR_PARAMETER, "btk_stft_analysis: tile needs %zu B of LDS", lds);
  auto kern = stft_kernel<LOG2N>;
  if (lds > 64 * 1024)
    BTK_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)nblocks), dim3(NT), lds, st, pcm, nsamples, pcm_stride, fb->d_win, fb->d_tw, fb->D, N,
                     X, T_stride, t0, tcount, ntiles, nchan);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

bool pow2_in(int n, int lo, int hi) { return n >= lo && n <= hi && (n & (n - 1)) == 0; }

// tw[j] = e^{+j pi j / n}, j < 2 n, on the device
int upload_twiddles(int n, float2** d_tw)
{
  std::vector<float2> tw(2 * (size_t)n);
  for (int j = 0; j < 2 * n; j++) {
    const double a = M_PI * (double)j / (double)n;
    tw[j] = make_float2((float)std::cos(a), (float)std::sin(a));
  }
  BTK_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(d_tw), sizeof(float2) * tw.size()));
  BTK_HIP_CHECK(hipMemcpy(*d_tw, tw.data(), sizeof(float2) * tw.size(), hipMemcpyHostToDevice));
  return BTK_OK;
}

}  // namespace

extern "C" {

// get_window (modulated.cc:47-72): 0 rectangular, 2 Hann, anything else Hamming
int btk_get_window(int type, int len, double* out)
{
  if (len < 0 || (len > 0 && !out)) return btk_set_error(BTK_ERR_PARAMETER, "btk_get_window: bad argument");
  switch (type) {
    case 0:
      for (int i = 0; i < len; i++) out[i] = 1.0;
      break;
    case 2:
      for (int i = 0; i < len; i++) out[i] = 0.5 * (1 - std::cos((2.0 * M_PI * i) / (double)(len - 1)));
      break;
    default: {
      const double temp = 2. * M_PI / (double)(len - 1);
      for (int i = 0; i < len; i++) out[i] = 0.54 - 0.46 * std::cos(temp * i);
      break;
    }
  }
  return BTK_OK;
}

// PerfectReconstructionFilterBank ctor (modulated.cc:284-300)
int btk_prfb_create(btk_prfb_t** out, int M, int m, int r, int synthesis, const double* prototype, long prototype_len)
{
  if (!out || !prototype) return btk_set_error(BTK_ERR_PARAMETER, "btk_prfb_create: null argument");
  if (!pow2_in(M, 8, 1024)) return btk_set_error(BTK_ERR_PARAMETER, "btk_prfb_create: M=%d must be a power of two in [8, 1024]", M);
  if (m < 1 || m > 64) return btk_set_error(BTK_ERR_PARAMETER, "btk_prfb_create: m=%d out of range [1, 64]", m);
  if (r < 0 || r > 2) return btk_set_error(BTK_ERR_PARAMETER, "btk_prfb_create: r=%d out of range [0, 2]", r);
  if (prototype_len != 2L * M * m)
    return btk_set_error(BTK_ERR_CONSISTENCY, "Prototype sizes do not match (%d vs. %d).", (int)prototype_len, 2 * M * m);
  btk_prfb* fb = new btk_prfb();
  fb->M = M; fb->M2 = 2 * M; fb->m = m; fb->r = r; fb->R = 1 << r; fb->D = M / fb->R; fb->q = r + 2; fb->pd = 2 * m - 1;
  fb->synthesis = synthesis ? 1 : 0;
  fb->d_proto = nullptr; fb->d_tw = nullptr; fb->d_rot = nullptr;
  const int M2 = fb->M2;
  std::vector<float> hp((size_t)m * M2);
  for (int k = 0; k < m; k++)
    for (int i = 0; i < M2; i++) {
      // analysis :694-697 flip = (-1)^k on polyphase(i, k); synthesis :881-886 flip = (-1)^{k+m-1} on polyphase(i, m-k-1)
      const int row = synthesis ? m - 1 - k : k;
      const int neg = synthesis ? (k + m - 1) & 1 : k & 1;
      const float h = (float)prototype[(size_t)i + (size_t)M2 * row];
      hp[(size_t)i + (size_t)M2 * k] = neg ? -h : h;
    }
  std::vector<float2> rot(M2);
  for (int i = 0; i < M2; i++) {
    const double a = -M_PI * (double)i / (double)M2;
    rot[i] = make_float2((float)(std::cos(a) / M2), (float)(std::sin(a) / M2));
  }
  int rc = upload_twiddles(M2, &fb->d_tw);
  hipError_t e = hipSuccess;
  if (rc == BTK_OK) {
    e = hipMalloc(reinterpret_cast<void**>(&fb->d_proto), sizeof(float) * hp.size());
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&fb->d_rot), sizeof(float2) * rot.size());
    if (e == hipSuccess) e = hipMemcpy(fb->d_proto, hp.data(), sizeof(float) * hp.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(fb->d_rot, rot.data(), sizeof(float2) * rot.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess)
      rc = btk_set_error(e == hipErrorOutOfMemory ? BTK_ERR_ALLOCATION : BTK_ERR_HIP, "btk_prfb_create: %s", hipGetErrorString(e));
  }
  if (rc != BTK_OK) { btk_prfb_destroy(fb); return rc; }
  *out = fb;
  return BTK_OK;
}

void btk_prfb_destroy(btk_prfb_t* fb)
{
  if (!fb) return;
  if (fb->d_proto) (void)hipFree(fb->d_proto);
  if (fb->d_tw) (void)hipFree(fb->d_tw);
  if (fb->d_rot) (void)hipFree(fb->d_rot);
  delete fb;
}

int btk_prfb_processing_delay(const btk_prfb_t* fb) { return fb ? fb->pd : -1; }

// every input block yields a frame, then processing_delay zero-padded frames (update_buffer_, modulated.cc:727-756)
long btk_prfb_num_frames(const btk_prfb_t* fb, long nsamples)
{
  if (!fb || nsamples < 0) return -1;
  return (nsamples + fb->D - 1) / fb->D + fb->pd;
}

long btk_prfb_num_blocks(const btk_prfb_t* fb, long nframes)
{
  if (!fb) return -1;
  return nframes > fb->pd ? nframes - fb->pd : 0;
}

int btk_prfb_analysis(const btk_prfb_t* fb, const float* pcm, long nsamples, long pcm_stride, int S, int N, void* X,
                      long T_stride, long t0, long tcount, void* stream)
{
  if (!fb || fb->synthesis) return btk_set_error(BTK_ERR_PARAMETER, "btk_prfb_analysis: not an analysis plan");
  if (S <= 0 || N <= 0 || nsamples < 0 || t0 < 0 || tcount < 0 || T_stride < tcount || pcm_stride < nsamples)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_prfb_analysis: bad sizes S=%d N=%d t0=%ld tcount=%ld T_stride=%ld", S, N, t0, tcount, T_stride);
  if (tcount == 0) return BTK_OK;
  if (!X || (!pcm && nsamples > 0)) return btk_set_error(BTK_ERR_PARAMETER, "btk_prfb_analysis: null argument");
  hipStream_t st = as_stream(stream);
  return for_log2n(fb->M2, 16, [&](auto L) {
    if constexpr (decltype(L)::value >= 4)
      return launch_pr_analysis<decltype(L)::value>(fb, pcm, nsamples, pcm_stride, S, N, static_cast<float2*>(X), T_stride, t0, tcount, st);
    else return (int)BTK_ERR_PARAMETER;
  });
}

int btk_prfb_synthesis(const btk_prfb_t* fb, const void* Y, long nframes, long T_stride, int S, float* out, long out_stride,
                       long b0, long bcount, void* stream)
{
  if (!fb || !fb->synthesis) return btk_set_error(BTK_ERR_PARAMETER, "btk_prfb_synthesis: not a synthesis plan");
  if (S <= 0 || b0 < 0 || bcount < 0 || nframes < 0 || nframes > T_stride || out_stride < bcount * fb->D)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_prfb_synthesis: bad sizes S=%d b0=%ld bcount=%ld nframes=%ld T_stride=%ld", S, b0, bcount, nframes, T_stride);
  if (bcount == 0) return BTK_OK;
  if (!out || (!Y && nframes > 0)) return btk_set_error(BTK_ERR_PARAMETER, "btk_prfb_synthesis: null argument");
  hipStream_t st = as_stream(stream);
  return for_log2n(fb->M2, 16, [&](auto L) {
    if constexpr (decltype(L)::value >= 4)
      return launch_pr_synthesis<decltype(L)::value>(fb, static_cast<const float2*>(Y), nframes, T_stride, S, out, out_stride, b0, bcount, st);
    else return (int)BTK_ERR_PARAMETER;
  });
}

// NormalFFTAnalysisBank ctor (modulated.cc:96-132)
int btk_stft_create(btk_stft_t** out, int M, int r, int window_type)
{
  if (!out) return btk_set_error(BTK_ERR_PARAMETER, "btk_stft_create: null argument");
  if (!pow2_in(M, 8, 2048)) return btk_set_error(BTK_ERR_PARAMETER, "btk_stft_create: M=%d must be a power of two in [8, 2048]", M);
  if (r < 0 || (M >> r) < 1) return btk_set_error(BTK_ERR_PARAMETER, "btk_stft_create: r=%d leaves no frame shift", r);
  btk_stft* fb = new btk_stft();
  fb->M = M; fb->r = r; fb->R = 1 << r; fb->D = M / fb->R; fb->window_type = window_type;
  fb->d_win = nullptr; fb->d_tw = nullptr;
  std::vector<double> w(M);
  btk_get_window(window_type, M, w.data());
  std::vector<float> wf(w.begin(), w.end());
  int rc = upload_twiddles(M, &fb->d_tw);
  if (rc == BTK_OK) {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&fb->d_win), sizeof(float) * M);
    if (e == hipSuccess) e = hipMemcpy(fb->d_win, wf.data(), sizeof(float) * M, hipMemcpyHostToDevice);
    if (e != hipSuccess)
      rc = btk_set_error(e == hipErrorOutOfMemory ? BTK_ERR_ALLOCATION : BTK_ERR_HIP, "btk_stft_create: %s", hipGetErrorString(e));
  }
  if (rc != BTK_OK) { btk_stft_destroy(fb); return rc; }
  *out = fb;
  return BTK_OK;
}

void btk_stft_destroy(btk_stft_t* fb)
{
  if (!fb) return;
  if (fb->d_win) (void)hipFree(fb->d_win);
  if (fb->d_tw) (void)hipFree(fb->d_tw);
  delete fb;
}

// every input block yields a frame, then one zero-padded frame (processing_delay_ = 2 * 1 - 1, modulated.cc:105, :162-201)
long btk_stft_num_frames(const btk_stft_t* fb, long nsamples)
{
  if (!fb || nsamples < 0) return -1;
  return (nsamples + fb->D - 1) / fb->D + 1;
}

int btk_stft_analysis(const btk_stft_t* fb, const float* pcm, long nsamples, long pcm_stride, int S, int N, void* X,
                      long T_stride, long t0, long tcount, void* stream)
{
  if (!fb) return btk_set_error(BTK_ERR_PARAMETER, "btk_stft_analysis: null plan");
  if (S <= 0 || N <= 0 || nsamples < 0 || t0 < 0 || tcount < 0 || T_stride < tcount || pcm_stride < nsamples)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_stft_analysis: bad sizes S=%d N=%d t0=%ld tcount=%ld T_stride=%ld", S, N, t0, tcount, T_stride);
  if (tcount == 0) return BTK_OK;
  if (!X || (!pcm && nsamples > 0)) return btk_set_error(BTK_ERR_PARAMETER, "btk_stft_analysis: null argument");
  hipStream_t st = as_stream(stream);
  return for_log2n(fb->M, 8, [&](auto L) {
    return launch_stft<decltype(L)::value>(fb, pcm, nsamples, pcm_stride, S, N, static_cast<float2*>(X), T_stride, t0, tcount, st);
  });
}

}  // extern "C"
