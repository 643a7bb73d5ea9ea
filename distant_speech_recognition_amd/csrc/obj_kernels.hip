// obj_kernels.hip -- objective measures of objective_measure/objective_measure.cc for gfx950: the signal-to-noise ratio of
// calcSNR (:42-185) batched over pairs of signals, its segment rows, and the Itakura-Saito distance of calcISDistance (:284-331)
// fused with the windowed FFT bank.
//
// Arithmetic rule: element-wise values (centred and scaled samples, differences, bin powers, ratios) are float32 as in the
// reference; every sum is float64 in an order fixed by the sample / bin / frame index alone -- it does not depend on the batch,
// on a pair's place in it, on the strides or on which optional outputs are asked for.  No floating-point atomics.
// The file is compiled with -ffp-contract=off: v1 - v2 = x1 a1 - x2 a2 must round both products (csrc/Makefile).
//
// SNR, per pair (closed forms in include/btkhip.h).  A signal is cut into chunks of OBJ_CH = 16384 samples, one workgroup each;
// thread `tid` owns the samples (256 k + tid) 4 + j of a chunk, k < 16, j < 4, and adds them in that order (64 additions), the 64
// lanes of a wavefront are added by the butterfly of wave_ops.h (6), the four wavefronts in order (3), and the chunks of a pair
// by lane c mod 64 in order and the butterfly again (ceil(chunks / 64) + 6): the longest chain of additions behind a sum is
// 79 + ceil(chunks / 64).  Up to three passes -- the means (option bit 1), the scale statistics (bits 2, 4, 8), the sums -- each
// a kernel that writes partials per chunk; the next pass's workgroups each finish the previous totals themselves, in the same
// order, so no pass needs a finishing launch but the last.
//
// Itakura-Saito distance: one workgroup per (pair, tile of PrCfg::TT frames) stages both PCM spans in LDS, transforms signal 1
// with stft_tile_spectra (the bits of stft_kernel), keeps P1, transforms signal 2 in the same buffer, and reduces the M/2 terms
// of a frame over min(M/2, 64) lanes: lane l adds the bins l + 1, l + 1 + 64, ... in order, then the butterfly.  A second
// kernel adds the frames in range per pair: thread tid the frames lo + tid + 256 k in order, butterfly, four wavefronts in order.
#include "btk_internal.h"
#include "stft_tile.h"
#include "wave_ops.h"
#include <algorithm>
#include <cfloat>
#include <cmath>

namespace {

constexpr int OBJ_CH = 16384;        // samples of a chunk
constexpr int OBJ_PAIRS = 64;        // pairs of a launch: their lengths travel as kernel arguments
constexpr int NPQ = 10;              // partials per (pair, chunk)
enum { Q_X1 = 0, Q_X2, Q_MAX1, Q_MAX2, Q_S11, Q_S22, Q_S12, Q_SPARE, Q_SUM, Q_ERR };

struct ObjLens { long n1[OBJ_PAIRS], n2[OBJ_PAIRS]; };

__device__ __forceinline__ int chunks_of(long n) { return (int)((n + OBJ_CH - 1) / OBJ_CH); }

// f(i, x1, has1, x2, has2) for the samples of chunk `c` that thread `tid` owns, in the thread's order
template <class F>
__device__ __forceinline__ void for_owned(const float* __restrict__ r1, long n1, const float* __restrict__ r2, long n2, int c, int tid, F f)
{
  const bool al1 = (reinterpret_cast<uintptr_t>(r1) & 15) == 0, al2 = (reinterpret_cast<uintptr_t>(r2) & 15) == 0;
  const long nmax = n1 > n2 ? n1 : n2;
#pragma unroll 4
  for (int k = 0; k < OBJ_CH / (NT * 4); k++) {
    const long i0 = (long)c * OBJ_CH + ((long)k * NT + tid) * 4;
    if (i0 >= nmax) break;
    float a[4], b[4];
    if (al1 && i0 + 4 <= n1) { const float4 t = *reinterpret_cast<const float4*>(r1 + i0); a[0] = t.x; a[1] = t.y; a[2] = t.z; a[3] = t.w; }
    else
      for (int j = 0; j < 4; j++) a[j] = i0 + j < n1 ? r1[i0 + j] : 0.0f;
    if (al2 && i0 + 4 <= n2) { const float4 t = *reinterpret_cast<const float4*>(r2 + i0); b[0] = t.x; b[1] = t.y; b[2] = t.z; b[3] = t.w; }
    else
      for (int j = 0; j < 4; j++) b[j] = i0 + j < n2 ? r2[i0 + j] : 0.0f;
#pragma unroll
    for (int j = 0; j < 4; j++) f(i0 + j, a[j], i0 + j < n1, b[j], i0 + j < n2);
  }
}

// totals of K values over the workgroup, in every thread: butterfly in the wavefront, then the four wavefronts in order
template <int K> __device__ __forceinline__ void block_sum(double (&v)[K], double* sh, int tid)
{
#pragma unroll
  for (int q = 0; q < K; q++) v[q] = wave_sum(v[q]);
  __syncthreads();
  if ((tid & 63) == 0)
    for (int q = 0; q < K; q++) sh[(tid >> 6) * K + q] = v[q];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < K; q++) v[q] = ((sh[q] + sh[K + q]) + sh[2 * K + q]) + sh[3 * K + q];
}

// total of partial q over the nc chunks of a pair, in every lane: lane l adds chunks l, l + 64, ... in order, then the butterfly
__device__ __forceinline__ double pair_total(const double* __restrict__ part, int nc, int q, int lane)
{
  double a = 0.0;
  for (int c = lane; c < nc; c += 64) a += part[(long)c * NPQ + q];
  return wave_sum(a);
}
__device__ __forceinline__ float pair_max(const double* __restrict__ part, int nc, int q, int lane)
{
  float m = -10000.0f;
  for (int c = lane; c < nc; c += 64) m = fmaxf(m, (float)part[(long)c * NPQ + q]);
  return wave_max(m);
}

struct ObjScale { float mu1, mu2, a1, a2; };

__device__ __forceinline__ void pair_means(const double* __restrict__ part, int nc, long n1, long n2, int option, int lane, ObjScale* sc)
{
  sc->mu1 = sc->mu2 = 0.0f;
  if (option & 1) {
    sc->mu1 = (float)(pair_total(part, nc, Q_X1, lane) / (double)n1);
    sc->mu2 = (float)(pair_total(part, nc, Q_X2, lane) / (double)n2);
  }
}
// 2 over 4 over 8 (:93-131).  A float32 quotient of float32 operands is formed in float64 and rounded: 53 >= 2 * 24 + 2 bits make
// the double rounding harmless, and the result does not hang on the compiler's float32 division.
__device__ __forceinline__ void pair_scales(const double* __restrict__ part, int nc, long n1, long n2, int option, int lane, ObjScale* sc)
{
  pair_means(part, nc, n1, n2, option, lane, sc);
  sc->a1 = sc->a2 = 1.0f;
  if (option & 2) {
    sc->a1 = (float)(1.0 / (double)pair_max(part, nc, Q_MAX1, lane));
    sc->a2 = (float)(1.0 / (double)pair_max(part, nc, Q_MAX2, lane));
  } else if (option & 4) {
    const double p1 = pair_total(part, nc, Q_S11, lane) / (double)n1, p2 = pair_total(part, nc, Q_S22, lane) / (double)n2;
    sc->a2 = (float)sqrt(p1 / p2);
  } else if (option & 8) {
    sc->a2 = (float)(pair_total(part, nc, Q_S12, lane) / pair_total(part, nc, Q_S22, lane));
  }
}

struct SnrArgs {
  const float* x1; long stride1;
  const float* x2; long stride2;
  int s0, option, nchunk;            // first pair of the launch; partial rows per pair
  double* part;                      // [S][nchunk][NPQ]
};

#define OBJ_PAIR_PROLOGUE                                                        \
  const int tid = threadIdx.x, c = blockIdx.x, p = blockIdx.y;                   \
  const long n1 = lens.n1[p], n2 = lens.n2[p];                                   \
  const int nc = chunks_of(n1 > n2 ? n1 : n2);                                   \
  if (c >= nc) return;                                                           \
  const long s = a.s0 + p;                                                       \
  const float* r1 = a.x1 + s * a.stride1;                                        \
  const float* r2 = a.x2 + s * a.stride2;                                        \
  double* part = a.part + s * a.nchunk * NPQ;                                    \
  __shared__ double sh[4 * 4]

// pass 1: sum x_c over i < n_c
__global__ __launch_bounds__(NT) void snr_mean_kernel(SnrArgs a, ObjLens lens)
{
  OBJ_PAIR_PROLOGUE;
  double v[2] = {0.0, 0.0};
  for_owned(r1, n1, r2, n2, c, tid, [&](long, float x1, bool h1, float x2, bool h2) {
    if (h1) v[0] += (double)x1;
    if (h2) v[1] += (double)x2;
  });
  block_sum(v, sh, tid);
  if (tid == 0) { part[(long)c * NPQ + Q_X1] = v[0]; part[(long)c * NPQ + Q_X2] = v[1]; }
}

// pass 2: signed maxima (initial value -10000), sum x1^2, sum x2^2, sum_{i < n2} x1 x2 of the centred samples
__global__ __launch_bounds__(NT) void snr_scale_kernel(SnrArgs a, ObjLens lens)
{
  OBJ_PAIR_PROLOGUE;
  ObjScale sc;
  pair_means(part, nc, n1, n2, a.option, tid & 63, &sc);
  double v[3] = {0.0, 0.0, 0.0};
  float m1 = -10000.0f, m2 = -10000.0f;
  for_owned(r1, n1, r2, n2, c, tid, [&](long, float x1, bool h1, float x2, bool h2) {
    const float c1 = x1 - sc.mu1, c2 = x2 - sc.mu2;
    if (h1) { m1 = fmaxf(m1, c1); v[0] += (double)c1 * (double)c1; }
    if (h2) { m2 = fmaxf(m2, c2); v[1] += (double)c2 * (double)c2; }
    if (h1 && h2) v[2] += (double)c1 * (double)c2;
  });
  block_sum(v, sh, tid);
  m1 = wave_max(m1); m2 = wave_max(m2);
  __shared__ float shm[8];
  if ((tid & 63) == 0) { shm[tid >> 6] = m1; shm[4 + (tid >> 6)] = m2; }
  __syncthreads();
  if (tid == 0) {
    double* o = part + (long)c * NPQ;
    o[Q_MAX1] = (double)fmaxf(fmaxf(shm[0], shm[1]), fmaxf(shm[2], shm[3]));
    o[Q_MAX2] = (double)fmaxf(fmaxf(shm[4], shm[5]), fmaxf(shm[6], shm[7]));
    o[Q_S11] = v[0]; o[Q_S22] = v[1]; o[Q_S12] = v[2];
  }
}

// pass 3: sum and err; the longer signal's tail adds v^2 to both (:159-176)
__global__ __launch_bounds__(NT) void snr_sum_kernel(SnrArgs a, ObjLens lens)
{
  OBJ_PAIR_PROLOGUE;
  ObjScale sc;
  pair_scales(part, nc, n1, n2, a.option, tid & 63, &sc);
  double v[2] = {0.0, 0.0};
  for_owned(r1, n1, r2, n2, c, tid, [&](long, float x1, bool h1, float x2, bool h2) {
    const float v1 = (x1 - sc.mu1) * sc.a1, v2 = (x2 - sc.mu2) * sc.a2;
    if (h1 && h2) {
      const float d = v1 - v2;
      v[0] += (double)v1 * (double)v1;
      v[1] += (double)d * (double)d;
    } else if (h1 || h2) {
      const double t = h1 ? (double)v1 * (double)v1 : (double)v2 * (double)v2;
      v[0] += t;
      v[1] += t;
    }
  });
  block_sum(v, sh, tid);
  if (tid == 0) { part[(long)c * NPQ + Q_SUM] = v[0]; part[(long)c * NPQ + Q_ERR] = v[1]; }
}

// finish: one wavefront per pair writes mu1, mu2, a1, a2, sum, err
__global__ __launch_bounds__(64) void snr_finish_kernel(SnrArgs a, ObjLens lens, double* __restrict__ stats)
{
  const int lane = threadIdx.x, p = blockIdx.x;
  const long n1 = lens.n1[p], n2 = lens.n2[p], s = a.s0 + p;
  const int nc = chunks_of(n1 > n2 ? n1 : n2);
  const double* part = a.part + s * a.nchunk * NPQ;
  ObjScale sc;
  pair_scales(part, nc, n1, n2, a.option, lane, &sc);
  const double sum = pair_total(part, nc, Q_SUM, lane), err = pair_total(part, nc, Q_ERR, lane);
  if (lane == 0) {
    double* o = stats + s * 6;
    o[0] = sc.mu1; o[1] = sc.mu2; o[2] = sc.a1; o[3] = sc.a2; o[4] = sum; o[5] = err;
  }
}

// segment rows: one wavefront per whole segment of L samples below nmin; lane l adds the samples l, l + 64, ... of it in order
__global__ __launch_bounds__(NT) void snr_segment_kernel(SnrArgs a, ObjLens lens, const double* __restrict__ stats, long L,
                                                         double* __restrict__ seg, long seg_stride)
{
  const int lane = threadIdx.x & 63, p = blockIdx.y;
  const long n1 = lens.n1[p], n2 = lens.n2[p], s = a.s0 + p;
  const long B = (n1 < n2 ? n1 : n2) / L;
  const long b = (long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* r1 = a.x1 + s * a.stride1;
  const float* r2 = a.x2 + s * a.stride2;
  const float mu1 = (float)stats[s * 6 + 0], mu2 = (float)stats[s * 6 + 1], a1 = (float)stats[s * 6 + 2], a2 = (float)stats[s * 6 + 3];
  double sum = 0.0, err = 0.0;
  for (long i = b * L + lane; i < (b + 1) * L; i += 64) {
    const float v1 = (r1[i] - mu1) * a1, v2 = (r2[i] - mu2) * a2;
    const float d = v1 - v2;
    sum += (double)v1 * (double)v1;
    err += (double)d * (double)d;
  }
  sum = wave_sum(sum); err = wave_sum(err);
  if (lane == 0) { seg[(s * seg_stride + b) * 2] = sum; seg[(s * seg_stride + b) * 2 + 1] = err; }
}

// ------------------------------------------------------------------ Itakura-Saito distance
__device__ __forceinline__ long frames_of(long n, int D) { return (n + D - 1) / D + 1; }

template <int LOG2N>
__global__ __launch_bounds__(NT)
void is_tile_kernel(const float* __restrict__ x1, long stride1, const float* __restrict__ x2, long stride2, ObjLens lens, int s0,
                    const float* __restrict__ win, const float2* __restrict__ twg, int D, double* __restrict__ eis, long e_stride)
{
  using C = PrCfg<LOG2N>;
  constexpr int M = C::N, TT = C::TT, STRIDE = C::STRIDE, H = M / 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float2* zbuf = reinterpret_cast<float2*>(smem);                 // [TT][STRIDE]
  float2* tw = zbuf + TT * STRIDE;                                // [2 M]
  const int span = (TT - 1) * D + M, span4 = (span + 3) & ~3;
  float* xs1 = reinterpret_cast<float*>(tw + 2 * M);              // [span4]
  float* xs2 = xs1 + span4;                                       // [span4]
  float* p1 = xs2 + span4;                                        // [TT][H]: P1 of the bins 1 .. M/2

  const int tid = threadIdx.x, p = blockIdx.y;
  const long n1 = lens.n1[p], n2 = lens.n2[p], s = s0 + p;
  const long F1 = frames_of(n1, D), F2 = frames_of(n2, D), F = F1 < F2 ? F1 : F2;
  const long tt0 = (long)blockIdx.x * TT;
  if (tt0 >= F) return;

  for (int j = tid; j < 2 * M; j += NT) tw[j] = twg[j];
  const long g0 = (tt0 + 1) * (long)D - M;
  const float* r1 = x1 + s * stride1;
  const float* r2 = x2 + s * stride2;
  stage_span(xs1, r1, r1, 0, n1, g0, span, D, tid);
  stage_span(xs2, r2, r2, 0, n2, g0, span, D, tid);
  __syncthreads();

  stft_tile_spectra<LOG2N>(zbuf, tw, xs1, win, D, tid);
  for (int idx = tid; idx < TT * H; idx += NT) {
    const float2 z = zbuf[(idx / H) * STRIDE + idx % H + 1];
    p1[idx] = (float)((double)z.x * (double)z.x + (double)z.y * (double)z.y);
  }
  __syncthreads();
  stft_tile_spectra<LOG2N>(zbuf, tw, xs2, win, D, tid);

  constexpr int LPF = H < 64 ? H : 64;                            // lanes of a frame
  constexpr int FPP = NT / LPF;                                   // frames of a round
  const int l = tid % LPF;
  for (int f0 = 0; f0 < TT; f0 += FPP) {
    const int f = f0 + tid / LPF;
    const bool live = f < TT && tt0 + f < F;
    double acc = 0.0;
    if (live)
      for (int k = l; k < H; k += LPF) {
        const float2 z = zbuf[f * STRIDE + k + 1];
        const float P2 = (float)((double)z.x * (double)z.x + (double)z.y * (double)z.y);
        const float P1 = p1[f * H + k];
        if (P1 > 0.0f && P2 > 0.0f) {
          const double ratio = (double)(float)((double)P1 / (double)P2);
          acc += ratio - log(ratio) - 1.0;
        }
      }
    acc = group_sum<LPF>(acc);
    if (live && l == 0) eis[s * e_stride + tt0 + f] = acc / (double)H;
  }
}

// mean of Eis over lo <= t < hi per pair; no frame in range gives the reference's 0/0
__global__ __launch_bounds__(NT)
void is_mean_kernel(const double* __restrict__ eis, long e_stride, ObjLens lens, int s0, int D, long bframe, long eframe,
                    double* __restrict__ dist, long long* __restrict__ count)
{
  const int tid = threadIdx.x, p = blockIdx.x;
  const long n1 = lens.n1[p], n2 = lens.n2[p], s = s0 + p;
  const long F1 = frames_of(n1, D), F2 = frames_of(n2, D), F = F1 < F2 ? F1 : F2;
  const long lo = bframe, hi = (eframe >= 0 && eframe + 1 < F) ? eframe + 1 : F;
  __shared__ double sh[4];
  double v[1] = {0.0};
  for (long t = lo + tid; t < hi; t += NT) v[0] += eis[s * e_stride + t];
  block_sum(v, sh, tid);
  if (tid == 0) {
    const long cnt = hi > lo ? hi - lo : 0;
    dist[s] = cnt > 0 ? v[0] / (double)cnt : __longlong_as_double(0x7ff8000000000000LL);
    count[s] = cnt;
  }
}

template <int LOG2N> size_t is_lds_bytes(int D)
{
  using C = PrCfg<LOG2N>;
  const size_t span4 = ((size_t)(C::TT - 1) * D + C::N + 3) & ~(size_t)3;
  return sizeof(float2) * (C::TT * C::STRIDE + 2 * C::N) + sizeof(float) * (2 * span4 + (size_t)C::TT * (C::N / 2));
}

int check_lengths(const char* who, int S, const long* n1, const long* n2, long nlow, long stride1, long stride2, long* nmax)
{
  if (S < 1 || S > 65535 * OBJ_PAIRS) return btk_set_error(BTK_ERR_DIMENSION, "%s: S=%d out of range", who, S);
  if (!n1 || !n2) return btk_set_error(BTK_ERR_PARAMETER, "%s: null argument", who);
  *nmax = 0;
  for (int s = 0; s < S; s++) {
    if (n1[s] < nlow || n2[s] < nlow || n1[s] > stride1 || n2[s] > stride2)
      return btk_set_error(BTK_ERR_DIMENSION, "%s: pair %d has lengths %ld, %ld in rows of %ld, %ld", who, s, n1[s], n2[s], stride1, stride2);
    *nmax = std::max(*nmax, std::max(n1[s], n2[s]));
  }
  return BTK_OK;
}

}  // namespace

extern "C" {

long btk_obj_snr_workspace_bytes(int S, long nmax)
{
  if (S < 1 || nmax < 1) return -1;
  return (long)sizeof(double) * NPQ * S * ((nmax + OBJ_CH - 1) / OBJ_CH);
}

int btk_obj_snr(const float* x1, long stride1, const float* x2, long stride2, int S, const long* n1, const long* n2, int option,
                double* stats, long seg_len, double* seg, long seg_stride, void* workspace, void* stream)
{
  long nmax = 0;
  const int rc = check_lengths("btk_obj_snr", S, n1, n2, 1, stride1, stride2, &nmax);
  if (rc != BTK_OK) return rc;
  if (!x1 || !x2 || !stats || !workspace) return btk_set_error(BTK_ERR_PARAMETER, "btk_obj_snr: null argument");
  if (option < 0 || option > 15) return btk_set_error(BTK_ERR_PARAMETER, "btk_obj_snr: option=%d has unknown bits", option);
  if ((option & 8) && !(option & 6))
    for (int s = 0; s < S; s++)
      if (n1[s] < n2[s])
        return btk_set_error(BTK_ERR_DIMENSION, "btk_obj_snr: option 8 needs n1 >= n2 (pair %d: %ld < %ld)", s, n1[s], n2[s]);
  long Bmax = 0;
  if (seg) {
    if (seg_len < 1) return btk_set_error(BTK_ERR_DIMENSION, "btk_obj_snr: segment length %ld", seg_len);
    for (int s = 0; s < S; s++) Bmax = std::max(Bmax, std::min(n1[s], n2[s]) / seg_len);
    if (seg_stride < Bmax || (Bmax + 3) / 4 > 0x7fffffffL)
      return btk_set_error(BTK_ERR_DIMENSION, "btk_obj_snr: %ld segments in rows of %ld", Bmax, seg_stride);
  }
  hipStream_t st = as_stream(stream);
  SnrArgs a{x1, stride1, x2, stride2, 0, option, (int)((nmax + OBJ_CH - 1) / OBJ_CH), static_cast<double*>(workspace)};
  for (int s0 = 0; s0 < S; s0 += OBJ_PAIRS) {
    const int Sc = std::min(OBJ_PAIRS, S - s0);
    ObjLens lens{};
    long cmax = 0, bmax = 0;
    for (int p = 0; p < Sc; p++) {
      lens.n1[p] = n1[s0 + p]; lens.n2[p] = n2[s0 + p];
      cmax = std::max(cmax, std::max(lens.n1[p], lens.n2[p]));
      if (seg) bmax = std::max(bmax, std::min(lens.n1[p], lens.n2[p]) / seg_len);
    }
    a.s0 = s0;
    const dim3 grid((unsigned)((cmax + OBJ_CH - 1) / OBJ_CH), (unsigned)Sc);
    if (option & 1) hipLaunchKernelGGL(snr_mean_kernel, grid, dim3(NT), 0, st, a, lens);
    if (option & 14) hipLaunchKernelGGL(snr_scale_kernel, grid, dim3(NT), 0, st, a, lens);
    hipLaunchKernelGGL(snr_sum_kernel, grid, dim3(NT), 0, st, a, lens);
    hipLaunchKernelGGL(snr_finish_kernel, dim3((unsigned)Sc), dim3(64), 0, st, a, lens, stats);
    if (seg && bmax > 0)
      hipLaunchKernelGGL(snr_segment_kernel, dim3((unsigned)((bmax + 3) / 4), (unsigned)Sc), dim3(NT), 0, st, a, lens, stats, seg_len,
                         seg, seg_stride);
  }
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

// calcSNR's last line (:180-184), one definition for the engine and the node layer.  log10f is the float64 logarithm rounded to
// float32: a library's log10f may be an ulp off, which the factor 10 turns into two of the result
float btk_obj_snr_db(double sum, double err)
{
  if (!(err > 0.0)) return FLT_MAX;
  const float ratio = (float)(sum / err);
  return 10 * (float)log10((double)ratio);
}

int btk_obj_is_tile_frames(const btk_stft_t* fb)
{
  if (!fb) return -1;
  return fb->M >= 64 ? 4096 / fb->M : (fb->M >= 16 ? 64 : 128);
}

int btk_obj_is_distance(const btk_stft_t* fb, const float* x1, long stride1, const float* x2, long stride2, int S, const long* n1,
                        const long* n2, long bframe, long eframe, double* dist, long long* count, double* eis, long e_stride,
                        void* stream)
{
  if (!fb) return btk_set_error(BTK_ERR_PARAMETER, "btk_obj_is_distance: null plan");
  long nmax = 0;
  const int rc = check_lengths("btk_obj_is_distance", S, n1, n2, 0, stride1, stride2, &nmax);
  if (rc != BTK_OK) return rc;
  if (!x1 || !x2 || !dist || !count || !eis) return btk_set_error(BTK_ERR_PARAMETER, "btk_obj_is_distance: null argument");
  if (bframe < 0) return btk_set_error(BTK_ERR_DIMENSION, "btk_obj_is_distance: bframe=%ld", bframe);
  long Fmax = 0;
  for (int s = 0; s < S; s++) Fmax = std::max(Fmax, btk_stft_num_frames(fb, std::min(n1[s], n2[s])));
  if (e_stride < Fmax) return btk_set_error(BTK_ERR_DIMENSION, "btk_obj_is_distance: %ld frames in rows of %ld", Fmax, e_stride);
  hipStream_t st = as_stream(stream);
  return for_log2n(fb->M, 8, [&](auto L) {
    constexpr int LOG2N = decltype(L)::value;
    const size_t lds = is_lds_bytes<LOG2N>(fb->D);
    if (lds > LDS_MAX) return btk_set_error(BTK_ERR_PARAMETER, "btk_obj_is_distance: tile needs %zu B of LDS", lds);
    auto kern = is_tile_kernel<LOG2N>;
    if (lds > 64 * 1024)
      BTK_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (int s0 = 0; s0 < S; s0 += OBJ_PAIRS) {
      const int Sc = std::min(OBJ_PAIRS, S - s0);
      ObjLens lens{};
      long fmax = 0;
      for (int p = 0; p < Sc; p++) {
        lens.n1[p] = n1[s0 + p]; lens.n2[p] = n2[s0 + p];
        fmax = std::max(fmax, btk_stft_num_frames(fb, std::min(lens.n1[p], lens.n2[p])));
      }
      const long ntiles = (fmax + PrCfg<LOG2N>::TT - 1) / PrCfg<LOG2N>::TT;
      hipLaunchKernelGGL(kern, dim3((unsigned)ntiles, (unsigned)Sc), dim3(NT), lds, st, x1, stride1, x2, stride2, lens, s0, fb->d_win,
                         fb->d_tw, fb->D, eis, e_stride);
      hipLaunchKernelGGL(is_mean_kernel, dim3((unsigned)Sc), dim3(NT), 0, st, eis, e_stride, lens, s0, fb->D, bframe, eframe, dist, count);
    }
    BTK_HIP_CHECK(hipGetLastError());
    return (int)BTK_OK;
  });
}

}  // extern "C"
