// tdoa_kernels.hip -- GCC-PHAT time delay of arrival: the spectral front end of the reference's TDOA scripts
// (HammingFeature / FFTFeature, feature/feature.cc:1177-1258, :29-43) and the per-pair phase transform with its peak search
// (PHATFeature.next / TDOAFeature.next, lib/pytdoa.py:32-54, :87-114), for every frame of a block in one launch each.
//
// Both kernels hold one L-point real transform per workgroup as an L/2-point complex transform in LDS (fft_long.h: twiddles
// from a float64-rounded table read through L2, mu = 2^-24) with the split / pre-twist step of rfft_long.h, so at L = 16384 a
// workgroup declares 64 KB and two of them share a CU.  The correlation never leaves LDS unless the caller asks for it.
#include "btk_internal.h"
#include "rfft_long.h"

namespace {

// ---- stage 1: Hamming window (float64 product rounded to float32; win == NULL: the frame as it is), zero padding to L, forward
// real transform, frame energy.  One workgroup per (stream, channel, frame); rows of pcm are pcm_stride apart.
template <int LOG2NF, int NT>
__global__ __launch_bounds__(NT) void tdoa_spectra_kernel(const float* __restrict__ pcm, long len, long pcm_stride, long T, int D,
                                                          const double* __restrict__ win, const float2* __restrict__ tw,
                                                          float2* __restrict__ X, float* __restrict__ energy)
{
  constexpr int NF = 1 << LOG2NF;
  extern __shared__ float2 buf[];
  __shared__ float red[NT / 64];
  const int tid = threadIdx.x;
  const long f = blockIdx.x;                       // (s C + c) T + t
  const long t = f % T, row = f / T;
  const float* x = pcm + row * pcm_stride;
  const long s0 = t * (long)D;
  for (int n = tid; n < NF; n += NT) {
    const int i0 = 2 * n, i1 = 2 * n + 1;
    float2 z = make_float2(0.f, 0.f);
    if (i0 < D && s0 + i0 < len) z.x = win ? (float)(win[i0] * (double)x[s0 + i0]) : x[s0 + i0];
    if (i1 < D && s0 + i1 < len) z.y = win ? (float)(win[i1] * (double)x[s0 + i1]) : x[s0 + i1];
    buf[n] = z;
  }
  __syncthreads();
  fft_long<LOG2NF, NT, -1>(buf, tw, tid);
  float2* Xr = X + f * (NF + 1);
  float e = 0.f;
  for (int k = tid; k <= NF / 2; k += NT) {
    float2 x0, x1;
    rfft_split<NF>(buf, tw, k, NF - k, x0, x1);
    Xr[k] = x0;
    e += x0.x * x0.x + x0.y * x0.y;
    if (k != NF - k) {
      Xr[NF - k] = x1;
      e += x1.x * x1.x + x1.y * x1.y;
    }
  }
  for (int off = 32; off > 0; off >>= 1) e += __shfl_down(e, off);
  if ((tid & 63) == 0) red[tid >> 6] = e;
  __syncthreads();
  if (tid == 0) {
    float tot = 0.f;
    for (int w = 0; w < NT / 64; w++) tot += red[w];
    energy[f] = 2.f * tot;                         // energy1 of PHATFeature.next (lib/pytdoa.py:47)
  }
}

// a conj(b) / |a conj(b)| without overflow or underflow of the intermediate products: both operands are first scaled by exact
// powers of two.  zero: the float64 product of the reference is exactly zero, which is when a or b is.
__device__ __forceinline__ float2 phat_unit(float2 a, float2 b, bool& zero)
{
  const float ma = fmaxf(fabsf(a.x), fabsf(a.y)), mb = fmaxf(fabsf(b.x), fabsf(b.y));
  if (ma == 0.f || mb == 0.f) { zero = true; return make_float2(0.f, 0.f); }
  int ea, eb;
  frexpf(ma, &ea);
  frexpf(mb, &eb);
  a.x = ldexpf(a.x, -ea); a.y = ldexpf(a.y, -ea);
  b.x = ldexpf(b.x, -eb); b.y = ldexpf(b.y, -eb);
  const float cx = fmaf(a.x, b.x, a.y * b.y), cy = fmaf(a.y, b.x, -a.x * b.y);
  const float n = sqrtf(fmaf(cx, cx, cy * cy));
  return make_float2(cx / n, cy / n);
}

// ---- stage 2: phase transform, inverse real transform and peak search.  One workgroup per (stream, frame, pair), the pair
// index running fastest so that the workgroups in flight share their channels' spectra in L2.
template <int LOG2NF, int NT>
__global__ __launch_bounds__(NT) void tdoa_gcc_kernel(const float2* __restrict__ X, const float* __restrict__ energy,
                                                      const int* __restrict__ pairs, int P, float thr, int C, long T,
                                                      const float2* __restrict__ tw, int* __restrict__ lag,
                                                      float* __restrict__ height, float* __restrict__ gcc)
{
  constexpr int NF = 1 << LOG2NF, L = 2 * NF;
  extern __shared__ float2 buf[];
  __shared__ float redv[NT / 64];
  __shared__ int redi[NT / 64];
  const int tid = threadIdx.x;
  const long f = blockIdx.x;
  const int p = (int)(f % P);
  const long st = f / P, t = st % T, s = st / T;
  const long o = (s * P + p) * T + t;
  const int ca = pairs[2 * p], cb = pairs[2 * p + 1];
  float* g = gcc ? gcc + o * L : nullptr;
  const bool bad = ca < 0 || ca >= C || cb < 0 || cb >= C;
  const long fa = (s * C + (bad ? 0 : ca)) * T + t, fb = (s * C + (bad ? 0 : cb)) * T + t;
  // the gate is an AND (lib/pytdoa.py:49); the condition is uniform over the workgroup
  if (bad || (energy[fa] <= thr && energy[fb] <= thr)) {
    if (tid == 0) { lag[o] = BTK_TDOA_NO_PEAK; height[o] = 0.f; }
    if (g) for (int n = tid; n < L; n += NT) g[n] = 0.f;
    return;
  }
  const float2* Xa = X + fa * (NF + 1);
  const float2* Xb = X + fb * (NF + 1);
  bool zero = false;
  // irfft as an NF-point complex transform
  for (int k = tid; k <= NF / 2; k += NT) {
    const float2 Gk = phat_unit(Xa[k], Xb[k], zero), Gm = phat_unit(Xa[NF - k], Xb[NF - k], zero);
    float2 zk, zm;
    rfft_pretwist<NF>(Gk, Gm, tw, k, zk, zm);
    buf[k] = zk;
    if (k != 0 && k != NF - k) buf[NF - k] = zm;
  }
  // a zero bin makes every lag NaN in the reference (0/0), and no NaN compares greater: no peak
  if (__syncthreads_or(zero)) {
    if (tid == 0) { lag[o] = BTK_TDOA_NO_PEAK; height[o] = 0.f; }
    if (g) for (int n = tid; n < L; n += NT) g[n] = __builtin_nanf("");
    return;
  }
  fft_long<LOG2NF, NT, +1>(buf, tw, tid);
  // z[n] = L (g[2n] + i g[2n+1]); first index of the largest |g| (strict >, scanning upwards)
  constexpr float invL = 1.f / (float)L;
  float bv = 0.f;
  int bi = 0x7fffffff;
  for (int n = tid; n < NF; n += NT) {
    const float2 z = buf[n];
    const float g0 = z.x * invL, g1 = z.y * invL;
    if (g) *reinterpret_cast<float2*>(g + 2 * n) = make_float2(g0, g1);
    if (fabsf(g0) > bv) { bv = fabsf(g0); bi = 2 * n; }
    if (fabsf(g1) > bv) { bv = fabsf(g1); bi = 2 * n + 1; }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_down(bv, off);
    const int oi = __shfl_down(bi, off);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  if ((tid & 63) == 0) { redv[tid >> 6] = bv; redi[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < NT / 64; w++)
      if (redv[w] > bv || (redv[w] == bv && redi[w] < bi)) { bv = redv[w]; bi = redi[w]; }
    const bool peak = bv > 0.f;
    lag[o] = peak ? (bi < NF ? bi : bi - L) : BTK_TDOA_NO_PEAK;
    height[o] = peak ? bv : 0.f;
  }
}

template <int LOG2NF>
int launch_spectra(const float* pcm, long len, long pcm_stride, long rows, long T, int D, const double* win, const float2* tw,
                   void* X, void* energy, hipStream_t st)
{
  constexpr int NF = 1 << LOG2NF, NT = rfft_threads<LOG2NF>;
  constexpr auto kern = tdoa_spectra_kernel<LOG2NF, NT>;
  const size_t lds = sizeof(float2) * NF;
  if (int rc = btk_allow_lds<kern>(lds)) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)(rows * T)), dim3(NT), lds, st, pcm, len, pcm_stride, T, D, win, tw,
                     reinterpret_cast<float2*>(X), reinterpret_cast<float*>(energy));
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

template <int LOG2NF>
int launch_gcc(const void* X, const void* energy, const int* pairs, int P, float thr, int S, int C, long T, const float2* tw,
               void* lag, void* height, void* gcc, hipStream_t st)
{
  constexpr int NF = 1 << LOG2NF, NT = rfft_threads<LOG2NF>;
  constexpr auto kern = tdoa_gcc_kernel<LOG2NF, NT>;
  const size_t lds = sizeof(float2) * NF;
  if (int rc = btk_allow_lds<kern>(lds)) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)((long)S * T * P)), dim3(NT), lds, st, reinterpret_cast<const float2*>(X),
                     reinterpret_cast<const float*>(energy), pairs, P, thr, C, T, tw, reinterpret_cast<int*>(lag),
                     reinterpret_cast<float*>(height), reinterpret_cast<float*>(gcc));
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

}  // namespace

extern "C" {

long btk_tdoa_frames(long len, int D) { return (len > 0 && D > 0) ? (len + D - 1) / D : 0; }

int btk_tdoa_spectra(const float* pcm, long len, long pcm_stride, int S, int C, int D, int L, int window, void* X, void* energy,
                     void* stream)
{
  const int lg = longfft_log2(L);
  if (lg < 0)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_tdoa_spectra: L=%d must be a power of two from %d to %d", L, RFFT_MIN_L, RFFT_MAX_L);
  if (D < 2 || D > L) return btk_set_error(BTK_ERR_DIMENSION, "btk_tdoa_spectra: window length D=%d, need 2 <= D <= L=%d", D, L);
  if (S < 1 || C < 1 || len < 1 || pcm_stride < len)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_tdoa_spectra: S=%d C=%d len=%ld pcm_stride=%ld", S, C, len, pcm_stride);
  if (!pcm || !X || !energy) return btk_set_error(BTK_ERR_PARAMETER, "btk_tdoa_spectra: null argument");
  if (window != BTK_TDOA_WINDOW_NONE && window != BTK_TDOA_WINDOW_HAMMING)
    return btk_set_error(BTK_ERR_PARAMETER, "btk_tdoa_spectra: window %d", window);
  const long T = btk_tdoa_frames(len, D), rows = (long)S * C;
  if (rows * T > 0x7fffffffL) return btk_set_error(BTK_ERR_DIMENSION, "btk_tdoa_spectra: %ld frames in one launch", rows * T);
  const float2* tw;
  const double* win = nullptr;
  int rc = longfft_twiddles(&tw);
  if (!rc && window == BTK_TDOA_WINDOW_HAMMING) rc = longfft_hamming("btk_tdoa_spectra", D, &win);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  return longfft_dispatch(lg, [&](auto n) {
    return launch_spectra<decltype(n)::value>(pcm, len, pcm_stride, rows, T, D, win, tw, X, energy, st);
  });
}

int btk_tdoa_gcc_peaks(const void* X, const void* energy, const int* pairs, int P, float energy_threshold, int S, int C, long T,
                       int L, void* lag, void* height, void* gcc, void* stream)
{
  const int lg = longfft_log2(L);
  if (lg < 0)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_tdoa_gcc_peaks: L=%d must be a power of two from %d to %d", L, RFFT_MIN_L, RFFT_MAX_L);
  if (S < 1 || C < 1 || T < 1 || P < 1)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_tdoa_gcc_peaks: S=%d C=%d T=%ld P=%d", S, C, T, P);
  if (!X || !energy || !pairs || !lag || !height) return btk_set_error(BTK_ERR_PARAMETER, "btk_tdoa_gcc_peaks: null argument");
  if ((long)S * T * P > 0x7fffffffL)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_tdoa_gcc_peaks: %ld correlations in one launch", (long)S * T * P);
  const float2* tw;
  if (int rc = longfft_twiddles(&tw)) return rc;
  hipStream_t st = as_stream(stream);
  return longfft_dispatch(lg, [&](auto n) {
    return launch_gcc<decltype(n)::value>(X, energy, pairs, P, energy_threshold, S, C, T, tw, lag, height, gcc, st);
  });
}

}  // extern "C"
