// tdoa_kernels.hip -- GCC-PHAT time delay of arrival: the spectral front end of the reference's TDOA scripts
// (HammingFeature / FFTFeature, feature/feature.cc:1177-1258, :29-43) and the per-pair phase transform with its peak search
// (PHATFeature.next / TDOAFeature.next, lib/pytdoa.py:32-54, :87-114), for every frame of a block in one launch each.
//
// Both kernels hold one L-point real transform per workgroup as an L/2-point complex transform in LDS (fft_long.h: twiddles
// from a float64-rounded table read through L2, mu = 2^-24) with the usual split / pre-twist step, so at L = 16384 a workgroup
// declares 64 KB and two of them share a CU.  The correlation never leaves LDS unless the caller asks for it.
#include <atomic>
#include <cmath>
#include <map>
#include <mutex>
#include <utility>
#include <vector>
#include "btk_internal.h"
#include "fft_long.h"

namespace {

constexpr int TDOA_MIN_L = 256, TDOA_MAX_L = 16384;

template <int LOG2NF> struct tdoa_cfg {
  static constexpr int NF = 1 << LOG2NF;
  static constexpr int NT = NF / 4 < 64 ? 64 : (NF / 4 > 512 ? 512 : NF / 4);
};

// ---- stage 1: Hamming window (float64 product rounded to float32; win == NULL: the frame as it is), zero padding to L, forward
// real transform, frame energy.  One workgroup per (stream, channel, frame); rows of pcm are pcm_stride apart.
template <int LOG2NF, int NT>
__global__ __launch_bounds__(NT) void tdoa_spectra_kernel(const float* __restrict__ pcm, long len, long pcm_stride, long T, int D,
                                                          const double* __restrict__ win, const float2* __restrict__ tw,
                                                          float2* __restrict__ X, float* __restrict__ energy)
{
  constexpr int NF = 1 << LOG2NF;
  constexpr int TS = BTK_LONGFFT_TWN / (2 * NF);   // table entries per step of exp(-i 2 pi / L)
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
  // split step: Z = E + i O of the even / odd samples, X[k] = E[k] + w^k O[k], X[NF-k] = conj(E[k] - w^k O[k]), w = exp(-i 2 pi / L)
  float2* Xr = X + f * (NF + 1);
  float e = 0.f;
  for (int k = tid; k <= NF / 2; k += NT) {
    const float2 A = buf[k], B = cconjf(buf[(NF - k) & (NF - 1)]);
    const float2 E = make_float2(0.5f * (A.x + B.x), 0.5f * (A.y + B.y));
    const float2 O = make_float2(0.5f * (A.y - B.y), -0.5f * (A.x - B.x));   // (A - B) / (2 i)
    const float2 wO = k == 0 ? O : cmulf(O, tw[k * TS]);
    const float2 x0 = caddf(E, wO), x1 = cconjf(csubf(E, wO));
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
  constexpr int TS = BTK_LONGFFT_TWN / L;
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
  // irfft as an NF-point complex transform: Z[k] = (G[k] + conj G[NF-k]) + i v^k (G[k] - conj G[NF-k]), v = exp(+i 2 pi / L);
  // the imaginary parts of G[0] and G[NF] are ignored, as numpy's irfft ignores them
  for (int k = tid; k <= NF / 2; k += NT) {
    const float2 Gk = phat_unit(Xa[k], Xb[k], zero), Gm = phat_unit(Xa[NF - k], Xb[NF - k], zero);
    if (k == 0) {
      buf[0] = make_float2(Gk.x + Gm.x, Gk.x - Gm.x);
    } else {
      const float2 Sm = make_float2(Gk.x + Gm.x, Gk.y - Gm.y), Df = make_float2(Gk.x - Gm.x, Gk.y + Gm.y);
      const float2 Q = cmulf(Df, cconjf(tw[k * TS]));
      buf[k] = make_float2(Sm.x - Q.y, Sm.y + Q.x);
      if (k != NF - k) buf[NF - k] = make_float2(Sm.x + Q.y, Q.x - Sm.y);
    }
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

// ---- tables: one twiddle table per device, one window per (device, D); built in float64 on the host, uploaded once
std::mutex g_mu;
std::map<int, float2*> g_tw;
std::map<std::pair<int, int>, double*> g_win;

int tdoa_twiddles(const float2** out)
{
  int dev = 0;
  BTK_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_tw.find(dev);
  if (it == g_tw.end()) {
    std::vector<float2> h(BTK_LONGFFT_TWN);
    for (int j = 0; j < BTK_LONGFFT_TWN; j++) {
      const double a = -2.0 * M_PI * (double)j / (double)BTK_LONGFFT_TWN;
      h[j] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    float2* d = nullptr;
    BTK_HIP_CHECK(hipMalloc(&d, sizeof(float2) * BTK_LONGFFT_TWN));
    BTK_HIP_CHECK(hipMemcpy(d, h.data(), sizeof(float2) * BTK_LONGFFT_TWN, hipMemcpyHostToDevice));
    it = g_tw.emplace(dev, d).first;
  }
  *out = it->second;
  return BTK_OK;
}

// Windows live as long as the process: a pointer handed out may belong to a launch another host thread has not made yet, so
// nothing is ever freed.  Bounded by bytes instead (64 lengths of the largest window); a process that asks for more distinct
// lengths than fit gets BTK_ERR_ALLOCATION.  The first use of a length (and of a device) allocates and copies, so it cannot be
// part of a stream capture; every later launch with that length is capturable.
constexpr size_t TDOA_WINDOW_BYTES_MAX = 64 * sizeof(double) * TDOA_MAX_L;
size_t g_win_bytes = 0;

int tdoa_window(int D, const double** out)
{
  int dev = 0;
  BTK_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_win.find({dev, D});
  if (it == g_win.end()) {
    if (g_win_bytes + sizeof(double) * D > TDOA_WINDOW_BYTES_MAX)
      return btk_set_error(BTK_ERR_ALLOCATION, "btk_tdoa_spectra: more than %zu bytes of distinct window lengths in one process",
                           TDOA_WINDOW_BYTES_MAX);
    std::vector<double> h(D);                      // HammingFeature's window, in its own order of operations (feature.cc:1181-1183)
    const double temp = 2. * M_PI / (double)(D - 1);
    for (int i = 0; i < D; i++) h[i] = 0.54 - 0.46 * std::cos(temp * i);
    double* d = nullptr;
    BTK_HIP_CHECK(hipMalloc(&d, sizeof(double) * D));
    BTK_HIP_CHECK(hipMemcpy(d, h.data(), sizeof(double) * D, hipMemcpyHostToDevice));
    g_win_bytes += sizeof(double) * D;
    it = g_win.emplace(std::make_pair(dev, D), d).first;
  }
  *out = it->second;
  return BTK_OK;
}

// a workgroup's LDS exceeds the default limit at the largest transform: raised once per kernel instantiation and device
// (TAG tells the instantiations apart: kernels of one signature share a function-pointer type)
template <int TAG, class K> int tdoa_allow_lds(K kern, size_t lds)
{
  static std::atomic<unsigned long long> done{0};
  int dev = 0;
  BTK_HIP_CHECK(hipGetDevice(&dev));
  const unsigned long long bit = 1ull << (dev & 63);
  if (done.load(std::memory_order_acquire) & bit) return BTK_OK;
  BTK_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  done.fetch_or(bit, std::memory_order_release);
  return BTK_OK;
}

int log2_of_L(int L)
{
  if (L < TDOA_MIN_L || L > TDOA_MAX_L || (L & (L - 1))) return -1;
  int n = 0;
  while ((1 << n) < L) n++;
  return n;
}

template <int LOG2NF>
int launch_spectra(const float* pcm, long len, long pcm_stride, long rows, long T, int D, const double* win, const float2* tw,
                   void* X, void* energy, hipStream_t st)
{
  constexpr int NF = 1 << LOG2NF, NT = tdoa_cfg<LOG2NF>::NT;
  auto kern = tdoa_spectra_kernel<LOG2NF, NT>;
  const size_t lds = sizeof(float2) * NF;
  if (int rc = tdoa_allow_lds<2 * LOG2NF>(kern, lds)) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)(rows * T)), dim3(NT), lds, st, pcm, len, pcm_stride, T, D, win, tw,
                     reinterpret_cast<float2*>(X), reinterpret_cast<float*>(energy));
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

template <int LOG2NF>
int launch_gcc(const void* X, const void* energy, const int* pairs, int P, float thr, int S, int C, long T, const float2* tw,
               void* lag, void* height, void* gcc, hipStream_t st)
{
  constexpr int NF = 1 << LOG2NF, NT = tdoa_cfg<LOG2NF>::NT;
  auto kern = tdoa_gcc_kernel<LOG2NF, NT>;
  const size_t lds = sizeof(float2) * NF;
  if (int rc = tdoa_allow_lds<2 * LOG2NF + 1>(kern, lds)) return rc;
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
  const int lg = log2_of_L(L);
  if (lg < 0)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_tdoa_spectra: L=%d must be a power of two from %d to %d", L, TDOA_MIN_L, TDOA_MAX_L);
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
  int rc = tdoa_twiddles(&tw);
  if (!rc && window == BTK_TDOA_WINDOW_HAMMING) rc = tdoa_window(D, &win);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  switch (lg - 1) {
    case 7: return launch_spectra<7>(pcm, len, pcm_stride, rows, T, D, win, tw, X, energy, st);
    case 8: return launch_spectra<8>(pcm, len, pcm_stride, rows, T, D, win, tw, X, energy, st);
    case 9: return launch_spectra<9>(pcm, len, pcm_stride, rows, T, D, win, tw, X, energy, st);
    case 10: return launch_spectra<10>(pcm, len, pcm_stride, rows, T, D, win, tw, X, energy, st);
    case 11: return launch_spectra<11>(pcm, len, pcm_stride, rows, T, D, win, tw, X, energy, st);
    case 12: return launch_spectra<12>(pcm, len, pcm_stride, rows, T, D, win, tw, X, energy, st);
    default: return launch_spectra<13>(pcm, len, pcm_stride, rows, T, D, win, tw, X, energy, st);
  }
}

int btk_tdoa_gcc_peaks(const void* X, const void* energy, const int* pairs, int P, float energy_threshold, int S, int C, long T,
                       int L, void* lag, void* height, void* gcc, void* stream)
{
  const int lg = log2_of_L(L);
  if (lg < 0)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_tdoa_gcc_peaks: L=%d must be a power of two from %d to %d", L, TDOA_MIN_L, TDOA_MAX_L);
  if (S < 1 || C < 1 || T < 1 || P < 1)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_tdoa_gcc_peaks: S=%d C=%d T=%ld P=%d", S, C, T, P);
  if (!X || !energy || !pairs || !lag || !height) return btk_set_error(BTK_ERR_PARAMETER, "btk_tdoa_gcc_peaks: null argument");
  if ((long)S * T * P > 0x7fffffffL)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_tdoa_gcc_peaks: %ld correlations in one launch", (long)S * T * P);
  const float2* tw;
  int rc = tdoa_twiddles(&tw);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  switch (lg - 1) {
    case 7: return launch_gcc<7>(X, energy, pairs, P, energy_threshold, S, C, T, tw, lag, height, gcc, st);
    case 8: return launch_gcc<8>(X, energy, pairs, P, energy_threshold, S, C, T, tw, lag, height, gcc, st);
    case 9: return launch_gcc<9>(X, energy, pairs, P, energy_threshold, S, C, T, tw, lag, height, gcc, st);
    case 10: return launch_gcc<10>(X, energy, pairs, P, energy_threshold, S, C, T, tw, lag, height, gcc, st);
    case 11: return launch_gcc<11>(X, energy, pairs, P, energy_threshold, S, C, T, tw, lag, height, gcc, st);
    case 12: return launch_gcc<12>(X, energy, pairs, P, energy_threshold, S, C, T, tw, lag, height, gcc, st);
    default: return launch_gcc<13>(X, energy, pairs, P, energy_threshold, S, C, T, tw, lag, height, gcc, st);
  }
}

}  // extern "C"
