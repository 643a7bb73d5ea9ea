// fe_kernels.hip -- the recogniser's front end of unit_test/log_power_extractor.py and unit_test/mfcc_extractor.py:
// PreemphasisFeature (feature/feature.cc:1128-1144), HammingFeature / FFTFeature (:1177-1258), SpectralPowerFeature (:1291-1314),
// VTLNFeature (:1672-1792), MelFeature (:1892-2122, :2229-2242), LogFeature (:2326-2362) and CepstralFeature (:2370-2415,
// matrix/gslmatrix.cc:107-131), for every frame of a block in one launch.
//
// fe_pcm_kernel: G frames per workgroup, each on NT threads.  A frame is loaded (overlapping frames read the same samples from
// L2), pre-emphasised, windowed and transformed in LDS as tdoa_spectra_kernel does it (fft_long.h, rfft_long.h's split step:
// with the Hamming window, no pre-emphasis and shift = D the spectra have that kernel's bits).  The power vector stays in
// LDS; the later stages ping-pong between it and the transform's buffer, which is free by then, and only the requested stages
// are written to HBM.  The tables (a few KB at ASR sizes: the mel rows are 2-16 coefficients long and stored by row) are staged
// into LDS while they fit beside the frames, and read through L2 otherwise.
// fe_stage_kernel: the same device functions for vectors that enter at SPECTRUM or later.
// VTLN, MEL and CEP accumulate each output in float64 in the order of their row and round once, so a stage gives the same bits
// whichever kernel runs it and however the frames are grouped.
#include <cmath>
#include <vector>
#include "btk_internal.h"
#include "rfft_long.h"

namespace {

constexpr size_t FE_LDS_TABLE_LIMIT = 64 * 1024;   // tables go to LDS while the workgroup stays within this
constexpr size_t FE_LDS_MAX = 160 * 1024;

template <int LOG2NF> struct fe_cfg {
  static constexpr int NT = rfft_threads<LOG2NF>;                                // threads per frame
  static constexpr int G = NT >= 256 ? 1 : 256 / NT;                             // frames per workgroup: 256 threads at least
};
constexpr int FE_STAGE_NT = 64, FE_STAGE_G = 4;

struct fe_dev {
  long T, nframes, len, pcm_stride;
  int D, shift, preemph, in_stage, in_dim, powN, last;
  double mu;
  const float* prior0;
  const double* win;
  const float2* tw;
  int vtlnN, melN, cepN, log_floor;
  const int* vtln_rows;
  const double* vtln_w;
  const int* mel_rows;
  const float* mel_w;
  const float* dct;
  double log_m, log_a;
  float2* oX;
  float *oP, *oV, *oM, *oL, *oC;
  int tab_lds, n_vw, n_mw, n_dct;   // tables staged in LDS, and their coefficient counts
};

__device__ __forceinline__ float fe_abs2(float2 z) { return __fmaf_rn(z.x, z.x, __fmul_rn(z.y, z.y)); }

// the tables as the stages read them: in LDS behind the frames' buffers (tab_lds) or where the caller left them
struct fe_tabs {
  const int *vrows, *mrows;
  const double* vw;
  const float *mw, *dct;
};

__device__ __forceinline__ fe_tabs fe_stage_tables(const fe_dev& p, unsigned char* lds, int tid, int nthreads)
{
  fe_tabs t{p.vtln_rows, p.mel_rows, p.vtln_w, p.mel_w, p.dct};
  if (!p.tab_lds) return t;
  double* vw = reinterpret_cast<double*>(lds);
  float* mw = reinterpret_cast<float*>(vw + p.n_vw);
  float* dct = mw + p.n_mw;
  int* vrows = reinterpret_cast<int*>(dct + p.n_dct);
  int* mrows = vrows + (p.vtln_rows ? 3 * p.vtlnN : 0);
  if (p.vtln_rows) {
    for (int i = tid; i < p.n_vw; i += nthreads) vw[i] = p.vtln_w[i];
    for (int i = tid; i < 3 * p.vtlnN; i += nthreads) vrows[i] = p.vtln_rows[i];
    t.vw = vw; t.vrows = vrows;
  }
  if (p.mel_rows) {
    for (int i = tid; i < p.n_mw; i += nthreads) mw[i] = p.mel_w[i];
    for (int i = tid; i < 3 * p.melN; i += nthreads) mrows[i] = p.mel_rows[i];
    t.mw = mw; t.mrows = mrows;
  }
  if (p.dct) {
    for (int i = tid; i < p.n_dct; i += nthreads) dct[i] = p.dct[i];
    t.dct = dct;
  }
  return t;                                        // visible after the caller's next barrier
}

// element i of a vector that may be the lower half of a conjugate-symmetric power spectrum of length L (mirror: i > L/2 -> L - i)
__device__ __forceinline__ float fe_ld(const float* v, int i, int L, bool mir) { return (mir && i > L / 2) ? v[L - i] : v[i]; }

template <class W>
__device__ __forceinline__ void fe_apply_rows(const int* rows, const W* w, int nw, int N, const float* in, int n, int L, bool mir,
                                              float* out, float* gout, int lt, int nt)
{
  for (int j = lt; j < N; j += nt) {
    const int off = rows[3 * j], cnt = rows[3 * j + 1], st = rows[3 * j + 2];
    double acc = 0.0;
    for (int i = 0; i < cnt; i++) {
      const int idx = off + i;
      // (a coefficient outside the input vector or outside the packed table is ignored: a malformed row reads nothing else)
      if (idx >= 0 && idx < n && st + i >= 0 && st + i < nw) acc += (double)w[st + i] * (double)fe_ld(in, idx, L, mir);
    }
    const float r = (float)acc;
    out[j] = r;
    if (gout) gout[j] = r;
  }
}

// The stages after POWER (or after p.in_stage, whichever is later) on one frame's vector.  a holds the n input values (mir: the
// lower half of a mirrored spectrum of length L), b is the other buffer; every thread of the workgroup runs this with its
// frame's buffers (the barriers are workgroup-wide), f < 0 marks a frame that does not exist (nothing is stored for it).
__device__ __forceinline__ void fe_tail(const fe_dev& p, const fe_tabs& tb, float* a, float* b, int n, int L, bool mir, long f,
                                        int lt, int nt)
{
  float *cur = a, *oth = b;
  const bool st = f >= 0;
  if (p.last < BTK_FE_VTLN) return;
  if (p.in_stage < BTK_FE_VTLN && p.vtln_rows) {
    fe_apply_rows(tb.vrows, tb.vw, p.n_vw, p.vtlnN, cur, n, L, mir, oth, st && p.oV ? p.oV + f * p.vtlnN : nullptr, lt, nt);
    __syncthreads();
    float* s = cur; cur = oth; oth = s;
    n = p.vtlnN; mir = false;
  }
  if (p.last < BTK_FE_MEL) return;
  if (p.in_stage < BTK_FE_MEL && p.mel_rows) {
    fe_apply_rows(tb.mrows, tb.mw, p.n_mw, p.melN, cur, n, L, mir, oth, st && p.oM ? p.oM + f * p.melN : nullptr, lt, nt);
    __syncthreads();
    float* s = cur; cur = oth; oth = s;
    n = p.melN; mir = false;
  }
  if (p.last < BTK_FE_LOG) return;
  if (p.in_stage < BTK_FE_LOG) {
    // from a to b (b holds a whole spectrum where a holds half of one), in place in b
    float* dst = cur == a ? b : cur;
    float* gl = st && p.oL ? p.oL + f * n : nullptr;
    for (int i = lt; i < n; i += nt) {
      double val = (double)fe_ld(cur, i, L, mir);
      if (p.log_floor) {
        if (val < 1.0e-5) val = 1.0e-5;
      } else {
        val += p.log_a;
        if (val <= 0.0) val = 1.0;
      }
      const float r = (float)(p.log_m * log10(val));
      dst[i] = r;
      if (gl) gl[i] = r;
    }
    __syncthreads();
    if (dst != cur) { oth = cur; cur = dst; }
    mir = false;
  }
  if (p.last < BTK_FE_CEP) return;
  float* gc = st && p.oC ? p.oC + f * p.cepN : nullptr;
  for (int j = lt; j < p.cepN; j += nt) {
    const float* row = tb.dct + (long)j * n;
    double acc = 0.0;
    for (int i = 0; i < n; i++) acc += (double)row[i] * (double)cur[i];
    const float r = (float)acc;
    oth[j] = r;
    if (gc) gc[j] = r;
  }
}

template <int LOG2NF, int NT, int G>
__global__ __launch_bounds__(NT* G) void fe_pcm_kernel(const float* __restrict__ pcm, fe_dev p)
{
  constexpr int NF = 1 << LOG2NF, L = 2 * NF;
  constexpr int PWS = (NF + 2) & ~1;               // floats per frame of the power vector (even: the tables behind are 8-byte aligned)
  extern __shared__ float2 smem[];
  const int tid = threadIdx.x, g = tid / NT, lt = tid % NT;
  float2* buf = smem + g * NF;
  float* pw = reinterpret_cast<float*>(smem + G * NF) + g * PWS;
  const fe_tabs tb = fe_stage_tables(p, reinterpret_cast<unsigned char*>(reinterpret_cast<float*>(smem + G * NF) + G * PWS), tid, NT * G);
  const long f = blockIdx.x * (long)G + g;
  const bool valid = f < p.nframes;
  const long t = valid ? f % p.T : 0, row = valid ? f / p.T : 0;
  const float* x = pcm + row * p.pcm_stride;
  const long s0 = t * (long)p.shift;
  const int D = p.D;
  const double* win = p.win;
  auto raw = [&](long s) -> float { return s < p.len ? x[s] : 0.f; };
  auto sample = [&](int i) -> float {
    if (!p.preemph) {
      if (s0 + i >= p.len) return 0.f;
      return win ? (float)(win[i] * (double)x[s0 + i]) : x[s0 + i];
    }
    // PreemphasisFeature::next: block[i] - mu prior in float64, stored as float; prior_ is the sample handed out before
    const float prior = i > 0 ? raw(s0 + i - 1) : (t > 0 ? raw(s0 - p.shift + D - 1) : (p.prior0 ? p.prior0[row] : 0.f));
    const float v = (float)__dsub_rn((double)raw(s0 + i), __dmul_rn(p.mu, (double)prior));
    return win ? (float)(win[i] * (double)v) : v;
  };
  for (int n = lt; n < NF; n += NT) {
    const int i0 = 2 * n, i1 = 2 * n + 1;
    float2 z = make_float2(0.f, 0.f);
    if (valid) {
      if (i0 < D) z.x = sample(i0);
      if (i1 < D) z.y = sample(i1);
    }
    buf[n] = z;
  }
  __syncthreads();
  fft_long<LOG2NF, NT, -1>(buf, p.tw, lt);
  float2* Xr = valid && p.oX ? p.oX + f * (NF + 1) : nullptr;
  for (int k = lt; k <= NF / 2; k += NT) {
    float2 x0, x1;
    rfft_split<NF>(buf, p.tw, k, NF - k, x0, x1);
    if (Xr) Xr[k] = x0;
    pw[k] = fe_abs2(x0);
    if (k != NF - k) {
      if (Xr) Xr[NF - k] = x1;
      pw[NF - k] = fe_abs2(x1);
    }
  }
  if (p.last < BTK_FE_POWER) return;
  __syncthreads();
  if (valid && p.oP) {
    float* P = p.oP + f * p.powN;
    for (int i = lt; i < p.powN; i += NT) P[i] = fe_ld(pw, i, L, true);
  }
  fe_tail(p, tb, pw, reinterpret_cast<float*>(buf), p.powN, L, true, valid ? f : -1, lt, NT);
}

template <int G>
__global__ __launch_bounds__(FE_STAGE_NT* G) void fe_stage_kernel(const void* __restrict__ in, fe_dev p, int L, int cap)
{
  constexpr int NT = FE_STAGE_NT;
  extern __shared__ float2 smem[];
  const int tid = threadIdx.x, g = tid / NT, lt = tid % NT;
  float* a = reinterpret_cast<float*>(smem) + (long)g * 2 * cap;   // cap is even
  float* b = a + cap;
  const fe_tabs tb = fe_stage_tables(p, reinterpret_cast<unsigned char*>(reinterpret_cast<float*>(smem) + (long)G * 2 * cap), tid, NT * G);
  const long f = blockIdx.x * (long)G + g;
  const bool valid = f < p.nframes;
  int n;
  if (p.in_stage == BTK_FE_SPECTRUM) {
    n = p.powN;
    const float2* X = reinterpret_cast<const float2*>(in) + (valid ? f : 0) * (L / 2 + 1);
    float* P = valid && p.oP ? p.oP + f * n : nullptr;
    for (int i = lt; i < n; i += NT) {
      const float v = fe_abs2(X[i > L / 2 ? L - i : i]);
      a[i] = v;
      if (P) P[i] = v;
    }
  } else {
    n = p.in_dim;
    const float* v = reinterpret_cast<const float*>(in) + (valid ? f : 0) * n;
    for (int i = lt; i < n; i += NT) a[i] = v[i];
  }
  __syncthreads();
  fe_tail(p, tb, a, b, n, 0, false, valid ? f : -1, lt, NT);
}

size_t fe_table_bytes(const fe_dev& p)
{
  return sizeof(double) * p.n_vw + sizeof(float) * ((size_t)p.n_mw + p.n_dct) +
         sizeof(int) * 3 * ((size_t)(p.vtln_rows ? p.vtlnN : 0) + (p.mel_rows ? p.melN : 0));
}

template <int LOG2NF> int launch_pcm(const float* pcm, fe_dev p, hipStream_t st)
{
  constexpr int NF = 1 << LOG2NF, NT = fe_cfg<LOG2NF>::NT, G = fe_cfg<LOG2NF>::G, PWS = (NF + 2) & ~1;
  constexpr auto kern = fe_pcm_kernel<LOG2NF, NT, G>;
  size_t lds = sizeof(float2) * G * NF + sizeof(float) * G * PWS;
  const size_t tb = fe_table_bytes(p);
  p.tab_lds = lds + tb <= FE_LDS_TABLE_LIMIT;
  if (p.tab_lds) lds += tb;
  if (int rc = btk_allow_lds<kern>(FE_LDS_MAX)) return rc;
  const long blocks = (p.nframes + G - 1) / G;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(NT * G), lds, st, pcm, p);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

template <int G> int launch_stage_g(const void* in, fe_dev p, int L, int cap, hipStream_t st)
{
  size_t lds = sizeof(float) * 2 * (size_t)cap * G;
  const size_t tb = fe_table_bytes(p);
  p.tab_lds = lds + tb <= FE_LDS_TABLE_LIMIT;
  if (p.tab_lds) lds += tb;
  if (int rc = btk_allow_lds<fe_stage_kernel<G>>(FE_LDS_MAX)) return rc;
  const long blocks = (p.nframes + G - 1) / G;
  hipLaunchKernelGGL(fe_stage_kernel<G>, dim3((unsigned)blocks), dim3(FE_STAGE_NT * G), lds, st, in, p, L, cap);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

// four frames per workgroup while their vectors fit (two LDS vectors per frame), one frame for the long ones (up to 20480
// values: a whole 16384-point power spectrum)
int launch_stage(const void* in, fe_dev p, int L, int maxdim, hipStream_t st)
{
  const int cap = (maxdim + 1) & ~1;
  if (sizeof(float) * 2 * (size_t)cap * FE_STAGE_G <= FE_LDS_MAX) return launch_stage_g<FE_STAGE_G>(in, p, L, cap, st);
  if (sizeof(float) * 2 * (size_t)cap > FE_LDS_MAX)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_fe_process: stage length %d does not fit a workgroup's LDS", maxdim);
  return launch_stage_g<1>(in, p, L, cap, st);
}

// mel_ / hertz_ of MelFeature::SparseMatrix_ (feature/feature.cc:1892-1902)
float fe_mel(float hz) { return hz >= 0 ? (float)(2595.0 * std::log10(1.0 + (double)hz / 700.0)) : 0.0f; }
float fe_hertz(float m)
{
  const double d = m / 2595.0;
  return (float)(700.0 * (std::pow(10.0, d) - 1.0));
}

}  // namespace

extern "C" {

long btk_fe_frames(long len, int D, int shift, int pad_zeros)
{
  if (len <= 0 || D <= 0 || shift <= 0) return 0;
  if (pad_zeros) return (len + shift - 1) / shift;
  return D < len ? (len - D + shift - 1) / shift : 0;
}

int btk_fe_process(const btk_fe_params* q, const void* in, void* stream)
{
  if (!q || !in) return btk_set_error(BTK_ERR_PARAMETER, "btk_fe_process: null argument");
  if (q->in_stage < BTK_FE_PCM || q->in_stage >= BTK_FE_CEP)
    return btk_set_error(BTK_ERR_PARAMETER, "btk_fe_process: input stage %d", q->in_stage);
  int last = -1;
  for (int s = q->in_stage + 1; s <= BTK_FE_CEP; s++)
    if (q->out[s]) last = s;
  if (last < 0) return btk_set_error(BTK_ERR_PARAMETER, "btk_fe_process: no stage after %d is requested", q->in_stage);
  if (q->S < 1 || q->C < 1 || q->T < 1)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_fe_process: S=%d C=%d T=%ld", q->S, q->C, q->T);
  const long nframes = (long)q->S * q->C * q->T;
  if (nframes > 0x7fffffffL) return btk_set_error(BTK_ERR_DIMENSION, "btk_fe_process: %ld frames in one launch", nframes);
  fe_dev p{};
  p.T = q->T; p.nframes = nframes; p.in_stage = q->in_stage; p.last = last; p.in_dim = q->in_dim;
  int lg = 0, L = 0;
  int n;                                           // length of the vector the next stage reads
  if (q->in_stage <= BTK_FE_SPECTRUM) {
    L = q->L;
    lg = longfft_log2(L);
    if (lg < 0)
      return btk_set_error(BTK_ERR_DIMENSION, "btk_fe_process: L=%d must be a power of two from %d to %d", L, RFFT_MIN_L, RFFT_MAX_L);
    if (last >= BTK_FE_POWER && q->powN != L / 2 + 1 && q->powN != L)
      return btk_set_error(BTK_ERR_DIMENSION, "btk_fe_process: number of power coefficients %d does not match FFT length %d", q->powN, L);
    p.powN = q->powN;
    n = q->powN;
  } else {
    if (q->in_dim < 1) return btk_set_error(BTK_ERR_DIMENSION, "btk_fe_process: in_dim=%d", q->in_dim);
    n = q->in_dim;
  }
  if (q->in_stage == BTK_FE_PCM) {
    if (q->D < 2 || q->D > L) return btk_set_error(BTK_ERR_DIMENSION, "btk_fe_process: window length D=%d, need 2 <= D <= L=%d", q->D, L);
    if (q->shift < 1 || q->shift > q->D)
      return btk_set_error(BTK_ERR_DIMENSION, "btk_fe_process: shift=%d, need 1 <= shift <= D=%d", q->shift, q->D);
    if (q->len < 1 || q->pcm_stride < q->len)
      return btk_set_error(BTK_ERR_DIMENSION, "btk_fe_process: len=%ld pcm_stride=%ld", q->len, q->pcm_stride);
    if (q->window != BTK_TDOA_WINDOW_NONE && q->window != BTK_TDOA_WINDOW_HAMMING)
      return btk_set_error(BTK_ERR_PARAMETER, "btk_fe_process: window %d", q->window);
    p.len = q->len; p.pcm_stride = q->pcm_stride; p.D = q->D; p.shift = q->shift; p.preemph = q->preemph != 0; p.mu = q->mu;
    p.prior0 = q->prior0;
  }
  // the stages that run, their lengths and the largest of them
  const int half = L / 2 + 1;
  int maxdim = n;
  if (q->in_stage < BTK_FE_VTLN && last >= BTK_FE_VTLN && q->vtln_rows) {
    if (!q->vtln_w) return btk_set_error(BTK_ERR_PARAMETER, "btk_fe_process: VTLN rows without weights");
    if (q->vtlnN < 1 || (q->in_stage == BTK_FE_PCM && q->vtlnN > n))
      return btk_set_error(BTK_ERR_DIMENSION, "btk_fe_process: vtlnN=%d over %d power coefficients", q->vtlnN, n);
    p.vtln_rows = q->vtln_rows; p.vtln_w = q->vtln_w; p.vtlnN = n = q->vtlnN;
    if (n > maxdim) maxdim = n;
  }
  if (q->in_stage < BTK_FE_MEL && last >= BTK_FE_MEL && q->mel_rows) {
    if (!q->mel_w) return btk_set_error(BTK_ERR_PARAMETER, "btk_fe_process: mel rows without coefficients");
    if (q->melN < 1 || (q->in_stage == BTK_FE_PCM && q->melN > half))
      return btk_set_error(BTK_ERR_DIMENSION, "btk_fe_process: melN=%d", q->melN);
    p.mel_rows = q->mel_rows; p.mel_w = q->mel_w; p.melN = n = q->melN;
    if (n > maxdim) maxdim = n;
  }
  const int logdim = n;
  if (last >= BTK_FE_CEP) {
    if (!q->dct) return btk_set_error(BTK_ERR_PARAMETER, "btk_fe_process: cepstra without a cosine table");
    if (q->cepN < 1 || (q->in_stage == BTK_FE_PCM && q->cepN > half))
      return btk_set_error(BTK_ERR_DIMENSION, "btk_fe_process: cepN=%d", q->cepN);
    p.dct = q->dct; p.cepN = q->cepN;
    if ((long)q->cepN * logdim > 0x7fffffffL) return btk_set_error(BTK_ERR_DIMENSION, "btk_fe_process: cosine table %d x %d", q->cepN, logdim);
    p.n_dct = q->cepN * logdim;
    if (q->cepN > maxdim) maxdim = q->cepN;
  }
  p.log_m = q->log_m; p.log_a = q->log_a; p.log_floor = q->log_floor != 0;
  p.oX = reinterpret_cast<float2*>(q->out[BTK_FE_SPECTRUM]);
  p.oP = reinterpret_cast<float*>(q->out[BTK_FE_POWER]);
  p.oV = reinterpret_cast<float*>(q->out[BTK_FE_VTLN]);
  p.oM = reinterpret_cast<float*>(q->out[BTK_FE_MEL]);
  p.oL = reinterpret_cast<float*>(q->out[BTK_FE_LOG]);
  p.oC = reinterpret_cast<float*>(q->out[BTK_FE_CEP]);
  if (q->in_stage >= BTK_FE_SPECTRUM) p.oX = nullptr;
  if (q->in_stage >= BTK_FE_POWER) p.oP = nullptr;
  if (q->in_stage >= BTK_FE_VTLN) p.oV = nullptr;
  if (q->in_stage >= BTK_FE_MEL) p.oM = nullptr;
  if (q->in_stage >= BTK_FE_LOG) p.oL = nullptr;
  hipStream_t st = as_stream(stream);
  if (p.vtln_rows) {
    if (q->vtln_nw < 0) return btk_set_error(BTK_ERR_DIMENSION, "btk_fe_process: vtln_nw=%d", q->vtln_nw);
    p.n_vw = q->vtln_nw;
  }
  if (p.mel_rows) {
    if (q->mel_nw < 0) return btk_set_error(BTK_ERR_DIMENSION, "btk_fe_process: mel_nw=%d", q->mel_nw);
    p.n_mw = q->mel_nw;
  }
  if (q->in_stage == BTK_FE_PCM) {
    int rc = longfft_twiddles(&p.tw);
    if (!rc && q->window == BTK_TDOA_WINDOW_HAMMING) rc = longfft_hamming("btk_fe_process", q->D, &p.win);
    if (rc) return rc;
    const float* pcm = reinterpret_cast<const float*>(in);
    return longfft_dispatch(lg, [&](auto n) { return launch_pcm<decltype(n)::value>(pcm, p, st); });
  }
  return launch_stage(in, p, L, maxdim, st);
}

int btk_fe_mel_table(int powN, float rate, float low, float up, int filterN, int version, int* offset, int* count, float* coef,
                     int coef_cap, int* ncoef)
{
#pragma clang fp contract(off)
  if (!offset || !count || !coef || !ncoef) return btk_set_error(BTK_ERR_PARAMETER, "btk_fe_mel_table: null argument");
  if (version != 1 && version != 2) return btk_set_error(BTK_ERR_PARAMETER, "btk_fe_mel_table: unknown version %d", version);
  if (powN < 2 || filterN < 1) return btk_set_error(BTK_ERR_DIMENSION, "btk_fe_mel_table: powN=%d filterN=%d", powN, filterN);
  if (up <= 0) up = rate / 2.0;                    // MelFeature::MelFeature (:2206)
  const float df = rate / (4.0 * (powN / 2));      // spacing between FFT points in Hz
  const float mlow = fe_mel(low), mup = fe_mel(up);
  const float dm = (mup - mlow) / (filterN + 1);
  if (low < 0.0 || 2.0 * up > rate || low > up)
    return btk_set_error(BTK_ERR_PARAMETER, "btk_fe_mel_table: low=%g up=%g rate=%g", (double)low, (double)up, (double)rate);
  int total = 0;
  for (unsigned x = 0; x < (unsigned)filterN; x++) {
    const float left = fe_hertz(x * dm + mlow);
    const float center = fe_hertz((x + 1.0) * dm + mlow);
    const float right = fe_hertz((x + 2.0) * dm + mlow);
    const float height = 2.0 / (right - left);
    const float slope1 = height / (center - left);
    const float slope2 = height / (center - right);
    const int start = (int)std::ceil(left / df);
    const int end = (int)std::floor(right / df);
    const int cn = end - start + 1;
    if (start < 0 || cn < 0 || start + cn > powN)
      return btk_set_error(BTK_ERR_DIMENSION, "btk_fe_mel_table: filter %u covers bins %d .. %d of %d", x, start, end, powN);
    if (total + cn > coef_cap) return btk_set_error(BTK_ERR_DIMENSION, "btk_fe_mel_table: more than %d coefficients", coef_cap);
    offset[x] = start;
    count[x] = cn;
    float freq = start * df;
    for (int i = 0; i < cn; i++) {
      if (version == 1) freq += df;
      coef[total + i] = freq <= center ? slope1 * (freq - left) : slope2 * (freq - right);
      if (version == 2) freq += df;
    }
    total += cn;
  }
  *ncoef = total;
  return BTK_OK;
}

int btk_fe_vtln_table(int N, int inN, double ratio, double edge, int version, int* offset, int* count, double* w, int w_cap, int* nw)
{
#pragma clang fp contract(off)
  if (!offset || !count || !w || !nw) return btk_set_error(BTK_ERR_PARAMETER, "btk_fe_vtln_table: null argument");
  if (version != 1 && version != 2) return btk_set_error(BTK_ERR_PARAMETER, "btk_fe_vtln_table: unknown version number (%d)", version);
  if (N < 1 || inN < 1 || (version == 2 && inN != N))
    return btk_set_error(BTK_ERR_DIMENSION, "btk_fe_vtln_table: N=%d inN=%d version=%d", N, inN, version);
  if ((long)N * inN > (1L << 28)) return btk_set_error(BTK_ERR_DIMENSION, "btk_fe_vtln_table: %d x %d", N, inN);
  std::vector<double> W((size_t)N * inN, 0.0);
  if (version == 1) {
    const double yedge = (edge < ratio) ? (edge / ratio) : 1.0;
    const double b = (yedge < 1.0) ? (1.0 - edge) / (1.0 - yedge) : 0;
    for (int c = 0; c < N; c++) {
      double* Wr = W.data() + (size_t)c * inN;
      const double Y0 = double(c) / double(N), Y1 = double(c + 1) / double(N);
      const double X0 = ((Y0 < yedge) ? (ratio * Y0) : (b * Y0 + 1.0 - b)) * N;
      const double X1 = ((Y1 < yedge) ? (ratio * Y1) : (b * Y1 + 1.0 - b)) * N;
      int l1 = int(X1);
      const double alpha1 = X1 - l1;
      int l0 = int(X0);
      const double alpha0 = int(X0) + 1 - X0;
      if (l0 >= inN) l0 = inN - 1;
      if (l1 > inN) l1 = inN;
      if (l0 < 0 || l1 < 0) return btk_set_error(BTK_ERR_PARAMETER, "btk_fe_vtln_table: ratio=%g edge=%g warp below bin 0", ratio, edge);
      if (l0 == l1) {
        Wr[l0] += X1 - X0;
      } else {
        Wr[l0] += alpha0;
        for (int i = l0 + 1; i < l1; i++) Wr[i] += 1.0;
        if (l1 < inN) Wr[l1] += alpha1;
      }
    }
  } else {
    std::vector<double> aux(N, 0.0);
    const float b = N * edge;
    const float slope1 = ratio;
    float slope2 = ratio;
    if (slope1 < 1.0) slope2 = (N - slope1 * b) / (N - b);
    for (int s = 0; s < N; s++) {
      const float s1 = s - 0.5, s2 = s + 0.5;
      float d1 = s1 * slope1;
      if (s1 > b) d1 = b * slope1 + (s1 - b) * slope2;
      float d2 = s2 * slope1;
      if (s2 > b) d2 = b * slope1 + (s2 - b) * slope2;
      const int i1 = int(std::floor(d1)), i2 = int(std::ceil(d2));
      if (i1 <= N - 1) {
        const double alpha = 1.0;
        const double alpha1 = (1.0 - (d1 - i1)) * alpha, alpha2 = (i2 - d2) * alpha;
        for (int j = i1; j <= i2; j++) {
          int k = j;
          if (k < 0) k = 0;
          if (k >= N) break;
          double a = alpha;
          if (j == i1) a = alpha1;
          if (j == i2) a = alpha2;
          W[(size_t)k * N + s] += a;
          aux[k] += a;
        }
      }
    }
    for (int k = 0; k < N; k++)
      if (aux[k] > 1E-20)
        for (int s = 0; s < N; s++) W[(size_t)k * N + s] /= aux[k];
  }
  int total = 0;
  for (int k = 0; k < N; k++) {
    const double* Wr = W.data() + (size_t)k * inN;
    int lo = 0, hi = inN - 1;
    while (lo < inN && Wr[lo] == 0.0) lo++;
    while (hi >= lo && Wr[hi] == 0.0) hi--;
    const int cn = lo < inN ? hi - lo + 1 : 0;
    if (total + cn > w_cap) return btk_set_error(BTK_ERR_DIMENSION, "btk_fe_vtln_table: more than %d weights", w_cap);
    offset[k] = cn ? lo : 0;
    count[k] = cn;
    for (int i = 0; i < cn; i++) w[total + i] = Wr[lo + i];
    total += cn;
  }
  *nw = total;
  return BTK_OK;
}

int btk_fe_dct_table(int type, int cepN, int filterN, float* dct)
{
#pragma clang fp contract(off)
  if (!dct) return btk_set_error(BTK_ERR_PARAMETER, "btk_fe_dct_table: null argument");
  if (type < 0 || type > 2) return btk_set_error(BTK_ERR_PARAMETER, "btk_fe_dct_table: unknown DCT type %d", type);
  if (cepN < 1 || filterN < 1 || (type == 0 && filterN < 2))
    return btk_set_error(BTK_ERR_DIMENSION, "btk_fe_dct_table: cepN=%d filterN=%d", cepN, filterN);
  for (int k = 0; k < cepN; k++) {
    float* row = dct + (size_t)k * filterN;
    if (type == 0) {
      const double fac = k * M_PI / (double)(filterN - 1);
      row[0] = 1.0;
      for (int l = 1; l < filterN - 1; l++) row[l] = 2.0 * std::cos(fac * l);
      row[filterN - 1] = std::cos(k * M_PI);
    } else if (type == 1) {
      const double fac = k * M_PI / (double)filterN;
      for (int l = 0; l < filterN; l++) row[l] = std::cos(fac * (l + 0.5));
    } else {
      const double deltaF = M_PI * float(k) / filterN;
      for (int l = 0; l < filterN; l++) {
        const double frequency = deltaF * (l + 0.5);
        double c = std::cos(frequency) / filterN;
        if (l == 0) c *= 0.5;
        row[l] = c;
      }
    }
  }
  return BTK_OK;
}

}  // extern "C"
