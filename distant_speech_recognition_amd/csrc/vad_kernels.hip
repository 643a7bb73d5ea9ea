// vad_kernels.hip -- voice activity detection (reference sad/sad.cc) for gfx950: the energy family.
//
// Replaces SimpleEnergyVAD::next (:155-175), EnergyVADMetric::above_threshold_ / next (:518-588), the band powers and decisions of
// PowerSpectrumVADMetric / NormalizedEnergyMetric / TSPSVADMetric::next (:694-739, :777-830, :1005-1057) with the band edges of
// MultiChannelVADMetric (:629-663), and HangoverVADFeature::next with the three above_threshold_ rules (:1763-1843, :1859-1885,
// :1910-1951).  Layouts, state and limits: include/btkhip.h.
//
// Frame-parallel, stateless (one lane owns one frame and adds in the reference's order; neighbouring lanes own neighbouring frames;
// the inputs are read where their producers left them, through element strides, without a transposing copy):
//   1. vad_energy_kernel<CPLX>   : sum_n (double)x[n] (double)x[n] in index order (re^2 + im^2 per element for complex input).
//   2. vad_bandpower_kernel<KIND>: P_c = (sum_{k = lowX .. highX} w_k S_c[k]) / fftLen per channel, then the score and the +-1 value.
// The square of a float32 value is exact in float64 (24 + 24 <= 53 significand bits), and so is 2 x: a fused multiply-add and a
// product followed by a sum therefore round once, at the same place, and give the same bits -- the compiler may contract freely
// in 1. and 2.  Only re^2 + im^2 of one element is a sum of two exact products: fma(re, re, im im) rounds the exact sum once, as
// the reference's im im + re re does.  Divisions and square roots are the IEEE ones (hipcc's default for float64).
//
// Sequential in time, one wavefront per stream, state in a device struct between launches (a block cut anywhere continues with
// the very numbers an uncut launch carries):
//   3. vad_energy_metric_kernel  : the window of up to 1024 float64 energies lies over the 64 lanes as a ring (slot j in lane
//                                  j % 64, register j / 64; no order is needed: `sum > sorted[medianX]` holds exactly when more
//                                  than medianX slots are strictly below sum, and the shift overwrites the oldest slot).  The
//                                  count goes through one ballot + popcount per register row; the head/tail machine is uniform.
//   4. vad_recursion_kernel      : s <- gamma s + (1 - gamma) E with two rounded products and one rounded sum, E / s > threshold.
//   5. vad_hangover_kernel       : the single / MI / multi-stage rule per frame (lanes, 64 frames at a time), the detections as a
//                                  ballot mask, the head/tail machine over its bits; (start, end, ended) and the segment list.
//   6. vad_gather_kernel         : source rows [start, end) into the output block.
#include "btk_internal.h"
#include <cmath>
#include <cstdint>

namespace {

constexpr int VAD_NT = 64;
constexpr int VAD_MAXWIN = 1024;
constexpr int VAD_ROWS = VAD_MAXWIN / 64;
constexpr int VAD_MAXMETRICS = 8;

template <bool CPLX>
__global__ __launch_bounds__(VAD_NT)
void vad_energy_kernel(const float* __restrict__ x, int D, long T, long stream_stride, long frame_stride, long elem_stride,
                       double* __restrict__ energy, long e_stride)
{
  const long t = (long)blockIdx.x * VAD_NT + threadIdx.x;
  const int s = blockIdx.y;
  if (t >= T) return;
  double sum = 0.0;
  if (CPLX) {
    const float2* p = reinterpret_cast<const float2*>(x) + (long)s * stream_stride + t * frame_stride;
    for (int n = 0; n < D; n++) {
      const float2 v = p[(long)n * elem_stride];
      const double re = (double)v.x, im = (double)v.y;
      sum += fma(re, re, im * im);                              // gsl_complex_abs2: one rounding of the exact re^2 + im^2
    }
  } else {
    const float* p = x + (long)s * stream_stride + t * frame_stride;
    for (int n = 0; n < D; n++) {
      const double v = (double)p[(long)n * elem_stride];
      sum += v * v;
    }
  }
  energy[(long)s * e_stride + t] = sum;
}

template <int KIND>
__global__ __launch_bounds__(VAD_NT)
void vad_bandpower_kernel(const float* __restrict__ spec, int C, int M, long T, long stream_stride, long chan_stride,
                          long frame_stride, long bin_stride, int lowX, int highX, double E0, double thr,
                          double* __restrict__ P, double* __restrict__ score, double* __restrict__ value, long o_stride)
{
  const long t = (long)blockIdx.x * VAD_NT + threadIdx.x;
  const int s = blockIdx.y;
  if (t >= T) return;
  const int nyq1 = M / 2 + 1;                                   // the reference tests fftLen2_ + 1 (:715): Nyquist is doubled
  const double fftLen = (double)M;
  double total = 0.0, p0 = 0.0;
  for (int c = 0; c < C; c++) {
    const float* row = spec + (long)s * stream_stride + (long)c * chan_stride + t * frame_stride;
    double pw = 0.0;
    for (int k = lowX; k <= highX; k++) {
      const double v = (double)row[(long)k * bin_stride];
      pw += (k == 0 || k == nyq1) ? v : 2.0 * v;
    }
    pw /= fftLen;
    total += (KIND == BTK_VAD_NORMALIZED) ? sqrt(pw) : pw;
    if (c == 0) p0 = pw;
    if (P) P[((long)s * C + c) * o_stride + t] = pw;
  }
  double sc;
  bool speech;
  if (KIND == BTK_VAD_POWER) {
    sc = p0 / total;
    speech = sc > thr;
  } else if (KIND == BTK_VAD_NORMALIZED) {
    sc = sqrt(p0) / total;
    speech = sc > thr;
  } else {
    sc = log(p0 / (total - p0)) - log(E0 / total);
    speech = sc > 0.0;
  }
  const long o = (long)s * o_stride + t;
  if (score) score[o] = sc;
  value[o] = speech ? 1.0 : -1.0;
}

// state of one stream: int64 {ring position, recognizing, abovethresholdN, belowThresholdN}, then float64 ring[energiesN].
// ROWS: register rows of the ring, 64 ROWS >= energiesN (1, 4 or 16: the per-frame work is one compare + ballot and one
// conditional move per row)
template <int ROWS>
__global__ __launch_bounds__(64)
void vad_energy_metric_kernel(const double* __restrict__ energy, long e_stride, long T, int N, int medianX, unsigned headN,
                              unsigned tailN, long long* __restrict__ state, double* __restrict__ value, long v_stride)
{
  const int s = blockIdx.x, lane = threadIdx.x;
  long long* hdr = state + (long)s * (4 + N);
  double* ring = reinterpret_cast<double*>(hdr + 4);
  const int rows = (N + 63) >> 6;
  double w[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; r++) w[r] = (r < rows && r * 64 + lane < N) ? ring[r * 64 + lane] : 0.0;
  int pos = (int)hdr[0];
  bool recognizing = hdr[1] != 0;
  unsigned aboveN = (unsigned)hdr[2], belowN = (unsigned)hdr[3];
  const double* e = energy + (long)s * e_stride;
  double* out = value + (long)s * v_stride;
  for (long t0 = 0; t0 < T; t0 += 64) {
    const int n = (T - t0) < 64 ? (int)(T - t0) : 64;
    const double mine = lane < n ? e[t0 + lane] : 0.0;
    double res = 0.0;
    for (int j = 0; j < n; j++) {
      const double sum = __shfl(mine, j, 64);
      int cnt = 0;                                              // #{slots < sum}: a NaN on either side counts as not below
#pragma unroll
      for (int r = 0; r < ROWS; r++)
        if (r < rows) cnt += __popcll(__ballot(r * 64 + lane < N && w[r] < sum));
      const bool above = cnt > medianX;
      if (!recognizing && aboveN == 0) {                        // the sorted copy was taken first (:526-532)
        const int pr = pos >> 6, pl = pos & 63;
#pragma unroll
        for (int r = 0; r < ROWS; r++)
          if (r == pr && lane == pl) w[r] = sum;
        pos = pos + 1 == N ? 0 : pos + 1;
      }
      if (recognizing) {
        if (above) belowN = 0;
        else if (++belowN == tailN) { recognizing = false; aboveN = 0; }
      } else {
        if (above) { if (++aboveN == headN) { recognizing = true; belowN = 0; } }
        else aboveN = 0;
      }
      if (lane == j) res = above ? 1.0 : 0.0;
    }
    if (lane < n) out[t0 + lane] = res;
  }
#pragma unroll
  for (int r = 0; r < ROWS; r++)
    if (r < rows && r * 64 + lane < N) ring[r * 64 + lane] = w[r];
  if (lane == 0) { hdr[0] = pos; hdr[1] = recognizing ? 1 : 0; hdr[2] = aboveN; hdr[3] = belowN; }
}

// gamma s + (1 - gamma) E as the reference's x86 code rounds it: two products, one sum.  (__dmul_rn / __dadd_rn are plain
// operators to hipcc and would be contracted into a fused multiply-add; the pragma is what keeps the three roundings.)
__device__ __forceinline__ double vad_smooth(double gamma, double s, double omg, double E)
{
#pragma clang fp contract(off)
  const double a = gamma * s;
  const double b = omg * E;
  return a + b;
}

__global__ __launch_bounds__(64)
void vad_recursion_kernel(const double* __restrict__ energy, long e_stride, long T, double gamma, double omg, double threshold,
                          double* __restrict__ state, int* __restrict__ is_speech, double* __restrict__ smoothed, long o_stride)
{
  const int s = blockIdx.x, lane = threadIdx.x;
  const double* e = energy + (long)s * e_stride;
  double se = state[s];
  for (long t0 = 0; t0 < T; t0 += 64) {
    const int n = (T - t0) < 64 ? (int)(T - t0) : 64;
    const double mine = lane < n ? e[t0 + lane] : 0.0;
    double my_s = 0.0;
    for (int j = 0; j < n; j++) {
      const double E = __shfl(mine, j, 64);
      se = vad_smooth(gamma, se, omg, E);
      if (lane == j) my_s = se;
    }
    if (lane < n) {
      is_speech[(long)s * o_stride + t0 + lane] = (mine / my_s > threshold) ? 1 : 0;
      if (smoothed) smoothed[(long)s * o_stride + t0 + lane] = my_s;
    }
  }
  if (lane == 0) state[s] = se;
}

struct vad_metric_rows { const double* v[VAD_MAXMETRICS]; double thr[VAD_MAXMETRICS]; };

// state of one stream: int64 {abovethresholdN, belowThresholdN, recognizing, frames seen, start, end, ended, decision_metric}
__global__ __launch_bounds__(64)
void vad_hangover_kernel(vad_metric_rows rows, int R, int rule, long T, long v_stride, unsigned headN, unsigned tailN, int restart,
                         long long* __restrict__ state, int* __restrict__ decision, long d_stride, long long* __restrict__ segments,
                         int max_seg, int* __restrict__ nseg)
{
  const int s = blockIdx.x, lane = threadIdx.x;
  long long* st = state + (long)s * 8;
  unsigned aboveN = (unsigned)st[0], belowN = (unsigned)st[1];
  bool recognizing = st[2] != 0;
  const long base = st[3];
  long start = st[4], end = st[5];
  bool ended = st[6] != 0;
  int dm = (int)st[7];
  int ns = 0;
  // whether the rule assigns decision_metric_ at all: the single rule and a multi-stage rule short of metrics leave it as it is
  const bool sets = rule == BTK_VAD_RULE_MI || (rule == BTK_VAD_RULE_MULTISTAGE && R >= 3);
  for (long t0 = 0; t0 < T; t0 += 64) {
    const int n = (T - t0) < 64 ? (int)(T - t0) : 64;
    bool above = false;
    int code = 0;
    if (lane < n) {
      const long o = (long)s * v_stride + t0 + lane;
      if (rule == BTK_VAD_RULE_SINGLE) {
        above = rows.v[0][o] > rows.thr[0];
      } else if (rule == BTK_VAD_RULE_MI) {
        if (rows.v[0][o] < 0.5) { code = -1; }
        else if (rows.v[1][o] < 0.5) { code = 2; above = true; }
        else if (rows.v[2][o] > 0.5) { code = 3; above = true; }
        else code = -3;
      } else if (R >= 3) {                                      // multi-stage; with fewer than three metrics: always false (:1912)
        if (rows.v[0][o] < 0.5) code = -1;
        else {
          code = -R;
#pragma unroll
          for (int m = 1; m < VAD_MAXMETRICS; m++)              // unrolled: the row pointers stay scalar kernel arguments
            if (m < R && !above && rows.v[m][o] > 0.5) { code = m + 1; above = true; }
        }
      }
    }
    if (sets) dm = __shfl(code, n - 1, 64);                     // decision_metric_ after the block's last frame
    if (decision && lane < n) decision[(long)s * d_stride + t0 + lane] = sets ? code : dm;
    const unsigned long long mask = __ballot(above);
    for (int j = 0; j < n && !ended; j++) {
      const bool a = (mask >> j) & 1ull;
      const long f = base + t0 + j;
      if (recognizing) {
        if (a) belowN = 0;
        else if (++belowN == tailN) {
          end = f;
          if (lane == 0 && segments && ns < max_seg) {
            segments[((long)s * max_seg + ns) * 2] = start;
            segments[((long)s * max_seg + ns) * 2 + 1] = end;
          }
          ns++;
          if (restart) { recognizing = false; aboveN = belowN = 0; start = end = -1; }
          else ended = true;
        }
      } else {
        if (a) { if (++aboveN == headN) { recognizing = true; start = f - (long)headN + 1; } }
        else aboveN = 0;
      }
    }
  }
  if (lane == 0) {
    st[0] = aboveN; st[1] = belowN; st[2] = recognizing ? 1 : 0; st[3] = base + T; st[4] = start; st[5] = end;
    st[6] = ended ? 1 : 0; st[7] = dm;
    if (nseg) nseg[s] = ns;
  }
}

// dst[s][j] = src[s][start + j - frame_base] for start + j in [max(start, frame_base), min(end, frame_base + T)), j < dst_rows
__global__ __launch_bounds__(256)
void vad_gather_kernel(const float* __restrict__ src, long T, int D, long frame_base, const long long* __restrict__ hstate,
                       float* __restrict__ dst, long dst_rows, long long* __restrict__ count)
{
  const int s = blockIdx.y;
  const long start = hstate[(long)s * 8 + 4];
  long end = hstate[(long)s * 8 + 5];
  const long lim = frame_base + T;
  if (start < 0) { if (blockIdx.x == 0 && threadIdx.x == 0 && count) count[s] = 0; return; }
  if (end < 0 || end > lim) end = lim;
  const long first = start > frame_base ? start : frame_base;
  long j1 = end - start;                                        // output rows [j0, j1)
  const long j0 = first - start;
  if (j1 > dst_rows) j1 = dst_rows;
  if (blockIdx.x == 0 && threadIdx.x == 0 && count) count[s] = j1 > j0 ? j1 - j0 : 0;
  const long total = (j1 - j0) * D;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long j = j0 + i / D, n = i % D;
    dst[((long)s * dst_rows + j) * D + n] = src[((long)s * T + (start + j - frame_base)) * D + n];
  }
}

int vad_check_S(const char* who, int S, long T)
{
  if (S < 1 || S > 65535) return btk_set_error(BTK_ERR_DIMENSION, "%s: S=%d, 1 .. 65535 are supported", who, S);
  if (T < 0) return btk_set_error(BTK_ERR_DIMENSION, "%s: T=%ld", who, T);
  return BTK_OK;
}

}  // namespace

int btk_vad_frame_energy(const void* x, int is_complex, int S, int D, long T, long stream_stride, long frame_stride,
                         long elem_stride, double* energy, long e_stride, void* stream)
{
  const int rc = vad_check_S("btk_vad_frame_energy", S, T);
  if (rc != BTK_OK) return rc;
  if (D < 1 || D > 65536) return btk_set_error(BTK_ERR_DIMENSION, "btk_vad_frame_energy: D=%d, 1 .. 65536 are supported", D);
  if (frame_stride < 1 || elem_stride < 1 || stream_stride < 0 || e_stride < T)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_vad_frame_energy: strides %ld %ld %ld, energy rows of %ld for T=%ld", stream_stride,
                         frame_stride, elem_stride, e_stride, T);
  // rows of frames ([S][D][T_stride], the snapshot layout): T may not run into the next row
  if (elem_stride > frame_stride && T * frame_stride > elem_stride)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_vad_frame_energy: T=%ld frames at stride %ld in rows of %ld", T, frame_stride, elem_stride);
  if (!x || !energy) return btk_set_error(BTK_ERR_PARAMETER, "btk_vad_frame_energy: null argument");
  if (T == 0) return BTK_OK;
  const dim3 grid((unsigned)((T + VAD_NT - 1) / VAD_NT), (unsigned)S);
  hipLaunchKernelGGL(is_complex ? vad_energy_kernel<true> : vad_energy_kernel<false>, grid, dim3(VAD_NT), 0, as_stream(stream),
                     static_cast<const float*>(x), D, T, stream_stride, frame_stride, elem_stride, energy, e_stride);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

int btk_vad_band_limits(int fftLen, double samplerate, double lowCutoff, double highCutoff, int* lowX, int* highX, int* binN)
{
  if (!lowX || !highX || !binN) return btk_set_error(BTK_ERR_PARAMETER, "btk_vad_band_limits: null argument");
  if (fftLen < 2 || !(samplerate > 0.0)) return btk_set_error(BTK_ERR_DIMENSION, "btk_vad_band_limits: fftLen=%d samplerate=%g", fftLen, samplerate);
  unsigned lo = 0, hi = (unsigned)(fftLen / 2);
  if (!(lowCutoff < 0.0)) {
    if (!(lowCutoff < samplerate / 2.0)) return btk_set_error(BTK_ERR_DIMENSION, "Low cutoff cannot be %10.1f", lowCutoff);
    lo = (unsigned)((lowCutoff / samplerate) * (unsigned)fftLen);
  }
  if (!(highCutoff < 0.0)) {
    if (!(highCutoff < samplerate / 2.0)) return btk_set_error(BTK_ERR_DIMENSION, "High cutoff cannot be %10.1f", highCutoff);
    hi = (unsigned)((highCutoff / samplerate) * (unsigned)fftLen + 0.5);
  }
  *lowX = (int)lo;
  *highX = (int)hi;
  *binN = lo > 0 ? (int)(2 * (hi - lo + 1)) : (int)(2 * (hi - lo) + 1);
  return BTK_OK;
}

int btk_vad_band_power(const float* spec, int kind, int S, int C, int M, long T, long stream_stride, long chan_stride,
                       long frame_stride, long bin_stride, int lowX, int highX, double E0, double* P, double* score,
                       double* value, long o_stride, void* stream)
{
  const int rc = vad_check_S("btk_vad_band_power", S, T);
  if (rc != BTK_OK) return rc;
  if (C < 1 || C > 64) return btk_set_error(BTK_ERR_DIMENSION, "btk_vad_band_power: C=%d, 1 .. 64 are supported", C);
  if (M < 2 || M > 2048) return btk_set_error(BTK_ERR_DIMENSION, "btk_vad_band_power: M=%d, 2 .. 2048 are supported", M);
  if (lowX < 0 || lowX > highX || highX > M / 2)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_vad_band_power: bins %d .. %d outside 0 .. %d", lowX, highX, M / 2);
  if (frame_stride < 1 || bin_stride < 1 || stream_stride < 0 || chan_stride < 0 || o_stride < T)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_vad_band_power: strides %ld %ld %ld %ld, output rows of %ld for T=%ld", stream_stride,
                         chan_stride, frame_stride, bin_stride, o_stride, T);
  if (bin_stride > frame_stride && T * frame_stride > bin_stride)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_vad_band_power: T=%ld frames at stride %ld in rows of %ld", T, frame_stride, bin_stride);
  if (kind != BTK_VAD_POWER && kind != BTK_VAD_NORMALIZED && kind != BTK_VAD_TSPS)
    return btk_set_error(BTK_ERR_PARAMETER, "btk_vad_band_power: kind=%d", kind);
  if (!spec || !value) return btk_set_error(BTK_ERR_PARAMETER, "btk_vad_band_power: null argument");
  if (T == 0) return BTK_OK;
  const double thr = E0 / (unsigned)C;                          // E0_ / chanN (:733, :824)
  const dim3 grid((unsigned)((T + VAD_NT - 1) / VAD_NT), (unsigned)S);
  auto k = kind == BTK_VAD_POWER ? vad_bandpower_kernel<BTK_VAD_POWER>
         : kind == BTK_VAD_NORMALIZED ? vad_bandpower_kernel<BTK_VAD_NORMALIZED> : vad_bandpower_kernel<BTK_VAD_TSPS>;
  hipLaunchKernelGGL(k, grid, dim3(VAD_NT), 0, as_stream(stream), spec, C, M, T, stream_stride, chan_stride, frame_stride,
                     bin_stride, lowX, highX, E0, thr, P, score, value, o_stride);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

long btk_vad_energy_metric_state_bytes(int energiesN)
{
  if (energiesN < 1 || energiesN > VAD_MAXWIN) return -1;
  return 8L * (4 + energiesN);
}

int btk_vad_energy_metric(const double* energy, long e_stride, int S, long T, int energiesN, int medianX, unsigned headN,
                          unsigned tailN, void* state, double* value, long v_stride, void* stream)
{
  const int rc = vad_check_S("btk_vad_energy_metric", S, T);
  if (rc != BTK_OK) return rc;
  if (energiesN < 1 || energiesN > VAD_MAXWIN)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_vad_energy_metric: energiesN=%d, 1 .. %d are supported", energiesN, VAD_MAXWIN);
  if (medianX < 0 || medianX >= energiesN)                      // the reference reads past sorted_energies_ there (threshold >= 1)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_vad_energy_metric: median index %d outside 0 .. %d", medianX, energiesN - 1);
  if (e_stride < T || v_stride < T)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_vad_energy_metric: rows of %ld / %ld for T=%ld", e_stride, v_stride, T);
  if (!energy || !state || !value) return btk_set_error(BTK_ERR_PARAMETER, "btk_vad_energy_metric: null argument");
  if (T == 0) return BTK_OK;
  auto k = energiesN <= 64 ? vad_energy_metric_kernel<1> : energiesN <= 256 ? vad_energy_metric_kernel<4> : vad_energy_metric_kernel<VAD_ROWS>;
  hipLaunchKernelGGL(k, dim3((unsigned)S), dim3(64), 0, as_stream(stream), energy, e_stride, T, energiesN, medianX, headN, tailN,
                     static_cast<long long*>(state), value, v_stride);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

int btk_vad_simple_energy(const double* energy, long e_stride, int S, long T, double gamma, double threshold, double* state,
                          int* is_speech, double* smoothed, long o_stride, void* stream)
{
  const int rc = vad_check_S("btk_vad_simple_energy", S, T);
  if (rc != BTK_OK) return rc;
  if (e_stride < T || o_stride < T)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_vad_simple_energy: rows of %ld / %ld for T=%ld", e_stride, o_stride, T);
  if (!energy || !state || !is_speech) return btk_set_error(BTK_ERR_PARAMETER, "btk_vad_simple_energy: null argument");
  if (T == 0) return BTK_OK;
  hipLaunchKernelGGL(vad_recursion_kernel, dim3((unsigned)S), dim3(64), 0, as_stream(stream), energy, e_stride, T, gamma,
                     1.0 - gamma, threshold, state, is_speech, smoothed, o_stride);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

int btk_vad_hangover(const double* const* values, const double* thresholds, int R, int rule, int S, long T, long v_stride,
                     unsigned headN, unsigned tailN, int restart, long long* state, int* decision, long d_stride,
                     long long* segments, int max_seg, int* nseg, void* stream)
{
  const int rc = vad_check_S("btk_vad_hangover", S, T);
  if (rc != BTK_OK) return rc;
  if (R < 1 || R > VAD_MAXMETRICS)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_vad_hangover: %d metrics, 1 .. %d are supported", R, VAD_MAXMETRICS);
  if (headN == 0) return btk_set_error(BTK_ERR_DIMENSION, "btk_vad_hangover: headN=0 (the reference divides by it)");
  if (rule != BTK_VAD_RULE_SINGLE && rule != BTK_VAD_RULE_MI && rule != BTK_VAD_RULE_MULTISTAGE)
    return btk_set_error(BTK_ERR_PARAMETER, "btk_vad_hangover: rule=%d", rule);
  if (rule == BTK_VAD_RULE_MI && R != 3) return btk_set_error(BTK_ERR_DIMENSION, "btk_vad_hangover: the MI rule takes 3 metrics, got %d", R);
  if (v_stride < T || (decision && d_stride < T) || max_seg < 0)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_vad_hangover: rows of %ld / %ld for T=%ld, %d segment slots", v_stride, d_stride, T, max_seg);
  if (!values || !thresholds || !state || (max_seg > 0 && !segments))
    return btk_set_error(BTK_ERR_PARAMETER, "btk_vad_hangover: null argument");
  vad_metric_rows rows;
  for (int m = 0; m < VAD_MAXMETRICS; m++) {
    rows.v[m] = m < R ? values[m] : nullptr;
    rows.thr[m] = m < R ? thresholds[m] : 0.0;
    if (m < R && !values[m]) return btk_set_error(BTK_ERR_PARAMETER, "btk_vad_hangover: null value row %d", m);
  }
  hipLaunchKernelGGL(vad_hangover_kernel, dim3((unsigned)S), dim3(64), 0, as_stream(stream), rows, R, rule, T, v_stride, headN,
                     tailN, restart ? 1 : 0, state, decision, d_stride, max_seg > 0 ? segments : nullptr, max_seg, nseg);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

int btk_vad_gather(const float* src, int S, long T, int D, long frame_base, const long long* hangover_state, float* dst,
                   long dst_rows, long long* count, void* stream)
{
  const int rc = vad_check_S("btk_vad_gather", S, T);
  if (rc != BTK_OK) return rc;
  if (D < 1 || D > 65536 || dst_rows < 0 || frame_base < 0)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_vad_gather: D=%d, %ld output rows, first frame %ld", D, dst_rows, frame_base);
  if (!src || !hangover_state || (dst_rows > 0 && !dst)) return btk_set_error(BTK_ERR_PARAMETER, "btk_vad_gather: null argument");
  long blocks = ((dst_rows < T ? dst_rows : T) * D + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(vad_gather_kernel, dim3((unsigned)blocks, (unsigned)S), dim3(256), 0, as_stream(stream), src, T, D, frame_base,
                     hangover_state, dst, dst_rows, count);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}
