// conv_kernels.hip -- FFT block convolution: the reference's OverlapAdd / OverlapSave (convolution/convolution.cc:83-131, :196-230)
// as FIR filtering of whole rows, every output tile of every (stream, impulse response) in one launch.
//
// One kernel form, conv_tile_kernel: a workgroup owns one tile of one output row.  It reads a span of N samples (zero where the
// row has none), holds it as an N/2-point complex transform in LDS (fft_long.h, split / pre-twist steps as in tdoa_kernels.hip),
// multiplies the half spectrum by the filter's and stores n_out samples of the inverse transform starting at section index o:
// the overlap-SAVE arrangement.  OverlapAdd's output is the same linear convolution; its float32 running sum is not re-enacted.
// A filter longer than one section is cut into Q partitions of Bp taps; partition q reads the span shifted back by q Bp, the bin
// products are summed over q in registers, one inverse transform follows (Q + 1 transforms a tile).
//
// A span element that no stored sample depends on is read as zero (the samples behind the tile's last output, and in front of a
// short last partition), so the bits of an output sample are a function of the samples and taps its sum names and of the tile's
// position alone: calls that cut a row at tile boundaries reproduce the bits of one call over the whole row.
#include <atomic>
#include <cmath>
#include <map>
#include <mutex>
#include <vector>
#include "btk_internal.h"
#include "fft_long.h"

namespace {

constexpr int CONV_MIN_N = 256, CONV_MAX_N = 16384;

template <int LOG2NF> struct conv_cfg {
  static constexpr int NF = 1 << LOG2NF;
  static constexpr int NT = NF / 4 < 64 ? 64 : (NF / 4 > 512 ? 512 : NF / 4);
};
// waves per SIMD the tile kernel is compiled for.  N = 8192 would take 134 VGPRs, which leaves ONE workgroup of eight waves on a
// CU; held to 128 (no scratch) two fit.  The other lengths are where the compiler puts them (N = 16384: 228 VGPRs, one workgroup).
constexpr int conv_min_waves(int log2nf) { return log2nf == 12 ? 4 : 1; }

// bins k and NF - k of the N = 2 NF point real transform whose packed NF-point complex transform lies in buf
// (X[k] = E[k] + w^k O[k], X[NF-k] = conj(E[k] - w^k O[k]), w = exp(-i 2 pi / N)); k == 0 gives the two real bins 0 and N/2
template <int NF>
__device__ __forceinline__ void conv_split(const float2* __restrict__ buf, const float2* __restrict__ tw, int k, float2& x0,
                                           float2& x1)
{
  constexpr int TS = BTK_LONGFFT_TWN / (2 * NF);
  const float2 A = buf[k], B = cconjf(buf[(NF - k) & (NF - 1)]);
  const float2 E = make_float2(0.5f * (A.x + B.x), 0.5f * (A.y + B.y));
  const float2 O = make_float2(0.5f * (A.y - B.y), -0.5f * (A.x - B.x));   // (A - B) / (2 i)
  const float2 wO = k == 0 ? O : cmulf(O, tw[k * TS]);
  x0 = caddf(E, wO);
  x1 = cconjf(csubf(E, wO));
}

// span element i of a tile: sample `at + i` of a row that holds samples lo .. len - 1, for i0 <= i < i1 only
__device__ __forceinline__ float conv_sample(const float* __restrict__ x, long at, int i, int i0, int i1, long lo, long len)
{
  const long n = at + i;
  return (i >= i0 && i < i1 && n >= lo && n < len) ? x[n] : 0.f;
}

// ---- the tile kernel.  Workgroup f = row * tiles + tile, row = s C + c.
//   x + s x_stride: the stream's samples lo .. len - 1 (lo = -hist);  H + ((s or 0) C + c) Q (NF + 1): the filter's Q half spectra
//   span of partition q starts at sample  tile span_step - q Bp + span0;  taps_last: taps of partition Q - 1
//   outputs: section indices o .. o + n - 1 go to y[row y_stride + tile out_step + 0 .. n - 1], n = min(n_out, out_len - tile out_step)
template <int LOG2NF, int NT>
__global__ __launch_bounds__(NT, conv_min_waves(LOG2NF)) void conv_tile_kernel(const float* __restrict__ x, long x_stride, long lo, long len,
                                                       const float2* __restrict__ H, int per_stream, int C, int Q, int Bp,
                                                       int taps_last, long tiles, long span0, long span_step, int o,
                                                       float* __restrict__ y, long y_stride, long out_step, long out_len,
                                                       int n_out, const float2* __restrict__ tw)
{
  constexpr int NF = 1 << LOG2NF, N = 2 * NF;
  constexpr int TS = BTK_LONGFFT_TWN / N;
  constexpr int U = NF / 2 / NT;                   // bin pairs (k, NF - k), 0 <= k < NF/2, per thread; bin NF/2 is thread 0's
  static_assert(U >= 1 && U * NT == NF / 2, "the bin pairs must tile the workgroup");
  extern __shared__ float2 buf[];
  const int tid = threadIdx.x;
  const long f = blockIdx.x;
  const long tile = f % tiles, row = f / tiles;
  const long s = row / C, c = row % C;
  const float* xs = x + s * x_stride;
  const float2* Hr = H + ((per_stream ? s : 0) * C + c) * (long)Q * (NF + 1);
  const long left = out_len - tile * out_step;
  const int n = left < n_out ? (int)left : n_out;  // samples this tile stores (>= 1: the host launches no empty tile)
  const int i1 = o + n;                            // no stored sample depends on span elements from here on

  float2 acc0[U], acc1[U], accm = make_float2(0.f, 0.f);
#pragma unroll
  for (int u = 0; u < U; u++) acc0[u] = acc1[u] = make_float2(0.f, 0.f);

  for (int q = 0; q < Q; q++) {
    const long at = tile * span_step + span0 - (long)q * Bp;
    const int i0 = q == Q - 1 ? o - (taps_last - 1) : o - (Bp - 1);   // nor on the ones in front of the partition's reach
    if (q) __syncthreads();                        // the split step of the previous partition has read buf
    for (int m = tid; m < NF; m += NT)
      buf[m] = make_float2(conv_sample(xs, at, 2 * m, i0, i1, lo, len), conv_sample(xs, at, 2 * m + 1, i0, i1, lo, len));
    __syncthreads();
    fft_long<LOG2NF, NT, -1>(buf, tw, tid);
    const float2* Hq = Hr + (long)q * (NF + 1);
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int k = tid + u * NT;
      float2 x0, x1;
      conv_split<NF>(buf, tw, k, x0, x1);
      const float2 h0 = Hq[k], h1 = Hq[NF - k];
      if (k == 0) {                                // bins 0 and N/2: real times real (convolution.cc:103-104)
        acc0[u].x = fmaf(x0.x, h0.x, acc0[u].x);
        acc1[u].x = fmaf(x1.x, h1.x, acc1[u].x);
      } else {
        acc0[u] = caddf(acc0[u], cmulf(x0, h0));
        acc1[u] = caddf(acc1[u], cmulf(x1, h1));
      }
    }
    if (tid == 0) {
      float2 x0, x1;
      conv_split<NF>(buf, tw, NF / 2, x0, x1);
      accm = caddf(accm, cmulf(x0, Hq[NF / 2]));
    }
  }
  __syncthreads();
  // pre-twist: Z[k] = (G[k] + conj G[NF-k]) + i v^k (G[k] - conj G[NF-k]), v = exp(+i 2 pi / N)
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int k = tid + u * NT;
    const float2 Gk = acc0[u], Gm = acc1[u];
    if (k == 0) {
      buf[0] = make_float2(Gk.x + Gm.x, Gk.x - Gm.x);
    } else {
      const float2 Sm = make_float2(Gk.x + Gm.x, Gk.y - Gm.y), Df = make_float2(Gk.x - Gm.x, Gk.y + Gm.y);
      const float2 T = cmulf(Df, cconjf(tw[k * TS]));
      buf[k] = make_float2(Sm.x - T.y, Sm.y + T.x);
      buf[NF - k] = make_float2(Sm.x + T.y, T.x - Sm.y);
    }
  }
  if (tid == 0) {                                  // k == NF - k: G[k] meets itself
    const float2 Sm = make_float2(2.f * accm.x, 0.f), Df = make_float2(0.f, 2.f * accm.y);
    const float2 T = cmulf(Df, cconjf(tw[(NF / 2) * TS]));
    buf[NF / 2] = make_float2(Sm.x - T.y, Sm.y + T.x);
  }
  __syncthreads();
  fft_long<LOG2NF, NT, +1>(buf, tw, tid);
  // z[m] = N (g[2m] + i g[2m+1])
  constexpr float invN = 1.f / (float)N;
  float* yr = y + row * y_stride + tile * out_step;
  const float* g = reinterpret_cast<const float*>(buf);
  for (int j = tid; j < n; j += NT) yr[j] = g[o + j] * invN;
}

// ---- the filter's half spectra by the same forward path: workgroup (r, q) transforms taps q Bp .. of row r, zero padded to N
template <int LOG2NF, int NT>
__global__ __launch_bounds__(NT) void conv_spectrum_kernel(const float* __restrict__ h, long h_stride, int P, int Q, int Bp,
                                                           float2* __restrict__ H, const float2* __restrict__ tw)
{
  constexpr int NF = 1 << LOG2NF;
  extern __shared__ float2 buf[];
  const int tid = threadIdx.x;
  const long f = blockIdx.x;
  const int q = (int)(f % Q);
  const long r = f / Q;
  const int rest = P - q * Bp, taps = rest < Bp ? rest : Bp;
  const float* hr = h + r * h_stride + (long)q * Bp;
  for (int m = tid; m < NF; m += NT)
    buf[m] = make_float2(2 * m < taps ? hr[2 * m] : 0.f, 2 * m + 1 < taps ? hr[2 * m + 1] : 0.f);
  __syncthreads();
  fft_long<LOG2NF, NT, -1>(buf, tw, tid);
  float2* Hq = H + f * (NF + 1);
  for (int k = tid; k <= NF / 2; k += NT) {
    float2 x0, x1;
    conv_split<NF>(buf, tw, k, x0, x1);
    Hq[k] = x0;
    if (k != NF - k) Hq[NF - k] = x1;
  }
}

// ---- fft_long.h's twiddle table, one per device, built in float64 on the host and uploaded at the first use
std::mutex g_mu;
std::map<int, float2*> g_tw;

int conv_twiddles(const float2** out)
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

// a workgroup's LDS exceeds the default limit at the largest transform: raised once per kernel instantiation and device
template <int TAG, class K> int conv_allow_lds(K kern, size_t lds)
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

int conv_log2(int N)
{
  if (N < CONV_MIN_N || N > CONV_MAX_N || (N & (N - 1))) return -1;
  int n = 0;
  while ((1 << n) < N) n++;
  return n;
}

struct conv_launch {
  const float* x; long x_stride, lo, len;
  const float2* H; int per_stream, C, Q, Bp, taps_last;
  long rows, tiles, span0, span_step; int o;
  float* y; long y_stride, out_step, out_len; int n_out;
};

template <int LOG2NF> int launch_tiles(const conv_launch& a, const float2* tw, hipStream_t st)
{
  constexpr int NF = 1 << LOG2NF, NT = conv_cfg<LOG2NF>::NT;
  auto kern = conv_tile_kernel<LOG2NF, NT>;
  const size_t lds = sizeof(float2) * NF;
  if (int rc = conv_allow_lds<2 * LOG2NF>(kern, lds)) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)(a.rows * a.tiles)), dim3(NT), lds, st, a.x, a.x_stride, a.lo, a.len, a.H, a.per_stream,
                     a.C, a.Q, a.Bp, a.taps_last, a.tiles, a.span0, a.span_step, a.o, a.y, a.y_stride, a.out_step, a.out_len,
                     a.n_out, tw);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

template <int LOG2NF>
int launch_spectrum(const float* h, long h_stride, long R, int P, int Q, int Bp, float2* H, const float2* tw, hipStream_t st)
{
  constexpr int NF = 1 << LOG2NF, NT = conv_cfg<LOG2NF>::NT;
  auto kern = conv_spectrum_kernel<LOG2NF, NT>;
  const size_t lds = sizeof(float2) * NF;
  if (int rc = conv_allow_lds<2 * LOG2NF + 1>(kern, lds)) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)(R * Q)), dim3(NT), lds, st, h, h_stride, P, Q, Bp, H, tw);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

int dispatch_tiles(int lg, const conv_launch& a, hipStream_t st)
{
  if (a.rows * a.tiles > 0x7fffffffL)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_conv: %ld tiles in one launch", a.rows * a.tiles);
  const float2* tw;
  if (int rc = conv_twiddles(&tw)) return rc;
  switch (lg - 1) {
    case 7: return launch_tiles<7>(a, tw, st);
    case 8: return launch_tiles<8>(a, tw, st);
    case 9: return launch_tiles<9>(a, tw, st);
    case 10: return launch_tiles<10>(a, tw, st);
    case 11: return launch_tiles<11>(a, tw, st);
    case 12: return launch_tiles<12>(a, tw, st);
    default: return launch_tiles<13>(a, tw, st);
  }
}

int next_pow2(long v)
{
  long n = 1;
  while (n < v && n < (1L << 30)) n <<= 1;
  return (int)n;
}

}  // namespace

extern "C" {

int btk_conv_plan(int P, int n_max, int* N, int* Lk, int* Bp, int* Q)
{
  if (P < 1) return btk_set_error(BTK_ERR_DIMENSION, "btk_conv_plan: P=%d taps", P);
  if (conv_log2(n_max) < 0)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_conv_plan: n_max=%d must be a power of two from %d to %d", n_max, CONV_MIN_N,
                         CONV_MAX_N);
  if (!N || !Lk || !Bp || !Q) return btk_set_error(BTK_ERR_PARAMETER, "btk_conv_plan: null argument");
  // four times the taps, but not below 8192 where n_max admits it: with two workgroups on a CU that length filtered fastest
  // at 500 and at 2000 taps (bench_conv.py's sweep), and 4 P leads there or beyond from 1025 taps on anyway
  int n = next_pow2(4L * P);
  n = n < 8192 ? 8192 : n;
  n = n > n_max ? n_max : n;
  const int bp = P <= n / 2 + 1 ? P : n / 2;
  *N = n;
  *Bp = bp;
  *Q = (P + bp - 1) / bp;
  *Lk = n - bp + 1;
  return BTK_OK;
}

static int conv_check_plan(const char* who, int P, int N, int Bp, int Q)
{
  if (conv_log2(N) < 0)
    return btk_set_error(BTK_ERR_DIMENSION, "%s: N=%d must be a power of two from %d to %d", who, N, CONV_MIN_N, CONV_MAX_N);
  if (P < 1 || Bp < 1 || Q < 1 || Bp > N || (long)Q * Bp < P || (long)(Q - 1) * Bp >= P)
    return btk_set_error(BTK_ERR_DIMENSION, "%s: P=%d taps in Q=%d partitions of Bp=%d", who, P, Q, Bp);
  return BTK_OK;
}

int btk_conv_filter_spectra(const float* h, long h_stride, int R, int P, int N, int Bp, int Q, void* H, void* stream)
{
  if (int rc = conv_check_plan("btk_conv_filter_spectra", P, N, Bp, Q)) return rc;
  if (R < 1 || h_stride < P) return btk_set_error(BTK_ERR_DIMENSION, "btk_conv_filter_spectra: R=%d h_stride=%ld P=%d", R, h_stride, P);
  if ((long)R * Q > 0x7fffffffL) return btk_set_error(BTK_ERR_DIMENSION, "btk_conv_filter_spectra: %ld spectra", (long)R * Q);
  if (!h || !H) return btk_set_error(BTK_ERR_PARAMETER, "btk_conv_filter_spectra: null argument");
  const float2* tw;
  if (int rc = conv_twiddles(&tw)) return rc;
  hipStream_t st = as_stream(stream);
  float2* Hd = reinterpret_cast<float2*>(H);
  switch (conv_log2(N) - 1) {
    case 7: return launch_spectrum<7>(h, h_stride, R, P, Q, Bp, Hd, tw, st);
    case 8: return launch_spectrum<8>(h, h_stride, R, P, Q, Bp, Hd, tw, st);
    case 9: return launch_spectrum<9>(h, h_stride, R, P, Q, Bp, Hd, tw, st);
    case 10: return launch_spectrum<10>(h, h_stride, R, P, Q, Bp, Hd, tw, st);
    case 11: return launch_spectrum<11>(h, h_stride, R, P, Q, Bp, Hd, tw, st);
    case 12: return launch_spectrum<12>(h, h_stride, R, P, Q, Bp, Hd, tw, st);
    default: return launch_spectrum<13>(h, h_stride, R, P, Q, Bp, Hd, tw, st);
  }
}

int btk_conv_apply(const float* x, long len, long hist, long x_stride, int S, const void* H, int S_h, int C, int P, int N, int Lk,
                   int Bp, int Q, float* y, long out_len, long y_stride, void* stream)
{
  if (int rc = conv_check_plan("btk_conv_apply", P, N, Bp, Q)) return rc;
  if (Lk < 1 || (long)Lk + Bp - 1 > N)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_conv_apply: a tile of Lk=%d with Bp=%d taps does not fit N=%d", Lk, Bp, N);
  if (S < 1 || C < 1 || (S_h != 1 && S_h != S))
    return btk_set_error(BTK_ERR_DIMENSION, "btk_conv_apply: S=%d C=%d S_h=%d (1 or S)", S, C, S_h);
  if (len < 0 || hist < 0 || out_len < 1 || y_stride < out_len || (S > 1 && x_stride < len + hist))
    return btk_set_error(BTK_ERR_DIMENSION, "btk_conv_apply: len=%ld hist=%ld x_stride=%ld out_len=%ld y_stride=%ld", len, hist,
                         x_stride, out_len, y_stride);
  if (!x || !H || !y) return btk_set_error(BTK_ERR_PARAMETER, "btk_conv_apply: null argument");
  conv_launch a;
  a.x = x; a.x_stride = x_stride; a.lo = -hist; a.len = len;
  a.H = reinterpret_cast<const float2*>(H); a.per_stream = S_h != 1; a.C = C; a.Q = Q; a.Bp = Bp; a.taps_last = P - (Q - 1) * Bp;
  a.rows = (long)S * C; a.tiles = (out_len + Lk - 1) / Lk; a.span0 = -(long)(Bp - 1); a.span_step = Lk; a.o = Bp - 1;
  a.y = y; a.y_stride = y_stride; a.out_step = Lk; a.out_len = out_len; a.n_out = Lk;
  return dispatch_tiles(conv_log2(N), a, as_stream(stream));
}

int btk_conv_blocks(const float* x, long len, long x_stride, int S, long T, long block_step, const void* H, int S_h, int C, int P,
                    int L, float* y, void* stream)
{
  if (conv_log2(L) < 0)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_conv_blocks: L=%d must be a power of two from %d to %d", L, CONV_MIN_N, CONV_MAX_N);
  if (P < 1 || P >= L) return btk_set_error(BTK_ERR_DIMENSION, "btk_conv_blocks: cannot have P = %d and L = %d", P, L);
  if (S < 1 || C < 1 || (S_h != 1 && S_h != S))
    return btk_set_error(BTK_ERR_DIMENSION, "btk_conv_blocks: S=%d C=%d S_h=%d (1 or S)", S, C, S_h);
  if (T < 1 || block_step < 1 || len < 0 || (S > 1 && x_stride < len))
    return btk_set_error(BTK_ERR_DIMENSION, "btk_conv_blocks: T=%ld block_step=%ld len=%ld x_stride=%ld", T, block_step, len, x_stride);
  if (!x || !H || !y) return btk_set_error(BTK_ERR_PARAMETER, "btk_conv_blocks: null argument");
  const int n = L - P;
  conv_launch a;
  a.x = x; a.x_stride = x_stride; a.lo = 0; a.len = len;
  a.H = reinterpret_cast<const float2*>(H); a.per_stream = S_h != 1; a.C = C; a.Q = 1; a.Bp = P; a.taps_last = P;
  a.rows = (long)S * C; a.tiles = T; a.span0 = 0; a.span_step = block_step; a.o = P;
  a.y = y; a.y_stride = T * (long)n; a.out_step = n; a.out_len = T * (long)n; a.n_out = n;
  return dispatch_tiles(conv_log2(L), a, as_stream(stream));
}

}  // extern "C"
