// conv_kernels.hip -- FFT block convolution: the reference's OverlapAdd / OverlapSave (convolution/convolution.cc:83-131, :196-230)
// as FIR filtering of whole rows, every output tile of every (stream, impulse response) in one launch.
//
// One kernel form, conv_tile_kernel: a workgroup owns one tile of one output row.  It reads a span of N samples (zero where the
// row has none), holds it as an N/2-point complex transform in LDS (fft_long.h, the split / pre-twist steps of rfft_long.h),
// multiplies the half spectrum by the filter's and stores n_out samples of the inverse transform starting at section index o:
// the overlap-SAVE arrangement.  OverlapAdd's output is the same linear convolution; its float32 running sum is not re-enacted.
// A filter longer than one section is cut into Q partitions of Bp taps; partition q reads the span shifted back by q Bp, the bin
// products are summed over q in registers, one inverse transform follows (Q + 1 transforms a tile).
//
// A span element that no stored sample depends on is read as zero (the samples behind the tile's last output, and in front of a
// short last partition), so the bits of an output sample are a function of the samples and taps its sum names and of the tile's
// position alone: calls that cut a row at tile boundaries reproduce the bits of one call over the whole row.
#include "btk_internal.h"
#include "rfft_long.h"

namespace {

// waves per SIMD the tile kernel is compiled for.  N = 8192 would take 134 VGPRs, which leaves ONE workgroup of eight waves on a
// CU; held to 128 (no scratch) two fit.  The other lengths are where the compiler puts them (N = 16384: 228 VGPRs, one workgroup).
constexpr int conv_min_waves(int log2nf) { return log2nf == 12 ? 4 : 1; }

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
      rfft_split<NF>(buf, tw, k, x0, x1);
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
      rfft_split<NF>(buf, tw, NF / 2, x0, x1);
      accm = caddf(accm, cmulf(x0, Hq[NF / 2]));
    }
  }
  __syncthreads();
  float2 zk, zm;                                   // pre-twist
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int k = tid + u * NT;
    rfft_pretwist<NF>(acc0[u], acc1[u], tw, k, zk, zm);
    buf[k] = zk;
    if (k != 0) buf[NF - k] = zm;
  }
  if (tid == 0) {                                  // k == NF - k: G[k] meets itself
    rfft_pretwist<NF>(accm, accm, tw, NF / 2, zk, zm);
    buf[NF / 2] = zk;
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
    rfft_split<NF>(buf, tw, k, x0, x1);
    Hq[k] = x0;
    if (k != NF - k) Hq[NF - k] = x1;
  }
}

struct conv_launch {
  const float* x; long x_stride, lo, len;
  const float2* H; int per_stream, C, Q, Bp, taps_last;
  long rows, tiles, span0, span_step; int o;
  float* y; long y_stride, out_step, out_len; int n_out;
};

template <int LOG2NF> int launch_tiles(const conv_launch& a, const float2* tw, hipStream_t st)
{
  constexpr int NF = 1 << LOG2NF, NT = rfft_threads<LOG2NF>;
  constexpr auto kern = conv_tile_kernel<LOG2NF, NT>;
  const size_t lds = sizeof(float2) * NF;
  if (int rc = btk_allow_lds<kern>(lds)) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)(a.rows * a.tiles)), dim3(NT), lds, st, a.x, a.x_stride, a.lo, a.len, a.H, a.per_stream,
                     a.C, a.Q, a.Bp, a.taps_last, a.tiles, a.span0, a.span_step, a.o, a.y, a.y_stride, a.out_step, a.out_len,
                     a.n_out, tw);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

template <int LOG2NF>
int launch_spectrum(const float* h, long h_stride, long R, int P, int Q, int Bp, float2* H, const float2* tw, hipStream_t st)
{
  constexpr int NF = 1 << LOG2NF, NT = rfft_threads<LOG2NF>;
  constexpr auto kern = conv_spectrum_kernel<LOG2NF, NT>;
  const size_t lds = sizeof(float2) * NF;
  if (int rc = btk_allow_lds<kern>(lds)) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)(R * Q)), dim3(NT), lds, st, h, h_stride, P, Q, Bp, H, tw);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

int dispatch_tiles(int lg, const conv_launch& a, hipStream_t st)
{
  if (a.rows * a.tiles > 0x7fffffffL)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_conv: %ld tiles in one launch", a.rows * a.tiles);
  const float2* tw;
  if (int rc = longfft_twiddles(&tw)) return rc;
  return longfft_dispatch(lg, [&](auto n) { return launch_tiles<decltype(n)::value>(a, tw, st); });
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
  if (longfft_log2(n_max) < 0)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_conv_plan: n_max=%d must be a power of two from %d to %d", n_max, RFFT_MIN_L,
                         RFFT_MAX_L);
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
  if (longfft_log2(N) < 0)
    return btk_set_error(BTK_ERR_DIMENSION, "%s: N=%d must be a power of two from %d to %d", who, N, RFFT_MIN_L, RFFT_MAX_L);
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
  if (int rc = longfft_twiddles(&tw)) return rc;
  hipStream_t st = as_stream(stream);
  float2* Hd = reinterpret_cast<float2*>(H);
  return longfft_dispatch(longfft_log2(N), [&](auto n) {
    return launch_spectrum<decltype(n)::value>(h, h_stride, R, P, Q, Bp, Hd, tw, st);
  });
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
  return dispatch_tiles(longfft_log2(N), a, as_stream(stream));
}

int btk_conv_blocks(const float* x, long len, long x_stride, int S, long T, long block_step, const void* H, int S_h, int C, int P,
                    int L, float* y, void* stream)
{
  if (longfft_log2(L) < 0)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_conv_blocks: L=%d must be a power of two from %d to %d", L, RFFT_MIN_L, RFFT_MAX_L);
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
  return dispatch_tiles(longfft_log2(L), a, as_stream(stream));
}

}  // extern "C"
