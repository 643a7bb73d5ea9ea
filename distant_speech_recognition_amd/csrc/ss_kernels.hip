// ss_kernels.hip -- single-channel enhancement for gfx950: spectral subtraction, Wiener filter, spectral high-pass.
//
// Replaces SpectralSubtractor::next + AveragePSDEstimator::add_sample / average / clear (reference
// postfilter/spectralsubtraction.cc:216-285, :89-119, :57-87), WienerFilter::next (:314-362) and HighPassFilter::next
// (postfilter/postfilter.cc:1215-1239).  Layouts, state and limits: include/btkhip.h.
//
// The noise models are first-order recursions along time whose multiplier differs from frame to frame: a frame that does not
// train is the identity map, the first training frame since clear() REPLACES the estimate, later ones forget with alpha:
//     est_t = a_t est_{t-1} + b_t,   (a_t, b_t) = (1, 0) | (0, p_t) | (alpha, (1 - alpha) p_t),   p_t = |X_t|^2
// The Wiener filter's two PSDs obey the same form with (0, p) for the stream's first two frames and (1, 0) for the noise PSD
// of a frame that does not update it.  Affine maps compose associatively, so a 64-frame chunk is one inclusive scan of (a, b)
// pairs in the DPP network (the scan of pf_kernels.hip with one multiplier PER recursion), and the chunk's estimates are
// est_t = A_t carry + B_t with the carry in float64.
//
//   1. ss_rows_kernel     : one wavefront per (stream, bin) row, 64-frame chunks on multiples of 64 of the stream's frame counter,
//                           items = (chunk, channel) pairs, the loads of the next item issued before the current one is scanned;
//                           lane c keeps the float64 carries of channel c (estimate, averaging sum)
//   2. ss_frames_kernel   : no frame trains -> no dependency along time: one or two frames per lane (8- or 16-byte accesses),
//                           rows cut along T across workgroups (a stream of 257 rows is then T/512 x 257 workgroups instead of
//                           257 wavefronts)
//   3. ss_count_kernel    : count / added of the block, after the rows kernel (every row of a stream READS added)
//   4. wiener_rows_kernel : the rows form on (PSDs, PSDn)
//   5. spec_highpass_kernel
// Two kernels and no grid switch for the subtractor: the frame-parallel form needs none of the scan's registers, cross-lane
// steps or the per-lane carries, and its channel loop unrolls over independent loads.
// The outputs are written once and not read again by these kernels: non-temporal stores; X is read once: non-temporal loads.
#include "btk_internal.h"
#include "wave_ops.h"
#include <cstdint>

namespace {

constexpr int SS_MAXC = 64;
constexpr int SS_NT = 256;
constexpr int SS_UNROLL = 4;

// per channel: a = alpha (< 0: averaging channel), b = float(1 - alpha) rounded from float64
struct ss_alpha_t { float a[SS_MAXC]; float b[SS_MAXC]; };

// One step of the inclusive scan (affine_scan_schedule, wave_ops.h) of NB independent sequences of affine maps v -> a[i] v + b[i]: lanes without a source keep the
// identity map (1, 0).  A map with a = 0 forgets its past whatever that is (a NaN estimate is REPLACED by a first sample, as the
// reference's memcpy does), hence the select instead of 0 x p.
// Stated deviation: the select acts on every map whose multiplier is 0, composed maps included.  The reference computes
// alpha prev + (1 - alpha) p, in which 0 x NaN keeps a NaN or Inf estimate for good; here a recursive channel with alpha = 0, the
// Wiener filter at its default alpha = 0.0, and a chunk whose product of alphas underflows to 0 in float32 (0.25^64 = 2^-128)
// drop a non-finite past at the next frame.  Finite data gives the same values either way.
template <int NB, int CTRL, int ROW_MASK>
__device__ __forceinline__ void affine_scan_step(float (&a)[NB], float (&b)[NB])
{
  float a2[NB], p[NB];
#pragma unroll
  for (int i = 0; i < NB; i++) { a2[i] = dpp_or<CTRL, ROW_MASK>(1.f, a[i]); p[i] = dpp_or<CTRL, ROW_MASK>(0.f, b[i]); }
#pragma unroll
  for (int i = 0; i < NB; i++) {
    b[i] = (a[i] == 0.f) ? b[i] : fmaf(a[i], p[i], b[i]);      // (this o earlier)(v) = a (a2 v + p) + b
    a[i] *= a2[i];
  }
}
template <int NB>
__device__ __forceinline__ void affine_scan(float (&a)[NB], float (&b)[NB])
{
  affine_scan_schedule([&](auto ctrl, auto rows) { affine_scan_step<NB, decltype(ctrl)::value, decltype(rows)::value>(a, b); });
}
// the chunk's map applied to the float64 carry
__device__ __forceinline__ double affine_apply(float a, float b, double carry)
{
  return (a == 0.f) ? (double)b : fma((double)a, carry, (double)b);
}

__device__ __forceinline__ float ss_pow(float2 x) { return fmaf(x.x, x.x, x.y * x.y); }

// X sqrt(S2)/|X| with S2 = p - ft est floored (the comparison keeps a NaN, as `S2 <= flooringV_` does); p == 0: (sqrt(S2), 0)
__device__ __forceinline__ float2 ss_term(float2 x, float p, float est, float ft, float floorv)
{
  float s2 = fmaf(-ft, est, p);
  s2 = (s2 <= floorv) ? floorv : s2;
  const float r = sqrtf(s2);
  if (p == 0.f) return make_float2(r, 0.f);
  const float g = r / sqrtf(p);
  return make_float2(__fmul_rn(g, x.x), __fmul_rn(g, x.y));
}
// The channel sum and its scale, with every rounding written out: the row form and the frame-parallel form promise the same bits,
// and no contraction choice of the compiler (g x + sum as one fused multiply-add in one kernel and not in the other) may decide it.
__device__ __forceinline__ void ss_accumulate(float2& sum, float2 term)
{
  sum.x = __fadd_rn(sum.x, term.x);
  sum.y = __fadd_rn(sum.y, term.y);
}
__device__ __forceinline__ float2 ss_mean(float2 sum, float invC) { return make_float2(__fmul_rn(sum.x, invC), __fmul_rn(sum.y, invC)); }

// A guarded load (`ok ? p[t] : 0`) compiles to a branch around the load and a full wait behind it (tools/isa_wait_scan.py), which
// would put the next item's round trip in front of the scan.  The row kernels therefore load from a CLAMPED frame index, always
// inside the row (T >= 1), keep the raw value, and select it against the frame's validity only where it is consumed.
__device__ __forceinline__ long ss_clamp(long t, long T) { return t < 0 ? 0 : (t >= T ? T - 1 : t); }

template <bool HAS_FLAGS>
__global__ __launch_bounds__(64)
void ss_rows_kernel(const float2* __restrict__ X, float2* __restrict__ Y, int K, int C, long T_stride, long T,
                    const unsigned char* __restrict__ flags, int mode, float ft, float floorv, ss_alpha_t al, long frame_base,
                    double* __restrict__ est, double* __restrict__ acc, const unsigned char* __restrict__ added)
{
  const int k = blockIdx.x, s = blockIdx.y;
  const int lane = threadIdx.x;
  // lane c keeps the carries of channel c; a channel's value travels by a uniform-index shuffle
  double est_c = 0.0, acc_c = 0.0;
  int added_c = 0;
  const long sidx = ((long)s * C + lane) * K + k;
  if (lane < C) { est_c = est[sidx]; acc_c = acc[sidx]; added_c = added[(long)s * C + lane]; }
  const float2* x = X + ((long)s * K + k) * C * T_stride;
  float2* y = Y + ((long)s * K + k) * T_stride;
  const float invC = 1.0f / (float)C;
  // chunks on multiples of 64 of the STREAM's frame counter (see zelinski_iir_kernel): blocks cut there scan the same chunks
  const long ph = frame_base & 63;
  bool seen = false;                                            // a training frame earlier in this launch
  long t0 = -ph;
  int c = 0;
  float2 xn = btk_ld<true>(x + ss_clamp(t0 + lane, T));         // raw: validity is applied where the value is used
  int fn = HAS_FLAGS ? (int)flags[ss_clamp(t0 + lane, T)] : mode;
  int f = 0;
  float2 ysum = make_float2(0.f, 0.f);
  while (t0 < T) {
    const long t = t0 + lane;
    const bool ok = t >= 0 && t < T;
    if (c == 0) {
      f = ok ? fn : 0;
      ysum = make_float2(0.f, 0.f);
      if (HAS_FLAGS) fn = (int)flags[ss_clamp(t + 64, T)];
    }
    const float2 xv = ok ? xn : make_float2(0.f, 0.f);
    {                                                           // the next item's load goes out before this one is scanned
      const bool wrap = c + 1 == C;
      xn = btk_ld<true>(x + (long)(wrap ? 0 : c + 1) * T_stride + ss_clamp(wrap ? t + 64 : t, T));
    }
    const bool train = (f & BTK_SS_TRAIN) != 0;                 // f = 0 on lanes outside the block
    const unsigned long long tm = __ballot(train);
    const float alpha = al.a[c];
    const float p = ss_pow(xv);
    const double carry = __shfl(est_c, c, 64);
    double e_d = carry;
    if (tm != 0ull) {                                           // wave-uniform
      if (alpha < 0.f) {
        // averaging channel: products and sum in float64 (the sum has no forgetting factor); est moves in finish_training only
        double pd = train ? (double)xv.x * (double)xv.x + (double)xv.y * (double)xv.y : 0.0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) pd += __shfl_xor(pd, o, 64);
        if (lane == c) acc_c += pd;
      } else {
        const bool fresh = !seen && __shfl(added_c, c, 64) == 0;
        const bool first = fresh && lane == __ffsll((long long)tm) - 1;
        float a[1] = {train ? (first ? 0.f : alpha) : 1.f};
        float b[1] = {train ? (first ? p : al.b[c] * p) : 0.f};
        affine_scan<1>(a, b);
        e_d = affine_apply(a[0], b[0], carry);
        const int last = (T - t0) >= 64 ? 63 : (int)(T - t0) - 1;   // carry = state after the last valid frame of the chunk
        const double nc = __shfl(e_d, last, 64);
        if (lane == c) est_c = nc;
      }
    }
    float2 term = xv;
    if (f & BTK_SS_SUBTRACT) term = ss_term(xv, p, (float)e_d, ft, floorv);
    ss_accumulate(ysum, term);
    if (++c == C) {
      if (ok) btk_st<true>(y + t, ss_mean(ysum, invC));
      c = 0;
      t0 += 64;
      seen = seen || tm != 0ull;
    }
  }
  if (lane < C) { est[sidx] = est_c; acc[sidx] = acc_c; }
}

// VEC frames per lane: 8- or 16-byte accesses.  The arithmetic per frame is the same expression either way (same bits).
template <int VEC> struct ss_vec;
template <> struct ss_vec<1> { typedef float2 type; };
template <> struct ss_vec<2> { typedef float4 type; };

template <int VEC>
__device__ __forceinline__ void ss_frames_body(const float2* __restrict__ x, float2* __restrict__ y, const double* __restrict__ e,
                                               int K, int C, long T_stride, bool sub, float ft, float floorv)
{
  typedef typename ss_vec<VEC>::type vec_t;
  const float invC = 1.0f / (float)C;
  float2 ysum[VEC];
#pragma unroll
  for (int i = 0; i < VEC; i++) ysum[i] = make_float2(0.f, 0.f);
  auto step = [&](int c, vec_t v) {
    float2 xv[VEC];
    xv[0] = make_float2(v.x, v.y);
    if constexpr (VEC == 2) xv[1] = make_float2(v.z, v.w);
    const float est = sub ? (float)e[(long)c * K] : 0.f;        // wave-uniform: a scalar load
#pragma unroll
    for (int i = 0; i < VEC; i++) {
      float2 term = xv[i];
      if (sub) term = ss_term(xv[i], ss_pow(xv[i]), est, ft, floorv);
      ss_accumulate(ysum[i], term);
    }
  };
  int c = 0;
  for (; c + SS_UNROLL <= C; c += SS_UNROLL) {
    vec_t v[SS_UNROLL];
#pragma unroll
    for (int u = 0; u < SS_UNROLL; u++) v[u] = btk_ld<true>(reinterpret_cast<const vec_t*>(x + (long)(c + u) * T_stride));
#pragma unroll
    for (int u = 0; u < SS_UNROLL; u++) step(c + u, v[u]);
  }
  for (; c < C; c++) step(c, btk_ld<true>(reinterpret_cast<const vec_t*>(x + (long)c * T_stride)));
  if constexpr (VEC == 2)
  {
    const float2 y0 = ss_mean(ysum[0], invC), y1 = ss_mean(ysum[1], invC);
    btk_st<true>(reinterpret_cast<float4*>(y), make_float4(y0.x, y0.y, y1.x, y1.y));
  } else
    btk_st<true>(y, ss_mean(ysum[0], invC));
}

// VEC = 2 needs rows that start on 16 bytes (the host checks base pointers and an even T_stride); a row's odd last frame
// takes the 8-byte body.
template <int VEC>
__global__ __launch_bounds__(SS_NT)
void ss_frames_kernel(const float2* __restrict__ X, float2* __restrict__ Y, int K, int C, long T_stride, long T,
                      int mode, float ft, float floorv, const double* __restrict__ est)
{
  const int k = blockIdx.y, s = blockIdx.z;
  const long t = ((long)blockIdx.x * SS_NT + threadIdx.x) * VEC;
  if (t >= T) return;
  const float2* x = X + ((long)s * K + k) * C * T_stride + t;
  float2* y = Y + ((long)s * K + k) * T_stride + t;
  const double* e = est + (long)s * C * K + k;
  const bool sub = (mode & BTK_SS_SUBTRACT) != 0;
  if (VEC == 2 && t + 1 < T) ss_frames_body<2>(x, y, e, K, C, T_stride, sub, ft, floorv);
  else ss_frames_body<1>(x, y, e, K, C, T_stride, sub, ft, floorv);
}

// count (averaging channels) and added (recursive channels) of all S x C estimators after a block, one lane per estimator across
// a grid.  The number of training frames is the same for every estimator: with a flag stream every wavefront counts it for
// itself (T bytes from cache, 64 per step) rather than one wavefront for all.
__global__ __launch_bounds__(SS_NT)
void ss_count_kernel(const unsigned char* __restrict__ flags, long T, long ntrain_const, int SC, int C, ss_alpha_t al,
                     long long* __restrict__ count, unsigned char* __restrict__ added)
{
  const int lane = threadIdx.x & 63;
  long n = ntrain_const;
  if (flags) {
    n = 0;
    for (long t0 = 0; t0 < T; t0 += 64) {
      const long t = t0 + lane;
      n += __popcll(__ballot(t < T && (flags[t] & BTK_SS_TRAIN)));
    }
  }
  const int i = blockIdx.x * SS_NT + threadIdx.x;
  if (i >= SC) return;
  if (al.a[i % C] < 0.f) count[i] += n;
  else if (n > 0) added[i] = 1;
}

__global__ __launch_bounds__(SS_NT)
void ss_finish_training_kernel(long total, int K, int C, ss_alpha_t al, double* __restrict__ est, const double* __restrict__ acc,
                               const long long* __restrict__ count)
{
  const long i = (long)blockIdx.x * SS_NT + threadIdx.x;
  if (i >= total) return;
  const long sc = i / K;
  if (al.a[sc % C] < 0.f) est[i] = acc[i] * (1.0 / (double)(float)count[sc]);     // 1.0/(float)sampleN, :84
}

template <bool HAS_FLAGS, bool HAS_NOISE>
__global__ __launch_bounds__(64)
void wiener_rows_kernel(const float2* __restrict__ Sx, const float2* __restrict__ Nx, float2* __restrict__ Y, int K,
                        long T_stride, long T, const unsigned char* __restrict__ flags, int mode, float alpha, float omalpha,
                        float floorv, float beta, long frame_base, double* __restrict__ psd_s, double* __restrict__ psd_n)
{
  const int k = blockIdx.x, s = blockIdx.y;
  const int lane = threadIdx.x;
  const long row = (long)s * K + k;
  const float2* sx = Sx + row * T_stride;
  float2* y = Y + row * T_stride;
  if (k == 0) {                                                 // bin 0: the target's, no state (:329)
    for (long t = lane; t < T; t += 64) btk_st<true>(y + t, btk_ld<true>(sx + t));
    return;
  }
  const float2* nx = HAS_NOISE ? Nx + row * T_stride : nullptr;
  double cs = psd_s[row], cn = psd_n[row];
  const long ph = frame_base & 63;
  // raw values from clamped frame indices, selected where they are used (see ss_rows_kernel)
  float2 sn = btk_ld<true>(sx + ss_clamp(lane - ph, T));
  float2 nn = HAS_NOISE ? btk_ld<true>(nx + ss_clamp(lane - ph, T)) : make_float2(0.f, 0.f);
  int fn = HAS_FLAGS ? (int)flags[ss_clamp(lane - ph, T)] : mode;
  for (long t0 = -ph; t0 < T; t0 += 64) {
    const long t = t0 + lane;
    const bool ok = t >= 0 && t < T;
    const float2 sv = ok ? sn : make_float2(0.f, 0.f), nv = nn;
    const int f = ok ? fn : 0;
    {                                                           // the next chunk's loads go out before this one is scanned
      const long tn = ss_clamp(t + 64, T);
      sn = btk_ld<true>(sx + tn);
      if (HAS_NOISE) nn = btk_ld<true>(nx + tn);
      if (HAS_FLAGS) fn = (int)flags[tn];
    }
    const long g = frame_base + t;                              // frame_no_ before the increment = g - 1
    const float a0 = g >= 2 ? alpha : 0.f, b0 = g >= 2 ? omalpha : 1.f;
    const bool upd = (f & BTK_WIENER_UPDATE_NOISE) != 0;        // f = 0 on lanes outside the block
    float pn = ss_pow(nv);
    pn = (pn < floorv) ? floorv : pn;                           // :338-339
    float a[2] = {ok ? a0 : 1.f, upd ? a0 : 1.f};
    float b[2] = {ok ? b0 * ss_pow(sv) : 0.f, upd ? b0 * pn : 0.f};
    affine_scan<2>(a, b);
    const double ps_d = affine_apply(a[0], b[0], cs), pn_d = affine_apply(a[1], b[1], cn);
    if (ok) {
      const float ps = (float)ps_d;
      const float H = ps / fmaf(beta, (float)pn_d, ps);
      btk_st<true>(y + t, make_float2(H * sv.x, H * sv.y));
    }
    const int last = (T - t0) >= 64 ? 63 : (int)(T - t0) - 1;
    cs = __shfl(ps_d, last, 64);
    cn = __shfl(pn_d, last, 64);
  }
  if (lane == 0) { psd_s[row] = cs; psd_n[row] = cn; }
}

// (no __restrict__: X == Y is allowed)
__global__ __launch_bounds__(SS_NT)
void spec_highpass_kernel(const float2* X, float2* Y, int K, int cutoff, long T_stride, long T)
{
  const int k = blockIdx.y, s = blockIdx.z;
  const long t = (long)blockIdx.x * SS_NT + threadIdx.x;
  if (t >= T) return;
  const long o = ((long)s * K + k) * T_stride + t;
  btk_st<true>(Y + o, k < cutoff ? make_float2(0.f, 0.f) : btk_ld<true>(X + o));
}

int ss_check(const char* who, int S, int M, int C, long T_stride, long T)
{
  if (M < 2 || M > 2048 || (M & 1)) return btk_set_error(BTK_ERR_DIMENSION, "%s: M=%d must be even and in 2 .. 2048", who, M);
  if (C < 1 || C > SS_MAXC) return btk_set_error(BTK_ERR_DIMENSION, "%s: %d channels, 1 .. %d are supported", who, C, SS_MAXC);
  if (S < 1 || S > 65535 || T < 0 || T_stride < T)
    return btk_set_error(BTK_ERR_DIMENSION, "%s: bad sizes S=%d T=%ld T_stride=%ld", who, S, T, T_stride);
  return BTK_OK;
}

ss_alpha_t ss_alphas(const double* alpha, int C)
{
  ss_alpha_t al;
  for (int c = 0; c < SS_MAXC; c++) {
    const double a = c < C ? alpha[c] : 0.0;
    al.a[c] = a < 0.0 ? -1.f : (float)a;
    al.b[c] = a < 0.0 ? 0.f : (float)(1.0 - a);
  }
  return al;
}

}  // namespace

extern "C" {

int btk_ss_max_channels(void) { return SS_MAXC; }

int btk_ss_process(const void* X, void* Y, int S, int M, int C, long T_stride, long T, const unsigned char* flags, int mode,
                   double ft, double flooringV, const double* alpha, long frames_done, double* est, double* acc,
                   long long* count, unsigned char* added, int form, void* stream)
{
  const int rc = ss_check("btk_ss_process", S, M, C, T_stride, T);
  if (rc != BTK_OK) return rc;
  if (!X || !Y || !alpha || !est || !acc || !count || !added)
    return btk_set_error(BTK_ERR_PARAMETER, "btk_ss_process: null argument");
  if ((mode & ~(BTK_SS_TRAIN | BTK_SS_SUBTRACT)) || (form != BTK_SS_FORM_AUTO && form != BTK_SS_FORM_ROWS))
    return btk_set_error(BTK_ERR_PARAMETER, "btk_ss_process: unknown mode %d or form %d", mode, form);
  if (frames_done < 0) return btk_set_error(BTK_ERR_PARAMETER, "btk_ss_process: frames_done=%ld", frames_done);
  if (T == 0) return BTK_OK;
  const int K = M / 2 + 1;
  const bool may_train = flags != nullptr || (mode & BTK_SS_TRAIN);
  if (!may_train && form == BTK_SS_FORM_AUTO) {
    // two frames per lane in 16-byte accesses where every row starts on 16 bytes
    const bool wide = !(T_stride & 1) && !(reinterpret_cast<uintptr_t>(X) & 15) && !(reinterpret_cast<uintptr_t>(Y) & 15);
    const long per_block = (long)SS_NT * (wide ? 2 : 1);
    hipLaunchKernelGGL(wide ? ss_frames_kernel<2> : ss_frames_kernel<1>,
                       dim3((unsigned)((T + per_block - 1) / per_block), (unsigned)K, (unsigned)S), dim3(SS_NT), 0,
                       as_stream(stream), static_cast<const float2*>(X), static_cast<float2*>(Y), K, C, T_stride, T, mode,
                       (float)ft, (float)flooringV, est);
    BTK_HIP_CHECK(hipGetLastError());
    return BTK_OK;
  }
  const ss_alpha_t al = ss_alphas(alpha, C);
  hipLaunchKernelGGL(flags ? ss_rows_kernel<true> : ss_rows_kernel<false>, dim3((unsigned)K, (unsigned)S), dim3(64), 0,
                     as_stream(stream), static_cast<const float2*>(X), static_cast<float2*>(Y), K, C, T_stride, T, flags, mode,
                     (float)ft, (float)flooringV, al, frames_done, est, acc, added);
  BTK_HIP_CHECK(hipGetLastError());
  if (may_train) {
    hipLaunchKernelGGL(ss_count_kernel, dim3((unsigned)((S * C + SS_NT - 1) / SS_NT)), dim3(SS_NT), 0, as_stream(stream), flags, T, (mode & BTK_SS_TRAIN) ? T : 0L,
                       S * C, C, al, count, added);
    BTK_HIP_CHECK(hipGetLastError());
  }
  return BTK_OK;
}

int btk_ss_finish_training(int S, int M, int C, const double* alpha, double* est, const double* acc, const long long* count,
                           void* stream)
{
  const int rc = ss_check("btk_ss_finish_training", S, M, C, 0, 0);
  if (rc != BTK_OK) return rc;
  if (!alpha || !est || !acc || !count) return btk_set_error(BTK_ERR_PARAMETER, "btk_ss_finish_training: null argument");
  const int K = M / 2 + 1;
  const long total = (long)S * C * K;
  hipLaunchKernelGGL(ss_finish_training_kernel, dim3((unsigned)((total + SS_NT - 1) / SS_NT)), dim3(SS_NT), 0, as_stream(stream),
                     total, K, C, ss_alphas(alpha, C), est, acc, count);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

int btk_ss_clear(int S, int M, int C, int what, double* acc, long long* count, unsigned char* added, void* stream)
{
  const int rc = ss_check("btk_ss_clear", S, M, C, 0, 0);
  if (rc != BTK_OK) return rc;
  if (!acc || !count || !added) return btk_set_error(BTK_ERR_PARAMETER, "btk_ss_clear: null argument");
  if (what != 0 && what != 1) return btk_set_error(BTK_ERR_PARAMETER, "btk_ss_clear: what=%d", what);
  const long sc = (long)S * C;
  BTK_HIP_CHECK(hipMemsetAsync(acc, 0, sizeof(double) * sc * (M / 2 + 1), as_stream(stream)));
  BTK_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(long long) * sc, as_stream(stream)));
  if (what == 1) BTK_HIP_CHECK(hipMemsetAsync(added, 0, sc, as_stream(stream)));
  return BTK_OK;
}

int btk_wiener_process(const void* Sx, const void* Nx, void* Y, int S, int M, long T_stride, long T, const unsigned char* flags,
                       int mode, double alpha, double flooringV, double beta, long frames_done, double* psd_s, double* psd_n,
                       void* stream)
{
  const int rc = ss_check("btk_wiener_process", S, M, 1, T_stride, T);
  if (rc != BTK_OK) return rc;
  if (!Sx || !Y || !psd_s || !psd_n) return btk_set_error(BTK_ERR_PARAMETER, "btk_wiener_process: null argument");
  if (mode & ~BTK_WIENER_UPDATE_NOISE) return btk_set_error(BTK_ERR_PARAMETER, "btk_wiener_process: unknown mode %d", mode);
  if (!Nx && (flags || (mode & BTK_WIENER_UPDATE_NOISE)))
    return btk_set_error(BTK_ERR_PARAMETER, "btk_wiener_process: the noise PSD may be updated but Nx is null");
  if (frames_done < 0) return btk_set_error(BTK_ERR_PARAMETER, "btk_wiener_process: frames_done=%ld", frames_done);
  if (T == 0) return BTK_OK;
  const int K = M / 2 + 1;
  auto kernel = flags ? wiener_rows_kernel<true, true> : (Nx ? wiener_rows_kernel<false, true> : wiener_rows_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)K, (unsigned)S), dim3(64), 0, as_stream(stream),
                     static_cast<const float2*>(Sx), static_cast<const float2*>(Nx), static_cast<float2*>(Y), K, T_stride, T,
                     flags, mode, (float)alpha, (float)(1.0 - alpha), (float)flooringV, (float)beta, frames_done, psd_s, psd_n);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

int btk_spec_highpass(const void* X, void* Y, int S, int M, int cutoff, long T_stride, long T, void* stream)
{
  const int rc = ss_check("btk_spec_highpass", S, M, 1, T_stride, T);
  if (rc != BTK_OK) return rc;
  if (!X || !Y) return btk_set_error(BTK_ERR_PARAMETER, "btk_spec_highpass: null argument");
  const int K = M / 2 + 1;
  if (cutoff < 0 || cutoff > K) return btk_set_error(BTK_ERR_DIMENSION, "btk_spec_highpass: cutoff bin %d outside 0 .. %d", cutoff, K);
  if (T == 0) return BTK_OK;
  hipLaunchKernelGGL(spec_highpass_kernel, dim3((unsigned)((T + SS_NT - 1) / SS_NT), (unsigned)K, (unsigned)S), dim3(SS_NT), 0,
                     as_stream(stream), static_cast<const float2*>(X), static_cast<float2*>(Y), K, cutoff, T_stride, T);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

}  // extern "C"
