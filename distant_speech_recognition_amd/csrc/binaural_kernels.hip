// binaural_kernels.hip -- binaural binary-mask filters and their threshold estimators for gfx950.
//
// Replaces KimBinaryMaskFilter::masking1 / IIDBinaryMaskFilter::masking1 (reference postfilter/binauralprocessing.cc:138-179,
// :441-485, with calcITDf :17-38), the three accumStats1 (:314-353, :548-603, :794-838), the candidate walk they share
// (`for(float threshold=min;threshold<=max;threshold+=width)`) and the three calc_threshold (:382-407, :632-660, :867-898).
// Layouts, state and limits: include/btkhip.h.
//
//   1. bn_mask_kernel    : one wavefront per (stream, bin) row.  The mask obeys mu_t = alpha mu_{t-1} + (1 - alpha) b_t with
//                          b_t in {1, eta} decided per cell: a first-order affine recursion, scanned in the DPP network in 64-frame
//                          chunks that sit on multiples of 64 of the stream's frame counter (the scan of ss_kernels.hip with a
//                          constant multiplier).  The carry from chunk to chunk is the float32 mask itself -- what prevMu holds --,
//                          so a block cut at a multiple of 64 continues with the very number an uncut launch carries.
//   2. bn_stats_kernel   : Kim / IID sums.  One workgroup per (chunk of frames, stream); per frame the per-bin decision variable
//                          and the powers go to LDS once, lanes run over candidates and read the bins in order (every lane the
//                          same address: a broadcast).  Each lane owns its candidates' partial sums of the chunk.
//   3. bn_reduce_kernel  : partials of the chunks added in chunk order to the float64 state; no floating-point atomics anywhere.
//   4. bn_fdiid_kernel   : FD-IID sums, one workgroup per (stream, bin): a tile of frames' terms to LDS (one frame per lane,
//                          coalesced), then lanes run over candidates with the frames in order.
// Decisions (phases, magnitudes, comparisons) and every sum the reference keeps in double are float64; only the mask recursion
// and the masked output are float32, as prevMu_ and this project's subband samples are.
#include "btk_internal.h"
#include "wave_ops.h"
#include <cmath>
#include <cstdint>

namespace {

constexpr int BN_NT = 256;
constexpr int BN_MAXCAND = 4096;
constexpr int BN_MAXCHUNKS = 512;
constexpr int BN_MINFR = 4;

// one step of the inclusive scan (affine_scan_schedule, wave_ops.h) of affine maps v -> a v + b; lanes without a source keep the identity (1, 0); a = 0 forgets
// its past (see ss_kernels.hip)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void affine_scan_step(float& a, float& b)
{
  const float a2 = dpp_or<CTRL, ROW_MASK>(1.f, a), p = dpp_or<CTRL, ROW_MASK>(0.f, b);
  b = (a == 0.f) ? b : fmaf(a, p, b);
  a *= a2;
}
__device__ __forceinline__ void affine_scan(float& a, float& b)
{
  affine_scan_schedule([&](auto ctrl, auto rows) { affine_scan_step<decltype(ctrl)::value, decltype(rows)::value>(a, b); });
}

__device__ __forceinline__ long bn_clamp(long t, long T) { return t < 0 ? 0 : (t >= T ? T - 1 : t); }

// gsl_complex_arg: 0 for z = 0 whatever the signs of its zeros
__device__ __forceinline__ double bn_arg(float2 z)
{
  return (z.x == 0.f && z.y == 0.f) ? 0.0 : atan2((double)z.y, (double)z.x);
}
// calcITDf (:17-38): the wrapped phase difference over 2 pi k / M; k = 0 divides by zero as there (inf or NaN)
__device__ __forceinline__ double bn_itd(float2 xl, float2 xr, int k, int M)
{
  const double d = bn_arg(xl) - bn_arg(xr);
  const double d1 = fabs(d), d2 = fabs(d - 2 * M_PI), d3 = fabs(d + 2 * M_PI);
  double pd = d1 < d2 ? d1 : d2;
  if (d3 < pd) pd = d3;
  return pd / (2 * M_PI * (double)k / (double)M);
}
// |z| of a float32 pair in float64: the squares are exact, one rounding in the sum, one in the root
__device__ __forceinline__ double bn_abs(double re, double im) { return sqrt(re * re + im * im); }

template <int KIND>
__global__ __launch_bounds__(64)
void bn_mask_kernel(const float2* __restrict__ XL, const float2* __restrict__ XR, float2* __restrict__ Y, int K, int M,
                    long T_stride, long T, int chanX, float threshold, const float* __restrict__ thresholds, float alpha, float om,
                    float ome, long frame_base, float* __restrict__ prev_mu)
{
  const int k = blockIdx.x, s = blockIdx.y;
  const int lane = threadIdx.x;
  const long row = (long)s * K + k;
  const float2* xl = XL + row * T_stride;
  const float2* xr = XR + row * T_stride;
  float2* y = Y + row * T_stride;
  if (k == 0) {                                                 // bin 0: the LEFT input's whatever chanX is, no state (:145, :448)
    for (long t = lane; t < T; t += 64) btk_st<true>(y + t, btk_ld<true>(xl + t));
    return;
  }
  const double thr = (double)((KIND == BTK_BINAURAL_IID && thresholds) ? thresholds[k] : threshold);
  float carry = prev_mu[row];
  const long ph = frame_base & 63;
  float2 ln = btk_ld<true>(xl + bn_clamp(lane - ph, T)), rn = btk_ld<true>(xr + bn_clamp(lane - ph, T));
  for (long t0 = -ph; t0 < T; t0 += 64) {
    const long t = t0 + lane;
    const bool ok = t >= 0 && t < T;
    const float2 lv = ln, rv = rn;
    {
      const long tn = bn_clamp(t + 64, T);
      ln = btk_ld<true>(xl + tn);
      rn = btk_ld<true>(xr + tn);
    }
    bool one;                                                   // b_t = 1 (else eta)
    if (KIND == BTK_BINAURAL_KIM) {
      const bool le = bn_itd(lv, rv, k, M) <= thr;
      one = chanX == 0 ? le : !le;
    } else {
      const float2 xt = chanX == 0 ? lv : rv, xi = chanX == 0 ? rv : lv;
      one = !(bn_abs(xt.x, xt.y) <= bn_abs(xi.x, xi.y) + thr);
    }
    float a = ok ? alpha : 1.f;
    float b = ok ? (one ? om : ome) : 0.f;
    affine_scan(a, b);
    const float mu = (a == 0.f) ? b : (float)fma((double)a, (double)carry, (double)b);
    if (ok) {
      const float2 x = chanX == 0 ? lv : rv;
      btk_st<true>(y + t, make_float2(__fmul_rn(x.x, mu), __fmul_rn(x.y, mu)));
    }
    const int last = (T - t0) >= 64 ? 63 : (int)(T - t0) - 1;
    carry = __shfl(mu, last, 64);
  }
  if (lane == 0) prev_mu[row] = carry;
}

// Kim: per bin  itd, |XL|^2, |eta XL|^2, |XR|^2, |eta XR|^2          (NL = 5), sums NV = 5, per-frame terms NPF = 2
// IID: per bin  |XL|, |XR|, |XL|^2pc, |eta XL|^2pc, |XR|^2pc, |eta XR|^2pc  (NL = 6), sums NV = 6, per-frame terms NPF = 6
template <int KIND> struct bn_dims;
template <> struct bn_dims<BTK_BINAURAL_KIM> { static constexpr int NL = 5, NV = 5, NPF = 2; };
template <> struct bn_dims<BTK_BINAURAL_IID> { static constexpr int NL = 6, NV = 6, NPF = 6; };

template <int KIND>
__global__ __launch_bounds__(BN_NT)
void bn_stats_kernel(const float2* __restrict__ XL, const float2* __restrict__ XR, int K, int M, long T_stride, long T, int FR,
                     const float* __restrict__ cands, int nWalk, int nCand, double eta, double pc, int k0, int k1,
                     double* __restrict__ part, double* __restrict__ per_frame)
{
  constexpr int NV = bn_dims<KIND>::NV, NPF = bn_dims<KIND>::NPF;
  extern __shared__ double bn_lds[];
  const int chunk = blockIdx.x, nChunks = gridDim.x, s = blockIdx.y, tid = threadIdx.x;
  const int nb = k1 - k0;
  const long tA = (long)chunk * FR, tB = (tA + FR < T) ? tA + FR : T;
  double* out = part + ((long)s * nChunks + chunk) * nCand * NV;
  // a lane zeroes what it alone sums into below; slots the walk never reaches stay 0
  for (int c = tid; c < nCand; c += BN_NT) {
#pragma unroll
    for (int j = 0; j < NV; j++) out[c * NV + j] = 0.0;
  }
  for (long t = tA; t < tB; t++) {
    __syncthreads();                                            // the previous frame's bins have been read
    for (int i = tid; i < nb; i += BN_NT) {
      const int k = k0 + i;
      const long o = ((long)s * K + k) * T_stride + t;
      const float2 l = XL[o], r = XR[o];
      const double lx = l.x, ly = l.y, rx = r.x, ry = r.y;
      if (KIND == BTK_BINAURAL_KIM) {
        bn_lds[i] = bn_itd(l, r, k, M);
        bn_lds[nb + i] = lx * lx + ly * ly;
        bn_lds[2 * nb + i] = (lx * eta) * (lx * eta) + (ly * eta) * (ly * eta);
        bn_lds[3 * nb + i] = rx * rx + ry * ry;
        bn_lds[4 * nb + i] = (rx * eta) * (rx * eta) + (ry * eta) * (ry * eta);
      } else {
        const double pl = bn_abs(lx, ly), pr = bn_abs(rx, ry);
        bn_lds[i] = pl;
        bn_lds[nb + i] = pr;
        bn_lds[2 * nb + i] = pow(pl, 2.0 * pc);
        bn_lds[3 * nb + i] = pow(bn_abs(lx * eta, ly * eta), 2.0 * pc);
        bn_lds[4 * nb + i] = pow(pr, 2.0 * pc);
        bn_lds[5 * nb + i] = pow(bn_abs(rx * eta, ry * eta), 2.0 * pc);
      }
    }
    __syncthreads();
    for (int c = tid; c < nWalk; c += BN_NT) {
      const double thr = (double)cands[c];
      double v[NV], pf[NPF];
      if (KIND == BTK_BINAURAL_KIM) {
        double PT = 0.0, PI = 0.0;
        for (int i = 0; i < nb; i++) {
          const bool le = bn_lds[i] <= thr;
          PT += le ? bn_lds[nb + i] : bn_lds[2 * nb + i];
          PI += le ? bn_lds[4 * nb + i] : bn_lds[3 * nb + i];
        }
        const double RT = pow(PT, pc), RI = pow(PI, pc);
        pf[0] = RT; pf[1] = RI;
        v[0] = RT * RI; v[1] = RT; v[2] = RI; v[3] = RT * RT; v[4] = RI * RI;
      } else {
        double y1t = 0.0, y2t = 0.0, y4t = 0.0, y1i = 0.0, y2i = 0.0, y4i = 0.0;
        for (int i = 0; i < nb; i++) {
          const double pl = bn_lds[i], pr = bn_lds[nb + i];
          const double a = (pl <= pr + thr) ? bn_lds[3 * nb + i] : bn_lds[2 * nb + i];
          const double b = (pr <= pl + thr) ? bn_lds[5 * nb + i] : bn_lds[4 * nb + i];
          const double a2 = a * a, b2 = b * b;
          y1t += a; y2t += a2; y4t += a2 * a2;
          y1i += b; y2i += b2; y4i += b2 * b2;
        }
        v[0] = y1t; v[1] = y2t; v[2] = y4t; v[3] = y1i; v[4] = y2i; v[5] = y4i;
#pragma unroll
        for (int j = 0; j < NPF; j++) pf[j] = v[j];
      }
      if (per_frame) {
        double* q = per_frame + (((long)s * T + t) * nCand + c) * NPF;
#pragma unroll
        for (int j = 0; j < NPF; j++) q[j] = pf[j];
      }
#pragma unroll
      for (int j = 0; j < NV; j++) out[c * NV + j] += v[j];   // this lane alone touches candidate c of this chunk
    }
  }
}

__global__ __launch_bounds__(BN_NT)
void bn_reduce_kernel(const double* __restrict__ part, int nChunks, int n /* nCand NV */, long T, double* __restrict__ state,
                      long long* __restrict__ count)
{
  const int i = blockIdx.x * BN_NT + threadIdx.x, s = blockIdx.y;
  if (i == 0) count[s] += T;
  if (i >= n) return;
  const double* p = part + (long)s * nChunks * n + i;
  double sum = 0.0;
  for (int c = 0; c < nChunks; c++) sum += p[(long)c * n];
  state[(long)s * n + i] += sum;
}

__global__ __launch_bounds__(BN_NT)
void bn_count_kernel(int S, long T, long long* __restrict__ count)
{
  const int s = blockIdx.x * BN_NT + threadIdx.x;
  if (s < S) count[s] += T;
}

__global__ __launch_bounds__(BN_NT)
void bn_fdiid_kernel(const float2* __restrict__ XL, const float2* __restrict__ XR, int K, long T_stride, long T,
                     const float* __restrict__ cands, int nWalk, int nCand, double eta, double pc, double* __restrict__ state)
{
  __shared__ double sh[6][BN_NT];
  const int k = blockIdx.x + 1, s = blockIdx.y, tid = threadIdx.x;
  const long row = (long)s * K + k;
  const float2* xl = XL + row * T_stride;
  const float2* xr = XR + row * T_stride;
  double* st = state + row * nCand * 3;
  for (long t0 = 0; t0 < T; t0 += BN_NT) {
    const int n = (T - t0) < BN_NT ? (int)(T - t0) : BN_NT;
    __syncthreads();
    if (tid < n) {
      const float2 l = xl[t0 + tid], r = xr[t0 + tid];
      const double lx = l.x, ly = l.y, rx = r.x, ry = r.y;
      const double pl = bn_abs(lx, ly), pr = bn_abs(rx, ry);
      sh[0][tid] = pl;
      sh[1][tid] = pr;
      sh[2][tid] = pow(pl, 2.0 * pc);
      sh[3][tid] = pow(bn_abs(lx * eta, ly * eta), 2.0 * pc);
      sh[4][tid] = pow(pr, 2.0 * pc);
      sh[5][tid] = pow(bn_abs(rx * eta, ry * eta), 2.0 * pc);
    }
    __syncthreads();
    for (int c = tid; c < nWalk; c += BN_NT) {
      const double thr = (double)cands[c];
      double y4 = st[c * 3], mean = st[c * 3 + 1], sigma = st[c * 3 + 2];
      for (int i = 0; i < n; i++) {
        const double pl = sh[0][i], pr = sh[1][i];
        const double a = (pl <= pr + thr) ? sh[3][i] : sh[2][i];
        const double b = (pr <= pl + thr) ? sh[5][i] : sh[4][i];
        const double a2 = a * a, b2 = b * b;
        y4 += a2 * a2 + b2 * b2;
        mean += a + b;
        sigma += a2 + b2;
      }
      st[c * 3] = y4; st[c * 3 + 1] = mean; st[c * 3 + 2] = sigma;
    }
  }
}

int bn_check(const char* who, int S, int M, long T_stride, long T)
{
  if (M < 2 || M > 2048 || (M & 1)) return btk_set_error(BTK_ERR_DIMENSION, "%s: M=%d must be even and in 2 .. 2048", who, M);
  if (S < 1 || S > 65535 || T < 0 || T_stride < T)
    return btk_set_error(BTK_ERR_DIMENSION, "%s: bad sizes S=%d T=%ld T_stride=%ld", who, S, T, T_stride);
  return BTK_OK;
}

int bn_chunks(long T, int* FR)
{
  // chunks of at least BN_MINFR frames, at most BN_MAXCHUNKS of them: a function of T alone (T >= 1)
  long n = (T + BN_MINFR - 1) / BN_MINFR;
  if (n > BN_MAXCHUNKS) n = BN_MAXCHUNKS;
  const long fr = (T + n - 1) / n;
  *FR = (int)fr;
  return (int)((T + fr - 1) / fr);
}

int bn_nv(int kind) { return kind == BTK_BINAURAL_KIM ? 5 : (kind == BTK_BINAURAL_IID ? 6 : 3); }

}  // namespace

extern "C" {

int btk_binaural_max_candidates(void) { return BN_MAXCAND; }

int btk_binaural_mask(const void* XL, const void* XR, void* Y, int S, int M, long T_stride, long T, int kind, int chanX,
                      double threshold, const float* thresholds, double alpha, double eta, long frames_done, float* prev_mu,
                      void* stream)
{
  const int rc = bn_check("btk_binaural_mask", S, M, T_stride, T);
  if (rc != BTK_OK) return rc;
  if (!XL || !XR || !Y || !prev_mu) return btk_set_error(BTK_ERR_PARAMETER, "btk_binaural_mask: null argument");
  if ((kind != BTK_BINAURAL_KIM && kind != BTK_BINAURAL_IID) || (chanX != 0 && chanX != 1))
    return btk_set_error(BTK_ERR_PARAMETER, "btk_binaural_mask: kind=%d chanX=%d", kind, chanX);
  if (frames_done < 0) return btk_set_error(BTK_ERR_PARAMETER, "btk_binaural_mask: frames_done=%ld", frames_done);
  if (T == 0) return BTK_OK;
  const int K = M / 2 + 1;
  // alpha_, dEta_ and threshold_ are float members; (1 - alpha_) and (1 - alpha_) dEta_ are float expressions (:155-157)
  const float af = (float)alpha, ef = (float)eta, om = 1.f - af, ome = om * ef;
  hipLaunchKernelGGL(kind == BTK_BINAURAL_KIM ? bn_mask_kernel<BTK_BINAURAL_KIM> : bn_mask_kernel<BTK_BINAURAL_IID>,
                     dim3((unsigned)K, (unsigned)S), dim3(64), 0, as_stream(stream), static_cast<const float2*>(XL),
                     static_cast<const float2*>(XR), static_cast<float2*>(Y), K, M, T_stride, T, chanX, (float)threshold,
                     thresholds, af, om, ome, frames_done, prev_mu);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

long btk_binaural_stats_scratch_bytes(int kind, int S, long T, int nCand)
{
  if (kind != BTK_BINAURAL_KIM && kind != BTK_BINAURAL_IID) return 0;
  if (S < 1 || T < 1 || nCand < 1) return 0;
  int FR;
  return (long)sizeof(double) * S * bn_chunks(T, &FR) * nCand * bn_nv(kind);
}

int btk_binaural_stats(const void* XL, const void* XR, int S, int M, long T_stride, long T, int kind, const float* cands,
                       int nWalk, int nCand, double eta, double power_coeff, int fbin_min, int fbin_max, double* state,
                       long long* count, double* per_frame, void* scratch, long scratch_bytes, void* stream)
{
  const int rc = bn_check("btk_binaural_stats", S, M, T_stride, T);
  if (rc != BTK_OK) return rc;
  const int K = M / 2 + 1;
  if (nCand < 1 || nCand > BN_MAXCAND || nWalk < 0 || nWalk > nCand)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_binaural_stats: %d candidates walked, %d slots (1 .. %d)", nWalk, nCand, BN_MAXCAND);
  if (kind != BTK_BINAURAL_KIM && kind != BTK_BINAURAL_IID && kind != BTK_BINAURAL_FDIID)
    return btk_set_error(BTK_ERR_PARAMETER, "btk_binaural_stats: kind=%d", kind);
  if (kind != BTK_BINAURAL_FDIID && (fbin_min < 0 || fbin_max > K || fbin_min > fbin_max))
    return btk_set_error(BTK_ERR_DIMENSION, "btk_binaural_stats: bins [%d, %d) outside 0 .. %d", fbin_min, fbin_max, K);
  if (!XL || !XR || !cands || !state || !count) return btk_set_error(BTK_ERR_PARAMETER, "btk_binaural_stats: null argument");
  if (T == 0) return BTK_OK;
  const float ef = (float)eta, pf = (float)power_coeff;          // dEta_, dpower_coeff_ are float members
  const float2* xl = static_cast<const float2*>(XL);
  const float2* xr = static_cast<const float2*>(XR);
  if (kind == BTK_BINAURAL_FDIID) {
    if (per_frame) return btk_set_error(BTK_ERR_PARAMETER, "btk_binaural_stats: no per-frame terms for FD-IID");
    hipLaunchKernelGGL(bn_fdiid_kernel, dim3((unsigned)(K - 1), (unsigned)S), dim3(BN_NT), 0, as_stream(stream), xl, xr, K,
                       T_stride, T, cands, nWalk, nCand, (double)ef, (double)pf, state);
    BTK_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(bn_count_kernel, dim3((unsigned)((S + BN_NT - 1) / BN_NT)), dim3(BN_NT), 0, as_stream(stream), S, T, count);
    BTK_HIP_CHECK(hipGetLastError());
    return BTK_OK;
  }
  const long need = btk_binaural_stats_scratch_bytes(kind, S, T, nCand);
  if (!scratch || scratch_bytes < need)
    return btk_set_error(BTK_ERR_PARAMETER, "btk_binaural_stats: scratch of %ld bytes, %ld needed", scratch_bytes, need);
  int FR;
  const int nChunks = bn_chunks(T, &FR);
  const int nb = fbin_max - fbin_min;
  const int NL = kind == BTK_BINAURAL_KIM ? bn_dims<BTK_BINAURAL_KIM>::NL : bn_dims<BTK_BINAURAL_IID>::NL, NV = bn_nv(kind);
  const size_t lds = sizeof(double) * NL * (nb > 0 ? nb : 1);   // <= 6 x 1025 x 8 = 49200 bytes
  hipLaunchKernelGGL(kind == BTK_BINAURAL_KIM ? bn_stats_kernel<BTK_BINAURAL_KIM> : bn_stats_kernel<BTK_BINAURAL_IID>,
                     dim3((unsigned)nChunks, (unsigned)S), dim3(BN_NT), lds, as_stream(stream), xl, xr, K, M, T_stride, T, FR,
                     cands, nWalk, nCand, (double)ef, (double)pf, fbin_min, fbin_max, static_cast<double*>(scratch), per_frame);
  BTK_HIP_CHECK(hipGetLastError());
  const int n = nCand * NV;
  hipLaunchKernelGGL(bn_reduce_kernel, dim3((unsigned)((n + BN_NT - 1) / BN_NT), (unsigned)S), dim3(BN_NT), 0, as_stream(stream),
                     static_cast<const double*>(scratch), nChunks, n, T, state, count);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

int btk_binaural_candidates(double min, double max, double width, float* out, int cap, int* nWalk, int* nCand)
{
  if (!nWalk || !nCand) return btk_set_error(BTK_ERR_PARAMETER, "btk_binaural_candidates: null argument");
  const float lo = (float)min, hi = (float)max, w = (float)width;
  if (!(w > 0.f) || !std::isfinite(lo) || !std::isfinite(hi) || !(lo <= hi))
    return btk_set_error(BTK_ERR_PARAMETER, "btk_binaural_candidates: range %g .. %g in steps of %g", min, max, width);
  const double slots = (double)((hi - lo) / w) + 1.5;           // (int)( (max_threshold_-min_threshold_)/width + 1.5 ), :270
  if (!(slots < (double)BN_MAXCAND + 1.0))
    return btk_set_error(BTK_ERR_DIMENSION, "btk_binaural_candidates: %g candidates, at most %d are supported", slots, BN_MAXCAND);
  const int n = (int)slots;
  int i = 0;
  // the walk, cut at n (stated deviation: the reference writes past its arrays there)
  for (float t = lo; t <= hi && i < n; t = (float)(t + w), i++)
    if (out && i < cap) out[i] = t;
  *nWalk = i;
  *nCand = n;
  if (out && cap < i) return btk_set_error(BTK_ERR_DIMENSION, "btk_binaural_candidates: room for %d of %d candidates", cap, i);
  return BTK_OK;
}

int btk_binaural_threshold(int kind, int M, int nCand, int nWalk, const float* cands, const double* state, long long count,
                           double beta, double* threshold, double* cost, double* thresholds)
{
  if (M < 2 || M > 2048 || (M & 1)) return btk_set_error(BTK_ERR_DIMENSION, "btk_binaural_threshold: M=%d", M);
  if (nCand < 1 || nCand > BN_MAXCAND || nWalk < 0 || nWalk > nCand)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_binaural_threshold: %d candidates walked, %d slots", nWalk, nCand);
  if (!cands || !state || !threshold || !cost) return btk_set_error(BTK_ERR_PARAMETER, "btk_binaural_threshold: null argument");
  const double n = (double)(unsigned int)count;                  // nSamples_ is unsigned int; 0 divides by zero as there
  if (kind == BTK_BINAURAL_KIM) {
    float arg = nWalk > 0 ? cands[0] : 0.f;
    double min_rho = 1000000;
    for (int i = 0; i < nCand; i++) cost[i] = 0.0;
    for (int i = 0; i < nWalk; i++) {
      const double* v = state + (long)i * 5;
      const double mt = v[1] / n, mi = v[2] / n;
      const double st = v[3] / n - mt * mt, si = v[4] / n - mi * mi;
      cost[i] = v[0] / n;
      const double rho = fabs((cost[i] - mt * mi) / (sqrt(st) * sqrt(si)));
      if (rho < min_rho) { arg = cands[i]; min_rho = rho; }
    }
    *threshold = (double)arg;
    return BTK_OK;
  }
  if (kind == BTK_BINAURAL_IID) {
    float arg = nWalk > 0 ? cands[0] : 0.f;
    double min_rho = 1000000;
    for (int i = 0; i < nCand; i++) cost[i] = 0.0;
    for (int i = 0; i < nWalk; i++) {
      const double* v = state + (long)i * 6;
      const double sig2 = v[1] / n + v[4] / n;
      cost[i] = (v[2] / n + v[5] / n) - beta * sig2 * sig2;
      const double rho = -cost[i];
      if (rho < min_rho) { arg = cands[i]; min_rho = rho; }
    }
    *threshold = (double)arg;
    return BTK_OK;
  }
  if (kind == BTK_BINAURAL_FDIID) {
    if (!thresholds) return btk_set_error(BTK_ERR_PARAMETER, "btk_binaural_threshold: null argument");
    const int K = M / 2 + 1;
    float arg = 0.f;                                             // threshold_ as the constructor leaves it
    double min_rho = 1000000;
    for (long i = 0; i < (long)K * nCand; i++) cost[i] = 0.0;
    thresholds[0] = 0.0;                                         // never written in the reference
    for (int k = 1; k < K; k++) {
      double local = 1000000;
      thresholds[k] = 0.0;
      for (int i = 0; i < nWalk; i++) {
        const double* v = state + ((long)k * nCand + i) * 3;
        const double sigma = v[2] / n;
        const double cf = v[0] / n - beta * sigma * sigma;
        cost[(long)k * nCand + i] = cf;
        const double rho = -cf;
        if (rho <= min_rho) { arg = cands[i]; min_rho = rho; }
        if (rho <= local) { thresholds[k] = (double)cands[i]; local = rho; }
      }
    }
    *threshold = (double)arg;
    return BTK_OK;
  }
  return btk_set_error(BTK_ERR_PARAMETER, "btk_binaural_threshold: kind=%d", kind);
}

}  // extern "C"
