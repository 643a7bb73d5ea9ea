// Subband acoustic echo cancellation (gfx950), float64 recursion: the four canceller nodes of the reference's aec/aec.cc.
//
//   kind 0  NLMSAcousticEchoCancellationFeature::next            (aec/aec.cc:34-80)
//   kind 1  KalmanFilterEchoCancellationFeature::next            (aec/aec.cc:85-165)
//   kind 2  BlockKalmanFilterEchoCancellationFeature::next       (aec/aec.cc:172-307)
//   kind 3  DTDBlockKalmanFilterEchoCancellationFeature::next    (aec/aec.cc:801-942)
//
// V (played) and A (recorded) are complex64 [S][K][T_stride], K = M/2 + 1 (the analysis bank's output of one channel); the
// residual E = A - R^T v has the same layout.  All state is complex128 / float64 and caller-owned (include/btkhip.h).
//
// Played history.  ComplexBuffer_ (aec/aec.h:117-191) keeps the last P played frames, scaled by amp4play on entry, slot 0 the
// newest.  Inside a block the history of frame t IS the input row: v_t[i] = amp V[t-i] for i <= t; only the P frames before the
// block come from the state (hist[j] = v[j] of the previous block's last frame), which is rewritten once, at the end of a block.
//
// Mapping.
//   kinds 0, 1  one thread per (stream, bin), 64 bins per workgroup, V / A / E staged through LDS in 16-frame tiles.
//   kind 2      one (stream, bin) per group of 4 NP threads (NP = P rounded up to 4, 8, 16, 32, 64), the mapping of rls_kernels.hip:
//               thread (r, c) owns the row slice K[r][cW..cW+W) AND the column slice K[cW..cW+W)[r] (W = NP/4), so Kp conj(v) and
//               v^T Kp are W multiply-adds plus a DPP quad reduction each and the rank-one update is elementwise on both copies.
//               K is read and written in global memory once per block.
//   kind 3      the three scalars EkEnergy_, SkEnergy_, snr_ are shared by all bins of a stream and updated bin by bin, so a frame
//               of a stream is the unit: ONE workgroup per stream runs pass 1 (all residuals, one wavefront per bin), the ordered
//               walk over the bins (one lane, three first-order recurrences whose inputs pass 1 left in LDS), and pass 2 (the
//               Kalman update of every bin the walk did not skip, one wavefront per bin, lanes along the columns of K), with
//               two workgroup barriers per frame.  K lives in LDS for the block when (M/2+1) P^2 16 B fits, otherwise it is
//               updated in place in the exported state (L2-resident).  Workgroups never wait for each other.
#include "btk_internal.h"
#include "wave_ops.h"
#include <cstdint>

namespace {

constexpr int ATB = 16;                 // frames per LDS tile
constexpr int AEC_MAX_P = 64;
constexpr long AEC_FRAME_FROM_STATE = -(1L << 30);
constexpr int DTD_NT = 1024;            // kind 3: threads per stream
constexpr int DTD_NW = DTD_NT / 64;
constexpr size_t AEC_LDS_BUDGET = 160 * 1024 - 512;

struct AecParams {
  int kind;
  double beta, sigmau2, sigmak2, threshold, eng_threshold, smooth, amp;      // kind 0: beta = delta, sigmau2 = epsilon
  long frame_no0;
};

// played sample i frames before frame t of the block (i = 0: frame t itself), as it sits in ComplexBuffer_
__device__ __forceinline__ zd played(const float2* __restrict__ vrow, const zd* __restrict__ hist, int P, long T, double amp, long tf)
{
  if (tf >= T) return zmk(0.0, 0.0);
  if (tf >= 0) { const float2 f = vrow[tf]; return zmk(amp * (double)f.x, amp * (double)f.y); }
  const long j = -tf - 1;
  return j < P ? hist[j] : zmk(0.0, 0.0);
}

__global__ void aec_init_kernel(int kind, double sigv0, double k0, int K, int P, zd* __restrict__ R, zd* __restrict__ Kst,
                                double* __restrict__ sig, zd* __restrict__ hist, double* __restrict__ dtd)
{
  const long sk = (long)blockIdx.y * K + blockIdx.x;
  for (int e = threadIdx.x; e < P * P; e += blockDim.x) Kst[sk * P * P + e] = zmk((e / P == e % P) ? k0 : 0.0, 0.0);
  for (int e = threadIdx.x; e < P; e += blockDim.x) { R[sk * P + e] = zmk(0.0, 0.0); hist[sk * P + e] = zmk(0.0, 0.0); }
  if (threadIdx.x == 0) sig[sk] = sigv0;
  if (blockIdx.x == 0 && threadIdx.x < 4) dtd[4 * blockIdx.y + threadIdx.x] = 0.0;
}

__global__ void aec_count_kernel(double* __restrict__ dtd, int S, long T)
{
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < S) dtd[4 * s + 3] += (double)T;
}

// ---- kinds 0 and 1: scalar filters, one thread per (stream, bin)
__global__ __launch_bounds__(64)
void aec_scalar_kernel(const float2* __restrict__ V, const float2* __restrict__ A, float2* __restrict__ E,
                       unsigned char* __restrict__ flags, int K, long T_stride, long T, AecParams p,
                       zd* __restrict__ Rst, zd* __restrict__ Kst, double* __restrict__ sig)
{
  __shared__ float2 vt[64][ATB + 1], at[64][ATB + 1];
  __shared__ unsigned char ft[64][ATB + 4];
  const int tid = threadIdx.x, s = blockIdx.y, k0 = blockIdx.x * 64;
  const int k = k0 + tid;
  const bool kvalid = k < K;
  const long sk = (long)s * K + (kvalid ? k : K - 1);
  zd R = Rst[sk];
  double Kk = Kst[sk].x, sv = sig[sk];
  for (long t0 = 0; t0 < T; t0 += ATB) {
    for (int e = tid; e < 64 * ATB; e += 64) {
      const int b = e / ATB, f = e % ATB;
      const bool ok = k0 + b < K && t0 + f < T;
      const long off = ((long)s * K + k0 + b) * T_stride + t0 + f;
      vt[b][f] = ok ? V[off] : make_float2(0.f, 0.f);
      at[b][f] = ok ? A[off] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    const int nt = (T - t0 < ATB) ? (int)(T - t0) : ATB;
    for (int tt = 0; tt < nt; tt++) {
      const zd v = zmk((double)vt[tid][tt].x, (double)vt[tid][tt].y), a = zmk((double)at[tid][tt].x, (double)at[tid][tt].y);
      const zd e = zsub(a, zmul(R, v));
      const double v2 = zabs2(v);
      const bool adapt = v2 > p.threshold;                                   // update_ :34-39, :110-115
      if (adapt) {
        if (p.kind == 0) {
          const double inv = 1.0 / v2;
          const zd g = zscale(zmul(a, zconj(v)), inv);                       // A / V                                :64
          const zd dC = zsub(R, g);
          R = zsub(R, zscale(dC, p.sigmau2 * v2 / (p.beta + zabs2(a))));     // epsilon |V|^2 / (delta + |A|^2)      :69-71
        } else {
          sv = p.beta * sv + (1.0 - p.beta) * zabs2(e);                      // :143-145
          const double kp = Kk + p.sigmau2;                                  // :149
          const double ss = v2 * kp + sv;
          const zd g = zscale(zconj(v), kp / ss);
          R = zadd(R, zmul(g, e));                                           // :154
          Kk = (1.0 - kp * v2 / ss) * kp;                                    // :158
        }
      }
      vt[tid][tt] = make_float2((float)e.x, (float)e.y);
      ft[tid][tt] = adapt ? 1 : 0;
    }
    __syncthreads();
    for (int e = tid; e < 64 * ATB; e += 64) {
      const int b = e / ATB, f = e % ATB;
      if (k0 + b < K && t0 + f < T) {
        const long off = ((long)s * K + k0 + b) * T_stride + t0 + f;
        E[off] = vt[b][f];
        if (flags) flags[off] = ft[b][f];
      }
    }
    __syncthreads();
  }
  if (kvalid) { Rst[sk] = R; Kst[sk] = zmk(Kk, 0.0); sig[sk] = sv; }
}

// ---- kind 2: block Kalman filter, K in registers (row and column copies)
template <int NP>
__global__ __launch_bounds__((4 * NP < 64) ? 64 : 4 * NP)
void aec_block_kernel(const float2* __restrict__ V, const float2* __restrict__ A, float2* __restrict__ E,
                      unsigned char* __restrict__ flags, int K, int P, long T_stride, long T, AecParams p,
                      zd* __restrict__ Rst, zd* __restrict__ Kst, double* __restrict__ sig, zd* __restrict__ hist)
{
  constexpr int W = NP / 4;
  constexpr int TPB = 4 * NP;                              // threads per bin
  constexpr int NT = TPB < 64 ? 64 : TPB;
  constexpr int BPW = NT / TPB;                            // bins per workgroup
  constexpr int WIN = NP - 1 + ATB;                        // played frames t0-(NP-1) .. t0+ATB-1
  __shared__ zd win[BPW][WIN], atile[BPW][ATB], avec[BPW][NP], bvec[BPW][NP], rvec[BPW][NP];
  __shared__ float2 yout[BPW][ATB];
  __shared__ unsigned char fout[BPW][ATB];
  const int tid = threadIdx.x;
  const int sub = tid / TPB, ti = tid % TPB;
  const int r = ti >> 2, c = ti & 3;
  const int s = blockIdx.y;
  const int k = blockIdx.x * BPW + sub;
  const bool kvalid = k < K;
  const long sk = (long)s * K + (kvalid ? k : K - 1);
  const float2* vrow = V + sk * T_stride;
  const float2* arow = A + sk * T_stride;
  zd* Kk = Kst + sk * P * P;
  zd* hk = hist + sk * P;

  zd Krow[W], Kcol[W];
#pragma unroll
  for (int q = 0; q < W; q++) {
    const int j = c * W + q;
    const bool ok = r < P && j < P;
    Krow[q] = ok ? Kk[(long)r * P + j] : zmk(0.0, 0.0);
    Kcol[q] = ok ? Kk[(long)j * P + r] : zmk(0.0, 0.0);
  }
  zd R_r = r < P ? Rst[sk * P + r] : zmk(0.0, 0.0);
  if (c == 0) rvec[sub][r] = R_r;
  double sv = sig[sk];

  for (long t0 = 0; t0 < T; t0 += ATB) {
    for (int e = ti; e < WIN; e += TPB) win[sub][e] = played(vrow, hk, P, T, p.amp, t0 - (NP - 1) + e);
    if (ti < ATB) {
      const float2 f = (t0 + ti < T) ? arow[t0 + ti] : make_float2(0.f, 0.f);
      atile[sub][ti] = zmk((double)f.x, (double)f.y);
    }
    __syncthreads();
    const int nt = (T - t0 < ATB) ? (int)(T - t0) : ATB;
    for (int tt = 0; tt < nt; tt++) {
      zd xs[W];
      zd pe = zmk(0.0, 0.0);
#pragma unroll
      for (int q = 0; q < W; q++) {
        const int j = c * W + q;
        xs[q] = j < P ? win[sub][NP - 1 + tt - j] : zmk(0.0, 0.0);
        pe = zfma(rvec[sub][j], xs[q], pe);                                  // R^T v (zdotu)                        :263
      }
      const zd e = zsub(atile[sub][tt], quad_sum(pe));
      // the gate is per bin and a workgroup may hold several bins: every bin walks through the same barriers and `adapt`
      // masks the state change
      const bool adapt = zabs2(win[sub][NP - 1 + tt]) > p.threshold;         // update_ :227-232
      const double svn = p.beta * sv + (1.0 - p.beta) * zabs2(e);            // :273-275
      zd kr[W], kc[W];
      zd pa = zmk(0.0, 0.0), pb = zmk(0.0, 0.0);
#pragma unroll
      for (int q = 0; q < W; q++) {
        kr[q] = Krow[q]; kc[q] = Kcol[q];
        if (c * W + q == r && r < P) { kr[q].x += p.sigmau2; kc[q].x += p.sigmau2; }     // Kp = Sigma_u + K      :278-279
        pa = zfmabc(kr[q], xs[q], pa);                                       // (Kp conj(v))_r                       :281-282
        pb = zfma(xs[q], kc[q], pb);                                         // (v^T Kp)_r
      }
      const zd a_r = quad_sum(pa), b_r = quad_sum(pb);
      if (c == 0) { avec[sub][r] = a_r; bvec[sub][r] = b_r; }
      __syncthreads();
      zd pip = zmk(0.0, 0.0);
#pragma unroll
      for (int q = 0; q < W; q++) pip = zfma(xs[q], avec[sub][c * W + q], pip);          // v^T s                 :283
      const double inv = 1.0 / (quad_sum(pip.x) + svn);                      // :285-287
      if (adapt) {
        const zd g_r = zscale(a_r, inv);
        R_r = zfma(e, g_r, R_r);                                             // :290
#pragma unroll
        for (int q = 0; q < W; q++) {
          const zd g_q = zscale(avec[sub][c * W + q], inv);
          Krow[q] = zsub(kr[q], zmul(g_r, bvec[sub][c * W + q]));            // (I - G v^T) Kp = Kp - G (v^T Kp)     :293-301
          Kcol[q] = zsub(kc[q], zmul(g_q, b_r));
        }
        sv = svn;
      }
      if (c == 0) rvec[sub][r] = R_r;
      if (ti == 0) { yout[sub][tt] = make_float2((float)e.x, (float)e.y); fout[sub][tt] = adapt ? 1 : 0; }
      __syncthreads();
    }
    if (kvalid && ti < nt) {
      E[sk * T_stride + t0 + ti] = yout[sub][ti];
      if (flags) flags[sk * T_stride + t0 + ti] = fout[sub][ti];
    }
    __syncthreads();
  }

  // history of the next block: v of the last frame
  zd hn = zmk(0.0, 0.0);
  if (ti < P) hn = played(vrow, hk, P, T, p.amp, T - 1 - ti);
  __syncthreads();
  if (kvalid) {
    if (ti < P) hk[ti] = hn;
    if (r < P) {
#pragma unroll
      for (int q = 0; q < W; q++) {
        const int j = c * W + q;
        if (j < P) Kk[(long)r * P + j] = Krow[q];
      }
      if (c == 0) Rst[sk * P + r] = R_r;
    }
    if (ti == 0) sig[sk] = sv;
  }
}

template <int NP>
int launch_block(const float2* V, const float2* A, float2* E, unsigned char* flags, int S, int K, int P, long T_stride, long T,
                 const AecParams& p, zd* R, zd* Kst, double* sig, zd* hist, hipStream_t st)
{
  constexpr int TPB = 4 * NP;
  constexpr int NT = TPB < 64 ? 64 : TPB;
  constexpr int BPW = NT / TPB;
  hipLaunchKernelGGL(aec_block_kernel<NP>, dim3((unsigned)((K + BPW - 1) / BPW), (unsigned)S), dim3(NT), 0, st,
                     V, A, E, flags, K, P, T_stride, T, p, R, Kst, sig, hist);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

// ---- kind 3: double-talk detecting block Kalman filter, one workgroup per stream
// update_band_ (:821-853) in two halves.  The gate compares the running scalars with thresholds, so both halves keep the reference's
// operation order with separate multiplies and adds (no contraction into fused multiply-adds).
__device__ __forceinline__ void dtd_walk_inputs(double ce, double cs, double smth, double* o)
{
#pragma clang fp contract(off)
  o[0] = ce * smth;
  o[1] = cs * smth;
  const double csnr = cs / (ce + 1.0e-15);                                       // currSnr                                :839
  o[2] = csnr * smth;
}
__device__ __forceinline__ void dtd_walk(const double* in3, double* sfs, int K, double smth, bool early, double snr_th, double eng_th,
                                         double& ekE, double& skE, double& snr)
{
#pragma clang fp contract(off)
  const double om = 1.0 - smth;
  for (int m = 0; m < K; m++) {
    ekE = in3[3 * m + 0] + ekE * om;                                             // :837-840
    skE = in3[3 * m + 1] + skE * om;
    snr = in3[3 * m + 2] + snr * om;
    const bool go = early || (snr > snr_th && skE > eng_th);                     // threshold_ is snr_threshold       :805,:841
    double sf = -1.0;
    if (go) { const double ex = exp(-snr); sf = 2.0 / (1.0 + ex) - 1.0; }
    sfs[m] = sf;
  }
}
// LDS: es[K] zd (residuals) | in3[K][3] double (walk inputs) | sfs[K] double | Kl[K][P][P] zd (LDS_STATE)
template <bool LDS_STATE>
__global__ __launch_bounds__(DTD_NT)
void aec_dtd_kernel(const float2* __restrict__ V, const float2* __restrict__ A, float2* __restrict__ E,
                    unsigned char* __restrict__ flags, int K, int P, long T_stride, long T, AecParams p,
                    zd* __restrict__ Rst, zd* __restrict__ Kst, double* __restrict__ sig, zd* __restrict__ hist,
                    double* __restrict__ dtd)
{
  extern __shared__ __attribute__((aligned(16))) char smem[];
  zd* es = reinterpret_cast<zd*>(smem);
  double* in3 = reinterpret_cast<double*>(es + K);
  double* sfs = in3 + 3 * (long)K;
  zd* Kl = reinterpret_cast<zd*>(sfs + K);                       // 16 K + 8 (3 K + K) bytes in: 16-byte aligned
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int s = blockIdx.x;
  const long s0 = (long)s * K;
  const long PP = (long)P * P;
  zd* Kb = LDS_STATE ? Kl : Kst + s0 * PP;
  if constexpr (LDS_STATE) {
    for (long e = tid; e < K * PP; e += DTD_NT) Kl[e] = Kst[s0 * PP + e];
  }
  double ekE = dtd[4 * s + 0], skE = dtd[4 * s + 1], snr = dtd[4 * s + 2];       // (meaningful in thread 0 only)
  const long fbase = (p.frame_no0 <= AEC_FRAME_FROM_STATE) ? (long)dtd[4 * s + 3] : p.frame_no0;
  __syncthreads();

  for (long t = 0; t < T; t++) {
    const long fn = fbase >= 0 ? fbase + t : fbase;                              // the frame_no argument of next()       :902
    const bool early = fn < 100;
    const double smth = early ? 1.0 - (double)fn * (1.0 - p.smooth) / 100.0 : p.smooth;   // smoothEk_ == smoothSk_    :825-831
    // pass 1: residuals with the weights of the previous frame                                                      :878-890
    for (int m = w; m < K; m += DTD_NW) {
      const zd v = lane < P ? played(V + (s0 + m) * T_stride, hist + (s0 + m) * P, P, T, p.amp, t - lane) : zmk(0.0, 0.0);
      const zd rr = lane < P ? Rst[(s0 + m) * P + lane] : zmk(0.0, 0.0);
      const zd ip = wave_sum(zmul(rr, v));
      if (lane == 0) {
        const float2 af = A[(s0 + m) * T_stride + t];
        const zd a = zmk((double)af.x, (double)af.y);
        const zd e = zsub(a, ip);
        es[m] = e;
        const double ce = zabs2(e), cs = zabs2(zsub(a, e));                      // Sk = Ak - Ek                           :834-836
        dtd_walk_inputs(ce, cs, smth, in3 + 3 * m);
        E[(s0 + m) * T_stride + t] = make_float2((float)e.x, (float)e.y);
      }
    }
    __syncthreads();
    // the ordered walk: EkEnergy_, SkEnergy_, snr_ pass from bin to bin (update_band_ :821-853); plain multiplies and adds
    if (tid == 0) dtd_walk(in3, sfs, K, smth, early, p.threshold, p.eng_threshold, ekE, skE, snr);
    __syncthreads();
    // pass 2: Kalman update of the bins the walk let through                                                        :892-938
    for (int m = w; m < K; m += DTD_NW) {
      const double sf = sfs[m];
      if (lane == 0 && flags) flags[(s0 + m) * T_stride + t] = sf < 0.0 ? 0 : 1;
      if (sf < 0.0) continue;                                                    // (wavefront-uniform)
      const zd v = lane < P ? played(V + (s0 + m) * T_stride, hist + (s0 + m) * P, P, T, p.amp, t - lane) : zmk(0.0, 0.0);
      const zd e = es[m];
      // sigma2_v of a bin is loaded and stored by lane 0 alone and handed to the others through a register: no lane reads from
      // global memory what another lane wrote
      double sv_old = 0.0;
      if (lane == 0) sv_old = sig[s0 + m];
      sv_old = lane_d(sv_old, 0);
      const double svn = p.beta * sv_old + (1.0 - p.beta) * zabs2(e);            // :908-910
      const double dg = sf * p.sigmau2;                                          // Kp = sf Sigma_u + K                :913-915
      zd* Km = Kb + (long)m * PP;
      zd u = zmk(0.0, 0.0), sL = zmk(0.0, 0.0);
      for (int i = 0; i < P; i++) {
        zd kp = lane < P ? Km[(long)i * P + lane] : zmk(0.0, 0.0);
        if (lane == i) kp.x += dg;
        u = zfma(lane_z(v, i), kp, u);                                           // (v^T Kp)_lane
        const zd si = wave_sum(zfmabc(kp, v, zmk(0.0, 0.0)));                    // (Kp conj(v))_i                     :917-918
        if (lane == i) sL = si;
      }
      const double inv = 1.0 / (wave_sum(zmul(v, sL).x) + svn);                  // :919-923
      const zd g = zscale(sL, inv);
      if (lane < P) Rst[(s0 + m) * P + lane] = zfma(e, g, Rst[(s0 + m) * P + lane]);     // :926
      for (int i = 0; i < P; i++) {
        if (lane < P) {
          zd kp = Km[(long)i * P + lane];
          if (lane == i) kp.x += dg;
          Km[(long)i * P + lane] = zsub(kp, zmul(lane_z(g, i), u));              // Kp - G (v^T Kp)                    :929-937
        }
      }
      if (lane == 0) sig[s0 + m] = svn;
    }
    // (no barrier: pass 1 of the next frame touches only the bins this wavefront owns, and the walk starts after its barrier)
  }

  __syncthreads();
  // history of the next block: v of the last frame.  A lane reads and writes only its own slot; what a short block (T < P) moves
  // from slot j - T to slot j goes from lane to lane through registers
  for (int m = w; m < K; m += DTD_NW) {
    const zd own = lane < P ? hist[(s0 + m) * P + lane] : zmk(0.0, 0.0);
    const int src = (T <= lane) ? lane - (int)T : lane;
    const zd moved = zmk(__shfl(own.x, src, 64), __shfl(own.y, src, 64));
    zd hn = moved;
    if (lane < P && T - 1 - lane >= 0) {
      const float2 f = V[(s0 + m) * T_stride + (T - 1 - lane)];
      hn = zmk(p.amp * (double)f.x, p.amp * (double)f.y);
    }
    if (lane < P) hist[(s0 + m) * P + lane] = hn;
  }
  if constexpr (LDS_STATE) {
    for (long e = tid; e < K * PP; e += DTD_NT) Kst[s0 * PP + e] = Kl[e];
  }
  if (tid == 0) { dtd[4 * s + 0] = ekE; dtd[4 * s + 1] = skE; dtd[4 * s + 2] = snr; }
}

inline size_t dtd_lds_base(int K) { return sizeof(zd) * (size_t)K + sizeof(double) * (4 * (size_t)K + 2); }

}  // namespace

extern "C" {

int btk_aec_max_filter_length(void) { return AEC_MAX_P; }

int btk_aec_dtd_state_in_lds(int M, int P)
{
  const int K = M / 2 + 1;
  return dtd_lds_base(K) + sizeof(zd) * (size_t)K * P * P <= AEC_LDS_BUDGET ? 1 : 0;
}

static int aec_check(const char* who, int kind, int S, int M, int P)
{
  if (kind < 0 || kind > 3) return btk_set_error(BTK_ERR_PARAMETER, "%s: kind must be 0 (NLMS), 1 (Kalman), 2 (block Kalman) or 3 (DTD block Kalman)", who);
  if (S <= 0 || M < 2 || (M & 1)) return btk_set_error(BTK_ERR_DIMENSION, "%s: bad sizes S=%d M=%d", who, S, M);
  if (M > 2048) return btk_set_error(BTK_ERR_DIMENSION, "%s: M=%d exceeds this kernel (M <= 2048)", who, M);
  if (P < 1 || P > AEC_MAX_P) return btk_set_error(BTK_ERR_DIMENSION, "%s: sample_num P=%d exceeds this kernel (1 <= P <= %d)", who, P, AEC_MAX_P);
  if (kind < 2 && P != 1) return btk_set_error(BTK_ERR_DIMENSION, "%s: kinds 0 and 1 are one-tap filters (P=%d)", who, P);
  return BTK_OK;
}

int btk_aec_init(int kind, const double* params, int S, int M, int P, void* R_state, void* K_state, double* sigma2_v,
                 void* history, double* dtd_state, void* stream)
{
  const int rc = aec_check("btk_aec_init", kind, S, M, P);
  if (rc != BTK_OK) return rc;
  if (!params || !R_state || !K_state || !sigma2_v || !history || !dtd_state) return btk_set_error(BTK_ERR_PARAMETER, "btk_aec_init: null argument");
  // kind 1: sigma2_v = K = sigma2 (:95-98); kinds 2, 3: sigma2_v = sigmau2, K = sigmak2 I (:190-203); kind 0 keeps neither
  const double sigv0 = kind == 0 ? 0.0 : params[1];
  const double k0 = kind == 0 ? 0.0 : (kind == 1 ? params[1] : params[2]);
  hipLaunchKernelGGL(aec_init_kernel, dim3((unsigned)(M / 2 + 1), (unsigned)S), dim3(256), 0, as_stream(stream), kind, sigv0, k0, M / 2 + 1, P,
                     static_cast<zd*>(R_state), static_cast<zd*>(K_state), sigma2_v, static_cast<zd*>(history), dtd_state);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

int btk_aec_process(int kind, const double* params, const void* V, const void* A, void* E, void* adapted, int S, int M, int P,
                    long T_stride, long T, long frame_no0, void* R_state, void* K_state, double* sigma2_v, void* history,
                    double* dtd_state, void* stream)
{
  const int rc = aec_check("btk_aec_process", kind, S, M, P);
  if (rc != BTK_OK) return rc;
  if (!params || !V || !A || !E || !R_state || !K_state || !sigma2_v || !history || !dtd_state)
    return btk_set_error(BTK_ERR_PARAMETER, "btk_aec_process: null argument");
  if (T < 0 || T_stride < T) return btk_set_error(BTK_ERR_DIMENSION, "btk_aec_process: bad sizes T=%ld T_stride=%ld", T, T_stride);
  if (T == 0) return BTK_OK;
  const int K = M / 2 + 1;
  AecParams p = {};
  p.kind = kind;
  p.beta = params[0]; p.sigmau2 = params[1]; p.sigmak2 = params[2]; p.threshold = params[3];
  p.eng_threshold = params[4]; p.smooth = params[5]; p.amp = kind >= 2 ? params[6] : 1.0;
  p.frame_no0 = frame_no0;
  hipStream_t st = as_stream(stream);
  const float2* Vp = static_cast<const float2*>(V);
  const float2* Ap = static_cast<const float2*>(A);
  float2* Ep = static_cast<float2*>(E);
  unsigned char* fl = static_cast<unsigned char*>(adapted);
  zd* R = static_cast<zd*>(R_state);
  zd* Kst = static_cast<zd*>(K_state);
  zd* hist = static_cast<zd*>(history);
  int ret = BTK_OK;
  if (kind < 2) {
    hipLaunchKernelGGL(aec_scalar_kernel, dim3((unsigned)((K + 63) / 64), (unsigned)S), dim3(64), 0, st, Vp, Ap, Ep, fl, K, T_stride, T, p, R, Kst, sigma2_v);
    BTK_HIP_CHECK(hipGetLastError());
  } else if (kind == 2) {
    if (P <= 4)       ret = launch_block<4>(Vp, Ap, Ep, fl, S, K, P, T_stride, T, p, R, Kst, sigma2_v, hist, st);
    else if (P <= 8)  ret = launch_block<8>(Vp, Ap, Ep, fl, S, K, P, T_stride, T, p, R, Kst, sigma2_v, hist, st);
    else if (P <= 16) ret = launch_block<16>(Vp, Ap, Ep, fl, S, K, P, T_stride, T, p, R, Kst, sigma2_v, hist, st);
    else if (P <= 32) ret = launch_block<32>(Vp, Ap, Ep, fl, S, K, P, T_stride, T, p, R, Kst, sigma2_v, hist, st);
    else              ret = launch_block<64>(Vp, Ap, Ep, fl, S, K, P, T_stride, T, p, R, Kst, sigma2_v, hist, st);
    if (ret != BTK_OK) return ret;
  } else {
    const bool in_lds = btk_aec_dtd_state_in_lds(M, P) != 0;
    const size_t lds = dtd_lds_base(K) + (in_lds ? sizeof(zd) * (size_t)K * P * P : 0);
    if (in_lds) {
      BTK_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(aec_dtd_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(aec_dtd_kernel<true>, dim3((unsigned)S), dim3(DTD_NT), lds, st, Vp, Ap, Ep, fl, K, P, T_stride, T, p, R, Kst, sigma2_v, hist, dtd_state);
    } else {
      hipLaunchKernelGGL(aec_dtd_kernel<false>, dim3((unsigned)S), dim3(DTD_NT), lds, st, Vp, Ap, Ep, fl, K, P, T_stride, T, p, R, Kst, sigma2_v, hist, dtd_state);
    }
    BTK_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(aec_count_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, dtd_state, S, T);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

}  // extern "C"
