// hos_kernels.hip -- objective, gradient and minimiser of the maximum-empirical-kurtosis GSC beamformers (gfx950).
//
// SubbandMEKBeamformer / SubbandNMEKBeamformer of the reference (lib/pybeamformer.py:1596-1860) with the module functions
// fun_hos_bf / dfun_hos_bf (:1548-1593) they hand to the optimiser.  Per bin k and source s, with the packed active weights x:
//     wa_s   = unpack(x)_s ; NMEK: |gamma_s| wa_s / ||wa_s|| when ||wa_s|| > |gamma_s|, gamma_s = ||wuH[s][k]|| for gamma < 0 (:1845-1855)
//     woH_s  = wuH[s][k] - conj(wa_s) BmH[s][k]                                                  (:1484)
//     Y_s[t] = woH_s . X_k[t]                        (no conjugation of woH, :1485)
//     fun    = -(sum_s exY4_s - beta (sum_s exY2_s)^2 - 1e6) + alpha sum_s ||wa_s||^2            (:1632-1656, :1548-1569)
//     grad_s = -(dexY4_s - 2 beta exY2_s dexY2_s) + alpha wa_s                                    (:1658-1683, :1572-1593)
// All sums are float64; X is widened on load.  The frame weights factor out of the gradient,
//     dexY4_s = -BmH (sum_t 2 |Y|^2 conj(Y) X_t) / Ntot ,  dexY2_s = -BmH (sum_t conj(Y) X_t) / Ntot ,
// so BmH is read once for woH and once for the gradient, not once per frame.
//
// One workgroup of 8 wavefronts per bin, the frames in tiles of 512:
//   phase 1  one lane per frame: Y_s[t] (N complex multiply-adds against woH in LDS, X coalesced over the lanes), its powers into
//            the lane's running sums, conj(Y) and 2 |Y|^2 conj(Y) into LDS;
//   phase 2  (gradient only) wavefront w owns the channels w, w + 8, ...: each lane multiplies 8 frames of the tile into its own
//            partial sums of the two N-vectors -- 8 channels x 2 vectors complex float64 accumulators per lane, statically indexed.
//            With two sources the frames are passed over once per source: both sources' sums do not fit beside the loads.
//            The samples of a frame that is not selected are never read here (its lane reads the first selected frame against
//            its zero coefficients): the reference never touches such a frame, whatever it holds.
// Lane partials are combined by an xor butterfly, wavefront partials in wavefront order by one lane: a fixed order, no atomics,
// so two runs give the same bits.  hos_minimize_kernel runs the whole Polak-Ribiere+ / Armijo iteration of a bin inside its
// workgroup: the vectors of the optimiser live in LDS, every decision is taken by lane 0 and broadcast through LDS.
#include "btk_internal.h"
#include "wave_ops.h"

namespace {

constexpr int HOS_THREADS = 512;       // 8 wavefronts
constexpr int HOS_WAVES = HOS_THREADS / 64;
constexpr int HOS_TILE = HOS_THREADS;  // frames per tile, one per lane in phase 1
constexpr int HOS_MAXN = 64;           // channels: 8 per wavefront in phase 2
constexpr int HOS_CPW = HOS_MAXN / HOS_WAVES;
constexpr int HOS_FPL = HOS_TILE / 64; // frames per lane in phase 2
constexpr int HOS_MAXD = 2 * 2 * (HOS_MAXN - 1);
constexpr double HOS_OFFSET = -1.0e6;  // SubbandMEKBeamformer._OFFSET (:1606)

struct hos_args {
  const float2* X;        // [K][N][T_stride]
  const float* mask;      // [T] or null
  const double2* wuH;     // [NS][K][N]
  const double2* BmH;     // [NS][K][N-Nc][N]
  const double* pY2;      // [K][NS] or null
  const double* pY4;      // [K][NS] or null
  const long long* pN;    // [K][NS] or null
  double alpha, beta, gamma;
  int normalize, K, N, Nc;
  long T_stride, T;
};

template <int NS>
struct hos_lds {
  double2 woH[NS][HOS_MAXN];
  double2 wa[NS][HOS_MAXN];
  double2 c2[HOS_TILE];                      // conj(Y) and 2 |Y|^2 conj(Y) of the tile, for the source of the pass
  double2 c4[HOS_TILE];
  double2 v2[NS][HOS_MAXN];
  double2 v4[NS][HOS_MAXN];
  double part[HOS_WAVES][2 * NS + 2];
  double sum2[NS], sum4[NS], mix2, mix4;     // sum_t |Y_s|^2, |Y_s|^4; sum_t m_t, m_t^2 with m_t = sum_s |Y_s|^2 / NS
  double scale[NS], reg[NS];
  double fun;
  double grad[HOS_MAXD];
  long long tsel;
  int cnt[HOS_WAVES];
  // optimiser
  double x[HOS_MAXD], g[HOS_MAXD], d[HOS_MAXD], xt[HOS_MAXD];
  double sc[4];
  int flag;
  // phase 2 reads a frame that is not selected at the first selected one
  long long tfirst;
  long long first[HOS_WAVES];
  long long src[HOS_TILE];                   // the frame phase 2 reads for each frame of the tile: itself if it is selected
};

// number of selected frames of the block (the reference's len(self._observations)) and the first of them (0 if there is none)
template <int NS>
__device__ void hos_count_frames(const hos_args& a, hos_lds<NS>& L)
{
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int c = 0;
  long long first = a.T;
  for (long t = tid; t < a.T; t += HOS_THREADS) {
    const bool s = !a.mask || a.mask[t] != 0.f;
    c += s ? 1 : 0;
    first = s && t < first ? t : first;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    c += __shfl_xor(c, m);
    const long long o = __shfl_xor(first, m);
    first = o < first ? o : first;
  }
  if (lane == 0) { L.cnt[wave] = c; L.first[wave] = first; }
  __syncthreads();
  if (tid == 0) {
    long long n = 0, f = a.T;
    for (int w = 0; w < HOS_WAVES; w++) { n += L.cnt[w]; f = L.first[w] < f ? L.first[w] : f; }
    L.tsel = n;
    L.tfirst = f < a.T ? f : 0;
  }
  __syncthreads();
}

// One evaluation at the packed weights xin (LDS): L.fun, L.sum2/sum4/mix2/mix4 and, with want_grad, L.grad.
template <int NS>
__device__ void hos_pass(const hos_args& a, int k, const double* xin, bool want_grad, hos_lds<NS>& L)
{
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N, dim = a.N - a.Nc;

  // ---- norm_active_weight_vectors (:1845-1860): one lane per source, terms in index order
  if (tid < NS) {
    const int s = tid;
    double scale = -1.0;                                   // < 0: wa is taken as it is
    if (a.normalize) {
      double n2 = 0.0;
      for (int j = 0; j < dim; j++) {
        const double re = xin[2 * (s * dim + j)], im = xin[2 * (s * dim + j) + 1];
        n2 += re * re + im * im;
      }
      const double nrm = sqrt(n2);
      double gam = a.gamma;
      if (gam < 0.0) {
        const double2* wu = a.wuH + ((long)s * a.K + k) * N;
        double w2 = 0.0;
#pragma unroll 8
        for (int n = 0; n < N; n++) w2 += wu[n].x * wu[n].x + wu[n].y * wu[n].y;
        gam = sqrt(w2);
      }
      gam = fabs(gam);
      if (nrm > gam) { scale = gam; L.sc[2 + s] = nrm; }
    }
    L.scale[s] = scale;
  }
  __syncthreads();
  if (tid < NS * HOS_MAXN) {
    const int s = tid >> 6, j = tid & 63;
    if (j < dim) {
      double re = xin[2 * (s * dim + j)], im = xin[2 * (s * dim + j) + 1];
      const double sc = L.scale[s];
      if (sc >= 0.0) { const double nrm = L.sc[2 + s]; re = sc * re / nrm; im = sc * im / nrm; }
      L.wa[s][j] = make_double2(re, im);
    }
  }
  __syncthreads();
  // ---- woH = wuH - conj(wa) BmH (:1484) and the regulariser ||wa_s||^2 (:1567)
  if (tid < NS * HOS_MAXN) {
    const int s = tid >> 6, n = tid & 63;
    if (n < N) {
      const double2 wu = a.wuH[((long)s * a.K + k) * N + n];
      const double2* B = a.BmH + (((long)s * a.K + k) * dim) * N + n;
      double pr = 0.0, pi = 0.0;
#pragma unroll 8
      for (int j = 0; j < dim; j++) {                      // eight rows of BmH in flight
        const double2 w = L.wa[s][j], b = B[(long)j * N];
        pr += w.x * b.x + w.y * b.y;                       // conj(w) b
        pi += w.x * b.y - w.y * b.x;
      }
      L.woH[s][n] = make_double2(wu.x - pr, wu.y - pi);
    } else {
      L.woH[s][n] = make_double2(0.0, 0.0);
    }
  } else if (tid < NS * HOS_MAXN + NS) {
    const int s = tid - NS * HOS_MAXN;
    double r = 0.0;
    for (int j = 0; j < dim; j++) r += L.wa[s][j].x * L.wa[s][j].x + L.wa[s][j].y * L.wa[s][j].y;
    L.reg[s] = r;
  }
  __syncthreads();

  const float2* Xk = a.X + (long)k * N * a.T_stride;
  double s2[NS], s4[NS], m2 = 0.0, m4 = 0.0;
#pragma unroll
  for (int s = 0; s < NS; s++) { s2[s] = 0.0; s4[s] = 0.0; }

  // One pass over the frames per source when the gradient is wanted (the two N-vector sums of ONE source are what fits in
  // registers beside the loads), one pass altogether otherwise.  Phase 1 computes the outputs of every source in each pass --
  // the powers are summed in the first one only -- and hands the coefficients of the pass's source to phase 2.
  const int npass = want_grad ? NS : 1;
  for (int sp = 0; sp < npass; sp++) {
    double a2r[HOS_CPW], a2i[HOS_CPW], a4r[HOS_CPW], a4i[HOS_CPW];
#pragma unroll
    for (int i = 0; i < HOS_CPW; i++) { a2r[i] = 0.0; a2i[i] = 0.0; a4r[i] = 0.0; a4i[i] = 0.0; }

    for (long t0 = 0; t0 < a.T; t0 += HOS_TILE) {
      // ---- phase 1
      {
        const long t = t0 + tid;
        const bool sel = t < a.T && (!a.mask || a.mask[t] != 0.f);
        const float2* xt = Xk + (t < a.T ? t : a.T - 1);   // every lane loads from a valid address; what it read is dropped below
        double yr[NS], yi[NS];
#pragma unroll
        for (int s = 0; s < NS; s++) { yr[s] = 0.0; yi[s] = 0.0; }
        for (int n0 = 0; n0 < N; n0 += HOS_CPW) {
          float2 xf[HOS_CPW];
#pragma unroll
          for (int i = 0; i < HOS_CPW; i++) {              // eight loads in flight, none behind a branch
            const int n = n0 + i < N ? n0 + i : N - 1;
            xf[i] = xt[(long)n * a.T_stride];
          }
#pragma unroll
          for (int i = 0; i < HOS_CPW; i++) {
            const double xr = (double)xf[i].x, xi = (double)xf[i].y;
#pragma unroll
            for (int s = 0; s < NS; s++) {
              const double2 w = L.woH[s][n0 + i];          // zero beyond N
              yr[s] += w.x * xr - w.y * xi;
              yi[s] += w.x * xi + w.y * xr;
            }
          }
        }
        double m = 0.0;
#pragma unroll
        for (int s = 0; s < NS; s++) {
          yr[s] = sel ? yr[s] : 0.0;                       // a frame that is not selected contributes nothing
          yi[s] = sel ? yi[s] : 0.0;
          const double y2 = yr[s] * yr[s] + yi[s] * yi[s];
          if (sp == 0) { s2[s] += y2; s4[s] += y2 * y2; }
          m += y2;
          if (want_grad && s == sp) {                      // only phase 2 reads these
            L.c2[tid] = make_double2(yr[s], -yi[s]);
            L.c4[tid] = make_double2(2.0 * y2 * yr[s], -2.0 * y2 * yi[s]);
          }
        }
        m /= (double)NS;
        if (sp == 0) { m2 += m; m4 += m * m; }
        if (want_grad) L.src[tid] = sel ? t : L.tfirst;
      }
      // ---- phase 2: an objective-only pass (every line-search trial) has none, and no barrier in its tile loop
      if (want_grad) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < HOS_FPL; j++) {
          const int tt = lane + 64 * j;
          // A frame that is not selected (masked out, or beyond T) has zero coefficients in LDS, but zero times what it holds
          // is NaN if that is Inf or NaN, and the reference never touches such a frame: its lane loads the first selected
          // frame instead, whose samples are counted anyway.  Zero times those changes no bit of a sum.  Phase 1 leaves the
          // frame to read in LDS, so there is no select here: with one, hipcc serialised the BmH loads of the line-search passes.
          const float2* xt = Xk + L.src[tt];
          const double2 c2 = L.c2[tt], c4 = L.c4[tt];
          float2 xf[HOS_CPW];
#pragma unroll
          for (int i = 0; i < HOS_CPW; i++) {              // eight loads in flight, none behind a branch; channels beyond N
            const int n = wave + HOS_WAVES * i;            // read channel N - 1 into sums nobody stores
            xf[i] = xt[(long)(n < N ? n : N - 1) * a.T_stride];
          }
#pragma unroll
          for (int i = 0; i < HOS_CPW; i++) {
            const double xr = (double)xf[i].x, xi = (double)xf[i].y;
            a2r[i] += c2.x * xr - c2.y * xi;
            a2i[i] += c2.x * xi + c2.y * xr;
            a4r[i] += c4.x * xr - c4.y * xi;
            a4i[i] += c4.x * xi + c4.y * xr;
          }
        }
        __syncthreads();
      }
    }
    if (want_grad) {                                       // lane partials of the pass's source -> v2, v4
#pragma unroll
      for (int i = 0; i < HOS_CPW; i++) {
        const int n = wave + HOS_WAVES * i;
        if (n < N) {
          const double r0 = wave_sum(a2r[i]), r1 = wave_sum(a2i[i]);
          const double r2 = wave_sum(a4r[i]), r3 = wave_sum(a4i[i]);
          if (lane == 0) {                                 // no frame selected: every lane read frame 0, which does not count
            L.v2[sp][n] = L.tsel ? make_double2(r0, r1) : make_double2(0.0, 0.0);
            L.v4[sp][n] = L.tsel ? make_double2(r2, r3) : make_double2(0.0, 0.0);
          }
        }
      }
    }
  }

  // ---- lane partials -> wavefront partials -> totals, in a fixed order
#pragma unroll
  for (int s = 0; s < NS; s++) {
    const double r2 = wave_sum(s2[s]), r4 = wave_sum(s4[s]);
    if (lane == 0) { L.part[wave][2 * s] = r2; L.part[wave][2 * s + 1] = r4; }
  }
  {
    const double r2 = wave_sum(m2), r4 = wave_sum(m4);
    if (lane == 0) { L.part[wave][2 * NS] = r2; L.part[wave][2 * NS + 1] = r4; }
  }
  __syncthreads();
  if (tid == 0) {
    double q[2 * NS + 2];
    for (int i = 0; i < 2 * NS + 2; i++) {
      double v = 0.0;
      for (int w = 0; w < HOS_WAVES; w++) v += L.part[w][i];
      q[i] = v;
    }
    double ex4 = 0.0, ex2 = 0.0, reg = 0.0;
    for (int s = 0; s < NS; s++) {
      L.sum2[s] = q[2 * s];
      L.sum4[s] = q[2 * s + 1];
      const long long pn = a.pN ? a.pN[(long)k * NS + s] : 0;
      const double p2 = a.pY2 ? a.pY2[(long)k * NS + s] : 0.0, p4 = a.pY4 ? a.pY4[(long)k * NS + s] : 0.0;
      const double ntot = (double)(pn + L.tsel);
      ex4 += (p4 * (double)pn + q[2 * s + 1]) / ntot;
      ex2 += (p2 * (double)pn + q[2 * s]) / ntot;
      reg += a.alpha * L.reg[s];
    }
    L.mix2 = q[2 * NS];
    L.mix4 = q[2 * NS + 1];
    const double kurt = ex4 - a.beta * ex2 * ex2;
    L.fun = -(kurt + HOS_OFFSET) + reg;
  }
  __syncthreads();
  if (want_grad) {
    // row (s, j) of -BmH v / Ntot: the channels over the lanes, rows over the wavefronts
    for (int r = wave; r < NS * dim; r += HOS_WAVES) {
      const int s = r / dim, j = r - s * dim;
      double p2r = 0.0, p2i = 0.0, p4r = 0.0, p4i = 0.0;
      if (lane < N) {
        const double2 b = a.BmH[(((long)s * a.K + k) * dim + j) * N + lane];
        const double2 u = L.v2[s][lane], v = L.v4[s][lane];
        p2r = b.x * u.x - b.y * u.y; p2i = b.x * u.y + b.y * u.x;
        p4r = b.x * v.x - b.y * v.y; p4i = b.x * v.y + b.y * v.x;
      }
      p2r = wave_sum(p2r); p2i = wave_sum(p2i); p4r = wave_sum(p4r); p4i = wave_sum(p4i);
      if (lane == 0) {
        const long long pn = a.pN ? a.pN[(long)k * NS + s] : 0;
        const double ntot = (double)(pn + L.tsel);
        const double ex2 = L.sum2[s] / ntot;               // no previous-statistics term here (:1681)
        const double d4r = -p4r / ntot, d4i = -p4i / ntot, d2r = -p2r / ntot, d2i = -p2i / ntot;
        const double2 w = L.wa[s][j];
        L.grad[2 * r] = -(d4r - 2.0 * a.beta * ex2 * d2r) + a.alpha * w.x;
        L.grad[2 * r + 1] = -(d4i - 2.0 * a.beta * ex2 * d2i) + a.alpha * w.y;
      }
    }
    __syncthreads();
  }
}

// grid: K, block: 512.  x [K][D] or null (zero weights); fun [K]; grad [K][D] or null; stats [K][2 NS + 2] =
// (sum |Y_s|^2, sum |Y_s|^4) per source, then sum_t m_t and sum_t m_t^2, or null.
template <int NS>
__global__ __launch_bounds__(HOS_THREADS)
void hos_eval_kernel(hos_args a, const double* __restrict__ x, double* __restrict__ fun, double* __restrict__ grad,
                     double* __restrict__ stats)
{
  __shared__ hos_lds<NS> L;
  const int k = blockIdx.x, tid = threadIdx.x;
  const int D = 2 * NS * (a.N - a.Nc);
  if (tid < D) L.x[tid] = x ? x[(long)k * D + tid] : 0.0;
  hos_count_frames<NS>(a, L);
  hos_pass<NS>(a, k, L.x, grad != nullptr, L);
  if (tid == 0) {
    fun[k] = L.fun;
    if (stats) {
      for (int s = 0; s < NS; s++) { stats[(long)k * (2 * NS + 2) + 2 * s] = L.sum2[s]; stats[(long)k * (2 * NS + 2) + 2 * s + 1] = L.sum4[s]; }
      stats[(long)k * (2 * NS + 2) + 2 * NS] = L.mix2;
      stats[(long)k * (2 * NS + 2) + 2 * NS + 1] = L.mix4;
    }
  }
  if (grad && tid < D) grad[(long)k * D + tid] = L.grad[tid];
}

struct hos_opt {
  int maxiter, max_halvings;
  double gtol, mindelta, c1;
};

// dot product of two LDS vectors by one lane, terms in index order
__device__ __forceinline__ double hos_dot(const double* u, const double* v, int D)
{
  double r = 0.0;
  for (int i = 0; i < D; i++) r += u[i] * v[i];
  return r;
}

// grid: K, block: 512: Polak-Ribiere+ conjugate gradients with Armijo backtracking, the whole iteration of a bin in its workgroup.
//   x_out [K][D], f_out [K], iters [K] int32, trace_f [K][maxiter] (NaN where no step was accepted), halvings [K][maxiter] int32
//   (-1: no step accepted in that iteration, -2: iteration not reached)
template <int NS>
__global__ __launch_bounds__(HOS_THREADS)
void hos_minimize_kernel(hos_args a, hos_opt o, const double* __restrict__ x0, double* __restrict__ x_out,
                         double* __restrict__ f_out, int* __restrict__ iters, double* __restrict__ trace_f,
                         int* __restrict__ halvings)
{
  __shared__ hos_lds<NS> L;
  const int k = blockIdx.x, tid = threadIdx.x;
  const int D = 2 * NS * (a.N - a.Nc);
  if (tid < D) L.x[tid] = x0 ? x0[(long)k * D + tid] : 0.0;
  for (int i = tid; i < o.maxiter; i += HOS_THREADS) {
    trace_f[(long)k * o.maxiter + i] = __longlong_as_double(0x7ff8000000000000LL);
    halvings[(long)k * o.maxiter + i] = -2;
  }
  hos_count_frames<NS>(a, L);
  hos_pass<NS>(a, k, L.x, true, L);
  double f = L.fun;                                        // every lane carries the same scalars
  if (tid < D) { L.g[tid] = L.grad[tid]; L.d[tid] = -L.grad[tid]; }
  __syncthreads();
  double step = 0.0;
  int it = 0;
  for (; it < o.maxiter; it++) {
    if (tid == 0) {
      const double gg = hos_dot(L.g, L.g, D);
      double gd = hos_dot(L.g, L.d, D);
      L.flag = gd >= 0.0 ? 1 : 0;
      if (gd >= 0.0) gd = -gg;
      L.sc[0] = gg; L.sc[1] = gd;
    }
    __syncthreads();
    const double gg = L.sc[0], gd = L.sc[1];
    const int restart = L.flag;
    const double gnorm = sqrt(gg);
    if (gnorm < o.gtol) break;
    if (restart && tid < D) L.d[tid] = -L.g[tid];
    double al = it == 0 ? 2.0 / gnorm : 2.0 * step;
    int h = 0;
    bool ok = false;
    double ft = f;
    for (; h <= o.max_halvings; h++) {
      __syncthreads();
      if (tid < D) L.xt[tid] = L.x[tid] + al * L.d[tid];
      __syncthreads();
      hos_pass<NS>(a, k, L.xt, false, L);
      ft = L.fun;
      if (ft <= f + o.c1 * al * gd) { ok = true; break; }
      al *= 0.5;
    }
    if (!ok) {
      if (tid == 0) halvings[(long)k * o.maxiter + it] = -1;
      break;
    }
    __syncthreads();
    if (tid < D) L.x[tid] = L.xt[tid];
    __syncthreads();
    hos_pass<NS>(a, k, L.x, true, L);                      // the gradient at the accepted point; L.fun == ft, same sums
    if (tid == 0) {
      double num = 0.0;
      for (int i = 0; i < D; i++) num += L.grad[i] * (L.grad[i] - L.g[i]);
      const double b = num / gg;
      L.sc[0] = b > 0.0 ? b : 0.0;
      trace_f[(long)k * o.maxiter + it] = ft;
      halvings[(long)k * o.maxiter + it] = h;
    }
    __syncthreads();
    const double pr = L.sc[0];
    if (tid < D) { L.d[tid] = -L.grad[tid] + pr * L.d[tid]; L.g[tid] = L.grad[tid]; }
    __syncthreads();
    const double df = fabs(f - ft);
    f = ft;
    step = al;
    if (df < o.mindelta) { it++; break; }
  }
  __syncthreads();
  if (tid < D) x_out[(long)k * D + tid] = L.x[tid];
  if (tid == 0) { f_out[k] = f; iters[k] = it; }
}

int hos_check(const char* who, int K, int N, int Nc, int NS, long T_stride, long T)
{
  if (N < 2 || N > HOS_MAXN) return btk_set_error(BTK_ERR_DIMENSION, "%s: N=%d channels, need 2 .. %d", who, N, HOS_MAXN);
  if (Nc < 1 || Nc > 2 || Nc >= N) return btk_set_error(BTK_ERR_DIMENSION, "%s: Nc=%d constraints, need 1 or 2 and fewer than N=%d", who, Nc, N);
  if (NS < 1 || NS > 2) return btk_set_error(BTK_ERR_DIMENSION, "%s: NS=%d sources, need 1 or 2", who, NS);
  if (K < 1 || T < 1 || T_stride < T)
    return btk_set_error(BTK_ERR_DIMENSION, "%s: bad sizes K=%d T=%ld T_stride=%ld", who, K, T, T_stride);
  return BTK_OK;
}

hos_args hos_pack(const void* X, const void* mask, const void* wuH, const void* BmH, double alpha, double beta, double gamma,
                  int normalize, const void* prevAvgY2, const void* prevAvgY4, const void* prevFrameN, int K, int N, int Nc,
                  long T_stride, long T)
{
  hos_args a;
  a.X = static_cast<const float2*>(X);
  a.mask = static_cast<const float*>(mask);
  a.wuH = static_cast<const double2*>(wuH);
  a.BmH = static_cast<const double2*>(BmH);
  a.pY2 = static_cast<const double*>(prevAvgY2);
  a.pY4 = static_cast<const double*>(prevAvgY4);
  a.pN = static_cast<const long long*>(prevFrameN);
  a.alpha = alpha; a.beta = beta; a.gamma = gamma;
  a.normalize = normalize; a.K = K; a.N = N; a.Nc = Nc;
  a.T_stride = T_stride; a.T = T;
  return a;
}

}  // namespace

extern "C" {

int btk_hos_max_channels(void) { return HOS_MAXN; }

// everything the kernels keep between their phases lives in LDS: callers that size a workspace from this get 0
long btk_hos_workspace_bytes(int K, int N, int Nc, int NS, long T)
{
  (void)K; (void)N; (void)Nc; (void)NS; (void)T;
  return 0;
}

// fun_hos_bf / dfun_hos_bf with MEK / NMEK calc_obj_func and gradient for every bin (lib/pybeamformer.py:1548-1593, 1632-1683, 1845-1860)
int btk_hos_eval(const void* X, const void* mask, const void* wuH, const void* BmH, const void* x, double alpha, double beta,
                 double gamma, int normalize, const void* prevAvgY2, const void* prevAvgY4, const void* prevFrameN, int K, int N,
                 int Nc, int NS, long T_stride, long T, void* fun, void* grad, void* stats, void* stream)
{
  const int rc = hos_check("btk_hos_eval", K, N, Nc, NS, T_stride, T);
  if (rc != BTK_OK) return rc;
  if (!X || !wuH || !BmH || !fun) return btk_set_error(BTK_ERR_PARAMETER, "btk_hos_eval: null argument");
  const hos_args a = hos_pack(X, mask, wuH, BmH, alpha, beta, gamma, normalize, prevAvgY2, prevAvgY4, prevFrameN, K, N, Nc, T_stride, T);
  if (NS == 1)
    hipLaunchKernelGGL(hos_eval_kernel<1>, dim3((unsigned)K), dim3(HOS_THREADS), 0, as_stream(stream), a,
                       static_cast<const double*>(x), static_cast<double*>(fun), static_cast<double*>(grad), static_cast<double*>(stats));
  else
    hipLaunchKernelGGL(hos_eval_kernel<2>, dim3((unsigned)K), dim3(HOS_THREADS), 0, as_stream(stream), a,
                       static_cast<const double*>(x), static_cast<double*>(fun), static_cast<double*>(grad), static_cast<double*>(stats));
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

// the loop of estimate_active_weights (:1802-1827) for every bin at once, with the optimiser of DESIGN.md 3.15 in place of pygsl's
int btk_hos_minimize(const void* X, const void* mask, const void* wuH, const void* BmH, const void* x0, double alpha, double beta,
                     double gamma, int normalize, const void* prevAvgY2, const void* prevAvgY4, const void* prevFrameN, int K,
                     int N, int Nc, int NS, long T_stride, long T, int maxiter, double gtol, double mindelta, int max_halvings,
                     double armijo_c1, void* x_out, void* f_out, void* iters_out, void* trace_f, void* trace_halvings, void* stream)
{
  const int rc = hos_check("btk_hos_minimize", K, N, Nc, NS, T_stride, T);
  if (rc != BTK_OK) return rc;
  if (maxiter < 0 || max_halvings < 0 || max_halvings > 1000)
    return btk_set_error(BTK_ERR_PARAMETER, "btk_hos_minimize: maxiter=%d max_halvings=%d", maxiter, max_halvings);
  if (!X || !wuH || !BmH || !x_out || !f_out || !iters_out || (maxiter > 0 && (!trace_f || !trace_halvings)))
    return btk_set_error(BTK_ERR_PARAMETER, "btk_hos_minimize: null argument");
  const hos_args a = hos_pack(X, mask, wuH, BmH, alpha, beta, gamma, normalize, prevAvgY2, prevAvgY4, prevFrameN, K, N, Nc, T_stride, T);
  hos_opt o;
  o.maxiter = maxiter; o.max_halvings = max_halvings; o.gtol = gtol; o.mindelta = mindelta; o.c1 = armijo_c1;
  if (NS == 1)
    hipLaunchKernelGGL(hos_minimize_kernel<1>, dim3((unsigned)K), dim3(HOS_THREADS), 0, as_stream(stream), a, o,
                       static_cast<const double*>(x0), static_cast<double*>(x_out), static_cast<double*>(f_out),
                       static_cast<int*>(iters_out), static_cast<double*>(trace_f), static_cast<int*>(trace_halvings));
  else
    hipLaunchKernelGGL(hos_minimize_kernel<2>, dim3((unsigned)K), dim3(HOS_THREADS), 0, as_stream(stream), a, o,
                       static_cast<const double*>(x0), static_cast<double*>(x_out), static_cast<double*>(f_out),
                       static_cast<int*>(iters_out), static_cast<double*>(trace_f), static_cast<int*>(trace_halvings));
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

}  // extern "C"
