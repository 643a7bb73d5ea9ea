// track_kernels.hip -- EKF / IEKF speaker tracking over the TDOA peaks of a block of frames (lib/pykalman.py:84-266 over
// lib/pytdoa.py's tdoa / linearize / calc_linearized_observation), float64 throughout.
//
// One wavefront per stream, lanes over microphone pairs (a loop for P > 64), frames in order.  The reference inverts the
// nobs x nobs innovation covariance S = sigmaV2 I + H Kp H^T per frame; with A = H^T H (n x n, n <= 3) and
// M = (sigmaV2 I + A Kp)^-1 that inverse is S^-1 = (I - H Kp M H^T) / sigmaV2, so that
//     G = W H^T,  W = Kp (I - A Kp M) / sigmaV2 = Kp M,    G H = W A,    (I - G H) Kp = sigmaV2 W,
//     d2 = s^T S^-1 s = (s^T s - (H^T s)^T Kp M (H^T s)) / sigmaV2,
// and every IEKF round needs only H^T s and A: a frame is three wave reductions over the observed pairs (A, H^T s, s^T s, and
// the count) and scalar work in n <= 3 dimensions, which every lane does redundantly on the reduced (lane-identical) sums.
// Matrices are held 3 x 3, zero outside the leading n x n block (adding zeros and multiplying by the unit pad of the inverse
// are exact, so the arithmetic is that of the n x n problem).
//
// lag / height [S][P][T] are staged through LDS in tiles of frames: the global reads run along T, the per-frame reads of a
// lane's pair come from LDS.  The per-pair geometry lies in LDS too.
#include <cmath>
#include "btk_internal.h"
#include "wave_ops.h"

namespace {

constexpr int TRACK_LANES = 64;
constexpr int TRACK_MAX_TILE = 32;                  // frames per LDS tile at most
constexpr long TRACK_LDS_BYTES = 48 * 1024;         // per workgroup: P * (48 + 8 tile) bytes
constexpr int TRACK_GAMMA_ITMAX = 20000;            // both expansions need O(sqrt(a)) terms; a = nobs / 2

// regularised lower incomplete gamma P(a, x): the series for x < a + 1, the continued fraction (modified Lentz) otherwise
__device__ double track_gammainc(double a, double x)
{
  if (!(x > 0.0)) return 0.0;
  if (isinf(x)) return 1.0;
  const double EPS = 1.0e-16, FPMIN = 1.0e-300;
  const double front = exp(-x + a * log(x) - lgamma(a));
  if (x < a + 1.0) {
    double ap = a, del = 1.0 / a, sum = del;
    for (int i = 0; i < TRACK_GAMMA_ITMAX; ++i) {
      ap += 1.0;
      del *= x / ap;
      sum += del;
      if (fabs(del) < fabs(sum) * EPS) break;
    }
    return sum * front;
  }
  double b = x + 1.0 - a, c = 1.0 / FPMIN, d = 1.0 / b, h = d;
  for (int i = 1; i <= TRACK_GAMMA_ITMAX; ++i) {
    const double an = -(double)i * ((double)i - a);
    b += 2.0;
    d = an * d + b;
    if (fabs(d) < FPMIN) d = FPMIN;
    c = b + an / c;
    if (fabs(c) < FPMIN) c = FPMIN;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (fabs(del - 1.0) < EPS) break;
  }
  return 1.0 - front * h;
}

__device__ __forceinline__ void mat_mul(const double (&a)[3][3], const double (&b)[3][3], double (&c)[3][3])
{
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c[i][j] = a[i][0] * b[0][j] + a[i][1] * b[1][j] + a[i][2] * b[2][j];
}

__device__ __forceinline__ void mat_vec(const double (&a)[3][3], const double (&v)[3], double (&r)[3])
{
#pragma unroll
  for (int i = 0; i < 3; ++i) r[i] = a[i][0] * v[0] + a[i][1] * v[1] + a[i][2] * v[2];
}

__device__ __forceinline__ void mat_inv(const double (&m)[3][3], double (&r)[3][3])
{
  const double c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1];
  const double c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2];
  const double c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
  const double idet = 1.0 / (m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02);
  r[0][0] = c00 * idet;
  r[1][0] = c01 * idet;
  r[2][0] = c02 * idet;
  r[0][1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) * idet;
  r[1][1] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) * idet;
  r[2][1] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) * idet;
  r[0][2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) * idet;
  r[1][2] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) * idet;
  r[2][2] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) * idet;
}

// KalmanFilter.adjust_boundaries (lib/pykalman.py:113-139).  The reference wraps phi by repeated +- 2 pi; that is followed
// for up to 4096 turns, beyond which (a diverged state) the remaining whole turns are removed in one step so that the kernel
// always ends.
__device__ __forceinline__ void adjust_boundaries(double (&x)[3], int n)
{
  const double PI = 3.141592653589793;
  double theta = x[0], phi = n > 1 ? x[1] : 0.0;
  if (theta < 0.0) {
    theta = -theta;
    phi += PI;
  } else if (theta > PI) {
    theta -= PI;
    phi += PI;
  }
  int turns = 0;
  while (phi < -PI && turns < 4096) { phi += 2.0 * PI; ++turns; }
  while (phi > PI && turns < 4096) { phi -= 2.0 * PI; ++turns; }
  if (turns == 4096 && isfinite(phi)) phi -= 2.0 * PI * rint(phi / (2.0 * PI));
  x[0] = theta;
  if (n > 1) x[1] = phi;
}

__global__ __launch_bounds__(TRACK_LANES) void ekf_track_kernel(btk_ekf_params prm, const int* __restrict__ lag,
                                                                 const float* __restrict__ height,
                                                                 const double* __restrict__ geom,
                                                                 const int* __restrict__ t_begin, int P, long T, int tile,
                                                                 double* __restrict__ state, double* __restrict__ xk,
                                                                 double* __restrict__ Kf, int* __restrict__ flags)
{
  extern __shared__ double lds[];
  double* s_geom = lds;                                              // [P][6]
  int* s_lag = reinterpret_cast<int*>(lds + 6 * (long)P);            // [tile][P]
  float* s_height = reinterpret_cast<float*>(s_lag + (long)tile * P);  // [tile][P]
  const int s = blockIdx.x, lane = threadIdx.x, n = prm.n;
  const long in0 = (long)s * P * T;

  for (int i = lane; i < 6 * P; i += TRACK_LANES) s_geom[i] = geom[i];

  double* st = state + 16 * (long)s;
  double x[3], K[3][3], F[3][3], U[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    x[i] = i < n ? st[i] : 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const bool in = i < n && j < n;
      K[i][j] = in ? st[3 + 3 * i + j] : 0.0;
      F[i][j] = in ? prm.F[3 * i + j] : 0.0;
      U[i][j] = in ? prm.U[3 * i + j] : 0.0;
    }
  }
  double time = st[12], lastT = st[13];
  long tb = t_begin ? (long)t_begin[s] : 0;
  tb = tb < 0 ? 0 : tb;
  const double sigma = prm.sigmaV2, isigma = 1.0 / prm.sigmaV2;

  for (long t0 = 0; t0 < T; t0 += tile) {
    const int nt = (int)((T - t0) < (long)tile ? (T - t0) : (long)tile);
    __syncthreads();                                                 // the previous tile has been read
    for (int idx = lane; idx < P * tile; idx += TRACK_LANES) {
      const int p = idx / tile, tt = idx - p * tile;
      if (tt < nt) {
        const long g = in0 + (long)p * T + t0 + tt;
        s_lag[tt * P + p] = lag[g];
        s_height[tt * P + p] = height[g];
      }
    }
    __syncthreads();

    for (int tt = 0; tt < nt; ++tt) {
      const long t = t0 + tt;
      int fl = 0;
      if (t >= tb) {
        fl = BTK_EKF_TRACKED;
        double xp[3];
        mat_vec(F, x, xp);                                            // predict (lib/pykalman.py:107-111)
        // what the model needs of xp, the same in every lane
        double tr[6] = {0, 0, 0, 0, 0, 0};
        if (prm.model == BTK_EKF_MODEL_LINEAR) {
          tr[0] = cos(xp[0]);
          tr[1] = sin(xp[0]);
        } else if (prm.model == BTK_EKF_MODEL_CIRCULAR) {
          tr[0] = sin(xp[0]); tr[1] = cos(xp[0]); tr[2] = sin(xp[1]); tr[3] = cos(xp[1]);
        }
        double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0, b0 = 0, b1 = 0, b2 = 0, ss = 0, cnt = 0;
        for (int p = lane; p < P; p += TRACK_LANES) {
          const int lg = s_lag[tt * P + p];
          const float hh = s_height[tt * P + p];
          if ((double)hh > prm.threshold && lg != BTK_TDOA_NO_PEAK) {
            const double* g = s_geom + 6 * p;
            double tau, h0, h1 = 0.0, h2 = 0.0;
            if (prm.model == BTK_EKF_MODEL_LINEAR) {
              // FarfieldLinearArrayTDOAFeatureVector.tdoa / linearize: baseline cos(azimuth) / c, -baseline sin(azimuth) / c
              tau = g[0] * tr[0] / prm.c;
              h0 = -g[0] * tr[1] / prm.c;
            } else if (prm.model == BTK_EKF_MODEL_CIRCULAR) {
              // FarfieldCircularArrayTDOAFeatureVector: u . offset / c with u = (sin th cos ph, sin th sin ph, cos th)
              const double st_ = tr[0], ct = tr[1], sp = tr[2], cp = tr[3];
              tau = (st_ * cp * g[0] + st_ * sp * g[1] + ct * g[2]) / prm.c;
              h0 = (ct * cp * g[0] + ct * sp * g[1] + -st_ * g[2]) / prm.c;
              h1 = (-st_ * sp * g[0] + st_ * cp * g[1] + 0.0 * g[2]) / prm.c;
            } else {
              // TDOAFeatureVector: (|x - m1| - |x - m2|) / c, ((x - m1) / |x - m1| - (x - m2) / |x - m2|) / c
              const double d10 = xp[0] - g[0], d11 = xp[1] - g[1], d12 = xp[2] - g[2];
              const double d20 = xp[0] - g[3], d21 = xp[1] - g[4], d22 = xp[2] - g[5];
              const double r1 = sqrt(d10 * d10 + d11 * d11 + d12 * d12), r2 = sqrt(d20 * d20 + d21 * d21 + d22 * d22);
              tau = (r1 - r2) / prm.c;
              h0 = (d10 / r1 - d20 / r2) / prm.c;
              h1 = (d11 / r1 - d21 / r2) / prm.c;
              h2 = (d12 / r1 - d22 / r2) / prm.c;
            }
            const double delay = (double)lg * prm.Ts;                 // TDOAFeature.next (lib/pytdoa.py:112)
            const double hx = h0 * xp[0] + h1 * xp[1] + h2 * xp[2];
            const double y = delay - (tau - hx);                      // calc_linearized_observation
            const double sv = y - hx;                                 // calc_innovation (lib/pykalman.py:91-92)
            a00 += h0 * h0; a01 += h0 * h1; a02 += h0 * h2; a11 += h1 * h1; a12 += h1 * h2; a22 += h2 * h2;
            b0 += h0 * sv; b1 += h1 * sv; b2 += h2 * sv;
            ss += sv * sv;
            cnt += 1.0;
          }
        }
        a00 = wave_sum(a00); a01 = wave_sum(a01); a02 = wave_sum(a02); a11 = wave_sum(a11); a12 = wave_sum(a12);
        a22 = wave_sum(a22); b0 = wave_sum(b0); b1 = wave_sum(b1); b2 = wave_sum(b2); ss = wave_sum(ss); cnt = wave_sum(cnt);

        if (cnt >= (double)prm.minimum_pairs) {
          fl |= BTK_EKF_OBSERVED;
          const double A[3][3] = {{a00, a01, a02}, {a01, a11, a12}, {a02, a12, a22}};
          const double b[3] = {b0, b1, b2};
          const double el = (time - lastT) * prm.time_delta, el2 = el * el;
          double FK[3][3], Kp[3][3], Ft[3][3];
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) Ft[i][j] = F[j][i];
          mat_mul(F, K, FK);
          mat_mul(FK, Ft, Kp);
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) Kp[i][j] += el2 * U[i][j];    // K_predict (lib/pykalman.py:147)
          double Mi[3][3], M[3][3], W[3][3];
          mat_mul(A, Kp, Mi);
#pragma unroll
          for (int i = 0; i < 3; ++i) Mi[i][i] += i < n ? sigma : 1.0;
          mat_inv(Mi, M);
          mat_mul(Kp, M, W);                                          // W = Kp M: G = W H^T
          double Wb[3];
          mat_vec(W, b, Wb);
          const double d2 = (ss - (b[0] * Wb[0] + b[1] * Wb[1] + b[2] * Wb[2])) * isigma;
          // scipy.stats.chi.cdf(d2, nobs) of the reference (lib/pykalman.py:98-102): the chi distribution at the squared
          // distance.  update() asks it whatever gate_prob is (:150), so gate_prob 0 filters every innovation with cdf > 0.
          const double cdf = d2 > 0.0 ? track_gammainc(0.5 * cnt, 0.5 * d2 * d2) : 0.0;
          const bool gated = cdf > prm.gate_prob;
          if (!gated) {
            fl |= BTK_EKF_UPDATED;
            double xn[3];
            if (prm.type == BTK_EKF_TYPE_IEKF) {
              double eta[3] = {xp[0], xp[1], xp[2]};
              int rounds = 0;
              for (int it = 0; it < prm.num_iterations; ++it) {
                double v[3] = {b[0], b[1], b[2]};
                if (it > 0) {                                         // zeta = s - H (xp - eta): H^T zeta = b - A (xp - eta)
                  const double dx[3] = {xp[0] - eta[0], xp[1] - eta[1], xp[2] - eta[2]};
                  double Adx[3];
                  mat_vec(A, dx, Adx);
                  v[0] -= Adx[0]; v[1] -= Adx[1]; v[2] -= Adx[2];
                }
                double Wv[3];
                mat_vec(W, v, Wv);
                double diff2 = 0.0;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                  const double e = xp[i] + Wv[i], d = e - eta[i];
                  diff2 += d * d;
                  eta[i] = e;
                }
                rounds = it + 1;
                if (diff2 < prm.iteration_threshold) break;
              }
              fl |= rounds << BTK_EKF_ROUNDS_SHIFT;
#pragma unroll
              for (int i = 0; i < 3; ++i) xn[i] = eta[i];
            } else {
#pragma unroll
              for (int i = 0; i < 3; ++i) xn[i] = xp[i] + Wb[i];
            }
            adjust_boundaries(xn, n);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
              x[i] = xn[i];
#pragma unroll
              for (int j = 0; j < 3; ++j) K[i][j] = sigma * W[i][j];  // (I - G H) Kp = sigmaV2 Kp M
            }
            lastT = time;
          }
        }
        time += 1.0;
      }
      if (lane == 0) {
        const long o = (long)s * T + t;
        flags[o] = fl;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          xk[3 * o + i] = x[i];
#pragma unroll
          for (int j = 0; j < 3; ++j) Kf[9 * o + 3 * i + j] = K[i][j];
        }
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      st[i] = x[i];
#pragma unroll
      for (int j = 0; j < 3; ++j) st[3 + 3 * i + j] = K[i][j];
    }
    st[12] = time;
    st[13] = lastT;
  }
}

}  // namespace

extern "C" {

int btk_ekf_track(const btk_ekf_params* params, const void* lag, const void* height, const void* geom, const void* t_begin,
                  int S, int P, long T, void* state, void* xk, void* Kf, void* flags, void* stream)
{
  if (!params || !lag || !height || !geom || !state || !xk || !Kf || !flags)
    return btk_set_error(BTK_ERR_PARAMETER, "btk_ekf_track: null argument");
  const btk_ekf_params& q = *params;
  if (q.n < 1 || q.n > 3) return btk_set_error(BTK_ERR_PARAMETER, "btk_ekf_track: state length n=%d, need 1 .. 3", q.n);
  if (q.model != BTK_EKF_MODEL_LINEAR && q.model != BTK_EKF_MODEL_CIRCULAR && q.model != BTK_EKF_MODEL_CARTESIAN)
    return btk_set_error(BTK_ERR_PARAMETER, "btk_ekf_track: model %d", q.model);
  const int need = q.model == BTK_EKF_MODEL_LINEAR ? 1 : q.model == BTK_EKF_MODEL_CIRCULAR ? 2 : 3;
  if (q.n != need) return btk_set_error(BTK_ERR_PARAMETER, "btk_ekf_track: model %d has %d state variables, n=%d", q.model, need, q.n);
  if (q.type != BTK_EKF_TYPE_EKF && q.type != BTK_EKF_TYPE_IEKF) return btk_set_error(BTK_ERR_PARAMETER, "btk_ekf_track: type %d", q.type);
  if (q.type == BTK_EKF_TYPE_IEKF && (q.num_iterations < 1 || q.num_iterations > BTK_EKF_MAX_ROUNDS))
    return btk_set_error(BTK_ERR_PARAMETER, "btk_ekf_track: num_iterations=%d, need 1 .. %d", q.num_iterations, BTK_EKF_MAX_ROUNDS);
  if (!(q.sigmaV2 > 0.0) || !std::isfinite(q.sigmaV2)) return btk_set_error(BTK_ERR_PARAMETER, "btk_ekf_track: sigmaV2=%g must be positive", q.sigmaV2);
  if (!(q.c > 0.0) || !std::isfinite(q.Ts) || !std::isfinite(q.time_delta) || !std::isfinite(q.threshold))
    return btk_set_error(BTK_ERR_PARAMETER, "btk_ekf_track: c=%g Ts=%g time_delta=%g threshold=%g", q.c, q.Ts, q.time_delta, q.threshold);
  if (!(q.gate_prob >= 0.0 && q.gate_prob <= 1.0)) return btk_set_error(BTK_ERR_PARAMETER, "btk_ekf_track: gate_prob=%g outside [0, 1]", q.gate_prob);
  if (q.minimum_pairs < 1) return btk_set_error(BTK_ERR_PARAMETER, "btk_ekf_track: minimum_pairs=%d, need at least 1", q.minimum_pairs);
  if (S < 1 || P < 1 || T < 1) return btk_set_error(BTK_ERR_DIMENSION, "btk_ekf_track: S=%d P=%d T=%ld", S, P, T);
  const long per_pair = 48 + 8;                                      // geometry + one frame of lag and height
  if ((long)P * per_pair > TRACK_LDS_BYTES)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_ekf_track: P=%d pairs, at most %ld", P, TRACK_LDS_BYTES / per_pair);
  if ((long)S * P * T > 0x7fffffffffffL / 8) return btk_set_error(BTK_ERR_DIMENSION, "btk_ekf_track: S=%d P=%d T=%ld", S, P, T);
  long tile = (TRACK_LDS_BYTES - 48L * P) / (8L * P);
  tile = tile > TRACK_MAX_TILE ? TRACK_MAX_TILE : tile;
  tile = tile > T ? T : tile;
  const size_t lds = (size_t)P * (48 + 8 * (size_t)tile);
  hipLaunchKernelGGL(ekf_track_kernel, dim3((unsigned)S), dim3(TRACK_LANES), lds, as_stream(stream), q,
                     reinterpret_cast<const int*>(lag), reinterpret_cast<const float*>(height),
                     reinterpret_cast<const double*>(geom), reinterpret_cast<const int*>(t_begin), P, T, (int)tile,
                     reinterpret_cast<double*>(state), reinterpret_cast<double*>(xk), reinterpret_cast<double*>(Kf),
                     reinterpret_cast<int*>(flags));
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

}  // extern "C"
