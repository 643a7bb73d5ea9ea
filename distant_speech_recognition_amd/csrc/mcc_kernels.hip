// mcc_kernels.hip -- multichannel cross-correlation localisation on the samples themselves (gfx950).
//
// MCCLocalizer::calcCovarianceMatrix / doEigenValueDecomposition / calcObjectiveFunction / search (reference
// localization/mcc_localizer.cc:322-360, :362-411, :413-451), batched over streams, blocks and grid candidates: for every stream s,
// block b of L samples and candidate g with the sample delays tau[g][0..N)
//     R    = (1 / nS) sum_{f=0}^{nS-1} xt[f] xt[f]^T        nS = L - D,   xt_c[f] = x_c[f + tau_c]  (f + tau_c >= 0)
//                                                                                   x_c[L + f + tau_c]  (otherwise: SampleHolder
//                                                           is filled from the CURRENT block at :336, so the "previous" samples
//                                                           are the block's own last D, and no state crosses a block boundary)
//     cost = sum_j log d_j - sum_i log R_ii                 d_j: the pivots of R = L diag(d) L^T, i.e. sum log lambda_j(R)
//
//   mcc_cost_kernel   : one workgroup of four wavefronts per (stream, block, candidate).  The SYRK runs on v_mfma_f64_16x16x4_f64:
//                       for X X^T the A operand A[i = lane & 15][k = lane >> 4] and the B operand B[k = lane >> 4][j = lane & 15]
//                       of a tile pair are the same lane values (channel lane & 15 of the tile, sample lane >> 4 of the step), so
//                       a step of four samples costs one float load per 16-channel tile and lane, taken from global memory with the
//                       candidate's delay already in the address, and feeds the NT (NT + 1) / 2 tiles of the lower triangle.  The
//                       float32 samples become float64 exactly; their products are exact in float64.  Wavefront w sums the w-th
//                       quarter of the steps in step order; the four partial matrices are then added in LDS in the order
//                       ((w0 + w1) + w2) + w3.  Quarter and order depend on (N, L, D) alone -- not on S, B, G or the other
//                       candidates of a launch -- and there are no atomics: equal tau rows give equal bits.
//                       The determinant comes from an in-LDS LDL^T (the Cholesky without its square roots: L_jj^2 = d_j, so
//                       2 sum log L_jj = sum log d_j), right-looking, one barrier per column, rows on lanes.
//                       A pivot or an R_ii that is not > 0 gives cost 0.0 and flag 1 (the zero-eigenvalue branch of :386-397).
//                       With a pair list the same kernel writes R (mirrored) for the listed (block, candidate) pairs instead.
//   mcc_select_kernel : the N-best insertion of :431-443 (strict <, every entry starts at 100000), one lane per (stream, block).
//
// Host code of this file: the reference's float arithmetic for D, tau and the far-field walk of SGB4LinearArray (:54-161).
#include <cmath>
#include <vector>
#include "btk_internal.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int MCC_MAX_N = 64;
constexpr int MCC_MAX_G = 4096;
constexpr int MCC_MAX_L = 65536;
constexpr int MCC_MAX_NBEST = 16;
constexpr int MCC_WAVES = 4;           // wavefronts per work unit; each sums a quarter of the steps
constexpr int MCC_UNROLL = 4;          // steps of four samples whose loads are issued together
constexpr double MCC_RESET_COST = 100000.0;     // SourceCandidate's initial cost (mcc_localizer.h:155)

// grid: one workgroup per work unit.  pairs == null: unit = (s B + b) G + g, writes cost / flag.  pairs != null: unit p is
// (sb, g) = pairs[p], writes Rout [p][N][N].
template <int NT>
__global__ __launch_bounds__(64 * MCC_WAVES)
void mcc_cost_kernel(const float* __restrict__ x, long len, int N, int B, int L, int D, const int* __restrict__ tau, int G,
                     const int* __restrict__ pairs, int normalize, double* __restrict__ cost, unsigned char* __restrict__ flag,
                     double* __restrict__ Rout)
{
  constexpr int NP = 16 * NT, LD = NP + 1, NTRI = NT * (NT + 1) / 2;
  __shared__ double Rs[NP * LD];
  __shared__ double dg[NP], piv[NP];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ch = lane & 15, kq = lane >> 4;
  long sb;
  int g;
  if (pairs) { sb = pairs[2 * blockIdx.x]; g = pairs[2 * blockIdx.x + 1]; }
  else { sb = blockIdx.x / G; g = blockIdx.x % G; }
  const long s = sb / B, b = sb % B;

  const float* px[NT];
  int tc[NT];
  bool live[NT];
#pragma unroll
  for (int i = 0; i < NT; i++) {
    const int c = 16 * i + ch;
    live[i] = c < N;
    const int cc = live[i] ? c : 0;
    px[i] = x + (s * N + cc) * len + b * L;
    tc[i] = tau[(long)g * N + cc];
  }

  f64x4 acc[NTRI];
#pragma unroll
  for (int t = 0; t < NTRI; t++) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};

  const int nS = L - D, nsteps = (nS + 3) / 4, per = (nsteps + MCC_WAVES - 1) / MCC_WAVES;
  const int st0 = wave * per, st1 = min(nsteps, st0 + per);
  for (int st = st0; st < st1; st += MCC_UNROLL) {
    double a[MCC_UNROLL][NT];
#pragma unroll
    for (int u = 0; u < MCC_UNROLL; u++) {
      const int f = (st + u) * 4 + kq;
      const bool in = st + u < st1 && f < nS;
#pragma unroll
      for (int i = 0; i < NT; i++) {
        int idx = f + tc[i];
        idx += idx < 0 ? L : 0;                          // the block's own tail stands for the previous block (:336, :350-352)
        float v = 0.f;
        if (in && live[i] && (unsigned)idx < (unsigned)L) v = px[i][idx];
        a[u][i] = (double)v;
      }
    }
#pragma unroll
    for (int u = 0; u < MCC_UNROLL; u++) {
      int t = 0;
#pragma unroll
      for (int i = 0; i < NT; i++)
#pragma unroll
        for (int j = 0; j <= i; j++, t++) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][i], a[u][j], acc[t], 0, 0, 0);
    }
  }

  // C/D of the f64 instruction: col = lane & 15, row = (lane >> 4) + 4 reg.  The partial sums are added wavefront after wavefront.
#pragma unroll
  for (int w = 0; w < MCC_WAVES; w++) {
    if (wave == w) {
      int t = 0;
#pragma unroll
      for (int i = 0; i < NT; i++)
#pragma unroll
        for (int j = 0; j <= i; j++, t++)
#pragma unroll
          for (int r = 0; r < 4; r++) {
            double* p = &Rs[(16 * i + kq + 4 * r) * LD + 16 * j + ch];
            *p = w == 0 ? acc[t][r] : *p + acc[t][r];
          }
    }
    __syncthreads();
  }

  // gsl_matrix_scale(R, 1.0 / nSamples) (:357); only the lower triangle is used from here on
  const double inv = 1.0 / (double)nS;
  for (int e = tid; e < NP * NP; e += 64 * MCC_WAVES) {
    const int r = e / NP, c = e % NP;
    if (c <= r) Rs[r * LD + c] *= inv;
  }
  __syncthreads();
  if (Rout) {
    double* Ro = Rout + (long)blockIdx.x * N * N;
    for (int e = tid; e < N * N; e += 64 * MCC_WAVES) {
      const int r = e / N, c = e % N;
      Ro[e] = c <= r ? Rs[r * LD + c] : Rs[c * LD + r];
    }
    return;                                              // block-uniform
  }
  int bad = 0;
  if (tid < N) {
    const double v = Rs[tid * LD + tid];
    dg[tid] = v;
    bad = !(v > 0.0);
  }
  bad = __syncthreads_or(bad);

  // R = L diag(d) L^T in place: after step j column j holds d_j L_ij (never written again), the trailing block is updated
  // as R_ik -= (R_ij / d_j) R_kj.  Row i on lane i, the columns of a row dealt over the four wavefronts.
  if (!bad) {
    for (int j = 0; j < N; j++) {
      const double d = Rs[j * LD + j];
      if (!(d > 0.0)) { bad = 1; break; }                // every thread reads the same value
      if (tid == 0) piv[j] = d;
      const int i = lane;
      if (i > j && i < N) {
        const double lij = Rs[i * LD + j] / d;
        for (int k = j + 1 + wave; k <= i; k += MCC_WAVES) Rs[i * LD + k] = fma(-lij, Rs[k * LD + j], Rs[i * LD + k]);
      }
      __syncthreads();
    }
  }
  if (bad) {
    if (tid == 0) { cost[blockIdx.x] = 0.0; flag[blockIdx.x] = 1; }
    return;
  }
  if (tid < N) { piv[tid] = log(piv[tid]); dg[tid] = log(dg[tid]); }
  __syncthreads();
  if (tid == 0) {
    double ld = 0.0, ln = 0.0;
    for (int j = 0; j < N; j++) { ld += piv[j]; ln += dg[j]; }
    cost[blockIdx.x] = normalize ? ld - ln : ld;
    flag[blockIdx.x] = 0;
  }
}

// grid: ceil(SB / 256); one lane per (stream, block).  nbest_cost keeps 100000 and nbest_idx -1 where nothing was inserted.
__global__ __launch_bounds__(256)
void mcc_select_kernel(const double* __restrict__ cost, long SB, int G, int nbest, double* __restrict__ nb_cost,
                       int* __restrict__ nb_idx)
{
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= SB) return;
  double v[MCC_MAX_NBEST];
  int ix[MCC_MAX_NBEST];
#pragma unroll
  for (int j = 0; j < MCC_MAX_NBEST; j++) { v[j] = MCC_RESET_COST; ix[j] = -1; }
  for (int g = 0; g < G; g++) {
    double cv = cost[q * G + g];
    int ci = g;
    bool ins = false;
#pragma unroll
    for (int j = 0; j < MCC_MAX_NBEST; j++) {
      if (j < nbest && (ins || cv < v[j])) {             // the first strictly larger entry takes it, the rest shift down
        const double tv = v[j]; const int ti = ix[j];
        v[j] = cv; ix[j] = ci; cv = tv; ci = ti; ins = true;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < MCC_MAX_NBEST; j++)
    if (j < nbest) { nb_cost[q * nbest + j] = v[j]; nb_idx[q * nbest + j] = ix[j]; }
}

int mcc_check(const char* who, long len, int S, int N, int B, int L, int D, const int* tau_host, int G)
{
  if (N < 2 || N > MCC_MAX_N) return btk_set_error(BTK_ERR_DIMENSION, "%s: N=%d channels, need 2 .. %d", who, N, MCC_MAX_N);
  if (G < 1 || G > MCC_MAX_G) return btk_set_error(BTK_ERR_DIMENSION, "%s: G=%d candidates, need 1 .. %d", who, G, MCC_MAX_G);
  if (D < 0 || L < 1 || L > MCC_MAX_L || (long)L < 2L * D)
    return btk_set_error(BTK_ERR_DIMENSION, "%s: Data samples are insufficient (L=%d, D=%d; need 2 D <= L <= %d)", who, L, D, MCC_MAX_L);
  if (S < 1 || B < 1 || (long)B * L > len || (long)S * B * G > 0x7fffffffL)
    return btk_set_error(BTK_ERR_DIMENSION, "%s: bad sizes S=%d B=%d L=%d len=%ld G=%d", who, S, B, L, len, G);
  if (!tau_host) return btk_set_error(BTK_ERR_PARAMETER, "%s: null tau", who);
  for (long e = 0; e < (long)G * N; e++)
    if (tau_host[e] < -D || tau_host[e] > D)
      return btk_set_error(BTK_ERR_DIMENSION, "%s: tau[%ld][%ld]=%d outside -D .. D (D=%d)", who, e / N, e % N, tau_host[e], D);
  return BTK_OK;
}

void mcc_launch(int units, hipStream_t st, const float* x, long len, int N, int B, int L, int D, const int* tau, int G,
                const int* pairs, int normalize, double* cost, unsigned char* flag, double* Rout)
{
#define MCC_GO(NT)                                                                                                         \
  hipLaunchKernelGGL((mcc_cost_kernel<NT>), dim3((unsigned)units), dim3(64 * MCC_WAVES), 0, st, x, len, N, B, L, D, tau, G, \
                     pairs, normalize, cost, flag, Rout)
  switch ((N + 15) / 16) {
    case 1: MCC_GO(1); break;
    case 2: MCC_GO(2); break;
    case 3: MCC_GO(3); break;
    default: MCC_GO(4); break;
  }
#undef MCC_GO
}

}  // namespace

extern "C" {

// maxSampleDelay of MCCLocalizer (:273, :326): unsigned x float is a float product, truncated
long btk_mcc_max_sample_delay(unsigned int fs, float max_time_delay)
{
  const float p = fs * max_time_delay;
  return p > 0.f ? (long)(size_t)p : 0;
}

// _tau of calcCovarianceMatrix (:333-335): the double product rounded to float, then truncated toward zero
int btk_mcc_sample_delays(unsigned int fs, int n, const double* delays, int* tau_out)
{
  if (n < 1) return btk_set_error(BTK_ERR_DIMENSION, "btk_mcc_sample_delays: n=%d", n);
  if (!delays || !tau_out) return btk_set_error(BTK_ERR_PARAMETER, "btk_mcc_sample_delays: null argument");
  for (int c = 0; c < n; c++) {
    const float tau_l = fs * delays[c];
    tau_out[c] = (int)tau_l;
  }
  return BTK_OK;
}

// SGB4LinearArray (:54-161) and calcDelaysOfLinearMicrophoneArray (localization.cc:107-118), far field
int btk_mcc_linear_grid(unsigned int fs, int N, const double* positions, float distance, int max_points, int* n_points,
                        float* max_time_delay, float* const_v, double* azimuths, double* delays, int* tau)
{
  const double SSPEED = 343740.0, TPI = 6.28318530717958647692;
  if (N < 2) return btk_set_error(BTK_ERR_DIMENSION, "btk_mcc_linear_grid: N=%d microphones, need at least 2", N);
  if (!n_points) return btk_set_error(BTK_ERR_PARAMETER, "btk_mcc_linear_grid: null argument");
  std::vector<double> ypos((size_t)N);
  float constV, maxTimeDelay;
  if (positions) {                                       // setPositionsOfMicrophones (:68-100); microphone 0 is pos0 here
    float maxDist = -1;
    const float p0[3] = {(float)positions[0], (float)positions[1], (float)positions[2]};
    for (int m = 0; m < N; m++) {
      ypos[m] = positions[3 * m + 1];
      if (m == 0) continue;
      const float dx = p0[0] - (float)positions[3 * m], dy = p0[1] - (float)positions[3 * m + 1], dz = p0[2] - (float)positions[3 * m + 2];
      const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
      if (dist > maxDist) maxDist = dist;
    }
    if (!(maxDist > 0.f)) return btk_set_error(BTK_ERR_PARAMETER, "btk_mcc_linear_grid: all microphones at one point");
    constV = 0.99 * SSPEED / (maxDist * fs);
    maxTimeDelay = maxDist / SSPEED;
  } else {                                               // setDistanceBtwMicrophones (:54-66)
    if (!(distance > 0.f)) return btk_set_error(BTK_ERR_PARAMETER, "btk_mcc_linear_grid: distance=%g", (double)distance);
    const size_t nMic = (size_t)N;
    for (size_t m = 0; m < nMic; m++) ypos[m] = m * distance;
    constV = 0.99 * SSPEED / ((nMic - 1) * distance * fs);
    maxTimeDelay = (nMic - 1) * distance / SSPEED;
  }
  if (max_time_delay) *max_time_delay = maxTimeDelay;
  if (const_v) *const_v = constV;

  float azimuth = 0.f;                                   // SearchGridBuilder::reset (:31-36); _hypopos holds float values
  int n = 0;
  for (;;) {
    if (n >= MCC_MAX_G) return btk_set_error(BTK_ERR_DIMENSION, "btk_mcc_linear_grid: more than %d grid points", MCC_MAX_G);
    if (azimuths || delays || tau) {
      if (n >= max_points) return btk_set_error(BTK_ERR_DIMENSION, "btk_mcc_linear_grid: more than max_points=%d grid points", max_points);
      if (azimuths) azimuths[n] = (double)azimuth;
      for (int i = 0; i < N; i++) {                      // localization.cc:111-115
        double delayi = 0.0;
        if (i > 0) {
          const float dist = fabs(ypos[i] - ypos[0]);
          delayi = -dist * sin((double)azimuth) / SSPEED;
        }
        if (delays) delays[(size_t)n * N + i] = delayi;
        if (tau) { const float tau_l = fs * delayi; tau[(size_t)n * N + i] = (int)tau_l; }
      }
    }
    n++;
    // nextSearchGridFF (:119-148)
    const float oldSin = sinf(azimuth);
    float newAzimuth, newSin;
    if (azimuth < M_PI_2) {
      newSin = oldSin + constV;
      if (newSin >= 1) newAzimuth = M_PI_2;
      else newAzimuth = asinf(newSin);
    } else if (azimuth < (3 * M_PI_2)) {
      newAzimuth = 3 * M_PI_2;
    } else {
      newSin = oldSin + constV;
      if ((newSin + constV / 2.0) >= 0) break;
      newAzimuth = TPI + asinf(newSin);
    }
    azimuth = newAzimuth;
  }
  *n_points = n;
  return BTK_OK;
}

int btk_mcc_cost(const void* x, long len, int S, int N, int B, int L, int D, const int* tau_host, void* tau_dev, int G,
                 int normalize_variance, void* cost, void* flag, void* stream)
{
  const int rc = mcc_check("btk_mcc_cost", len, S, N, B, L, D, tau_host, G);
  if (rc != BTK_OK) return rc;
  if (!x || !tau_dev || !cost || !flag) return btk_set_error(BTK_ERR_PARAMETER, "btk_mcc_cost: null argument");
  BTK_HIP_CHECK(hipMemcpyAsync(tau_dev, tau_host, sizeof(int) * (size_t)G * N, hipMemcpyHostToDevice, as_stream(stream)));
  mcc_launch(S * B * G, as_stream(stream), static_cast<const float*>(x), len, N, B, L, D, static_cast<const int*>(tau_dev), G,
             nullptr, normalize_variance, static_cast<double*>(cost), static_cast<unsigned char*>(flag), nullptr);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

int btk_mcc_select(const void* cost, long SB, int G, int nbest, void* nbest_cost, void* nbest_idx, void* stream)
{
  if (nbest < 1 || nbest > MCC_MAX_NBEST)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_mcc_select: maxSource=%d, need 1 .. %d", nbest, MCC_MAX_NBEST);
  if (SB < 1 || G < 1 || G > MCC_MAX_G) return btk_set_error(BTK_ERR_DIMENSION, "btk_mcc_select: bad sizes SB=%ld G=%d", SB, G);
  if (!cost || !nbest_cost || !nbest_idx) return btk_set_error(BTK_ERR_PARAMETER, "btk_mcc_select: null argument");
  hipLaunchKernelGGL(mcc_select_kernel, dim3((unsigned)((SB + 255) / 256)), dim3(256), 0, as_stream(stream),
                     static_cast<const double*>(cost), SB, G, nbest, static_cast<double*>(nbest_cost), static_cast<int*>(nbest_idx));
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

int btk_mcc_matrices(const void* x, long len, int S, int N, int B, int L, int D, const int* tau_host, void* tau_dev, int G,
                     const int* pairs_host, void* pairs_dev, int P, void* R, void* stream)
{
  const int rc = mcc_check("btk_mcc_matrices", len, S, N, B, L, D, tau_host, G);
  if (rc != BTK_OK) return rc;
  if (P < 1) return btk_set_error(BTK_ERR_DIMENSION, "btk_mcc_matrices: P=%d pairs", P);
  if (!pairs_host) return btk_set_error(BTK_ERR_PARAMETER, "btk_mcc_matrices: null pair list");
  for (int p = 0; p < P; p++)
    if (pairs_host[2 * p] < 0 || pairs_host[2 * p] >= (long)S * B || pairs_host[2 * p + 1] < 0 || pairs_host[2 * p + 1] >= G)
      return btk_set_error(BTK_ERR_DIMENSION, "btk_mcc_matrices: pair %d = (%d, %d) outside [0, %ld) x [0, %d)", p,
                           pairs_host[2 * p], pairs_host[2 * p + 1], (long)S * B, G);
  if (!x || !tau_dev || !pairs_dev || !R) return btk_set_error(BTK_ERR_PARAMETER, "btk_mcc_matrices: null argument");
  BTK_HIP_CHECK(hipMemcpyAsync(tau_dev, tau_host, sizeof(int) * (size_t)G * N, hipMemcpyHostToDevice, as_stream(stream)));
  BTK_HIP_CHECK(hipMemcpyAsync(pairs_dev, pairs_host, sizeof(int) * 2 * (size_t)P, hipMemcpyHostToDevice, as_stream(stream)));
  mcc_launch(P, as_stream(stream), static_cast<const float*>(x), len, N, B, L, D, static_cast<const int*>(tau_dev), G,
             static_cast<const int*>(pairs_dev), 1, nullptr, nullptr, static_cast<double*>(R));
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

}  // extern "C"
