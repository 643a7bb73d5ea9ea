// srp_kernels.hip -- steered response power of a delay-and-sum beam over a grid of directions (gfx950).
//
// DOAEstimatorSRPDSBLA::next (reference beamformer/beamformer.cc:3091-3122, 3124-3191, 3221-3251) batched over the frames of a
// block: for every stream s, frame t and grid direction u
//     rp[u][t]  = sum_{k=fmin}^{fmax} c_k |sv[u][k]^H x_k[t]|^2 / (fmax - fmin + 1)        c_k = 2 (k < M/2), 1 (k = M/2)
//     energy[t] = sum_{k=fmin}^{fmax} c_k (sum_n |x_k[n][t]|^2)^2 / (M N)
// Per bin this is the complex product [U x N] . [N x T]; the beams it produces are squared and summed over the bins right out of the
// accumulator registers and never reach memory.
//
//   srp_power_kernel : v_mfma_f32_32x32x2_f32, four real products per complex one as in cov_mfma_kernel.  The B operand of the
//                      instruction is B[k = lane >> 5][j = lane & 31]: with frames on j and the channel pair on k a wavefront takes
//                      its 32-frame strip of X_k from global memory already in operand layout (256 contiguous bytes per channel row,
//                      no LDS, no barrier).  The strip of one bin (N <= 64: at most 64 VGPRs) is reused for every 32-direction tile
//                      of the pass; arrays of more than 64 channels go through it in chunks of 64 channels ONCE PER TILE, i.e. their
//                      snapshots are fetched up to four times per pass (from L2 at best) where N <= 64 fetches them once.  The
//                      power of every tile stays in registers for the whole bin loop: no atomics, a fixed summation order.
//   srp_nbest_kernel : the N-best insertion of :3157-3187 (strict >, so of equal powers the earlier grid index ranks first), one
//                      lane per frame, and the energy gate of :3148-3155.
//   srp_acc_kernel   : accRPs_ (:3162) in float64, one wavefront per (stream, direction), coalesced loads, frames added in index order.
#include "btk_internal.h"
#include "wave_ops.h"

namespace {


constexpr int SRP_FT = 32;             // frames per wavefront strip (the j extent of the 32x32x2 instruction)
constexpr int SRP_WAVES = 4;           // wavefronts (strips) per workgroup; they share nothing
constexpr int SRP_MAX_TILES = 4;       // 32-direction tiles per pass: 4 x 16 power registers + 32 beam + 64 strip registers
constexpr int SRP_MAX_NBEST = 16;

// channel pairs per bin in the packed table: the register chunk of the kernel that serves N (4, 8, 16 or a multiple of 32)
inline int srp_pairs_padded(int N)
{
  const int np = (N + 1) / 2;
  if (np <= 4) return 4;
  if (np <= 8) return 8;
  if (np <= 16) return 16;
  return (np + 31) / 32 * 32;
}
inline int srp_dirs_padded(int U) { return (U + 31) / 32 * 32; }

// grid: (ceil(T / 128), S); block 256 = 4 wavefronts, one 32-frame strip each.  TP: the packed table of btk_srp_pack_table,
// complex64 [K][PP][UP][2] with element [k][p][u][h] = sv[u][k][2 p + h] (zero beyond N and U), so that the A operand
// A[i = lane & 31][k = lane >> 5] of a tile and channel pair is one contiguous 512-byte load.
template <int NTILE, int NPAIR>
__global__ __launch_bounds__(256)
void srp_power_kernel(const float2* __restrict__ X, const float2* __restrict__ TP, float* __restrict__ rp,
                      float* __restrict__ energy, int K, int N, long T_stride, long T, int U, int UP, int PP, int u0,
                      int fmin, int fmax, int half, float nb, float edenom)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long t0 = ((long)blockIdx.x * SRP_WAVES + wave) * SRP_FT;
  if (t0 >= T) return;                                   // wave-uniform
  const int s = blockIdx.y;
  const int li = lane & 31, lk = lane >> 5;
  const long t = t0 + li;
  const bool tin = t < T;
  const int nchunk = PP / NPAIR;

  f32x16 pw[NTILE];
#pragma unroll
  for (int i = 0; i < NTILE; i++)
#pragma unroll
    for (int r = 0; r < 16; r++) pw[i][r] = 0.f;
  float en = 0.f;

  for (int k = fmin; k <= fmax; k++) {
    const float ck = k < half ? 2.f : 1.f;
    const float2* xk = X + ((long)s * K + k) * N * T_stride + t;
    const float2* tk = TP + ((long)k * PP * UP + u0 + li) * 2 + lk;
    float2 xs[NPAIR];
    float e = 0.f;
#pragma unroll
    for (int tile = 0; tile < NTILE; tile++) {
      f32x16 yr, yi;
#pragma unroll
      for (int r = 0; r < 16; r++) { yr[r] = 0.f; yi[r] = 0.f; }
      for (int c = 0; c < nchunk; c++) {
        if (tile == 0 || nchunk > 1) {                   // N <= 64: the strip loaded for the first tile serves them all
#pragma unroll
          for (int p = 0; p < NPAIR; p++) {
            const int n = 2 * (c * NPAIR + p) + lk;
            float2 v = make_float2(0.f, 0.f);
            if (tin && n < N) v = xk[(long)n * T_stride];
            xs[p] = v;
            if (tile == 0) e = fmaf(v.x, v.x, fmaf(v.y, v.y, e));
          }
        }
        const float2* tc = tk + ((long)c * NPAIR * UP + tile * 32) * 2;
#pragma unroll
        for (int p = 0; p < NPAIR; p++) {
          const float2 a = tc[(long)p * UP * 2];
          const float2 b = xs[p];
          // y = conj(a) b :  yr += ar br + ai bi ,  yi += ar bi - ai br
          yr = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, yr, 0, 0, 0);
          yr = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, yr, 0, 0, 0);
          yi = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.y, yi, 0, 0, 0);
          yi = __builtin_amdgcn_mfma_f32_32x32x2f32(-a.y, b.x, yi, 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; r++) pw[tile][r] = fmaf(ck, fmaf(yr[r], yr[r], yi[r] * yi[r]), pw[tile][r]);
    }
    e += __shfl_xor(e, 32);                              // the two channel halves of the frame
    en = fmaf(ck, e * e, en);
  }

  // C/D layout of 32x32: col = lane & 31 (frame), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (direction)
  if (tin) {
#pragma unroll
    for (int tile = 0; tile < NTILE; tile++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int u = u0 + tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        if (u < U) rp[((long)s * U + u) * T + t] = pw[tile][r] / nb;
      }
    if (u0 == 0 && lk == 0) energy[(long)s * T + t] = en / edenom;
  }
}

// grid: (ceil(T / 256), S).  The list is kept in float64 like the reference's nBestRPs_ (a gsl_vector), so that the reset value
// -10e10 compares as it does there; the values that come out are the float32 powers themselves.
__global__ __launch_bounds__(256)
void srp_nbest_kernel(const float* __restrict__ rp, const float* __restrict__ energy, float threshold, int nbest,
                      float* __restrict__ nb_rp, int* __restrict__ nb_idx, int* __restrict__ gate, int U, long T)
{
  const int s = blockIdx.y;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  double v[SRP_MAX_NBEST];
  int ix[SRP_MAX_NBEST];
#pragma unroll
  for (int j = 0; j < SRP_MAX_NBEST; j++) { v[j] = -10e10; ix[j] = -1; }
  const int g = energy[(long)s * T + t] < threshold ? 0 : 1;
  if (g) {
    for (int u = 0; u < U; u++) {
      double cv = (double)rp[((long)s * U + u) * T + t];
      int ci = u;
      bool ins = false;
#pragma unroll
      for (int j = 0; j < SRP_MAX_NBEST; j++) {
        if (j < nbest && (ins || cv > v[j])) {           // the first strictly smaller entry takes it, the rest shift down
          const double tv = v[j]; const int ti = ix[j];
          v[j] = cv; ix[j] = ci; cv = tv; ci = ti; ins = true;
        }
      }
    }
  }
  gate[(long)s * T + t] = g;
#pragma unroll
  for (int j = 0; j < SRP_MAX_NBEST; j++)
    if (j < nbest) {
      nb_rp[((long)s * T + t) * nbest + j] = (float)v[j];
      nb_idx[((long)s * T + t) * nbest + j] = ix[j];
    }
}

// grid: (U, S), one wavefront per (stream, direction): acc[s][u] += gate[t] rp[u][t] for t = 0, 1, ... in frame order, the order of
// the reference's per-frame `accRPs_ += rp` (:3162) -- so the sum does not depend on how an utterance is cut into blocks.  The
// lanes fetch 64 consecutive frames in one coalesced load; the additions then run over the lanes in index order (every lane keeps
// the same sum).  A gated frame adds 0.0, which leaves a float64 sum as it is.
__global__ __launch_bounds__(64)
void srp_acc_kernel(const float* __restrict__ rp, const int* __restrict__ gate, double* __restrict__ acc, int U, long T)
{
  const int u = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
  const float* r = rp + ((long)s * U + u) * T;
  const int* g = gate + (long)s * T;
  double sum = acc[(long)s * U + u];
  for (long t0 = 0; t0 < T; t0 += 64) {
    const long t = t0 + lane;
    const bool in = t < T && g[t] != 0;
    const int bits = __float_as_int(in ? r[t] : 0.f);
    const unsigned long long mask = __ballot(in);
#pragma unroll
    for (int i = 0; i < 64; i++) {
      const float x = __int_as_float(__builtin_amdgcn_readlane(bits, i));
      sum += ((mask >> i) & 1ull) ? (double)x : 0.0;
    }
  }
  if (lane == 0) acc[(long)s * U + u] = sum;
}

template <int NPAIR>
void srp_launch_tiles(int ntile, dim3 grid, hipStream_t st, const float2* X, const float2* TP, float* rp, float* energy, int K,
                      int N, long T_stride, long T, int U, int UP, int PP, int u0, int fmin, int fmax, int half, float nb,
                      float edenom)
{
#define SRP_GO(NT)                                                                                                          \
  hipLaunchKernelGGL((srp_power_kernel<NT, NPAIR>), grid, dim3(64 * SRP_WAVES), 0, st, X, TP, rp, energy, K, N, T_stride, \
                     T, U, UP, PP, u0, fmin, fmax, half, nb, edenom)
  switch (ntile) {
    case 1: SRP_GO(1); break;
    case 2: SRP_GO(2); break;
    case 3: SRP_GO(3); break;
    default: SRP_GO(4); break;
  }
#undef SRP_GO
}

}  // namespace

extern "C" {

long btk_srp_packed_elems(int U, int K, int N)
{
  if (U < 1 || K < 1 || N < 1) return 0;
  return (long)K * srp_pairs_padded(N) * srp_dirs_padded(U) * 2;
}

// host: table complex128 [U][K][N] (btk_srp_table) -> the kernel's operand order, complex64 [K][PP][UP][2]
int btk_srp_pack_table(const double* table, int U, int K, int N, float* packed)
{
  if (!table || !packed) return btk_set_error(BTK_ERR_PARAMETER, "btk_srp_pack_table: null argument");
  if (U < 1 || K < 1 || N < 1) return btk_set_error(BTK_ERR_DIMENSION, "btk_srp_pack_table: U=%d K=%d N=%d", U, K, N);
  const int PP = srp_pairs_padded(N), UP = srp_dirs_padded(U);
  for (int k = 0; k < K; k++)
    for (int p = 0; p < PP; p++)
      for (int u = 0; u < UP; u++)
        for (int h = 0; h < 2; h++) {
          const int n = 2 * p + h;
          const size_t o = ((((size_t)k * PP + p) * UP + u) * 2 + h) * 2;
          const bool in = u < U && n < N;
          const size_t i = (((size_t)u * K + k) * N + n) * 2;
          packed[o] = in ? (float)table[i] : 0.f;
          packed[o + 1] = in ? (float)table[i + 1] : 0.f;
        }
  return BTK_OK;
}

// DOAEstimatorSRPDSBLA::calc_response_power_ for every grid direction and frame of a block + calc_energy
// (beamformer.cc:3091-3122, 3221-3251)
int btk_srp_power(const void* X, const void* table_packed, void* rp, void* energy, int S, int M, int N, long T_stride, long T,
                  int U, int fbin_min, int fbin_max, void* stream)
{
  if (M < 2 || (M & (M - 1))) return btk_set_error(BTK_ERR_PARAMETER, "btk_srp_power: M=%d must be a power of two", M);
  if (N < 2 || N > 256) return btk_set_error(BTK_ERR_DIMENSION, "btk_srp_power: N=%d channels, need 2 .. 256", N);
  if (S < 1 || U < 1 || T < 0 || T_stride < T)
    return btk_set_error(BTK_ERR_DIMENSION, "btk_srp_power: bad sizes S=%d U=%d T=%ld T_stride=%ld", S, U, T, T_stride);
  if (fbin_min < 1 || fbin_min > fbin_max || fbin_max > M / 2)
    return btk_set_error(BTK_ERR_PARAMETER, "btk_srp_power: frequency range %d .. %d, need 1 <= fbinMin <= fbinMax <= %d", fbin_min,
                         fbin_max, M / 2);
  if (T == 0) return BTK_OK;
  if (!X || !table_packed || !rp || !energy) return btk_set_error(BTK_ERR_PARAMETER, "btk_srp_power: null argument");
  const int K = M / 2 + 1, PP = srp_pairs_padded(N), UP = srp_dirs_padded(U);
  const int tiles = UP / 32, passes = (tiles + SRP_MAX_TILES - 1) / SRP_MAX_TILES, per = (tiles + passes - 1) / passes;
  const dim3 grid((unsigned)((T + SRP_FT * SRP_WAVES - 1) / (SRP_FT * SRP_WAVES)), (unsigned)S);
  const float nb = (float)(fbin_max - fbin_min + 1), edenom = (float)M * (float)N;
  for (int tile0 = 0; tile0 < tiles; tile0 += per) {
    const int nt = tiles - tile0 < per ? tiles - tile0 : per;
#define SRP_ARGS nt, grid, as_stream(stream), static_cast<const float2*>(X), static_cast<const float2*>(table_packed),   \
                 static_cast<float*>(rp), static_cast<float*>(energy), K, N, T_stride, T, U, UP, PP, tile0 * 32, fbin_min, \
                 fbin_max, M / 2, nb, edenom
    switch (PP) {
      case 4: srp_launch_tiles<4>(SRP_ARGS); break;
      case 8: srp_launch_tiles<8>(SRP_ARGS); break;
      case 16: srp_launch_tiles<16>(SRP_ARGS); break;
      default: srp_launch_tiles<32>(SRP_ARGS); break;
    }
#undef SRP_ARGS
    BTK_HIP_CHECK(hipGetLastError());
  }
  return BTK_OK;
}

// the per-frame N-best list, the energy gate and accRPs_ of DOAEstimatorSRPDSBLA::next (beamformer.cc:3131-3187)
int btk_srp_select(const void* rp, const void* energy, float threshold, int nbest, void* nbest_rp, void* nbest_idx, void* gate,
                   void* acc, int S, int U, long T, void* stream)
{
  if (nbest < 1 || nbest > SRP_MAX_NBEST)
    return btk_set_error(BTK_ERR_PARAMETER, "btk_srp_select: nBest=%d, need 1 .. %d", nbest, SRP_MAX_NBEST);
  if (S < 1 || U < 1 || T < 0) return btk_set_error(BTK_ERR_DIMENSION, "btk_srp_select: bad sizes S=%d U=%d T=%ld", S, U, T);
  if (T == 0) return BTK_OK;
  if (!rp || !energy || !nbest_rp || !nbest_idx || !gate)
    return btk_set_error(BTK_ERR_PARAMETER, "btk_srp_select: null argument");
  hipLaunchKernelGGL(srp_nbest_kernel, dim3((unsigned)((T + 255) / 256), (unsigned)S), dim3(256), 0, as_stream(stream),
                     static_cast<const float*>(rp), static_cast<const float*>(energy), threshold, nbest,
                     static_cast<float*>(nbest_rp), static_cast<int*>(nbest_idx), static_cast<int*>(gate), U, T);
  BTK_HIP_CHECK(hipGetLastError());
  if (!acc) return BTK_OK;                               // a caller that accumulates frame by frame itself (the node layer)
  hipLaunchKernelGGL(srp_acc_kernel, dim3((unsigned)U, (unsigned)S), dim3(64), 0, as_stream(stream),
                     static_cast<const float*>(rp), static_cast<const int*>(gate), static_cast<double*>(acc), U, T);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

}  // extern "C"
