// fft_long.h -- one power-of-two complex FFT of up to 8192 points held in LDS, twiddles read through L2.
//
// fft_lds.h keeps 2 NF twiddles in LDS beside the data, which stops fitting where the data alone take 64 KB (NF = 8192, half of
// a 16384-point real transform).  Here the workgroup's LDS holds only buf[NF]; the twiddles come from ONE table in global memory,
//   tw[j] = exp(-i 2 pi j / BTK_LONGFFT_TWN),  j < BTK_LONGFFT_TWN,
// computed in float64 and rounded to float32 (accuracy mu = 2^-24 per component), shared by every transform length: the
// step exp(-i 2 pi / NF) is entry BTK_LONGFFT_TWN / NF.  128 KB, read by every workgroup, so it stays in L2; the early passes
// read a handful of distinct entries per wavefront.
//
// Same Stockham autosort passes as fft_lds.h (radix 4, plus one radix-2 pass when log2 NF is odd; read -> barrier -> write ->
// barrier, in place, natural order in and out, unnormalised).  SIGN < 0: forward (e^{-j}), SIGN > 0: backward.
// A radix-4 pass applies one twiddle product and two levels of additions to each point where two radix-2 passes apply two and
// two, so the rounding error of log2(NF)/2 radix-4 passes stays within Higham's bound for log2 NF radix-2 stages (Thm 24.2).
#pragma once
#include <hip/hip_runtime.h>
#include "fft_lds.h"

constexpr int BTK_LONGFFT_TWN = 16384;

template <int LOG2NF, int NT, int SIGN>
__device__ __forceinline__ void fft_long(float2* __restrict__ buf, const float2* __restrict__ tw, int tid)
{
  constexpr int NF = 1 << LOG2NF;
  constexpr int NB4 = NF / 4;                      // radix-4 butterflies per pass
  constexpr int U4 = (NB4 + NT - 1) / NT;
  constexpr int TS = BTK_LONGFFT_TWN / NF;         // table entries per step of exp(-i 2 pi / NF)
  static_assert(NB4 % NT == 0 || NB4 < NT, "NF/4 must be a multiple of the workgroup size, or smaller than it");
  static_assert(NF <= BTK_LONGFFT_TWN, "transform longer than the twiddle table");
  constexpr int NPASS4 = LOG2NF / 2;

  int Ns = 1;
#pragma unroll
  for (int pass = 0; pass < NPASS4; pass++) {
    float2 v[U4][4];
#pragma unroll
    for (int u = 0; u < U4; u++) {
      const int j = tid + u * NT;
      if (j < NB4) {
        const int k = j & (Ns - 1);
        // twiddle exp(SIGN i 2 pi k q / (4 Ns)), q = 1, 2, 3: table entry k q (NF / (4 Ns)) TS < 3/4 of the table
        const int tstep = k * (NF / (4 * Ns)) * TS;
        const float2* p = buf + j;
        float2 a0 = p[0], a1 = p[NF / 4], a2 = p[NF / 2], a3 = p[3 * NF / 4];
        if (pass > 0) {
          float2 w1 = tw[tstep], w2 = tw[2 * tstep], w3 = tw[3 * tstep];
          if (SIGN > 0) { w1 = cconjf(w1); w2 = cconjf(w2); w3 = cconjf(w3); }
          a1 = cmulf(a1, w1); a2 = cmulf(a2, w2); a3 = cmulf(a3, w3);
        }
        const float2 s02 = caddf(a0, a2), d02 = csubf(a0, a2);
        const float2 s13 = caddf(a1, a3), d13 = cmul_i<SIGN>(csubf(a1, a3));
        v[u][0] = caddf(s02, s13);
        v[u][1] = caddf(d02, d13);
        v[u][2] = csubf(s02, s13);
        v[u][3] = csubf(d02, d13);
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U4; u++) {
      const int j = tid + u * NT;
      if (j < NB4) {
        const int k = j & (Ns - 1);
        float2* q = buf + ((j - k) << 2) + k;
        q[0] = v[u][0]; q[Ns] = v[u][1]; q[2 * Ns] = v[u][2]; q[3 * Ns] = v[u][3];
      }
    }
    __syncthreads();
    Ns <<= 2;
  }
  if (LOG2NF & 1) {                                // final radix-2 pass, Ns == NF/2
    constexpr int NB2 = NF / 2;
    constexpr int U2 = (NB2 + NT - 1) / NT;
    static_assert(NB2 % NT == 0 || NB2 < NT, "radix-2 pass must tile the workgroup");
    float2 v[U2][2];
#pragma unroll
    for (int u = 0; u < U2; u++) {
      const int j = tid + u * NT;
      if (j < NB2) {
        float2 a0 = buf[j], a1 = buf[j + NF / 2];  // k == j because Ns == NF/2
        float2 w = tw[j * TS];                     // exp(-i 2 pi j / NF)
        if (SIGN > 0) w = cconjf(w);
        a1 = cmulf(a1, w);
        v[u][0] = caddf(a0, a1);
        v[u][1] = csubf(a0, a1);
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U2; u++) {
      const int j = tid + u * NT;
      if (j < NB2) { buf[j] = v[u][0]; buf[j + NF / 2] = v[u][1]; }
    }
    __syncthreads();
  }
}
