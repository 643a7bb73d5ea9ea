// fb_fused512.hip -- the production form of the fused analysis -> fixed-weight beamformer at M = 512, m = 4, r = 1 (gfx950),
// with the edge tiles of a launch dispatched first and served by the direct window loads.
//
// The arithmetic, the LDS layout and the interior channel loop are those of analysis512_bfz_kernel<2, 33231> in fb_analysis512.hip
// (see there for the formulation: beamformer sum in the Z domain, one Hermitian post-pass per tile, window loads one channel ahead,
// weight pairs by LDS-DMA, folded-constant radix-16 passes); that file and fft_packed.h are pinned by the measurement records of
// bench.py, so what changes at the tile and launch level lives here.  Three things differ:
//   * blockIdx -> (stream, tile): the tiles whose span is not wholly inside the recording (the first and the last of every stream
//     in a whole-utterance launch) take the LOWEST block indices.  They are the slowest workgroups of the launch; dispatched last
//     (the last tile of the last stream used to be the very last workgroup) they ran alone on a draining chip.  The interior tiles
//     of the launch, stream-major, are cut into eight equal contiguous pieces, one per XCD: neighbouring tiles of a stream stay on
//     one XCD (the halo comes from its L2) and every XCD gets the same number of tiles whatever the edge tiles leave per stream.
//   * an edge tile of an aligned launch no longer stages its whole span through registers with per-element guards and four
//     barriers per channel: its channel loop is the interior one (two barriers, window a channel ahead, LDS-DMA of the weight
//     pairs) with every window row guarded -- a row (8 bytes at g0 + col + i D) wholly inside the recording is loaded as in the
//     interior loop, a row wholly outside is zero, and the one row the end of a recording of odd length can cut is one element.
//     The polyphase sums see the same values in the same order: the bits do not change.
//   * every window row of a tile's span is loaded once: the workgroup is split by the parity of the span's 23 rows (threads
//     0..127 the 12 even rows, threads 128..255 the 11 odd ones) instead of by frame half (15 rows each, 7 of them twice).  Every
//     thread still does 4 taps x 16 outputs with the same operands in the same order.
// Unaligned or odd-strided PCM keeps the register-staged loop.
#include "btk_internal.h"
#include "fft_packed.h"
#include <mutex>
#include <type_traits>

namespace {

constexpr int F_M = 512, F_NF = 256, F_MT = 4, F_TT = 16, F_NT = 256, F_NWAVE = 4;
constexpr int F_D = F_M / 2;                                        // R = 2
constexpr int F_SPAN = (F_TT - 1) * F_D + F_MT * F_M;                // samples under the 16 frames of a tile
constexpr int F_FRZ = 272;                                          // float2 per FFT frame buffer (16 (mod 32): see fb_analysis512.hip)
constexpr int F_FB_BYTES = F_TT * F_FRZ * 8;
constexpr int F_WSTR = 320;                                         // float4 per channel in the weight-pair table
static_assert(F_WSTR == FB_WSTR512, "btk_fb_analysis_bf_scratch_bytes sizes the weight-pair table by fb_route.h");
constexpr int F_WQ_OFF = F_FB_BYTES;
constexpr int F_LDS = F_FB_BYTES + 2 * F_WSTR * 16;                 // frames (the staged loop's span aliases them) + two weight-pair buffers
constexpr int F_NV4 = (F_SPAN / 4 + F_NT - 1) / F_NT;
constexpr int F_NPG = 128, F_FPT = 8;                                // pair indices n0, n0 + 128; 8 outputs of each per thread
constexpr int F_NROW = F_TT - 1 + 2 * (F_MT - 1) + 2;                 // 23 window rows (of D samples) under a tile
constexpr int F_NWG = (F_NROW + 1) / 2;                              // 12 even rows; the odd half of the workgroup takes the 11 odd ones
static_assert(F_SPAN * 4 <= F_FB_BYTES, "the staged span shares the frame region");

enum { LOOP_INTERIOR = 0, LOOP_EDGE = 1, LOOP_STAGED = 2 };

// Wq [Sw][N][F_WSTR] float4 as pair_weights_kernel (fb_analysis512.hip) lays it out.  The edge tiles of all streams are the blocks
// [0, S (tile_lo + ntiles - tile_hi)), rounded up to a multiple of 8 so that for the interior blocks behind them blockIdx & 7 is the XCD;
// tiles_per_xcd = ceil(S (tile_hi - tile_lo) / 8) interior tiles of the launch per XCD.
template <typename PT>
__global__ __launch_bounds__(F_NT, 2)
void fused512_kernel(const PT* __restrict__ pcm, long nsamples, long pcm_stride,
                     const float* __restrict__ proto, const float2* __restrict__ twg,
                     int laN, float gain, int N, int K, const float4* __restrict__ Wq, long w_stream_stride,
                     float2* __restrict__ Y, long T_stride, long t0, long tcount, int ntiles, int tile_lo, int tile_hi,
                     int tiles_per_xcd, int S)
{
  constexpr int D = F_D, NWG = F_NWG, FPT = F_FPT, NPG = F_NPG, NROW = F_NROW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* xs = reinterpret_cast<float*>(smem);                                 // staged loop only: the PCM span, overwritten by the frames
  float2* fbuf = reinterpret_cast<float2*>(smem);
  float4* wq = reinterpret_cast<float4*>(smem + F_WQ_OFF);                    // [2][F_WSTR] weight pairs of a channel

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int ne = tile_lo + (ntiles - tile_hi);                                // edge tiles per stream: [0, tile_lo) and [tile_hi, ntiles)
  const int n_edge = ne * S, n_edge_pad = (n_edge + 7) & ~7;
  int s, tile;
  if (b < n_edge_pad) {
    if (b >= n_edge) return;
    s = b / ne;
    const int e = b - s * ne;
    tile = e < tile_lo ? e : tile_hi + (e - tile_lo);
  } else {
    // interior tiles of all streams as one sequence (stream-major); XCD x takes the x-th of eight equal contiguous pieces
    const int bi = b - n_edge_pad;
    const int xcd = bi & 7, j0 = bi >> 3;
    const int ni = tile_hi - tile_lo;
    const long g = (long)xcd * tiles_per_xcd + j0;
    if (g >= (long)ni * S) return;
    s = (int)(g / ni);
    tile = tile_lo + (int)(g - (long)s * ni);
  }
  const long tt0 = (long)tile * F_TT;
  const int fl = lane >> 4, j = lane & 15;

  constexpr bool I16 = sizeof(PT) == 2;
  const bool vec_ok = ((pcm_stride & 3) == 0) && ((reinterpret_cast<uintptr_t>(pcm) & (4 * sizeof(PT) - 1)) == 0);
  const long g0 = (t0 + tt0 + laN + 1) * (long)D - (long)F_MT * F_M;
  const bool inside = g0 >= 0 && g0 + F_SPAN <= nsamples;
  const float4* wts = Wq + (long)s * w_stream_stride;
  float4 pre[F_NV4];
  float4 wpre;
  float2 w256pre;
  const PT* pcm_e = pcm;                     // the staged loop's own copies of the two base pointers: laundered through an
  const float4* wts_e = wts;                 // asm at its entry so that hipcc cannot hoist its loads above the branch
  // staged loop: the span of channel n -> registers, element by element
  auto fetch = [&](int n) {
    const PT* src = pcm_e + ((long)s * N + n) * pcm_stride;
#pragma unroll
    for (int q = 0; q < F_NV4; q++) {
      const int l = (tid + q * F_NT) * 4;
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const long g = g0 + l + e;
        v[e] = (l + e < F_SPAN && g >= 0 && g < nsamples) ? (float)src[g] : 0.0f;
      }
      pre[q] = make_float4(v[0], v[1], v[2], v[3]);
    }
    wpre = wts_e[(long)n * F_WSTR + tid];
    const float4 t = wts_e[(long)n * F_WSTR + 256];
    w256pre = make_float2(t.x, t.y);
  };

  // polyphase mapping: output (pair index n0 + q 128, frame f, tap k) reads row f + 2 (m-1-k) + (1-q) of the span's 23 rows at
  // column wo, and the parity of that row is the parity of f + 1 - q whatever the tap.  The workgroup is split by row parity:
  // threads 0..127 load the 12 even rows and produce {q = 1, f even} and {q = 0, f odd}, threads 128..255 load the 11 odd rows
  // and produce {q = 1, f odd} and {q = 0, f even}: every word of the span is loaded once per tile, 16 outputs per thread.
  // A wavefront is all-even or all-odd, and the channel loop is instantiated for either parity (register rows are compile-time).
  const int n0 = tid % NPG;
  const int wo = F_M - 2 - 2 * n0 - F_M / 2;                                  // this thread's column within a row of the span
  float2 h[2][F_MT];
#pragma unroll
  for (int q = 0; q < 2; q++)
#pragma unroll
    for (int k = 0; k < F_MT; k++) h[q][k] = *reinterpret_cast<const float2*>(proto + 2 * (n0 + q * NPG) + F_M * k);
  f2 twr[15];                                                                 // W_256^{j k1}, k1 = 1..15, as (cos, tan)
#pragma unroll
  for (int k1 = 1; k1 < 16; k1++) { const float2 t = twg[(2 * j * k1) & 511]; twr[k1 - 1] = tw_tangent(t.x, t.y); }
  const f2 k_hc = f2{0.70710678118654752f, 0.92387953251128674f}, k_t1 = f2{0.41421356237309503f, 0.41421356237309503f};
  // The taps and twiddles are first used inside the channel loop; without a use in front of it hipcc keeps their
  // s_waitcnt vmcnt(k) inside the loop, where every iteration it also waits for the LDS-DMA of the NEXT channel
  // (vector-memory counters retire in order).  An empty asm that reads them retires those loads here.
#pragma unroll
  for (int q = 0; q < 2; q++)
#pragma unroll
    for (int k = 0; k < F_MT; k++) asm volatile("" : "+v"(h[q][k].x), "+v"(h[q][k].y));
#pragma unroll
  for (int k1 = 0; k1 < 15; k1++) asm volatile("" : "+v"(twr[k1]));
  f2 accA[16], accB[16];
#pragma unroll
  for (int k2 = 0; k2 < 16; k2++) { accA[k2] = f2{0.f, 0.f}; accB[k2] = f2{0.f, 0.f}; }
  float2 acc256 = make_float2(0.f, 0.f);

  // staged loop: registers -> LDS, PCM span + weight pairs of one channel
  auto stage = [&](int buf) {
#pragma unroll
    for (int q = 0; q < F_NV4; q++) {
      const int l = (tid + q * F_NT) * 4;
      if (l < F_SPAN) *reinterpret_cast<float4*>(xs + l) = pre[q];
    }
    wq[buf * F_WSTR + tid] = wpre;
    if (tid == 0) wq[buf * F_WSTR + 256] = make_float4(w256pre.x, w256pre.y, 0.f, 0.f);
  };
  // LDS-DMA (global_load_lds_dwordx4: 1 KiB per wave-instruction, lane-linear destination) of the weight pairs of channel n;
  // issued by asm so that hipcc does not order the FFT's LDS traffic behind it -- the matching s_waitcnt vmcnt(0) sits
  // before the barrier that opens channel n
  const unsigned xs_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;   // LDS byte offset of the dynamic region
  auto glds16s = [&](const void* gbase, unsigned voff, unsigned lds_dst) {       // uniform base (SGPR pair) + 32-bit lane offset
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(gbase), "s"(lds_dst) : "memory");
  };
  const int wv = __builtin_amdgcn_readfirstlane(wave);                          // wave index in an SGPR: piece bookkeeping stays scalar
  auto dma = [&](int n) {
    const float4* wsrc = wts + (long)n * F_WSTR;
    const unsigned wq_lds = xs_lds + F_WQ_OFF + (n & 1) * (F_WSTR * 16);
#pragma unroll
    for (int i = 0; i < (F_WSTR / 64 + F_NWAVE - 1) / F_NWAVE; i++) {
      const int c = wv + F_NWAVE * i;
      if (c < F_WSTR / 64) glds16s(wsrc, (unsigned)(c * 64 + lane) * 16u, wq_lds + c * 1024);
    }
  };

  // The channel loop exists three times: interior tiles (the loads of the loop are the asm LDS-DMA and the window loads, none of
  // them guarded), edge tiles of an aligned launch (the same loop with guarded window rows) and the register-staged loop of an
  // unaligned launch (guarded element loads, four barriers, compiler-managed waits).  One loop with runtime branches let hipcc
  // hoist the guarded loads above the branch.
  float2 win[NWG];                            // polyphase window of the channel about to be transformed (loaded a channel ahead)
  auto channels = [&](auto loop_kind, auto parity) {
  constexpr int LOOP = decltype(loop_kind)::value;
  constexpr int PAR = decltype(parity)::value;                  // win[i] = row PAR + 2 i of the span
  constexpr int NLD = (NROW - PAR + 1) / 2;                     // 12 even / 11 odd rows
  constexpr bool DIRECT = LOOP != LOOP_STAGED;
  if constexpr (!DIRECT) asm volatile("" : "+s"(pcm_e), "+s"(wts_e));
  // edge loop: which rows of the span lie wholly inside the recording at this thread's column, and the one row its end may cut.
  // Row r starts at g0 + r D + c with g0 a multiple of D (uniform) and c = wo = 254 - 2 n0 even, in [0, D): the start of the
  // recording never cuts a row and the rows in front of it are the same for every thread (r < row_lo); the end leaves rem samples
  // from this thread's column in row 0: row r is whole when r D + 1 < rem and cut when r D + 1 == rem (nsamples odd).
  int row_lo = 0, rem = 0;
  if constexpr (LOOP == LOOP_EDGE) {
    row_lo = g0 >= 0 ? 0 : (-g0 / D < NROW ? (int)(-g0 / D) : NROW);
    const long left = nsamples - g0 - wo;
    rem = left < 0 ? 0 : (left > NROW * D ? NROW * D : (int)left);
  }
  auto row_full = [&](int r) { return r >= row_lo && r * D + 1 < rem; };
  auto row_cut = [&](int r) { return r >= row_lo && r * D + 1 == rem; };
  // rows PAR, PAR + 2, ... of channel n straight from HBM / L2 (8-byte loads, 512 contiguous bytes per wave-instruction)
  auto wload = [&](float2 (&win)[NWG], int n) {
    const PT* wsrc = pcm + ((long)s * N + n) * pcm_stride + g0 + wo;
    if constexpr (I16) {
      // four-byte TYPED buffer loads: the load unit delivers the two samples as floats (btk_internal.h)
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<PT*>(pcm + ((long)s * N + n) * pcm_stride + g0), 0, 0x7fffffff,
                                                                          BTK_RSRC_I16X2_SSCALED);
      const int vo = wo * 2;
#pragma unroll
      for (int i = 0; i < NLD; i++) {
        const int r = PAR + 2 * i;
        if constexpr (LOOP == LOOP_INTERIOR) {
          const btk_f2v t = btk_buffer_load_i16x2_f32(rs, vo, r * D * 2, 0); win[i] = make_float2(t.x, t.y);
        } else {
          float2 v = make_float2(0.f, 0.f);
          if (row_full(r)) { const btk_f2v t = btk_buffer_load_i16x2_f32(rs, vo, r * D * 2, 0); v = make_float2(t.x, t.y); }
          else if (row_cut(r)) v.x = (float)wsrc[r * D];
          win[i] = v;
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < NLD; i++) {
        const int r = PAR + 2 * i;
        if constexpr (LOOP == LOOP_INTERIOR) {
          win[i] = *reinterpret_cast<const float2*>(wsrc + r * D);
        } else {
          float2 v = make_float2(0.f, 0.f);
          if (row_full(r)) v = *reinterpret_cast<const float2*>(wsrc + r * D);
          else if (row_cut(r)) v.x = (float)wsrc[r * D];
          win[i] = v;
        }
      }
    }
  };
  auto body = [&](int n, float2 (&win)[NWG]) {
    f2 w256s = f2{0.f, 0.f};
    if constexpr (DIRECT) {
      // (a plain load would become a VECTOR load: the asm statements of this loop clobber memory, so hipcc cannot call the table
      //  invariant.)  The scalar load lands long before the sums; its s_waitcnt sits in front of the packed FMA that reads the pair
      const float4* wp = wts + (long)n * F_WSTR + 256;
      asm volatile("s_load_dwordx2 %0, %1, 0x0" : "=s"(w256s) : "s"(wp));
    }
    // ---- phase 1: the weight pairs (and, staged, the span) of channel n are in LDS
    if constexpr (!DIRECT) stage(n & 1);
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // the LDS-DMA of channel n and its window have landed
    __syncthreads();
    const int wbuf = n & 1;

    // the polyphase stage -- 64 packed instructions between the channel's two barriers -- runs at wave priority 1 (fb_analysis512.hip)
    __builtin_amdgcn_s_setprio(1);
    // ---- phase 2: polyphase (sliding register window).  index n0 + q NPG, frame f = 2 u + ((PAR + q + 1) & 1), tap k uses row
    //      f + 2 (m-1-k) + (1-q) = PAR + 2 i of the span
    {
      if constexpr (!DIRECT) {
        const float* wbase = xs + wo;
#pragma unroll
        for (int i = 0; i < NLD; i++) win[i] = *reinterpret_cast<const float2*>(wbase + (PAR + 2 * i) * D);
        __syncthreads();                                   // the frames overwrite the span
      }
      // tap-major order: consecutive FMAs belong to different outputs (no dependent back-to-back packed FMAs)
      // z = (h.x x.y, h.y x.x) summed over the taps: one packed multiply-add per tap with the halves of x crossed by op_sel
      f2 po[2][FPT];
#pragma unroll
      for (int k = 0; k < F_MT; k++)
#pragma unroll
        for (int q = 0; q < 2; q++)
#pragma unroll
          for (int u = 0; u < FPT; u++) {
            const int f = 2 * u + ((PAR + q + 1) & 1);
            const float2 xw = win[(f + 2 * (F_MT - 1 - k) + (1 - q) - PAR) / 2];
            const f2 x = f2{xw.x, xw.y}, hk = f2{h[q][k].x, h[q][k].y};
            if (k == 0) po[q][u] = pk_mul_xswap(hk, x);
            else pk_fma_xswap(po[q][u], hk, x);
          }
      // frame by frame: index n0 + 128 of a frame and index n0 of the next one are 136 float2 apart (one ds_write2_b64)
      const int zoff = (n0 >> 4) * 17 + (n0 & 15);
      constexpr int ZQ = (NPG >> 4) * 17;
#pragma unroll
      for (int f = 0; f < F_TT; f++) {
        const int q = (f + 1 + PAR) & 1, u = f >> 1;
        fbuf[f * F_FRZ + zoff + q * ZQ] = make_float2(po[q][u].x, po[q][u].y);
      }
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
    if constexpr (!DIRECT) {
      if (n + 1 < N) fetch(n + 1);          // lands under phases 3-4
    } else {
      if (n + 1 < N) dma(n + 1);            // every read of the other weight buffer is behind the barrier; lands under phases 3-4
      // the window loads are unconditional (the last channel re-reads its own window) so that they share a basic block with the
      // FFT, and the scheduling groups at the end of the body interleave them with its work
      // (edge loop: the guarded rows are branches the scheduler does not move; they are issued here all the same)
      wload(win, n + 1 < N ? n + 1 : n);
    }

    // ---- phase 3: wave-private 256-point FFT of 4 frames; the result stays in registers
    f2 v[16];
    const f4* wl = reinterpret_cast<const f4*>(wq) + wbuf * F_WSTR + j;
    f4 wg[2][4];                                                      // weight pairs, fetched one group of 4 bins ahead
    {
      f2* fb = reinterpret_cast<f2*>(fbuf) + (wave * 4 + fl) * F_FRZ;
#pragma unroll
      for (int r = 0; r < 16; r++) v[r] = fb[r * 17 + j];
      dft16t(v, k_hc, k_t1);
#pragma unroll
      for (int k1 = 0; k1 < 16; k1++) fb[j * 17 + k1] = v[k1];
#pragma unroll
      for (int jp = 0; jp < 16; jp++) v[jp] = fb[jp * 17 + j];
#pragma unroll
      for (int q = 0; q < 4; q++) wg[0][q] = wl[q * 16];
      dft16t_tw(v, twr, k_hc, k_t1);                                  // v[k2] = Z[j + 16 k2]
    }
    // ---- phase 4: A[q] += conj(w[q]) Z[q],  B'[q] += conj(w[(256-q)&255]) conj(Z[q])
    {
#pragma unroll
      for (int g = 0; g < 4; g++) {
        if (g < 3) {
#pragma unroll
          for (int q = 0; q < 4; q++) wg[(g + 1) & 1][q] = wl[((g + 1) * 4 + q) * 16];
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int k2 = g * 4 + q;
          const f4 w4 = wg[g & 1][q];
          acc_conjw_z(accA[k2], w4.xy, v[k2]);
          acc_conjw_conjz(accB[k2], w4.zw, v[k2]);
        }
      }
      const float r = v[0].x - v[0].y;                                // bin 256 (lanes j == 0): X = gain (Z0.re - Z0.im)
      if constexpr (DIRECT) {
        // the channel's bin-256 weight is wave-uniform: one packed FMA with the SGPR pair (acc += (w.x, -w.y) r)
        f2 a2 = f2{acc256.x, acc256.y};
        const f2 rr = f2{r, r};
        asm volatile("s_waitcnt lgkmcnt(0)\n\tv_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[1,0,1] neg_hi:[1,0,0]" : "+v"(a2) : "s"(w256s), "v"(rr));
        acc256 = make_float2(a2.x, a2.y);
      } else {
        const float4 w256 = wq[wbuf * F_WSTR + 256];
        acc256.x = fmaf(w256.x, r, acc256.x);
        acc256.y = fmaf(-w256.y, r, acc256.y);
      }
    }
    if constexpr (LOOP == LOOP_INTERIOR) {
#pragma unroll
      for (int i = 0; i < NLD; i++) {
        __builtin_amdgcn_sched_group_barrier(0x080, 4, 0);    // four LDS instructions (anchors: the FFT's data flow fixes their order) ...
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);    // ... then one window load
      }
    }
    if constexpr (!DIRECT) __syncthreads();                            // frames and weight pairs consumed
  };
  if constexpr (!DIRECT) fetch(0);
  else { dma(0); wload(win, 0); }
  for (int n = 0; n < N; n++) body(n, win);
  };
  auto both_parities = [&](auto loop_kind) {
    if (__builtin_amdgcn_readfirstlane(tid / NPG) == 0) channels(loop_kind, std::integral_constant<int, 0>{});
    else channels(loop_kind, std::integral_constant<int, 1>{});
  };
  if (vec_ok) {
    if (inside) both_parities(std::integral_constant<int, LOOP_INTERIOR>{});
    else both_parities(std::integral_constant<int, LOOP_EDGE>{});
  } else {
    both_parities(std::integral_constant<int, LOOP_STAGED>{});
  }

  __syncthreads();
  // ---- once per tile: B[k] = B'[(256-k)&255] through the wave's own frame buffers, Hermitian post-pass,
  //      then a transposed store Y[s][k][tt0 .. tt0+15] (128-byte runs per bin)
  {
    const float hg = 0.5f * gain;
    float2* fb = fbuf + (wave * 4 + fl) * F_FRZ;
#pragma unroll
    for (int k2 = 0; k2 < 16; k2++) fb[k2 * 17 + j] = make_float2(accB[k2].x, accB[k2].y);
    float2 yv[16];
#pragma unroll
    for (int k2 = 0; k2 < 16; k2++) {
      const int k = j + 16 * k2;
      const int kp = (F_NF - k) & 255;
      const float2 Bk = fb[(kp >> 4) * 17 + (kp & 15)];
      const float2 w = twg[k];
      const float2 c1 = make_float2(1.f + w.y, -w.x), c2 = make_float2(1.f - w.y, w.x);
      const float2 a = make_float2(accA[k2].x, accA[k2].y);
      yv[k2] = make_float2(hg * ((c1.x * a.x - c1.y * a.y) + (c2.x * Bk.x - c2.y * Bk.y)),
                           hg * ((c1.x * a.y + c1.y * a.x) + (c2.x * Bk.y + c2.y * Bk.x)));
    }
#pragma unroll
    for (int k2 = 0; k2 < 16; k2++) fb[k2 * 17 + j] = yv[k2];
    if (j == 0) reinterpret_cast<float2*>(wq)[wave * 4 + fl] = make_float2(gain * acc256.x, gain * acc256.y);   // weights are dead
  }
  __syncthreads();
  {
    const int f = tid % F_TT, kq = tid / F_TT;             // 16 bin columns
    if (tt0 + f < tcount) {
      float2* yo = Y + (long)s * K * T_stride + tt0 + f;
      const float2* zf = fbuf + f * F_FRZ;
#pragma unroll 4
      for (int it = 0; it < 16; it++)     // non-temporal: Y is written once and read by another kernel
        __builtin_nontemporal_store(f2{zf[it * 17 + kq].x, zf[it * 17 + kq].y}, reinterpret_cast<f2*>(yo + (long)(kq + 16 * it) * T_stride));
      if (kq == 0) yo[(long)F_NF * T_stride] = reinterpret_cast<const float2*>(wq)[f];
    }
  }
}

// W [Sw][K][N] -> Wq [Sw][N][F_WSTR] float4: entry i < 256 = (w[i], w[(256-i) & 255]), entry 256 = (w[256], 0, 0), the rest 0
// (the layout of pair_weights_kernel in fb_analysis512.hip)
__global__ void fused512_pair_weights_kernel(const float2* __restrict__ W, float4* __restrict__ Wq, int K, int N, int Sw)
{
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)Sw * N * F_WSTR) return;
  const int e = (int)(i % F_WSTR);
  const int n = (int)((i / F_WSTR) % N);
  const long s = i / ((long)N * F_WSTR);
  const float2* Ws = W + s * (long)K * N;
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (e <= 256) {
    const float2 a = Ws[(long)e * N + n];
    const float2 bq = (e < 256) ? Ws[(long)((256 - e) & 255) * N + n] : make_float2(0.f, 0.f);
    o = make_float4(a.x, a.y, bq.x, bq.y);
  }
  Wq[i] = o;
}

long floor_div(long a, long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }      // b > 0

// the dynamic-LDS attribute is per device, and one process may drive several GPUs (btk_set_device): set once per (device, kernel)
template <typename PT>
int set_lds_once(const void* kern)
{
  constexpr int MAXDEV = 64;
  static std::mutex mu;
  static bool done[MAXDEV] = {};
  int dev = 0;
  BTK_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  if (dev >= 0 && dev < MAXDEV && done[dev]) return BTK_OK;
  BTK_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, F_LDS));
  if (dev >= 0 && dev < MAXDEV) done[dev] = true;
  return BTK_OK;
}

template <typename PT>
int launch_fused512(const btk_fb* fb, const PT* pcm, long nsamples, long pcm_stride, int S, int N, const float2* W,
                    int per_stream, void* scratch, float2* Y, long T_stride, long t0, long tcount, hipStream_t st)
{
  const int K = fb->K;
  const int Sw = per_stream ? S : 1;
  const float gain = fb->gain_factor > 0 ? (float)fb->gain_factor : 1.0f;
  float4* Wq = static_cast<float4*>(scratch);
  const int ntiles = (int)((tcount + F_TT - 1) / F_TT);
  // interior tiles [lo, hi): the span [g0, g0 + F_SPAN), g0 = (t0 + 16 tile + laN + 1) D - m M, lies inside [0, nsamples)
  const long f0 = t0 + fb->laN + 1;                                             // frame number that sets g0 of tile 0
  long lo = floor_div((long)F_MT * F_M / F_D - f0 + F_TT - 1, F_TT);            // first tile with g0 >= 0
  long hi = floor_div(floor_div(nsamples - F_SPAN + (long)F_MT * F_M, F_D) - f0, F_TT) + 1;   // tiles with g0 + F_SPAN <= nsamples
  lo = lo < 0 ? 0 : (lo > ntiles ? ntiles : lo);
  hi = hi < lo ? lo : (hi > ntiles ? ntiles : hi);
  const int n_int = (int)(hi - lo), n_edge = (int)(lo + ntiles - hi);
  const int tiles_per_xcd = (int)(((long)n_int * S + 7) / 8);                    // interior tiles of the whole launch per XCD
  const long nblocks = (((long)n_edge * S + 7) & ~7L) + (long)8 * tiles_per_xcd;
  const long nw = (long)Sw * N * F_WSTR;
  hipLaunchKernelGGL(fused512_pair_weights_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, W, Wq, K, N, Sw);
  auto kern = fused512_kernel<PT>;
  const int rc = set_lds_once<PT>(reinterpret_cast<const void*>(kern));
  if (rc != BTK_OK) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)nblocks), dim3(F_NT), F_LDS, st, pcm, nsamples, pcm_stride, fb->d_proto, fb->d_tw,
                     fb->laN, gain, N, K, Wq, per_stream ? (long)N * F_WSTR : 0L, Y, T_stride, t0, tcount, ntiles, (int)lo, (int)hi,
                     tiles_per_xcd, S);
  BTK_HIP_CHECK(hipGetLastError());
  return BTK_OK;
}

}  // namespace

// Fused analysis + fixed-weight beamformer, production form: the FB_FUSED512 route of fb_route.h (M = 512, m = 4, r = 1, whole bin
// range, no diagnostic variant selected); i16: pcm holds 16-bit samples
int btk_fused512(const btk_fb* fb, const void* pcm, int i16, long nsamples, long pcm_stride, int S, int N, const void* W,
                 int per_stream, void* Wt_scratch, void* Y, long T_stride, long t0, long tcount, hipStream_t st)
{
  if (fb->M != F_M || fb->m != F_MT || fb->R != 2 || fb->kx0 != 0 || fb->kx1 != fb->K)
    return btk_set_error(BTK_ERR_PARAMETER, "btk_fused512: not the geometry of this kernel (M=%d m=%d r=%d)", fb->M, fb->m, fb->r);
  const float2* Wp = static_cast<const float2*>(W);
  float2* Yp = static_cast<float2*>(Y);
  return i16 ? launch_fused512<short>(fb, static_cast<const short*>(pcm), nsamples, pcm_stride, S, N, Wp, per_stream, Wt_scratch, Yp, T_stride, t0, tcount, st)
             : launch_fused512<float>(fb, static_cast<const float*>(pcm), nsamples, pcm_stride, S, N, Wp, per_stream, Wt_scratch, Yp, T_stride, t0, tcount, st);
}
