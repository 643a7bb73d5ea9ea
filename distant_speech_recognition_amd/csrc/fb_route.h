// fb_route.h -- which filter-bank kernel covers a plan: the ONE statement of the rule that the queries, the scratch size and the
// dispatch of fb_kernels.hip all read.  Pure host arithmetic: no HIP header, no environment (tests/test_fb_route_cpu.py builds it
// with a plain C++ compiler).  A new kernel form is one more line here and its launch in fb_kernels.hip.
#pragma once

struct fb_geom { int M, m, R, K; bool whole_range /* every bin is stored: not the bin shard of btk_fb_analysis_bins */, synthesis; };

// the A/B switches of btk_switches_t (btk_internal.h, which derives from this) that decide coverage
struct fb_switches {
  bool disable_analysis512, disable_synthesis512, disable_fast, disable_fused, syn_narrow;
  bool fused512_new /* BTK_FUSED512_NEW=0: the M = 512, r = 1 fused launch goes to analysis512_bfz_kernel (fb_analysis512.hip) instead of fused512_kernel (fb_fused512.hip) */;
  int fused_var /* BTK_FUSED_VAR; -1: default */;
};

enum fb_analysis_route_t { FB_ANA_A512 /* fb_analysis512.hip */, FB_ANA_FAST /* fb_fast.hip */, FB_ANA_GENERIC /* fb_kernels.hip; float samples only */ };
enum fb_fused_route_t { FB_FUSED512 /* fused512_kernel, fb_fused512.hip */, FB_BFZ512 /* analysis512_bfz_kernel, fb_analysis512.hip */,
                        FB_BIG /* fb_fused_big.hip */, FB_FAST256 /* fb_fast.hip */, FB_STAGED /* btk_fb_analysis + btk_bf_apply; float samples only */ };
enum fb_synthesis_route_t { FB_SYN_S512 /* fb_analysis512.hip */, FB_SYN_FAST /* fb_fast.hip */, FB_SYN_GENERIC /* fb_kernels.hip */ };

// float4 per channel in the weight-pair table of both M = 512 fused kernels: 257 used, padded to 5 x 64.  fb_fused512.hip asserts its
// F_WSTR against this; fb_analysis512.hip is pinned byte for byte by the benchmark's records and keeps its own WSTR = 320.
constexpr int FB_WSTR512 = 320;
constexpr int FB_BIG_TT = 8;                       // frames per tile of the M = 1024 / 2048 fused kernel

// every specialised kernel is built for four prototype taps per phase and r <= 2
inline bool fb_m4_r012(const fb_geom& g) { return g.m == 4 && (g.R == 1 || g.R == 2 || g.R == 4); }

// The same for float and 16-bit samples (a bin shard included); the int16 entry has no generic kernel and refuses FB_ANA_GENERIC.
inline fb_analysis_route_t fb_analysis_route(const fb_geom& g, const fb_switches& sw)
{
  if (fb_m4_r012(g) && g.M == 512 && !sw.disable_analysis512) return FB_ANA_A512;
  if (fb_m4_r012(g) && g.M >= 256 && !sw.disable_fast) return FB_ANA_FAST;
  return FB_ANA_GENERIC;
}

// i16: the samples are 16-bit PCM; that entry refuses FB_STAGED.
inline fb_fused_route_t fb_fused_route(const fb_geom& g, const fb_switches& sw, int i16)
{
  if (sw.disable_fused || !g.whole_range || !fb_m4_r012(g)) return FB_STAGED;
  switch (g.M) {
    case 512: return g.R == 2 && sw.fused512_new && sw.fused_var < 0 ? FB_FUSED512 : FB_BFZ512;
    // BTK_DISABLE_FAST takes the int16 form of this kernel away and leaves the float form: an asymmetry of long standing that the
    // profiling scripts may rely on, recorded here and kept
    case 256: return i16 && sw.disable_fast ? FB_STAGED : FB_FAST256;
    case 1024: case 2048: return g.R == 2 ? FB_BIG : FB_STAGED;
  }
  return FB_STAGED;
}

inline fb_synthesis_route_t fb_synthesis_route(const fb_geom& g, const fb_switches& sw)
{
  if (fb_m4_r012(g) && g.M == 512 && !sw.disable_synthesis512) return FB_SYN_S512;
  // (M = 2048, r = 2: the ring of TT + 4 R frames of the fb_fast.hip kernel does not fit the LDS)
  if (fb_m4_r012(g) && g.M >= 256 && !sw.disable_fast && !(g.M == 2048 && g.R == 4)) return FB_SYN_FAST;
  return FB_SYN_GENERIC;
}

// the wider kernel form for aligned launches (btk_fb_synthesis_aligned_form): synthesis512w_kernel, fast_synthesis_w_kernel
inline bool fb_synthesis_aligned_form(const fb_geom& g, const fb_switches& sw)
{
  const fb_synthesis_route_t rt = fb_synthesis_route(g, sw);
  return !sw.syn_narrow && g.R <= 2 && (rt == FB_SYN_S512 || (rt == FB_SYN_FAST && g.M >= 1024));
}

// FB_BIG, channel groups per tile: enough workgroups for the chip (about two per CU of work items), never fewer than 8 channels per
// group (C5 block, 64 tiles: 8 groups 0.279 ms, 4 groups -- one round of 256 workgroups -- 0.286, 16 groups 0.298)
inline int big_cg(int S, int N, long tcount)
{
  const long tiles = (tcount + FB_BIG_TT - 1) / FB_BIG_TT * (long)S;
  int cg = 1;
  while (cg < 16 && tiles * cg < 384 && N / (2 * cg) >= 8) cg *= 2;
  return cg;
}

// bytes of `scratch` a route's launch needs (btk_fb_analysis_bf_scratch_bytes); complex64 = 8 bytes, a weight pair = 16
inline long fb_fused_scratch_bytes(fb_fused_route_t rt, const fb_geom& g, int S, int N, int per_stream, long tcount)
{
  const long Sw = per_stream ? S : 1;
  switch (rt) {
    case FB_FUSED512: case FB_BFZ512: return 16 * Sw * N * FB_WSTR512;                     // weight pairs [Sw][N][320]
    case FB_FAST256: return 8 * Sw * N * g.K;                                              // transposed weights [Sw][N][K]
    case FB_BIG: {                                                                         // weight pairs [Sw][N][M/2 + 16] + the partial blocks of a channel-split launch
      const int cg = big_cg(S, N, tcount);
      return 16 * Sw * N * (g.M / 2 + 16) + (cg > 1 ? 8L * cg * S * g.K * tcount : 0) + 16;
    }
    case FB_STAGED: break;
  }
  return 8L * S * g.K * N * tcount;                                                        // the snapshots [S][K][N][tcount]
}
