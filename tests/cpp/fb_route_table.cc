// Prints the filter-bank route table of csrc/fb_route.h (tests/test_fb_route_cpu.py compares it with the table written out there).
// One line per (switch setting, M, m, r): routes, the five query answers as fb_kernels.hip derives them, scratch bytes of four shapes for the float and for the int16 route.
#include "fb_route.h"
#include <cstdio>

int main()
{
  static const char* const AN[] = {"A512", "FAST", "GENERIC"};
  static const char* const FN[] = {"FUSED512", "BFZ512", "BIG", "FAST256", "STAGED"};
  static const char* const SN[] = {"S512", "FAST", "GENERIC"};
  static const char* const SWN[] = {"default", "BTK_DISABLE_ANALYSIS512", "BTK_DISABLE_SYNTHESIS512", "BTK_DISABLE_FAST", "BTK_DISABLE_FUSED",
                                    "BTK_SYN_NARROW", "BTK_FUSED_VAR", "BTK_FUSED512_NEW=0"};
  static const int SHAPES[4][4] = {{1, 1, 0, 1}, {2, 3, 1, 2}, {32, 64, 0, 4096}, {1, 64, 0, 512}};   // S, N, per_stream, tcount (the last: channel groups at M >= 1024)
  for (int si = 0; si < 8; si++) {
    fb_switches sw{false, false, false, false, false, true, -1};
    switch (si) {
      case 1: sw.disable_analysis512 = true; break;
      case 2: sw.disable_synthesis512 = true; break;
      case 3: sw.disable_fast = true; break;
      case 4: sw.disable_fused = true; break;
      case 5: sw.syn_narrow = true; break;
      case 6: sw.fused_var = 3; break;
      case 7: sw.fused512_new = false; break;
    }
    for (int M = 64; M <= 2048; M *= 2)
      for (int m = 2; m <= 4; m += 2)
        for (int r = 0; r <= 3; r++)
          for (int whole = 1; whole >= 0; whole--) {
            const fb_geom ga{M, m, 1 << r, M / 2 + 1, whole != 0, false}, gs{M, m, 1 << r, M / 2 + 1, true, true};
            const fb_analysis_route_t a = fb_analysis_route(ga, sw);
            const fb_fused_route_t ff = fb_fused_route(ga, sw, 0), fi = fb_fused_route(ga, sw, 1);
            std::printf("%s %d %d %d %s ana %s fused %s fused_i16 %s syn %s queries %d %d %d %d bytes", SWN[si], M, m, r, whole ? "whole" : "shard", AN[a], FN[ff],
                        FN[fi], SN[fb_synthesis_route(gs, sw)], a != FB_ANA_GENERIC, (int)fb_synthesis_aligned_form(gs, sw), ff != FB_STAGED, fi != FB_STAGED);
            for (const auto& s : SHAPES) std::printf(" %ld", fb_fused_scratch_bytes(ff, ga, s[0], s[1], s[2], s[3]));
            for (const auto& s : SHAPES) std::printf(" %ld", fb_fused_scratch_bytes(fi, ga, s[0], s[1], s[2], s[3]));
            std::printf("\n");
          }
  }
  return 0;
}
