// Stand-alone host check of the conv+pool planner (csrc/convpool.hip convpool_plan) over the geometry space of
// scripts/convpool_cases.py, for a sanitizer build run on the CPU (no GPU is touched: planning needs none):
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Icsrc -Xarch_host -fsanitize=address,undefined \
//       scripts/convpool_plan_check.hip csrc/convpool.hip -o /tmp/convpool_plan_check && /tmp/convpool_plan_check
//
// Prints the number of supported geometries (2192) and checks every plan's instantiation against its key.
#include <cstdio>

#include "common.h"
#include "kernels.h"

int main() {
  const int KS[] = {1, 2, 3, 5, 7}, HS[] = {6, 8, 10, 12, 14, 16}, CS[] = {1, 2, 3, 4, 6, 8, 12, 16},
            NS[] = {1, 4, 6, 8, 12, 16, 20, 32};
  int supported = 0, bad = 0;
  for (int k : KS) {
    const int pads[] = {0, (k - 1) / 2, k - 1};  // ascending; equal neighbours are one value
    for (int i = 0; i < 3; ++i) {
      if (i > 0 && pads[i] == pads[i - 1]) continue;
      const int pad = pads[i];
      for (int H : HS)
        for (int C : CS)
          for (int N : NS) {
            const dfa::CPPlan& p = dfa::convpool_plan(H, H, C, k, k, pad, N);
            if (&p != &dfa::convpool_plan(H, H, C, k, k, pad, N)) ++bad;  // cached: one plan per geometry
            if (!p.ok) continue;
            ++supported;
            bad += p.fwd_NK < p.fwd_nk || p.wg_KTMAX < p.wg_KT || p.dg_NKMAX < p.dg_nk || p.fwd.cap < 1 ||
                   p.wgrad.cap < 1 || p.dgrad.cap < 1;
          }
    }
  }
  std::printf("%d supported geometries, %d bad\n", supported, bad);
  return bad != 0;
}
