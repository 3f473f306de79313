// The launch plans of the implicit GEMMs: forward / data gradient (kernels.h ConvPlan) and weight gradient
// (kernels.h WgradPlan, at the end of this file).  Host code only.
//
// Kernel order: pooled epilogue (igemm64 only), the 3x3 halo kernel, igemm64, the C = 1 kernels, the generic
// kernel.  Every tile shape, split and variant is chosen here, once: the launchers pick the instantiation the
// plan names, the bindings size workspaces from it.  DISTRIFLOW_DIAG is read once per process (csrc/diag.h).
#include "common.h"
#include "kernels.h"
#include "diag.h"

namespace dfa {

namespace {

bool aligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) == 0; }
long long tiles_of(const IGemmArgs& a, int BM, int BN) { return (long long)cdiv(a.M, BM) * cdiv(a.N, BN); }

bool igemm64_supported(const IGemmArgs& a, int mode) {
  if (!aligned(a.src, 15) || !aligned(a.w, 15) || a.Kpad % 8 || a.M <= 0 || a.N <= 0) return false;
  if (mode == MODE_DIRECT) return a.lda % 8 == 0 && a.K % 8 == 0;
  return !a.irregular && a.SC % 8 == 0 && a.OH > 0 && a.OW > 0;
}

// Split-K for under-filled launches: fewer than ~2 workgroups per CU and a long K (ResNet-18 layers 3-4:
// M = B*8*8 or B*4*4 with K up to 4608) leave one wave per SIMD waiting on every step
int splitk_for(const IGemmArgs& a, int BM, int BN) {
  const long long tiles = tiles_of(a, BM, BN);
  const int nk = cdiv(a.K, 64);
  if (a.N % 4 || a.ldc % 4 || tiles >= 512 || nk < 32) return 1;
  if (!aligned(a.out, 15) || (((uintptr_t)a.res | (uintptr_t)a.resmask | (uintptr_t)a.mask) & 7)) return 1;
  int s = 1;
  while (s < 4 && tiles * s * 2 <= 1024 && nk / (s * 2) >= 16) s *= 2;
  // severely under-filled (the Keras CNN's 9216 -> 128 dense: 16 tiles): up to 16 splits of >= 4 steps
  if (tiles * s < 256)
    while (s < 16 && tiles * s * 2 <= 512 && nk / (s * 2) >= 4) s *= 2;
  return s;
}

// FAST gather eligibility (see igemm64_kernel): whole 64-channel blocks per tap, <= 32 taps, stride-1
// data gradient, and operands addressable with 32-bit byte offsets below the out-of-range marker
bool igemm64_fast_ok(const IGemmArgs& a, int mode) {
  if (mode == MODE_DIRECT || a.SC % 64 || a.K != a.KH * a.KW * a.SC || a.KH * a.KW > 32 || a.Kpad < a.K) return false;
  if (mode == MODE_DGRAD && a.stride != 1 && a.stride != 2) return false;
  if (a.OH <= 0 || a.OW <= 0 || a.M % (a.OH * a.OW)) return false;
  static const bool off = diag_int("igemm_fast", 1) == 0;
  if (off) return false;
  const long long sbytes = (long long)(a.M / (a.OH * a.OW)) * a.SH * a.SW * a.SC * 2;
  const long long wbytes = (long long)round_up(a.N, 16) * a.Kpad * 2;
  return sbytes < (1LL << 30) && wbytes < (1LL << 30);
}

// tile geometry of the halo kernels on an H x W image: R rows of TI images per tile of P output pixels;
// false if the image does not tile (each caller adds its own staging limits)
bool halo_geom(int H, int W, int P, int& R, int& TI) {
  if (W < 4 || W > 64 || P % W != 0) return false;
  const int rpt = P / W;
  if (rpt <= H) {
    if (H % rpt != 0) return false;
    R = rpt, TI = 1;
  } else {
    if (rpt % H != 0) return false;
    R = H, TI = rpt / H;
  }
  return true;
}

bool conv3_halo_supported(const IGemmArgs& a, int mode, int& R, int& TI) {
  static const int on = diag_int("conv_halo", 1);
  if (!on || (mode != MODE_FWD && mode != MODE_DGRAD)) return false;
  return a.KH == 3 && a.KW == 3 && a.stride == 1 && a.pad == 1 && a.SH == a.OH && a.SW == a.OW && a.SC % 64 == 0 &&
         a.N % 64 == 0 && a.K == 9 * a.SC && a.Kpad >= a.K && a.Kpad % 8 == 0 && a.ldc % 4 == 0 && !a.bias &&
         !a.out_f32 && !a.drop.on && !a.pool_code &&
         a.M % kCP == 0 && a.M % (a.OH * a.OW) == 0 && halo_geom(a.OH, a.OW, kCP, R, TI) &&
         TI * (R + 2) * (a.OW + 2) <= kCXR && TI * (R + 2) * (a.OW == 16 ? 32 : a.OW + 2) <= kCXL &&
         (long long)a.M * a.ldc * 2 < (1LL << 32) &&  // one 32-bit byte offset per epilogue element
         aligned(a.src, 15) && aligned(a.w, 15) && aligned(a.out, 7) &&
         (((uintptr_t)a.res | (uintptr_t)a.resmask | (uintptr_t)a.mask) & 7) == 0;
}

// igemm64: tile, variant, grid.  `s64` is the split-K the tile policy asks for (1: none).
void plan_igemm64(const IGemmArgs& a, int mode, int s64, ConvPlan& p) {
  p.family = CONV_IGEMM64;
  p.grid = (int)tiles_of(a, p.BM, p.BN);
  if ((p.pool = a.pool_code != nullptr)) return;
  p.fast = igemm64_fast_ok(a, mode);
  if (mode == MODE_DGRAD && a.stride == 2) {  // never split; FAST: parity classes, grid = the 4 classes' tiles
    if (!(p.par = p.fast)) return;
    const int nimg = a.M / (a.OH * a.OW);
    p.grid = 0;
    for (int cl = 0; cl < 4; ++cl) {
      const int hc = (a.OH - (cl >> 1) + 1) >> 1, wc = (a.OW - (cl & 1) + 1) >> 1;
      p.grid += cdiv(nimg * hc * wc, p.BM) * cdiv(a.N, p.BN);
    }
    return;
  }
  p.splits = s64;
  if (p.splits > 1) p.grid *= p.splits, p.combine = true, p.splitk_floats = (long long)p.splits * a.M * a.N;
}

// halo: the weights-resident 64 -> 64 kernel, else 64- or 128-channel tiles, split over the input channel
// blocks when under-filled.  `ws64`: the scratch igemm64's split-K policy grants this problem, which bounds
// the halo split as well.
void plan_halo(const IGemmArgs& a, long long ws64, ConvPlan& p) {
  const int ntiles = a.M / kCP, hrows = p.TI * (p.R + 2) * (a.OW + 2);
  static const int c64 = diag_int("conv_halo_c64", 1);
  if (c64 && a.SC == 64 && a.N == 64 && hrows <= kC64XR && ntiles >= 512) {
    // weights resident: one 8-wave workgroup per CU, tiles split evenly (an even count per workgroup)
    p.family = CONV_HALO_C64, p.BN = 64, p.block = 512;
    p.tps = 2 * cdiv(ntiles, 2 * 256), p.grid = cdiv(ntiles, p.tps);
    return;
  }
  p.family = CONV_HALO;
  // 128-channel tiles while that still gives >= 2 workgroups per CU
  p.wide = a.N % 128 == 0 && (long long)ntiles * (a.N / 128) >= 512;
  p.BN = p.wide ? 128 : 64;
  static const int row = diag_int("conv_halo_row", 1);  // a kernel row per step (conv3_halo_kernel ROW)
  p.row = !p.wide && row;
  const int nco = a.N / p.BN, ncb = a.SC / 64;
  // under-filled launches (ResNet layer 4: 256 workgroups of 72 steps) split the input channel blocks
  // over workgroups; a fixed-order combine applies the epilogue
  static const int ksplit = diag_int("conv_halo_splitk", 1);
  static const int ksmax = diag_int("conv_halo_ks", 2);  // 2 measured faster than 4 (layer 4: 38.4 vs 43.1 us)
  if (ksplit && ntiles * nco < 512)
    while (p.ks < ksmax && ncb % (2 * p.ks) == 0 && (long long)ntiles * nco * p.ks * 2 <= 1024 &&
           (long long)(2 * p.ks) * a.M * a.N <= ws64)
      p.ks *= 2;
  if (p.ks > 1) p.splitk_floats = (long long)p.ks * a.M * a.N;
  // two splits: the tile's last arriver combines and runs the epilogue in this launch (c3_tickets); the
  // combine launch otherwise
  static const int fold = diag_int("conv_halo_fold", 1);
  p.fold = fold && p.ks == 2 && ntiles * nco <= kC3Tickets && (long long)p.ks * ntiles * kCP * a.N * 4 < (1LL << 31);
  p.combine = p.ks > 1 && !p.fold;
  p.grid = ntiles * nco * p.ks;
}

void plan_generic(const IGemmArgs& a, int mode, ConvPlan& p) {
  p.family = CONV_GENERIC;
  p.vec = aligned(a.src, 15) && (mode == MODE_DIRECT ? a.lda % 8 == 0 && a.K % 8 == 0 : a.SC % 8 == 0);
  // Tile choice: N fits one tile where possible; shrink BM when M alone cannot fill 256 CUs.
  p.BM = cdiv(a.M, 128) < 512 ? 64 : 128;
  p.BN = a.N <= 16 ? 16 : a.N <= 32 ? 32 : a.N <= 64 ? 64 : 128;
  p.grid = (int)tiles_of(a, p.BM, p.BN);
}

// Can the launch accumulate BatchNorm sums of its output (a.bacc, csrc/bn_acc.h)?  The halo and igemm64
// kernels (and their split-K combine) in both modes, with the vectorised bf16 epilogue; the generic kernel
// the forward sums only.
bool bacc_ok(const IGemmArgs& a, int mode, int family) {
  if (mode == MODE_DIRECT || a.out_f32 || a.drop.on || a.pool_code) return false;
  if (a.bacc.nrep < 1 || a.bacc.nrep > kBnAccMaxRep || (a.bacc.mode == 1 && (!a.bacc.x || !a.bacc.mean))) return false;
  if (a.bacc.acc2 && (a.bacc.mode != 1 || !a.bacc.x2 || !a.bacc.mean2)) return false;
  if (family == CONV_GENERIC) return mode == MODE_FWD && a.bacc.mode == 0;
  if (family == CONV_SMALLC) return false;
  if (!aligned(a.out, 15) ||
      (((uintptr_t)a.res | (uintptr_t)a.resmask | (uintptr_t)a.mask | (uintptr_t)a.bacc.x | (uintptr_t)a.bacc.x2) & 7))
    return false;
  return bacc_combine_ok(a);  // (a split-K combine may apply the epilogue)
}

}  // namespace

bool bacc_combine_ok(const IGemmArgs& a) {
  return a.N % 4 == 0 && a.N <= 1024 && 256 % (a.N / 4) == 0 && !a.out_f32 && !a.drop.on && a.ldc % 4 == 0;
}

ConvPlan conv_plan(const IGemmArgs& a, int mode) {
  ConvPlan p{};
  p.family = CONV_NOP, p.splits = 1, p.ks = 1, p.block = 256;
  if (a.M <= 0 || a.N <= 0) return p;
  p.family = CONV_INVALID;
  // igemm64's tile: N in one tile up to 64 channels (Keras CNN conv2, 32 channels: no half-empty tiles; a
  // 256 x 64 tile with 4 x 1 waves of 64 x 64 measured 9-16% slower on ResNet layer 1: 8 waves per CU
  // instead of 12), then 128 x 128 while that still gives >= 2 workgroups per CU, else 64 x 128
  const bool ok64 = igemm64_supported(a, mode);
  p.BN = a.N <= 32 ? 32 : a.N <= 64 ? 64 : 128;
  p.BM = a.N > 64 && tiles_of(a, 128, 128) < 512 ? 64 : 128;
  // ... and its split-K: only the under-filled 64 x 128 launches, never with pooling
  static const bool splitk = diag_int("igemm_splitk", 1) != 0;
  const int s64 = splitk && ok64 && p.BM == 64 && !a.pool_code ? splitk_for(a, 64, 128) : 1;
  if (a.drop.on && (a.out_f32 || a.ldc != a.N)) return p;
  if (a.irregular && a.pool_code) return p;
  if (a.pool_code) {  // the pooled epilogue is igemm64's, plain conv forward only
    if (mode == MODE_FWD && ok64 && a.OH % 2 == 0 && a.OW % 2 == 0 && a.N % 4 == 0 && a.ldc == a.N && !a.out_f32 &&
        !a.mask && !a.res && aligned(a.out, 7) && aligned(a.pool_code, 3))
      plan_igemm64(a, mode, 1, p);
  } else if (!a.irregular && conv3_halo_supported(a, mode, p.R, p.TI)) {
    plan_halo(a, s64 > 1 ? (long long)s64 * a.M * a.N : 0, p);
  } else if (ok64) {
    plan_igemm64(a, mode, s64, p);  // (dropout in its epilogues)
  } else {
    if (!a.irregular && smallc_fwd_supported(a, mode)) p.family = CONV_SMALLC, p.grid = 0;
    else plan_generic(a, mode, p);
    p.drop_after = a.drop.on;
  }
  p.bacc_ok = p.family != CONV_INVALID && bacc_ok(a, mode, p.family);
  if (a.bacc.acc && !p.bacc_ok) p.family = CONV_INVALID;
  return p;
}

// ---------------------------------------------------------------------------------- weight gradient
namespace {

bool wgrad_halo_supported(const WgradArgs& a, int mode, int& R, int& TI) {
  static const int on = diag_int("wgrad_halo", 1);
  return on && mode == MODE_FWD && !a.with_bias && a.KH == 3 && a.KW == 3 && a.stride == 1 && a.pad == 1 &&
         a.OH == a.SH && a.OW == a.SW && a.SC % 64 == 0 && a.N % 64 == 0 && a.K == 9 * a.SC && a.ldd % 8 == 0 &&
         a.M % kHP == 0 && a.M == a.OH * a.OW * (a.M / (a.OH * a.OW)) && halo_geom(a.SH, a.SW, kHP, R, TI) &&
         TI * (R + 2) * (a.SW + 2) <= kHXR && aligned(a.dy, 15) && aligned(a.src, 15);
}

bool wgrad_tr_supported(const WgradArgs& a, int mode) {
  return mode == MODE_FWD && (!a.with_bias || a.gb != nullptr) && a.SC % 8 == 0 && a.N % 8 == 0 && a.ldd % 8 == 0 && a.M > 0 &&
         a.OH > 0 && a.OW > 0 && aligned(a.dy, 15) && aligned(a.src, 15);
}

bool smallc_wgrad_supported(const WgradArgs& a, int mode) {
  return mode == MODE_FWD && a.SC == 1 && a.K < kSmallMaxK && a.N % 8 == 0 && a.N <= kSmallMaxN &&
         a.N * (a.K + 1) <= 8 * 256 && a.ldd % 8 == 0 && aligned(a.dy, 15) && a.OH > 0 && a.OW > 0 &&
         (!a.with_bias || a.gb != nullptr);
}

// The split of a reduction of `rows` (a launch of `tiles` output tiles) over workgroups: enough splits for
// `target` workgroups, each reducing at least `min_rows`, as many as `cap` floats of slabs (`slab` each) hold;
// the rows per split are rounded up to `quantum` and the split count re-rounded to what that leaves.
int split_rows(int target, int tiles, int rows, int quantum, int min_rows, long long slab, long long cap, int& per) {
  int s = max(1, min(cdiv(target, tiles), cdiv(rows, min_rows)));
  while (s > 1 && s * slab > cap) --s;
  per = round_up(cdiv(rows, s), quantum);
  return cdiv(rows, per);
}

}  // namespace

WgradPlan wgrad_plan(const WgradArgs& a, int mode, size_t ws_floats) {
  WgradPlan p{};
  p.family = WGRAD_NOP, p.splits = 1, p.block = 256;
  if (a.M <= 0 || a.N <= 0) return p;
  const long long unlimited = 1LL << 62, ws = ws_floats < (size_t)unlimited ? (long long)ws_floats : unlimited;
  const int Kt = a.K + (a.with_bias ? 1 : 0);
  const long long slab = (long long)a.N * Kt;  // (every family: with_bias is 0 on the halo kernel)
  // the specialised kernels are conv only (MODE_FWD) and refuse an irregular geometry
  int target, tiles, rows = a.M, quantum, min_rows, per;
  if (!a.irregular && wgrad_halo_supported(a, mode, p.R, p.TI)) {
    // one 8-wave workgroup per CU (140 KB of LDS), the 64-pixel tiles split over them
    p.family = WGRAD_HALO;
    static const int groups = diag_int("halo_groups", 2) == 1 ? 1 : 2;
    static const int halo_wg = diag_int("halo_wg", groups == 2 ? 256 : 512);
    p.groups = groups, p.block = 256 * groups;
    target = halo_wg, tiles = (a.N / 64) * (a.SC / 64), rows = a.M / kHP, quantum = 1, min_rows = 1;
  } else if (!a.irregular && wgrad_tr_supported(a, mode)) {
    p.family = WGRAD_TR;
    static const int t128 = diag_int("wgrad128", 32);
    p.BK = 128, p.WN = 2, p.WK = 2, p.BM = 64, p.MAXOCC = 4;
    if (a.N >= 128) {
      // 128 x 128 tiles: 32 rows per step at 3 workgroups per CU (170 VGPRs each: no spills).  At 4 per CU
      // that needs more than their 128 VGPRs and spills, which the inline-asm loads (destinations unprotected
      // until their counted wait) cannot tolerate: the 4-per-CU variant stays at 64 rows.
      p.BN = 128;
      if (t128 == 32) p.BM = 32, p.MAXOCC = 3;
    } else if (a.N <= 32) {
      p.BN = 32, p.WN = 1, p.WK = 4;  // Keras CNN conv2: no empty rows
    } else {
      // 64-channel tiles step 32 rows at a time: 36.9 KB of LDS -> 4 workgroups per CU (ResNet layer 1:
      // 104 -> 82 us)
      p.BN = 64, p.BM = 32;
    }
    // about two workgroups per CU (73.7 KB of LDS each at BM = 64), each reducing >= 256 rows
    static const int wgrad_wg = diag_int("wgrad_wg", 512);
    target = wgrad_wg, tiles = cdiv(a.N, p.BN) * cdiv(a.K + (a.with_bias ? 8 : 0), p.BK), quantum = p.BM, min_rows = 256;
  } else if (!a.irregular && smallc_wgrad_supported(a, mode)) {
    // one slab per workgroup, always reduced: the image-resident kernel when its slabs fit, else persistent
    // workgroups, halved until theirs do (a single slab is written whatever the workspace: callers check
    // scratch_floats)
    const bool c1 = c1_ok(a.SC, a.KH, a.KW, a.stride, a.pad, a.N, a.SH, a.SW) && a.K == 9;
    const int nb = cdiv(a.M / (a.OH * a.OW), C1_IMGS);
    int grid = min(cdiv(a.M, 64), 1024);
    p.wanted_floats = (c1 ? nb : grid) * slab;
    if (c1 && nb * slab <= ws) {
      p.family = WGRAD_C1, grid = nb;
    } else {
      p.family = WGRAD_SMALLC;
      while (grid > 1 && grid * slab > ws) grid /= 2;
    }
    p.splits = p.grid = grid, p.reduce = true, p.scratch_floats = grid * slab;
    p.capped = p.scratch_floats < p.wanted_floats;
    return p;
  } else {
    p.family = WGRAD_GENERIC;
    p.dvec = aligned(a.dy, 15) && a.ldd % 8 == 0;
    p.xvec = aligned(a.src, 15) && (mode == MODE_DIRECT ? a.lda : a.SC) % 8 == 0;
    p.BK = 64, p.WN = 2, p.WK = 2;
    p.BN = a.N <= 16 ? 16 : a.N <= 32 ? 32 : 64;
    if (p.BN == 16) p.WN = 1, p.WK = 4;
    // enough splits to put ~2 workgroups on each of the 256 CUs, each reducing >= 128 rows
    target = 512, tiles = cdiv(a.N, p.BN) * cdiv(Kt, p.BK), quantum = 32, min_rows = 128;
  }
  const int want = split_rows(target, tiles, rows, quantum, min_rows, slab, unlimited, per);
  p.splits = split_rows(target, tiles, rows, quantum, min_rows, slab, ws, per);
  (p.family == WGRAD_HALO ? p.tps : p.m_per_split) = per;
  p.grid = tiles * p.splits;
  p.reduce = p.splits > 1;
  p.scratch_floats = p.reduce ? p.splits * slab : 0;
  p.wanted_floats = want > 1 ? want * slab : 0;
  p.capped = p.scratch_floats < p.wanted_floats;
  return p;
}

}  // namespace dfa
