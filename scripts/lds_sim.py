#!/usr/bin/env python3
"""LDS bank-conflict model of the fused LeNet-5 train kernel's hot LDS reads (csrc/lenet_fused.hip).

For each phase it replays the byte addresses every lane of every wave issues per LDS instruction over one
workgroup's loop iterations and prices them with the gfx950 banking rules (MI355X_MICROARCH.md, LDS):
an instruction's lanes are serviced in fixed lane groups, one LDS cycle per group when conflict-free;
each extra distinct dword address on a bank within a group costs one more cycle.  Prints, per phase,
LDS-array cycles and the conflict share -- the same ratio as SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE.
Phase A is replayed as the kernel runs it (two kernel rows x 16 pixels per K-step, from Xs alone), as it ran
before (one kernel row x 32 pixels, odd columns from the shifted copy) and with a per-image skew of Xs that
was priced and not built (the 2-way conflicts are between rows of one image, 4 rows = 256 bytes apart).
Phase E is replayed as 8 waves x 26 steps over 16 tile slots (the kernel before the split) and as the
2 K-halves x 4 column groups it runs now.  Phases D (stores), E and F are replayed for two dC2 layouts: the
XOR swizzle t ^ ((t >> 3) & 7) of window-order rows (the kernel before the diagonal placement, kept for
comparison) and the diagonal placement with class-matched zero rows (distriflow_amd.ops.lenet_conv2_tables,
which the tables built here must equal).
Phase B is replayed as the kernel runs it and, for the record, with the cross-image tiles and the searched tap
order that were tried and measured no faster (docs/RESULTS.md).
Usage: python3 scripts/lds_sim.py
"""
import os
import sys
from collections import defaultdict

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

IMG, NT, NW = 8, 512, 8
XS_ELEMS = IMG * 1024 + 32
OFF_XS = 0
OFF_P1 = OFF_XS + XS_ELEMS * 2
OFF_C1 = OFF_P1 + IMG * 196 * 16
OFF_K = OFF_C1 + IMG * 196 * 4
DC2_RS = 104
NM = IMG * DC2_RS
OFF_PX = OFF_K + 32
OFF_FT = OFF_PX + NM * 2
OFF_W = OFF_FT + 98 * 2 * 16
OFF_U = OFF_W + 128 + 32
OFF_XS1 = OFF_U + 32
OFF_DC2 = OFF_U
LD0, LD1, LD2, LD3 = 424, 136, 104, 40
OFF_H0 = OFF_U
OFF_ZR = OFF_U + IMG * LD0 * 2 + IMG * LD1 * 2 + IMG * LD2 * 2 + IMG * LD3 * 2 + IMG * LD2 * 2 + IMG * LD1 * 2
KO = OFF_K
KZ = OFF_W + 128
# behind the union: dense biases, stamps, the per-image row table, then the 8-row zero block of phase F at a
# multiple of 256 bytes from dC2 (its row k has bank class k)
U_DENSE = OFF_ZR + LD0 * 2 + IMG * 16 * 4 + IMG * 25 * 16 - OFF_U
OFF_DB = OFF_U + (max(NM * 32, 32 + XS_ELEMS * 2 + 4 * 16 * 32 * 4, U_DENSE + 7 * 64 * 16) + 15) // 16 * 16
OFF_RT = OFF_DB + 864 + 128
OFF_ZB = OFF_DC2 + (OFF_RT + 208 - OFF_DC2 + 255) // 256 * 256
LDS_BYTES = OFF_ZB + 256
# conv2 forward, tried and not adopted: a tap order (tap of slot 4 s + g; 25 = none) found by
# scripts/lds_tap_search.py for tiles made of one pool window of 4 consecutive images.  The kernel gives slot
# k tap k (csrc/lenet_frag.h).
C2_TAP_K = list(range(25)) + [25] * 3
C2_ORDER = [0, 7, 1, 8, 4, 3, 6, 13, 9, 2, 10, 24, 14, 25, 15, 22, 16, 23, 17, 21, 18, 11, 19, 5, 20, 12, 25, 25]
FPERM = [0, 1, 2, 3, 8, 9, 10, 11, 12, 13, 14, 15, 4, 5, 6, 7]  # phase F: A row of lane i (diagonal layout)

B128_GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
               list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
               list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
               list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]
HALF_GROUPS = [list(range(0, 32)), list(range(32, 64))]


def cycles(kind, addr, active=None):
    """LDS-array cycles of one wave instruction; addr[lane] = byte address (None = inactive lane)."""
    if kind == "b128":
        groups, nd, nb = B128_GROUPS, 4, 64
    elif kind in ("b64", "tr"):
        groups, nd, nb = HALF_GROUPS, 2, 64
    elif kind in ("b32", "b16"):
        groups, nd, nb = HALF_GROUPS, 1, 32
    else:
        raise ValueError(kind)
    total = 0
    for grp in groups:
        banks = defaultdict(set)
        for ln in grp:
            a = addr[ln]
            if a is None:
                continue
            d0 = a // 4
            for k in range(nd):
                banks[(d0 + k) % nb].add(d0 + k)
        total += max([len(v) for v in banks.values()] + [1])
    return total, len(groups)


class Phase:
    def __init__(self, name):
        self.name, self.cyc, self.ideal, self.n = name, 0, 0, 0

    def add(self, kind, addr):
        c, ideal = cycles(kind, addr)
        self.cyc += c
        self.ideal += ideal
        self.n += 1

    def report(self):
        conf = self.cyc - self.ideal
        print(f"{self.name:<28} instr {self.n:6d}  LDS cycles {self.cyc:7d}  conflict {conf:7d} "
              f"({100.0 * conf / max(self.cyc, 1):5.1f} %)")
        return self.cyc, conf


def lanes():
    for lane in range(64):
        yield lane, lane & 15, lane >> 4


def phase_a(ph, rows2=True, skew=0):
    """A reads of conv1.  rows2 (the kernel): rows (image, y), 4 x tiles of 8 columns, K-step ks = kernel rows
    2 ks and 2 ks + 1 (the sixth slot reads row 4 again) x 16 pixels.  Before: rows (image, y, parity) from Xs /
    Xs1, 2 x halves, one kernel row of 32 pixels per step.  skew: bytes by which image k's rows would be
    shifted (k * skew), priced only."""
    for w in range(NW):
        for u in range(w, 56, NW):
            if rows2:
                mt, x0 = u >> 2, (u & 3) * 8
                for ks in range(3):
                    addr = []
                    for lane, i, g in lanes():
                        img, y = divmod(16 * mt + i, 28)
                        ky = min(2 * ks + (g >> 1), 4)
                        addr.append(OFF_XS + img * skew + 2 * (img * 1024 + (y + ky) * 32 + x0 + 8 * (g & 1)))
                    ph.add("b128", addr)
                continue
            mt, x0 = u >> 1, (u & 1) * 16
            for ky in range(5):
                addr = []
                for lane, i, g in lanes():
                    m = 16 * mt + i
                    img, rem = divmod(m, 56)
                    base = (OFF_XS1 if rem & 1 else OFF_XS) + 2 * (img * 1024 + (rem >> 1) * 32 + x0 + 8 * g)
                    addr.append(base + 2 * ky * 32)
                ph.add("b128", addr)


def trow(oy, ox):
    """window-order row of conv2 output position (oy, ox)"""
    return (((oy >> 1) * 5 + (ox >> 1)) << 2) + ((oy & 1) << 1) + (ox & 1)


def dc2_class(oy, ox):
    return ((ox >> 1) + 7 * oy + 4 * (ox & 1)) % 8


def winpix():
    """window-order row t of an image -> pool1 pixel inside the image (padding rows: pixel 0)"""
    wp = np.zeros(DC2_RS, dtype=np.int64)
    for oy in range(10):
        for ox in range(10):
            wp[trow(oy, ox)] = oy * 14 + ox
    return wp


def dc2_swz(t):
    return t ^ ((t >> 3) & 7)


def placement(diag):
    """t -> physical row of the image's dC2 block"""
    if not diag:
        return np.array([dc2_swz(t) for t in range(DC2_RS)])
    place, fill = np.full(DC2_RS, -1, dtype=np.int64), [0] * 8
    for t, (oy, ox) in sorted((trow(oy, ox), (oy, ox)) for oy in range(10) for ox in range(10)):
        c = dc2_class(oy, ox)
        place[t] = c + 8 * fill[c]
        fill[c] += 1
    place[100:] = sorted(set(range(DC2_RS)) - set(place[:100].tolist()))
    return place


def pxtab(diag):
    """physical dC2 row (image * 104 + row) -> pool1 pixel (phase E)"""
    rp = np.zeros(DC2_RS, dtype=np.int64)
    rp[placement(diag)] = winpix()
    return (np.arange(IMG)[:, None] * 196 + rp[None, :]).reshape(-1)


def phase_b(ph, cross=False, order=None):
    """A reads of conv2: a tile is 16 consecutive rows of the padded per-image row space, slot 4 s + g of
    K-step s holds tap 4 s + g.  Tried (cross, order): tile mt = pool window mt % 26 of images
    4 (mt / 26) + (i >> 2), row i = position i & 3; another tap of slot 4 s + g."""
    WP = winpix()
    order = C2_TAP_K if order is None else order
    for w in range(NW):
        for mt in range(w, NM // 16, NW):
            for s in range(7):
                addr = []
                for lane, i, g in lanes():
                    tap = order[4 * s + g]
                    toff = ((tap // 5) * 14 + tap % 5) * 8 if tap < 25 else 0
                    if cross:
                        img, t = 4 * (mt // 26) + (i >> 2), 4 * (mt % 26) + (i & 3)
                    else:
                        img, t = divmod(16 * mt + i, DC2_RS)
                    addr.append(OFF_P1 + 2 * ((img * 196 + int(WP[t])) * 8 + toff))
                ph.add("b128", addr)


def phase_d(ph, diag=True):
    """dC2 stores: thread (image, window, 16-byte half) writes the window's 4 rows"""
    place = placement(diag)
    for d in range(4):
        for k in range(2):
            for w in range(NW):
                addr = []
                for lane in range(64):
                    it = 64 * w + lane + k * NT
                    if it >= IMG * 50:
                        addr.append(None)
                        continue
                    img, rem = divmod(it, 50)
                    addr.append(OFF_DC2 + 2 * ((img * DC2_RS + int(place[(rem >> 1) * 4 + d])) * 16 + 8 * (rem & 1)))
                ph.add("b128", addr)


def e_waves(split):
    """Phase E's work per wave: (first step, end step, column tiles).  Parent: every wave runs all 26 steps
    over KT = 2 tile slots T = w + 8 k (16 slots for 13 tiles: a slot past tile 12 reads tap 0 and is
    dropped).  Split: 2 K-halves x 4 column groups, tiles T = cg + 4 k < 13, no dummy slot."""
    nE = NM // 32
    for w in range(NW):
        if split:
            h, cg = w >> 2, w & 3
            nlo = (nE + 1) >> 1
            yield (nlo if h else 0), (nE if h else nlo), [T for T in range(cg, 13, NW // 2)]
        else:
            yield 0, nE, [w + NW * k for k in range((13 + NW - 1) // NW)]


def phase_e(ph, ph2=None, ph3=None, split=True, diag=True):
    """A (dC2) reads into ph, the im2col B (P1) reads into ph2, the u16 pixel-index reads and (split) the
    cross-half exchange through P1 into ph3 (default: ph for all).  A step's lane (g, q) takes physical
    rows 32 s + 4 g + q and + 16 (diag) or, before, window-order rows 32 s + 8 g + q and + 4 through the XOR swizzle."""
    PX = pxtab(diag)
    ph2 = ph2 if ph2 is not None else ph
    ph3 = ph3 if ph3 is not None else ph
    for w, (s0, s1, tiles) in enumerate(e_waves(split)):
        for s in range(s0, s1):
            # A: two transposed reads of dC2 (ldAv; before: row mA ^ sx, the swizzle term of its 8-row block)
            for half in range(2):
                addr = []
                for lane, i, g in lanes():
                    q, p = (lane & 15) >> 2, lane & 3
                    mA = 32 * s + (16 * half + 4 * g + q if diag else 8 * g + q + 4 * half)
                    b = 4 * s + g
                    sx = 0 if diag else (b - 13 * ((b * 79) >> 10)) & 7
                    addr.append(OFF_DC2 + 2 * ((mA ^ sx) * 16 + 4 * p))
                ph.add("tr", addr)
            # the step's two pixel indices (PX + 8 g + q, + 4)
            for half in range(2):
                q = lambda lane: (lane & 15) >> 2  # noqa: E731
                ph3.add("b16", [OFF_PX + 2 * (32 * s + (16 * half + 4 * g + q(lane) if diag else 8 * g + q(lane) + 4 * half))
                                for lane, i, g in lanes()])
            for T in tiles:
                for half in range(2):
                    addr = []
                    for lane, i, g in lanes():
                        q, p = (lane & 15) >> 2, lane & 3
                        mA = 32 * s + (16 * half + 4 * g + q if diag else 8 * g + q + 4 * half)
                        tap = 2 * T + (p >> 1)
                        tp = tap if tap < 25 else 0
                        toff = ((tp // 5) * 14 + tp % 5) * 8 + 4 * (p & 1)
                        b = 4 * s + g
                        sx = 0 if diag else (b - 13 * ((b * 79) >> 10)) & 7
                        addr.append(OFF_P1 + 2 * (int(PX[mA ^ sx]) * 8 + toff))
                    ph2.add("tr", addr)
        if split:  # upper half writes, lower half reads [tile][lane] 16-byte pieces at the start of P1
            for T in tiles:
                ph3.add("b128", [OFF_P1 + (T * 64 + lane) * 16 for lane in range(64)])


def ftab(diag):
    """[98][2][16]: physical row of the position pixel pair (y, X2) gathers in step s of k-half hf; no tap:
    128 + class, row `class` of the zero block (before: the image's zero padding row dc2_swz(100))"""
    place = placement(diag)
    ft = np.zeros((98, 2, 16), dtype=np.int64)
    for yx in range(98):
        y, X2 = divmod(yx, 7)
        for hf in range(2):
            for s in range(16):
                ky, u = divmod(2 * s + hf, 6)
                oy, ox = y - ky, 2 * X2 + 1 - u
                if ky < 5 and 0 <= oy < 10 and 0 <= ox < 10:
                    ft[yx, hf, s] = place[trow(oy, ox)]
                else:
                    ft[yx, hf, s] = 128 + dc2_class(oy, ox) if diag else place[100]
    return ft


def phase_f(ph, diag=True, perm=True):
    """A reads; perm: lane i holds A row FPERM[i] of the tile"""
    FT = ftab(diag)
    for w in range(NW):
        for mt in range(w, 49, NW):
            for s in range(15):
                addr = []
                for lane, i, g in lanes():
                    m = 16 * mt + (FPERM[i] if perm else i)
                    img, rem = divmod(m, 98)
                    t = int(FT[rem, g >> 1, s])
                    if t >= 128:
                        addr.append(OFF_ZB + 32 * (t - 128) + 16 * (g & 1))
                    else:
                        addr.append(OFF_DC2 + 2 * ((img * DC2_RS + t) * 16 + 8 * (g & 1)))
                ph.add("b128", addr)


def check_tables():
    """the tables replayed here are the ones the kernel is given"""
    from distriflow_amd.ops import lenet_conv2_tables

    place, ft, rowpix, wp = lenet_conv2_tables()
    assert np.array_equal(place, placement(True)) and np.array_equal(ft, ftab(True)), "placement / ftab"
    assert np.array_equal(wp, winpix()), "winpix"
    assert np.array_equal((np.arange(IMG)[:, None] * 196 + rowpix[None, :]).reshape(-1), pxtab(True)), "pxtab"
    assert (OFF_ZB - OFF_DC2) % 256 == 0 and 2 * LDS_BYTES <= 160 * 1024
    assert sorted(C2_ORDER) == list(range(25)) + [25] * 3


def phase_g(ph):
    kxs1 = (OFF_XS1 - OFF_XS) // 2
    for w in range(NW):
        for rp in range(w, IMG * 14, NW):
            img, py = divmod(rp, 14)
            p0 = (img * 14 + py) * 14
            # pool codes of the lane's 4 windows: two 8-byte reads
            for h in range(2):
                ph.add("b64", [OFF_C1 + 4 * (p0 + 4 * g + 2 * h) for lane, i, g in lanes()])
            # pool gradients: 4 u16 reads per lane, every lane (rows (c, dy): i < 12; the rest re-read c = 5)
            for wd in range(4):
                addr = []
                for lane, i, g in lanes():
                    ca = i if i < 6 else (i - 6 if i < 12 else 5)
                    addr.append(OFF_P1 + 2 * ((p0 + 4 * g + wd) * 8 + ca))
                ph.add("b16", addr)
            # B: extended tap e = 16 T + i (30 taps ky' 0 .. 5, kx 0 .. 4; 30 = ones, 31 = zeros): two
            # ds_read2_b32 (dwords 0, 1 and 2, 3) from a dword-aligned start
            rowb = OFF_XS + 2 * (img * 1024 + 2 * py * 32)
            for T in range(2):
                for h in range(2):
                    addr = []
                    for lane, i, g in lanes():
                        e = 16 * T + i
                        if e < 30:
                            ky, kx = divmod(e, 5)
                            addr.append(rowb + 2 * ((kxs1 if kx & 1 else 0) + ky * 32 + 8 * g + 2 * (kx >> 1)) + 8 * h)
                        else:
                            addr.append((KO if e == 30 else KZ) + 8 * h)
                    ph.add("b64", addr)


def main():
    check_tables()
    old = "XOR swizzle (before)"
    rows = [("A conv1, one kernel row per step (before)", lambda p: phase_a(p, rows2=False), False),
            ("A conv1 (A reads)", phase_a, True),
            ("A conv1, priced: image k skewed by 32 k B", lambda p: phase_a(p, skew=32), False),
            ("B conv2 (A reads)", phase_b, True),
            ("B conv2, tried: cross-image tiles", lambda p: phase_b(p, cross=True), False),
            ("B conv2, tried: cross-image tiles, searched tap order", lambda p: phase_b(p, cross=True, order=C2_ORDER), False),
            ("B conv2, tried: per-image tiles, searched tap order", lambda p: phase_b(p, order=C2_ORDER), False),
            ("D dC2 stores, " + old, lambda p: phase_d(p, diag=False), False),
            ("D dC2 stores", phase_d, True),
            ("E conv2 wgrad, 8 x 26 steps, " + old, lambda *p: phase_e(*p, split=False, diag=False), False),
            ("E conv2 wgrad, 2 x 4 split, " + old, lambda *p: phase_e(*p, diag=False), False),
            ("E conv2 wgrad, 2 x 4 split", phase_e, True),
            ("F conv2 dgrad, " + old, lambda p: phase_f(p, diag=False, perm=False), False),
            ("F conv2 dgrad, rows i", lambda p: phase_f(p, perm=False), False),
            ("F conv2 dgrad (A reads)", phase_f, True), ("G conv1 wgrad", phase_g, True)]
    tot = conf = 0
    for name, fn, counted in rows:  # (rows not counted: the kernel as it was, or a variant that was tried, shown for comparison)
        ph = Phase(name)
        if name.startswith("E "):
            ph_a, ph_b, ph_x = Phase("  dC2 (tr reads)"), Phase("  im2col P1 (tr reads)"), Phase("  indices, exchange")
            fn(ph_a, ph_b, ph_x)
            for q in (ph_a, ph_b, ph_x):
                ph.cyc += q.cyc
                ph.ideal += q.ideal
                ph.n += q.n
        else:
            fn(ph)
        c, k = ph.report()
        if name.startswith("E "):
            for q in (ph_a, ph_b, ph_x):
                q.report()
        if counted:
            tot += c
            conf += k
    print(f"{'modelled total':<28} {'':13} LDS cycles {tot:7d}  conflict {conf:7d} ({100.0 * conf / tot:5.1f} %)")


if __name__ == "__main__":
    main()
