#!/usr/bin/env python3
"""LDS bank-conflict model of the fused LeNet-5 train kernel's hot LDS reads (csrc/lenet_fused.hip).

For each phase it replays the byte addresses every lane of every wave issues per LDS instruction over one
workgroup's loop iterations and prices them with the gfx950 banking rules (MI355X_MICROARCH.md, LDS):
an instruction's lanes are serviced in fixed lane groups, one LDS cycle per group when conflict-free;
each extra distinct dword address on a bank within a group costs one more cycle.  Prints, per phase,
LDS-array cycles and the conflict share -- the same ratio as SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE.
Phase E is replayed twice: as 8 waves x 26 steps over 16 tile slots (the kernel before the split) and as the
2 K-halves x 4 column groups it runs now.
Usage: python3 scripts/lds_sim.py
"""
from collections import defaultdict

import numpy as np

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


def phase_a(ph):
    for w in range(NW):
        for u in range(w, 56, NW):
            mt, x0 = u >> 1, (u & 1) * 16
            for ky in range(5):
                addr = []
                for lane, i, g in lanes():
                    m = 16 * mt + i
                    img, rem = divmod(m, 56)
                    base = (OFF_XS1 if rem & 1 else OFF_XS) + 2 * (img * 1024 + (rem >> 1) * 32 + x0 + 8 * g)
                    addr.append(base + 2 * ky * 32)
                ph.add("b128", addr)


def pxtab():
    px = np.zeros(NM, dtype=np.int64)
    for m in range(NM):
        img, q = divmod(m, DC2_RS)
        if q >= 100:
            px[m] = img * 196
            continue
        win, d = divmod(q, 4)
        py, pxx = divmod(win, 5)
        px[m] = img * 196 + (2 * py + (d >> 1)) * 14 + 2 * pxx + (d & 1)
    return px


def phase_b(ph):
    PX = pxtab()
    for w in range(NW):
        for mt in range(w, NM // 16, NW):
            for s in range(7):
                addr = []
                for lane, i, g in lanes():
                    tap = 4 * s + g
                    toff = ((tap // 5) * 14 + tap % 5) * 8 if tap < 25 else 0
                    addr.append(OFF_P1 + 2 * (int(PX[16 * mt + i]) * 8 + toff))
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


def phase_e(ph, ph2=None, ph3=None, split=True):
    """A (dC2) reads into ph, the im2col B (P1) reads into ph2, the u16 pixel-index reads and (split) the
    cross-half exchange through P1 into ph3 (default: ph for all)."""
    PX = pxtab()
    ph2 = ph2 if ph2 is not None else ph
    ph3 = ph3 if ph3 is not None else ph
    for w, (s0, s1, tiles) in enumerate(e_waves(split)):
        for s in range(s0, s1):
            # A: two transposed reads of dC2 (ldAv: the swizzle term comes from the 8-row block)
            for half in range(2):
                addr = []
                for lane, i, g in lanes():
                    q, p = (lane & 15) >> 2, lane & 3
                    mA = 32 * s + 8 * g + q + 4 * half
                    b = 4 * s + g
                    sx = (b - 13 * ((b * 79) >> 10)) & 7
                    img, t = divmod(mA, DC2_RS)
                    assert (mA ^ sx) == img * DC2_RS + dc2_swz(t)
                    addr.append(OFF_DC2 + 2 * ((mA ^ sx) * 16 + 4 * p))
                ph.add("tr", addr)
            # the step's two pixel indices (PX + 8 g + q, + 4)
            for half in range(2):
                ph3.add("b16", [OFF_PX + 2 * (32 * s + 8 * g + ((lane & 15) >> 2) + 4 * half) for lane, i, g in lanes()])
            for T in tiles:
                for half in range(2):
                    addr = []
                    for lane, i, g in lanes():
                        q, p = (lane & 15) >> 2, lane & 3
                        mA = 32 * s + 8 * g + q + 4 * half
                        tap = 2 * T + (p >> 1)
                        tp = tap if tap < 25 else 0
                        toff = ((tp // 5) * 14 + tp % 5) * 8 + 4 * (p & 1)
                        addr.append(OFF_P1 + 2 * (int(PX[mA]) * 8 + toff))
                    ph2.add("tr", addr)
        if split:  # upper half writes, lower half reads [tile][lane] 16-byte pieces at the start of P1
            for T in tiles:
                ph3.add("b128", [OFF_P1 + (T * 64 + lane) * 16 for lane in range(64)])


def ftab():
    ft = np.full((98, 2, 16), 100, dtype=np.int64)
    for yx in range(98):
        y, X2 = divmod(yx, 7)
        for hf in range(2):
            for s in range(16):
                P = 2 * s + hf
                if P >= 30:
                    continue
                ky, u = divmod(P, 6)
                oy, ox = y - ky, 2 * X2 + 1 - u
                if 0 <= oy < 10 and 0 <= ox < 10:
                    ft[yx, hf, s] = (((oy >> 1) * 5 + (ox >> 1)) << 2) + ((oy & 1) << 1) + (ox & 1)
    return ft


def dc2_swz(t):
    return t ^ ((t >> 3) & 7)


def phase_f(ph):
    FT = ftab()
    for w in range(NW):
        for mt in range(w, 49, NW):
            for s in range(15):
                addr = []
                for lane, i, g in lanes():
                    m = 16 * mt + i
                    img, rem = divmod(m, 98)
                    t = int(FT[rem, g >> 1, s])
                    addr.append(OFF_DC2 + 2 * ((img * DC2_RS + dc2_swz(t)) * 16 + 8 * (g & 1)))
                ph.add("b128", addr)


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
    tot = conf = 0
    for name, fn in [("A conv1 (A reads)", phase_a), ("B conv2 (A reads)", phase_b),
                     ("E conv2 wgrad, 8 x 26 steps", lambda *p: phase_e(*p, split=False)),
                     ("E conv2 wgrad, 2 x 4 split", phase_e), ("F conv2 dgrad (A reads)", phase_f),
                     ("G conv1 wgrad", phase_g)]:
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
        if "8 x 26" in name:  # the kernel as it was: shown for comparison, not part of the total
            continue
        tot += c
        conf += k
    print(f"{'modelled total':<28} {'':13} LDS cycles {tot:7d}  conflict {conf:7d} ({100.0 * conf / tot:5.1f} %)")


if __name__ == "__main__":
    main()
