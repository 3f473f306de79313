#!/usr/bin/env python3
"""Search for a conv2 forward tap order of the fused LeNet-5 train kernel (phase B of csrc/lenet_fused.hip;
the fragment maps of csrc/lenet_frag.h) with scripts/lds_sim.py's banking model.  The order it finds
(lds_sim.C2_ORDER) removed the modelled and the measured bank conflicts of phase B but not its time, and was
not adopted (docs/RESULTS.md): the kernel gives slot k tap k.

Phase B's K-step s gives lane group g the tap order[4 s + g] (28 slots for 25 taps; a slot without a tap reads
at tap 0's offset against zero weights).  A ds_read_b128 serves lanes 0 .. 31 (g = 0, 1) and lanes 32 .. 63
(g = 2, 3) in separate groups, so an order's LDS cycles are the sum over its 14 slot pairs (4 s, 4 s + 1) and
(4 s + 2, 4 s + 3) of a pair cost that depends only on the two taps and on how the 16 rows of a tile are
composed: "cross" = one pool window of 4 consecutive images (the full-batch kernel), "image" = 16 consecutive
window-order rows of one image's 104-row block (the trimmed kernel).  The search minimises the cross cost over
pairings by random-restart pair exchanges, keeping the image cost no worse than today's order (slot k = tap k).

Usage: python3 scripts/lds_tap_search.py [seconds] [seed]
"""
import random
import sys
import time

import lds_sim as S

NTILE = S.NM // 16
PAD = 25  # a slot without a tap


def tile_pixels(comp, mt):
    """P1 pixel (over the workgroup's 8 images) of tile row i"""
    wp = S.winpix()
    if comp == "cross":
        win, i0 = mt % 26, 4 * (mt // 26)
        return [(i0 + (i >> 2)) * 196 + int(wp[4 * win + (i & 3)]) for i in range(16)]
    return [(m // S.DC2_RS) * 196 + int(wp[m % S.DC2_RS]) for m in range(16 * mt, 16 * mt + 16)]


def tap_off(tap):
    """pixel offset of a tap (a slot without a tap: tap 0's)"""
    return (tap // 5) * 14 + tap % 5 if tap < 25 else 0


def pair_costs(comp):
    """cost[a][b]: LDS cycles over all tiles of 32 lanes, lanes 0 .. 15 on tap a and lanes 16 .. 31 on tap b"""
    tiles = [tile_pixels(comp, mt) for mt in range(NTILE)]
    cost = [[0] * 26 for _ in range(26)]
    for a in range(26):
        for b in range(26):
            tot = 0
            for px in tiles:
                addr = [S.OFF_P1 + 16 * (p + tap_off(a)) for p in px] + [S.OFF_P1 + 16 * (p + tap_off(b)) for p in px]
                # lanes 32 .. 63 idle: their two service groups cost the minimum of one cycle each
                tot += S.cycles("b128", addr + [None] * 32)[0] - 2
            cost[a][b] = tot
    return cost


def order_cost(cost, order):
    return sum(cost[order[k]][order[k + 1]] for k in range(0, 28, 2))


def search(seconds, seed):
    cross, image = pair_costs("cross"), pair_costs("image")
    today = list(range(25)) + [PAD] * 3
    bound = order_cost(image, today)
    rng = random.Random(seed)
    best, best_c = None, None
    t0 = time.time()
    while time.time() - t0 < seconds:
        cur = today[:]
        rng.shuffle(cur)
        # penalised objective: the image composition may not cost more than it does today
        f = lambda o: order_cost(cross, o) + 1000 * max(0, order_cost(image, o) - bound)  # noqa: E731
        c, stale = f(cur), 0
        while stale < 4000:
            i, j = rng.randrange(28), rng.randrange(28)
            if cur[i] == cur[j]:
                stale += 1
                continue
            cur[i], cur[j] = cur[j], cur[i]
            n = f(cur)
            if n <= c:
                stale = stale + 1 if n == c else 0
                c = n
            else:
                cur[i], cur[j] = cur[j], cur[i]
                stale += 1
        if best_c is None or c < best_c:
            best, best_c = cur[:], c
    # canonical form: pairs in the order of their first tap; the taps keep their (even, odd) roles
    pairs = sorted((best[k], best[k + 1]) for k in range(0, 28, 2))
    order = [t for p in pairs for t in p]
    return order, cross, image, today


def main():
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 70.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    order, cross, image, today = search(seconds, seed)
    print(f"model LDS cycles of phase B's A reads per workgroup (8 images, {NTILE} tiles):")
    for name, o in (("today (slot k = tap k)", today), ("found", order)):
        print(f"  {name:<24} cross-image tiles {order_cost(cross, o):5d}   per-image tiles {order_cost(image, o):5d}")
    print("order (tap of slot 4 s + g; 25 = no tap):")
    print("  " + ", ".join(str(t) for t in order))


if __name__ == "__main__":
    main()
