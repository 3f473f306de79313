"""Generate tests/golden/convpool_cases.json: the shapes of the exact fused conv+pool tests.

    python scripts/convpool_cases.py

csrc/convpool.hip picks one of about 50 template instantiations per launch from three lists.  What decides
is the plan of the geometry, which the bindings give without a GPU (``ops.convpool_plan``), so the list is
generated, not guessed: over a bounded space of geometries the script reads three keys per supported geometry,

    fwd    (pair, cdiv(N, 16), Kpad2 / 32)            forward: pair / plain, channel tiles, k steps
    wgrad  (cdiv(N, 16), cdiv(K + 1, 16))             weight gradient: channel tiles, k tiles (bias column)
    dgrad  (pair | vec (N % 8 == 0) | scalar, K2pad / 32)

and greedily picks geometries until every distinct key VALUE is covered (most uncovered keys first, the
cheapest among equals).  Covering values rather than instantiations means the test does not depend on the
instantiation lists, and it runs instantiations partly filled as well as full.  No GPU needed; the
extension must be built (as for scripts/conv_plan_fixture.py).
"""
from __future__ import annotations

import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "convpool_cases.json")

KS = (1, 2, 3, 5, 7)
HS = (6, 8, 10, 12, 14, 16)
CS = (1, 2, 3, 4, 6, 8, 12, 16)
NS = (1, 4, 6, 8, 12, 16, 20, 32)
BATCH = 3   # odd, more than one workgroup


def keys_of(H, W, C, N, k, pad):
    """The three dispatch keys of one geometry, as JSON-friendly lists."""
    from distriflow_amd import ops
    p = ops.convpool_plan(H, W, C, k, k, pad, N)
    return {kind: p[kind]["key"] for kind in ("fwd", "wgrad", "dgrad")}


def space():
    for k in KS:
        for pad in sorted({0, (k - 1) // 2, k - 1}):
            for H, C, N in itertools.product(HS, CS, NS):
                yield H, H, C, N, k, pad


def cost(H, W, C, N, k, pad):
    return (H + 2 * pad) * (W + 2 * pad) * C * N * k * k


def tagged(keys):
    return {(kind, json.dumps(v)) for kind, v in keys.items()}


def main():
    from distriflow_amd import ops
    geoms = [g for g in space() if ops.convpool_supported(g[0], g[1], g[2], g[4], g[4], g[5], g[3])]
    keys = {g: tagged(keys_of(*g)) for g in geoms}
    todo = set().union(*keys.values())
    covered = {kind: sorted(json.loads(v) for kd, v in todo if kd == kind) for kind in ("fwd", "wgrad", "dgrad")}
    geoms.sort(key=lambda g: (cost(*g), g))   # cheapest first: max() below keeps the first among equals
    picked = []
    while todo:
        best = max(geoms, key=lambda g: len(keys[g] & todo))
        assert keys[best] & todo
        todo -= keys[best]
        picked.append(best)
    picked.sort(key=lambda g: (cost(*g), g))
    cases = [dict(B=BATCH, H=g[0], W=g[1], C=g[2], N=g[3], k=g[4], pad=g[5], **keys_of(*g)) for g in picked]
    with open(OUT, "w") as f:
        f.write('{"space": ' + json.dumps(dict(k=KS, H=HS, C=CS, N=NS, pad="0, (k-1)//2, k-1", supported=len(geoms))))
        f.write(',\n "covered": {\n')
        f.write(",\n".join(f'  "{kind}": {json.dumps(covered[kind])}' for kind in ("fwd", "wgrad", "dgrad")))
        f.write('\n },\n "cases": [\n')
        f.write(",\n".join("  " + json.dumps(c) for c in cases))
        f.write("\n]}\n")
    print(f"{len(geoms)} supported geometries, {sum(map(len, covered.values()))} keys, {len(cases)} cases -> {OUT}")


if __name__ == "__main__":
    main()
