"""Fused LeNet-5 train kernel, conv1 forward with two kernel rows per MFMA step (csrc/lenet_fused.hip phase A,
csrc/lenet_frag.h ``lenet_conv1_frag_pos``): the position rule of the nine banded B fragments and the A
addressing that goes with it, replayed in numpy against a direct convolution; the LDS model's figures for the
phase (scripts/lds_sim.py) against the committed output.  No GPU."""
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG, XS_ELEMS = 8, 8 * 1024 + 32
NFRAG_C1, NFRAG_C1_USED = 15, 9  # FR_C2 - FR_C1; kConv1Frags


@pytest.fixture(scope="module")
def fmap():
    from distriflow_amd import native

    mp = native.require().lenet_conv1_frag_map().numpy()
    assert mp.shape == (150, 8) and mp.dtype == np.int32
    return mp.astype(np.int64)


def test_map_positions_are_distinct_and_inside_fragments_0_to_8(fmap):
    flat = fmap.reshape(-1)
    assert len(set(flat.tolist())) == 150 * 8
    assert flat.min() >= 0 and flat.max() < NFRAG_C1_USED * 512
    assert not ((flat >= NFRAG_C1_USED * 512) & (flat < NFRAG_C1 * 512)).any()
    # weight (c, ky, kx) lies in fragment (ky >> 1) * 3 + (c >> 1), once per band offset
    for j in range(150):
        c, ky = j // 25, (j % 25) // 5
        assert set((fmap[j] // 512).tolist()) == {(ky >> 1) * 3 + (c >> 1)}


def _b_matrices(fmap, w):
    """The nine B operands [f][k][n] the MFMA sees: element e of lane (i, g) is B[8 g + e][i]."""
    buf = np.zeros(NFRAG_C1 * 512)
    for j in range(150):
        buf[fmap[j]] = w[j]
    assert not buf[NFRAG_C1_USED * 512:].any()
    fr = buf.reshape(NFRAG_C1, 4, 16, 8)  # [f][g][i][e]
    return fr.transpose(0, 1, 3, 2).reshape(NFRAG_C1, 32, 16)


def test_replayed_kernel_addressing_is_the_same_convolution(fmap):
    rng = np.random.default_rng(0)
    w = rng.standard_normal(150)
    B = _b_matrices(fmap, w)
    # the padded images as phase 0 leaves them: [8][32][32], pixel (y, x) at (y + 2, x + 2), zero border and tail
    xs = np.zeros(XS_ELEMS)
    img = rng.uniform(0.1, 1.0, (IMG, 28, 28))  # no zero pixel: a read of the wrong place cannot hide
    xs[:IMG * 1024].reshape(IMG, 32, 32)[:, 2:30, 2:30] = img
    out = np.full((IMG, 6, 28, 28), np.nan)
    wrapped = clamped = crossing = 0
    for mt in range(14):
        rows = [divmod(16 * mt + i, 28) for i in range(16)]
        crossing += len({im for im, _ in rows}) > 1
        for xt in range(4):
            x0 = 8 * xt
            acc = np.zeros((3, 16, 16))
            for ks in range(3):
                A = np.zeros((16, 32))
                for i, (im, y) in enumerate(rows):
                    for g in range(4):
                        ky = 2 * ks + (g >> 1)
                        clamped += ky == 5
                        at = im * 1024 + (y + min(ky, 4)) * 32 + x0 + 8 * (g & 1)
                        assert at % 8 == 0 and at + 8 <= XS_ELEMS, "one aligned 16-byte read inside Xs"
                        wrapped += x0 + 8 * (g & 1) >= 32
                        A[i, 8 * g:8 * g + 8] = xs[at:at + 8]
                for T in range(3):
                    acc[T] += A @ B[ks * 3 + T]
            for T in range(3):
                for i, (im, y) in enumerate(rows):
                    for n in range(16):
                        x = x0 + (n & 7)
                        if x < 28:
                            assert np.isnan(out[im, 2 * T + (n >> 3), y, x]), "an output computed twice"
                            out[im, 2 * T + (n >> 3), y, x] = acc[T, i, n]
    assert wrapped and clamped and crossing >= 6, (wrapped, clamped, crossing)
    xp = xs[:IMG * 1024].reshape(IMG, 32, 32)
    ref = np.zeros((IMG, 6, 28, 28))
    w5 = w.reshape(6, 5, 5)
    for ky in range(5):
        for kx in range(5):
            ref += w5[None, :, ky, kx, None, None] * xp[:, None, ky:ky + 28, kx:kx + 28]
    assert not np.isnan(out).any()
    # fp64 on both sides, 25 terms of magnitude <= ~4: only the summation order differs
    assert np.abs(out - ref).max() < 1e-12


def _sim():
    spec = importlib.util.spec_from_file_location("lds_sim", os.path.join(ROOT, "scripts", "lds_sim.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_model_prices_phase_a_as_the_committed_output_says():
    sim = _sim()
    ph = sim.Phase("A")
    sim.phase_a(ph)
    assert (ph.n, ph.cyc, ph.cyc - ph.ideal) == (168, 1344, 672)
    old = sim.Phase("A before")
    sim.phase_a(old, rows2=False)
    assert (old.n, old.cyc, old.cyc - old.ideal) == (280, 1120, 0)
    text = open(os.path.join(ROOT, "profiles", "lenet_conv1_rows", "lds_sim.txt")).read()
    m = re.search(r"^A conv1 \(A reads\)\s+instr\s+(\d+)\s+LDS cycles\s+(\d+)\s+conflict\s+(\d+)", text, flags=re.M)
    assert m and tuple(int(v) for v in m.groups()) == (168, 1344, 672)
