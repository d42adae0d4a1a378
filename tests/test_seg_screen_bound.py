"""The bound behind k_seg's screened products (mtr_seg.hip: SCREEN), on the host.

A chunk's first product F = sum Ghi Xhi is kept; the other two, sum Ghi Xlo + Glo Xhi, may move an output by at most
eps = SCREEN_K_REL * M + SCREEN_K_ABS (accumulator units: scaled sample x 2^15), M = a bound on the column's scaled samples.
Here the split is modelled in numpy with the library's own tap table: the norms the derivation uses, the per-word bounds,
and |rest| plus the f32 rounding allowance of the four MFMAs that add it against eps, on random and adversarial windows —
full-scale alternating, impulses at the window's edges, samples just under 2^15, the clamped scale of levels under 2^-97
(f16 subnormals) and ring words rescaled in place."""
import os
import re

import numpy as np
import pytest

import meters.lv2_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "meters.lv2_amd", "csrc", "mtr_seg.hip")).read()
K_REL = np.float32(float(re.search(r"SCREEN_K_REL\s*=\s*([0-9.e+-]+)f", SRC).group(1)))
K_ABS = np.float32(float(re.search(r"SCREEN_K_ABS\s*=\s*([0-9.e+-]+)f", SRC).group(1)))
F16 = np.float16


def _taps():
    """A[p][m][t] of mtr_mfma16_fir.h (16 rows x 64 window positions per phase), as f16 hi / lo halves of g * 2^15."""
    tab = M.fir_table()
    g = np.zeros((3, 48), np.float32)
    for ph in range(1, 4):
        for i in range(48):
            g[ph - 1, i] = tab[24 * ph + i] if i < 24 else tab[24 * (4 - ph) + (47 - i)]
    h = g * np.float32(32768.0)
    hi = h.astype(F16)
    lo = (h - hi.astype(np.float32)).astype(F16)
    A_hi = np.zeros((3, 16, 64))
    A_lo = np.zeros((3, 16, 64))
    for m in range(16):
        A_hi[:, m, 1 + m:49 + m] = hi.astype(np.float64)
        A_lo[:, m, 1 + m:49 + m] = lo.astype(np.float64)
    return A_hi.reshape(48, 64), A_lo.reshape(48, 64)


A_HI, A_LO = _taps()


def _scale(mx):
    """Scale::set: a power of two that puts mx into [2^3, 2^4), clamped at 2^111 (levels under 2^-97)."""
    e = int(np.float32(mx).view(np.uint32) >> 23)
    se = min(238, 257 - e)
    return np.float32(2.0 ** (se - 127))


def _split(h):
    hi = h.astype(F16)
    lo = (h - hi.astype(np.float32)).astype(F16)      # x - Xhi is exact in f32; v_fma_mix rounds it once
    return hi, lo


def _check(hi, lo, M_):
    """|rest| + the MFMAs' rounding allowance <= eps, for all 48 outputs of one column; and the per-word bounds."""
    M_ = np.float32(M_)
    xh, xl = hi.astype(np.float64), lo.astype(np.float64)
    assert np.all(np.abs(xh) <= (1 + 2.0 ** -11) * M_ + 2.0 ** -24)
    assert np.all(np.abs(xl) <= 2.0 ** -11 * (1 + 2.0 ** -11) * M_ + 2.0 ** -24 * (1 + 2.0 ** -12))
    rest = A_HI @ xl + A_LO @ xh
    s_first = np.abs(A_HI) @ np.abs(xh)
    s_rest = np.abs(A_HI) @ np.abs(xl) + np.abs(A_LO) @ np.abs(xh)
    allowance = 2.0 ** -17 * (4 * (s_first + s_rest) + s_rest)     # four MFMAs: |C| + sum |products| each
    eps = np.float32(np.float32(K_REL * M_) + K_ABS)               # (fmaf in the kernel: one rounding, this one has two)
    worst = (np.abs(rest) + allowance).max()
    assert worst <= float(eps), (worst, float(eps), float(M_))
    return worst / float(eps)


def test_tap_norms_are_the_derivations():
    """LH = max row sum |Ghi| and LL = max row sum |Glo|, the two norms written next to the kernel."""
    LH = np.abs(A_HI).sum(1).max()
    LL = np.abs(A_LO).sum(1).max()
    assert LH <= 84157.0 and LL <= 11.41, (LH, LL)
    rel = (LH * 2.0 ** -11 + LL) * (1 + 2.0 ** -11) + 4 * 2.0 ** -17 * (LH + LL + 52.6)
    ab = (LH + LL) * 2.0 ** -24 * (1 + 2.0 ** -12)
    assert rel * (1 + 2.0 ** -20) < float(K_REL) and ab < float(K_ABS), (rel, ab)


def test_random_windows():
    rng = np.random.default_rng(1234)
    worst = 0.0
    for k in range(400):
        level = 2.0 ** rng.uniform(-60, 10)
        raw = (rng.standard_normal((64,)) * level).astype(np.float32)
        sc = _scale(np.abs(raw).max())
        h = raw * sc
        hi, lo = _split(h)
        worst = max(worst, _check(hi, lo, np.abs(h).max()))
    assert worst > 0.01                                           # (the bound is not vacuous on ordinary data)


def test_adversarial_windows():
    rng = np.random.default_rng(99)
    cases = []
    big = np.float32(2.0 ** 15 * (1 - 2.0 ** -12))
    cases.append(np.where(np.arange(64) % 2 == 0, big, -big).astype(np.float32))                     # full-scale alternating
    for pos in (0, 1, 62, 63):                                                                     # impulses at the edges
        v = np.zeros(64, np.float32)
        v[pos] = np.float32(2.0 ** 15 * 0.99997)
        cases.append(v)
    # samples whose lo word is as large as it gets, with the sign of each row's Ghi: the rest adds up coherently
    off = np.float32(1 + 2.0 ** -11 * 0.9999)
    for row in (0, 17, 40):
        cases.append((np.sign(A_HI[row]) * np.float32(2.0 ** 14) * off).astype(np.float32))
    cases.append((rng.uniform(-1, 1, 64) * 2.0 ** 15 * 0.9999).astype(np.float32))                  # near 2^15
    for v in cases:
        h = v.astype(np.float32)
        hi, lo = _split(h)
        _check(hi, lo, np.abs(h).max())


@pytest.mark.parametrize("level", [2.0 ** -97, 2.0 ** -110, 1e-38, 2.0 ** -140, 2.0 ** -149])
def test_subnormal_levels(level):
    """Levels under 2^-97: the scale is clamped at 2^111 and the scaled samples sit in f16's subnormals (or under them)."""
    rng = np.random.default_rng(7)
    for k in range(40):
        raw = (rng.uniform(-1, 1, 64) * level).astype(np.float32)
        if k % 4 == 0:
            raw[rng.integers(64)] = np.float32(level)
        mx = np.abs(raw).max()
        sc = _scale(mx)
        h = raw * sc
        hi, lo = _split(h)
        _check(hi, lo, np.abs(h).max())


@pytest.mark.parametrize("shift", [12, 13, 20, 24, 25, 30])
def test_rescaled_ring_words(shift):
    """Words split in one scale and rescaled in place by r = 2^-shift (an f16 multiply; r rounds to 0 under 2^-24), once and
    twice; M scales with them."""
    rng = np.random.default_rng(shift)
    r = F16(2.0 ** -shift)
    for k in range(60):
        level = 2.0 ** rng.uniform(-40, 0)
        raw = (rng.standard_normal(64) * level).astype(np.float32)
        sc = _scale(np.abs(raw).max())
        h = raw * sc
        hi, lo = _split(h)
        M_ = np.abs(h).max()
        for _ in range(2):
            hi, lo = (hi * r).astype(F16), (lo * r).astype(F16)
            M_ = np.float32(M_ * np.float32(r))
            _check(hi, lo, M_)
