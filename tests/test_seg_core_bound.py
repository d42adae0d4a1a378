"""The bound behind k_seg's core screen (mtr_seg.hip: the core screen, CORE), on the host: the counterpart of test_seg_screen_bound.py.

A chunk's screen product is F' = the sum of Ghi Xhi over each row's core — the taps inside one 32-sample stretch of the window,
three fragments of 16 rows (mtr_mfma16_fir.h: mtr_m16_build_core) — and the dense value Y = sum Ghi Xhi + Ghi Xlo + Glo Xhi may
differ from it by at most eps' = CORE_K_REL * M + CORE_K_ABS (accumulator units: scaled sample x 2^15), M = a bound on the column's
scaled samples.  Here the fragments are rebuilt in numpy from the library's tap table and the row table (row n = 3 f + p of the
frame-major list goes to fragment n // 16, stretch [8 (w + 1), 8 (w + 1) + 32)) and pinned to what the library builds, bit for bit;
LT (the largest row sum of dropped |Ghi|) and the constants are held to the derivation next to the kernel; and |Y - F'| plus the
f32 rounding allowance of the six dense MFMAs and the one core MFMA an output lies in stays under eps' on random windows, windows
that follow the signs of each row's dropped taps at full scale, impulses at the window's edges, samples just under 2^15, the
subnormal levels and ring words rescaled in place once and twice."""
import ctypes
import os
import re

import numpy as np
import pytest

import meters.lv2_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "meters.lv2_amd", "csrc", "mtr_seg.hip")).read()
K_REL = np.float32(float(re.search(r"\bCORE_K_REL\s*=\s*([0-9.e+-]+)f", SRC).group(1)))
K_ABS = np.float32(float(re.search(r"\bCORE_K_ABS\s*=\s*([0-9.e+-]+)f", SRC).group(1)))
F16 = np.float16


def _taps():
    """A[p][m][t] of mtr_mfma16_fir.h (16 rows x 64 window positions per phase), f16 hi / lo halves of g * 2^15, and hi's bits."""
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
    bits = np.zeros((3, 16, 64), np.uint16)
    for m in range(16):
        A_hi[:, m, 1 + m:49 + m] = hi.astype(np.float64)
        A_lo[:, m, 1 + m:49 + m] = lo.astype(np.float64)
        bits[:, m, 1 + m:49 + m] = hi.view(np.uint16)
    return A_hi, A_lo, bits


_AH, _AL, _BITS = _taps()
# frame-major rows: n = 3 f + p
ROWS = [(n // 3, n % 3) for n in range(48)]
A_HI = np.stack([_AH[p, f] for f, p in ROWS])                        # [48, 64]
A_LO = np.stack([_AL[p, f] for f, p in ROWS])
STRETCH = [8 * (n // 16 + 1) for n in range(48)]                     # first window position of row n's stretch
A_CORE = np.zeros((48, 64))
for _n in range(48):
    A_CORE[_n, STRETCH[_n]:STRETCH[_n] + 32] = A_HI[_n, STRETCH[_n]:STRETCH[_n] + 32]
A_TAIL = A_HI - A_CORE                                               # the dropped taps
LH = np.abs(A_HI).sum(1).max()
LL = np.abs(A_LO).sum(1).max()
LT = np.abs(A_TAIL).sum(1).max()


def test_fragments_are_the_librarys():
    """Fragment w, lane (m' = lane & 15, kg = lane >> 4), half e = Ghi of row 16 w + m' at window position 8 (w + 1) + 8 kg + e."""
    want = np.zeros((3, 64, 8), np.uint16)
    for w in range(3):
        for lane in range(64):
            f, p = ROWS[16 * w + (lane & 15)]
            t0 = 8 * (w + 1) + 8 * (lane >> 4)
            want[w, lane] = _BITS[p, f, t0:t0 + 8]
    got = np.zeros(3 * 64 * 8, np.uint16)
    assert M.lib.mtr_debug_m16_core(ctypes.c_void_p(got.ctypes.data)) == 0
    assert np.array_equal(got.reshape(3, 64, 8), want), np.argwhere(got.reshape(3, 64, 8) != want)[:8]
    # every row keeps at least 98.7 % of its L1 norm inside its fragment's stretch (LT = 854.62 against the smallest row norm, 2.13 x 2^15)
    kept = np.abs(A_CORE).sum(1)
    assert (kept > 0.987 * np.abs(A_HI).sum(1)).all(), (kept / np.abs(A_HI).sum(1)).min()


def test_tail_norm_and_constants_are_the_derivations():
    assert LH <= 84157.0 and LL <= 11.41 and 854.0 < LT <= 854.62, (LH, LL, LT)
    assert abs(LT / 32768.0 - 0.02608) < 1e-5
    S = (LH + LL) * (1 + 2.0 ** -11) + 52.6                           # |C| + sum |products| of a dense MFMA, per M
    rel = (LH * 2.0 ** -11 + LL) * (1 + 2.0 ** -11) + LT * (1 + 2.0 ** -11) + 6 * 2.0 ** -17 * S + 2.0 ** -17 * LH * (1 + 2.0 ** -11)
    ab = (LH + LL) * 2.0 ** -24 * (1 + 2.0 ** -12) + LT * 2.0 ** -24 + 7 * 2.0 ** -17 * (LH + LL) * 2.0 ** -24
    assert rel < 912.06 and rel * (1 + 2.0 ** -20) < float(K_REL) and ab < 0.00508 and ab < float(K_ABS), (rel, ab)
    assert float(K_REL) < 1.01 * rel, "the constant is the derivation's sum, rounded up by under 1 %"


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
    """|Y - F'| + the MFMAs' rounding allowance <= eps', for all 48 outputs of one column; and the per-word bound on Xhi."""
    M_ = np.float32(M_)
    xh, xl = hi.astype(np.float64), lo.astype(np.float64)
    assert np.all(np.abs(xh) <= (1 + 2.0 ** -11) * M_ + 2.0 ** -24)
    dense = A_HI @ xh + A_HI @ xl + A_LO @ xh
    core = A_CORE @ xh
    s_dense = np.abs(A_HI) @ (np.abs(xh) + np.abs(xl)) + np.abs(A_LO) @ np.abs(xh)
    s_core = np.abs(A_CORE) @ np.abs(xh)
    allowance = 2.0 ** -17 * (6 * s_dense + s_core)                  # six dense MFMAs and one core MFMA: |C| + sum |products| each
    eps = np.float32(np.float32(K_REL * M_) + K_ABS)                 # (fmaf in the kernel: one rounding, this one has two)
    worst = (np.abs(dense - core) + allowance).max()
    assert worst <= float(eps), (worst, float(eps), float(M_))
    return worst / float(eps)


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


def test_windows_aligned_with_the_dropped_taps():
    """Full-scale samples with the signs of each row's dropped taps (the kept ones' elsewhere): the tail adds up coherently, and with
    the lo words as large as they get the rest does too.  The worst row comes within a few per cent of the bound."""
    off = np.float32(1 + 2.0 ** -11 * 0.9999)
    worst = 0.0
    for n in range(48):
        sg = np.where(A_TAIL[n] != 0, np.sign(A_TAIL[n]), np.where(A_HI[n] != 0, np.sign(A_HI[n]), 1.0))
        for amp in (np.float32(2.0 ** 15 * (1 - 2.0 ** -12)), np.float32(2.0 ** 14) * off):
            h = (sg * amp).astype(np.float32)
            hi, lo = _split(h)
            worst = max(worst, _check(hi, lo, np.abs(h).max()))
    assert worst > 0.9, worst                                     # (K_REL' is tight: LT is reached)


def test_adversarial_windows():
    rng = np.random.default_rng(99)
    cases = []
    big = np.float32(2.0 ** 15 * (1 - 2.0 ** -12))
    cases.append(np.where(np.arange(64) % 2 == 0, big, -big).astype(np.float32))                     # full-scale alternating
    for pos in (0, 1, 7, 8, 23, 24, 39, 40, 55, 56, 62, 63):                                         # impulses at the window's and the stretches' edges
        v = np.zeros(64, np.float32)
        v[pos] = np.float32(2.0 ** 15 * 0.99997)
        cases.append(v)
    cases.append((rng.uniform(-1, 1, 64) * 2.0 ** 15 * 0.9999).astype(np.float32))                  # near 2^15
    cases.append(np.full(64, np.float32(2.0 ** 15 * (1 - 2.0 ** -13)), np.float32))
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
