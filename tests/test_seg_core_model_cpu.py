"""The host model's core rule (tools/seg_screen_model.py, rule 4) against the completion rates measured on the full shape.

k_seg's core form (MTR_SEG_SCREEN=4) votes on the truncated product — each row's taps inside the 32-sample stretch of its fragment —
with eps' = CORE_K_REL M; the model's rule 4 votes on that product itself, in the core's row layout, and folds completed chunks'
exact outputs as every rule does.  Held here, with the tolerance test_seg_screen_model_cpu.py uses for the rule it pins: on 16
streams of each of bench.py's three signals the modelled share of completed chunks lies within 5 % (relative) of the share measured
on 8192 streams under form 4 (profiles/r30_kseg_core/completion_rates.txt); the model's constant is the kernel's; and its core
matrix is the library's fragments.  No GPU: numpy and the library's host entry points only."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    spec = importlib.util.spec_from_file_location("seg_screen_model", os.path.join(ROOT, "tools", "seg_screen_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _measured():
    """{signal: completed / screened} of the file's MTR_SEG_SCREEN=4 block."""
    out, on = {}, False
    for line in open(os.path.join(ROOT, "profiles", "r30_kseg_core", "completion_rates.txt")):
        if "MTR_SEG_SCREEN=" in line:
            on = "MTR_SEG_SCREEN=4" in line
        m = re.match(r"signal (\d): streams \d+ chunks screened (\d+) completed (\d+)", line)
        if m and on:
            out[int(m.group(1))] = int(m.group(3)) / int(m.group(2))
    assert sorted(out) == [0, 1, 2], out
    return out


def test_constant_is_the_kernels(model):
    src = open(os.path.join(ROOT, "meters.lv2_amd", "csrc", "mtr_seg.hip")).read()
    k = float(re.search(r"\bCORE_K_REL\s*=\s*([0-9.e+-]+)f", src).group(1))
    assert model.K_REL_CORE == k / 32768.0


def test_core_matrix_is_the_librarys_fragments(model):
    """where the library's fragments hold a tap the model's matrix holds it too (to the f16 rounding of g * 2^15), zeros alike"""
    import meters.lv2_amd as M
    got = np.zeros(3 * 64 * 8, np.uint16)
    assert M.lib.mtr_debug_m16_core(ctypes.c_void_p(got.ctypes.data)) == 0
    frag = got.view(np.float16).astype(np.float64).reshape(3, 64, 8)
    cm = model.core_matrix(model.taps()) * 32768.0
    for w in range(3):
        for lane in range(64):
            n, t0 = 16 * w + (lane & 15), 8 * (w + 1) + 8 * (lane >> 4)
            assert np.all(np.abs(frag[w, lane] - cm[n, t0:t0 + 8]) <= 2.0 ** -11 * np.abs(cm[n, t0:t0 + 8]) + 1e-2), (w, lane)
            assert np.array_equal(frag[w, lane] == 0, cm[n, t0:t0 + 8] == 0), (w, lane)
    for n in range(48):
        w = n // 16
        assert not cm[n, :8 * (w + 1)].any() and not cm[n, 8 * (w + 1) + 32:].any()


@pytest.mark.parametrize("kind", [1, 0, 2])
def test_core_rule_reproduces_the_measured_rate(model, kind):
    scr, fin = model.run(kind, 16, 4)
    got, want = fin / scr, _measured()[kind]
    print("signal %d: modelled %.4f measured %.4f (%+.1f %%)" % (kind, got, want, 100 * (got / want - 1)))
    assert abs(got - want) <= 0.05 * want, (kind, got, want)
