"""The host model of k_seg's completion rule (tools/seg_screen_model.py) against the measured rates.

The model predicts what a change of the screen's rule buys before anybody builds it; it is worth that only while it
reproduces the rule that was measured.  Held here: on 16 streams of each of bench.py's three signals, the modelled share of
completed chunks under rule 1 (the stream reference without completed interpolated peaks) lies within 5 % (relative) of the
share measured on 8192 streams (profiles/r23_kseg_trim/completion_rates.txt), and the LCG of the model's signals is the
serial generator's.  No GPU and no library: numpy only."""
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
    """{signal: completed / screened} of the file's last block (old and new are equal there)."""
    out = {}
    for line in open(os.path.join(ROOT, "profiles", "r23_kseg_trim", "completion_rates.txt")):
        m = re.match(r"signal (\d): streams \d+ chunks screened (\d+) completed (\d+)", line)
        if m:
            out[int(m.group(1))] = int(m.group(3)) / int(m.group(2))
    assert sorted(out) == [0, 1, 2], out
    return out


def test_lcg_is_the_serial_generator(model):
    u = model.lcg_noise(1000, 777)
    s, want = 777, []
    for _ in range(2000):
        s = (1664525 * s + 1013904223) & 0xFFFFFFFF
        want.append(np.float32((s >> 8) - (1 << 23)) / np.float32(1 << 23))
    assert np.array_equal(u.reshape(-1), np.array(want, np.float32))


def test_taps_are_the_library_table(model):
    """the model's float64 taps against the library's table (rounded to f32 there)"""
    import meters.lv2_amd as M
    tab = M.fir_table()
    g = model.taps()
    for ph in (1, 2, 3):
        for i in range(48):
            assert abs(g[ph - 1, i] - (tab[24 * ph + i] if i < 24 else tab[24 * (4 - ph) + (47 - i)])) < 1e-7


@pytest.mark.parametrize("kind", [1, 0, 2])
def test_rule_1_reproduces_the_measured_rate(model, kind):
    scr, fin = model.run(kind, 16, 1)
    got, want = fin / scr, _measured()[kind]
    print("signal %d: modelled %.4f measured %.4f (%+.1f %%)" % (kind, got, want, 100 * (got / want - 1)))
    assert abs(got - want) <= 0.05 * want, (kind, got, want)
