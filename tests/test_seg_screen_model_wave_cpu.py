"""The host model's per-wave figure (tools/seg_screen_model.py: wave_steps), pinned.

k_seg's lazy form (MTR_SEG_SCREEN=3) pays for a completion per wave and step — a step of a wave in which at least one chunk
completes takes the cold branch and builds lo words there — so what its cold path may cost was estimated from the share of a
wave's steps with at least one completing chunk, not from the share of completed chunks.  Held here: for 16 streams (two waves of
8) under rule 2, on bench.py's three signals, that share is what the tool printed when the lazy form was decided on, 0.0232 /
0.0259 / 0.0879 (signals 1 / 0 / 2), within +-0.002 absolute: the envelopes are float64 and the run is deterministic, so the band
only covers a different libm.  No GPU and no library: numpy only."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PINNED = {1: 0.0232, 0: 0.0259, 2: 0.0879}


@pytest.fixture(scope="module")
def model():
    spec = importlib.util.spec_from_file_location("seg_screen_model", os.path.join(ROOT, "tools", "seg_screen_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("kind", [1, 0, 2])
def test_share_of_a_waves_steps_that_complete(model, kind):
    share, per_step = model.wave_steps(kind, 16, 2)
    print("signal %d: a wave completes in %.4f of its steps, %.2f chunks per such step" % (kind, share, per_step))
    assert abs(share - PINNED[kind]) <= 0.002, (kind, share, PINNED[kind])
    assert 1.0 <= per_step <= 8.0, per_step


def test_waves_do_not_change_the_chunk_counts(model):
    """the per-wave bookkeeping is a by-product: run () counts the same chunks with and without it"""
    w = {}
    assert model.run(1, 8, 2, waves=w) == model.run(1, 8, 2)
    assert w["steps"] == 3749 and 0 < w["cold"] <= w["chunks"]
