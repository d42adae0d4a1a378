"""mo_kmeter_process_f64, the float64 yardstick of the dense K-meter kernels (tests/test_gpu_kmeter.py), tied to mo_kmeter_process, the
restatement that is bit-identical to the reference's Kmeterdsp (tests/test_needle_oracle_vs_ref.py).

The two are the same statements; the yardstick runs z1, z2 and the filter's arithmetic in double and rounds the states to f32 where the
reference stores them.  So they agree to the f32 recurrence's own rounding on programme material, bit for bit on everything that is not
the filter — the peak, its hold counter — and exactly wherever the flushes of kmeterdsp.cc:101-103 decide the reading (0, Inf).  How far
the f32 recurrence itself is from the double one is printed (pytest -s): on stationary inputs it stalls, which is why the kernels are
held to the yardstick and not to it."""
import numpy as np
import pytest

from test_gpu_kmeter import NF_CALLS, NF_FS, Yard, bind, bits, not_finite_batch, rate_signal, run_yard, signal


@pytest.mark.parametrize("fs", [48000.0, 44100.0])
def test_yardstick_matches_the_restatement_on_programme(oracle, fs):
    lib, S = bind(oracle.lib), 5
    calls = [1024, 1023, 4096 * 3 + 6, 4096 * 3 + 6, 1, 3, int(fs * 2) + 1, 512, 512, 512]   # test_kmeter_batch_matches_the_restatement's
    x = np.stack([signal(sum(calls), 300 + s, fs) for s in range(S)])
    a, b = Yard(lib, fs, S, 2, False), Yard(lib, fs, S, 2, True)
    pos = 0
    for i, n in enumerate(calls):
        a.process(x[:, pos:pos + n])
        b.process(x[:, pos:pos + n])
        pos += n
        assert np.array_equal(a.field("cnt"), b.field("cnt")), i
        assert np.array_equal(bits(a.field("peak")), bits(b.field("peak"))), i
        if i in {2, 3, 6, 9}:
            (ra, pa), (rb, pb) = a.read(), b.read()
            assert (np.abs(ra - rb) <= 1e-5 * np.maximum(ra, 1e-3)).all(), (i, ra, rb)
            assert np.array_equal(bits(pa), bits(pb)), i


@pytest.mark.parametrize("pair", [False, True])
def test_yardstick_flushes_as_the_restatement(oracle, pair):
    lib = bind(oracle.lib)
    clean, x, ch = not_finite_batch(pair)
    a, b = run_yard(lib, NF_FS, x, NF_CALLS, f64=False), run_yard(lib, NF_FS, x, NF_CALLS, f64=True)
    for i in range(2):
        (ra, pa), (rb, pb) = a[i], b[i]
        edge = (ra == 0) | np.isinf(ra) | (rb == 0) | np.isinf(rb)
        assert np.array_equal(bits(ra[edge]), bits(rb[edge])), (i, ra, rb)
        assert not np.isnan(ra).any() and not np.isnan(rb).any()
        assert np.array_equal(bits(pa), bits(pb)), i
        assert (np.abs(ra[~edge] - rb[~edge]) <= 1e-5 * ra[~edge]).all(), i
    r1 = a[0][0]
    assert all(r1[s, ch[s]] == 0 for s in (1, 2, 3, 4, 7)) and np.isinf(r1[5, ch[5]]) and edge.sum() == 0   # the second call reads neither


def test_gap_between_the_f32_and_the_double_recurrence(oracle):
    """A 1 s call from a zero state: |rms_f32 - rms_f64| / rms_f64, printed.  The f32 one-pole stalls on a stationary input — more the
    smaller omega is — so 1e-5 against the restatement cannot hold a kernel on DC or a sine; noise it can."""
    lib, gap = bind(oracle.lib), {}
    for kind in ("noise", "sine", "dc"):
        for fs in (8000.0, 48000.0, 192000.0):
            x = rate_signal(kind, int(fs), fs)[None]
            (ra, _), = run_yard(lib, fs, x, [int(fs)], f64=False)
            (rb, _), = run_yard(lib, fs, x, [int(fs)], f64=True)
            gap[kind, fs] = float(np.max(np.abs(ra.astype(np.float64) - rb) / rb))
        print("f32 against double recurrence, %-5s: " % kind + "  ".join("%g Hz %.1e" % (fs, gap[kind, fs]) for fs in (8000.0, 48000.0, 192000.0)))
    assert all(np.isfinite(v) for v in gap.values())
    assert gap["noise", 48000.0] < 1e-5 < gap["dc", 192000.0]
