"""tests/_gate.py — the restatement the gate kernels are held to — anchored to the oracle, and the programmes shown to reach the gate's
edges (no GPU).

oracle.ebu (x, 8000, block, want_frag=True) gives each programme's fragment powers and its final record; the model is fed those powers.
  * both histograms and both counts: bit for bit;
  * M, S, max M, max S: within ULP_DB = 10 x spacing (float32 (32)) = 3.8e-5 dB — the oracle rounds glibc's log10f, the model a double
    log10; they differ by at most one float32 ulp of a logarithm under 32, times ten, so bit equality is not demanded; the largest
    deviation is printed;
  * I, I_thr, Rmin, Rmax, R_thr of the model's snapshot at the last wrap through hist_loudness (log10f on both sides): bit for bit the
    oracle's;
  * the model fed call by call at the GPU tests' cuts ends where the model fed in one call ends;
  * coverage (_gate.assert_coverage), on the oracle's own results.
"""
import numpy as np
import pytest

import _gate as G

BLOCK = 1024


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def runs(oracle):
    x = G.batch()
    return {nm: oracle.ebu(x[s], G.FS, BLOCK, want_frag=True) for s, nm in enumerate(G.NAMES)}


def test_model_gives_the_oracles_record(runs):
    worst = 0.0
    for nm, o in runs.items():
        assert o["frag_power"].size == G.NFRAG
        g = G.Gate()
        r = g.call_powers(o["frag_power"])
        assert np.array_equal(r["hist_M"], o["hist_M"]) and np.array_equal(r["hist_S"], o["hist_S"]), nm
        assert tuple(r["count"]) == tuple(o["counts"]), (nm, r["count"], o["counts"])
        got = np.array([r["last_M"], r["max_M"], r["last_S"], r["max_S"]], np.float64)
        dev = np.abs(got - o["out9"][:4].astype(np.float64)).max()
        worst = max(worst, dev)
        assert dev <= G.ULP_DB, (nm, got, o["out9"][:4])
        e = G.expected(r["snap_M"], r["snap_S"])
        want = [e[k] for k in ("I", "I_thr", "Rmin", "Rmax", "R_thr")]
        assert np.array_equal(_bits(want), _bits(o["out9"][4:])), (nm, want, o["out9"][4:])
    print(f"\nmodel against the oracle, {len(runs)} programmes of {G.NFRAG} fragments: largest |d| of M, S, max M, max S {worst:.2e} dB (bound {G.ULP_DB:.2e})")
    print("steady stream: %.4f LUFS for a target of -23" % runs["steady"]["out9"][2])


def test_model_call_by_call_is_the_model_in_one_call(runs):
    ends = G.call_ends(G.NFRAG * G.FRAG + G.TAIL)
    for nm in ("up", "late", "fuzz0", "over"):
        p = runs[nm]["frag_power"]
        one, g, a = G.Gate().call_powers(p), G.Gate(), 0
        M, S = [], []
        for e in ends:
            r = g.call_powers(p[a:e // G.FRAG])
            a = e // G.FRAG
            M.append(r["M"])
            S.append(r["S"])
        assert np.array_equal(_bits(np.concatenate(M)), _bits(one["M"])) and np.array_equal(_bits(np.concatenate(S)), _bits(one["S"]))
        for k in ("hist_M", "hist_S", "count", "error", "wraps", "snap_M", "snap_S"):
            assert np.array_equal(r[k], one[k]), (nm, k)
        # the series alone drives the bookkeeping to the same record
        b = G.Gate().call_ms(one["M"], one["S"])
        assert np.array_equal(b["hist_M"], one["hist_M"]) and np.array_equal(b["hist_S"], one["hist_S"])


def test_integr_off_moves_no_count_and_no_divider():
    rng = np.random.default_rng(3)
    p = (10.0 ** rng.uniform(-5, 0, 45)).astype(np.float32)
    g = G.Gate()
    g.call_powers(p[:13])
    before = (g.hist.copy(), g.count.copy(), g.div1, g.div2)
    r = g.call_powers(p[13:24], integr=False)
    assert np.array_equal(g.hist, before[0]) and np.array_equal(g.count, before[1]) and (g.div1, g.div2) == before[2:]
    assert r["last_M"] == r["M"][-1] and r["max_M"] >= r["M"].max()
    r = g.call_powers(p[24:])                          # div2 stood at 3: the next S point comes 7 fragments on, at fragment 30
    assert r["count"][1] == 1 + (45 - 24 - 7) // 10 + 1


def test_programmes_reach_the_edges(runs, oracle):
    rec = {}
    for nm, o in runs.items():
        rec[nm] = dict(hist_M=o["hist_M"], hist_S=o["hist_S"], count=o["counts"], wraps=(G.NFRAG // 2, G.NFRAG // 10),
                       I_thr=o["out9"][5], R_thr=o["out9"][8], Rmin=o["out9"][6], Rmax=o["out9"][7])
    x = G.batch()[G.NAMES.index("late")]
    rec["late"]["counts_per_call"] = [tuple(oracle.ebu(x[:e], G.FS, BLOCK)["counts"]) for e in G.call_ends(x.shape[0])]
    G.assert_coverage(rec)
