"""The numpy restatement of DR-14 (tests/_dr14.py) pinned to the oracle's (mo_dr14_run, oracle/mtr_oracle.c), on the very inputs of
tests/test_gpu_dr14_score.py in the same call blocks; and those inputs held to what they are meant to exercise.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import _dr14 as D
from _oracle import MoTp
from test_gpu_dr14 import Ports

F = C.c_float


class MoKmeter(C.Structure):                                         # mo_kmeter (oracle/mtr_oracle.h)
    _fields_ = [("z1", F), ("z2", F), ("rms", F), ("peak", F), ("cnt", C.c_int), ("fpp", C.c_int), ("fall", F), ("flag", C.c_int),
                ("hold", C.c_int), ("fsamp", F), ("omega", F)]


class MoDr14(C.Structure):                                           # mo_dr14
    _fields_ = [("n_channels", C.c_int), ("dr_mode", C.c_int), ("rate", C.c_double), ("n_sample_cnt", C.c_uint64),
                ("sample_count", C.c_uint64), ("num_fragments", C.c_uint64), ("m_dbtp", F * 2), ("m_peak", F * 2), ("m_rms", F * 2),
                ("rms_sum", F * 2), ("peak_cur", F * 2), ("peak_hist", F * 2 * 2), ("km", MoKmeter * 2), ("tp", MoTp * 2),
                ("hist", C.c_uint32 * D.HISTBINS * 2)]


def oracle_readings(oracle, x, fs, calls):
    """mo_dr14_run over x [T, C] in the call blocks (8192 frames at a time: TruePeakdsp::process takes no more); after every call
    (ports, m_peak [C] of the score, num_fragments, hist [C, 8000], peak_hist [C, 2])"""
    lib, chn = oracle.lib, x.shape[1]
    lib.mo_dr14_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double]
    lib.mo_dr14_run.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(Ports)]
    d = MoDr14()
    lib.mo_dr14_init(C.byref(d), chn, 1, float(fs))
    assert d.n_sample_cnt == D.window(fs) - 1 and d.m_rms[0] == -81 and d.n_channels == chn      # (the layout above is the library's)
    chans = [np.ascontiguousarray(x[:, c]) for c in range(chn)]
    out, pos, ports = [], 0, Ports()
    for n in calls:
        for q in range(pos, pos + n, 8192):
            m = min(8192, pos + n - q)
            ptrs = (C.c_void_p * 2)(*[ch.ctypes.data + 4 * q for ch in chans], *([None] * (2 - chn)))
            lib.mo_dr14_run(C.byref(d), ptrs, m, C.byref(ports))
        pos += n
        out.append((Ports.from_buffer_copy(ports), list(d.m_peak)[:chn], int(d.num_fragments),
                    np.ctypeslib.as_array(d.hist)[:chn].copy(), np.ctypeslib.as_array(d.peak_hist)[:chn].copy()))
    return out


WORST = {"cpu": 0.0}


def against_the_oracle(oracle, x, fs, calls):
    a, b = D.checked(x, fs, calls)
    assert [r[:10] for r in a.readings] == [r[:10] for r in b.readings]                    # equal bins: the same score, bit for bit
    assert all(np.array_equal(p.hist, q.hist) and np.array_equal(p.peak_hist, q.peak_hist) for p, q in zip(a.readings, b.readings))
    chn = x.shape[1]
    for i, (r, (ports, m_peak, nf, hist, ph)) in enumerate(zip(b.readings, oracle_readings(oracle, x, fs, calls))):
        if i == 0 and calls[0] == 0:
            continue
        assert r.num_fragments == nf and r.block_count == ports.block_count, (i, r.num_fragments, nf)
        assert np.array_equal(r.hist, hist), (i, np.argwhere(r.hist != hist))
        assert np.array_equal(r.peak_hist, ph), (i, r.peak_hist, ph)
        dev = [abs(r.m_rms[c] - ports.m_rms[c]) for c in range(chn)] + [abs(r.m_peak[c] - m_peak[c]) for c in range(chn)] \
            + [abs(r.dr[c] - ports.dr[c]) for c in range(chn)] + [abs(r.dr_total - ports.dr_total)]
        WORST["cpu"] = max(WORST["cpu"], float(max(dev)))
        assert max(dev) <= D.TOL_SCORE, (i, dev, r[:5])
    return a


def streams(kind, fs):
    if kind == "many":
        c = D.many_windows(fs)
    elif kind == "small":
        c = D.small(fs)
    else:
        c = D.edge_case(fs, D.window(fs) + int(kind[4:]))
    return c


KINDS = ["many", "small", "edge-1", "edge+0", "edge+1"]


@pytest.mark.parametrize("fs", D.RATES)
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_matches_the_oracle_stereo(oracle, kind, fs):
    c = streams(kind, fs)
    for s in range(c.x.shape[0]):
        against_the_oracle(oracle, c.x[s], fs, c.calls)
    print("worst deviation from mo_dr14_run so far: %.3g dB" % WORST["cpu"])


@pytest.mark.parametrize("fs", D.RATES)
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_matches_the_oracle_mono(oracle, kind, fs):
    c = streams(kind, fs)
    c = D.edge_mono(c) if kind.startswith("edge") else D.mono(c)
    for s in range(c.x.shape[0]):
        against_the_oracle(oracle, c.x[s], fs, c.calls)
    print("worst deviation from mo_dr14_run so far: %.3g dB" % WORST["cpu"])


@pytest.mark.parametrize("fs", D.RATES)
def test_restatement_matches_the_oracle_track_lengths(oracle, fs):
    c = D.edge_case(fs, D.window(fs))
    for s, L in enumerate(D.edge_lengths(fs)):
        against_the_oracle(oracle, c.x[s, :L], fs, D.frames_per_call(L, c.calls))
        assert c.x[s, L - 1, s >> 1] >= 0.3 and c.x[s, L, s >> 1] >= 0.3                 # a spike either side of the end


# ---- the inputs exercise what they are for ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs", D.RATES)
def test_many_windows_reach_every_part_of_the_walk(fs):
    c = D.many_windows(fs)
    W = D.window(fs)
    assert W % 2 == (fs == 8000.0)
    ends = np.cumsum(c.calls)
    assert {0, 1, W - 1} <= set((ends % W).tolist()) and max(c.calls) >= 5 * W and 1 in c.calls     # on a window's end, either side of it
    for s in range(c.x.shape[0]):
        a, _ = D.checked(c.x[s], fs, c.calls)
        nfs = [r.num_fragments for r in a.readings]
        assert nfs[-1] >= 40 and max(r.m_cut[0] for r in a.readings) >= 8 and len(set(nfs)) >= 12
        assert (a.bins == D.SILENT).all(1).sum() == 3
        kept = a.bins[a.bins[:, 0] > 0]
        assert kept.max(0).min() - kept.min(0).max() > 64 * 40                           # spread over many 64-bin chunks
        for ch in range(2):
            rs = a.readings
            assert any(r.n_cut[ch] > r.m_cut[ch] for r in rs), "no bin's count overshoots m_cut"
            assert any(r.chunks[ch] > 1 for r in rs) and a.readings[-1].chunks[ch] > 3
            assert rs[-1].hist[ch].max() == 3 and (rs[-1].hist[ch] == 2).any()
            assert any(r.left[ch] > 0 for r in rs), "the walk never stops inside a chunk with occupied bins left in it"
            i3 = np.nonzero(rs[-1].hist[ch] == 3)[0][0]              # the loudest window's chunk holds a second bin
            assert ((D.HISTBINS - 1 - np.nonzero(rs[-1].hist[ch][i3 + 1:])[0] - i3 - 1) // 64).tolist()[-2:] == [(D.HISTBINS - 1 - a.bins[3, ch]) // 64] * 2


@pytest.mark.parametrize("fs", D.RATES)
def test_small_streams_sit_on_the_edges_they_name(fs):
    c = D.small(fs)
    runs = {n: D.checked(c.x[s], fs, c.calls)[0] for s, n in enumerate(c.names)}
    end = {n: r.readings[-1] for n, r in runs.items()}
    nw = D.SMALL_WINDOWS
    r = end["two_bins"]                                              # the walk runs off the bottom with n_cut < m_cut
    assert r.num_fragments == nw and r.m_cut == [3, 3] and r.n_cut == [2, 2] and (runs["two_bins"].bins == -1).sum() == 2 * (nw - 2)
    r = end["no_bin"]                                                # counted, never in a bin
    assert (runs["no_bin"].bins == -1).all() and r.block_count == 3 * nw and r.m_rms == [-81, -81] and r.dr == [21, 21] and r.dr_total == 21
    assert r.hist.sum() == 0
    r = end["last_chunk"]                                            # bins 1 .. 63 only, bin 63 (lane 0 of the last chunk) among them
    occ = np.nonzero(r.hist.sum(0))[0]
    assert occ.min() >= 1 and occ.max() == 63 and r.hist[1, 1] == 1 and min(r.n_cut) >= 3 and r.hist[0, 63] == 2 and r.hist[1, 62] >= 1
    b = runs["bin_0_and_1"].bins                                     # bin 0 is dropped, bin 1 kept
    assert b[3].tolist() == [0, 1] and b[6].tolist() == [1, 0] and end["bin_0_and_1"].hist.sum() == 2
    assert end["bin_0_and_1"].hist[0, 1] == 1 and end["bin_0_and_1"].hist[1, 1] == 1 and end["bin_0_and_1"].n_cut == [1, 1]
    assert abs(end["bin_0_and_1"].m_rms[0] - (-79.98)) < 1e-3
    d = D.levels(c.x[c.names.index("loud")], fs)[0]                  # above 0 dB: the clamp
    assert (d[[2, 7]] > D.HISTBINS + 100).all() and (runs["loud"].bins[[2, 7]] == D.HISTBINS - 1).all()
    assert D.HISTBINS - 64 < runs["loud"].bins[5].min() < D.HISTBINS - 1
    assert end["loud"].hist[0, -1] == 2 and end["loud"].peak_hist.min() > 1.0 and end["loud"].m_peak[0] > 0 and end["loud"].n_cut == [3, 3]
    assert end["dr_20"].dr == [20, 20] and end["dr_20"].dr_total == 20 and end["dr_20"].m_peak[0] == 0
    assert end["tie"].peak_hist[0].tolist() == [np.float32(0.7)] * 2 and abs(end["tie"].m_peak[0] - 20 * np.log10(0.7)) < 1e-4
    r = end["negative"]                                              # never positive: peak 0, m_peak -80, dr 21; the total from channel 0 alone
    assert r.peak_hist[1].tolist() == [0, 0] and r.m_peak[1] == -80 and r.dr[1] == 21 and r.m_rms[1] > -80 and r.dr_total == r.dr[0] < 20
    r, b = end["spike_in_silence"], runs["spike_in_silence"].bins
    assert (b[3] == D.SILENT).all() and (b != D.SILENT).any(1).sum() == nw - 1
    assert r.peak_hist[1, 1] == np.float32(0.004) and r.peak_hist[1, 0] > 0.008 and np.abs(c.x[c.names.index("spike_in_silence"), 4 * D.window(fs):5 * D.window(fs)]).max() < 0.0031


@pytest.mark.parametrize("fs", D.RATES)
def test_edge_spikes_carry_their_windows(fs):
    W, x = D.window(fs), D.edge(fs)
    for s in range(4):
        ch = s >> 1
        spikes = np.nonzero(x[s, :, ch] >= 0.3)[0]
        assert {0, W - 1, W, W + 1, 2 * W - 1, 2 * W, 5 * W - 1, 5 * W} <= set(spikes.tolist()) and np.abs(x[s, :, 1 - ch]).max() <= 1e-3
        for first in (W - 1, W, W + 1):
            ends = np.cumsum(D.edge_case(fs, first).calls)[:-1]
            assert set(ends.tolist()) | set((ends - 1).tolist()) <= set(spikes.tolist())    # the first and the last frame of every call
        d = D.levels(x[s], fs)[0][:, ch]
        for k in range(D.EDGE_WINDOWS):                              # any single spike dropped, doubled or moved: more than 20 bins
            mine = spikes[(spikes >= k * W) & (spikes < (k + 1) * W)]
            e = (x[s, k * W:(k + 1) * W, ch].astype(np.float64) ** 2).sum()
            assert len(mine) >= 1 and 1000.0 * np.log10(e / (e - (x[s, mine, ch].astype(np.float64) ** 2).min())) > 20
    for first in (W - 1, W, W + 1):
        calls = D.edge_case(fs, first).calls
        assert calls[0] == first and calls[1] == 1 and calls[2] == 2 and calls.count(1) >= 4 and calls.count(2) >= 4
