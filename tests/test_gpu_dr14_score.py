"""DR-14's score (mtr_dr14.hip: k_dr14_sums, k_dr14_windows) over many windows, on window edges and at odd levels, against the numpy
restatement of src/dr14.c (tests/_dr14.py, pinned to mo_dr14_run by tests/test_dr14_cpu.py).

The older DR-14 tests never pass ten windows, so their cut is m_cut = max (1, nf / 5) = 1 and only the first occupied bin of the
histogram is ever read; a frame is 1 / 144001 of their windows and never carries one.  Here, at 8000 Hz (W = 24001, odd) and 8001 Hz
(W = 24004, even), mono and stereo, the stereo streams at an even and an odd stride (window and piece starts of both parities on the
16-byte path):
  * 46 windows per stream (m_cut up to 8), levels over 4400 bins, bins that hold 2 and 3 windows, silent windows; calls cut off the
    windows, on a window's last frame and one frame either side, calls of one frame and calls of many windows;
  * fragments that count but have no bin (-87 .. -80 dB), the walk running off the bottom, the last chunk's bins 63 .. 1, bin 0
    (dropped) against bin 1, RMS above 0 dB (the clamp to bin 7999), peaks above 0 dBFS, dr clamped at 20;
  * the second-highest window peak itself: equal maxima, a channel that is never positive, a spike kept through a silent window;
  * single spikes that carry their windows on the first and last frames of windows and of calls, calls of 1 and 2 frames across the
    boundaries, and the same streams through the _tracks entry with a spike on the last metered frame and one just past it.

The engine is read AFTER EVERY CALL (the reference scores at every window, the kernel at the end of a call that closed one) and held to
the restatement: block_count, the histogram (from the state blob: DR-14's sections are its last) and both window peaks exactly;
m_rms, m_peak, dr and dr_total within TOL_SCORE.  The score is discontinuous in the bins, so every case first asserts on the CPU
(_dr14.checked) that the f64 and the sequential-f32 sums put every window into the same bin and that none lies within 1e-3 bin of an edge.

Out of scope: non-finite samples.  With a NaN or Inf sum the reference converts a non-finite float to int (undefined); and its
MAX (peak_cur, v) returns a NaN sample, forgetting the window's earlier peak, where the kernel's fmaxf skips it."""
import numpy as np
import pytest

import _dr14 as D

pytestmark = pytest.mark.gpu
LAYOUTS = ["mono", "stereo_even", "stereo_odd"]                     # (channels, the parity of stream_stride_frames)
WORST = {"gpu": 0.0}


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def gpu_readings(M, case, fs, layout, lengths=None):
    """the case's calls over a device buffer [S, stride, C]; after every call (dr14 () results, hist [S, C, 8000], peak_hist [S, 2, 2]).
    What lies behind the streams' frames is NaN: never read.  lengths: through process_device_tracks with each stream's own length."""
    import torch
    x = case.x
    S, T, chn = x.shape
    assert chn == (1 if layout == "mono" else 2)
    stride = T + 2 + ((T + (layout == "stereo_odd")) & 1)
    assert stride % 2 == (layout == "stereo_odd")
    buf = np.full((S, stride, chn), np.nan, np.float32)
    buf[:, :T] = x
    dev = torch.from_numpy(buf).cuda()
    nh = S * chn * D.HISTBINS * 4
    out, pos = [], 0
    with M.Engine(S, fs, M.METER_DR14, n_channels=chn) as e:
        for i, n in enumerate(case.calls):
            ptr = dev.data_ptr() + pos * chn * 4
            if lengths is None:
                e.process_device(ptr, n, stride=stride)
            else:
                e.process_device_tracks(ptr, n, np.array([D.frames_per_call(L, case.calls)[i] for L in lengths], np.uint64), stride=stride)
            pos += n
            res = e.dr14()
            blob = np.frombuffer(e.state_export(0, S), np.uint8)
            hist = blob[-nh:].copy().view(np.uint32).reshape(S, chn, D.HISTBINS)
            state = blob[-nh - S * 52:-nh].copy().view(np.float32).reshape(S, 13)        # mtr_dr14_state: peak_hist is floats 4 .. 7
            out.append(([(list(r.m_rms), list(r.m_peak), list(r.dr), r.dr_total, r.block_count) for r in res], hist,
                        state[:, 4:8].reshape(S, 2, 2)[:, :chn]))
    return out


def hold(got, s, want, what):
    """stream s of the readings after every call against the restatement's"""
    chn = len(want.readings[0].m_rms)
    assert len(got) == len(want.readings)
    for i, ((res, hist, ph), r) in enumerate(zip(got, want.readings)):
        m_rms, m_peak, dr, dr_total, blocks = res[s]
        assert blocks == r.block_count, (what, s, i, blocks, r.block_count)
        assert np.array_equal(hist[s], r.hist), (what, s, i, "histogram", np.argwhere(hist[s] != r.hist).tolist(), np.nonzero(r.hist))
        assert np.array_equal(ph[s], r.peak_hist), (what, s, i, "window peaks", ph[s], r.peak_hist)
        dev = [abs(m_rms[c] - r.m_rms[c]) for c in range(chn)] + [abs(m_peak[c] - r.m_peak[c]) for c in range(chn)] \
            + [abs(dr[c] - r.dr[c]) for c in range(chn)] + [abs(dr_total - r.dr_total)]
        WORST["gpu"] = max(WORST["gpu"], float(max(dev)))
        assert max(dev) <= D.TOL_SCORE, (what, s, i, dev, res[s], r[:5])


def shaped(case, layout, edge=False):
    return case if layout != "mono" else (D.edge_mono(case) if edge else D.mono(case))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fs", D.RATES)
def test_many_windows(M, fs, layout):
    case = shaped(D.many_windows(fs), layout)
    want = [D.checked(case.x[s], fs, case.calls)[0] for s in range(case.x.shape[0])]
    for w in want:
        assert w.readings[-1].num_fragments >= 40 and max(w.readings[-1].m_cut) >= 8
        assert any(r.n_cut[0] > r.m_cut[0] for r in w.readings) and any(r.left[0] for r in w.readings) and w.readings[-1].chunks[0] > 3
    got = gpu_readings(M, case, fs, layout)
    for s, w in enumerate(want):
        hold(got, s, w, case.names[s])
    print("worst deviation from the restatement so far: %.3g dB" % WORST["gpu"])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fs", D.RATES)
def test_level_edges_loud_windows_and_peaks(M, fs, layout):
    case = shaped(D.small(fs), layout)
    want = [D.checked(case.x[s], fs, case.calls)[0] for s in range(case.x.shape[0])]
    got = gpu_readings(M, case, fs, layout)
    for s, w in enumerate(want):
        hold(got, s, w, case.names[s])
    # what the streams are for, said directly (behind the last call; the mono streams are channel 1 of the stereo ones)
    end = {n: dict(zip(("m_rms", "m_peak", "dr", "dr_total", "block_count"), got[-1][0][s])) for s, n in enumerate(case.names)}
    c, stereo = (0, False) if layout == "mono" else (1, True)
    r = end["no_bin"]
    assert r["block_count"] == 3 * D.SMALL_WINDOWS and r["m_rms"][c] == -81 and r["dr"][c] == 21 and (not stereo or r["dr_total"] == 21)
    assert end["two_bins"]["block_count"] == 3 * D.SMALL_WINDOWS and end["two_bins"]["m_rms"][c] > -35
    assert -80 < end["last_chunk"]["m_rms"][c] < -79.3
    assert abs(end["bin_0_and_1"]["m_rms"][c] - (-79.98)) <= 1e-3                        # bin 1 alone: (1 - 7999) / 100
    r = end["loud"]
    assert -0.1 < r["m_rms"][c] <= 0 and r["m_peak"][c] > 0 and r["dr"][c] == 1          # two windows in bin 7999; min (0, peak dB)
    assert end["dr_20"]["dr"][c] == 20 and (not stereo or end["dr_20"]["dr_total"] == 20)
    assert abs(end["tie"]["m_peak"][c] - 20 * np.log10(0.6)) <= D.TOL_SCORE
    assert not stereo or abs(end["tie"]["m_peak"][0] - 20 * np.log10(0.7)) <= D.TOL_SCORE
    r = end["negative"]
    assert r["m_peak"][c] == -80 and r["dr"][c] == 21 and (not stereo or r["dr_total"] == r["dr"][0] < 20)
    assert abs(end["spike_in_silence"]["m_peak"][c] - 20 * np.log10(0.004)) <= D.TOL_SCORE
    print("worst deviation from the restatement so far: %.3g dB" % WORST["gpu"])


@pytest.mark.parametrize("first", [-1, 0, 1])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fs", D.RATES)
def test_spikes_on_edge_frames(M, fs, layout, first):
    case = shaped(D.edge_case(fs, D.window(fs) + first), layout, edge=True)
    want = [D.checked(case.x[s], fs, case.calls)[0] for s in range(4)]
    got = gpu_readings(M, case, fs, layout)
    for s, w in enumerate(want):
        hold(got, s, w, case.names[s])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fs", D.RATES)
def test_spikes_either_side_of_a_track_end(M, fs, layout):
    case = shaped(D.edge_case(fs, D.window(fs)), layout, edge=True)
    Ls = D.edge_lengths(fs)
    want = [D.checked(case.x[s, :L], fs, D.frames_per_call(L, case.calls))[0] for s, L in enumerate(Ls)]
    got = gpu_readings(M, case, fs, layout, lengths=Ls)
    for s, w in enumerate(want):
        hold(got, s, w, (case.names[s], Ls[s]))
    print("worst deviation from the restatement so far: %.3g dB" % WORST["gpu"])
