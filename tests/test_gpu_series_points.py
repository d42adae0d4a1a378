"""The per-stream point counts of the four reading series that end streams at their own lengths (STCORR, NEEDLE, KMETER: mtr_engine_series_points;
SPECTR30: mtr_engine_spectr_points) in ONE engine, across a closing mtr_engine_process_host_ends call, a state import and a reset — what the
call path counts on the host for every meter that keeps such a series, whichever meter it is.
Shapes: 3 streams, stereo, 48 kHz, every series with period 2400 (the smallest STCORR and KMETER take at 48 kHz, a multiple of four for
the needles) and capacity 8; one call of 6000 frames with frames = [6000, 5000, 0]."""
import numpy as np
import pytest

from test_gpu_parity import M  # noqa: F401  (M: the module fixture)

pytestmark = pytest.mark.gpu

S, FS, P, CAP, N = 3, 48000.0, 2400, 8, 6000
FRAMES = [6000, 5000, 0]


def counts(M, e):
    """the four counts, [4, S]: STCORR, NEEDLE, KMETER through series_points, SPECTR30 through spectr_points"""
    return np.stack([e.series_points(M.METER_STCORR), e.series_points(M.METER_NEEDLE), e.series_points(M.METER_KMETER), e.spectr_points()])


def test_series_points_of_all_four_meters_across_close_import_reset(M):
    rng = np.random.default_rng(2400)
    x = (rng.standard_normal((S, N, 2)) * 0.01).astype(np.float32)     # low-level noise
    # (a stream that stays open completes whole blocks only; one that closes inside a block adds the truncated one; 0 frames: nothing)
    want = [sum(M.series_cut(0, P, N, f)) for f in FRAMES]
    assert want == [2, 3, 0]
    with M.Engine(S, FS, M.METER_STCORR | M.METER_NEEDLE | M.METER_KMETER | M.METER_SPECTR30) as e:
        e.stcorr_set_period(P, CAP)
        e.needle_configure(M.NEEDLE_VU, P, CAP)
        e.kmeter_set_period(P, CAP)
        e.spectr_set_period(P, CAP)
        assert not counts(M, e).any()
        e.process_ends(x, np.array(FRAMES, np.uint64))
        assert counts(M, e).tolist() == [want] * 4
        frames, closed = e.stream_frames()
        assert frames.tolist() == FRAMES and closed.tolist() == [False, True, True]
        # mtr_engine_series_points knows three meters; the bank's count has its own getter
        with pytest.raises(M.EngineError) as err:
            e.series_points(M.METER_SPECTR30)
        assert err.value.code == M.engine.ERR_ARG
        # an imported stream is open again and stands where the open streams do: its series have their points
        blob = e.state_export(0, 1)
        e.state_import(blob, first=1)
        e.state_import(blob, first=2)
        assert counts(M, e).tolist() == [[want[0]] * S] * 4
        frames, closed = e.stream_frames()
        assert frames.tolist() == [N, 0, 0] and closed.tolist() == [False] * S
        e.reset()
        assert not counts(M, e).any()
        frames, closed = e.stream_frames()
        assert not frames.any() and not closed.any()
