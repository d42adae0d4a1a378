"""mtr_engine_state_export / mtr_engine_state_import (include/mtr_engine.h; SURVEY.md 5 "checkpoint / resume"; VERDICT r4
item 5): everything a stream carries from call to call travels as one opaque blob — out of an engine, into another engine
of the same configuration with a DIFFERENT number of streams and a DIFFERENT slot, in this process or (below) in another —
and processing continues BIT FOR BIT as if it had never stopped: every result of every meter, for both fused kernels.

The reference has nothing like it (it persists one UI word, src/ebulv2.cc:514-553): this is what lets a multi-hour batch be
checkpointed and the streams of a job be re-sharded between its ranks."""
import hashlib
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import _signals as sig
from test_gpu_hostpath import _records

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _start(M, e, meters):
    if meters & M.METER_EBU:
        e.integr_start()


def _straight(M, x, calls, meters, fs, C, **kw):
    """ONE engine over all the streams and all the calls: the record after every call."""
    import torch
    dev = torch.from_numpy(x).cuda()
    st = torch.cuda.current_stream().cuda_stream
    recs = []
    with M.Engine(x.shape[0], fs, meters, n_channels=C, **kw) as e:
        _start(M, e, meters)
        pos = 0
        for n in calls:
            e.process_device(dev.data_ptr() + pos * C * 4, n, x.shape[1], st)
            recs.append(_records(M, e, meters))
            pos += n
        seg = e.seg_stats()[0]
    return recs, seg


def _rows(rec, sel):
    """The streams `sel` of a record (every array is [stream, ...]; fragment powers belong to the last call only)."""
    return {k: v[sel] for k, v in rec.items()}


def _checkpointed(M, x, calls, k_stop, meters, fs, C, **kw):
    """The same job, stopped after call k_stop: its streams leave in two blobs (the batch cut at an odd place), the engine
    is DESTROYED, and two new engines of other sizes take them into other slots and process the rest."""
    import torch
    S = x.shape[0]
    cut = S // 3 + 1
    dev = torch.from_numpy(x).cuda()
    st = torch.cuda.current_stream().cuda_stream
    with M.Engine(S, fs, meters, n_channels=C, **kw) as e:
        _start(M, e, meters)
        pos = 0
        for n in calls[:k_stop]:
            e.process_device(dev.data_ptr() + pos * C * 4, n, x.shape[1], st)
            before = _records(M, e, meters)                                # (read after every call, as the straight run is: Kmeterdsp::read arms a flag)
            pos += n
        assert e.state_bytes(cut) == len(e.state_export(0, cut))
        blob_a, blob_b = e.state_export(0, cut), e.state_export(cut, S - cut)
    # engine A': more streams than the blob, the blob's streams in slots [2, 2 + cut); engine B': exactly the rest, slot 0
    pad = 3
    xa = np.concatenate([np.zeros((2,) + x.shape[1:], np.float32), x[:cut], np.zeros((pad - 2,) + x.shape[1:], np.float32)])
    da, db = torch.from_numpy(xa).cuda(), torch.from_numpy(np.ascontiguousarray(x[cut:])).cuda()
    out = []
    with M.Engine(cut + pad, fs, meters, n_channels=C, **kw) as ea, M.Engine(S - cut, fs, meters, n_channels=C, **kw) as eb:
        assert ea.state_import(blob_a, first=2) == cut and eb.state_import(blob_b) == S - cut
        # what came out is what went in, before anything is processed
        ra, rb = _records(M, ea, meters), _records(M, eb, meters)
        for k, v in before.items():
            if k == "frag":
                continue                                                   # (the last call's fragment powers are a diagnostic of that call)
            assert np.array_equal(np.concatenate([ra[k][2:2 + cut], rb[k]]), v, equal_nan=True), k
        p = pos
        for n in calls[k_stop:]:
            ea.process_device(da.data_ptr() + p * C * 4, n, x.shape[1], st)
            eb.process_device(db.data_ptr() + p * C * 4, n, x.shape[1], st)
            ra, rb = _records(M, ea, meters), _records(M, eb, meters)
            out.append({k: np.concatenate([ra[k][2:2 + cut], rb[k]]) for k in ra})
            p += n
        seg = ea.seg_stats()[0]
    return out, seg


CASES = [
    # (meters, channels, fs, engine options, signal, uneven calls (the checkpoint falls INSIDE a 50 ms fragment, a DR-14 window, a bank toggle))
    ("ebu+tp: k_kwtp16", "EBU|TRUEPEAK", 2, 48000.0, {"tune_layout": 6, "tune_segments": 1}, "g2", [2400 * 9 + 1000, 2400 * 6 + 333, 1500, 2400 * 12 + 67]),
    ("ebu+tp: k_seg", "EBU|TRUEPEAK", 2, 48000.0, {"tune_segments": 3}, "g2", [2400 * 9 + 1000, 2400 * 6 + 333, 1500, 2400 * 12 + 67]),
    ("ebu+tp: k_seg at 44.1 kHz", "EBU|TRUEPEAK", 2, 44100.0, {"tune_segments": 2}, "g2", [2205 * 8, 2205 * 7 + 5, 2205 * 9 + 2200]),
    ("ebu: k_kw", "EBU", 2, 48000.0, {}, "g2", [2400 * 9 + 1000, 2400 * 6 + 333, 1500, 2400 * 12 + 67]),
    ("bank + ballistics + DR-14 + K-meter", "SPECTR30|TPBALLIST|DR14|KMETER", 2, 48000.0, {}, "g2", [30011, 7, 48000 * 3 + 5, 20000]),
    ("mono ballistics + bank", "SPECTR30|TPBALLIST", 1, 48000.0, {}, "mono", [30011, 7, 40000]),
    ("integer meters", "BITSTATS|SIGDIST", 1, 48000.0, {}, "g5", [20000, 1, 29999]),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_export_destroy_import_continue_is_one_run_bit_for_bit(M, case):
    _, names, C, fs, kw, kind, calls = case
    meters = 0
    for n in names.split("|"):
        meters |= getattr(M, "METER_" + n)
    T, S = sum(calls), 13
    if kind == "g2":
        x = np.stack([sig.g2(T, 500 + s, fs) * np.float32(2.0 ** -(s % 3)) for s in range(S)])
    elif kind == "mono":
        x = np.stack([sig.g2(T, 600 + s, fs)[:, 0] * np.float32(2.0 ** -(s % 3)) for s in range(S)])
    else:
        x = np.stack([sig.g5(T, 4300 + s) for s in range(S)])
        x[4, 100] = 1.5                                                    # the SDH's skipped-sample regime, before the checkpoint
    x = np.ascontiguousarray(x, np.float32)
    want, seg_w = _straight(M, x, calls, meters, fs, C, **kw)
    for k_stop in (1, 2):
        got, seg_g = _checkpointed(M, x, calls, k_stop, meters, fs, C, **kw)
        for a, b in zip(want[k_stop:], got):
            _same(a, b)
    if kw.get("tune_segments") and not kw.get("tune_layout"):
        assert seg_w >= 2 and seg_g >= 1                                   # both sides of the checkpoint went through k_seg
    else:
        assert seg_w == 0 and seg_g == 0


def test_import_refuses_what_does_not_fit(M):
    import torch
    fs, T = 48000.0, 5000
    x = np.stack([sig.g2(T, 50 + s) for s in range(4)])
    dev = torch.from_numpy(x).cuda()
    st = torch.cuda.current_stream().cuda_stream
    with M.Engine(4, fs, M.METER_EBU | M.METER_TRUEPEAK) as e:
        e.process_device(dev.data_ptr(), 1000, T, st)
        blob = e.state_export(1, 2)
        assert len(blob) == e.state_bytes(2)
        with pytest.raises(M.EngineError):
            e.state_export(3, 2)                                           # stream range
        # another configuration: meters, rate
        for other in (dict(meters=M.METER_EBU), dict(sample_rate=44100.0)):
            with M.Engine(4, other.get("sample_rate", fs), other.get("meters", M.METER_EBU | M.METER_TRUEPEAK)) as o:
                with pytest.raises(M.EngineError) as ei:
                    o.state_import(blob)
                assert ei.value.code == M.engine.ERR_STATE
        # not a blob, a truncated blob, a blob that does not fit the slots
        with M.Engine(2, fs, M.METER_EBU | M.METER_TRUEPEAK) as o:
            for bad in (b"", b"x" * 100, blob[:-1], bytes(len(blob))):
                with pytest.raises(M.EngineError) as ei:
                    o.state_import(bad)
                assert ei.value.code == M.engine.ERR_STATE
            with pytest.raises(M.EngineError):
                o.state_import(blob, first=1)                              # two streams into slots [1, 3) of two
            assert o.state_import(blob) == 2                               # a fresh engine takes the blob's cursors (1000 frames into a fragment)
            o.process_device(dev.data_ptr() + 1000 * 8, 500, T, st)
            with pytest.raises(M.EngineError) as ei:
                o.state_import(blob)                                       # ... and now stands somewhere else
            assert ei.value.code == M.engine.ERR_STATE
        # the same engine, at the same cursors: allowed (streams swap slots inside a job)
        was = [(r.truepeak[0], r.truepeak[1], r.loudness_M) for r in e.results()]
        e.state_import(blob, first=0)
        now = [(r.truepeak[0], r.truepeak[1], r.loudness_M) for r in e.results()]
        assert now == [was[1], was[2], was[2], was[3]] and len(set(was)) == 4


def test_import_checks_the_blob_before_it_trusts_it(M):
    """a checkpoint that rotted — a flipped bit in the payload, a fragment cursor of 0 or beyond the fragment, an
    open DR-14 window longer than a window — is refused with MTR_ERR_STATE and leaves the engine untouched (still fresh: the
    good blob goes in afterwards and processing continues bit for bit); and the documented asymmetry: a fresh engine on which
    integr_start () was called takes the BLOB's integration flag."""
    import struct
    import torch
    fs, T = 48000.0, 9000
    meters = M.METER_EBU | M.METER_TRUEPEAK
    x = np.stack([sig.g2(T, 80 + s) for s in range(3)])
    dev = torch.from_numpy(x).cuda()
    st = torch.cuda.current_stream().cuda_stream
    with M.Engine(3, fs, meters) as e:
        e.process_device(dev.data_ptr(), 3000, T, st)                      # integration OFF (never started)
        blob = e.state_export()
        e.process_device(dev.data_ptr() + 3000 * 8, 6000, T, st)
        want = _records(M, e, meters)
    # header: magic, version, header_bytes, meters, n_channels, rate, count, per_stream, stream_state_bytes, frcnt, integr, omega, dr_scnt, fnv
    hdr = struct.Struct("<IIIIIfIIIIIfQQ")
    f = list(hdr.unpack_from(blob))
    assert f[1] == 2 and f[9] == 2400 - 3000 % 2400 and f[10] == 0

    def with_field(i, v):
        g = list(f); g[i] = v
        return hdr.pack(*g) + blob[hdr.size:]
    rotten = [bytearray(blob) for _ in range(2)]
    rotten[0][hdr.size + 5] ^= 0x10                                        # one bit of stream 0's K-filter state
    rotten[1][-1] ^= 0x01                                                  # the last byte of the payload
    bad = [bytes(r) for r in rotten] + [with_field(9, 0), with_field(9, 2401), with_field(9, 1 << 31), with_field(10, 7),
                                        with_field(11, 2.0), with_field(12, 1 << 40)]
    with M.Engine(3, fs, meters) as o:
        o.integr_start()                                                   # overridden by the import below: the blob says off
        for b in bad:
            with pytest.raises(M.EngineError) as ei:
                o.state_import(b)
            assert ei.value.code == M.engine.ERR_STATE
        assert o.state_import(blob) == 3                                   # still a fresh engine: nothing above moved it
        o.process_device(dev.data_ptr() + 3000 * 8, 6000, T, st)
        got = _records(M, o, meters)
    for k in want:
        assert np.array_equal(want[k], got[k], equal_nan=True), k
    assert want["counts"].sum() == 0                                       # integration stayed off, as in the blob


# the blob's header: magic, version, header_bytes, meters, n_channels, rate, count, per_stream, stream_state_bytes, frcnt, integr, omega,
# dr_scnt, and the FNV-1a (64 bit) of the payload behind it
HDR = struct.Struct("<IIIIIfIIIIIfQQ")


def _fnv1a64(b):
    h = 0xcbf29ce484222325
    for v in b:
        h = ((h ^ v) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def _feed(e, x, calls, pos=0):
    for n in calls:
        e.process(np.ascontiguousarray(x[:, pos:pos + n]))
        pos += n


# The engine of the test below: three meters whose sections carry a host-owned header (STCORR at the end of its entry, NEEDLE in front
# of a variable-pitch one, SCOPE as the whole entry of the first of nine sections) behind one that has none
MIX_CALLS, MIX_STOP, MIX_KINDS = [5000, 7001, 9000, 4803], 2, ("NEEDLE_VU", "NEEDLE_IEC2")


def _mix_engine(M, S=5):
    e = M.Engine(S, 48000.0, M.METER_KMETER | M.METER_STCORR | M.METER_NEEDLE | M.METER_SCOPE)
    e.stcorr_set_period(2400, 64)
    e.needle_configure(M.NEEDLE_VU | M.NEEDLE_IEC2, 18, 4000)
    e.scope_configure(256, 64)
    return e


def _mix_signal():
    return np.stack([sig.g2(sum(MIX_CALLS), 900 + s) * np.float32(2.0 ** -(s % 3)) for s in range(5)])


def _mix_record(M, e, first, count):
    rec = {}
    rec["sc_pts"], rec["sc_n"], _ = e.stcorr_series(first, count)
    rec["sc_corr"], rec["sc_state"] = e.stcorr_read(first, count)
    for k in MIX_KINDS:
        rec[k + "_pts"], rec[k + "_n"], _ = e.needle_series(getattr(M, k), first, count)
        rec[k + "_level"], rec[k + "_state"] = e.needle_read(getattr(M, k), first, count)
    rec.update({"sp_" + k: v for k, v in e.scope_read(first, count).items()})
    rec["sp_analyses"] = e.scope_analyses()
    rec["km_rms"], rec["km_peak"] = e.kmeter_read(first, count)
    return rec


def test_several_header_carrying_meters_in_one_blob(M):
    """KMETER | STCORR | NEEDLE | SCOPE in one engine: the blob's sections of the three meters that keep configuration and cursors in
    their entries follow one another, so each must be found where it is.  Stopped inside a period of both series and inside a hop,
    streams [2, 5) travel into slots [1, 4) of a fresh engine configured alike and go on bit for bit; a NEEDLE header that differs in
    ONE stream is refused, by the checksum and — the checksum made to fit — by the comparison of the streams' headers."""
    x = _mix_signal()
    done = sum(MIX_CALLS[:MIX_STOP])
    assert done % 2400 and done % 18 and done % 64                       # inside a period of each series, inside a hop
    with _mix_engine(M) as e:
        _feed(e, x, MIX_CALLS)
        want = _mix_record(M, e, 2, 3)
    with _mix_engine(M) as e:
        _feed(e, x, MIX_CALLS[:MIX_STOP])
        blob = e.state_export(2, 3)
        assert e.state_bytes(3) == len(blob)
    rest = np.zeros((5, x.shape[1] - done, 2), np.float32)
    rest[1:4] = x[2:5, done:]
    with _mix_engine(M) as e:
        assert e.state_import(blob, first=1) == 3
        assert e.state_export(1, 3) == blob                                # out again as it came in, before anything is processed
        _feed(e, rest, MIX_CALLS[MIX_STOP:])
        got = _mix_record(M, e, 1, 3)
    assert want.keys() == got.keys()
    for k, w in want.items():
        if k.endswith("_n"):                                               # the points restart with the engine's
            P = 2400 if k == "sc_n" else 18
            assert got[k] == w - done // P, k
        elif k.endswith("_pts"):
            P = 2400 if k == "sc_pts" else 18
            assert np.array_equal(got[k].view(np.uint32), w[:, done // P:].view(np.uint32)), k
        else:
            assert np.array_equal(np.asarray(got[k]).view(np.uint32), np.asarray(w).view(np.uint32)) if isinstance(w, np.ndarray) else got[k] == w, k
    # NEEDLE's section stands behind the core's three arrays, KMETER's and STCORR's: what a KMETER | STCORR engine carries per stream
    with M.Engine(1, 48000.0, M.METER_KMETER | M.METER_STCORR) as o:
        before = o.state_bytes(1) - o.state_bytes(0)
    pitch = 32 + 2 * 2 * 32                                                # mtr_needle_hdr + [kinds][channels] detectors
    at = HDR.size + 3 * before + 1 * pitch                                 # stream 1's header: kinds, period, fill, pad
    assert struct.unpack_from("<III", blob, at) == (M.NEEDLE_VU | M.NEEDLE_IEC2, 18, done % 18)
    bad = bytearray(blob)
    bad[at + 4] ^= 0x01                                                    # period 18 -> 19, in this stream's entry only
    with _mix_engine(M) as e:
        assert M.lib.mtr_engine_state_import(e._h, 1, bytes(bad), len(bad)) == M.engine.ERR_STATE
        assert b"checksum" in M.lib.mtr_last_error()
        f = list(HDR.unpack_from(bad))
        f[-1] = _fnv1a64(bad[HDR.size:])
        assert f[-1] != HDR.unpack_from(blob)[-1]
        fit = HDR.pack(*f) + bytes(bad[HDR.size:])
        assert M.lib.mtr_engine_state_import(e._h, 1, fit, len(fit)) == M.engine.ERR_STATE
        assert b"needle" in M.lib.mtr_last_error()
        assert e.state_import(blob, first=1) == 3                          # still a fresh engine: the good blob goes in


def _blob_cases(M):
    """name -> the state blob of a small engine after fixed input (tests/golden/golden_state_blobs_v1.json holds their SHA-256)."""
    out = {}
    with _mix_engine(M) as e:
        _feed(e, _mix_signal(), MIX_CALLS[:MIX_STOP])
        out["kmeter+stcorr+needle+scope"] = e.state_export(2, 3)
    x = np.stack([sig.g2(12001, 300 + s) * np.float32(2.0 ** -(s % 3)) for s in range(3)])
    x5 = np.ascontiguousarray(np.concatenate([x, np.roll(x, 1, 0), np.roll(x, 2, 0)[:, :, :1]], 2))
    with M.Engine(3, 48000.0, M.METER_SURROUND, n_channels=5) as e:
        e.surround_set_period(2400, 16)
        _feed(e, x5, [5000, 7001])
        out["surround, 5 channels"] = e.state_export()
    with M.Engine(3, 48000.0, M.METER_EBU | M.METER_TRUEPEAK | M.METER_STCORR) as e:
        e.integr_start()
        e.stcorr_set_period(2400, 8)
        _feed(e, x, [5000, 7001])
        out["ebu+truepeak+stcorr"] = e.state_export()
    with M.Engine(3, 48000.0, M.METER_SPECTR30 | M.METER_TPBALLIST | M.METER_DR14 | M.METER_KMETER) as e:
        _feed(e, x, [5000, 7001])
        out["spectr30+tpballist+dr14+kmeter"] = e.state_export()
    return out


def test_blobs_are_byte_for_byte_the_recorded_ones(M):
    """The blob format is a contract with every checkpoint on disk: four small configurations, after fixed input, give the bytes whose
    SHA-256 and length were recorded when the host side of the side meters moved behind one table."""
    with open(os.path.join(ROOT, "tests", "golden", "golden_state_blobs_v1.json")) as f:
        want = json.load(f)
    got = {k: {"bytes": len(b), "sha256": hashlib.sha256(b).hexdigest()} for k, b in _blob_cases(M).items()}
    assert got == want


WORKER = r'''
import os, sys
import numpy as np, torch, torch.distributed as dist
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import meters.lv2_amd as M
from meters.lv2_amd import dist as mdist
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
import datetime
dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=120))
torch.cuda.set_device(0)
S, T, fs = 24, 48000 * 2, 48000.0                      # streams per rank; every rank holds the WHOLE job's audio, meters its own shard
st = torch.cuda.current_stream().cuda_stream
full = torch.empty((2 * S, 3 * T, 2), dtype=torch.float32, device="cuda")
M.synth_fill_device(full.data_ptr(), 2 * S, 3 * T, 3 * T, 777, fs, 1, st)
first, count = mdist.shard(2 * S, world, rank)
half = S // 2
own = list(range(first, first + count))               # job-wide stream ids in this engine's slots
def process(e, ids, pos, n):
    # the engine's slots hold arbitrary job streams after the swap: gather them into a contiguous batch for the call
    batch = full[ids, pos:pos + n].contiguous()
    e.process_device(batch.data_ptr(), n, n, st)
    torch.cuda.synchronize()
with M.Engine(S, fs, M.METER_EBU | M.METER_TRUEPEAK, **%(kw)r) as e:
    e.integr_start()
    process(e, own, 0, T + 1000)                      # the job stops INSIDE a fragment
    # mid-job: every rank gives the second half of its streams to the other rank and takes the other's
    mine = e.state_export(half, S - half)
    blobs = [None, None]
    dist.all_gather_object(blobs, mine)
    e.state_import(blobs[1 - rank], first=half)
    own = own[:half] + list(range((1 - rank) * S + half, (1 - rank) * S + S))
    process(e, own, T + 1000, 2 * T - 1000)
    hist = torch.zeros(2 * 751, dtype=torch.int32, device="cuda")
    mx = torch.zeros(4, dtype=torch.float32, device="cuda")
    e.aggregate_device(hist.data_ptr(), mx.data_ptr(), st)
    torch.cuda.synchronize()
    per = {own[i]: (r.integrated, r.truepeak[0], r.truepeak[1], r.hist_M_count, r.loudness_S) for i, r in enumerate(e.results())}
hist, mx = hist.cpu(), mx.cpu()
mdist.all_reduce_aggregate(hist, mx)
allper = [None, None]
dist.all_gather_object(allper, per)
if rank == 0:
    import json
    merged = {}
    for d in allper:
        merged.update(d)
    print("STATE_SWAP " + json.dumps({"programme": mdist.programme_summary(hist, mx), "per": [merged[i] for i in range(2 * S)]}), flush=True)
dist.barrier()
dist.destroy_process_group()
'''


@pytest.mark.parametrize("segments", [0, 2], ids=["k_kwtp16", "k_seg"])
def test_two_ranks_swap_half_their_streams_mid_job(M, tmp_path, segments):
    """Two gloo ranks (sharing this box's one GPU) meter a job of 48 streams, 24 each; in mid-job — inside a 50 ms fragment —
    each hands the second half of its streams to the other as a state blob over the control plane and goes on with what it
    received.  The job's programme record (summed histograms -> mtr_hist_loudness, max of peaks) and every stream's own
    results equal ONE engine over all 48 streams fed the same two calls, bit for bit."""
    import torch
    from meters.lv2_amd import dist as mdist
    script = tmp_path / "swap_worker.py"
    # (the segmentation is pinned: left to itself the engine picks it from the batch size, and 24 and 48 streams need not agree)
    kw = {"tune_segments": 2} if segments else {"tune_layout": 6, "tune_segments": 2}
    script.write_text(WORKER % dict(root=ROOT, kw=kw))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(29700 + os.getpid() % 200), str(script)], env=env, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("STATE_SWAP ")]
    assert out.returncode == 0 and len(lines) == 1, (out.stdout[-2000:], out.stderr[-4000:])
    got = json.loads(lines[0][len("STATE_SWAP "):])
    S, T, fs = 48, 48000 * 2, 48000.0
    st = torch.cuda.current_stream().cuda_stream
    full = torch.empty((S, 3 * T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(full.data_ptr(), S, 3 * T, 3 * T, 777, fs, 1, st)
    hist = torch.zeros(2 * 751, dtype=torch.int32, device="cuda")
    mx = torch.zeros(4, dtype=torch.float32, device="cuda")
    with M.Engine(S, fs, M.METER_EBU | M.METER_TRUEPEAK, **kw) as e:
        e.integr_start()
        for pos, n in ((0, T + 1000), (T + 1000, 2 * T - 1000)):
            batch = full[:, pos:pos + n].contiguous()
            e.process_device(batch.data_ptr(), n, n, st)
            torch.cuda.synchronize()
        e.aggregate_device(hist.data_ptr(), mx.data_ptr(), st)
        torch.cuda.synchronize()
        per = [[r.integrated, r.truepeak[0], r.truepeak[1], r.hist_M_count, r.loudness_S] for r in e.results()]
    want = mdist.programme_summary(hist, mx)
    for k, v in want.items():
        g = got["programme"][k]
        assert (list(g) == list(v)) if isinstance(v, tuple) else (g == v), (k, g, v)
    assert got["per"] == per
