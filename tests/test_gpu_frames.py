"""Frame layouts on the GPU: mtr_engine_set_frame_layout (include/mtr_engine.h), k_pick (mtr_source.hip) in front of the meters.

The rule of tests/test_gpu_pcm.py, no tolerance anywhere: a call with a layout on the WIDE buffer against the same entry point with
the default layout on pick_decode of that buffer (for PCM: on the compacted integers), same set_host_chunk_bytes — every record of
every meter np.array_equal, seg_stats () equal, state blobs byte-equal after the last call.  (tests/test_frames_cpu.py pins
mtr_pick_decode_host to numpy bit for bit.)  The unnamed channels of every frame, the frames behind a stream's length and the row
padding of the device buffers hold NaN, Inf and 1e30 (integer PCM: the extreme codes).  Two cases go against the reference instead:
the mono cases of golden_mc_v1 (a stereo engine reading the one channel twice) and WAVE 5.1 against the multichannel oracle.
Every non-default layout is staged through k_pick, but WAVE 5.1 in device f32 on a 5-channel engine: k_kwmc51 reads those frames itself.
"""
import os

import numpy as np
import pytest

import _mc
import _signals as sig

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "golden_mc_v1.npz"))

# tests/test_gpu_multichannel.py's tolerances and helpers (the tolerances of tests/test_gpu_parity.py)
DB_TOL = 1e-3
TP_REL = 2e-6
MOVED_MAX, MOVED_RATE = 2, 5e-4


def moved_points(got, want):
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    assert got.sum() == want.sum(), (got.sum(), want.sum())
    d = got - want
    far = 0
    for row in d.reshape(-1, d.shape[-1]):
        c = 0
        for x in np.cumsum(row):
            c = c + 1 if x != 0 else 0
            far = max(far, c)
    return int(np.abs(d).sum() // 2), far


def check_hist(got, want):
    moved, far = moved_points(got, want)
    assert far <= 1 and moved <= max(MOVED_MAX, int(np.ceil(MOVED_RATE * int(np.asarray(want).sum())))), (moved, far)
    return moved


def check9(got9, want9):
    assert np.allclose(got9[:6], want9[:6], atol=DB_TOL), (got9, want9)


FORMATS = ["f32", "s16", "s24", "s32"]
BITS = {"s16": 16, "s24": 24, "s32": 32, "f32": 32}
JUNK = np.array([np.nan, np.inf, 1e30, -np.inf], np.float32)
WAVE51 = (0, 1, 2, 4, 5)


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def _fmt(M, name):
    return {"f32": 0, "s16": M.PCM_S16, "s24": M.PCM_S24, "s32": M.PCM_S32}[name]


def _mask(M, names):
    m = 0
    for n in names.split("|"):
        m |= getattr(M, "METER_" + n)
    return m


def _quant(x, name):
    k = BITS[name] - 1
    v = np.rint(np.asarray(x, np.float64).clip(-2.0, 2.0) * 2.0 ** k).clip(-2.0 ** k, 2.0 ** k - 1).astype(np.int64)
    return v.astype(np.int16 if name == "s16" else np.int32)


def _raw(q, name):
    """what the entry points take: [S, T, W] float32 / int16 / int32 as they are, s24 packed little endian as uint8 [S, T * W * 3]"""
    if name != "s24":
        return np.ascontiguousarray(q)
    b = np.ascontiguousarray(q.astype("<i4")).view(np.uint8).reshape(q.shape[0], -1, 4)[:, :, :3]
    return np.ascontiguousarray(b).reshape(q.shape[0], -1)


def _records(M, e, meters):
    """every record of every meter (the list of tests/test_gpu_pcm.py:_records)"""
    out = {}
    if meters & (M.METER_EBU | M.METER_TRUEPEAK | M.METER_TPBALLIST):
        r = e.results()
        out["o9"] = e.out9()
        out["counts"] = np.array([[x.hist_M_count, x.hist_S_count] for x in r])
        out["tp"] = np.array([[x.truepeak[0], x.truepeak[1], x.truepeak_call[0], x.truepeak_call[1]] for x in r], np.float32)
        out["tpb"] = np.array([[x.tpb_level[0], x.tpb_level[1], x.tpb_peak[0], x.tpb_peak[1]] for x in r], np.float32)
    if meters & M.METER_TRUEPEAK:
        out["tpc_hold"], out["tpc_last"] = e.truepeak_channels()
    if meters & M.METER_EBU:
        out["hm"], out["hs"] = e.histograms()
        out["frag"] = e.fragment_powers()
    if meters & M.METER_SPECTR30:
        sp = e.spectrum()
        out["val"], out["max"] = sp["val"], sp["max"]
    if meters & M.METER_BITSTATS:
        out.update({"b_" + k: v for k, v in e.bitstats().items()})
    if meters & M.METER_SIGDIST:
        out.update({"d_" + k: v for k, v in e.sigdist().items()})
    if meters & M.METER_DR14:
        out["dr"] = np.array([[x.m_rms[0], x.m_rms[1], x.m_peak[0], x.m_peak[1], x.dr[0], x.dr[1], x.dr_total, x.block_count] for x in e.dr14()])
    if meters & M.METER_KMETER:
        out["km_rms"], out["km_peak"] = e.kmeter_read()
    return out


def _same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _chunk_bytes(n, C, chunk_streams):
    return chunk_streams * (((n + 3) & ~3) if C != 2 else ((n + 1) & ~1)) * C * 4


def _wide(name, sigs, fc, m):
    """[S, T, fc] in the format's sample type: every channel a signal, then the channels the map does not name overwritten with junk
    in every frame (f32: NaN / Inf / 1e30 / -Inf in turn; integers: the two extreme codes in turn)"""
    S, T = sigs.shape[:2]
    w = np.empty((S, T, fc), np.float32)
    for c in range(fc):
        w[:, :, c] = sigs[:, :, c % sigs.shape[2]] * np.float32(0.9 ** c)
    named = set(m)
    if name == "f32":
        for c in range(fc):
            if c not in named:
                w[:, :, c] = JUNK[(np.arange(T) + c) % 4][None, :]
        return w
    q = _quant(w, name)
    k = BITS[name] - 1
    for c in range(fc):
        if c not in named:
            q[:, :, c] = np.where((np.arange(T) + c) % 2, -(1 << k), (1 << k) - 1)[None, :]
    return q


def _compact(M, name, w, m):
    """the right-hand side's input: pick_decode of the wide floats, the compacted integers for PCM"""
    if name == "f32":
        return M.pick_decode(0, w, m)
    return np.ascontiguousarray(w[:, :, list(m)])


def _junk_rows(torch, raw, pitch, base):
    """the rows of `raw` (uint8 [S, row_bytes]) in a device buffer at byte `base` + s * pitch; every other byte of the buffer is part
    of a NaN / Inf / 1e30 pattern (as floats) and of near-full-scale codes (as integers)"""
    S, rb = raw.shape
    pat = np.array([np.nan, np.inf, 1e30, -np.inf], np.float32).view(np.uint8)
    host = np.resize(pat, base + S * pitch + 64)
    for s in range(S):
        host[base + s * pitch: base + s * pitch + rb] = raw[s]
    return torch.from_numpy(host).cuda()


def _run(M, name, w, fc, m, C, meters, calls, fs, chunk_streams, entry, lengths=None, base_samples=0, extra_stride=0, aligned_compact=False, **kw):
    """One engine over `calls`, with the layout on the wide input (wide=True) or the default layout on its compact form.
    entry: "host" (process / process_lengths / process_pcm) or "device" (process_device / _device_lengths / _device_pcm)."""
    import torch
    S = w.shape[0]
    sb = BITS[name] // 8
    # the calls' inputs: the wide cut (with junk behind each stream's length) and its compact form
    cuts, pos = [], 0
    for i, n in enumerate(calls):
        cw = np.ascontiguousarray(w[:, pos:pos + n])
        fr = None if lengths is None or lengths[i] is None else np.minimum(lengths[i], n).astype(np.uint64)
        if fr is not None:
            for s in range(S):
                k = n - int(fr[s])
                cw[s, int(fr[s]):] = JUNK[np.arange(k) % 4][:, None] if name == "f32" else (1 << (BITS[name] - 1)) - 1
        cuts.append((cw, _compact(M, name, cw, m), fr))
        pos += n
    assert pos == w.shape[1]
    got = []
    for wide in (True, False):
        W = fc if wide else C
        recs, closed = [], np.zeros(S, bool)
        with M.Engine(S, fs, meters, n_channels=C, **kw) as e:
            if wide:
                e.set_frame_layout(fc, m)
                assert e.frame_layout() == (fc, tuple(m))
            if meters & M.METER_EBU:
                e.integr_start()
            for i, n in enumerate(calls):
                e.set_host_chunk_bytes(_chunk_bytes(n, C, chunk_streams))
                cut, fr = cuts[i][0 if wide else 1], cuts[i][2]
                raw = _raw(cut, name)
                if entry == "host":
                    if name == "f32":
                        e.process(raw) if fr is None else e.process_lengths(raw, fr)
                    else:
                        e.process_pcm(raw, _fmt(M, name), frames=fr)
                else:
                    rows = raw.view(np.uint8).reshape(S, -1)
                    stride = n + extra_stride
                    base = base_samples * sb
                    if not wide and aligned_compact:                 # rows on 16 bytes, as the staged ones are
                        stride, base = (n + 3) & ~3, 0
                    buf = _junk_rows(torch, rows, stride * W * sb, base)
                    st = torch.cuda.current_stream().cuda_stream
                    if name == "f32":
                        if fr is None:
                            e.process_device(buf.data_ptr() + base, n, stride, st)
                        else:
                            e.process_device_lengths(buf.data_ptr() + base, n, fr, stride, st)
                    else:
                        e.process_device_pcm(buf.data_ptr() + base, _fmt(M, name), n, stride=stride, frames=fr, stream=st)
                    e.sync()
                    del buf
                rec = _records(M, e, meters)
                if "frag" in rec and (fr is not None or closed.any()):
                    # fragment powers exist for the fragments that end in front of a stream's end: what lies behind it in the getter's
                    # rows is never written (tests/test_gpu_pcm.py:_snap leaves the record out for the same reason)
                    # (`lengths` may name the FIRST call only: it starts on a fragment boundary, so fr // fragment is the count below)
                    assert fr is None or i == 0, "_run: lengths only for calls[0]"
                    f = rec["frag"].copy()
                    for s in range(S):
                        if closed[s]:
                            f[s] = 0
                        elif fr is not None and fr[s] < n:
                            f[s, int(fr[s]) // (int(fs) // 20):] = 0
                    rec["frag"] = f
                if fr is not None:
                    closed |= fr < n
                recs.append(rec)
            staged, direct = e.layout_stats()
            want = (sum(-(-S // chunk_streams) for _ in calls), 0) if wide else (0, 0)
            if wide and entry == "device" and name == "f32" and (C, fc, tuple(m)) == (5, 6, WAVE51):
                want = (0, len(calls))                               # device f32 WAVE 5.1: k_kwmc reads the wide frames itself
            assert (staged, direct) == want, (staged, direct, want)
            got.append((recs, e.seg_stats(), e.state_export(), e.stream_frames(), e.pcm_stats()[:2]))
    (a, seg_a, blob_a, fr_a, pcm_a), (b, seg_b, blob_b, fr_b, pcm_b) = got
    assert seg_a == seg_b                                                # the same kernels served both
    for i, (x_, y_) in enumerate(zip(a, b)):
        _same(x_, y_, (name, entry, "call", i))
    assert blob_a == blob_b
    assert np.array_equal(fr_a[0], fr_b[0]) and np.array_equal(fr_a[1], fr_b[1])
    if name == "f32":
        assert pcm_a == (0, 0) and (entry == "device" or pcm_b == (0, 0))   # wide f32 is no PCM
    else:
        assert pcm_a[0] == pcm_b[0] and pcm_a[1] * C == pcm_b[1] * fc      # the same chunks, the source bytes by frame width
    return seg_a


T4 = 2400 * 12 + 1234
CALLS4 = [2400 * 5 + 1001, 1, 2400 * 3 + 777, T4 - (2400 * 8 + 1779)]    # the first ends mid-fragment; one of 1 frame; odd counts


def _stereo(S, T, seed):
    return np.stack([sig.g2(T, seed + s) * np.float32(2.0 ** -(s % 4)) for s in range(S)])


@pytest.fixture(scope="module")
def sigs():
    S = 11
    return _stereo(S, T4, 300)


CONFIGS = {
    # name: (meters, engine channels, frame_channels, map, fs, chunk_streams, engine knobs, k_seg calls expected or None)
    "stereo_of_8": ("EBU|TRUEPEAK", 2, 8, (6, 7), 48000.0, 5, {}, 0),
    "stereo_of_8_seg": ("EBU|TRUEPEAK", 2, 8, (6, 7), 48000.0, 11, dict(tune_segments=2), None),
    "five_of_6": ("EBU|TRUEPEAK", 5, 6, WAVE51, 48000.0, 5, {}, None),
    "three_of_8": ("EBU|TRUEPEAK", 3, 8, (7, 2, 5), 44100.0, 1, {}, None),
    "four_of_8": ("EBU", 4, 8, (3, 0, 6, 1), 48000.0, 5, {}, None),
    "bank_of_4": ("SPECTR30", 2, 4, (2, 1), 48000.0, 5, {}, None),
    "tpb_dr_km_of_4": ("TPBALLIST|DR14|KMETER", 2, 4, (3, 0), 44100.0, 11, {}, None),
    "mono_int_of_2": ("BITSTATS|SIGDIST", 1, 2, (1,), 48000.0, 1, {}, None),
    "mono_file": ("EBU|TRUEPEAK", 2, 1, (0, 0), 48000.0, 5, {}, None),
}


@pytest.mark.timeout(900)
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("name", FORMATS)
def test_host_entries_equal_the_compact_call(M, sigs, name, cfg):
    names, C, fc, m, fs, cs, kw, want_seg = CONFIGS[cfg]
    w = _wide(name, sigs, fc, m)
    seg = _run(M, name, w, fc, m, C, _mask(M, names), CALLS4, fs, cs, "host", **kw)
    if want_seg is not None:
        assert seg[0] == want_seg, seg


@pytest.mark.timeout(900)
@pytest.mark.parametrize("cfg", ["stereo_of_8", "five_of_6", "three_of_8", "tpb_dr_km_of_4", "mono_int_of_2", "mono_file"])
@pytest.mark.parametrize("name", FORMATS)
def test_device_entries_equal_the_compact_call(M, sigs, name, cfg):
    """... the device forms on rows that start an odd number of samples into the buffer, odd strides, junk between the rows"""
    names, C, fc, m, fs, cs, kw, _ = CONFIGS[cfg]
    w = _wide(name, sigs, fc, m)
    # (the SDH's double sums are grouped by the alignment of the floats the meters read, tests/test_gpu_hostpath.py: the compact f32
    # rows of that engine lie on 16 bytes, as the staged ones do)
    al = "SIGDIST" in names and name == "f32"
    _run(M, name, w, fc, m, C, _mask(M, names), CALLS4, fs, cs, "device", base_samples=3, extra_stride=1, aligned_compact=al, **kw)
    _run(M, name, w[:, :sum(CALLS4[:2])], fc, m, C, _mask(M, names), CALLS4[:2], fs, 11, "device", aligned_compact=al, **kw)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("name", FORMATS)
def test_lengths_entries(M, sigs, name, entry):
    """the two _lengths entries and the PCM entries with lengths: streams that close inside the call, at 0, one frame short"""
    S = sigs.shape[0]
    n = CALLS4[0]
    L0 = np.array([n, 2400 * 3 + 1001, 0, n, 1, 2400 * 2, n - 1, n, 5000, n, 77], np.uint64)[:S]
    for cfg in ("stereo_of_8", "five_of_6"):
        names, C, fc, m, fs, cs, kw, _ = CONFIGS[cfg]
        w = _wide(name, sigs, fc, m)
        _run(M, name, w, fc, m, C, _mask(M, names), CALLS4, fs, cs, entry, lengths=[L0, None, None, None], **kw)


@pytest.mark.timeout(900)
def test_big_batch_through_k_seg(M):
    """stereo from 8-channel s16 frames at a batch the planner sends to k_seg by itself (the shape of tests/test_gpu_pcm.py's big
    case, asked of mtr_plan_query), device memory: equal to the device PCM call on the compacted integers"""
    import torch
    S, n = 4096, 2400 * 64
    assert M.plan_query(S, n)["uses_seg"] == 1
    g = torch.Generator(device="cuda"); g.manual_seed(12)
    q = torch.randint(-12000, 12000, (S, n, 8), dtype=torch.int16, device="cuda", generator=g)
    q[:, :, :6] = torch.where(torch.arange(n, device="cuda")[None, :, None] % 2 == 0, 32767, -32768).to(torch.int16)   # the unnamed channels
    q[17, 4711, 6], q[4095, n - 1, 7] = -32768, 32767
    comp = q[:, :, 6:].contiguous()
    st = torch.cuda.current_stream().cuda_stream
    got = []
    for wide in (True, False):
        with M.Engine(S, 48000.0, M.METER_EBU | M.METER_TRUEPEAK) as e:
            e.integr_start()
            e.set_host_chunk_bytes(S * n * 2 * 4)
            if wide:
                e.set_frame_layout(8, (6, 7))
                e.process_device_pcm(q.data_ptr(), M.PCM_S16, n, stream=st)
            else:
                e.process_device_pcm(comp.data_ptr(), M.PCM_S16, n, stream=st)
            got.append((_records(M, e, M.METER_EBU | M.METER_TRUEPEAK), e.seg_stats(), e.state_export(), e.layout_stats()))
    assert got[0][1] == got[1][1] and got[0][1][0] >= 1, got[0][1]      # k_seg took both
    _same(got[0][0], got[1][0], "4096 x 3.2 s")
    assert got[0][2] == got[1][2]
    assert got[0][3] == (1, 0) and got[1][3] == (0, 0)


def test_routing_and_stats(M, sigs):
    """After a device f32 call with the WAVE 5.1 layout layout_stats shows a direct call and no staged chunk (k_kwmc51 read the wide
    frames itself) and pcm_stats is untouched; with a permuted 5-of-6 map the same engine stages, and gives the same records as the
    direct form on suitably arranged input — two calls each, one with lengths; the host forms of WAVE 5.1 stage; the explicit identity
    and frame_channels = 0 stage nothing and count nothing"""
    import torch
    S, n = sigs.shape[0], 2400 * 4 + 10
    meters = M.METER_EBU | M.METER_TRUEPEAK
    w = _wide("f32", sigs[:, :n], 6, WAVE51)
    perm = (5, 0, 4, 1, 2)
    w2 = np.full_like(w, np.nan)
    for c in range(5):
        w2[:, :, perm[c]] = w[:, :, WAVE51[c]]                          # the same programme, arranged for the other map
    st = torch.cuda.current_stream().cuda_stream
    recs = []
    h = 2400 * 2 + 7
    L = np.array([n - h, 1000, 0, n - h, 1, 2400, n - h - 1, n - h, 500, n - h, 77], np.uint64)[:S]
    for lay, x, want in (((6, WAVE51), w, (0, 2)), ((6, perm), w2, (2, 0))):
        dev = torch.from_numpy(x).cuda()
        with M.Engine(S, 48000.0, meters, n_channels=5) as e:
            e.integr_start()
            e.set_frame_layout(*lay)
            e.process_device(dev.data_ptr(), h, n, st)                   # (ends mid-fragment; the rows of the second call start on 8 bytes)
            r0 = _records(M, e, meters)
            e.process_device_lengths(dev.data_ptr() + h * 6 * 4, n - h, L, n, st)
            r1 = _records(M, e, meters)
            r1.pop("frag")                                               # (rows behind a closed stream's end are never written)
            recs.append((r0, r1, e.state_export()))
            assert e.layout_stats() == want and e.pcm_stats() == (0, 0, 0.0)
            if lay[1] == WAVE51:
                e.process(np.ascontiguousarray(x[:, :100]))              # the host form of the same layout stages
                assert e.layout_stats() == (1, 2)
    _same(recs[0][0], recs[1][0], "direct against staged")
    _same(recs[0][1], recs[1][1], "direct against staged, with lengths")
    assert recs[0][2] == recs[1][2]
    five = M.pick_decode(0, w, WAVE51)
    dev = torch.from_numpy(five).cuda()
    with M.Engine(S, 48000.0, meters, n_channels=5) as e:
        e.integr_start()
        e.set_frame_layout(5, (0, 1, 2, 3, 4))
        assert e.frame_layout() == (5, (0, 1, 2, 3, 4))
        e.process_device(dev.data_ptr(), n, n, st)
        e.process(five)
        a = _records(M, e, meters)
        e.set_frame_layout(0)
        assert e.frame_layout() == (5, (0, 1, 2, 3, 4))
        e.process(five)
        assert e.layout_stats() == (0, 0)
    with M.Engine(S, 48000.0, meters, n_channels=5) as e:
        e.integr_start()
        e.process_device(dev.data_ptr(), n, n, st)
        e.process(five)
        _same(a, _records(M, e, meters), "the explicit identity")


def test_switching_layouts_continues_the_streams(M, sigs):
    S, meters = sigs.shape[0], M.METER_EBU | M.METER_TRUEPEAK
    h = T4 // 2 + 3
    wa = _wide("f32", sigs[:, :h], 8, (6, 7))
    wb = _wide("s24", sigs[:, h:], 4, (2, 0))
    ca, cb = M.pick_decode(0, wa, (6, 7)), np.ascontiguousarray(wb[:, :, [2, 0]])
    with M.Engine(S, 48000.0, meters) as e:
        e.integr_start()
        e.set_frame_layout(8, (6, 7))
        e.process(wa)
        e.set_frame_layout(4, (2, 0))
        e.process_pcm(_raw(wb, "s24"), M.PCM_S24)
        a, blob_a = _records(M, e, meters), e.state_export()
        e.reset()                                                        # (the layout describes buffers: a reset keeps it)
        assert e.frame_layout() == (4, (2, 0))
    with M.Engine(S, 48000.0, meters) as e:
        e.integr_start()
        e.process(ca)
        e.process_pcm(_raw(cb, "s24"), M.PCM_S24)
        _same(a, _records(M, e, meters), "one engine fed the compact halves")
        assert blob_a == e.state_export()


def test_bad_arguments_leave_layout_and_results(M, sigs):
    S, meters = sigs.shape[0], M.METER_EBU | M.METER_TRUEPEAK
    w = _wide("f32", sigs[:, :5000], 6, WAVE51)
    L = M.lib
    with M.Engine(S, 48000.0, meters, n_channels=5) as e:
        e.integr_start()
        e.set_frame_layout(6, WAVE51)
        e.process(w)
        before, blob = _records(M, e, meters), e.state_export()
        ok = np.array(WAVE51, np.uint8)
        bad = np.array([0, 1, 2, 4, 6], np.uint8)
        assert L.mtr_engine_set_frame_layout(e._h, 9, ok.ctypes.data) == -1
        assert L.mtr_engine_set_frame_layout(e._h, 6, None) == -1
        assert L.mtr_engine_set_frame_layout(e._h, 6, bad.ctypes.data) == -1
        assert L.mtr_engine_set_frame_layout(e._h, 4, ok.ctypes.data) == -1           # entries 4 and 5 >= 4
        assert e.frame_layout() == (6, WAVE51)
        _same(before, _records(M, e, meters), "after argument errors")
        assert blob == e.state_export() and e.layout_stats() == (1, 0)
        assert L.mtr_engine_process_host(e._h, w.ctypes.data, 5000, 4999) == -1     # stride < n_frames
        assert e.layout_stats() == (1, 0)
        with pytest.raises(ValueError):
            e.set_frame_layout(6, (0, 1))


@pytest.mark.parametrize("case", [c for c in _mc.GOLDEN_CASES if c[0] == 1], ids=lambda c: f"c1_{int(c[1])}_{c[2]}")
def test_mono_file_vs_golden_mc(M, case):
    """The reference's own mono results (golden_mc_v1, c1_*): a stereo engine, frame_channels = 1, map {0, 0}, the seed rule of
    tests/test_gpu_multichannel.py::test_vs_golden_mc."""
    import torch
    n, fs, blk, sec, start = case
    T = int(sec * fs)
    x = _mc.programme(T, 1, seed=n * 10 + int(fs) % 7 + blk % 3)
    dev = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    with M.Engine(1, fs, M.METER_EBU | M.METER_TRUEPEAK) as e:
        e.set_frame_layout(1, (0, 0))
        for i, o in enumerate(range(0, T, blk)):
            if i == start:
                e.integr_start()
            e.process_device(dev.data_ptr() + o * 4, min(blk, T - o), T)
        torch.cuda.synchronize()
        out9, (hm, hs), tp = e.out9(), e.histograms(), e.truepeak()
        hold = e.truepeak_channels()[0]
    k = f"c1_{int(fs)}_{blk}"
    check9(out9[0], G[k + "_out9"])
    check_hist(hm[0], G[k + "_hist_M"]); check_hist(hs[0], G[k + "_hist_S"])
    assert tp[0, 0] == tp[0, 1] and hold[0, 0] == hold[0, 1]
    assert np.allclose(tp[0, 0], G[k + "_tp"], rtol=TP_REL, atol=0)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("fs", [48000.0, 44100.0])
def test_wave51_vs_oracle(M, fs):
    """16 streams x 30 s of 6-channel programme, WAVE 5.1 layout, from device f32 (direct) and from host S24 (staged): every 4th stream against the
    multichannel oracle on the picked channels."""
    import torch
    S, T = 16, int(30 * fs)
    x = np.stack([_mc.programme(T, 6, 600 + s) for s in range(S)])
    q = _quant(x, "s24")
    meters = M.METER_EBU | M.METER_TRUEPEAK
    res = {}
    dev = torch.from_numpy(x).cuda()
    for how in ("device", "host_s24"):
        with M.Engine(S, fs, meters, n_channels=5) as e:
            e.set_frame_layout(6, WAVE51)
            e.integr_start()
            if how == "device":
                e.process_device(dev.data_ptr(), T, T, torch.cuda.current_stream().cuda_stream)
            else:
                e.process_pcm(_raw(q, "s24"), M.PCM_S24)
            res[how] = (e.out9(), e.histograms(), e.truepeak_channels()[0], e.layout_stats())
    assert res["device"][3] == (0, 1) and res["host_s24"][3][0] >= 1 and res["host_s24"][3][1] == 0   # direct / staged
    for how, src in (("device", x[:, :, list(WAVE51)]), ("host_s24", M.pick_decode(M.PCM_S24, _raw(q, "s24").reshape(S, T, 18), WAVE51))):
        out9, (hm, hs), hold, _ = res[how]
        for s in range(0, S, 4):
            o = _mc.McStream(5, fs)
            o.start()
            o.process(np.ascontiguousarray(src[s]))
            want9, whm, whs, _ = o.get()
            check9(out9[s], want9)
            check_hist(hm[s], whm); check_hist(hs[s], whs)
            assert np.allclose(hold[s], o.hold, rtol=TP_REL, atol=0), (how, s)
