"""Plane layouts on the GPU: mtr_engine_set_plane_layout (include/mtr_planes.h), k_plane (mtr_source.hip) in front of the meters.

The rule of tests/test_gpu_frames.py, no tolerance anywhere: a call with a plane layout on the PLANAR buffer against the same entry point
with the default layout on plane_decode of that buffer (for PCM: on the interleaved integers, whose pcm_decode is checked to be that
plane_decode), same set_host_chunk_bytes — every record of every meter np.array_equal, seg_stats () equal, state blobs byte-equal after
the last call.  (tests/test_planes_cpu.py pins mtr_plane_decode_host to numpy bit for bit.)  The planes the map does not name, the samples
behind n_frames up to the stride, the frames behind a stream's length and every other byte of the buffers hold NaN, Inf and 1e30 (integer
PCM: the extreme codes); everything lies inside the allocations.

The shapes: 5 streams, n_frames in {1, 3, 4, 7, 2401, 5003} — fewer frames than a group of four, whole groups only, groups and a rest,
more than a fragment, more than a tile of 4096 — with strides n_frames + {0, 1, 2, 3, 5}, which put the plane starts on and off 16, 8, 4
and 2 bytes; where chunking is exercised the chunk size cuts the 5 streams into 2 + 2 + 1.  The engines of a case are made once and
reset between its runs."""
import numpy as np
import pytest

import _signals as sig
import test_gpu_frames as F

pytestmark = pytest.mark.gpu

S = 5
SIZES = [1, 3, 4, 7, 2401, 5003]
EXTRA = [0, 1, 2, 3, 5]
FS = 48000.0
BITS = F.BITS
NP_T = {"f32": np.float32, "s16": np.int16, "s32": np.int32}
STEREO_ENGINES = ["EBU|TRUEPEAK", "SPECTR30|TPBALLIST", "DR14|KMETER|STCORR|NEEDLE", "SCOPE", "GONIO"]
STEREO_LAYOUTS = [(2, (0, 1)), (2, (1, 0)), (1, (0, 0)), (4, (3, 1))]


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


@pytest.fixture(scope="module")
def audio():
    """[8, 2 * 5003 + 16] float32, read-only: eight channels' worth of programme, computed once"""
    T = 2 * SIZES[-1] + 16
    a = np.concatenate([sig.g2(T, 900 + k).T * np.float32(0.9 ** k) for k in range(4)]).astype(np.float32)
    a.setflags(write=False)
    return a


def _sb(name):
    return BITS[name] // 8


def _junk_bytes(name, n):
    """n bytes of the pattern everything unnamed holds: NaN / Inf / 1e30 / -Inf as f32, the two extreme codes in turn as integers"""
    if name == "f32":
        pat = F.JUNK.view(np.uint8)
    else:
        k = BITS[name] - 1
        pat = np.array([(1 << k) - 1, -(1 << k)], "<i4").view(np.uint8).reshape(2, 4)[:, : _sb(name)] if name == "s24" else \
            np.array([(1 << k) - 1, -(1 << k)], "<i2" if name == "s16" else "<i4").view(np.uint8)
    return np.resize(np.ascontiguousarray(pat).reshape(-1), n)


def _pack(x, name):
    """typed samples [..., n] as bytes [..., n * sample bytes] (s24: packed little endian)"""
    if name == "s24":
        b = np.ascontiguousarray(x.astype("<i4")).view(np.uint8).reshape(x.shape + (4,))[..., :3]
        return np.ascontiguousarray(b).reshape(x.shape[:-1] + (-1,))
    return np.ascontiguousarray(x).view(np.uint8).reshape(x.shape[:-1] + (-1,))


class Planar:
    """One planar buffer: S streams of P planes, `stride` samples apart, `lead` bytes into a junk-filled allocation; the named planes hold
    `total` samples of programme (stream s scaled by 2^-(s mod 4), plane p taking channel p of `audio`), everything else junk."""

    def __init__(self, audio, name, P, m, total, stride, lead, C):
        self.name, self.P, self.m, self.total, self.stride, self.lead, self.C = name, P, tuple(m), total, stride, lead, C
        sb = _sb(name)
        self.buf = np.concatenate([_junk_bytes(name, lead), _junk_bytes(name, S * P * stride * sb + 64)])   # (the pattern starts with plane 0)
        self.x = {}                                                       # (s, p) -> typed samples [total]
        for s in range(S):
            for p in set(m):
                v = audio[p % audio.shape[0], 11 * s: 11 * s + total] * np.float32(2.0 ** -(s % 4))
                self.x[(s, p)] = v if name == "f32" else F._quant(v, name)
                self._put(s, p, 0, self.x[(s, p)])

    def _at(self, s, p, t0=0):
        return self.lead + ((s * self.P + p) * self.stride + t0) * _sb(self.name)

    def _put(self, s, p, t0, v):
        b = _pack(np.asarray(v), self.name).reshape(-1)
        self.buf[self._at(s, p, t0): self._at(s, p, t0) + b.size] = b

    def cut(self, t0, n, fr):
        """junk behind each stream's length fr[s] inside the window [t0, t0 + n) of its named planes"""
        for s in range(S):
            k = n - int(fr[s])
            if k:
                for p in set(self.m):
                    at = self._at(s, p, t0 + int(fr[s]))
                    self.buf[at: at + k * _sb(self.name)] = _junk_bytes(self.name, k * _sb(self.name))

    def window(self, t0, n):
        """the window [t0, t0 + n) of every plane, a VIEW of the buffer: bytes [S, P, n * sample bytes]"""
        sb = _sb(self.name)
        return self.buf[self.lead: self.lead + S * self.P * self.stride * sb].reshape(S, self.P, self.stride * sb)[:, :, t0 * sb: (t0 + n) * sb]

    def compact(self, M, t0, n):
        """the window as the reference takes it: [S, n, C] float32 = plane_decode of the buffer (f32), or the interleaved integers"""
        w = self.window(t0, n)
        dec = M.plane_decode(F._fmt(M, self.name), w if self.name == "s24" else w.view(NP_T[self.name]), self.m)
        if self.name == "f32":
            return dec
        sb = _sb(self.name)
        q = np.ascontiguousarray(w.reshape(S, self.P, n, sb)[:, list(self.m)].transpose(0, 2, 1, 3)).reshape(S, n * self.C * sb)   # [S, n, C] samples as bytes
        typed = q if self.name == "s24" else q.view(NP_T[self.name]).reshape(S, n, self.C)
        want = M.pcm_decode(F._fmt(M, self.name), typed).reshape(S, n, self.C)
        assert np.array_equal(want.view(np.uint32), dec.view(np.uint32))    # the integers' decode IS plane_decode of the planes
        return typed


def _setup(M, e, meters):
    if meters & M.METER_EBU:
        e.integr_start()
    if meters & M.METER_NEEDLE:
        e.needle_configure(M.NEEDLE_VU | M.NEEDLE_IEC1 | M.NEEDLE_IEC2 | M.NEEDLE_MS)
    if meters & M.METER_SCOPE:
        e.scope_configure(256, 100)
    if meters & M.METER_GONIO:
        e.gonio_configure(period_frames=480, capacity=16, tune_piece=1024, shift=2)


def _records(M, e, meters, ragged):
    """every record of every meter: tests/test_gpu_frames.py's list and the meters it does not hold"""
    out = F._records(M, e, meters)
    if ragged:
        out.pop("frag", None)                                             # (rows behind a closed stream's end are never written)
    groups = {}
    if meters & M.METER_STCORR:
        groups["stcorr"] = e.stcorr_read()
    if meters & M.METER_NEEDLE:
        for k in (M.NEEDLE_VU, M.NEEDLE_IEC1, M.NEEDLE_IEC2, M.NEEDLE_MS):
            groups[f"needle{k}"] = e.needle_read(k)
    if meters & M.METER_SCOPE:
        groups["scope"] = tuple(v for _, v in sorted(e.scope_read().items())) + (np.array([e.scope_analyses()]),)
    if meters & M.METER_GONIO:
        groups["gonio"] = e.gonio_image() + e.gonio_read() + (np.array(e.gonio_blocks()),)
    if meters & M.METER_SURROUND:
        groups["sur"] = e.surround_read() + (e.surround_pair_states(),)
    for g, vals in groups.items():
        for i, v in enumerate(vals):
            out[f"{g}[{i}]"] = np.asarray(v)
    return out


def _dstride(n, C):
    return (n + 1) & ~1 if C == 2 else (n + 3) & ~3


class Pair:
    """The two engines of a case: `a` takes the planar buffers under a plane layout, `b` their plane_decode under the default layout."""

    def __init__(self, M, names, C=2, **kw):
        self.M, self.meters, self.C = M, F._mask(M, names), C
        self.a, self.b = M.Engine(S, FS, self.meters, n_channels=C, **kw), M.Engine(S, FS, self.meters, n_channels=C, **kw)
        self.staged = 0

    def close(self):
        self.a.close(), self.b.close()

    def run(self, pl, calls, host, chunked, family=None, lengths=None):
        """calls: [(t0, n)] windows of the buffer `pl`; lengths: per call None or [S] frames; compares after every call"""
        import torch
        M, a, b, C = self.M, self.a, self.b, self.C
        fmt, sb = F._fmt(M, pl.name), _sb(pl.name)
        for e in (a, b):
            e.reset()
            _setup(M, e, self.meters)
        a.set_plane_layout(pl.P, pl.m)
        assert a.plane_layout() == (pl.P, pl.m) and a.frame_layout() == (C, tuple(range(C)))
        assert b.plane_layout() == (0, tuple(range(C)))
        for (t0, n), fr in zip(calls, lengths or [None] * len(calls)):
            fr = None if fr is None else np.asarray(fr, np.uint64)
            family = family if fr is not None else None                    # (a dense call rides the plain entry point)
            if fr is not None:
                pl.cut(t0, n, fr)
            comp = pl.compact(M, t0, n)
            chunk = F._chunk_bytes(n, C, 2 if chunked else S)
            a.set_host_chunk_bytes(chunk), b.set_host_chunk_bytes(chunk)
            if host:
                a.process_raw(pl.buf.ctypes.data + pl.lead + t0 * sb, n, pl.stride, fmt, fr, family, host=True)
                b.process_raw(comp.ctypes.data, n, n, fmt, fr, family, host=True)
            else:
                st = torch.cuda.current_stream().cuda_stream
                dev = torch.from_numpy(pl.buf).cuda()
                a.process_raw(dev.data_ptr() + pl.lead + t0 * sb, n, pl.stride, fmt, fr, family, stream=st)
                # the reference's rows lie as the staged ones do (on 16 bytes, the staged stride: tests/test_gpu_frames.py, aligned_compact), junk between them
                ds = _dstride(n, C)
                rows = F._junk_rows(torch, comp.reshape(S, -1).view(np.uint8), ds * C * sb, 0)
                b.process_raw(rows.data_ptr(), n, ds, fmt, fr, family, stream=st)
                a.sync(), b.sync()
                del dev, rows
            self.staged += -(-S // 2) if chunked else 1
            what = (pl.name, pl.P, pl.m, n, pl.stride, pl.lead, "host" if host else "device", family)
            F._same(_records(M, a, self.meters, fr is not None or a.stream_frames()[1].any()),
                    _records(M, b, self.meters, fr is not None or b.stream_frames()[1].any()), what)
            assert np.array_equal(a.stream_frames()[0], b.stream_frames()[0]) and np.array_equal(a.stream_frames()[1], b.stream_frames()[1]), what
        assert a.seg_stats() == b.seg_stats(), what                        # the same kernels served both
        assert a.state_export() == b.state_export(), what
        assert a.plane_stats() == self.staged and b.plane_stats() == 0, (a.plane_stats(), self.staged)
        assert a.layout_stats() == (0, 0)                                  # k_pick's count does not move
        if pl.name != "f32":
            assert a.pcm_stats()[0] == b.pcm_stats()[0]                    # the same chunks


def _lead(name, i):
    """bytes in front of plane 0: whole samples (S24: any byte), so that with the strides the planes start on and off 16, 8, 4 and 2"""
    return (0, 3, 1, 2)[i % 4] * (1 if name == "s24" else _sb(name))


@pytest.mark.parametrize("names", STEREO_ENGINES)
@pytest.mark.parametrize("name", F.FORMATS)
def test_stereo_engines_one_call(M, audio, name, names):
    """every format x engine: the four layouts, host and device, every size, every stride; chunks of 2 + 2 + 1 on every other run"""
    pair = Pair(M, names)
    try:
        i = 0
        for P, m in STEREO_LAYOUTS:
            for host in (True, False):
                for n in SIZES:
                    pl = Planar(audio, name, P, m, n, n + EXTRA[i % 5], _lead(name, i), 2)
                    pair.run(pl, [(0, n)], host, chunked=i % 2 == 0)
                    i += 1
    finally:
        pair.close()


@pytest.mark.parametrize("names", STEREO_ENGINES)
@pytest.mark.parametrize("name", F.FORMATS)
def test_stereo_engines_two_windows_of_a_long_buffer(M, audio, name, names):
    """two calls walking one long buffer: base + t0, stride = the planes' whole length (and more)"""
    pair = Pair(M, names)
    try:
        i = 0
        for P, m in STEREO_LAYOUTS:
            for host in (True, False):
                for n1, n2 in ((2401, 5003), (7, 4), (1, 3), (5003, 1)):
                    total = n1 + n2 + 5
                    pl = Planar(audio, name, P, m, total, total + EXTRA[i % 5], _lead(name, i + 1), 2)
                    pair.run(pl, [(0, n1), (n1, n2)], host, chunked=i % 2 == 1)
                    i += 1
    finally:
        pair.close()


WIDTHS = {
    # name: (meters, engine channels, [(P, map)])
    "five_of_6": ("EBU|TRUEPEAK", 5, [(6, (0, 1, 2, 4, 5))]),
    "mono_of_3": ("BITSTATS|SIGDIST", 1, [(3, (2,))]),
    "surround6": ("SURROUND", 6, [(6, (0, 1, 2, 3, 4, 5)), (6, (5, 2, 0, 3, 1, 4))]),
    "surround8": ("SURROUND", 8, [(8, (0, 1, 2, 3, 4, 5, 6, 7)), (8, (7, 0, 3, 6, 5, 1, 4, 2))]),
}


@pytest.mark.parametrize("cfg", list(WIDTHS))
@pytest.mark.parametrize("name", F.FORMATS)
def test_other_widths(M, audio, name, cfg):
    names, C, layouts = WIDTHS[cfg]
    pair = Pair(M, names, C=C)
    try:
        i = 0
        for P, m in layouts:
            for host in (True, False):
                for n in SIZES:
                    pl = Planar(audio, name, P, m, n, n + EXTRA[(i + 1) % 5], _lead(name, i), C)
                    pair.run(pl, [(0, n)], host, chunked=i % 2 == 0)
                    i += 1
                pl = Planar(audio, name, P, m, 2401 + 7 + 2, 2401 + 7 + 2 + EXTRA[i % 5], _lead(name, i), C)
                pair.run(pl, [(0, 2401), (2401, 7)], host, chunked=True)
    finally:
        pair.close()


FAMILIES = {
    # family: an engine it accepts
    "lengths": "EBU|TRUEPEAK",
    "tracks": "EBU|TRUEPEAK|DR14|KMETER",
    "ragged": "TRUEPEAK|STCORR|NEEDLE",
    "ends": "EBU|SPECTR30",
    "tpb": "SPECTR30|TPBALLIST",
    "any": "KMETER|SCOPE",
    "gonio_ends": "STCORR|GONIO",
}


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_per_stream_lengths(M, audio, family, host):
    """the seven families on an engine each accepts: ends 0, 1, mid-call and n_frames; a dense call on the partly closed batch behind it;
    the PCM entry points with lengths ride the first family"""
    pair = Pair(M, FAMILIES[family])
    try:
        n, more = 5003, 2401
        L = np.array([0, 1, 2400 + 77, n, 4096], np.uint64)
        for i, name in enumerate(F.FORMATS if family == "lengths" else ["f32"]):
            for P, m in ((2, (1, 0)), (4, (3, 1))):
                total = n + more + 3
                pl = Planar(audio, name, P, m, total, total + EXTRA[(i + P) % 5], _lead(name, i + P), 2)
                pair.run(pl, [(0, n), (n, more)], host, chunked=True, family=family, lengths=[L, None])
    finally:
        pair.close()


def test_layout_rules(M, audio):
    meters = M.METER_EBU | M.METER_TRUEPEAK
    n = 2401
    pl = Planar(audio, "f32", 4, (3, 1), n, n + 3, 4, 2)
    comp = pl.compact(M, 0, n)
    L = M.lib
    with M.Engine(S, FS, meters) as e, M.Engine(S, FS, meters) as never:
        for x in (e, never):
            x.integr_start()
        assert e.plane_layout() == (0, (0, 1))
        # setting one layout puts the other back to its default
        e.set_frame_layout(8, (6, 7))
        e.set_plane_layout(4, (3, 1))
        assert e.plane_layout() == (4, (3, 1)) and e.frame_layout() == (2, (0, 1))
        e.set_frame_layout(8, (6, 7))
        assert e.plane_layout() == (0, (0, 1)) and e.frame_layout() == (8, (6, 7))
        e.set_plane_layout(2)                                              # map=None: the identity — still planar
        assert e.plane_layout() == (2, (0, 1)) and e.frame_layout() == (2, (0, 1))
        with pytest.raises(ValueError):
            e.set_plane_layout(3)                                          # the identity needs n_planes == n_channels
        e.set_plane_layout(4, (3, 1))
        # bad arguments leave the layout as it was
        ok, bad = np.array([3, 1], np.uint8), np.array([3, 4], np.uint8)
        assert L.mtr_engine_set_plane_layout(e._h, 9, ok.ctypes.data) == -1
        assert L.mtr_engine_set_plane_layout(e._h, 4, None) == -1
        assert L.mtr_engine_set_plane_layout(e._h, 4, bad.ctypes.data) == -1
        assert L.mtr_engine_set_plane_layout(e._h, 3, ok.ctypes.data) == -1   # entry 3 >= 3
        assert L.mtr_engine_set_frame_layout(e._h, 9, ok.ctypes.data) == -1   # ... and a refused frame layout does not take it away
        assert e.plane_layout() == (4, (3, 1)) and e.frame_layout() == (2, (0, 1))
        # plane_stats counts the chunks, layout_stats does not move; the layout survives reset () and is absent from the blob
        e.set_host_chunk_bytes(F._chunk_bytes(n, 2, 2)), never.set_host_chunk_bytes(F._chunk_bytes(n, 2, 2))
        e.process_raw(pl.buf.ctypes.data + pl.lead, n, pl.stride, host=True)
        never.process(comp)
        assert e.plane_stats() == 3 and e.layout_stats() == (0, 0) and never.plane_stats() == 0
        assert L.mtr_engine_process_host(e._h, pl.buf.ctypes.data + pl.lead, n, n - 1) == -1     # stride < n_frames
        assert e.plane_stats() == 3
        blob = e.state_export()
        assert blob == never.state_export()
        F._same(_records(M, e, meters, False), _records(M, never, meters, False), "plane layout against a never-configured engine")
        e.reset(), never.reset()
        assert e.plane_layout() == (4, (3, 1))
        assert len(e.state_export()) == len(blob) and e.state_export() == never.state_export()
        # P == 0 restores the default: the next call equals a never-configured engine's
        e.set_plane_layout(0)
        assert e.plane_layout() == (0, (0, 1)) and e.frame_layout() == (2, (0, 1))
        for x in (e, never):
            x.integr_start()
            x.process(comp)
        assert e.plane_stats() == 3 and e.layout_stats() == (0, 0)
        F._same(_records(M, e, meters, False), _records(M, never, meters, False), "after P == 0")
        assert e.state_export() == never.state_export()
        # a blob of a planar engine goes into a plain one and back
        never.state_import(e.state_export())
        assert never.plane_layout() == (0, (0, 1))


@pytest.mark.parametrize("where", ["device", "cpu", "numpy"])
def test_process_tensor(M, audio, where):
    import torch
    meters = M.METER_EBU | M.METER_TRUEPEAK
    n, total = 5003, 5003 + 2401
    x = np.stack([np.stack([audio[c, 13 * s: 13 * s + total] for c in range(2)]) for s in range(S)])      # [S, 2, total]
    for dt in ("f32", "s16", "s32"):
        first_np = x if dt == "f32" else F._quant(x, dt)
        last_np = np.ascontiguousarray(first_np.transpose(0, 2, 1))
        blobs = []
        for arr, cf in ((first_np, True), (last_np, False)):
            t = arr if where == "numpy" else torch.from_numpy(arr)
            if where == "device":
                t = t.cuda()
            with M.Engine(S, FS, meters) as e:
                e.integr_start()
                e.set_frame_layout(4, (3, 1))                              # what stood before the calls ...
                # the whole length in two windows, the first by shape (width 2 on one axis only), the second as told
                w1 = t[:, :, :n] if cf else t[:, :n]
                w2 = t[:, :, n:] if cf else t[:, n:]
                e.process_tensor(w1)
                assert e.frame_layout() == (4, (3, 1)) and e.plane_layout() == (0, (0, 1))      # ... stands after them
                e.set_plane_layout(3, (2, 0))
                e.process_tensor(w2, channels_first=cf)
                assert e.plane_layout() == (3, (2, 0)) and e.frame_layout() == (2, (0, 1))
                assert e.plane_stats() == (2 if cf else 0)
                # a refused tensor, and a call refused by the library, leave layout and results alone
                before = e.state_export()
                with pytest.raises(ValueError):
                    e.process_tensor(w1.swapaxes(1, 2))
                with pytest.raises(ValueError):
                    e.process_tensor(w1[:3])                               # three streams
                with pytest.raises(ValueError):
                    e.process_tensor(arr.astype(np.float64) if where == "numpy" else t.double())
                with pytest.raises(M.EngineError):
                    e.process_tensor(w1, frames=[n + 1] * S)
                assert e.plane_layout() == (3, (2, 0)) and e.frame_layout() == (2, (0, 1))
                assert e.state_export() == before
                blobs.append((before, F._records(M, e, meters)))
        assert blobs[0][0] == blobs[1][0], (where, dt)                     # channels first and channels last of the same samples
        F._same(blobs[0][1], blobs[1][1], (where, dt))
    # ... and equal to the raw calls on the interleaved floats
    with M.Engine(S, FS, meters) as e:
        e.integr_start()
        il = np.ascontiguousarray(F._quant(x, "s32").transpose(0, 2, 1))
        e.process_pcm(np.ascontiguousarray(il[:, :n]))
        e.process_pcm(np.ascontiguousarray(il[:, n:]))
        assert e.state_export() == blobs[0][0]


def test_process_tensor_families_and_maps(M, audio):
    """frames / family reach the entry points; a map over a wider tensor; a mono tensor on a stereo engine"""
    import torch
    n = 2401
    x = np.stack([np.stack([audio[c, 7 * s: 7 * s + n] for c in range(4)]) for s in range(S)])           # [S, 4, n]
    t = torch.from_numpy(x).cuda()
    L = np.array([0, 1, 1200, n, 2400], np.uint64)
    with M.Engine(S, FS, M.METER_KMETER | M.METER_SCOPE) as a, M.Engine(S, FS, M.METER_KMETER | M.METER_SCOPE) as b:
        a.process_tensor(t, map=(3, 1), frames=L, family="any")
        a.sync()
        b.process_any(M.plane_decode(0, x, (3, 1)), L)
        assert a.state_export() == b.state_export() and a.plane_stats() == 1
        with pytest.raises(M.EngineError):
            a.process_tensor(t, map=(3, 1), frames=L, family="lengths")    # (the family refuses the engine)
        with pytest.raises(ValueError):
            a.process_tensor(t, map=(3, 1), family="any")                  # a family takes lengths
    with M.Engine(S, FS, M.METER_EBU | M.METER_TRUEPEAK) as a, M.Engine(S, FS, M.METER_EBU | M.METER_TRUEPEAK) as b:
        a.process_tensor(t[:, 2:3], map=(0, 0))                            # (S, 1, n): one plane, 4 n apart from stream to stream
        a.sync()
        mono = np.ascontiguousarray(x[:, 2])
        b.process(np.stack([mono, mono], axis=2))
        assert a.state_export() == b.state_export()
