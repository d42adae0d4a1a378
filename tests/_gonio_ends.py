"""The yardstick of the goniometer's track lengths (include/mtr_gonio_ends.h; tests/test_gonio_ends_cpu.py, tests/test_gpu_gonio_ends.py): the
restatement of tests/_gonio.py for a batch of tracks of unequal length.

What the reference does at a track's end: goniometer_run (src/goniometerlv2.c:145-186) fills the ring, draw_rb (gui/goniometer.c:299-538)
takes whatever the ring holds (:301) and returns at n_samples < 64 (:302).  A host that stops calling run () at the track's end and exposes
the display once more gets one last draw_rb of the r frames the track has of its open display update — or none, if r < 64.

One lock-step pass of _gonio.Gonio over the whole batch; per stream, at the frame where it comes to stand, its state, image and counters
are snapshot and the closing draw_rb of r frames is applied to the snapshot: _gonio.Gonio._block_end with rms_c = r and the attack pair of
elapsed = r / rate (libm through ctypes, as _gonio.derive takes the block's).  Nothing is applied for r < 64.

Where a stream comes to stand depends on how the audio is cut into calls, because the engine cannot un-draw: with E its end, `start` the
first frame of the call that closes it (the call with start <= E < start + n) and r = E mod P,
    E == start          nothing of it changes in that call: it stands at E, whatever r is, with everything earlier calls drew (frames[s] = 0)
    r == 0              it stands at E, behind a whole update
    r >= 64             it stands at E, behind a closing update of r frames
    0 < r < 64          it stands at max (E - r, start): behind its last whole update, but not in front of the closing call"""
import copy

import numpy as np

import _gonio

F32 = np.float32
FLOOR = 64                                   # draw_rb's `n_samples < 64` return (:302)
STATE = ("lp0", "lp1", "last_x", "last_y", "gain", "xmax", "xmin", "ymax", "ymin", "rms0", "rms1", "bd", "bc", "drawn", "clipped", "skipped")


def cut(fill, P, n_frames, E):
    """what mtr_gonio_cut answers but for the attack pair: (whole, closing_frames, drawn_frames) of a stream that takes E frames of a call
    of n_frames which starts `fill` frames into a display update of P"""
    assert 0 <= fill < P and 0 <= E <= n_frames
    tot = fill + E
    whole, r = tot // P, tot % P
    if not 0 < E < n_frames or r == 0:
        return whole, 0, E
    if r < FLOOR:
        return whole, 0, E - min(E, r)
    return whole, r, E


def attack(rate, r, dials=_gonio.DIALS):
    """the closing update's attack pair: `attack` of :524 for elapsed = (float) ((size_t) r / rate)"""
    return _gonio.derive(rate, P=r, dials=dials).attack


def stand(E, T, P, calls):
    """(where the stream comes to stand, r of its closing update or 0) for a track of E frames in a batch of T, cut into `calls`"""
    if E >= T:
        return T, 0
    start = 0
    for n in calls:
        if start <= E < start + n:
            break
        start += n
    r = E % P
    if E == start or r == 0:
        return E, 0
    if r < FLOOR:
        return max(E - r, start), 0
    return E, r


class Ends:
    """the batch behind its tracks' ends: img [S, G, G], drawn / clipped / skipped [S], gain / lp0 / lp1 / last_x / last_y [S], the open
    block's accumulators, the series as three [S, blocks] arrays (0 behind a stream's own points), updates [S], and the guard's notes"""


def run(x, ends, rate, calls=None, **kw):
    """x float32 [S, T, 2], ends [S] in 0 .. T (T: the stream stays open), calls: the lengths the audio is cut into (None: one call)"""
    x = np.asarray(x, F32)
    S, T = x.shape[0], x.shape[1]
    calls = list(calls) if calls else [T]
    assert sum(calls) == T and len(ends) == S
    g = _gonio.Gonio(S, rate, **kw)
    P = g.d.P
    at = [stand(int(E), T, P, calls) for E in ends]
    o = Ends()
    o.P, o.T, o.blocks = P, T, T // P
    o.img = np.zeros_like(g.img)
    for k in STATE:
        setattr(o, k, np.zeros_like(getattr(g, k)))
    o.s_gain, o.s_drawn, o.s_clipped = np.zeros((S, o.blocks), F32), np.zeros((S, o.blocks), np.uint32), np.zeros((S, o.blocks), np.uint32)
    o.updates = np.zeros(S, np.uint64)
    o.stand = np.array([a[0] for a in at])
    o.r = np.array([a[1] for a in at])
    o.tail = np.array([int(E) % P if int(E) < T else 0 for E in ends])          # the frames the track has of its open update
    o.moved, o.painted = np.zeros(S, bool), np.zeros(S, bool)                    # the closing update moved the gain / painted
    pos = 0
    for t in sorted(set(o.stand.tolist())):
        g.run(x[:, pos:t])
        pos = t
        idx = np.nonzero(o.stand == t)[0]
        whole = len(g.series)
        for k in STATE:
            getattr(o, k)[idx] = getattr(g, k)[idx]
        o.img[idx] = g.img[idx]
        for b in range(min(whole, o.blocks)):
            o.s_gain[idx, b], o.s_drawn[idx, b], o.s_clipped[idx, b] = g.series[b][0][idx], g.series[b][1][idx], g.series[b][2][idx]
        o.updates[idx] = whole
        cl = idx[o.r[idx] > 0]
        if cl.size:                                                              # (one r per t: r = t mod P)
            r = int(o.r[cl[0]])
            assert (o.r[cl] == r).all() and r >= FLOOR
            h = _gonio.Gonio(cl.size, rate, **kw)
            for k in STATE:
                setattr(h, k, getattr(o, k)[cl].copy())
            h.d = copy.copy(g.d)
            h.d.P, h.d.attack = r, attack(rate, r, kw.get("dials", _gonio.DIALS))
            before = h.gain.copy()
            with np.errstate(all="ignore"):
                h._block_end()                                                   # :494-536 with n_samples = r
            pg, pd, pc = h.series[-1]
            o.moved[cl] = pg.view(np.uint32) != before.view(np.uint32)
            o.painted[cl] = pd > 0
            for k in STATE:
                getattr(o, k)[cl] = getattr(h, k)
            if whole < o.blocks:
                o.s_gain[cl, whole], o.s_drawn[cl, whole], o.s_clipped[cl, whole] = pg, pd, pc
            o.updates[cl] += 1
    return o                                                                     # (behind the last stand nothing is drawn any more)


def planted_ends(S, T, P, seed=11):
    """[S] uint64 for batches of 67 streams and more, T >= 2048 + P: the edges — T (open), 0, 1, 63, 64, P (r = 0), P + 63, P + 64, 2 P - 1, 128,
    1024, 2048, 1025, T - 1 — and seeded random ends for the rest, arranged by workgroups of 16 lanes: streams 0 .. 15 hold open, closing
    and long-closed lanes together; streams 16 .. 31 all end at or before frame 2048 (the call's third piece of 1024 never sees them)"""
    assert S >= 67 and T >= 2048 + P
    r = np.random.default_rng(seed)
    e = r.integers(0, T + 1, S).astype(np.uint64)
    # (P - 100 and P - 80: r = 0 and 0 < r < 64 where a dense call of 100 frames went in front)
    e[0:16] = [T, 5, T - 1, T, P - 100, 2500, T, 1, 3000 + FLOOR, T, 0, 4000, T, P - 80, T, 64]
    e[16:32] = [0, 1, 63, 64, P, P + 63, P + 64, 2 * P - 1, 128, 1024, 2048, 1025, 3 * P, 2 * P + 200, 777, 1500]
    e[64:67] = [T, 2 * P + 100, 1024 + P]
    return e


def coverage_ends(o, autogain):
    """the guard, on the restatement alone: the ends meet every rule, and the signal set every rule of _gonio.coverage"""
    closing = o.stand < o.T
    assert (closing & (o.r >= FLOOR) & o.painted).any(), "no closing stream painted in its closing update"
    if autogain:
        assert (closing & (o.r >= FLOOR) & o.moved).any(), "no closing update moved the gain"
    assert (closing & (o.tail > 0) & (o.tail < FLOOR)).any(), "no closing stream with 0 < r < 64"
    assert (closing & (o.tail == 0) & (o.stand > 0)).any(), "no stream ends with r = 0"
    _gonio.coverage(o, o.T)
