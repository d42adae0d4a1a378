"""tools/integlog_rate.py — what the integration log (mtr_engine_integlog_set_every; the EVAL instantiations of k_gate, mtr_gate.hip)
costs.  GPU box only.  The programme is the bench step's: 8192 streams x 10 s at 48 kHz (mtr_synth_fill_device kind 1), EBU R128 + true
peak, integration on.

    python tools/integlog_rate.py --step [reps]
the step with the log off — one engine, each step from its call to the end of mtr_engine_sync (the deferred tail included) between
two events on the caller's stream; MTR_LIB names another build of libmtr_engine.so.

    python tools/integlog_rate.py --ab PARENT_LIB [pairs] [reps]
runs --step in alternating child processes, the parent commit's library and this build's, `pairs` times each, and says whether this
build's median lies inside the parent's own min - max of the session.

    python tools/integlog_rate.py [reps]
log off, K = 1 and K = 2, each in both tail modes (1 serial, 2 deferred), taking turns step by step on one buffer, every step from a
reset engine: the whole step as above and the gate's own time (mtr_engine_timing_query: ms_gate).  In the same session the alternative
the log replaces: the engine without the log called 20 times with 24 000 frames and results () after each.

    python tools/integlog_rate.py --long [reps]
long calls, 1 x 3600 s and 64 x 600 s: the log on (K = 1: one workgroup per stream walks the call) against the log off (k_gate_frag +
k_gate_final).
Does not read the reference tree.
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402

FS, S, T = 48000.0, 8192, 480000
WARM = 2


def buffer(torch, M, s=S, t=T):
    buf = torch.empty((s, t, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), s, t, t, 777, FS, 1)
    torch.cuda.synchronize()
    return buf


def one_step(torch, e, buf, t, st, ev0, ev1):
    ev0.record()
    e.process_device(buf.data_ptr(), t, t, st)
    e.sync()                                                           # (the deferred tail included)
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1)


def step(reps):
    import torch
    import meters.lv2_amd as M
    buf = buffer(torch, M)
    st = torch.cuda.current_stream().cuda_stream
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with M.Engine(S, FS, M.METER_EBU | M.METER_TRUEPEAK) as e:
        e.integr_start()
        t = [one_step(torch, e, buf, T, st, ev0, ev1) for _ in range(WARM + reps)][WARM:]
    v = np.asarray(t)
    print("STEP %s median %.3f min %.3f max %.3f" % (os.environ.get("MTR_LIB") or "this build", np.median(v), v.min(), v.max()))


def ab(parent, pairs, reps):
    res = {"parent": [], "this": []}
    for _ in range(pairs):
        for name, lib in (("parent", parent), ("this", None)):
            env = dict(os.environ)
            env.pop("MTR_LIB", None)
            if lib:
                env["MTR_LIB"] = os.path.abspath(lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", str(reps)], env=env, check=True, capture_output=True,
                                 text=True, timeout=300).stdout
            line = [ln for ln in out.splitlines() if ln.startswith("STEP")][0]
            print(name, line, flush=True)
            res[name].append(float(line.split("median")[1].split()[0]))
    p, t = np.asarray(res["parent"]), np.asarray(res["this"])
    inside = p.min() <= np.median(t) <= p.max()
    print("parent medians: median %.3f ms  min %.3f  max %.3f | this build: median %.3f ms  min %.3f  max %.3f | this build's median %s the parent's min - max"
          % (np.median(p), p.min(), p.max(), np.median(t), t.min(), t.max(), "lies inside" if inside else ("is below" if np.median(t) < p.min() else "is ABOVE")))


def report(name, whole, gate):
    w, g = np.asarray(whole), np.asarray(gate)
    print("%-22s step median %7.3f ms  min %7.3f  max %7.3f | ms_gate median %6.3f  min %6.3f  max %6.3f" % (
        name, np.median(w), w.min(), w.max(), np.median(g), g.min(), g.max()), flush=True)
    return float(np.median(w))


def forms(reps):
    import torch
    import meters.lv2_amd as M
    buf = buffer(torch, M)
    st = torch.cuda.current_stream().cuda_stream
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    engines = []
    for tail in (1, 2):
        for K in (0, 1, 2):
            e = M.Engine(S, FS, M.METER_EBU | M.METER_TRUEPEAK)
            e.set_deferred_tail(tail)
            if K:
                e.integlog_set_every(K, T // 24000)
            e.timing_enable(True)
            engines.append(("%s, tail %d" % ("K = %d" % K if K else "log off", tail), K, e))
    whole = {n: [] for n, _, _ in engines}
    gate = {n: [] for n, _, _ in engines}
    poll, CALLS = [], 20
    for it in range(WARM + reps):
        order = engines[it % len(engines):] + engines[:it % len(engines)]      # rotating order
        for name, K, e in order:
            e.reset()
            e.integr_start()
            e.sync()
            ms = one_step(torch, e, buf, T, st, ev0, ev1)
            q = e.timing_query()
            if it >= WARM:
                whole[name].append(ms)
                gate[name].append(q["ms_gate"])
        # the alternative: 20 calls of 24 000 frames, results () after each
        e = engines[0][2]
        e.reset()
        e.integr_start()
        e.sync()
        ev0.record()
        for c in range(CALLS):
            e.process_device(buf.data_ptr() + c * (T // CALLS) * 8, T // CALLS, T, st)
            e.out9()
        ev1.record()
        torch.cuda.synchronize()
        e.timing_query()                                               # (the query sums over the calls since the last one: drain the twenty)
        if it >= WARM:
            poll.append(ev0.elapsed_time(ev1))
    med = {}
    for name, K, e in engines:
        med[name] = report(name, whole[name], gate[name])
        if K:
            il = e.integlog_series(0, 8)
            assert (il["n_points"] == T // 24000 // K).all(), il["n_points"]
        e.close()
    p = np.asarray(poll)
    print("20 calls + results ()  median %7.3f ms  min %7.3f  max %7.3f | %.2f x the one call with K = 1 (tail 1), %.2f x (tail 2)" % (
        np.median(p), p.min(), p.max(), np.median(p) / med["K = 1, tail 1"], np.median(p) / med["K = 1, tail 2"]))


def long_calls(reps):
    import torch
    import meters.lv2_amd as M
    st = torch.cuda.current_stream().cuda_stream
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for s, secs in ((1, 3600), (64, 600)):
        t = int(FS) * secs
        buf = buffer(torch, M, s, t)
        for K in (0, 1):
            with M.Engine(s, FS, M.METER_EBU | M.METER_TRUEPEAK) as e:
                if K:
                    e.integlog_set_every(K, t // 24000)
                e.timing_enable(True)
                whole, gate = [], []
                for it in range(WARM + reps):
                    e.reset()
                    e.integr_start()
                    e.sync()
                    ms = one_step(torch, e, buf, t, st, ev0, ev1)
                    q = e.timing_query()
                    if it >= WARM:
                        whole.append(ms)
                        gate.append(q["ms_gate"])
                report("%d x %d s, %s" % (s, secs, "K = 1" if K else "log off"), whole, gate)
                if K:
                    assert (e.integlog_series()["n_points"] == t // 24000).all()
        del buf


if __name__ == "__main__":
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--ab" in flags:
        ab(args[0], int(args[1]) if len(args) > 1 else 3, int(args[2]) if len(args) > 2 else 9)
    else:
        n = int(args[0]) if args else 9
        step(n) if "--step" in flags else long_calls(n) if "--long" in flags else forms(n)
