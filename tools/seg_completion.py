"""tools/seg_completion.py [-s SEGMENTS] [streams] [kinds...] — the share of k_seg's screened chunks that complete (mtr_engine_refine_stats) on the
bench's shape: `streams` x 10 s at 48 kHz of bench.py's synthesis (kind 1 programme, 0 stationary noise, 2 rising level), EBU R128 +
true peak, one call, the planner's own layout and segmentation (-s: layout 7 with that many segments per stream).  MTR_LIB selects
another build of the library."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import meters.lv2_amd as M

args = sys.argv[1:]
tune = {}
if args[:1] == ["-s"]:
    tune = dict(tune_segments=int(args[1]), tune_layout=7)
    args = args[2:]
S = int(args[0]) if args else 8192
kinds = [int(k) for k in args[1:]] or [1, 0, 2]
T, fs = 480000, 48000.0
buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
st = torch.cuda.current_stream().cuda_stream
for kind in kinds:
    M.synth_fill_device(buf.data_ptr(), S, T, T, 777, fs, kind, st)
    with M.Engine(S, fs, M.METER_EBU | M.METER_TRUEPEAK, **tune) as e:
        e.integr_start()
        e.process_device(buf.data_ptr(), T, T, st)
        torch.cuda.synchronize()
        scr, fin = e.refine_stats()
        print("signal %d: streams %d chunks screened %d completed %d rate %.4f (k_seg calls %d)" % (kind, S, scr, fin, fin / max(scr, 1), e.seg_stats()[0]))
