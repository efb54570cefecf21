#!/usr/bin/env python3
"""What motion export costs (h264bsdmiSetMotionExport) and what a motion pull costs (h264bsdmiOutputMotionRegions / pull_motion).

--leg decode [--motion]: N instances decode --rounds pictures of the 1080p golden stream through BatchDriver, one tick per round
    (h264bsdmiFlush), motion export off or on, and nothing else — the process to wrap in
        rocprofv3 --kernel-trace --stats -d <dir> -- python tools/motion_bench.py --leg decode [--motion]
    whose kernel statistics give the device time of the tick's kernels; with --motion they hold k_motion_keep beside k_recon_inter,
    without it k_motion_keep must not appear at all.  Prints the wall time per round as one JSON line.
--leg pull: with motion export on, every repetition decodes and pops one more picture per instance, then times (HIP events on a
    torch stream around the call) pull_motion of: the whole window to 640 x 384 letterboxed, NEAREST and AREA; the native grid;
    1,024 seeded boxes to 56 x 56 (AREA) — and pull_regions (k_tensor_roi, bilinear_aa, float16 RGB) for the same boxes and size.
    Prints one JSON line.

usage: motion_bench.py --leg decode|pull [--motion] [--streams 256] [--rounds 24] [--reps 10] [--warmup 2]"""
import argparse
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                    # noqa: E402  (torch's HIP runtime first: capi._share_torch_hip_runtime)
import h264bsd_amd as h                         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--leg", required=True, choices=["decode", "pull"])
ap.add_argument("--motion", action="store_true")
ap.add_argument("--streams", type=int, default=256)
ap.add_argument("--rounds", type=int, default=24)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()

data = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "test_1920x1080.h264"), "rb").read()
N = args.streams
L = h.api_lib()
motion = args.motion or args.leg == "pull"
decs = [h.Decoder(no_output_reordering=1, motion=motion) for _ in range(N)]
rounds = args.rounds if args.leg == "decode" else 5 * (args.warmup + args.reps) + 1
drv = h.BatchDriver(decs, [data * (rounds // 73 + 2)] * N)


def next_round(pop):
    assert len(drv.step()) == N
    assert L.h264bsdmiFlush() == 0
    if pop:
        for d in decs:
            assert d.next_output_info() is not None


if args.leg == "decode":
    next_round(False)                           # the IDR picture, allocations, code object load
    t0 = time.perf_counter()
    for _ in range(args.rounds - 1):
        next_round(False)
    ms = (time.perf_counter() - t0) * 1e3 / (args.rounds - 1)
    print(json.dumps({"leg": "decode", "motion": bool(args.motion), "streams": N, "rounds": args.rounds, "wall_ms_per_round": round(ms, 3),
                      "device_errors": h.device_errors()}))
    sys.exit(0)


def timed(call):
    st = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for rep in range(args.warmup + args.reps):
        next_round(True)
        torch.cuda.synchronize()
        e0.record(st)
        call(st)
        e1.record(st)
        st.synchronize()
        if rep >= args.warmup:
            ms.append(e0.elapsed_time(e1))
    return round(sorted(ms)[len(ms) // 2], 4)


rng = random.Random(1)
boxes = []
for k in range(1024):
    w, hh = rng.randint(64, 400), rng.randint(64, 400)
    boxes.append((k % N, rng.randint(-32, 1920 - w + 32), rng.randint(-32, 1080 - hh + 32), w, hh))
res = {"leg": "pull", "streams": N}
out = torch.empty((N, 3, 384, 640), dtype=torch.float16, device="cuda")
for sampler in ("nearest", "area"):
    res[f"window_640x384_letterbox_{sampler}_ms"] = timed(lambda st: h.pull_motion(decs, size=(384, 640), fit="letterbox", sampler=sampler,
                                                                                   out=out, stream=st))
out = torch.empty((N, 3, 270, 480), dtype=torch.float16, device="cuda")
res["native_grid_ms"] = timed(lambda st: h.pull_motion(decs, out=out, stream=st))
out = torch.empty((len(boxes), 3, 56, 56), dtype=torch.float16, device="cuda")
res["boxes_1024_56x56_area_ms"] = timed(lambda st: h.pull_motion(decs, boxes, 56, sampler="area", out=out, stream=st))
res["boxes_1024_56x56_k_tensor_roi_ms"] = timed(lambda st: h.pull_regions(decs, boxes, 56, mode="bilinear", antialias=True, out=out, stream=st))
res["device_errors"] = h.device_errors()
print(json.dumps(res))
