#!/usr/bin/env python3
"""What the background spread costs (h264bsdmiBlendCurrentPicturesSpread / blend_pictures(spread=...)) beside the plain blend, and the
SPREAD mode of the cell maps beside their CHANGE mode.

N instances decode the 1080p golden stream through BatchDriver and start their models with a spread blend; every repetition decodes one
more picture per instance, then times the calls one after the other, in an order that alternates from repetition to repetition (HIP
events on a torch stream around each call; median, minimum and maximum over --reps):
  blend_ms           blend_pictures(shift=4, hold=12) into models whose fraction is valid: one k_blend launch, 5 frame sizes of traffic
                     (k_blend is the kernel of the commit before this feature, unchanged: the baseline, taken in the same process);
  spread_all_ms      the same with spread=dict(update="all"): one k_blend_spread launch, 7 frame sizes;
  spread_still_ms    update="still": the same traffic, the step under the moving mask;
  spread_none_ms     update="none": the luma of V is read and nothing of it written, 5 + 2/3 frame sizes (6 is the bound that counts
                     the chroma of V as read);
  cells_above_ms     pull_cells(cell=16, planes="above", against="kept") of the N whole windows: two frames read;
  cells_fore_ms      pull_cells(cell=16, planes="fore", against="spread") on the same grid: three frames read.
Also the ratios to blend_ms and to cells_above_ms with what the bytes predict, and the rates.  Prints one JSON line.

usage: spread_bench.py [--streams 256] [--reps 15] [--warmup 3]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                    # noqa: E402  (torch's HIP runtime first: capi._share_torch_hip_runtime)
import h264bsd_amd as h                         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=256)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()

data = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "test_1920x1080.h264"), "rb").read()
N = args.streams
L = h.api_lib()
decs = [h.Decoder(no_output_reordering=1) for _ in range(N)]
rounds = args.warmup + args.reps + 4
drv = h.BatchDriver(decs, [data * (rounds // 73 + 2)] * N)
st = torch.cuda.Stream()


def next_round():
    assert len(drv.step()) == N
    assert L.h264bsdmiFlush() == 0
    for d in decs:
        assert d.next_output_info() is not None


def timed(call):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(st):
        e0.record(st)
        call()
        e1.record(st)
    st.synchronize()
    return e0.elapsed_time(e1)


def spread(update):
    return dict(gain=2, lowest=2, highest=255, update=update)


GRID = (68, 120)
maps = torch.empty((N, 1, GRID[0], GRID[1]), dtype=torch.int32, device="cuda")
BLEND = dict(shift=4, hold=12, stream=st)
LEGS = {
    "blend_ms": lambda: h.blend_pictures(decs, **BLEND),
    "spread_all_ms": lambda: h.blend_pictures(decs, spread=spread("all"), **BLEND),
    "spread_still_ms": lambda: h.blend_pictures(decs, spread=spread("still"), **BLEND),
    "spread_none_ms": lambda: h.blend_pictures(decs, spread=spread("none"), **BLEND),
    "cells_above_ms": lambda: h.pull_cells(decs, None, cell=16, grid=GRID, planes=("above",), against="kept", threshold=4, out=maps, stream=st),
    "cells_fore_ms": lambda: h.pull_cells(decs, None, cell=16, grid=GRID, planes=("fore",), against="spread", threshold=4, out=maps, stream=st),
}
times = {k: [] for k in LEGS}
next_round()
assert h.blend_pictures(decs, spread=spread("all"))[:2] == ([1] * N, [0] * N)
for rep in range(args.warmup + args.reps):
    next_round()
    order = list(LEGS) if rep % 2 == 0 else list(LEGS)[::-1]
    for k in order:
        ms = timed(LEGS[k])
        if rep >= args.warmup:
            times[k].append(ms)

res = {"streams": N, "reps": args.reps, "variant": os.environ.get("H264BSD_VARIANT", "")}
frame = 120 * 68 * 384 * N
for k, v in times.items():
    v = sorted(v)
    res[k] = round(v[len(v) // 2], 4)
    res[k.replace("_ms", "_min_max_ms")] = [round(v[0], 4), round(v[-1], 4)]
for k, predicted in (("spread_all", 7 / 5), ("spread_still", 7 / 5), ("spread_none", 6 / 5)):
    res[k + "_over_blend"] = round(res[k + "_ms"] / res["blend_ms"], 3)
    res[k + "_over_blend_by_bytes"] = round(predicted, 3)
res["fore_over_above"] = round(res["cells_fore_ms"] / res["cells_above_ms"], 3)
res["fore_over_above_by_bytes"] = 1.5
res["blend_GBps"] = round(5 * frame / res["blend_ms"] / 1e6, 1)
res["spread_all_GBps"] = round(7 * frame / res["spread_all_ms"] / 1e6, 1)
res["cells_above_GBps"] = round(2 * frame * 2 / 3 / res["cells_above_ms"] / 1e6, 1)      # source "y": the luma of the frames
res["cells_fore_GBps"] = round(3 * frame * 2 / 3 / res["cells_fore_ms"] / 1e6, 1)
res["device_errors"] = h.device_errors()
print(json.dumps(res))
