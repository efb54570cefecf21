#!/usr/bin/env python3
"""What region statistics cost (h264bsdmiOutputRegionStats / pull_stats) beside what a caller does without them.

N instances decode the 1080p golden stream through BatchDriver; every repetition decodes one more picture per instance, then times
(HIP events on a torch stream around the work, the median over --reps):
  stats_<source>_bins<B>_ms     pull_stats of the N whole windows, source y / ycbcr / rgb, bins 0 and 256 (the pictures were popped
                                with h264bsdmiNextOutputInfo: nothing is pulled);
  boxes_1024_<source>_ms        pull_stats of 1,024 seeded detector-sized boxes, bins 256;
  torch_<channels>_pull_ms      the same answers without the call: a full-size pull_tensor (uint8, channels "Y" / "RGB", which pops
  torch_<channels>_sums_ms      the pictures), then sums, sums of squares, minima and maxima in torch,
  torch_<channels>_histc_ms     then torch.histc per picture and channel (torch has no batched histogram).
Also the bytes the statistics kernel reads per call and the read rate that makes.  Prints one JSON line.

usage: stats_bench.py [--streams 256] [--reps 10] [--warmup 2]"""
import argparse
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                    # noqa: E402  (torch's HIP runtime first: capi._share_torch_hip_runtime)
import h264bsd_amd as h                         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=256)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()

data = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "test_1920x1080.h264"), "rb").read()
N = args.streams
L = h.api_lib()
decs = [h.Decoder(no_output_reordering=1) for _ in range(N)]
LEGS = 6 + 3 + 2                               # the timed calls that decode a picture per repetition
rounds = LEGS * (args.warmup + args.reps) + 1
drv = h.BatchDriver(decs, [data * (rounds // 73 + 2)] * N)


def next_round(pop):
    assert len(drv.step()) == N
    assert L.h264bsdmiFlush() == 0
    if pop:
        for d in decs:
            assert d.next_output_info() is not None


def timed(call, pop=True, decode=True):
    st = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for rep in range(args.warmup + args.reps):
        if decode:
            next_round(pop)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            e0.record(st)
            call(st)
            e1.record(st)
        st.synchronize()
        if rep >= args.warmup:
            ms.append(e0.elapsed_time(e1))
    return round(sorted(ms)[len(ms) // 2], 4)


res = {"streams": N}
mbs = 120 * 68 * N
for source in ("y", "ycbcr", "rgb"):
    for bins in (0, 256):
        out = torch.empty((N, h.stats_record_bytes(source, bins)), dtype=torch.uint8, device="cuda")
        ms = timed(lambda st: h.pull_stats(decs, None, source=source, bins=bins, out=out, stream=st))
        res[f"stats_{source}_bins{bins}_ms"] = ms
        read = mbs * (256 if source == "y" else 384)
        res[f"stats_{source}_bins{bins}_read_GBps"] = round(read / ms / 1e6, 1)
rng = random.Random(1)
boxes = []
for k in range(1024):
    w, hh = rng.randint(64, 400), rng.randint(64, 400)
    boxes.append((k % N, rng.randint(-32, 1920 - w + 32), rng.randint(-32, 1080 - hh + 32), w, hh))
for source in ("y", "ycbcr", "rgb"):
    out = torch.empty((1024, h.stats_record_bytes(source, 256)), dtype=torch.uint8, device="cuda")
    res[f"boxes_1024_{source}_ms"] = timed(lambda st: h.pull_stats(decs, boxes, source=source, bins=256, out=out, stream=st))

# what a caller does today: the pictures as a uint8 tensor, then torch
for channels in ("Y", "RGB"):
    C = 1 if channels == "Y" else 3
    t = torch.empty((N, C, 1080, 1920), dtype=torch.uint8, device="cuda")
    res[f"torch_{channels}_pull_ms"] = timed(lambda st: h.pull_tensor(decs, dtype=torch.uint8, channels=channels, out=t, stream=st), pop=False)

    def sums(st):
        v = t.view(N, C, -1)
        f = v.to(torch.int32)
        return v.sum(2, dtype=torch.int64), (f * f).sum(2, dtype=torch.int64), v.amin(2), v.amax(2)

    def histc(st):
        return [torch.histc(t[i, c].float(), bins=256, min=0, max=256) for i in range(N) for c in range(C)]

    res[f"torch_{channels}_sums_ms"] = timed(sums, decode=False)
    res[f"torch_{channels}_histc_ms"] = timed(histc, decode=False)
res["device_errors"] = h.device_errors()
print(json.dumps(res))
