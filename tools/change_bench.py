#!/usr/bin/env python3
"""What kept pictures and change statistics cost (h264bsdmiKeepCurrentPictures / keep_pictures, h264bsdmiOutputRegionChange /
pull_change) beside what a caller does without them.

N instances decode the 1080p golden stream through BatchDriver and keep their first picture; every repetition decodes one more
picture per instance, then times (HIP events on a torch stream around the work, the median over --reps):
  keep_ms                        keep_pictures of the N current pictures alone (one k_keep launch);
  change_<source>_bins<B>_ms     pull_change of the N whole windows against the kept pictures: y without a histogram, y, ycbcr and
                                 rgb with 256 bins;
  same_<source>_bins256_ms       the same call right after a keep, without decoding: the two pictures are equal and every sample
                                 lands in bin 0, what a static camera gives all day;
  stats_<source>_bins<B>_ms      pull_stats on the same pictures: one tile stream instead of two;
  torch_<channels>_pull_ms       the same answers without the call: the previous full-size pull_tensor result retained (uint8, channels
  torch_<channels>_diff_ms       "Y" / "RGB"), a new one pulled, then the difference and its sums, maximum and count above a
  torch_<channels>_histc_ms      threshold in torch, then torch.histc per picture and channel (torch has no batched histogram).
Also the bytes the change kernel reads per call (both frames once) and the read rate that makes.  Prints one JSON line.

usage: change_bench.py [--streams 256] [--reps 10] [--warmup 2]"""
import argparse
import json
import os
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
VARIANTS = (("y", 0), ("y", 256), ("ycbcr", 256), ("rgb", 256))
LEGS = 1 + len(VARIANTS) + 2                   # the timed calls that decode a picture per repetition
rounds = LEGS * (args.warmup + args.reps) + 4
drv = h.BatchDriver(decs, [data * (rounds // 73 + 2)] * N)


def next_round(pop):
    assert len(drv.step()) == N
    assert L.h264bsdmiFlush() == 0
    if pop:
        for d in decs:
            assert d.next_output_info() is not None


def timed(call, pop=True, decode=True, before=None):
    st = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for rep in range(args.warmup + args.reps):
        if decode:
            next_round(pop)
        if before:
            before()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            e0.record(st)
            call(st)
            e1.record(st)
        st.synchronize()
        if rep >= args.warmup:
            ms.append(e0.elapsed_time(e1))
    return round(sorted(ms)[len(ms) // 2], 4)


res = {"streams": N, "variant": os.environ.get("H264BSD_VARIANT", "")}
mbs = 120 * 68 * N
next_round(True)
assert h.keep_pictures(decs)[0] == [1] * N
res["keep_ms"] = timed(lambda st: h.keep_pictures(decs, stream=st))
res["keep_GBps"] = round(2 * mbs * 384 / res["keep_ms"] / 1e6, 1)      # read + written
for source, bins in VARIANTS:
    out = torch.empty((N, h.change_record_bytes(source, bins)), dtype=torch.uint8, device="cuda")
    ms = timed(lambda st: h.pull_change(decs, None, source=source, bins=bins, threshold=8, out=out, stream=st))
    res[f"change_{source}_bins{bins}_ms"] = ms
    res[f"change_{source}_bins{bins}_read_GBps"] = round(2 * mbs * (256 if source == "y" else 384) / ms / 1e6, 1)
    sout = torch.empty((N, h.stats_record_bytes(source, bins)), dtype=torch.uint8, device="cuda")
    res[f"stats_{source}_bins{bins}_ms"] = timed(lambda st: h.pull_stats(decs, None, source=source, bins=bins, out=sout, stream=st), decode=False)
    if bins:
        res[f"same_{source}_bins{bins}_ms"] = timed(lambda st: h.pull_change(decs, None, source=source, bins=bins, threshold=8, out=out, stream=st),
                                                    decode=False, before=lambda: h.keep_pictures(decs))
        first = h.RegionChange(out.cpu(), 1 if source == "y" else 3, bins, [], [], [], [], [])
        assert not first.sad.any() and bool((first.hist[:, :, 0] == first.count[:, None]).all())

# what a caller does today: the previous pictures retained as a uint8 tensor, the new ones pulled, then torch
for channels in ("Y", "RGB"):
    C = 1 if channels == "Y" else 3
    prev = torch.empty((N, C, 1080, 1920), dtype=torch.uint8, device="cuda")
    t = torch.empty((N, C, 1080, 1920), dtype=torch.uint8, device="cuda")
    next_round(False)
    h.pull_tensor(decs, dtype=torch.uint8, channels=channels, out=prev)
    torch.cuda.synchronize()
    res[f"torch_{channels}_pull_ms"] = timed(lambda st: h.pull_tensor(decs, dtype=torch.uint8, channels=channels, out=t, stream=st), pop=False)
    state = {}

    def diff(st):
        d = t.view(N, C, -1).to(torch.int16) - prev.view(N, C, -1).to(torch.int16)
        a = d.abs()
        f = a.to(torch.int32)
        state["a"] = a
        return a.sum(2, dtype=torch.int64), (f * f).sum(2, dtype=torch.int64), d.sum(2, dtype=torch.int64), a.amax(2), (a > 8).sum(2)

    def histc(st):
        a = state["a"]
        return [torch.histc(a[i, c].float(), bins=256, min=0, max=256) for i in range(N) for c in range(C)]

    res[f"torch_{channels}_diff_ms"] = timed(diff, decode=False)
    res[f"torch_{channels}_histc_ms"] = timed(histc, decode=False)
    del prev, t, state
res["device_errors"] = h.device_errors()
print(json.dumps(res))
