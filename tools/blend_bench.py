#!/usr/bin/env python3
"""What the background model costs (h264bsdmiBlendCurrentPictures / blend_pictures) beside a plain keep (keep_pictures) and beside the
same update done in torch on retained full-size pulls.

N instances decode the 1080p golden stream through BatchDriver and start their models; every repetition decodes one more picture per
instance, then times the calls one after the other, in an order that alternates from repetition to repetition (HIP events on a torch
stream around each call; median, minimum and maximum over --reps):
  keep_ms            keep_pictures of the N current pictures (one k_keep launch: 2 frame sizes of traffic);
  blend_ms           blend_pictures(shift=4) into models whose fraction is valid (one k_blend launch: 5 frame sizes — an untimed blend
                     goes ahead of every timed one, because a keep resets the fraction and the blend behind it reads 4);
  blend_gated_ms     the same with hold=12, moving_shift="frozen" and count_moving: the hold mask, the counters and their zeroing;
  blend_after_keep_ms  the blend right behind a keep (4 frame sizes);
  torch_pull_ms      pull_regions of the N current pictures' whole windows as uint8 luma [N, 1, 1080, 1920], what a caller has to do
                     first today;
  torch_update_ms    the update of section "Background model" in torch on a retained int32 state of those LUMA tensors alone (two
                     thirds of the samples of the frame, no chroma gate), hold mask included.
Also blend_ms / keep_ms and the rates the byte counts give.  Prints one JSON line.

usage: blend_bench.py [--streams 256] [--reps 15] [--warmup 3]"""
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


def timed(call, prime=None):
    if prime:
        prime()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(st):
        e0.record(st)
        call()
        e1.record(st)
    st.synchronize()
    return e0.elapsed_time(e1)


Y = torch.empty((N, 1, 1080, 1920), dtype=torch.uint8, device="cuda")
WINDOWS = [(i, 0, 0, 1920, 1080) for i in range(N)]
S = None


def torch_update(shift=4, hold=12):
    """S' = S + ((T - S + 2^(k-1)) >> k) where still, S where moving (frozen), on the luma tensors"""
    global S
    T = Y.to(torch.int32) * 256 + 128
    if S is None:
        S = T
        return
    moving = (Y.to(torch.int16) - (S >> 8).to(torch.int16)).abs() > hold
    S = torch.where(moving, S, S + ((T - S + (1 << (shift - 1))) >> shift))


prime = lambda: h.blend_pictures(decs, shift=4)
LEGS = {
    "keep_ms": (lambda: h.keep_pictures(decs, stream=st), None),
    "blend_ms": (lambda: h.blend_pictures(decs, shift=4, stream=st), prime),
    "blend_gated_ms": (lambda: h.blend_pictures(decs, shift=4, hold=12, moving_shift="frozen", count_moving=True, stream=st), prime),
    "blend_after_keep_ms": (lambda: h.blend_pictures(decs, shift=4, stream=st), lambda: h.keep_pictures(decs)),
    "torch_pull_ms": (lambda: h.pull_regions(decs, WINDOWS, (1080, 1920), dtype=torch.uint8, channels="Y", out=Y, stream=st), None),
    "torch_update_ms": (torch_update, None),
}
times = {k: [] for k in LEGS}
next_round()
assert h.blend_pictures(decs)[:2] == ([1] * N, [0] * N)
for rep in range(args.warmup + args.reps):
    next_round()
    first = [k for k in LEGS if not k.startswith("torch")]
    order = (first if rep % 2 == 0 else first[::-1]) + ["torch_pull_ms", "torch_update_ms"]
    for k in order:
        ms = timed(*LEGS[k])
        if rep >= args.warmup:
            times[k].append(ms)

res = {"streams": N, "reps": args.reps, "variant": os.environ.get("H264BSD_VARIANT", "")}
frame = 120 * 68 * 384 * N
for k, v in times.items():
    v = sorted(v)
    res[k] = round(v[len(v) // 2], 4)
    res[k.replace("_ms", "_min_max_ms")] = [round(v[0], 4), round(v[-1], 4)]
res["blend_over_keep"] = round(res["blend_ms"] / res["keep_ms"], 3)
res["keep_GBps"] = round(2 * frame / res["keep_ms"] / 1e6, 1)
res["blend_GBps"] = round(5 * frame / res["blend_ms"] / 1e6, 1)
res["blend_after_keep_GBps"] = round(4 * frame / res["blend_after_keep_ms"] / 1e6, 1)
res["device_errors"] = h.device_errors()
print(json.dumps(res))
