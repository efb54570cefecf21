#!/usr/bin/env python3
"""What the region shift costs (h264bsdmiOutputRegionShift / pull_shift) beside what a caller does without it.

N instances decode the 1080p golden stream through BatchDriver, keep their first picture and pop their second; every timed call then
searches the kept picture in the current one (HIP events on a torch stream around the work; per figure [median, min, max] in ms over
--reps after --warmup calls of the same shape; the 2 N frames of a call are 1.6 GB at N = 256, far beyond the caches, so repeating a
call on the same pictures does not flatter it):
  shift_r<R>_ms, shift_r<R>_surface_ms   pull_shift of the N whole windows at each of --radii, without and with the surface;
  shift_boxes_r8_ms                      4096 boxes of 64 x 64 spread over the instances, radius 8, one call;
  change_y_ms                            pull_change, luma, no histogram, of the same whole windows: it reads the same two pictures
                                         once and is the floor for radius 0;
  torch_pull_ms                          the full-size luma pull a caller needs per picture (pull_regions of the whole windows at
                                         scale 1, which pops nothing; the previous picture's is retained);
  torch_r<R>_ms                          then, in torch: replicate padding, (2R+1)^2 sliced |a - b|.sum() reductions and the argmin
                                         under the call's tie rule, over --torch-reps; its surface and answer are first checked EQUAL
                                         to the kernel's.
--kernel-only leaves torch out: the figure to compare between libraries built with another inner loop (tools/experiments/
shift_inner_loops.patch applied, then -DSHIFT_INNER=1 / 2 through tools/experiments/build_variant.sh, chosen with H264BSD_VARIANT).  Prints one JSON line.

usage: shift_bench.py [--streams 256] [--reps 10] [--warmup 2] [--torch-reps 3] [--radii 0,2,4,8,16] [--kernel-only]"""
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
ap.add_argument("--torch-reps", type=int, default=3)
ap.add_argument("--radii", default="0,2,4,8,16")
ap.add_argument("--kernel-only", action="store_true")
args = ap.parse_args()
radii = [int(r) for r in args.radii.split(",")]

data = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "test_1920x1080.h264"), "rb").read()
N, W, H = args.streams, 1920, 1080
L = h.api_lib()
decs = [h.Decoder(no_output_reordering=1) for _ in range(N)]
drv = h.BatchDriver(decs, [data] * N)


def next_round():
    assert len(drv.step()) == N
    assert L.h264bsdmiFlush() == 0
    for d in decs:
        assert d.next_output_info() is not None


def timed(call, reps):
    st = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for rep in range(args.warmup + reps):
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            e0.record(st)
            call(st)
            e1.record(st)
        st.synchronize()
        if rep >= args.warmup:
            ms.append(e0.elapsed_time(e1))
    ms.sort()
    return [round(ms[len(ms) // 2], 4), round(ms[0], 4), round(ms[-1], 4)]


WHOLE = [(i, 0, 0, W, H) for i in range(N)]
res = {"streams": N, "variant": os.environ.get("H264BSD_VARIANT", ""), "reps": args.reps, "torch_reps": args.torch_reps}
next_round()
prev = None
if not args.kernel_only:
    prev = h.pull_regions(decs, WHOLE, (H, W), dtype=torch.uint8, channels="Y")[0]
assert h.keep_pictures(decs)[0] == [1] * N
next_round()
next_round()                                    # two pictures on: more than noise between them

records = {}
for R in radii:
    for surface in (False, True):
        out = torch.empty((N, h.shift_record_bytes(R, surface)), dtype=torch.uint8, device="cuda")
        res[f"shift_r{R}{'_surface' if surface else ''}_ms"] = timed(lambda st: h.pull_shift(decs, None, radius=R, surface=surface, out=out, stream=st), args.reps)
        if surface:
            records[R] = h.pull_shift(decs, None, radius=R, surface=True, out=out)
            torch.cuda.synchronize()
boxes = [(k % N, 64 * ((k // N) % 29), 64 * ((k // (29 * N)) % 16) + 7, 64, 64) for k in range(4096)]
out = torch.empty((4096, h.shift_record_bytes(8, False)), dtype=torch.uint8, device="cuda")
res["shift_boxes_r8_ms"] = timed(lambda st: h.pull_shift(decs, boxes, radius=8, out=out, stream=st), args.reps)
cout = torch.empty((N, h.change_record_bytes("y", 0)), dtype=torch.uint8, device="cuda")
res["change_y_ms"] = timed(lambda st: h.pull_change(decs, None, source="y", bins=0, out=cout, stream=st), args.reps)
ch = h.pull_change(decs, None, source="y", bins=0, out=cout)
for R, sh in records.items():
    assert bool((sh.still.long() & 0xFFFFFFFF == ch.sad[:, 0]).all()), R      # SAD(0, 0) is the sibling's luma sad
if radii and 0 in radii:
    res["r0_over_change"] = round(res["shift_r0_ms"][0] / res["change_y_ms"][0], 2)

if not args.kernel_only:
    cur = torch.empty((N, 1, H, W), dtype=torch.uint8, device="cuda")
    res["torch_pull_ms"] = timed(lambda st: h.pull_regions(decs, WHOLE, (H, W), dtype=torch.uint8, channels="Y", out=cur, stream=st), args.reps)
    kept16 = None

    def search(R):
        """[N, D, D] int64 SADs, then (dx, dy) under the tie rule"""
        D = 2 * R + 1
        pad = torch.nn.functional.pad(cur.float(), (R, R, R, R), mode="replicate").to(torch.int16)
        sad = torch.empty((N, D, D), dtype=torch.int64, device="cuda")
        for dy in range(D):
            for dx in range(D):
                sad[:, dy, dx] = (kept16 - pad[:, :, dy:dy + H, dx:dx + W]).abs().sum((1, 2, 3), dtype=torch.int64)
        off = torch.arange(-R, R + 1, device="cuda")
        rank = ((off[:, None] ** 2 + off[None, :] ** 2) * 4096 + (off[:, None] + R) * 64 + (off[None, :] + R)).view(1, -1)
        at = (sad.view(N, -1) * (1 << 22) + rank).argmin(1)
        return sad, at % D - R, at // D - R

    kept16 = prev.to(torch.int16)
    for R in radii:
        sad, dx, dy = search(R)
        sh = records[R]
        assert bool((sh.surface.long() & 0xFFFFFFFF == sad).all()), R
        assert bool((sh.dx == dx).all()) and bool((sh.dy == dy).all()), R
        res[f"torch_r{R}_ms"] = timed(lambda st: search(R), args.torch_reps)
res["device_errors"] = h.device_errors()
print(json.dumps(res))
