#!/usr/bin/env python3
"""What warping the kept pictures costs (h264bsdmiWarpKeptPictures / warp_kept) beside the two calls that write kept pictures and the
route a caller had without it.

N instances decode the 1080p golden stream through BatchDriver and pop a picture.  The timed calls (HIP events on a torch stream around
the work; per figure [median, min, max] in ms over --reps after --warmup calls of the same shape), all over the N whole pictures:
  keep_ms, blend_ms                    keep_pictures and blend_pictures(shift=4, hold=24): they move 2 and 5 frame sizes;
  warp_<map>_<lo>_<outside>_ms         warp_kept; map = identity, near (1 degree, 1 % zoom and an (8, 5) shift about the centre: what
                                       stabilisation asks for) and quarter (a quarter turn about the centre); lo = hi (after a plain
                                       keep: the picture alone) or hilo (after blends: picture and fraction); outside = replicate or
                                       current.  It moves 2 to 4 frame sizes (hi, lo in and out), the current picture's where the
                                       source was outside, and the halo of the blocks;
  outside_<map>                        the mean share of a window's luma samples whose source was outside;
  grid_sample_<map>_ms                 (not with --kernel-only) for orientation: torch.nn.functional.grid_sample (bilinear, border) of a
                                       RETAINED float16 tensor [N, 3, 1080, 1920] — what a full-size pull_tensor leaves — through the
                                       same map, in chunks of 32 pictures.  It cannot write the result back into the kept pictures,
                                       which is the point of the call.
H264BSD_VARIANT=<name> runs a library built by tools/experiments/build_variant.sh (how the kernel with and without its LDS staging
were compared: docs/EXPERIMENTS.md, "Warped kept pictures").  Prints one JSON line.

usage: warp_bench.py [--streams 256] [--reps 20] [--warmup 2] [--kernel-only]"""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                    # noqa: E402  (torch's HIP runtime first: capi._share_torch_hip_runtime)
import h264bsd_amd as h                         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=256)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--kernel-only", action="store_true")
args = ap.parse_args()

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


def timed(call, reps, warmup):
    st = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for rep in range(warmup + reps):
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            e0.record(st)
            call(st)
            e1.record(st)
        st.synchronize()
        if rep >= warmup:
            ms.append(e0.elapsed_time(e1))
    ms.sort()
    return [round(ms[len(ms) // 2], 4), round(ms[0], 4), round(ms[-1], 4)]


def about_the_centre(a, b, d, e, dx=0.0, dy=0.0):
    """the transform kept -> current that keeps the window's centre and then moves by (dx, dy), float64 [2, 3]"""
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    return [[a, b, cx - a * cx - b * cy + dx], [d, e, cy - d * cx - e * cy + dy]]


c, s = 1.01 * math.cos(math.radians(1.0)), 1.01 * math.sin(math.radians(1.0))
THETA = {"identity": [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], "near": about_the_centre(c, -s, s, c, 8.0, 5.0), "quarter": about_the_centre(0.0, -1.0, 1.0, 0.0)}
COEF = {k: np.stack(h.warp_coefficients(np.array([t] * N, np.float64))) for k, t in THETA.items()}

res = {"streams": N, "reps": args.reps, "library": os.environ.get("H264BSD_VARIANT", "product")}
next_round()
res["keep_ms"] = timed(lambda st: h.keep_pictures(decs, stream=st), args.reps, args.warmup)
for lo in ("hi", "hilo"):
    if lo == "hilo":
        res["blend_ms"] = timed(lambda st: h.blend_pictures(decs, shift=4, hold=24, stream=st), args.reps, args.warmup)
    for name, coef in COEF.items():
        for outside in ("replicate", "current"):
            call = lambda st: h.warp_kept(decs, coefficients=coef, outside=outside, stream=st)
            res[f"warp_{name}_{lo}_{outside}_ms"] = timed(call, args.reps, args.warmup)
        if lo == "hi":
            counts = h.warp_kept(decs, coefficients=coef, count_outside=True)[2]
            res[f"outside_{name}"] = round(float(counts.double().mean()) / (W * H), 4)
    if lo == "hi":
        next_round()
        assert h.blend_pictures(decs, shift=4, hold=24)[0] == [1] * N       # lo is valid from here on
if not args.kernel_only:
    CH = 32
    held = torch.rand((N, 3, H, W), device="cuda").to(torch.float16)        # what a full-size pull_tensor leaves
    out = torch.empty((CH, 3, H, W), dtype=torch.float16, device="cuda")
    for name, coef in COEF.items():
        a, b, cc, d, e, f = (float(v) / 65536.0 for v in coef[0])           # output -> source in samples, to align_corners=True units
        sx, sy = (W - 1) / 2.0, (H - 1) / 2.0
        m = torch.tensor([[a, b * sy / sx, (a * sx + b * sy + cc) / sx - 1.0], [d * sx / sy, e, (d * sx + e * sy + f) / sy - 1.0]], dtype=torch.float16, device="cuda")

        def route(st):
            grid = torch.nn.functional.affine_grid(m[None].expand(CH, 2, 3), (CH, 3, H, W), align_corners=True)
            for at in range(0, N, CH):
                n = min(CH, N - at)
                out[:n] = torch.nn.functional.grid_sample(held[at:at + n], grid[:n], mode="bilinear", padding_mode="border", align_corners=True)
        res[f"grid_sample_{name}_ms"] = timed(route, 3, 1)
res["device_errors"] = h.device_errors()
print(json.dumps(res))
