#!/usr/bin/env python3
"""What the corner points cost (h264bsdmiOutputCornerPoints / pull_corners) beside what a caller does without them.

N instances decode the 1080p golden stream through BatchDriver and pop a picture; every timed call then works on those current
pictures (HIP events on a torch stream around the work; per figure [median, min, max] in ms over --reps after --warmup calls of the
same shape; the N frames of a call are 0.8 GB at N = 256, far beyond the caches, so repeating a call on the same pictures does not
flatter it).  nms 3, K 64, block 3, both scores:
  corners_<score>_ms, corners_<score>_grid_ms   pull_corners of the N whole windows (a few row bands each, merged through the scratch)
                                                and of an 8 x 8 grid of 240 x 135 boxes per picture (64 N regions, one workgroup each);
  stats_y_ms, stats_y_grid_ms                   pull_stats, luma, no histogram, of the same regions: it reads the same bytes once and is
                                                the floor;
  shift_r0_ms, shift_r0_grid_ms                 pull_shift at radius 0 of the same regions against a kept copy of the same picture: the
                                                nearest sibling with LDS staging;
  torch_pull_ms                                 the full-size luma pull a caller needs first (pull_regions of the whole windows at scale 1);
  torch_<score>_ms, torch_<score>_grid_ms       then, in torch, float32: replicate padding, Sobel conv2d, box avg_pool2d of the three
                                                products, the score, max_pool2d for the suppression, topk per window / per box, over
                                                --torch-reps, in chunks of --torch-chunk pictures; *_with_pull_ms adds torch_pull_ms.
The torch composition is in floats and breaks ties by whatever topk does: it is a baseline for time, not for the records.  top8_agree:
whether the 8 strongest MIN_EIGEN points of picture 0 are at the same places in a float64 torch evaluation.  Prints one JSON line.

usage: corners_bench.py [--streams 256] [--reps 10] [--warmup 2] [--torch-reps 3] [--torch-chunk 32] [--kernel-only]"""
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
ap.add_argument("--torch-chunk", type=int, default=32)
ap.add_argument("--kernel-only", action="store_true")
args = ap.parse_args()

data = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "test_1920x1080.h264"), "rb").read()
N, W, H = args.streams, 1920, 1080
NMS, K, BLOCK, GRID = 3, 64, 3, 8
GW, GH = W // GRID, H // GRID
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
BOXES = [(i, GW * gx, GH * gy, GW, GH) for i in range(N) for gy in range(GRID) for gx in range(GRID)]
res = {"streams": N, "reps": args.reps, "torch_reps": args.torch_reps, "nms": NMS, "max_points": K, "block": BLOCK, "grid": GRID}
next_round()
next_round()
next_round()
assert h.keep_pictures(decs)[0] == [1] * N       # pull_shift's other picture: a copy of the current one

for name, regions in (("", WHOLE), ("_grid", BOXES)):
    R = len(regions)
    for score in ("min_eigen", "harris"):
        out = torch.empty((R, h.corners_record_bytes(K)), dtype=torch.uint8, device="cuda")
        res[f"corners_{score}{name}_ms"] = timed(lambda st: h.pull_corners(decs, regions, score=score, block=BLOCK, nms=NMS, max_points=K, out=out, stream=st), args.reps)
    sout = torch.empty((R, h.stats_record_bytes("y", 0)), dtype=torch.uint8, device="cuda")
    res[f"stats_y{name}_ms"] = timed(lambda st: h.pull_stats(decs, regions, source="y", bins=0, out=sout, stream=st), args.reps)
    hout = torch.empty((R, h.shift_record_bytes(0, False)), dtype=torch.uint8, device="cuda")
    res[f"shift_r0{name}_ms"] = timed(lambda st: h.pull_shift(decs, regions, radius=0, out=hout, stream=st), args.reps)
    res[f"corners_over_stats{name}"] = round(res[f"corners_min_eigen{name}_ms"][0] / res[f"stats_y{name}_ms"][0], 2)

cp = h.pull_corners(decs, WHOLE, score="min_eigen", block=BLOCK, nms=NMS, max_points=K)
torch.cuda.synchronize()
res["found_mean"] = round(float(cp.found.double().mean()), 1)
res["energy_mean"] = round(float(cp.energy.double().mean()), 1)

if not args.kernel_only:
    cur = torch.empty((N, 1, H, W), dtype=torch.uint8, device="cuda")
    res["torch_pull_ms"] = timed(lambda st: h.pull_regions(decs, WHOLE, (H, W), dtype=torch.uint8, channels="Y", out=cur, stream=st), args.reps)
    F = torch.nn.functional

    def score_planes(luma, score, dtype):
        """[n, 1, H, W] scores of [n, 1, H, W] uint8 luma, replicated at the window's border as the call replicates it"""
        kx = torch.tensor([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], dtype=dtype, device="cuda")
        hb = BLOCK // 2
        pad = F.pad(luma.to(dtype), (hb + 1,) * 4, mode="replicate")
        g = F.conv2d(pad, torch.stack([kx, kx.t()])[:, None])                               # [n, 2, H + 2 hb, W + 2 hb]
        gx, gy = g[:, :1], g[:, 1:]
        A, B, C = (F.avg_pool2d(p, BLOCK, stride=1) * (BLOCK * BLOCK) for p in (gx * gx, gy * gy, gx * gy))
        if score == "harris":
            return 16 * (A * B - C * C) - (A + B) * (A + B)
        return A + B - torch.sqrt((A - B) * (A - B) + 4 * C * C)

    def compose(score, grid, dtype=torch.float32, pictures=None):
        """(values, indices) of the K strongest local maxima per window (grid: per box), chunk by chunk"""
        tops = []
        src = cur if pictures is None else cur[:pictures]
        for at in range(0, src.shape[0], args.torch_chunk):
            S = score_planes(src[at:at + args.torch_chunk], score, dtype)
            peak = F.max_pool2d(S, 2 * NMS + 1, stride=1, padding=NMS)
            S = torch.where((S == peak) & (S > 0), S, torch.zeros_like(S))
            if grid:
                S = S.view(-1, GRID, GH, GRID, GW).permute(0, 1, 3, 2, 4).reshape(-1, GH * GW)
            else:
                S = S.view(-1, H * W)
            tops.append(S.topk(K, dim=1))
        return tops

    for score in ("min_eigen", "harris"):
        for name, grid in (("", False), ("_grid", True)):
            t = timed(lambda st: compose(score, grid), args.torch_reps)
            res[f"torch_{score}{name}_ms"] = t
            res[f"torch_{score}{name}_with_pull_ms"] = round(t[0] + res["torch_pull_ms"][0], 4)
    idx = compose("min_eigen", False, torch.float64, pictures=1)[0][1][0, :8]
    mine = (cp.y[0, :8].long() * W + cp.x[0, :8].long())
    res["top8_agree"] = bool((idx.sort()[0] == mine.sort()[0]).all())
    res["faster_than_torch_with_pull"] = bool(res["corners_min_eigen_ms"][0] < res["torch_min_eigen_with_pull_ms"])
res["device_errors"] = h.device_errors()
print(json.dumps(res))
