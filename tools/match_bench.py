#!/usr/bin/env python3
"""What the point matches cost (h264bsdmiOutputPointMatches / pull_matches) beside the call they sit next to and the routes a caller
had without them.

N instances decode the 1080p golden stream through BatchDriver; pull_corners of the whole windows at K points, the pictures are kept,
two more are popped and pull_corners again; every timed call then works on that pair of pictures (HIP events on a torch stream around
the work; per figure [median, min, max] in ms over --reps after --warmup calls of the same shape), for each K of --points:
  matches_k<K>_ms        pull_matches of the N whole windows with the two CornerPoints, defaults;
  corners_k<K>_ms        pull_corners alone on the same pictures: the cost it sits beside;
  shift_route_k<K>_ms    the in-product alternative: pull_shift at radius 16 on CornerPoints.regions(29) of the kept points, 65535
                         regions a call, the region array built once outside the timed window and the C entry called directly;
                         shift_route_k<K>_regions is their number;
  torch_pull_ms, torch_k<K>_ms   (not with --kernel-only) the full-size luma pull a caller needs per picture (the previous one is
                         retained), then in torch: replicate padding, 5 x 5 sums (avg_pool2d with divisor 1), two gathers per test,
                         the bits packed to bytes, xor and an 8-bit popcount table, best / second / column minimum; j, best, second
                         and the mutual flag are first checked EQUAL to the call's.
Prints one JSON line.

usage: match_bench.py [--streams 256] [--reps 20] [--warmup 2] [--points 64,256] [--kernel-only]"""
import argparse
import ctypes
import json
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
ap.add_argument("--points", default="64,256")
ap.add_argument("--kernel-only", action="store_true")
args = ap.parse_args()
points = [int(k) for k in args.points.split(",")]

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


WHOLE = [(i, 0, 0, W, H) for i in range(N)]
res = {"streams": N, "reps": args.reps, "points": points}
next_round()
c0 = {K: h.pull_corners(decs, max_points=K) for K in points}
prev = None if args.kernel_only else h.pull_regions(decs, WHOLE, (H, W), dtype=torch.uint8, channels="Y")[0]
assert h.keep_pictures(decs)[0] == [1] * N
next_round()
next_round()                                    # two pictures on: more than noise between them
cur = None
if not args.kernel_only:
    cur = torch.empty((N, 1, H, W), dtype=torch.uint8, device="cuda")
    res["torch_pull_ms"] = timed(lambda st: h.pull_regions(decs, WHOLE, (H, W), dtype=torch.uint8, channels="Y", out=cur, stream=st), args.reps, args.warmup)


def shift_route(arr, R, records, st):
    """boxes around the kept points through the region shift, 65535 a call"""
    dec = (ctypes.c_void_p * N)(*[d._st for d in decs])
    got = (ctypes.c_uint32 * 65535)()
    base = ctypes.addressof(arr)
    for at in range(0, R, 65535):
        k = min(65535, R - at)
        spec = h.ShiftSpec(records.data_ptr() + 32 * at, 16, 0, 1, 0)
        regs = ctypes.cast(base + at * ctypes.sizeof(h.Region), ctypes.POINTER(h.Region))
        rc = L.h264bsdmiOutputRegionShift(N, dec, k, regs, ctypes.byref(spec), st.cuda_stream, got, None, None, None, None)
        assert rc == 0, rc


PATTERN = torch.tensor(h.descriptor_pattern().astype(np.int64), device="cuda")
POPCOUNT = torch.tensor([bin(v).count("1") for v in range(256)], dtype=torch.uint8, device="cuda")
BITS = (1 << torch.arange(8, device="cuda")).view(1, 1, 1, 8)


def describe(luma, pts):
    """[N, K, 32] uint8 descriptors of the points (x, y [N, K]) on luma [N, 1, H, W]"""
    pad = torch.nn.functional.pad(luma.float(), (14, 14, 14, 14), mode="replicate")
    B = torch.nn.functional.avg_pool2d(pad, 5, 1, divisor_override=1)[:, 0]                     # [N, H + 24, W + 24], exact in float32
    n = torch.arange(luma.shape[0], device="cuda").view(-1, 1, 1)
    x, y = pts[0].long().unsqueeze(2) + 12, pts[1].long().unsqueeze(2) + 12
    bits = B[n, y + PATTERN[:, 1], x + PATTERN[:, 0]] < B[n, y + PATTERN[:, 3], x + PATTERN[:, 2]]
    return (bits.view(bits.shape[0], bits.shape[1], 32, 8) * BITS).sum(3).to(torch.uint8)


def torch_route(K, kp, cp):
    """(j, best, second, mutual) [N, K] of the defaults without a gate, every slot valid"""
    dk, dc = describe(prev, kp), describe(cur, cp)
    out = [torch.empty((N, K), dtype=torch.int64, device="cuda") for _ in range(4)]
    step = max(1, (1 << 28) // (K * K * 32))                                                     # a quarter of a gibi-element a time
    for at in range(0, N, step):
        D = POPCOUNT[(dk[at:at + step, :, None, :] ^ dc[at:at + step, None, :, :]).long()].sum(3, dtype=torch.int64)
        key = (D * 1024 + torch.arange(K, device="cuda").view(1, 1, K)).min(2).values            # smallest d, then smallest j
        j, best = key % 1024, key // 1024
        rest = D.scatter(2, j.unsqueeze(2), 1 << 20).min(2).values
        col = (D * 1024 + torch.arange(K, device="cuda").view(1, K, 1)).min(1).values % 1024    # per current slot: smallest d, then i
        for o, v in zip(out, (j, best, torch.where(rest < (1 << 20), rest, torch.full_like(rest, 257)),
                              col.gather(1, j) == torch.arange(K, device="cuda").view(1, K))):
            o[at:at + step] = v
    return out


for K in points:
    corners = torch.empty((N, h.corners_record_bytes(K)), dtype=torch.uint8, device="cuda")
    res[f"corners_k{K}_ms"] = timed(lambda st: h.pull_corners(decs, max_points=K, out=corners, stream=st), args.reps, args.warmup)
    c1 = h.pull_corners(decs, max_points=K)
    out = torch.empty((N, h.matches_record_bytes(K)), dtype=torch.uint8, device="cuda")
    res[f"matches_k{K}_ms"] = timed(lambda st: h.pull_matches(decs, c0[K], c1, out=out, stream=st), args.reps, args.warmup)
    m = h.pull_matches(decs, c0[K], c1, out=out)
    torch.cuda.synchronize()
    res[f"accepted_k{K}"] = int(m.accepted.sum())
    boxes = c0[K].regions(29, WHOLE)
    R = len(boxes)
    arr = (h.Region * R)(*[h.Region(*b) for b in boxes])
    records = torch.empty((R, 32), dtype=torch.uint8, device="cuda")
    res[f"shift_route_k{K}_regions"] = R
    res[f"shift_route_k{K}_ms"] = timed(lambda st: shift_route(arr, R, records, st), args.reps, args.warmup)
    if args.kernel_only:
        continue
    assert bool((c0[K].written == K).all()) and bool((c1.written == K).all())                   # 1080p windows: every slot is a point
    kp, cp = (c0[K].x, c0[K].y), (c1.x, c1.y)
    j, best, second, mutual = torch_route(K, kp, cp)
    assert bool((m.j == j).all()) and bool((m.best == best).all()) and bool((m.second == second).all())
    assert bool(((m.flags & 2) != 0).eq(mutual).all())
    res[f"torch_k{K}_ms"] = timed(lambda st: torch_route(K, kp, cp), 3, 1)
res["device_errors"] = h.device_errors()
print(json.dumps(res))
