#!/usr/bin/env python3
"""What the cell shift costs (h264bsdmiOutputCellShift / pull_flow) beside the routes a caller had without it.

N instances decode the 1080p golden stream through BatchDriver, keep their first picture and pop two more; every timed call then
searches every cell of the kept pictures in the current ones (HIP events on a torch stream around the work; per figure [median, min,
max] in ms over --reps after --warmup calls of the same shape):
  flow_c<cell>_r<R>_ms      pull_flow of the N whole windows, planes dx, dy, best, still, ties, at each of --cells x --radii;
  regions_c<cell>_r<R>_ms   the route that existed before: the same cells as regions through h264bsdmiOutputRegionShift, 65535 a call,
                            in as many calls as that takes, the region array built once outside the timed window and the C entry called
                            directly (no Python marshalling), over --route-reps; its dx, dy, best, still, ties are first checked EQUAL
                            to the maps; regions_c<cell>_calls is the number of calls;
  shift_r<R>_ms             pull_shift of the N whole windows at the same radius: the same sample differences, one argmin a window;
  torch_pull_ms, torch_c16_r4_ms   (not with --kernel-only) the full-size luma pull a caller needs per picture (the previous one is
                            retained), then in torch: replicate padding, (2R+1)^2 sliced |a - b|, pooled per cell of 16, and the argmin
                            under the call's tie rule; checked EQUAL to the maps first.
Ratios: over_regions_* = regions / flow, over_shift_* = flow / shift.  Prints one JSON line.

usage: flow_bench.py [--streams 256] [--reps 10] [--warmup 2] [--route-reps 10] [--cells 8,16,32] [--radii 0,2,4,8,16] [--kernel-only] [--no-route]"""
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
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--route-reps", type=int, default=10)
ap.add_argument("--cells", default="8,16,32")
ap.add_argument("--radii", default="0,2,4,8,16")
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--no-route", action="store_true")
args = ap.parse_args()
cells = [int(c) for c in args.cells.split(",")]
radii = [int(r) for r in args.radii.split(",")]

data = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "test_1920x1080.h264"), "rb").read()
N, W, H = args.streams, 1920, 1080
L = h.api_lib()
decs = [h.Decoder(no_output_reordering=1) for _ in range(N)]
drv = h.BatchDriver(decs, [data] * N)
PLANES = ("dx", "dy", "best", "still", "ties")


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
res = {"streams": N, "reps": args.reps, "route_reps": args.route_reps, "cells": cells, "radii": radii}
next_round()
prev = None
if not args.kernel_only:
    prev = h.pull_regions(decs, WHOLE, (H, W), dtype=torch.uint8, channels="Y")[0]
assert h.keep_pictures(decs)[0] == [1] * N
next_round()
next_round()                                    # two pictures on: more than noise between them

for R in radii:
    out = torch.empty((N, h.shift_record_bytes(R, False)), dtype=torch.uint8, device="cuda")
    res[f"shift_r{R}_ms"] = timed(lambda st: h.pull_shift(decs, None, radius=R, out=out, stream=st), args.reps, args.warmup)


def cell_regions(cell):
    """every cell of every window as a region, in the order of the maps: a ctypes Region array, and its length"""
    rows, cols = -(-H // cell), -(-W // cell)
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    one = np.zeros((rows, cols), dtype=[("instance", "<u4"), ("x", "<i4"), ("y", "<i4"), ("w", "<u4"), ("h", "<u4")])
    one["x"], one["y"] = j * cell, i * cell
    one["w"], one["h"] = np.minimum(cell, W - j * cell), np.minimum(cell, H - i * cell)
    regs = np.broadcast_to(one.reshape(1, -1), (N, rows * cols)).copy()
    regs["instance"] = np.arange(N, dtype=np.uint32)[:, None]
    regs = np.ascontiguousarray(regs.reshape(-1))
    assert regs.itemsize == ctypes.sizeof(h.Region)
    return (h.Region * regs.size).from_buffer(regs), regs.size, regs


def region_route(arr, K, R, records, st):
    """the cells as regions through the region shift, 65535 a call"""
    dec = (ctypes.c_void_p * N)(*[d._st for d in decs])
    got = (ctypes.c_uint32 * 65535)()
    base = ctypes.addressof(arr)
    for at in range(0, K, 65535):
        k = min(65535, K - at)
        spec = h.ShiftSpec(records.data_ptr() + 32 * at, R, 0, 1, 0)
        regs = ctypes.cast(base + at * ctypes.sizeof(h.Region), ctypes.POINTER(h.Region))
        rc = L.h264bsdmiOutputRegionShift(N, dec, k, regs, ctypes.byref(spec), st.cuda_stream, got, None, None, None, None)
        assert rc == 0, rc


for cell in cells:
    grid = (-(-H // cell), -(-W // cell))
    maps = torch.empty((N, len(PLANES), grid[0], grid[1]), dtype=torch.int32, device="cuda")
    if not args.no_route:
        arr, K, keepalive = cell_regions(cell)
        assert K == N * grid[0] * grid[1]
        records = torch.empty((K, 32), dtype=torch.uint8, device="cuda")
        res[f"regions_c{cell}_calls"] = -(-K // 65535)
    for R in radii:
        name = f"c{cell}_r{R}"
        res[f"flow_{name}_ms"] = timed(lambda st: h.pull_flow(decs, None, cell=cell, grid=grid, radius=R, planes=PLANES, out=maps, stream=st),
                                       args.reps, args.warmup)
        res[f"over_shift_{name}"] = round(res[f"flow_{name}_ms"][0] / res[f"shift_r{R}_ms"][0], 2)
        if args.no_route:
            continue
        res[f"regions_{name}_ms"] = timed(lambda st: region_route(arr, K, R, records, st), args.route_reps, args.warmup)
        torch.cuda.synchronize()
        w32 = records.view(torch.int32).view(N, grid[0], grid[1], 8)
        for p, word in enumerate((2, 3, 4, 5, 6)):          # dx, dy, best, still, ties of the record
            assert bool((w32[..., word] == maps[:, p]).all()), (name, PLANES[p])
        res[f"over_regions_{name}"] = round(res[f"regions_{name}_ms"][0] / res[f"flow_{name}_ms"][0], 1)

if not args.kernel_only and 16 in cells and 4 in radii:
    cell, R = 16, 4
    D, rows, cols = 2 * R + 1, -(-H // cell), -(-W // cell)
    cur = torch.empty((N, 1, H, W), dtype=torch.uint8, device="cuda")
    res["torch_pull_ms"] = timed(lambda st: h.pull_regions(decs, WHOLE, (H, W), dtype=torch.uint8, channels="Y", out=cur, stream=st), args.reps, args.warmup)
    kept16 = prev.to(torch.int16)

    def search():
        """[N, D D, rows, cols] int32 SADs per cell, then (dx, dy, best) under the tie rule"""
        pad = torch.nn.functional.pad(cur.float(), (R, R, R, R), mode="replicate").to(torch.int16)
        sad = torch.empty((N, D * D, rows, cols), dtype=torch.int32, device="cuda")
        for dy in range(D):
            for dx in range(D):
                d = (kept16 - pad[:, :, dy:dy + H, dx:dx + W]).abs()
                d = torch.nn.functional.pad(d, (0, cols * cell - W, 0, rows * cell - H))
                sad[:, dy * D + dx] = d.view(N, rows, cell, cols, cell).sum((2, 4), dtype=torch.int32)
        off = torch.arange(-R, R + 1, device="cuda")
        rank = ((off[:, None] ** 2 + off[None, :] ** 2) * 4096 + (off[:, None] + R) * 64 + (off[None, :] + R)).view(1, -1, 1, 1)
        at = (sad.long() * (1 << 22) + rank).argmin(1)
        return at % D - R, at // D - R, sad.gather(1, at[:, None])[:, 0]

    dx, dy, best = search()
    ref = h.pull_flow(decs, None, cell=cell, grid=(rows, cols), radius=R, planes=("dx", "dy", "best"))
    assert bool((ref.dx == dx).all()) and bool((ref.dy == dy).all()) and bool((ref.best == best).all())
    res["torch_c16_r4_ms"] = timed(lambda st: search(), 3, 1)
res["device_errors"] = h.device_errors()
print(json.dumps(res))
