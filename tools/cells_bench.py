#!/usr/bin/env python3
"""What the cell maps cost (h264bsdmiOutputCellMaps / pull_cells) beside the two routes a caller had without them.

N instances decode the 1080p golden stream through BatchDriver and keep their first picture; per variant they decode one more picture
and pop it, and the cell maps, route (a) and the floor are timed on those same N current (and kept) pictures, which no such call pops;
route (b) pops by its nature, so each of its repetitions decodes one more picture per instance first (HIP events on a torch stream
around the work, the median over the repetitions):
  cells_<variant>_ms       one pull_cells call over the N whole windows.  Variants: sad16, sad8, sad64 — luma SAD + COUNT against the
                           kept pictures at cell 16, 8 and 64; ycbcr16 — YCbCr, all six CHANGE planes at cell 16; moments16 — luma
                           SUM + SUMSQ of the current pictures at cell 16;
  boxes_<variant>_ms       route (a): the same cells as explicit boxes through h264bsdmiOutputRegionChange / RegionStats (bins 0), in as
                           many calls of at most 65535 regions as that takes (boxes_<variant>_calls), the region arrays built before
                           the clock starts; --boxes-reps repetitions;
  torch_<variant>_ms       route (b): the previous full-size pull_tensor result retained (uint8; "Y", for ycbcr16 "RGB": there is no
                           YCbCr pull), a new one pulled, then the absolute difference (moments16: the samples and their squares) and
                           avg_pool2d over the cells in torch (torch_<variant>_pull_ms is the pull alone);
  floor_<variant>_ms       ONE whole-window pull_change / pull_stats launch without a histogram over the same pictures: it reads the
                           same bytes and writes almost nothing;
and the ratios boxes / cells, torch / cells and cells / floor.  Prints one JSON line.

usage: cells_bench.py [--streams 256] [--reps 10] [--boxes-reps 3] [--warmup 2] [--skip-boxes8]"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                              # noqa: E402
import torch                                    # noqa: E402  (torch's HIP runtime first: capi._share_torch_hip_runtime)
import h264bsd_amd as h                         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=256)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--boxes-reps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--skip-boxes8", action="store_true", help="leave out route (a) at cell 8 (four times the boxes of cell 16)")
args = ap.parse_args()

data = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "test_1920x1080.h264"), "rb").read()
N, W, H = args.streams, 1920, 1080
L = h.api_lib()
decs = [h.Decoder(no_output_reordering=1) for _ in range(N)]
drv = h.BatchDriver(decs, [data * 2] * N)
handles = (ctypes.c_void_p * N)(*[d._st for d in decs])


def next_round(pop=True):
    assert len(drv.step()) == N
    assert L.h264bsdmiFlush() == 0
    if pop:
        for d in decs:
            assert d.next_output_info() is not None


def timed(call, reps, before=None):
    st = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for rep in range(args.warmup + reps):
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


def cell_boxes(cell):
    """every cell of every window as a region, [M, 5] int32 in the layout of h264bsdmi_region"""
    rows, cols = -(-H // cell), -(-W // cell)
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    one = np.stack([np.zeros_like(i), j * cell, i * cell, np.minimum(cell, W - j * cell), np.minimum(cell, H - i * cell)], -1).reshape(-1, 5)
    every = np.tile(one, (N, 1)).astype(np.int32)
    every[:, 0] = np.repeat(np.arange(N), rows * cols)
    return np.ascontiguousarray(every)


def boxes_route(change, source, cell):
    """route (a) as a callable for timed(): (calls, the callable)"""
    boxes = cell_boxes(cell)
    M = len(boxes)
    stride = (h.change_record_bytes if change else h.stats_record_bytes)(source, 0)
    out = torch.empty((M, stride), dtype=torch.uint8, device="cuda")
    regs = (h.Region * M).from_buffer(boxes)
    got = (ctypes.c_uint32 * 65535)()
    src = h.capi.STATS_SOURCES[source][0]
    chunks = [(at, min(65535, M - at)) for at in range(0, M, 65535)]

    def call(st):
        for at, k in chunks:
            part = ctypes.cast(ctypes.byref(regs, at * ctypes.sizeof(h.Region)), ctypes.POINTER(h.Region))
            if change:
                spec = h.ChangeSpec(out.data_ptr() + at * stride, src, 0, 1, (ctypes.c_uint32 * 3)(8, 8, 8), 0)
                rc = L.h264bsdmiOutputRegionChange(N, handles, k, part, ctypes.byref(spec), st.cuda_stream, got, None, None, None, None)
            else:
                spec = h.StatsSpec(out.data_ptr() + at * stride, src, 0, 1)
                rc = L.h264bsdmiOutputRegionStats(N, handles, k, part, ctypes.byref(spec), st.cuda_stream, got, None, None)
            assert rc == 0
    return len(chunks), call, out


res = {"streams": N, "variant": os.environ.get("H264BSD_VARIANT", "")}
next_round()
assert h.keep_pictures(decs)[0] == [1] * N
prev = {ch: torch.empty((N, C, H, W), dtype=torch.uint8, device="cuda") for ch, C in (("Y", 1), ("RGB", 3))}
for ch in prev:
    next_round(False)
    assert h.pull_tensor(decs, dtype=torch.uint8, channels=ch, out=prev[ch])[1] == [1] * N      # what route (b) retained of an earlier picture
torch.cuda.synchronize()

VARIANTS = (("sad16", "kept", "y", 16, ("count", "sad")), ("sad8", "kept", "y", 8, ("count", "sad")), ("sad64", "kept", "y", 64, ("count", "sad")),
            ("ycbcr16", "kept", "ycbcr", 16, ("count", "sad", "ssd", "dsum", "dmax", "above")), ("moments16", None, "y", 16, ("sum", "sumsq")))
for name, against, source, cell, planes in VARIANTS:
    C = 1 if source == "y" else 3
    next_round()
    first = h.pull_cells(decs, None, cell=cell, source=source, planes=planes, against=against, threshold=8 if against else 0)
    out = first.maps
    grid = tuple(out.shape[2:])
    res[f"cells_{name}_ms"] = timed(lambda st: h.pull_cells(decs, None, cell=cell, grid=grid, source=source, planes=planes, against=against,
                                                            threshold=8 if against else 0, out=out, stream=st), args.reps)
    # the floor: one launch over the whole windows, no histogram
    if against:
        fout = torch.empty((N, h.change_record_bytes(source, 0)), dtype=torch.uint8, device="cuda")
        res[f"floor_{name}_ms"] = timed(lambda st: h.pull_change(decs, None, source=source, bins=0, threshold=8, out=fout, stream=st), args.reps)
        whole = h.RegionChange(fout.cpu(), C, 0, [], [], [], [], [])
        assert bool((out[:, 1:1 + C].sum((2, 3), dtype=torch.int64).cpu() == whole.sad).all())         # the cells add up to the window
    else:
        fout = torch.empty((N, h.stats_record_bytes(source, 0)), dtype=torch.uint8, device="cuda")
        res[f"floor_{name}_ms"] = timed(lambda st: h.pull_stats(decs, None, source=source, bins=0, out=fout, stream=st), args.reps)
        whole = h.RegionStats(fout.cpu(), C, 0, [], [], [])
        assert bool((out[:, 0:C].sum((2, 3), dtype=torch.int64).cpu() == whole.sum).all())
    res[f"cells_{name}_over_floor"] = round(res[f"cells_{name}_ms"] / res[f"floor_{name}_ms"], 2)
    # route (a)
    if not (cell == 8 and args.skip_boxes8):
        calls, call, bout = boxes_route(against is not None, source, cell)
        res[f"boxes_{name}_calls"] = calls
        res[f"boxes_{name}_ms"] = timed(call, args.boxes_reps)
        res[f"boxes_{name}_over_cells"] = round(res[f"boxes_{name}_ms"] / res[f"cells_{name}_ms"], 1)
        rows, cols = out.shape[2:]
        w32 = bout.view(torch.int32)
        if against:                                                               # record: count, zero, then per channel sad (u64) ...
            assert bool((w32[:, 0].reshape(N, rows, cols) == out[:, 0]).all()) and bool((w32[:, 2].reshape(N, rows, cols) == out[:, 1]).all())
        else:
            assert bool((w32[:, 2].reshape(N, rows, cols) == out[:, 0]).all())
        del bout, w32, call
    # route (b)
    ch = "RGB" if C == 3 else "Y"
    t = torch.empty((N, C, H, W), dtype=torch.uint8, device="cuda")

    def pull(st):
        assert h.pull_tensor(decs, dtype=torch.uint8, channels=ch, out=t, stream=st)[1] == [1] * N

    res[f"torch_{name}_pull_ms"] = timed(pull, max(args.boxes_reps, 3), before=lambda: next_round(False))

    def pool(st):
        pull(st)
        if against:
            d = t.to(torch.int16) - prev[ch].to(torch.int16)
            a = d.abs().float()
            maps = [torch.nn.functional.avg_pool2d(a, cell, ceil_mode=True)]
            if len(planes) > 2:
                maps += [torch.nn.functional.avg_pool2d(a * a, cell, ceil_mode=True), torch.nn.functional.avg_pool2d(d.float(), cell, ceil_mode=True),
                         torch.nn.functional.max_pool2d(a, cell, ceil_mode=True), torch.nn.functional.avg_pool2d((a > 8).float(), cell, ceil_mode=True)]
        else:
            v = t.float()
            maps = [torch.nn.functional.avg_pool2d(v, cell, ceil_mode=True), torch.nn.functional.avg_pool2d(v * v, cell, ceil_mode=True)]
        return maps

    res[f"torch_{name}_ms"] = timed(pool, max(args.boxes_reps, 3), before=lambda: next_round(False))
    res[f"torch_{name}_over_cells"] = round(res[f"torch_{name}_ms"] / res[f"cells_{name}_ms"], 1)
    del t, out, first
    torch.cuda.empty_cache()
res["beats_boxes_at_cell16"] = bool(res["boxes_sad16_ms"] > res["cells_sad16_ms"])
res["device_errors"] = h.device_errors()
print(json.dumps(res))
