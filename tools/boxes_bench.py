#!/usr/bin/env python3
"""What the cell boxes cost (h264bsdmiOutputCellBoxes / pull_boxes) beside the route a caller had without them.

N instances decode the 1080p golden stream through BatchDriver, keep their first picture, decode one more and pop it; everything is
timed on those same N current and kept pictures, which no such call pops (HIP events on a torch stream around the work, the median
over the repetitions after the warm-ups; min and max are the run-to-run spread).  Luma SAD against the kept pictures at cell 16 (68 x
120 cells per window), 8 neighbours, min_cells 2, max_boxes 64; the level is the median of the map, so the maps are neither empty nor full.
  boxes_ms       one pull_boxes call over the N whole windows: the maps, the boxes;
  cells_ms       pull_cells with the same arguments on the same pictures: boxes_ms - cells_ms is the price of the boxes;
  host_ms        the route of today: pull_cells, the maps to host memory, then scipy.ndimage.label + find_objects per stream on a pool
                 of --threads threads (wall clock around all of it, from the call to the last list of boxes; left out, and said so,
                 when scipy does not import);
  *_d2h_bytes    what crosses to the host on each route: the boxes tensor, or the maps;
  worst_ms       pull_boxes of ONE region at the cap whose map is the serpentine of tests/test_gpu_cell_boxes.py, the longest component
                 a slice can hold, and of the 8192 single cells of the checkerboard (cap_* keys; --no-cap leaves them out).
Prints one JSON line.

usage: boxes_bench.py [--streams 256] [--reps 10] [--warmup 2] [--threads 16] [--no-cap]"""
import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                              # noqa: E402
import torch                                    # noqa: E402  (torch's HIP runtime first: capi._share_torch_hip_runtime)
import h264bsd_amd as h                         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=256)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--no-cap", action="store_true")
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
data = open(os.path.join(ROOT, "tests", "golden", "test_1920x1080.h264"), "rb").read()
N = args.streams
L = h.api_lib()
decs = [h.Decoder(no_output_reordering=1) for _ in range(N)]
drv = h.BatchDriver(decs, [data * 2] * N)


def next_round():
    assert len(drv.step()) == N
    assert L.h264bsdmiFlush() == 0
    for d in decs:
        assert d.next_output_info() is not None


def spread(ms):
    ms = sorted(ms)
    return dict(median=round(ms[len(ms) // 2], 4), min=round(ms[0], 4), max=round(ms[-1], 4))


def timed(call, reps, wall=False):
    """the median, min and max over reps of `call` in ms: between HIP events on a side stream, or (wall) by the host's clock"""
    st = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for rep in range(args.warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.stream(st):
            e0.record(st)
            call(st)
            e1.record(st)
        st.synchronize()
        if rep >= args.warmup:
            ms.append((time.perf_counter() - t0) * 1e3 if wall else e0.elapsed_time(e1))
    return spread(ms)


res = {"streams": N, "variant": os.environ.get("H264BSD_VARIANT", ""), "reps": args.reps, "warmup": args.warmup}
next_round()
assert h.keep_pictures(decs)[0] == [1] * N
next_round()
KW = dict(cell=16, source="y", planes=("sad",), against="kept")
BOX = dict(connectivity=8, min_cells=2, max_boxes=64)
first = h.pull_cells(decs, None, **KW)
torch.cuda.synchronize()
maps = first.maps
level = int(maps.to(torch.float32).median().item())
res["level"], res["grid"] = level, list(maps.shape[2:])
bout = torch.empty((N, 1 + BOX["max_boxes"], 8), dtype=torch.int32, device="cuda")
mout = torch.empty_like(maps)

res["cells_ms"] = timed(lambda st: h.pull_cells(decs, None, out=mout, stream=st, **KW), args.reps)
res["boxes_ms"] = timed(lambda st: h.pull_boxes(decs, None, level=level, out=mout, boxes_out=bout, stream=st, **KW, **BOX), args.reps)
res["boxes_minus_cells_ms"] = round(res["boxes_ms"]["median"] - res["cells_ms"]["median"], 4)
cb = h.pull_boxes(decs, None, level=level, out=mout, boxes_out=bout, **KW, **BOX)
torch.cuda.synchronize()
assert bool(torch.equal(mout, maps))
header = cb.header.cpu().numpy()
res["found_median"], res["found_max"], res["foreground_share"] = int(np.median(header[:, 0])), int(header[:, 0].max()), round(float(header[:, 2].mean()) / maps[0].numel(), 3)
res["boxes_d2h_bytes"], res["host_d2h_bytes"] = bout.numel() * 4, maps.numel() * 4
# the same call with the boxes copied to the host and turned into the region list: what a loop pays per tick
res["boxes_to_regions_ms"] = timed(lambda st: h.pull_boxes(decs, None, level=level, out=mout, boxes_out=bout, stream=st, **KW, **BOX).regions(), args.reps, wall=True)

try:
    from scipy import ndimage
except ImportError:
    ndimage = None
    res["host_ms"] = None
    res["host_route"] = "left out: scipy does not import here"
if ndimage is not None:
    pinned = torch.empty(maps.shape, dtype=torch.int32).pin_memory()
    eight = np.ones((3, 3), int)

    def label_one(m):
        lab, n = ndimage.label(m > level, structure=eight)
        sizes = np.bincount(lab.ravel(), minlength=n + 1)[1:]
        return [sl for sl, size in zip(ndimage.find_objects(lab), sizes) if size >= BOX["min_cells"]][:BOX["max_boxes"]]

    pool = ThreadPoolExecutor(args.threads)

    def host_route(st):
        h.pull_cells(decs, None, out=mout, stream=st, **KW)
        pinned.copy_(mout, non_blocking=True)
        st.synchronize()
        return list(pool.map(label_one, pinned.numpy()[:, 0]))

    res["host_ms"] = timed(host_route, args.reps, wall=True)
    res["host_threads"] = args.threads
    # the two routes find the same components (the kernel against scipy, on every stream)
    theirs = host_route(torch.cuda.current_stream())
    records = cb.records.cpu().numpy()
    for r in range(N):
        mine = [(int(x) // 16, int(y) // 16) for x, y, _, _, _, _, _, _ in records[r, :int(header[r, 1])]]
        assert mine == [(sl[1].start, sl[0].start) for sl in theirs[r]], r
    res["host_over_boxes"] = round(res["host_ms"]["median"] / res["boxes_to_regions_ms"]["median"], 2)
    pool.shutdown()

if not args.no_cap:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from pcm_pictures import pcm_stream          # noqa: E402

    def painted(mask):
        Y = np.kron(mask.astype(np.uint8), np.ones((4, 4), np.uint8)) * 255
        return Y, np.full((256, 256), 128, np.uint8), np.full((256, 256), 128, np.uint8)

    serp = np.zeros((128, 128), bool)
    serp[0::2], serp[1::4, -1], serp[3::4, 0] = True, True, True
    i, j = np.indices((128, 128))
    stream = pcm_stream([painted(serp), painted((i + j) % 2 == 0)])
    buf = ctypes.create_string_buffer(stream, len(stream))
    one, off = h.Decoder(1), 0
    for name, conn in (("serpentine", 8), ("checkerboard", 4)):
        r = stall = 0
        while r != h.H264BSD_PIC_RDY and stall <= 3:
            r, rb = one.decode(ctypes.addressof(buf) + off, len(stream) - off)
            off += rb
            stall = stall + 1 if rb == 0 else 0
        assert r == h.H264BSD_PIC_RDY
        assert one.next_output_info() is not None
        kw = dict(cell=4, planes=("max",), against=None, connectivity=conn, max_boxes=512)
        res[f"cap_{name}_cells_ms"] = timed(lambda st: h.pull_cells([one], None, cell=4, planes=("max",), stream=st), args.reps)
        res[f"cap_{name}_boxes_ms"] = timed(lambda st: h.pull_boxes([one], None, stream=st, **kw), args.reps)
        res[f"cap_{name}_found"] = h.pull_boxes([one], None, **kw).found[0]
    one.close()
res["device_errors"] = h.device_errors()
print(json.dumps(res))
