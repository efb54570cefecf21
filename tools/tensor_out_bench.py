#!/usr/bin/env python3
"""Batched device-resident output (h264bsdmiNextOutputTensorBatch / pull_tensor) against what a caller had to do before.

256 instances decode the 1080p golden stream (no output reordering: one picture per instance and round).  Before every timed
repetition each instance decodes one more picture and the device finishes it (h264bsdmiFlush), so that only the pull is timed:
  (a) pull_tensor -> [256, 3, 1080, 1920] float16, ImageNet-normalised, no resize     HIP events on a torch stream around the call
  (b) pull_tensor -> [256, 3, 224, 224] float16, resized + normalised                   (the same)
  (c) the same two results the old way: 256 x next_output_picture_device(FMT_RGBA, crop=True) + clone, stack, cast,
      F.interpolate (for b), normalise                                                    wall clock, synchronised (host waits inside)
  (d) (b)'s result with --filter's antialiasing the old way: pull (a) unnormalised, F.interpolate(antialias=True) to 224 x 224,
      normalise, cast                                                                   HIP events on the torch stream (no host wait)
(a) is also given in GB/s (tiles read + tensor written) next to the device-to-device copy ceiling, measured here the way
`bench.py --full` does (1 GiB copy, read + write).  --colour / --range / --chroma pull (a) and (b) in that colour space
(h264bsdmiNextOutputTensorBatchColour; default: the reference conversion, h264bsdmiNextOutputTensorBatch).  --filter / --fit pull (b)
with that resampling filter and fit (h264bsdmiNextOutputTensorBatchResize; default: bilinear, stretch).  Prints one JSON line.

--regions K is a leg of its own (h264bsdmiOutputTensorRegions / pull_regions): K seeded boxes per instance with sides between 64 and
400 luma samples, a few of them over the picture's edge, into [K * streams, 3, 256, 128] float16, ImageNet-normalised, bilinear_aa,
letterboxed.  Every repetition decodes one more picture per instance and pops it (h264bsdmiNextOutputInfo) before the clock starts:
  (e) one pull_regions call                                                              HIP events on a torch stream around the call
  (f) the same tensor without it: pull_tensor(size=None), then per box slice (padded where it hangs over the edge),
      F.interpolate(antialias=True) to the letterbox rectangle, paste into a padded tensor; normalise, cast     (the same clock)
  (b) with the same filter, stretched to 224 x 224, for the cost per output element next to (e)'s; (a), (c), (d) are not run.

usage: tensor_out_bench.py [--streams 256] [--reps 20] [--warmup 3] [--old-reps 3] [--colour reference|auto|bt601|bt709|...]
                           [--range auto|limited|full] [--chroma nearest|bilinear] [--filter bilinear|bilinear_aa|bicubic_aa]
                           [--fit stretch|letterbox] [--only-b] [--no-old] [--regions K] [--remap]

--remap is a leg of its own (h264bsdmiOutputTensorRemap / pull_remap), on the current pictures, HIP events, the median of 10:
  (g) one pull_remap call: every picture through ONE shared smooth (barrel) map -> [N, 3, 540, 960] f16, bilinear
  (h) the same with calls the library had before: a full-size pull_tensor, then grid_sample(align_corners=True) with that map
  (i) 4 rotated 128 x 64 boxes per picture (affine_maps) in one pull_remap call -> [4 N, 3, 64, 128]
  (j) the same boxes as pull_regions of their axis-aligned hulls (-> 160 x 160, bilinear), then grid_sample with the rotation"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                    # noqa: E402  (torch's HIP runtime first: capi._share_torch_hip_runtime)
import torch.nn.functional as F                 # noqa: E402
import h264bsd_amd as h                         # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=256)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--old-reps", type=int, default=3)
ap.add_argument("--colour", default="reference", choices=sorted(h.capi.MATRICES))
ap.add_argument("--range", default="auto", choices=sorted(h.capi.RANGES))
ap.add_argument("--chroma", default="nearest", choices=sorted(h.capi.CHROMA))
ap.add_argument("--filter", default="bilinear", choices=["bilinear", "bilinear_aa", "bicubic_aa"])
ap.add_argument("--fit", default="stretch", choices=sorted(h.capi.FITS))
ap.add_argument("--only-b", action="store_true", help="time (b) and (d) only")
ap.add_argument("--no-old", action="store_true", help="skip (c), (d) and the copy ceiling")
ap.add_argument("--regions", type=int, default=0, help="K boxes per instance: time (e), (f) and (b) with bilinear_aa only")
ap.add_argument("--remap", action="store_true", help="time (g) .. (j) only: pull_remap against the full-size pull + grid_sample")
args = ap.parse_args()
if args.regions:
    args.filter, args.fit, args.only_b, args.no_old = "bilinear_aa", "stretch", True, True

data = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "test_1920x1080.h264"), "rb").read()
N = args.streams
rounds = 2 * (args.warmup + args.reps) + 3 * (1 + args.old_reps) + 2
if args.regions:
    rounds += args.warmup + args.reps + 1 + args.old_reps
if args.remap:
    rounds = 2 * (args.warmup + 10) + 2 * (1 + args.old_reps) + 2
decs = [h.Decoder(no_output_reordering=1) for _ in range(N)]
drv = h.BatchDriver(decs, [data * (rounds // 73 + 2)] * N)
L = h.api_lib()


def next_round():
    """every instance decodes one more picture; the device has finished it on return"""
    assert len(drv.step()) == N
    assert L.h264bsdmiFlush() == 0


def time_pull(size, out, **resize):
    st = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms, wall = [], []
    for rep in range(args.warmup + args.reps):
        next_round()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record(st)
        _, got, _, _, _ = h.pull_tensor(decs, size=size, dtype=torch.float16, mean=MEAN, std=STD, out=out, stream=st, **COLOUR, **resize)
        e1.record(st)
        st.synchronize()
        t1 = time.perf_counter()
        assert got == [1] * N
        if rep >= args.warmup:
            ms.append(e0.elapsed_time(e1))
            wall.append((t1 - t0) * 1e3)
    return sorted(ms)[len(ms) // 2], sorted(wall)[len(wall) // 2], min(ms)


def time_old(size):
    mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    wall = []
    for rep in range(1 + args.old_reps):
        next_round()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pics = [d.next_output_picture_device(h.FMT_RGBA, crop=True)[0].clone() for d in decs]
        x = torch.stack(pics)[..., :3].permute(0, 3, 1, 2).float()
        del pics
        if size is not None:
            x = F.interpolate(x, size=size, mode="bilinear", align_corners=False, antialias=False)
        y = ((x / 255 - mean) / std).half()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        del x, y
        torch.cuda.empty_cache()
    return sorted(wall[1:])[len(wall[1:]) // 2]


def time_old_aa(size):
    """(d): the full-size pull, unnormalised, then torch's antialiased interpolate and the normalisation on the same stream"""
    mode, aa = FILTER[args.filter]
    mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    full = torch.empty((N, 3, 1080, 1920), dtype=torch.float16, device="cuda")
    st = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for rep in range(1 + args.old_reps):
        next_round()
        torch.cuda.synchronize()
        e0.record(st)
        h.pull_tensor(decs, dtype=torch.float16, out=full, stream=st, **COLOUR)
        with torch.cuda.stream(st):
            y = ((F.interpolate(full, size=size, mode=mode, antialias=aa, align_corners=False) - mean) / std).half()
        e1.record(st)
        st.synchronize()
        ms.append(e0.elapsed_time(e1))
        del y
    del full
    torch.cuda.empty_cache()
    return sorted(ms[1:])[len(ms[1:]) // 2]


ROI_SIZE, ROI_PAD = (256, 128), (0.5, 0.5, 0.5)


def region_boxes(k):
    """k seeded boxes per instance as (instance, x, y, w, h): sides 64..400, origins that let a few of them hang over the edge"""
    import numpy as np
    rng = np.random.default_rng(2048)
    w, hh = rng.integers(64, 401, N * k), rng.integers(64, 401, N * k)
    x, y = rng.integers(-32, 1920 - w + 33), rng.integers(-32, 1080 - hh + 33)
    return [(i // k, int(x[i]), int(y[i]), int(w[i]), int(hh[i])) for i in range(N * k)]


def time_regions(regions):
    """(e): one pull_regions call on the pictures popped just before"""
    out = torch.empty((len(regions), 3) + ROI_SIZE, dtype=torch.float16, device="cuda")
    st = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms, wall = [], []
    for rep in range(args.warmup + args.reps):
        next_round()
        for d in decs:
            assert d.next_output_info() is not None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record(st)
        _, got, boxes, _, _ = h.pull_regions(decs, regions, ROI_SIZE, dtype=torch.float16, mean=MEAN, std=STD, out=out, stream=st,
                                             mode="bilinear", antialias=True, fit="letterbox", pad=ROI_PAD, **COLOUR)
        e1.record(st)
        st.synchronize()
        t1 = time.perf_counter()
        assert all(got)
        if rep >= args.warmup:
            ms.append(e0.elapsed_time(e1))
            wall.append((t1 - t0) * 1e3)
    return sorted(ms)[len(ms) // 2], sorted(wall)[len(wall) // 2], min(ms), boxes


def time_regions_old(regions, boxes):
    """(f): the full-size pull, then slice, pad, antialiased interpolate and paste per box, normalise and cast once"""
    mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    full = torch.empty((N, 3, 1080, 1920), dtype=torch.float16, device="cuda")
    st = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for rep in range(1 + args.old_reps):
        next_round()
        torch.cuda.synchronize()
        e0.record(st)
        h.pull_tensor(decs, dtype=torch.float16, out=full, stream=st, **COLOUR)
        with torch.cuda.stream(st):
            canvas = torch.full((len(regions), 3) + ROI_SIZE, ROI_PAD[0], dtype=torch.float16, device="cuda")
            for k, ((i, x, y, w, hh), (left, top, iw, ih)) in enumerate(zip(regions, boxes)):
                xa, xb, ya, yb = max(x, 0), min(x + w, 1920), max(y, 0), min(y + hh, 1080)
                crop = full[i:i + 1, :, ya:yb, xa:xb]
                if (xa, xb, ya, yb) != (x, x + w, y, y + hh):
                    crop = F.pad(crop, (xa - x, x + w - xb, ya - y, y + hh - yb), value=ROI_PAD[0])
                canvas[k:k + 1, :, top:top + ih, left:left + iw] = F.interpolate(crop, size=(ih, iw), mode="bilinear", antialias=True,
                                                                                align_corners=False)
            y_ = ((canvas - mean) / std).half()
        e1.record(st)
        st.synchronize()
        ms.append(e0.elapsed_time(e1))
        del y_, canvas
    del full
    torch.cuda.empty_cache()
    return sorted(ms[1:])[len(ms[1:]) // 2]


def copy_ceiling_gbs():
    src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    dst.copy_(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    return 10 * 2 * src.numel() / (e0.elapsed_time(e1) * 1e-3) / 1e9


def remap_legs():
    import math
    import numpy as np
    H, W, K, BH, BW, HULL = 540, 960, 4, 64, 128, 160
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    u, t = 2 * (j + 0.5) / W - 1, 2 * (i + 0.5) / H - 1
    s = (1 + 0.35 * (u * u + t * t) / 2) / 1.35                        # barrel: pulled towards the centre, the corners stay
    barrel = torch.from_numpy(np.stack([959.5 + u * s * 964.5, 539.5 + t * s * 544.5], axis=-1).astype(np.float32)).cuda()
    grid = torch.stack([barrel[..., 0] / 959.5 - 1, barrel[..., 1] / 539.5 - 1], dim=-1).half()       # x = (gx + 1) (W - 1) / 2
    rng = np.random.default_rng(1024)
    ang, cx, cy = rng.uniform(0, 2 * math.pi, N * K), rng.uniform(100, 1820, N * K), rng.uniform(100, 980, N * K)
    co, si = np.cos(ang), np.sin(ang)
    # output (i, j) of a BH x BW box <- centre + R (j - (BW - 1) / 2, i - (BH - 1) / 2)
    theta = np.stack([np.stack([co, -si, cx - co * (BW - 1) / 2 + si * (BH - 1) / 2], -1),
                      np.stack([si, co, cy - si * (BW - 1) / 2 - co * (BH - 1) / 2], -1)], 1)
    rot_maps = h.affine_maps(theta, (BH, BW))
    inst = [k // K for k in range(N * K)]
    hulls = [(k // K, int(round(cx[k])) - HULL // 2, int(round(cy[k])) - HULL // 2, HULL, HULL) for k in range(N * K)]
    # the same rotation inside the hull, as a normalised align_corners=True grid over its HULL samples
    hx = (rot_maps[..., 0] - torch.tensor([b[1] for b in hulls], device="cuda").view(-1, 1, 1)) / ((HULL - 1) / 2) - 1
    hy = (rot_maps[..., 1] - torch.tensor([b[2] for b in hulls], device="cuda").view(-1, 1, 1)) / ((HULL - 1) / 2) - 1
    hull_grid = torch.stack([hx, hy], dim=-1).half()
    st = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()

    def timed(reps, fn, pop=True):
        ms = []
        for rep in range(reps[0] + reps[1]):
            next_round()
            for d in decs if pop else []:
                assert d.next_output_info() is not None
            torch.cuda.synchronize()
            e0.record(st)
            fn()
            e1.record(st)
            st.synchronize()
            if rep >= reps[0]:
                ms.append(e0.elapsed_time(e1))
        return sorted(ms)[len(ms) // 2], min(ms)

    out_g = torch.empty((N, 3, H, W), dtype=torch.float16, device="cuda")
    out_i = torch.empty((N * K, 3, BH, BW), dtype=torch.float16, device="cuda")
    kw = dict(dtype=torch.float16, mean=MEAN, std=STD, stream=st, **COLOUR)

    def leg_g():
        assert all(h.pull_remap(decs, [barrel] * N, out=out_g, **kw)[1])

    def leg_i():
        assert all(h.pull_remap(decs, rot_maps, instances=inst, out=out_i, **kw)[1])

    g_ms, g_min = timed((args.warmup, 10), leg_g)
    i_ms, i_min = timed((args.warmup, 10), leg_i)
    del out_g, out_i
    full = torch.empty((N, 3, 1080, 1920), dtype=torch.float16, device="cuda")
    hull_t = torch.empty((N * K, 3, HULL, HULL), dtype=torch.float16, device="cuda")

    def leg_h():
        h.pull_tensor(decs, out=full, **kw)             # pops the pictures itself
        with torch.cuda.stream(st):
            F.grid_sample(full, grid.expand(N, H, W, 2), mode="bilinear", padding_mode="zeros", align_corners=True)

    def leg_j():
        h.pull_regions(decs, hulls, (HULL, HULL), out=hull_t, **kw)
        with torch.cuda.stream(st):
            F.grid_sample(hull_t, hull_grid, mode="bilinear", padding_mode="zeros", align_corners=True)

    h_ms, h_min = timed((1, args.old_reps), leg_h, pop=False)
    j_ms, j_min = timed((1, args.old_reps), leg_j)
    print(json.dumps(dict(streams=N, colour=args.colour, chroma=args.chroma, g_ms=round(g_ms, 3), g_min_ms=round(g_min, 3),
                          h_ms=round(h_ms, 3), h_min_ms=round(h_min, 3), speedup_g=round(h_ms / g_ms, 2),
                          g_ns_per_element=round(g_ms * 1e6 / (N * 3 * H * W), 5),
                          boxes=N * K, i_ms=round(i_ms, 3), i_min_ms=round(i_min, 3), j_ms=round(j_ms, 3), j_min_ms=round(j_min, 3),
                          speedup_i=round(j_ms / i_ms, 2), device_errors=h.device_errors())))


COLOUR = {} if args.colour == "reference" else dict(colour=args.colour, colour_range=args.range, chroma=args.chroma)
FILTER = {"bilinear": ("bilinear", False), "bilinear_aa": ("bilinear", True), "bicubic_aa": ("bicubic", True)}
RESIZE = dict(mode=FILTER[args.filter][0], antialias=FILTER[args.filter][1], fit=args.fit)
nan = float("nan")
next_round()            # warm-up of the decoders (pinned staging, lanes); its pictures are dropped by the next round
if args.remap:
    remap_legs()
    for d in decs:
        d.close()
    sys.exit(0)
a_ms = a_wall = a_min = nan
if not args.only_b:
    out_a = torch.empty((N, 3, 1080, 1920), dtype=torch.float16, device="cuda")
    a_ms, a_wall, a_min = time_pull(None, out_a)
    del out_a
out_b = torch.empty((N, 3, 224, 224), dtype=torch.float16, device="cuda")
b_ms, b_wall, b_min = time_pull((224, 224), out_b, **RESIZE)
del out_b
torch.cuda.empty_cache()
e_ms = e_wall = e_min = f_ms = nan
if args.regions:
    REGIONS = region_boxes(args.regions)
    e_ms, e_wall, e_min, roi_boxes = time_regions(REGIONS)
    f_ms = time_regions_old(REGIONS, roi_boxes)
d_ms = time_old_aa((224, 224)) if not args.no_old and args.fit == "stretch" else nan
c_a = time_old(None) if not args.no_old and not args.only_b else nan
c_b = time_old((224, 224)) if not args.no_old and not args.only_b else nan
ceiling = copy_ceiling_gbs() if not args.no_old and not args.only_b else nan
moved = N * (8160 * 384 + 3 * 1080 * 1920 * 2)           # tiles read + tensor written (tiles of macroblock rows outside the crop included)
a_gbs = moved / (a_ms * 1e-3) / 1e9
print(json.dumps(dict(streams=N, reps=args.reps, colour=args.colour, range=args.range, chroma=args.chroma, filter=args.filter, fit=args.fit,
                      a_ms=round(a_ms, 3), a_min_ms=round(a_min, 3), a_wall_ms=round(a_wall, 3), a_gbs=round(a_gbs, 1),
                      copy_ceiling_gbs=round(ceiling, 1), a_fraction_of_copy=round(a_gbs / ceiling, 3),
                      b_ms=round(b_ms, 3), b_min_ms=round(b_min, 3), b_wall_ms=round(b_wall, 3),
                      c_a_ms=round(c_a, 2), c_b_ms=round(c_b, 2), d_ms=round(d_ms, 3),
                      speedup_a=round(c_a / a_wall, 1), speedup_b=round(c_b / b_wall, 1),
                      regions=args.regions, e_ms=round(e_ms, 3), e_min_ms=round(e_min, 3), e_wall_ms=round(e_wall, 3), f_ms=round(f_ms, 2),
                      e_ns_per_element=round(e_ms * 1e6 / max(N * args.regions * 3 * ROI_SIZE[0] * ROI_SIZE[1], 1), 5),
                      b_ns_per_element=round(b_ms * 1e6 / (N * 3 * 224 * 224), 5),
                      device_errors=h.device_errors())))
for d in decs:
    d.close()
