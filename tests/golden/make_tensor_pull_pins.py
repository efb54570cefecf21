#!/usr/bin/env python3
"""The pins of the tensor pulls: the SHA-256 of the bytes every pull family writes, for all 30 (dtype, layout, channels, REF)
instantiations of each, on shapes small enough to reach every branch in a few seconds.  tests/test_gpu_tensor_pins.py holds a build
to tensor_pull_pins.json; this file is its generator and holds the one list of cases both use.

The pins are taken from a build whose output is known good (the commit before a refactoring of the pull kernels), on the GPU:

    python3 tests/golden/make_tensor_pull_pins.py            # writes tests/golden/tensor_pull_pins.json
    python3 tests/golden/make_tensor_pull_pins.py --out X    # elsewhere; two runs must give identical files

The crop stream: 80 x 48 coded, cropping window 70 x 42 at (2, 2) — the window starts off a multiple of 8 columns, and its width is
a multiple of neither 8 nor 64 —, BT.709 by the writer's defaults, an intra picture and an inter picture.  Two decoders share every
call: one gives the intra picture, the other the inter picture behind it.  The 640 x 360 cases exist for one branch only: a band
wider than 320 source columns, where the chunk walk of k_tensor_aa / k_tensor_roi takes two chunks and carries partial sums."""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PINS = os.path.join(HERE, "tensor_pull_pins.json")

FAMILIES = ("out", "resize", "aa", "roi", "remap")
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
PAD = (0.25, 114 / 255, 1.0)
FILTERS = {"bilinear": ("bilinear", False), "bilinear_aa": ("bilinear", True), "bicubic_aa": ("bicubic", True)}
WIN_W, WIN_H = 70, 42           # the crop stream's window
SMALL = (19, 37)                # (H, W) of the resized cases on the crop stream
# window-relative (x, y, w, h): inside, an odd origin, across the left / right / top / bottom edge, wholly outside
BOXES = [(8, 6, 40, 30), (13, 7, 31, 21), (-9, 5, 30, 20), (WIN_W - 13, 5, 41, 17), (21, -7, 25, 19), (11, WIN_H - 8, 23, 15),
         (WIN_W + 10, 3, 20, 20)]


def instantiations():
    """the 30 (dtype, layout, channels, colour) a family is compiled for: 3 dtypes x (NCHW: 1, 3 channels; NHWC: 1, 3, 4) x REF"""
    return [(dt, lay, ch, colour) for colour in ("reference", "bt709") for dt in ("u8", "f16", "f32")
            for lay, chs in (("NCHW", ("Y", "RGB")), ("NHWC", ("Y", "RGB", "BGRA"))) for ch in chs]


def cases():
    """every case as (id, family, stream, variant, dtype, layout, channels, colour); the id is the key of the pin file.  variant:
    out: None; resize: None; aa, roi: (filter, fit, (H, W)); remap: (mode, border)"""
    variants = {
        "out": [("crop", None)],
        "resize": [("crop", None)],
        "aa": [("crop", ("bilinear_aa", "stretch", SMALL)), ("crop", ("bicubic_aa", "letterbox", SMALL)),
               ("crop", ("bilinear", "letterbox", SMALL)), ("640x360", ("bicubic_aa", "stretch", (8, 8)))],
        "roi": [("crop", ("bilinear", "stretch", SMALL)), ("crop", ("bilinear_aa", "letterbox", SMALL)),
                ("crop", ("bicubic_aa", "stretch", SMALL)), ("640x360", ("bicubic_aa", "stretch", (8, 8)))],
        "remap": [("crop", (mode, border)) for mode in ("bilinear", "nearest") for border in ("constant", "replicate")],
    }
    out = []
    for family in FAMILIES:
        for stream, v in variants[family]:
            for dt, lay, ch, colour in instantiations():
                what = "" if v is None else "-".join(str(x) for x in v[:2]) + "/"
                out.append((f"{family}/{stream}/{what}{dt}-{lay}-{ch}-{colour}", family, stream, v, dt, lay, ch, colour))
    return out


def crop_stream():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from h264writer import StreamWriter
    w = StreamWriter(wmb=5, hmb=3, n_pics=2, seed=17)
    w.sps["crop"] = (1, 4, 1, 2)        # left, right, top, bottom in units of 2 luma samples
    return w.build()


def remap_map(w, h):
    """a seeded [19, 37, 2] float32 map over a w x h window: fractions inside, then coordinates in (-1, 0), beyond each edge, NaN
    and the infinities"""
    H, W = SMALL
    rng = np.random.default_rng(2030)
    m = np.stack([rng.uniform(0, w - 1, (H, W)), rng.uniform(0, h - 1, (H, W))], axis=-1).astype(np.float32)
    xs = [-0.25, -0.75, -1.0, -3.5, w - 0.5, w, w + 2.25, np.nan, np.inf, -np.inf, 0.0, w - 1, 0.5, w - 1.5]
    ys = [-0.25, -0.75, -1.0, -3.5, h - 0.5, h, h + 2.25, np.nan, np.inf, -np.inf, 0.0, h - 1, 0.5, h - 1.5]
    m[1, :len(xs), 0] = xs
    m[3:3 + len(ys), 2, 1] = ys
    for k, (x, y) in enumerate(zip(xs, ys)):        # both at once: the corners
        m[18, k] = (x, y)
    m[17, 20] = (np.nan, 3.0)
    m[17, 21] = (3.0, np.inf)
    m[17, 22] = (-0.5, h - 0.5)
    m[17, 23] = (w - 0.5, -0.5)
    return m


class _Feed:
    """one decoder (no output reordering) and its private copy of a stream"""

    def __init__(self, h, data):
        self.h, self.data = h, data
        self.buf = ctypes.create_string_buffer(data, len(data))
        self.off = 0
        self.dec = h.Decoder(1)

    def step(self):
        while self.off < len(self.data):
            r, rb = self.dec.decode(ctypes.addressof(self.buf) + self.off, len(self.data) - self.off)
            self.off += rb
            assert r < self.h.H264BSD_ERROR
            if r == self.h.H264BSD_PIC_RDY:
                return True
        return False


class Runner:
    """runs cases against the library `h` (the h264bsd_amd package) and returns the SHA-256 of each output tensor's bytes"""

    def __init__(self, h):
        import torch
        self.h, self.torch = h, torch
        self.data = {"crop": crop_stream(), "640x360": open(os.path.join(HERE, "test_640x360.h264"), "rb").read()}
        self.current = {}           # stream -> two feeds whose current pictures are the first and the second of the stream
        self.maps = None

    def _pair(self, stream, popped):
        """two decoders: the first picture of the stream is the next (or, popped, the current) one of the first, the second
        picture that of the second"""
        a, b = _Feed(self.h, self.data[stream]), _Feed(self.h, self.data[stream])
        assert a.step() and b.step()
        assert b.dec.next_output_info() is not None and b.step()
        if popped:
            assert a.dec.next_output_info() is not None and b.dec.next_output_info() is not None
        return a, b

    def _current(self, stream):
        if stream not in self.current:
            self.current[stream] = self._pair(stream, True)
        return [f.dec for f in self.current[stream]]

    def run(self, case):
        _, family, stream, v, dt, lay, ch, colour = case
        h, torch = self.h, self.torch
        kw = dict(layout=lay, dtype=getattr(torch, {"u8": "uint8", "f16": "float16", "f32": "float32"}[dt]), channels=ch)
        if dt != "u8":
            kw.update(mean=IMAGENET_MEAN, std=IMAGENET_STD)
        if colour != "reference":
            kw.update(colour="bt709", colour_range="full", chroma="bilinear")
        if family in ("out", "resize", "aa"):
            feeds = self._pair(stream, False)
            if family == "out":
                res = h.pull_tensor([f.dec for f in feeds], size=None, **kw)
            elif family == "resize":
                res = h.pull_tensor([f.dec for f in feeds], size=SMALL, mode="bilinear", **kw)
            else:
                mode, aa = FILTERS[v[0]]
                res = h.pull_tensor([f.dec for f in feeds], size=v[2], mode=mode, antialias=aa, fit=v[1], pad=PAD, **kw)
            t, got = res[0], res[1]
        elif family == "roi":
            decs = self._current(stream)
            mode, aa = FILTERS[v[0]]
            boxes = BOXES if stream == "crop" else [(0, 0, 640, 360), (-7, 3, 650, 200)]
            regions = [(i,) + b for i in range(2) for b in boxes]
            t, got = h.pull_regions(decs, regions, v[2], mode=mode, antialias=aa, fit=v[1], pad=PAD, **kw)[:2]
        else:
            decs = self._current(stream)
            if self.maps is None:
                m = torch.from_numpy(remap_map(WIN_W, WIN_H)).cuda()
                torch.cuda.synchronize()
                self.maps = [m, m]
            t, got = h.pull_remap(decs, self.maps, mode=v[0], border=v[1], pad=PAD, **kw)[:2]
        torch.cuda.synchronize()
        assert all(got), case[0]
        digest = hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()
        if family in ("out", "resize", "aa"):
            for f in feeds:
                f.dec.close()
        return digest

    def close(self):
        for pair in self.current.values():
            for f in pair:
                f.dec.close()
        self.current = {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=PINS)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch                    # noqa: F401  (torch's HIP runtime first)
    import h264bsd_amd as h
    h.use_product_library(True)
    run = Runner(h)
    pins, seconds = {}, dict.fromkeys(FAMILIES, 0.0)
    for c in cases():
        t0 = time.perf_counter()
        pins[c[0]] = run.run(c)
        seconds[c[1]] += time.perf_counter() - t0
    run.close()
    print({k: round(v, 2) for k, v in seconds.items()})
    assert h.device_errors() == 0
    with open(args.out, "w") as f:
        json.dump(pins, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(pins), "pins ->", args.out)


if __name__ == "__main__":
    main()
