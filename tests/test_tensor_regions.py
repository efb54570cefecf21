"""h264bsdmiOutputTensorRegions without a GPU: the ABI (symbol, h264bsdmi_region's layout), the checks that refuse a call before
anything is enqueued, pull_regions' argument checks, and the float64 model of a region (tests/region_model.py: convert, pad, crop,
resample) held to torch's F.pad -> slice -> F.interpolate."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import region_model as gm
from conftest import ROOT
from test_tensor_output import _capture_until_output, _exported, _spec

SYMBOL = "h264bsdmiOutputTensorRegions"
LIMIT = 16384


def test_symbol_is_declared_exported_and_mirrored(built):
    text = open(os.path.join(ROOT, "include", "h264bsd_mi355x.h")).read()
    assert re.search(r"\bint\s+" + SYMBOL + r"\s*\(", text)
    assert SYMBOL in built.EXPORTED_SYMBOLS
    built.lib()
    assert SYMBOL in _exported(built.LIB_PATH)
    assert SYMBOL in _exported(built.capi.BENCH_LIB_PATH)
    assert hasattr(built, "pull_regions") and hasattr(built, "Region")


def test_region_layout_matches_the_ctypes_mirror(built, tmp_path):
    fields = [f[0] for f in built.Region._fields_]
    assert fields == ["instance", "x", "y", "w", "h"]
    src = tmp_path / "region.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "h264bsd_mi355x.h"\nint main(void) {\n'
                   '    h264bsdmi_region r = { 0, -1, -1, 0, 0 };\n'
                   '    printf("%zu\\n", sizeof(h264bsdmi_region));\n' +
                   "".join(f'    printf("%zu\\n", offsetof(h264bsdmi_region, {f}));\n' for f in fields) +
                   '    printf("%d %d\\n", r.x < 0, r.y < 0);\n    return 0;\n}\n')
    exe = tmp_path / "region"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(built.Region)] + [getattr(built.Region, f).offset for f in fields] + [1, 1]     # x, y are signed
    r = built.Region(3, -5, -7, 9, 11)
    assert (r.instance, r.x, r.y, r.w, r.h) == (3, -5, -7, 9, 11)


def _resize(built, filter_=1, fit=0, pad=(0, 0, 0)):
    return built.ResizeSpec(filter_, fit, (ctypes.c_float * 3)(*pad))


SENTINEL = 99


def _call(built, decoders, regions, spec, resize=None, colour=None, null_regions=False, null_got=False, n_regions=None):
    """(rc, got, box, current, picId) of one raw call; the output arrays start as SENTINEL"""
    L = built.api_lib()
    n, K = len(decoders), len(regions) if n_regions is None else n_regions
    got, box = (ctypes.c_uint32 * max(K, 1))(*([SENTINEL] * max(K, 1))), (ctypes.c_uint32 * max(4 * K, 4))(*([SENTINEL] * max(4 * K, 4)))
    cur, ids = (ctypes.c_uint32 * max(n, 1))(*([SENTINEL] * max(n, 1))), (ctypes.c_uint32 * max(n, 1))(*([SENTINEL] * max(n, 1)))
    dec = (ctypes.c_void_p * max(n, 1))(*[d._st for d in decoders])
    regs = (built.Region * max(len(regions), 1))(*[built.Region(*r) for r in regions])
    rc = L.h264bsdmiOutputTensorRegions(n, dec, K, None if null_regions else regs, ctypes.byref(spec),
                                        None if colour is None else ctypes.byref(colour), None if resize is None else ctypes.byref(resize),
                                        None, None if null_got else got, box, cur, ids)
    return rc, list(got), list(box), list(cur), list(ids)


def _good_spec(built, **kw):
    return _spec(built, resize=1, width=128, height=256, **kw)


GOOD_RESIZE = [None, dict(filter_=0), dict(filter_=1), dict(filter_=2), dict(filter_=0, fit=1), dict(filter_=2, fit=1, pad=(1, 0.5, 0))]
BAD_RESIZE = [dict(filter_=3), dict(fit=2), dict(pad=(-0.01, 0, 0)), dict(pad=(0, 1.01, 0)), dict(pad=(0, 0, math.nan)),
              dict(pad=(math.inf, 0, 0))]
BAD_SPEC = [dict(data=0), dict(width=0), dict(height=0), dict(dtype=3), dict(layout=2), dict(channels=5), dict(layout=0, channels=2),
            dict(std=(1, 0, 1)), dict(dtype=0, mean=(0.5, 0, 0)), dict(resize=0), dict(resize=2)]
BAD_COLOUR = [(7, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (1, 0, 0, 0), (3, 3, 0, 0), (3, 0, 2, 0), (3, 0, 0, 1)]


@pytest.mark.parametrize("good", GOOD_RESIZE)
def test_an_empty_call_with_valid_specs_is_accepted(built, good):
    """no instances, no regions: the specs are all there is to check; nothing is written"""
    rc, got, box, cur, ids = _call(built, [], [], _good_spec(built), None if good is None else _resize(built, **good))
    assert rc == 0 and got == [SENTINEL] and box == [SENTINEL] * 4
    assert _call(built, [], [], _good_spec(built), None, built.ColourSpec(3, 2, 1, 0))[0] == 0
    assert _call(built, [], [], _good_spec(built), None, None, null_regions=True, null_got=True)[0] == 0


@pytest.mark.parametrize("bad", BAD_RESIZE)
def test_invalid_resize_specs_are_refused_before_the_instances(built, bad):
    assert _call(built, [], [], _good_spec(built), _resize(built, **bad))[0] == -1


@pytest.mark.parametrize("bad", BAD_SPEC)
def test_invalid_tensor_specs_are_refused_before_the_instances(built, bad):
    """everything the resize call refuses, and spec->resize != 1 even without a resize spec"""
    assert _call(built, [], [], _spec(built, **{**dict(resize=1, width=128, height=256), **bad}))[0] == -1
    assert _call(built, [], [], _spec(built, **{**dict(resize=1, width=128, height=256), **bad}), _resize(built))[0] == -1


@pytest.mark.parametrize("bad", BAD_COLOUR)
def test_invalid_colour_specs_are_refused_before_the_instances(built, bad):
    assert _call(built, [], [], _good_spec(built), None, built.ColourSpec(*bad))[0] == -1


def test_region_checks_come_before_the_instances(built):
    """without instances every region names an instance >= n; NULL arrays and the grid limit are refused as well"""
    spec = _good_spec(built)
    assert _call(built, [], [(0, 0, 0, 16, 16)], spec)[0] == -1
    assert _call(built, [], [], spec, n_regions=65536, null_regions=True)[0] == -1


BAD_REGIONS = [(1, 0, 0, 16, 16), (2 ** 32 - 1, 0, 0, 16, 16), (0, 0, 0, 0, 16), (0, 0, 0, 16, 0), (0, 0, 0, LIMIT + 1, 16),
               (0, 0, 0, 16, LIMIT + 1), (0, LIMIT + 1, 0, 16, 16), (0, -LIMIT - 1, 0, 16, 16), (0, 0, LIMIT + 1, 16, 16),
               (0, 0, -LIMIT - 1, 16, 16), (0, -2 ** 31, 0, 16, 16)]


def test_every_refusal_is_minus_one_and_a_capture_instance_keeps_its_picture(built):
    """a parser-only instance has no pixels: the call is refused whatever the regions, bad regions, NULL arrays, too many regions and
    repeated instances included; nothing is written, and the instance's output queue is what an untouched twin's is"""
    a, keep_a = _capture_until_output(built)
    b, keep_b = _capture_until_output(built)
    spec = _good_spec(built)
    untouched = (-1, [SENTINEL], [SENTINEL] * 4, [SENTINEL], [SENTINEL])
    for good in [(0, 0, 0, 16, 16), (0, -5, 3, 17, 31), (0, LIMIT, -LIMIT, LIMIT, LIMIT)]:
        for r in (None, _resize(built, 1), _resize(built, 2, 1, (0.5, 0.5, 0.5))):
            assert _call(built, [a], [good], spec, r) == untouched          # capture mode
    for bad in BAD_REGIONS:
        assert _call(built, [a], [bad], spec) == untouched, bad
    assert _call(built, [a], [(0, 0, 0, 16, 16)], spec, null_regions=True) == untouched
    assert _call(built, [a], [(0, 0, 0, 16, 16)], spec, null_got=True)[0] == -1
    assert _call(built, [a], [(0, 0, 0, 16, 16)], spec, n_regions=65536)[0] == -1
    assert _call(built, [a], [], spec)[0] == -1                              # capture mode, even without regions
    rc, got, box, cur, ids = _call(built, [a, a], [(0, 0, 0, 16, 16), (1, 0, 0, 16, 16)], spec)
    assert rc == -1 and got == [SENTINEL] * 2 and cur == [SENTINEL] * 2     # repeated (and capture mode)
    info = a.next_output_info()
    assert info is not None and info == b.next_output_info()
    a.close()
    b.close()


@pytest.mark.parametrize("kw", [dict(mode="bicubic"), dict(mode="nearest"), dict(fit="crop"), dict(pad=(0, 0, 1.5)), dict(pad=(0, 0)),
                                dict(layout="CHWN"), dict(channels="GBR"), dict(colour="bt470"), dict(colour="reference", chroma="bilinear"),
                                dict(size=None), dict(regions=[(0, 0, 0, 0, 8)]), dict(regions=[(0, 0, 0, 8, LIMIT + 1)]),
                                dict(regions=[(0, -LIMIT - 1, 0, 8, 8)]), dict(regions=[(0, 0.5, 0, 8, 8)]), dict(regions=[(0, 0, 0, 8)]),
                                dict(regions=[(1, 0, 0, 8, 8)]), dict(regions=[(-1, 0, 0, 8, 8)]), dict(regions=[(0, 0, 0, 8, 8)] * 65536)])
def test_pull_regions_refuses_bad_arguments(built, kw):
    """before any device work: pull_tensor's checks, a missing size, and regions that are not five host integers in range"""
    a, keep = _capture_until_output(built)
    args = dict(regions=[(0, 0, 0, 8, 8)], size=(8, 8))
    args.update(kw)
    with pytest.raises(ValueError):
        built.pull_regions([a], args.pop("regions"), args.pop("size"), **args)
    a.close()


# ---- the model against torch, float64 ----
BOXES = {"inside, odd origin and size": (7, 5, 33, 21), "whole window": (0, 0, 80, 45), "left edge": (-9, 10, 30, 20),
         "right edge": (61, 3, 41, 17), "top edge": (20, -7, 25, 19), "bottom edge": (11, 38, 23, 15), "corner": (-6, -11, 29, 31),
         "far corner": (70, 40, 35, 27), "around the window": (-10, -10, 100, 65), "wholly outside": (90, 50, 20, 20),
         "wholly outside, left": (-40, 5, 40, 9), "one sample": (79, 44, 1, 1)}
SIZES = [(17, 29), (64, 48), (8, 8), (45, 80), (1, 3)]


def _torch_region(v, box, size, fill, mode, antialias):
    import torch
    import torch.nn.functional as F
    x, y, w, h = box
    wh, ww, C = v.shape
    l, r, t, b = max(-x, 0), max(x + w - ww, 0), max(-y, 0), max(y + h - wh, 0)
    chans = []
    for c in range(C):          # F.pad takes one constant: per channel
        p = F.pad(torch.from_numpy(np.ascontiguousarray(v[:, :, c]))[None, None], (l, r, t, b), mode="constant", value=float(fill[c]))
        chans.append(p[:, :, y + t:y + t + h, x + l:x + l + w])
    s = torch.cat(chans, dim=1)
    if s.shape[2] != h or s.shape[3] != w:       # a box beyond the padded picture altogether
        s = torch.from_numpy(np.broadcast_to(np.asarray(fill[:C], np.float64)[None, :, None, None], (1, C, h, w)).copy())
    return F.interpolate(s, size=size, mode=mode, antialias=antialias, align_corners=False)[0].permute(1, 2, 0).numpy()


@pytest.mark.parametrize("name", list(BOXES))
@pytest.mark.parametrize("filt", ["bilinear_aa", "bicubic_aa"])
def test_model_is_pad_crop_interpolate_in_torch(filt, name):
    """F.pad(picture, constant) -> slice -> F.interpolate(antialias=True) in float64, up- and downscaling, within 1e-12"""
    rng = np.random.default_rng(11)
    v = rng.random((45, 80, 3))
    fill = (0.25, 114 / 255, 1.0)
    box = BOXES[name]
    for size in SIZES:
        rect, got = gm.region(v, box, size, filt, fill=fill)
        assert rect == (0, 0, size[1], size[0])
        want = _torch_region(v, box, size, fill, filt[:-3], True)
        assert np.abs(got - want).max() < 1e-12, (name, size)
        if gm.whole_outside(box, 80, 45):
            assert np.abs(got - np.asarray(fill)[None, None, :]).max() < 1e-12


@pytest.mark.parametrize("name", list(BOXES))
def test_model_bilinear_without_antialias_is_torchs(name):
    """within 1e-4 of full scale: the model computes the source coordinate in fp32 as the kernels do, torch rounds its own differently"""
    rng = np.random.default_rng(12)
    v = rng.random((45, 80, 3))
    fill = (0.5, 0.0, 1.0)
    for size in SIZES:
        _, got = gm.region(v, BOXES[name], size, "bilinear", fill=fill)
        want = _torch_region(v, BOXES[name], size, fill, "bilinear", False)
        assert np.abs(got - want).max() < 1e-4, (name, size)


def test_model_letterbox_is_the_boxs_not_the_windows():
    rng = np.random.default_rng(13)
    v = rng.random((45, 80, 1))
    rect, got = gm.region(v, (-5, 3, 30, 60), (256, 128), "bilinear_aa", fit="letterbox", fill=(0.5,) * 3)
    assert rect == (0, 0, 128, 256) and got.shape == (256, 128, 1)
    rect, got = gm.region(v, (10, 10, 40, 20), (256, 128), "bicubic_aa", fit="letterbox")
    assert rect == (0, 96, 128, 64) and got.shape == (64, 128, 1)


def test_model_sample_pad():
    assert list(gm.sample_pad((0.0, 0.5, 1.0), True)) == [0.0, 128.0, 255.0]
    assert list(gm.sample_pad((0.0, 0.5, 1.0), False)) == [0.0, 0.5, 1.0]


def test_kernel_header_and_its_resource_profile():
    """k_tensor_roi lives in a header of its own, included after k_tensor_aa's and outside the sources that key the counter tables;
    the committed tools/kres.sh profile lists all 30 instantiations without scratch or vector spills"""
    from h264bsd_amd import srchash
    engine = open(os.path.join(ROOT, "h264bsd_amd", "csrc", "engine.hip")).read()
    assert 0 < engine.index('#include "kernels/k_tensor_aa.hip.h"') < engine.index('#include "kernels/k_tensor_roi.hip.h"')
    assert not any("k_tensor" in f for f in srchash._FILES)
    rows = [line.split() for line in open(os.path.join(ROOT, "profiles", "tensor_roi_kres.txt")) if "k_tensor_roi" in line and not line.startswith("#")]
    assert len(rows) == 30 and len({r[0] for r in rows}) == 30
    for name, vgpr, sgpr, vspill, sspill, scratch, occ in rows:
        assert int(scratch) == 0 and int(vspill) == 0 and int(vgpr) <= 128, name
