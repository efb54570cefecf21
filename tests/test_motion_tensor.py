"""Motion export without a GPU: the ABI of h264bsdmiSetMotionExport / h264bsdmiOutputMotionRegions (symbols, h264bsdmi_motion_spec's
layout), every refusal that comes before anything is enqueued, pull_motion's argument checks, and the model of
tests/motion_model.py held to itself where two of its paths must agree."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import motion_model as mm
from conftest import ROOT
from test_tensor_output import _capture_until_output, _exported

SYMBOLS = ["h264bsdmiSetMotionExport", "h264bsdmiOutputMotionRegions"]
LIMIT = 16384
SENTINEL = 99


def test_symbols_are_declared_exported_and_mirrored(built):
    text = open(os.path.join(ROOT, "include", "h264bsd_mi355x.h")).read()
    built.lib()
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+" + sym + r"\s*\(", text)
        assert sym in built.EXPORTED_SYMBOLS
        assert sym in _exported(built.LIB_PATH)
        assert sym in _exported(built.capi.BENCH_LIB_PATH)
    assert hasattr(built, "pull_motion") and hasattr(built, "MotionSpec")
    for name, value in [("H264BSDMI_MOTION_NEAREST", 0), ("H264BSDMI_MOTION_AREA", 1), ("H264BSDMI_MOTION_PLANE_MV", 1),
                        ("H264BSDMI_MOTION_PLANE_VALID", 2), ("H264BSDMI_MOTION_PLANE_AGE", 4), ("H264BSDMI_MOTION_PLANE_QP", 8),
                        ("H264BSDMI_MOTION_UNITS_SOURCE", 0), ("H264BSDMI_MOTION_UNITS_OUTPUT", 1)]:
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"u?\b", text), name
    assert built.capi.MOTION_PLANES == {"mv": (1, 2), "valid": (2, 1), "age": (4, 1), "qp": (8, 1)}


def test_motion_spec_layout_matches_the_ctypes_mirror(built, tmp_path):
    fields = [f[0] for f in built.MotionSpec._fields_]
    assert fields == ["data", "width", "height", "layout", "dtype", "planes", "crop", "fit", "sampler", "units", "per_picture"]
    src = tmp_path / "spec.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "h264bsd_mi355x.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(h264bsdmi_motion_spec));\n' +
                   "".join(f'    printf("%zu\\n", offsetof(h264bsdmi_motion_spec, {f}));\n' for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "spec"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(built.MotionSpec)] + [getattr(built.MotionSpec, f).offset for f in fields]


def _spec(built, **kw):
    s = dict(data=0x1000, width=128, height=96, layout=0, dtype=2, planes=3, crop=1, fit=0, sampler=0, units=0, per_picture=0)
    s.update(kw)
    return built.MotionSpec(*[s[f[0]] for f in built.MotionSpec._fields_])


def _call(built, decoders, regions, spec, null_regions=False, null_got=False, n_regions=None):
    """(rc, got, box, current, picId) of one raw call; the output arrays start as SENTINEL"""
    L = built.api_lib()
    n, K = len(decoders), len(regions) if n_regions is None else n_regions
    got, box = (ctypes.c_uint32 * max(K, 1))(*([SENTINEL] * max(K, 1))), (ctypes.c_uint32 * max(4 * K, 4))(*([SENTINEL] * max(4 * K, 4)))
    cur, ids = (ctypes.c_uint32 * max(n, 1))(*([SENTINEL] * max(n, 1))), (ctypes.c_uint32 * max(n, 1))(*([SENTINEL] * max(n, 1)))
    dec = (ctypes.c_void_p * max(n, 1))(*[d._st for d in decoders])
    regs = (built.Region * max(len(regions), 1))(*[built.Region(*r) for r in regions])
    rc = L.h264bsdmiOutputMotionRegions(n, dec, K, None if null_regions else regs, ctypes.byref(spec), None,
                                        None if null_got else got, box, cur, ids)
    return rc, list(got), list(box), list(cur), list(ids)


def test_an_empty_call_with_a_valid_spec_is_accepted(built):
    for good in [dict(), dict(dtype=1, layout=1), dict(planes=15), dict(planes=8), dict(fit=1, sampler=1, units=1, per_picture=1)]:
        rc, got, box, cur, ids = _call(built, [], [], _spec(built, **good))
        assert rc == 0 and got == [SENTINEL] and box == [SENTINEL] * 4, good
    assert _call(built, [], [], _spec(built), null_regions=True, null_got=True)[0] == 0       # regions == NULL, nRegions == n == 0


BAD_SPEC = [dict(data=0), dict(width=0), dict(height=0), dict(layout=2), dict(dtype=0), dict(dtype=3), dict(planes=0), dict(planes=16),
            dict(planes=3 | 32), dict(fit=2), dict(sampler=2), dict(units=2), dict(per_picture=2)]


@pytest.mark.parametrize("bad", BAD_SPEC)
def test_invalid_specs_are_refused_before_the_instances(built, bad):
    assert _call(built, [], [], _spec(built, **bad))[0] == -1


BAD_REGIONS = [(1, 0, 0, 16, 16), (2 ** 32 - 1, 0, 0, 16, 16), (0, 0, 0, 0, 16), (0, 0, 0, 16, 0), (0, 0, 0, LIMIT + 1, 16),
               (0, 0, 0, 16, LIMIT + 1), (0, LIMIT + 1, 0, 16, 16), (0, -LIMIT - 1, 0, 16, 16), (0, 0, LIMIT + 1, 16, 16),
               (0, 0, -LIMIT - 1, 16, 16), (0, -2 ** 31, 0, 16, 16)]


def test_every_refusal_is_minus_one_and_nothing_is_written_or_popped(built):
    """a parser-only instance has no device to keep motion on: h264bsdmiSetMotionExport refuses it, before and after it has decoded,
    and so every pull is refused — whatever else is wrong with it; the sentinels stay, and the instance's output queue is what an
    untouched twin's is"""
    L = built.api_lib()
    fresh = built.Decoder(capture="discard")
    assert L.h264bsdmiSetMotionExport(fresh._st, 1) == -1 and L.h264bsdmiSetMotionExport(fresh._st, 0) == -1
    assert L.h264bsdmiSetMotionExport(None, 1) == -1
    fresh.close()
    with pytest.raises(RuntimeError):
        built.Decoder(capture="discard", motion=True)
    a, keep_a = _capture_until_output(built)
    b, keep_b = _capture_until_output(built)
    assert L.h264bsdmiSetMotionExport(a._st, 1) == -1                        # has decoded already (and capture mode)
    spec = _spec(built)
    untouched = (-1, [SENTINEL], [SENTINEL] * 4, [SENTINEL], [SENTINEL])
    for good in [(0, 0, 0, 16, 16), (0, -5, 3, 17, 31), (0, LIMIT, -LIMIT, LIMIT, LIMIT)]:
        for kw in (dict(), dict(fit=1, sampler=1), dict(planes=15, dtype=1, layout=1)):
            assert _call(built, [a], [good], _spec(built, **kw)) == untouched
    for bad in BAD_REGIONS:
        assert _call(built, [a], [bad], spec) == untouched, bad
    for bad in BAD_SPEC:
        assert _call(built, [a], [(0, 0, 0, 16, 16)], _spec(built, **bad)) == untouched, bad
    assert _call(built, [a], [(0, 0, 0, 16, 16)], spec, null_regions=True) == untouched      # whole windows, but no motion export
    assert _call(built, [a], [(0, 0, 0, 16, 16)] * 2, spec, null_regions=True)[0] == -1      # regions == NULL with nRegions != n
    assert _call(built, [a], [(0, 0, 0, 16, 16)], spec, null_got=True)[0] == -1
    assert _call(built, [a], [(0, 0, 0, 16, 16)], spec, n_regions=65536)[0] == -1
    assert _call(built, [a], [], spec)[0] == -1
    rc, got, box, cur, ids = _call(built, [a, a], [(0, 0, 0, 16, 16), (1, 0, 0, 16, 16)], spec)
    assert rc == -1 and got == [SENTINEL] * 2 and cur == [SENTINEL] * 2
    info = a.next_output_info()
    assert info is not None and info == b.next_output_info()
    a.close()
    b.close()


@pytest.mark.parametrize("kw", [dict(dtype="u8"), dict(layout="CHWN"), dict(planes=()), dict(planes=("mv", "flow")), dict(fit="crop"),
                                dict(sampler="bilinear"), dict(units="pixels"), dict(size=None), dict(regions=[(0, 0, 0, 0, 8)]),
                                dict(regions=[(0, 0, 0, 8, LIMIT + 1)]), dict(regions=[(0, 0.5, 0, 8, 8)]), dict(regions=[(1, 0, 0, 8, 8)]),
                                dict(regions=[(0, 0, 0, 8, 8)] * 65536)])
def test_pull_motion_refuses_bad_arguments(built, kw):
    """before any device work: names that are not in the tables, regions that are not five host integers in range, regions
    without a size"""
    import torch
    a, keep = _capture_until_output(built)
    args = dict(regions=[(0, 0, 0, 8, 8)], size=(8, 8))
    args.update(kw)
    if args.get("dtype") == "u8":
        args["dtype"] = torch.uint8
    with pytest.raises(ValueError):
        built.pull_motion([a], **args)
    a.close()


# ---- the model against itself ----
def _random_side(rng, hmb, wmb):
    hb4, wb4 = 4 * hmb, 4 * wmb
    valid = np.repeat(np.repeat(rng.random((2 * hmb, 2 * wmb)) < 0.8, 2, 0), 2, 1)
    age = np.repeat(np.repeat(rng.integers(0, 6, (2 * hmb, 2 * wmb)), 2, 0), 2, 1) * valid
    mv = rng.integers(-200, 200, (hb4, wb4, 2)) * valid[..., None]
    qp = np.repeat(np.repeat(rng.integers(10, 52, (hmb, wmb)), 4, 0), 4, 1)
    return mm.Side(mv.astype(np.int16), valid, age.astype(np.uint8), qp.astype(np.uint8), np.zeros((hmb, wmb), np.uint8), 0, 0, 1)


@pytest.mark.parametrize("opts", [dict(), dict(per_picture=True), dict(units="output"), dict(per_picture=True, units="output")])
def test_area_at_the_native_grid_of_an_aligned_window_is_nearest(opts):
    """one output pixel per 4x4 block, footprint = the block: the weighted mean over one block is the block"""
    side = _random_side(np.random.default_rng(1), 6, 10)
    for window in [(0, 0, 160, 96), (16, 8, 128, 80), (0, 0, 156, 90)]:      # the last one: a partial block column and row at the end
        size = mm.native_size(window)
        box = (0, 0, 4 * size[1], 4 * size[0])                               # the grid's own extent: it may end beyond the window
        rn, near, _ = mm.motion_region(side, window, box, size, sampler="nearest", **opts)
        ra, area, _ = mm.motion_region(side, window, box, size, sampler="area", **opts)
        assert rn == ra == (0, 0, size[1], size[0])
        full = np.ones(size, bool)
        full[:, -1] = window[2] % 4 == 0
        full[-1, :] &= window[3] % 4 == 0
        assert np.array_equal(near[full], area[full])
        if window[3] % 4 == 2:
            # the last block row has two of its four sample rows inside the window: its centre (NEAREST) lies outside, AREA sees
            # the clipped footprint, and its VALID is half of what the block row above the edge would give alone
            assert not near[-1].any()
            ky, kx0 = (window[1] + window[3]) >> 2, window[0] >> 2
            assert np.array_equal(area[-1, :, 2], 0.5 * side.valid[ky, kx0:kx0 + size[1]])


def test_area_valid_of_a_box_half_outside_the_window_is_half():
    side = _random_side(np.random.default_rng(2), 4, 4)
    window = (0, 0, 64, 64)
    _, inside, _ = mm.motion_region(side, window, (0, 0, 32, 64), (1, 1), sampler="area", planes=("valid",))
    _, half, _ = mm.motion_region(side, window, (-32, 0, 64, 64), (1, 1), sampler="area", planes=("valid",))
    assert inside[0, 0, 0] > 0 and half[0, 0, 0] == 0.5 * inside[0, 0, 0]
    _, out, _ = mm.motion_region(side, window, (64, 0, 16, 16), (2, 2), sampler="area")
    assert not out.any()


def test_outside_the_window_and_outside_the_rectangle_is_zero():
    side = _random_side(np.random.default_rng(3), 4, 6)
    window = (0, 0, 96, 64)
    for sampler in ("nearest", "area"):
        rect, v, _ = mm.motion_region(side, window, (-20, -10, 60, 30), (32, 32), fit="letterbox", sampler=sampler)
        assert rect == (0, 8, 32, 16)
        assert not v[:8].any() and not v[24:].any()
        assert not v[8:8 + 5, :].any() and not v[:, :10].any()               # rows above y = 0, columns left of x = 0
        assert v[8 + 6:, 11:].any()


def test_side_info_of_the_bundled_stream(built, captured):
    """the first picture is an IDR picture: every block invalid, no vector, no age; later pictures move, every valid block from a
    picture decoded before it (age >= 1, and never further back than the pictures there are), and P_Skip macroblocks are valid like
    every other inter macroblock"""
    jobs, _, info = captured("test_640x360")
    sides = mm.side_info(jobs)
    assert len(sides) == len([j for j in jobs if not built.job_header(j)["ghost"]])
    first = sides[0]
    assert first.valid.shape == (4 * info["height_mbs"], 4 * info["width_mbs"]) == (92, 160)
    assert not first.valid.any() and not first.mv.any() and not first.age.any()
    assert first.qp.any()
    later = sides[1:12]
    assert all(s.valid.any() for s in later) and any(s.mv.any() for s in later)
    for k, s in enumerate(later, 1):
        assert 1 <= s.age[s.valid].min() and s.age[s.valid].max() <= k
        assert not s.mv[~s.valid].any() and not s.age[~s.valid].any()
        assert np.array_equal(np.repeat(np.repeat(np.isin(s.kind, (0, 5)), 4, 0), 4, 1), s.valid)
