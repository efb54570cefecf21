"""h264bsdmiOutputTensorRemap without a GPU: the ABI (symbol, the layouts of h264bsdmi_remap and h264bsdmi_remap_spec), the checks
that refuse a call before anything is enqueued, pull_remap's and affine_maps' argument handling, and the float64 model of
tests/remap_model.py held to torch's grid_sample(align_corners=True) and to array slicing / np.rot90."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import remap_model as mm
from conftest import ROOT
from test_tensor_output import _capture_until_output, _exported, _spec
from test_tensor_regions import BAD_COLOUR, BAD_SPEC

SYMBOL = "h264bsdmiOutputTensorRemap"
SENTINEL = 99
MAP = 0x10000          # a well-aligned "device" address: every call here is refused, or samples nothing, before it is read


def test_symbol_is_declared_exported_and_mirrored(built):
    text = open(os.path.join(ROOT, "include", "h264bsd_mi355x.h")).read()
    assert re.search(r"\bint\s+" + SYMBOL + r"\s*\(", text)
    assert "aliases" in text and "NO antialiasing" in text
    assert SYMBOL in built.EXPORTED_SYMBOLS
    built.lib()
    assert SYMBOL in _exported(built.LIB_PATH)
    assert SYMBOL in _exported(built.capi.BENCH_LIB_PATH)
    for name in ("pull_remap", "affine_maps", "Remap", "RemapSpec", "__version__"):
        assert hasattr(built, name), name


def test_struct_layouts_match_the_ctypes_mirrors(built, tmp_path):
    structs = {"h264bsdmi_remap": built.Remap, "h264bsdmi_remap_spec": built.RemapSpec}
    assert [f[0] for f in built.Remap._fields_] == ["instance", "map"]
    assert [f[0] for f in built.RemapSpec._fields_] == ["filter", "border", "pad"]
    lines = []
    for cname, mirror in structs.items():
        lines.append(f'    printf("%zu\\n", sizeof({cname}));\n')
        lines += [f'    printf("%zu\\n", offsetof({cname}, {f[0]}));\n' for f in mirror._fields_]
    src = tmp_path / "remap.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "h264bsd_mi355x.h"\nint main(void) {\n' + "".join(lines) +
                   '    printf("%d %d %d %d\\n", H264BSDMI_REMAP_NEAREST, H264BSDMI_REMAP_BILINEAR, H264BSDMI_BORDER_CONSTANT,'
                   ' H264BSDMI_BORDER_REPLICATE);\n    return 0;\n}\n')
    exe = tmp_path / "remap"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for mirror in structs.values():
        want += [ctypes.sizeof(mirror)] + [getattr(mirror, f[0]).offset for f in mirror._fields_]
    assert got == want + [built.capi.REMAP_FILTERS["nearest"], built.capi.REMAP_FILTERS["bilinear"], built.capi.BORDERS["constant"],
                          built.capi.BORDERS["replicate"]]


def _remap(built, filter_=1, border=0, pad=(0, 0, 0)):
    return built.RemapSpec(filter_, border, (ctypes.c_float * 3)(*pad))


def _call(built, decoders, maps, spec, remap=None, colour=None, null_maps=False, null_got=False, n_maps=None):
    """(rc, got, current, picId) of one raw call; maps: (instance, address); the output arrays start as SENTINEL"""
    L = built.api_lib()
    n, K = len(decoders), len(maps) if n_maps is None else n_maps
    got = (ctypes.c_uint32 * max(K, 1))(*([SENTINEL] * max(K, 1)))
    cur, ids = (ctypes.c_uint32 * max(n, 1))(*([SENTINEL] * max(n, 1))), (ctypes.c_uint32 * max(n, 1))(*([SENTINEL] * max(n, 1)))
    dec = (ctypes.c_void_p * max(n, 1))(*[d._st for d in decoders])
    ms = (built.Remap * max(len(maps), 1))(*[built.Remap(*m) for m in maps])
    rc = L.h264bsdmiOutputTensorRemap(n, dec, K, None if null_maps else ms, ctypes.byref(spec),
                                      None if colour is None else ctypes.byref(colour), None if remap is None else ctypes.byref(remap),
                                      None, None if null_got else got, cur, ids)
    return rc, list(got), list(cur), list(ids)


def _good_spec(built, **kw):
    return _spec(built, resize=1, width=64, height=40, **kw)


GOOD_REMAP = [None, dict(filter_=0), dict(filter_=1), dict(border=1), dict(filter_=0, border=1, pad=(1, 0.5, 0))]
BAD_REMAP = [dict(filter_=2), dict(border=2), dict(filter_=2 ** 32 - 1), dict(pad=(-0.01, 0, 0)), dict(pad=(0, 1.01, 0)),
             dict(pad=(0, 0, math.nan)), dict(pad=(math.inf, 0, 0)), dict(pad=(0, -math.inf, 0))]


@pytest.mark.parametrize("good", GOOD_REMAP)
def test_an_empty_call_with_valid_specs_returns_zero_and_writes_nothing(built, good):
    rc, got, cur, ids = _call(built, [], [], _good_spec(built), None if good is None else _remap(built, **good))
    assert rc == 0 and got == [SENTINEL] and cur == [SENTINEL] and ids == [SENTINEL]
    assert _call(built, [], [], _good_spec(built), None, built.ColourSpec(3, 2, 1, 0))[0] == 0
    assert _call(built, [], [], _good_spec(built), None, None, null_maps=True, null_got=True)[0] == 0


@pytest.mark.parametrize("bad", BAD_REMAP)
def test_invalid_remap_specs_are_refused_before_the_instances(built, bad):
    assert _call(built, [], [], _good_spec(built), _remap(built, **bad))[0] == -1


@pytest.mark.parametrize("bad", BAD_SPEC)
def test_invalid_tensor_specs_are_refused_before_the_instances(built, bad):
    """everything the region call refuses in spec, spec->resize != 1 included"""
    assert _call(built, [], [], _spec(built, **{**dict(resize=1, width=64, height=40), **bad}))[0] == -1
    assert _call(built, [], [], _spec(built, **{**dict(resize=1, width=64, height=40), **bad}), _remap(built))[0] == -1


@pytest.mark.parametrize("bad", BAD_COLOUR)
def test_invalid_colour_specs_are_refused_before_the_instances(built, bad):
    assert _call(built, [], [], _good_spec(built), None, built.ColourSpec(*bad))[0] == -1


def test_map_checks_come_before_the_instances(built):
    """without instances every map names an instance >= n; the grid limit is refused as well"""
    spec = _good_spec(built)
    assert _call(built, [], [(0, MAP)], spec)[0] == -1
    assert _call(built, [], [], spec, n_maps=65536, null_maps=True)[0] == -1


BAD_MAPS = [(1, MAP), (2 ** 32 - 1, MAP), (0, None), (0, MAP + 4), (0, MAP + 1), (0, MAP + 7)]


def test_every_refusal_is_minus_one_and_a_capture_instance_keeps_its_picture(built):
    """a parser-only instance has no pixels: the call is refused whatever the maps; bad maps, NULL arrays, too many maps and
    repeated instances too.  Nothing is written, and the instance's output queue is what an untouched twin's is"""
    a, keep_a = _capture_until_output(built)
    b, keep_b = _capture_until_output(built)
    spec = _good_spec(built)
    untouched = (-1, [SENTINEL], [SENTINEL], [SENTINEL])
    for r in (None, _remap(built, 0), _remap(built, 1, 1, (0.5, 0.5, 0.5))):
        assert _call(built, [a], [(0, MAP)], spec, r) == untouched               # capture mode
    for bad in BAD_MAPS:
        assert _call(built, [a], [bad], spec) == untouched, bad
    for bad in BAD_REMAP:
        assert _call(built, [a], [(0, MAP)], spec, _remap(built, **bad)) == untouched, bad
    assert _call(built, [a], [(0, MAP)], spec, null_maps=True) == untouched
    assert _call(built, [a], [(0, MAP)], spec, null_got=True)[0] == -1
    assert _call(built, [a], [(0, MAP)], spec, n_maps=65536)[0] == -1
    assert _call(built, [a], [], spec)[0] == -1                                  # capture mode, even without maps
    rc, got, cur, ids = _call(built, [a, a], [(0, MAP), (1, MAP)], spec)
    assert rc == -1 and got == [SENTINEL] * 2 and cur == [SENTINEL] * 2          # repeated (and capture mode)
    info = a.next_output_info()
    assert info is not None and info == b.next_output_info()
    a.close()
    b.close()


def test_pull_remap_refuses_maps_it_would_have_to_copy(built):
    """before any device work: maps that are not contiguous float32 device tensors raise ValueError, nothing is converted"""
    import torch
    a, keep = _capture_until_output(built)
    good = torch.zeros((8, 8, 2), dtype=torch.float32)
    for maps in ([good], [good.double()], good[None].expand(1, 8, 8, 2).transpose(1, 2), [np.zeros((8, 8, 2), np.float32)],
                 torch.zeros((8, 8, 2), dtype=torch.float32)):
        with pytest.raises(ValueError):
            built.pull_remap([a], maps)
    for kw in (dict(mode="bicubic"), dict(border="reflect")):
        with pytest.raises(ValueError):
            built.pull_remap([a], [good], **kw)
    a.close()


# ---- the model against torch, float64 ----
def _random_map(rng, H, W, w, h):
    m = np.stack([rng.uniform(-3, w + 2, (H, W)), rng.uniform(-3, h + 2, (H, W))], axis=-1).astype(np.float32)
    m[0, 0] = (-3, h + 2)
    m[0, 1] = (w + 2, -3)
    m[1, 0] = (w - 1, h - 1)
    m[1, 1] = (-1, -1)
    m[2, 0] = (w, h)
    m[2, 1] = (w - 0.5, -0.5)
    return m


@pytest.mark.parametrize("border", ["constant", "replicate"])
@pytest.mark.parametrize("size", [(17, 11), (64, 40)])
def test_model_is_grid_sample_with_align_corners(size, border):
    """random float64 images and maps whose coordinates stay within [-3, W + 2]: CONSTANT with pad 0 is padding_mode="zeros",
    REPLICATE is "border"; within 1e-9"""
    import torch
    import torch.nn.functional as F
    w, h = size
    rng = np.random.default_rng(w * h)
    v = rng.random((h, w, 3))
    for H, W in ((13, 29), (40, 64)):
        m = _random_map(rng, H, W, w, h)
        for fma in (False, True):
            got, padded = mm.remap(v, m, "bilinear", border, fma=fma)
            assert not padded.any()
            gx, gy = 2 * m[:, :, 0].astype(np.float64) / (w - 1) - 1, 2 * m[:, :, 1].astype(np.float64) / (h - 1) - 1
            grid = torch.from_numpy(np.stack([gx, gy], axis=-1))[None]
            want = F.grid_sample(torch.from_numpy(v.transpose(2, 0, 1).copy())[None], grid, mode="bilinear",
                                 padding_mode="zeros" if border == "constant" else "border", align_corners=True)
            assert np.abs(got - want[0].permute(1, 2, 0).numpy()).max() < 1e-9, (size, border, (H, W), fma)


def _grid(H, W):
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return i, j


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_model_identity_translation_and_rotation_are_exact(mode):
    rng = np.random.default_rng(5)
    h, w = 11, 17
    v = rng.random((h, w, 3))
    fill = (0.25, 0.5, 1.0)
    i, j = _grid(h, w)
    ident = np.stack([j, i], axis=-1).astype(np.float32)
    for border in ("constant", "replicate"):
        for fma in (False, True):
            got, padded = mm.remap(v, ident, mode, border, fill, fma)
            assert (got == v).all() and not padded.any()
    for dx, dy in ((3, 2), (-4, 5), (6, -3), (-2, -7), (20, 0), (0, -12)):
        m = np.stack([j + dx, i + dy], axis=-1).astype(np.float32)
        want = np.empty_like(v)
        want[:] = np.asarray(fill)
        ya, yb, xa, xb = max(-dy, 0), min(h - dy, h), max(-dx, 0), min(w - dx, w)
        if ya < yb and xa < xb:
            want[ya:yb, xa:xb] = v[ya + dy:yb + dy, xa + dx:xb + dx]
        assert (mm.remap(v, m, mode, "constant", fill)[0] == want).all(), (dx, dy)
        clamped = v[np.clip(i + dy, 0, h - 1), np.clip(j + dx, 0, w - 1)]
        assert (mm.remap(v, m, mode, "replicate", fill)[0] == clamped).all(), (dx, dy)
    # np.rot90 (counter-clockwise): out[i, j] = v[j, w - 1 - i], an output of w rows x h columns
    i, j = _grid(w, h)
    rot = np.stack([w - 1 - i, j], axis=-1).astype(np.float32)
    assert (mm.remap(v, rot, mode, "constant", fill)[0] == np.rot90(v)).all()


def test_model_special_values():
    """non-finite coordinates are padded; huge finite ones clamp to outside (CONSTANT: the fill) or to the edge (REPLICATE); -1 and w
    are outside, -0.5 and w - 0.5 blend half of the fill in"""
    v = np.arange(12, dtype=np.float64).reshape(3, 4, 1) + 1
    fill = (100.0,) * 3
    xs = [np.nan, np.inf, -np.inf, 1e30, -1e30, -1, -0.5, 3, 3.5, 4, 1.5]
    m = np.stack([np.asarray(xs, np.float32), np.zeros(len(xs), np.float32)], axis=-1)[None]
    got, padded = mm.remap(v, m, "bilinear", "constant", fill)
    assert list(padded[0]) == [True] * 3 + [False] * 8
    assert list(got[0, 3:, 0]) == [100, 100, 100, 50.5, 4, 52, 100, 2.5]
    got, padded = mm.remap(v, m, "bilinear", "replicate", fill)
    assert list(padded[0]) == [True] * 3 + [False] * 8
    assert list(got[0, 3:, 0]) == [4, 1, 1, 1, 4, 4, 4, 2.5]
    got, _ = mm.remap(v, m, "nearest", "constant", fill)
    assert list(got[0, 3:, 0]) == [100, 100, 100, 1, 4, 100, 100, 3]      # -0.5 -> 0, 3.5 -> 4 (outside), 1.5 -> 2
    ymap = np.stack([np.zeros(2, np.float32), np.asarray([np.nan, 1.0], np.float32)], axis=-1)[None]
    assert list(mm.remap(v, ymap, "nearest", "replicate", fill)[1][0]) == [True, False]


def test_near_rounding_boundary():
    assert list(mm.near_rounding_boundary(np.asarray([0.5, 0.499, 0.497, 7.5015, 7.503, 254.0]))) == [True, True, False, True, False, False]


def test_affine_maps_gives_the_expected_coordinates(built):
    import torch
    theta = [[[1, 0, 0], [0, 1, 0]], [[0, -1, 16], [1, 0, 0]], [[0.5, 0.25, -3.125], [-0.75, 2, 1e-3]]]
    maps = built.affine_maps(theta, (5, 7), device="cpu")
    assert maps.dtype == torch.float32 and tuple(maps.shape) == (3, 5, 7, 2) and maps.is_contiguous()
    m = maps.numpy()
    i, j = _grid(5, 7)
    assert (m[0, :, :, 0] == j).all() and (m[0, :, :, 1] == i).all()
    assert (m[1, :, :, 0] == 16 - i).all() and (m[1, :, :, 1] == j).all()
    want = np.stack([0.5 * j + 0.25 * i - 3.125, -0.75 * j + 2.0 * i + 1e-3], axis=-1).astype(np.float32)      # float64, rounded once
    assert (m[2] == want).all()
    assert tuple(built.affine_maps(torch.tensor(theta[:1]), 4, device="cpu").shape) == (1, 4, 4, 2)
    for bad in ([[1, 0, 0], [0, 1, 0]], [[[1, 0], [0, 1]]]):
        with pytest.raises(ValueError):
            built.affine_maps(bad, (5, 7), device="cpu")


def test_kernel_header_and_its_resource_profile():
    """k_tensor_remap lives in a header of its own, included after k_tensor_roi's and outside the sources that key the counter
    tables; the committed tools/kres.sh profile lists all 30 instantiations without scratch or spills"""
    from h264bsd_amd import srchash
    engine = open(os.path.join(ROOT, "h264bsd_amd", "csrc", "engine.hip")).read()
    assert 0 < engine.index('#include "kernels/k_tensor_roi.hip.h"') < engine.index('#include "kernels/k_tensor_remap.hip.h"')
    assert "k_tensor_remap" not in open(os.path.join(ROOT, "h264bsd_amd", "csrc", "kernels.hip.h")).read()
    assert not any("k_tensor" in f for f in srchash._FILES)
    rows = [line.split() for line in open(os.path.join(ROOT, "profiles", "tensor_remap_kres.txt"))
            if "k_tensor_remap" in line and not line.startswith("#")]
    assert len(rows) == 30 and len({r[0] for r in rows}) == 30
    for name, vgpr, sgpr, vspill, sspill, scratch, occ in rows:
        assert int(scratch) == 0 and int(vspill) == 0 and int(sspill) == 0 and int(vgpr) <= 128, name
