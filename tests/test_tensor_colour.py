"""h264bsdmiNextOutputTensorBatchColour without a GPU: the ABI (symbol, h264bsdmi_colour_spec's layout), the checks that refuse a
call before anything is popped, the Python argument mapping, and the float64 model (tests/colour_model.py) pinned to the reference's
integer conversion."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import colour_model as cm
from conftest import ROOT
from test_tensor_output import _capture_until_output, _exported, _spec

SYMBOL = "h264bsdmiNextOutputTensorBatchColour"


def test_symbol_is_declared_exported_and_mirrored(built):
    text = open(os.path.join(ROOT, "include", "h264bsd_mi355x.h")).read()
    assert re.search(r"\bint\s+" + SYMBOL + r"\s*\(", text)
    assert SYMBOL in built.EXPORTED_SYMBOLS
    built.lib()
    assert SYMBOL in _exported(built.LIB_PATH)
    assert SYMBOL in _exported(built.capi.BENCH_LIB_PATH)


def test_colour_spec_layout_matches_the_ctypes_mirror(built, tmp_path):
    fields = [f[0] for f in built.ColourSpec._fields_]
    src = tmp_path / "colour.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "h264bsd_mi355x.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(h264bsdmi_colour_spec));\n' +
                   "".join(f'    printf("%zu\\n", offsetof(h264bsdmi_colour_spec, {f}));\n' for f in fields) +
                   '    printf("%d %d %d %d %d %d %d\\n", H264BSDMI_MATRIX_REFERENCE, H264BSDMI_MATRIX_AUTO, H264BSDMI_MATRIX_BT601, '
                   'H264BSDMI_MATRIX_BT709, H264BSDMI_MATRIX_BT2020, H264BSDMI_MATRIX_FCC, H264BSDMI_MATRIX_SMPTE240);\n'
                   '    printf("%d %d %d %d %d\\n", H264BSDMI_RANGE_AUTO, H264BSDMI_RANGE_LIMITED, H264BSDMI_RANGE_FULL, '
                   'H264BSDMI_CHROMA_NEAREST, H264BSDMI_CHROMA_BILINEAR);\n    return 0;\n}\n')
    exe = tmp_path / "colour"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [ctypes.sizeof(built.ColourSpec)] + [getattr(built.ColourSpec, f).offset for f in fields]
    assert got[: len(want)] == want
    m = built.capi.MATRICES
    assert got[len(want):] == [m[k] for k in ("reference", "auto", "bt601", "bt709", "bt2020", "fcc", "smpte240")] + \
        [built.capi.RANGES[k] for k in ("auto", "limited", "full")] + [built.capi.CHROMA[k] for k in ("nearest", "bilinear")]


def _colour(built, matrix=3, range_=0, chroma=0, unspecified=0):
    return built.ColourSpec(matrix, range_, chroma, unspecified)


def _call(built, decoders, spec, colour):
    L = built.api_lib()
    n = len(decoders)
    got = (ctypes.c_uint32 * max(n, 1))()
    dec = (ctypes.c_void_p * max(n, 1))(*[d._st for d in decoders])
    return L.h264bsdmiNextOutputTensorBatchColour(n, dec, ctypes.byref(spec), None if colour is None else ctypes.byref(colour), None,
                                                 got, None, None, None)


GOOD = [None, dict(matrix=0), dict(matrix=1, unspecified=2), dict(matrix=1, unspecified=6, range_=2, chroma=1),
        dict(matrix=2), dict(matrix=3, range_=1), dict(matrix=4, range_=2), dict(matrix=5, chroma=1), dict(matrix=6, unspecified=3)]
BAD = [dict(matrix=7), dict(matrix=99), dict(range_=3), dict(chroma=2), dict(unspecified=1), dict(unspecified=7),
       dict(matrix=1), dict(matrix=1, unspecified=1), dict(matrix=1, unspecified=7),
       dict(matrix=0, range_=1), dict(matrix=0, range_=2), dict(matrix=0, chroma=1), dict(matrix=0, unspecified=2)]


@pytest.mark.parametrize("good", GOOD)
def test_valid_colour_specs_are_accepted(built, good):
    assert _call(built, [], _spec(built), None if good is None else _colour(built, **good)) == 0


@pytest.mark.parametrize("bad", BAD)
def test_invalid_colour_specs_are_refused(built, bad):
    """checked before any instance is looked at: an empty batch with a bad colour spec fails, the same batch without it succeeds"""
    assert _call(built, [], _spec(built), None) == 0
    assert _call(built, [], _spec(built), _colour(built, **bad)) < 0


@pytest.mark.parametrize("spec_bad", [dict(data=0), dict(dtype=3), dict(layout=0, channels=2), dict(std=(1, 0, 1))])
def test_tensor_spec_checks_still_apply(built, spec_bad):
    assert _call(built, [], _spec(built, **spec_bad), _colour(built)) < 0


def test_capture_mode_instance_is_refused_and_keeps_its_picture(built):
    a, keep_a = _capture_until_output(built)
    b, keep_b = _capture_until_output(built)
    assert _call(built, [a], _spec(built), _colour(built, matrix=3, range_=2, chroma=1)) < 0
    assert _call(built, [a], _spec(built, resize=1, width=224, height=224), _colour(built, matrix=1, unspecified=2)) < 0
    info = a.next_output_info()
    assert info is not None and info == b.next_output_info()
    a.close()
    b.close()


@pytest.mark.parametrize("kw", [dict(colour="bt999"), dict(colour="bt709", colour_range="studio"), dict(colour="bt709", chroma="bicubic"),
                                dict(colour="auto", unspecified="auto"), dict(colour="auto", unspecified="reference"),
                                dict(colour_range="full"), dict(chroma="bilinear")])
def test_pull_tensor_refuses_bad_colour_arguments(built, kw):
    """before any device work: names outside the tables, and colour_range / chroma with the reference conversion"""
    with pytest.raises(ValueError):
        built.pull_tensor([], size=(8, 8), **kw)


def test_model_bt601_limited_reproduces_the_reference_conversion():
    """rint(255 v) of the model's BT.601 limited range, nearest chroma, is the reference's integer conversion (the CPU oracle's
    twin of yuv_pixel) within one level in every channel, over all 2^24 (Y, Cb, Cr)"""
    from oracle import pyoracle
    pyoracle.build()
    W = H = 512                                       # chroma 256 x 256: every (Cb, Cr) once; each 2 x 2 luma block 4 Y values
    cb, cr = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="xy")
    worst = 0
    for k in range(64):
        Y = (np.arange(4) * 64 + k).reshape(2, 2)
        y = np.tile(Y, (H // 2, W // 2)).astype(np.uint8)
        frame = np.concatenate([y.ravel(), cb.ravel(), cr.ravel()])
        ref = pyoracle.oracle_convert(0, W, H, frame).view(np.uint8).reshape(H, W, 4)[:, :, :3].astype(np.int64)
        got = np.rint(255 * cm.colour_hwc(frame, (W, H, 0, 0, W, H), "bt601", False, "nearest")).astype(np.int64)
        worst = max(worst, int(np.abs(got - ref).max()))
    assert worst <= 1


def test_model_bilinear_chroma_is_exact_and_clamps_to_the_window():
    """weights 3/4 and 1/4 between rows, 1/2 between columns; the window's edges repeat its own samples"""
    c = np.arange(64, dtype=np.uint8).reshape(8, 8) * 3
    up = cm.upsample(c, 2, 2, 8, 8, "bilinear")        # chroma window rows / columns 1..4
    win = c[1:5, 1:5].astype(np.float64)
    assert up[0, 0] == win[0, 0]                       # top row: the row above is clamped to the window's first
    assert up[1, 0] == 0.75 * win[0, 0] + 0.25 * win[1, 0]
    assert up[2, 0] == 0.75 * win[1, 0] + 0.25 * win[0, 0]
    assert up[2, 1] == 0.75 * (win[1, 0] + win[1, 1]) / 2 + 0.25 * (win[0, 0] + win[0, 1]) / 2
    assert up[7, 7] == win[3, 3]                       # bottom right: clamped in both directions
    assert np.array_equal(cm.upsample(c, 2, 2, 8, 8, "nearest"), np.repeat(np.repeat(win, 2, 0), 2, 1))


def test_model_matrices_keep_grey_grey_and_map_the_range_ends():
    for m in cm.KR_KB:
        for full in (False, True):
            lo, hi = (0, 255) if full else (16, 235)
            v = cm.rgb(np.array([lo, hi, 128]), np.full(3, 128), np.full(3, 128), m, full)
            assert np.allclose(v[0], 0) and np.allclose(v[1], 1) and np.allclose(v[2], v[2][0])
