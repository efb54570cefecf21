"""h264bsdmiNextOutputTensorBatchResize without a GPU: the ABI (symbol, h264bsdmi_resize_spec's layout), the checks that refuse a
call before anything is popped, pull_tensor's argument checks, and the float64 model of the weights and the letterbox geometry
(tests/resize_model.py) held to torch's F.interpolate(antialias=True)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import resize_model as rm
from conftest import ROOT
from test_tensor_output import _capture_until_output, _exported, _spec

SYMBOL = "h264bsdmiNextOutputTensorBatchResize"


def test_symbol_is_declared_exported_and_mirrored(built):
    text = open(os.path.join(ROOT, "include", "h264bsd_mi355x.h")).read()
    assert re.search(r"\bint\s+" + SYMBOL + r"\s*\(", text)
    assert SYMBOL in built.EXPORTED_SYMBOLS
    built.lib()
    assert SYMBOL in _exported(built.LIB_PATH)
    assert SYMBOL in _exported(built.capi.BENCH_LIB_PATH)


def test_resize_spec_layout_matches_the_ctypes_mirror(built, tmp_path):
    fields = [f[0] for f in built.ResizeSpec._fields_]
    src = tmp_path / "resize.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "h264bsd_mi355x.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(h264bsdmi_resize_spec));\n' +
                   "".join(f'    printf("%zu\\n", offsetof(h264bsdmi_resize_spec, {f}));\n' for f in fields) +
                   '    printf("%d %d %d %d %d\\n", H264BSDMI_FILTER_BILINEAR, H264BSDMI_FILTER_BILINEAR_AA, H264BSDMI_FILTER_BICUBIC_AA, '
                   'H264BSDMI_FIT_STRETCH, H264BSDMI_FIT_LETTERBOX);\n    return 0;\n}\n')
    exe = tmp_path / "resize"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [ctypes.sizeof(built.ResizeSpec)] + [getattr(built.ResizeSpec, f).offset for f in fields]
    assert got[: len(want)] == want
    f = built.capi.FILTERS
    assert got[len(want):] == [f[("bilinear", False)], f[("bilinear", True)], f[("bicubic", True)],
                               built.capi.FITS["stretch"], built.capi.FITS["letterbox"]]


def _resize(built, filter_=1, fit=0, pad=(0, 0, 0)):
    return built.ResizeSpec(filter_, fit, (ctypes.c_float * 3)(*pad))


def _call(built, decoders, spec, resize, colour=None):
    L = built.api_lib()
    n = len(decoders)
    got = (ctypes.c_uint32 * max(n, 1))()
    box = (ctypes.c_uint32 * max(4 * n, 4))(*([99] * max(4 * n, 4)))
    dec = (ctypes.c_void_p * max(n, 1))(*[d._st for d in decoders])
    rc = L.h264bsdmiNextOutputTensorBatchResize(n, dec, ctypes.byref(spec), None if colour is None else ctypes.byref(colour),
                                                None if resize is None else ctypes.byref(resize), None, got, None, None, None, box)
    return rc, list(box)


GOOD = [dict(filter_=0), dict(filter_=1), dict(filter_=2), dict(filter_=0, fit=1), dict(filter_=2, fit=1, pad=(1, 0.5, 0)),
        dict(fit=1, pad=(0.0, 1.0, 0.25))]
BAD = [dict(filter_=3), dict(filter_=99), dict(fit=2), dict(pad=(-0.01, 0, 0)), dict(pad=(0, 1.01, 0)), dict(pad=(0, 0, math.nan)),
       dict(pad=(math.inf, 0, 0)), dict(pad=(0, -math.inf, 0)), dict(fit=1, pad=(0, 0, 2))]


@pytest.mark.parametrize("good", GOOD)
def test_valid_resize_specs_are_accepted(built, good):
    assert _call(built, [], _spec(built, resize=1, width=224, height=224), _resize(built, **good))[0] == 0


@pytest.mark.parametrize("bad", BAD)
def test_invalid_resize_specs_are_refused(built, bad):
    """checked before any instance is looked at: an empty batch with a bad resize spec fails, the same batch with a good one succeeds"""
    spec = _spec(built, resize=1, width=224, height=224)
    assert _call(built, [], spec, _resize(built)) == (0, [99] * 4)
    rc, box = _call(built, [], spec, _resize(built, **bad))
    assert rc < 0 and box == [99] * 4


@pytest.mark.parametrize("good", GOOD)
def test_a_resize_spec_needs_resize_1(built, good):
    assert _call(built, [], _spec(built), None)[0] == 0
    assert _call(built, [], _spec(built), _resize(built, **good))[0] < 0
    assert _call(built, [], _spec(built, resize=2, width=224, height=224), _resize(built, **good))[0] < 0


@pytest.mark.parametrize("spec_bad", [dict(data=0), dict(dtype=3), dict(layout=0, channels=2), dict(std=(1, 0, 1))])
def test_tensor_and_colour_checks_still_apply(built, spec_bad):
    assert _call(built, [], _spec(built, resize=1, **spec_bad), _resize(built))[0] < 0
    assert _call(built, [], _spec(built, resize=1), _resize(built), built.ColourSpec(7, 0, 0, 0))[0] < 0
    assert _call(built, [], _spec(built, resize=1), _resize(built), built.ColourSpec(3, 2, 1, 0))[0] == 0


def test_capture_mode_instance_is_refused_and_keeps_its_picture(built):
    a, keep_a = _capture_until_output(built)
    b, keep_b = _capture_until_output(built)
    spec = _spec(built, resize=1, width=224, height=224)
    for r in (None, _resize(built, 1), _resize(built, 2, 1, (0.5, 0.5, 0.5))):
        rc, box = _call(built, [a], spec, r)
        assert rc < 0 and box == [99] * 4
    info = a.next_output_info()
    assert info is not None and info == b.next_output_info()
    a.close()
    b.close()


@pytest.mark.parametrize("kw", [dict(mode="bicubic"), dict(mode="nearest"), dict(mode="area", antialias=True), dict(fit="crop"),
                                dict(pad=(0, 0, 1.5)), dict(pad=(0, 0)), dict(pad=(math.nan, 0, 0)), dict(pad=(-1, 0, 0))])
def test_pull_tensor_refuses_bad_resize_arguments(built, kw):
    """before any device work: bicubic without antialias, names outside the tables, a pad outside [0, 1]"""
    with pytest.raises(ValueError):
        built.pull_tensor([], size=(8, 8), **kw)


@pytest.mark.parametrize("kw", [dict(antialias=True), dict(mode="bicubic", antialias=True), dict(fit="letterbox")])
def test_pull_tensor_resampling_needs_a_size(built, kw):
    with pytest.raises(ValueError):
        built.pull_tensor([], size=None, **kw)


SIZES = [(1920, 224), (1080, 224), (640, 257), (360, 333), (640, 1280), (360, 720), (1920, 8), (1080, 8), (1920, 640), (7, 3), (2, 1),
         (1, 5), (16, 16), (90, 61)]


@pytest.mark.parametrize("mode", ["bilinear", "bicubic"])
def test_model_weights_are_torchs_antialiased_interpolate(mode):
    """the float64 weight matrices reproduce F.interpolate(antialias=True) in float64 (it is linear: resampling the identity gives
    its matrix), every (in, out) of a sweep that covers downscaling, upscaling, 1080p -> 8 and odd sizes"""
    import torch
    import torch.nn.functional as F
    for n_in, n_out in SIZES:
        eye = torch.eye(n_in, dtype=torch.float64).reshape(1, n_in, 1, n_in)       # n_in pictures of one row, one per unit vector
        got = F.interpolate(eye, size=(1, n_out), mode=mode, antialias=True, align_corners=False)[0, :, 0, :].numpy().T
        want = rm.aa_weights(n_in, n_out, mode)
        assert np.abs(got - want).max() < 1e-12, (n_in, n_out)


def test_model_tap_counts_at_1080p_to_224():
    assert rm.tap_counts(1920, 224, "bilinear").max() == 18 and rm.tap_counts(1080, 224, "bilinear").max() == 10
    assert rm.tap_counts(1920, 224, "bicubic").max() == 35 and rm.tap_counts(1080, 224, "bicubic").max() == 20


def test_model_bilinear_without_antialias_is_torchs():
    """up to the rounding of torch's own fp32 source coordinates (which the model computes as the kernels do)"""
    import torch
    import torch.nn.functional as F
    for n_in, n_out in SIZES:
        eye = torch.eye(n_in, dtype=torch.float32).reshape(1, n_in, 1, n_in)
        got = F.interpolate(eye, size=(1, n_out), mode="bilinear", antialias=False, align_corners=False)[0, :, 0, :].double().numpy().T
        assert np.abs(got - rm.bilinear_weights(n_in, n_out)).max() < 1e-4, (n_in, n_out)


def test_model_resample_is_separable_torch():
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(5)
    v = rng.random((45, 80, 3))
    for filt, (mode, aa) in (("bilinear_aa", ("bilinear", True)), ("bicubic_aa", ("bicubic", True))):
        for size in ((17, 29), (90, 33), (8, 8)):
            want = F.interpolate(torch.from_numpy(v).permute(2, 0, 1)[None], size=size, mode=mode, antialias=aa, align_corners=False)
            got = rm.resample_hwc(v, size, filt)
            assert np.abs(got - want[0].permute(1, 2, 0).numpy()).max() < 1e-12


def test_model_letterbox_geometry():
    assert rm.letterbox(320, 320, 1920, 1080) == (0, 70, 320, 180)
    assert rm.letterbox(512, 256, 1920, 1080) == (28, 0, 455, 256)
    assert rm.letterbox(640, 640, 640, 360) == (0, 140, 640, 360)
    assert rm.letterbox(320, 320, 96, 64) == (0, 53, 320, 213)
    assert rm.letterbox(8, 8, 1920, 2) == (0, 3, 8, 1)            # never an empty rectangle
    assert rm.letterbox(224, 224, 224, 224) == (0, 0, 224, 224)
    for W, H, w, h in ((333, 257, 1920, 1080), (1, 1, 640, 360), (1000, 3, 90, 60)):
        left, top, iw, ih = rm.letterbox(W, H, w, h)
        assert 1 <= iw <= W and 1 <= ih <= H and left + iw <= W and top + ih <= H and (iw == W or ih == H)
