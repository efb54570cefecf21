"""No GPU: the symbol of the corner points (declared, exported, mirrored), the stride formula, the spec's layout, what pull_corners
refuses before any device work, and the numpy model (tests/corners_model.py) against independent formulations: the gradients and the
box sums against scipy.ndimage.correlate (mode "nearest": the same replication), the non-maximum suppression against a double loop,
and the properties the definition promises.  What the C entry refuses, and what an accepted call hands to the engine, is shown in C by
tests/test_corner_points_host.py; the device by tests/test_gpu_corner_points.py."""
import ctypes
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import corners_model as cm
from conftest import ROOT
from test_tensor_output import _capture_until_output

SYMBOL = "h264bsdmiOutputCornerPoints"
W, H = 64, 48


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_the_symbol_is_declared_exported_and_mirrored(built):
    text = open(os.path.join(ROOT, "include", "h264bsd_mi355x.h")).read()
    built.lib()
    assert re.search(r"\bint\s+" + SYMBOL + r"\s*\(", text)
    assert SYMBOL in built.EXPORTED_SYMBOLS
    assert SYMBOL in _exported(built.LIB_PATH) and SYMBOL in _exported(built.capi.BENCH_LIB_PATH)
    for name in ("pull_corners", "corners_record_bytes", "CornersSpec", "CornerPoints"):
        assert hasattr(built, name)
    assert re.search(r"#define\s+H264BSDMI_CORNERS_MAX_NMS\s+7u\b", text) and re.search(r"#define\s+H264BSDMI_CORNERS_MAX_POINTS\s+256u\b", text)
    assert re.search(r"#define\s+H264BSDMI_CORNERS_MIN_EIGEN\s+0u\b", text) and re.search(r"#define\s+H264BSDMI_CORNERS_HARRIS\s+1u\b", text)
    assert (built.capi.CORNERS_MAX_NMS, built.capi.CORNERS_MAX_POINTS) == (7, 256) and built.capi.CORNER_SCORES == dict(min_eigen=0, harris=1)
    assert tuple(int(v) for v in built.__version__.split(".")) >= (0, 9, 0)


def test_corners_spec_layout_matches_the_ctypes_mirror(built, tmp_path):
    fields = [f[0] for f in built.CornersSpec._fields_]
    src = tmp_path / "spec.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "h264bsd_mi355x.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(h264bsdmi_corners_spec));\n' +
                   "".join(f'    printf("%zu\\n", offsetof(h264bsdmi_corners_spec, {f}));\n' for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "spec"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(built.CornersSpec)] + [getattr(built.CornersSpec, f).offset for f in fields]
    assert got[0] == 40 and fields == ["data", "score", "block", "nms", "max_points", "crop", "zero", "min_score"]


@pytest.mark.parametrize("K", [1, 16, 64, 256])
def test_record_bytes_is_the_headers_formula(built, K):
    assert built.corners_record_bytes(K) == 32 + 16 * K == cm.record_bytes(K)
    for bad in (0, 257, -1, 1.0, None, True):
        with pytest.raises(ValueError):
            built.corners_record_bytes(bad)


@pytest.mark.parametrize("kw", [dict(score="fast"), dict(block=4), dict(block=7), dict(block=3.0), dict(nms=0), dict(nms=8), dict(max_points=0),
                                dict(max_points=257), dict(min_score=-1), dict(min_score=2 ** 64), dict(score="harris", min_score=2 ** 63),
                                dict(min_score=0.5), dict(regions=[(0, 0, 0, 0, 8)]), dict(regions=[(1, 0, 0, 8, 8)]),
                                dict(regions=[(0, 0, 0, 8, 8)] * 65536)])
def test_pull_corners_refuses_bad_arguments(built, kw):
    """before any device work: a score, a block, an nms, a K, a min_score or a region out of range"""
    a, keep = _capture_until_output(built)
    args = dict(regions=[(0, 0, 0, 8, 8)])
    args.update(kw)
    with pytest.raises(ValueError):
        built.pull_corners([a], **args)
    a.close()


def test_the_c_entry_refuses_a_capture_instance_and_bad_specs_without_a_device(built):
    """through the built library: no spec, bad fields with no instances at all (refused before the instances), and an instance in
    capture mode, which has no pixels; the arrays keep their sentinel"""
    L = built.api_lib()
    S = 0xA5A5A5A5
    good = dict(data=0x1000, score=0, block=3, nms=3, max_points=64, crop=1, zero=0, min_score=0)

    def call(decs, **kw):
        f = dict(good)
        f.update(kw)
        spec = built.CornersSpec(*[f[k[0]] for k in built.CornersSpec._fields_])
        n = len(decs)
        arrays = [(ctypes.c_uint32 * 1)(S) for _ in range(3)]
        rc = L.h264bsdmiOutputCornerPoints(n, (ctypes.c_void_p * max(n, 1))(*[d._st for d in decs]), n, None, ctypes.byref(spec), None, *arrays)
        return rc, [a[0] for a in arrays]

    assert L.h264bsdmiOutputCornerPoints(0, None, 0, None, None, None, None, None, None) == -1
    assert call([]) == (0, [S, S, S])
    assert call([], score=1, block=5, nms=7, max_points=256, crop=0, min_score=2 ** 63 - 1)[0] == 0
    assert call([], min_score=2 ** 64 - 1)[0] == 0
    for bad in (dict(data=0), dict(data=0x1004), dict(score=2), dict(block=0), dict(block=4), dict(block=6), dict(nms=0), dict(nms=8),
                dict(max_points=0), dict(max_points=257), dict(crop=2), dict(zero=1), dict(score=1, min_score=2 ** 63)):
        assert call([], **bad) == (-1, [S, S, S]), bad
    a, keep = _capture_until_output(built)
    assert call([a]) == (-1, [S, S, S])
    a.close()


# ---- the model against independent formulations ----
def _random(seed, shape=(H, W)):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _checkerboard(w=W, h=H, cell=8):
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    return ((((x // cell) + (y // cell)) & 1) * 255).astype(np.uint8)


@pytest.mark.parametrize("block", [3, 5])
def test_gradients_and_box_sums_equal_scipys_correlation(block):
    """correlate(mode="nearest") replicates the array at its border and filters THAT: for the gradients this is the definition.  The box
    sums of the definition run over gradients of the replicated picture BEYOND the window, not over replicated gradients, so they are
    compared on a padded picture, inside it"""
    from scipy import ndimage
    win = _random(1)
    kx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], np.int64)
    gx, gy = cm.gradients(win)
    o = cm.PAD - 1
    assert np.array_equal(gx[o:o + H, o:o + W], ndimage.correlate(win.astype(np.int64), kx, mode="nearest"))
    assert np.array_equal(gy[o:o + H, o:o + W], ndimage.correlate(win.astype(np.int64), kx.T, mode="nearest"))
    assert np.abs(gx).max() <= 1020 and np.abs(gy).max() <= 1020
    big = np.pad(win, 4, mode="edge").astype(np.int64)                     # the replicated picture, 4 samples out
    bx, by = ndimage.correlate(big, kx, mode="nearest"), ndimage.correlate(big, kx.T, mode="nearest")
    ones = np.ones((block, block), np.int64)
    A, B, C = cm.tensor(win, block)
    for mine, prod in ((A, bx * bx), (B, by * by), (C, bx * by)):
        assert np.array_equal(mine, ndimage.correlate(prod, ones, mode="constant")[4:4 + H, 4:4 + W])


def _brute_candidates(S, nms, min_score):
    h, w = S.shape
    out = np.zeros((h, w), bool)
    for y in range(h):
        for x in range(w):
            p = S[y, x]
            if not p > min_score:
                continue
            best = True
            for v in range(max(y - nms, 0), min(y + nms, h - 1) + 1):
                for u in range(max(x - nms, 0), min(x + nms, w - 1) + 1):
                    if (v, u) != (y, x) and (S[v, u] > p or (S[v, u] == p and (v, u) < (y, x))):
                        best = False
            out[y, x] = best
    return out


@pytest.mark.parametrize("score", [cm.MIN_EIGEN, cm.HARRIS])
def test_nms_equals_the_double_loop(score):
    S = cm.scores(_random(2, (24, 32)), score, 3)
    for nms in (1, 3, 7):
        for min_score in (0, int(np.median(S[S > 0]))):
            assert np.array_equal(cm.candidates(S, nms, min_score), _brute_candidates(S, nms, min_score)), (nms, min_score)
    T = cm.scores(_checkerboard(32, 24, 8), score, 3)                     # ties everywhere
    assert np.array_equal(cm.candidates(T, 3, 0), _brute_candidates(T, 3, 0))


def test_min_eigen_is_the_floor_formula_and_stays_below_2_26():
    for win in (_random(3), _checkerboard(), (np.indices((H, W)).sum(0) & 1).astype(np.uint8) * 255):
        for block in (3, 5):
            A, B, C = cm.tensor(win, block)
            S = cm.scores(win, cm.MIN_EIGEN, block)
            assert S.min() >= 0 and S.max() < 2 ** 26 and max(A.max(), B.max(), np.abs(C).max()) < 2 ** 25
            for y, x in ((0, 0), (5, 9), (H - 1, W - 1), (17, 40)):
                a, b, c = int(A[y, x]), int(B[y, x]), int(C[y, x])
                assert int(S[y, x]) == a + b - math.isqrt((a - b) ** 2 + 4 * c * c)


def test_harris_extremes_stay_inside_i64():
    """the worst pictures at block 5: alternating 0 / 255 columns, isolated 255 dots on a 2-sample lattice, and columns two samples wide
    (every |gx| is 1020 there, A at its largest and B = 0: the most negative score there is).  Evaluated in Python integers and compared
    with the int64 arithmetic"""
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    wide = (((x >> 1) & 1) * 255).astype(np.uint8)
    for win in (((x & 1) * 255).astype(np.uint8), (((x & 1) & (y & 1)) * 255).astype(np.uint8), wide):
        A, B, C = (p.astype(object) for p in cm.tensor(win, 5))
        exact = 16 * (A * B - C * C) - (A + B) * (A + B)
        assert max(abs(int(v)) for v in exact.ravel()) < 2 ** 54
        assert np.array_equal(cm.scores(win, cm.HARRIS, 5).astype(object), exact)
    assert cm.scores(wide, cm.HARRIS, 5).min() == -(25 * 1020 * 1020) ** 2


def test_the_checkerboard_ties_at_one_score_and_raster_order_decides():
    for score, value in ((cm.MIN_EIGEN, 6242400), (cm.HARRIS, 116902673280000)):
        w = cm.Window(_checkerboard(), score, 3)
        count, energy, pts = w.points((0, 0, W, H), 3)
        assert count == W * H and len(pts) == 35 and {p[2] for p in pts} == {value}
        assert [(p[1], p[0]) for p in pts] == sorted((p[1], p[0]) for p in pts)         # one score: the order is y, then x
        # of the four tied samples around a crossing the earliest in raster order stands
        assert all((p[0] % 8, p[1] % 8) == (7, 7) for p in pts)


def test_a_constant_picture_has_no_points_and_no_energy():
    for score in (cm.MIN_EIGEN, cm.HARRIS):
        w = cm.Window(np.full((H, W), 131, np.uint8), score, 5)
        assert w.points((0, 0, W, H), 1) == (W * H, 0, [])
        rec = w.record((3, 3, 20, 20), 1, 4)
        assert rec == struct.pack("<IIIIQQ", 400, 0, 0, 0, 0, 0) + bytes(64)


@pytest.mark.parametrize("score", [cm.MIN_EIGEN, cm.HARRIS])
def test_candidates_of_a_box_are_the_windows_candidates_in_the_box(score):
    rng = np.random.default_rng(8)
    w = cm.Window(_random(4), score, 3)
    for nms in (1, 3, 7):
        _, _, whole = w.points((0, 0, W, H), nms)
        for _ in range(12):
            x, y = int(rng.integers(-10, W)), int(rng.integers(-10, H))
            bw, bh = int(rng.integers(1, 50)), int(rng.integers(1, 40))
            count, energy, pts = w.points((x, y, bw, bh), nms)
            assert pts == [p for p in whole if x <= p[0] < x + bw and y <= p[1] < y + bh]
            x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + bw, W), min(y + bh, H)
            assert count == max(x1 - x0, 0) * max(y1 - y0, 0)


def test_records_truncate_sort_and_pad():
    w = cm.Window(_random(5), cm.MIN_EIGEN, 3)
    count, energy, pts = w.points((0, 0, W, H), 1)
    assert len(pts) > 16 and energy > 0
    rec = w.record((0, 0, W, H), 1, 16)
    assert len(rec) == cm.record_bytes(16) and struct.unpack_from("<IIIIQQ", rec) == (W * H, len(pts), 16, 0, energy, 0)
    got = [struct.unpack_from("<iiq", rec, 32 + 16 * k) for k in range(16)]
    assert got == pts[:16] and all(a[2] >= b[2] for a, b in zip(got, got[1:]))
    few = w.record((0, 0, W, H), 7, 256)
    n = struct.unpack_from("<I", few, 4)[0]
    assert 0 < n < 256 and few[32 + 16 * n:] == bytes(16 * (256 - n))
    assert w.record((200, 200, 8, 8), 3, 4) == bytes(cm.record_bytes(4))                 # a miss: all zero
    top = pts[0][2]
    assert w.points((0, 0, W, H), 1, top)[2] == [] and len(w.points((0, 0, W, H), 1, top - 1)[2]) >= 1     # the comparison is strict
