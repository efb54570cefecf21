"""No GPU: the symbol of the cell maps (declared, exported, mirrored), the struct and the constants against the header, what
h264bsdmiOutputCellMaps refuses before it looks at a device (through the built library, on parser-only instances), the argument errors
of pull_cells, the plane order and the views of CellMaps on a hand-filled buffer, and the numpy model (tests/cells_model.py): the
direct computation against the cell-by-cell records of the siblings' models, which is the interface's definition."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cells_model as clm
import stats_model as sm
from conftest import ROOT
from test_tensor_output import _capture_until_output

SENTINEL = 0xA5A5A5A5
LIMIT = 16384
CONSTANTS = dict(H264BSDMI_CELLS_PICTURE=0, H264BSDMI_CELLS_CHANGE=1, H264BSDMI_CELL_COUNT=1, H264BSDMI_CELL_SUM=2, H264BSDMI_CELL_SUMSQ=4,
                 H264BSDMI_CELL_MIN=8, H264BSDMI_CELL_MAX=16, H264BSDMI_CELL_SAD=2, H264BSDMI_CELL_SSD=4, H264BSDMI_CELL_DSUM=8,
                 H264BSDMI_CELL_DMAX=16, H264BSDMI_CELL_ABOVE=32)


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_symbol_is_declared_exported_and_mirrored(built):
    text = open(os.path.join(ROOT, "include", "h264bsd_mi355x.h")).read()
    built.lib()
    name = "h264bsdmiOutputCellMaps"
    assert re.search(r"\bint\s+" + name + r"\s*\(", text)
    assert name in built.EXPORTED_SYMBOLS
    assert name in _exported(built.LIB_PATH) and name in _exported(built.capi.BENCH_LIB_PATH)
    for attr in ("pull_cells", "CellsSpec", "CellMaps"):
        assert hasattr(built, attr)
    assert tuple(int(v) for v in built.__version__.split(".")) >= (0, 5, 0)
    assert "THE DEFINITION" in text and "min(cell, w - j cell)" in text           # the sentence that defines a cell is in the header


def test_cells_spec_layout_and_constants_match_the_header(built, tmp_path):
    fields = [f[0] for f in built.CellsSpec._fields_]
    assert fields == ["data", "cols", "rows", "cell", "source", "crop", "mode", "planes", "threshold", "keep_after"]
    src = tmp_path / "spec.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "h264bsd_mi355x.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(h264bsdmi_cells_spec));\n' +
                   "".join(f'    printf("%zu\\n", offsetof(h264bsdmi_cells_spec, {f}));\n' for f in fields) +
                   "".join(f'    printf("%u\\n", (unsigned){c});\n' for c in CONSTANTS) + "    return 0;\n}\n")
    exe = tmp_path / "spec"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(built.CellsSpec)] + [getattr(built.CellsSpec, f).offset for f in fields] + list(CONSTANTS.values())
    picture, change = built.capi.CELL_PLANES
    assert picture == clm.PLANES[0] == {k.split("_")[-1].lower(): CONSTANTS[k] for k in
                                        ("H264BSDMI_CELL_COUNT", "H264BSDMI_CELL_SUM", "H264BSDMI_CELL_SUMSQ", "H264BSDMI_CELL_MIN", "H264BSDMI_CELL_MAX")}
    assert change == clm.PLANES[1] == {k.split("_")[-1].lower(): CONSTANTS[k] for k in
                                       ("H264BSDMI_CELL_COUNT", "H264BSDMI_CELL_SAD", "H264BSDMI_CELL_SSD", "H264BSDMI_CELL_DSUM", "H264BSDMI_CELL_DMAX", "H264BSDMI_CELL_ABOVE")}
    assert built.capi.CELL_SIZES == clm.CELLS == (4, 8, 16, 32, 64)


def _spec(built, **kw):
    s = dict(data=0x1000, cols=6, rows=5, cell=8, source=1, crop=1, mode=1, planes=63, threshold=(0, 0, 0), keep_after=0)
    s.update(kw)
    return built.CellsSpec(s["data"], s["cols"], s["rows"], s["cell"], s["source"], s["crop"], s["mode"], s["planes"],
                           (ctypes.c_uint32 * 3)(*s["threshold"]), s["keep_after"])


def _call(built, decoders, regions, spec, null_regions=False, null_got=False, n_regions=None, null_dec=False):
    """(rc, got, current, kept, picId, keptPicId) of one raw call; the output arrays start as SENTINEL"""
    L = built.api_lib()
    n, K = len(decoders), len(regions) if n_regions is None else n_regions
    got = (ctypes.c_uint32 * max(K, 1))(*([SENTINEL] * max(K, 1)))
    per = [(ctypes.c_uint32 * max(n, 1))(*([SENTINEL] * max(n, 1))) for _ in range(4)]
    dec = (ctypes.c_void_p * max(n, 1))(*[d._st for d in decoders])
    regs = (built.Region * max(len(regions), 1))(*[built.Region(*r) for r in regions])
    rc = L.h264bsdmiOutputCellMaps(n, None if null_dec else dec, K, None if null_regions else regs, ctypes.byref(spec), None,
                                   None if null_got else got, *per)
    return (rc, list(got)) + tuple(list(a) for a in per)


def test_an_empty_call_with_a_valid_spec_is_accepted_and_launches_nothing(built):
    for source in (0, 1, 2):
        for cell in clm.CELLS:
            for kw in (dict(mode=0, planes=31), dict(mode=0, planes=1), dict(mode=1, planes=63, threshold=(255, 0, 7), keep_after=1),
                       dict(mode=1, planes=32), dict(cols=4096, rows=4096), dict(cols=1, rows=1), dict(data=0x1004)):
                res = _call(built, [], [], _spec(built, source=source, cell=cell, **kw))
                assert res[0] == 0 and res[1] == [SENTINEL], (source, cell, kw)
    assert _call(built, [], [], _spec(built), null_regions=True, null_got=True)[0] == 0        # regions == NULL, nRegions == n == 0


BAD_SPEC = [dict(data=0), dict(data=0x1002), dict(data=0x1001), dict(cols=0), dict(rows=0), dict(cols=4097), dict(rows=4097),
            dict(cols=2 ** 32 - 1), dict(cell=0), dict(cell=2), dict(cell=12), dict(cell=128), dict(cell=2 ** 31), dict(source=3),
            dict(source=2 ** 32 - 1), dict(crop=2), dict(mode=2), dict(planes=0), dict(planes=64), dict(planes=2 ** 31 | 1),
            dict(mode=0, planes=32), dict(mode=0, planes=63), dict(threshold=(256, 0, 0)), dict(threshold=(0, 256, 0)),
            dict(threshold=(0, 0, 2 ** 32 - 1)), dict(mode=0, planes=3, threshold=(1, 0, 0)), dict(mode=0, planes=3, threshold=(0, 0, 1)),
            dict(mode=0, planes=3, keep_after=1), dict(keep_after=2)]


@pytest.mark.parametrize("bad", BAD_SPEC)
def test_invalid_specs_are_refused_before_the_instances(built, bad):
    assert _call(built, [], [], _spec(built, **bad))[0] == -1
    assert built.api_lib().h264bsdmiOutputCellMaps(0, None, 0, None, None, None, None, None, None, None, None) == -1      # no spec at all


BAD_REGIONS = [(1, 0, 0, 16, 16), (2 ** 32 - 1, 0, 0, 16, 16), (0, 0, 0, 0, 16), (0, 0, 0, 16, 0), (0, 0, 0, LIMIT + 1, 16),
               (0, 0, 0, 16, LIMIT + 1), (0, LIMIT + 1, 0, 16, 16), (0, -LIMIT - 1, 0, 16, 16), (0, 0, LIMIT + 1, 16, 16),
               (0, 0, -LIMIT - 1, 16, 16), (0, -2 ** 31, 0, 16, 16)]


def test_every_refusal_is_minus_one_and_nothing_is_written_or_popped(built):
    """an instance in capture mode has no pixels: every call that names it is refused, whatever else is wrong with it; the
    sentinels stay, and the instance's output queue is what an untouched twin's is"""
    a, keep_a = _capture_until_output(built)
    b, keep_b = _capture_until_output(built)
    spec = _spec(built)
    untouched = (-1, [SENTINEL]) + ([SENTINEL],) * 4
    for good in [(0, 0, 0, 16, 16), (0, -5, 3, 17, 31), (0, LIMIT, -LIMIT, LIMIT, LIMIT)]:
        for kw in (dict(), dict(mode=0, planes=31, source=0), dict(source=2, cell=64, crop=0, keep_after=1)):
            assert _call(built, [a], [good], _spec(built, **kw)) == untouched
    for bad in BAD_REGIONS:
        assert _call(built, [a], [bad], spec) == untouched, bad
    for bad in BAD_SPEC:
        assert _call(built, [a], [(0, 0, 0, 16, 16)], _spec(built, **bad)) == untouched, bad
    assert _call(built, [a], [(0, 0, 0, 16, 16)], spec, null_regions=True) == untouched      # whole windows, but capture mode
    assert _call(built, [a], [(0, 0, 0, 16, 16)] * 2, spec, null_regions=True)[0] == -1      # regions == NULL with nRegions != n
    assert _call(built, [], [(0, 0, 0, 16, 16)], spec, null_regions=True)[0] == -1           # likewise, n == 0
    assert _call(built, [a], [(0, 0, 0, 16, 16)], spec, null_got=True)[0] == -1
    assert _call(built, [a], [(0, 0, 0, 16, 16)], spec, n_regions=65536)[0] == -1
    assert _call(built, [a], [], spec)[0] == -1                                              # the instances are checked as in the region pull
    assert _call(built, [a], [], spec, null_dec=True)[0] == -1
    res = _call(built, [a, a], [(0, 0, 0, 16, 16), (1, 0, 0, 16, 16)], spec)
    assert res[0] == -1 and res[1] == [SENTINEL] * 2 and res[2] == [SENTINEL] * 2 and res[3] == [SENTINEL] * 2
    info = a.next_output_info()
    assert info is not None and info == b.next_output_info()
    a.close()
    b.close()


@pytest.mark.parametrize("kw", [dict(source="yuv"), dict(cell=12), dict(cell=2), dict(cell=128), dict(against="previous"), dict(planes=()),
                                dict(planes=("sad",)), dict(planes=("count", "hist")), dict(against="kept", planes=("sum",)),
                                dict(threshold=1), dict(keep=True), dict(against="kept", planes=("sad",), threshold=256),
                                dict(against="kept", planes=("sad",), threshold=-1), dict(against="kept", planes=("sad",), threshold=(1, 2)),
                                dict(against="kept", planes=("sad",), threshold=1.5), dict(grid=(0, 4)), dict(grid=(4, 4097)), dict(grid=7),
                                dict(grid=(2.0, 2)), dict(grid=(1, 2, 3)), dict(regions=[(0, 0, 0, 0, 8)]), dict(regions=[(1, 0, 0, 8, 8)]),
                                dict(regions=[(0, 0, 0, 8, 8)] * 65536)])
def test_pull_cells_refuses_bad_arguments(built, kw):
    """before any device work: names that are not in the tables, planes of the other mode, thresholds, grids and regions out of range"""
    a, keep = _capture_until_output(built)
    args = dict(regions=[(0, 0, 0, 8, 8)], source="ycbcr")
    args.update(kw)
    with pytest.raises(ValueError, match="pull_cells"):
        built.pull_cells([a], **args)
    a.close()


class _Buffer:
    """what CellMaps needs of a tensor: slicing"""

    def __init__(self, a):
        self.a = a

    def __getitem__(self, k):
        return self.a[k]


@pytest.mark.parametrize("mode,C,names", [(0, 1, ("count", "sum")), (0, 3, ("sum", "sumsq", "min", "max", "count")), (0, 3, ("max",)),
                                          (1, 1, ("sad",)), (1, 3, ("count", "above")), (1, 3, ("above", "dmax", "dsum", "ssd", "sad", "count")),
                                          (1, 1, ("dsum", "ssd"))])
def test_plane_order_and_views_on_a_hand_filled_buffer(built, mode, C, names):
    """map p of a slice is filled with p: COUNT first, then the planes in ascending bit order whatever order they were named in, C maps each"""
    bits = clm.plane_bits(mode, names)
    P = clm.n_maps(mode, C, bits)
    R, rows, cols = 2, 3, 4
    maps = np.broadcast_to(np.arange(P, dtype=np.int32)[None, :, None, None], (R, P, rows, cols)).copy()
    maps[1] += 100
    cm = built.CellMaps(_Buffer(maps), mode, C, bits, [1, 1], [1], [1], [7], [6])
    at = 0
    for name, bit in built.capi.CELL_PLANES[mode].items():
        view = getattr(cm, name)
        if not bits & bit:
            assert view is None, name
            continue
        width = 1 if bit == 1 else C
        assert view.shape == ((R, rows, cols) if bit == 1 else (R, C, rows, cols)), name
        want = np.arange(at, at + width, dtype=np.int32)
        assert np.array_equal(view.reshape(R, width, rows, cols)[0, :, 0, 0], want) and np.array_equal(view.reshape(R, width, rows, cols)[1, :, 2, 3], want + 100)
        at += width
    assert at == P and cm.maps is not None and (cm.got, cm.current, cm.kept, cm.pic_id, cm.kept_pic_id) == ([1, 1], [1], [1], [7], [6])
    other = set(built.capi.CELL_PLANES[1 - mode]) - set(built.capi.CELL_PLANES[mode])
    assert not any(hasattr(cm, name) for name in other)


# ---- the model: the direct computation against the siblings' records, cell by cell ----
W, H = 112, 80
WINDOW = (2, 2, 90, 60)
MODEL_BOXES = [(0, 0, 90, 60), (0, 0, 1, 1), (16, 16, 16, 16), (13, 11, 37, 23), (-9, 10, 30, 20), (70, -5, 40, 20), (5, 50, 9, 30),
               (-40, 0, 30, 30), (95, 3, 10, 10)]


@pytest.fixture(scope="module")
def planes():
    rng = np.random.default_rng(23)
    frames = [rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8) for _ in range(2)]
    return {s: [sm.channels(f, W, H, s) for f in frames] for s in ("y", "ycbcr")}


@pytest.mark.parametrize("source", ["y", "ycbcr"])
@pytest.mark.parametrize("cell", clm.CELLS)
def test_model_equals_the_cell_by_cell_records(planes, source, cell):
    cur, kept = planes[source]
    for box in MODEL_BOXES:
        for grid in (clm.default_grid([(box[3], box[2])], cell), (5, 6), (1, 2)):
            a = clm.maps(clm.PICTURE, 31, cur, None, WINDOW, box, cell, grid)
            b = clm.maps_by_records(clm.PICTURE, 31, cur, None, WINDOW, box, cell, grid)
            assert np.array_equal(a, b), (box, grid)
            a = clm.maps(clm.CHANGE, 63, cur, kept, WINDOW, box, cell, grid, threshold=(40, 0, 254))
            b = clm.maps_by_records(clm.CHANGE, 63, cur, kept, WINDOW, box, cell, grid, threshold=(40, 0, 254))
            assert np.array_equal(a, b), (box, grid)


def test_model_geometry_of_the_two_named_boxes():
    """(13, 11, 37, 23) on a 5 x 6 grid of 8: a last column 5 wide, a last row 7 tall, empty cells beyond; (-9, 10, 30, 20): a first
    column entirely outside the window and a second that is 7 wide"""
    flat = np.full((1, H, W), 9, np.uint8)
    count = clm.maps(clm.PICTURE, 1, flat, None, WINDOW, (13, 11, 37, 23), 8, (5, 6))[0]
    assert count[0].tolist() == [64, 64, 64, 64, 40, 0] and count[:, 0].tolist() == [64, 64, 56, 0, 0] and count[2, 4] == 35
    count = clm.maps(clm.PICTURE, 1, flat, None, WINDOW, (-9, 10, 30, 20), 8, (5, 6))[0]
    assert count[0].tolist() == [0, 56, 64, 48, 0, 0] and count[2].tolist() == [0, 28, 32, 24, 0, 0]
    full = clm.maps(clm.PICTURE, 31, flat, None, WINDOW, (-9, 10, 30, 20), 8, (5, 6))
    assert full[1, 0, 1] == 9 * 56 and full[2, 0, 1] == 81 * 56 and full[3, 0, 1] == full[4, 0, 1] == 9
    assert (full[1, :, 0] == 0).all() and (full[3, :, 0] == 255).all() and (full[4, :, 0] == 0).all()        # count 0: sum 0, min 255, max 0


def test_model_a_smaller_grid_truncates_and_subsets_select(planes):
    cur, kept = planes["ycbcr"]
    box = (13, 11, 37, 23)
    whole = clm.maps(clm.CHANGE, 63, cur, kept, WINDOW, box, 8, (5, 6), threshold=(3, 3, 3))
    small = clm.maps(clm.CHANGE, 63, cur, kept, WINDOW, box, 8, (2, 3), threshold=(3, 3, 3))
    assert np.array_equal(small, whole[:, :2, :3])
    assert np.array_equal(clm.maps(clm.CHANGE, 2, cur, kept, WINDOW, box, 8, (5, 6)), whole[1:4])
    assert np.array_equal(clm.maps(clm.CHANGE, 33, cur, kept, WINDOW, box, 8, (5, 6), threshold=(3, 3, 3)), whole[[0, 13, 14, 15]])
    same = clm.maps(clm.CHANGE, 63, cur, cur.copy(), WINDOW, box, 8, (5, 6))
    assert same[0].sum() == 37 * 23 and not same[1:].any()
