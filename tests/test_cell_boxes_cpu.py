"""No GPU: the symbol of the cell boxes (declared, exported, mirrored), the struct and the constants against the header, every refusal
of h264bsdmiOutputCellBoxes before it looks at a device (through the built library, on parser-only instances), the argument errors of
pull_boxes, the views of CellBoxes on a hand-filled buffer, and the numpy model (tests/boxes_model.py): against scipy where scipy
imports, and its own corner cases."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import boxes_model as bm
from conftest import ROOT
from test_tensor_output import _capture_until_output

SENTINEL = 0xA5A5A5A5
CONSTANTS = dict(H264BSDMI_BOXES_MAX_CELLS=16384, H264BSDMI_BOXES_MAX_BOXES=512, H264BSDMI_BOXES_ABOVE=0, H264BSDMI_BOXES_BELOW=1)


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_symbol_is_declared_exported_and_mirrored(built):
    text = open(os.path.join(ROOT, "include", "h264bsd_mi355x.h")).read()
    built.lib()
    name = "h264bsdmiOutputCellBoxes"
    assert re.search(r"\bint\s+" + name + r"\s*\(", text)
    assert name in built.EXPORTED_SYMBOLS
    assert name in _exported(built.LIB_PATH) and name in _exported(built.capi.BENCH_LIB_PATH)
    for attr in ("pull_boxes", "BoxesSpec", "CellBoxes"):
        assert hasattr(built, attr)
    assert tuple(int(v) for v in built.__version__.split(".")) >= (0, 6, 0)
    for phrase in ("FOREGROUND", "COMPONENTS", "NUMBERING", "SLICE LAYOUT", "THE CAP", "not part of this interface yet"):
        assert phrase in text, phrase


def test_boxes_spec_layout_and_constants_match_the_header(built, tmp_path):
    fields = [f[0] for f in built.BoxesSpec._fields_]
    assert fields == ["data", "max_boxes", "plane", "channel", "sense", "level", "connectivity", "min_cells"]
    src = tmp_path / "spec.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "h264bsd_mi355x.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(h264bsdmi_boxes_spec));\n' +
                   "".join(f'    printf("%zu\\n", offsetof(h264bsdmi_boxes_spec, {f}));\n' for f in fields) +
                   "".join(f'    printf("%u\\n", (unsigned){c});\n' for c in CONSTANTS) + "    return 0;\n}\n")
    exe = tmp_path / "spec"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(built.BoxesSpec)] + [getattr(built.BoxesSpec, f).offset for f in fields] + list(CONSTANTS.values())
    assert (built.capi.BOXES_MAX_CELLS, built.capi.BOXES_MAX_BOXES) == (bm.MAX_CELLS, bm.MAX_BOXES) == (16384, 512)
    assert built.capi.BOXES_SENSES == dict(above=bm.ABOVE, below=bm.BELOW)


def _cells(built, **kw):
    s = dict(data=0x1000, cols=6, rows=5, cell=8, source=1, crop=1, mode=1, planes=63, threshold=(0, 0, 0), keep_after=0)
    s.update(kw)
    return built.CellsSpec(s["data"], s["cols"], s["rows"], s["cell"], s["source"], s["crop"], s["mode"], s["planes"],
                           (ctypes.c_uint32 * 3)(*s["threshold"]), s["keep_after"])


def _boxes(built, **kw):
    s = dict(data=0x2000, max_boxes=64, plane=2, channel=0, sense=0, level=10, connectivity=8, min_cells=1)
    s.update(kw)
    return built.BoxesSpec(s["data"], s["max_boxes"], s["plane"], s["channel"], s["sense"], s["level"], s["connectivity"], s["min_cells"])


def _call(built, decoders, regions, cells, boxes, null_regions=False, null_got=False, null_boxes=False):
    """(rc, got, current, kept, picId, keptPicId) of one raw call; the output arrays start as SENTINEL"""
    L = built.api_lib()
    n, K = len(decoders), len(regions)
    got = (ctypes.c_uint32 * max(K, 1))(*([SENTINEL] * max(K, 1)))
    per = [(ctypes.c_uint32 * max(n, 1))(*([SENTINEL] * max(n, 1))) for _ in range(4)]
    dec = (ctypes.c_void_p * max(n, 1))(*[d._st for d in decoders])
    regs = (built.Region * max(K, 1))(*[built.Region(*r) for r in regions])
    rc = L.h264bsdmiOutputCellBoxes(n, dec, K, None if null_regions else regs, ctypes.byref(cells), None if null_boxes else ctypes.byref(boxes), None,
                                    None if null_got else got, *per)
    return (rc, list(got)) + tuple(list(a) for a in per)


GOOD = [dict(), dict(max_boxes=1), dict(max_boxes=512), dict(plane=1), dict(plane=32, channel=2), dict(plane=16, channel=1), dict(sense=1, level=2 ** 32 - 1),
        dict(connectivity=4), dict(min_cells=2 ** 32 - 1), dict(data=0x2004)]


def test_an_empty_call_with_valid_specs_is_accepted_and_launches_nothing(built):
    for kw in GOOD:
        res = _call(built, [], [], _cells(built), _boxes(built, **kw))
        assert res[0] == 0 and res[1] == [SENTINEL], kw
    # the cap, from below: 128 x 128 = 16384 cells; PICTURE mode, where bit 8 is MIN and may be chosen
    assert _call(built, [], [], _cells(built, cols=128, rows=128), _boxes(built))[0] == 0
    assert _call(built, [], [], _cells(built, cols=4096, rows=4), _boxes(built))[0] == 0
    assert _call(built, [], [], _cells(built, mode=0, planes=31), _boxes(built, plane=8, channel=2))[0] == 0
    assert _call(built, [], [], _cells(built, source=0), _boxes(built, plane=4, channel=0))[0] == 0
    assert _call(built, [], [], _cells(built), _boxes(built), null_regions=True, null_got=True)[0] == 0


# one per clause of the header's list, with the boundary pairs
BAD_BOXES = [dict(data=0), dict(data=0x2002), dict(data=0x2001), dict(max_boxes=0), dict(max_boxes=513), dict(max_boxes=2 ** 32 - 1),
             dict(plane=0), dict(plane=3), dict(plane=6), dict(plane=64), dict(plane=2 ** 31), dict(plane=8),      # 8: DSUM in CHANGE mode
             dict(channel=3), dict(channel=2 ** 32 - 1), dict(plane=1, channel=1), dict(sense=2), dict(sense=2 ** 32 - 1),
             dict(connectivity=0), dict(connectivity=6), dict(connectivity=12), dict(min_cells=0)]
BAD_PAIRS = [(dict(cols=16385, rows=1), dict()), (dict(cols=4096, rows=4096), dict()), (dict(cols=1, rows=4097), dict()),
             (dict(planes=33), dict(plane=2)),                      # a plane that was not asked for
             (dict(source=0), dict(plane=2, channel=1)),            # luma has one channel
             (dict(cell=12), dict()), (dict(planes=0), dict()), (dict(threshold=(256, 0, 0)), dict()), (dict(data=0), dict()),
             (dict(mode=0, planes=31, keep_after=1), dict()), (dict(mode=0, planes=31), dict(plane=32))]


def test_the_cap_is_sixteen_thousand_three_hundred_and_eighty_four_cells(built):
    assert _call(built, [], [], _cells(built, cols=2048, rows=8), _boxes(built))[0] == 0            # 16384
    assert _call(built, [], [], _cells(built, cols=129, rows=127), _boxes(built))[0] == 0           # 16383
    assert _call(built, [], [], _cells(built, cols=1, rows=4096), _boxes(built))[0] == 0
    assert _call(built, [], [], _cells(built, cols=3277, rows=5), _boxes(built))[0] == -1           # 16385
    assert _call(built, [], [], _cells(built, cols=129, rows=128), _boxes(built))[0] == -1
    assert _call(built, [], [], _cells(built, cols=120, rows=135), _boxes(built))[0] == 0           # 1080p at cell 16 is 68 x 120; this is 16200
    assert _call(built, [], [], _cells(built, cols=240, rows=135), _boxes(built))[0] == -1          # 1080p at cell 8
    assert _call(built, [], [], _cells(built, cols=240, rows=135, planes=3), _boxes(built))[0] == -1
    built_cells = built.api_lib().h264bsdmiOutputCellMaps                                            # ... which the maps alone take
    assert built_cells(0, None, 0, None, ctypes.byref(_cells(built, cols=240, rows=135)), None, None, None, None, None, None) == 0


@pytest.mark.parametrize("bad", BAD_BOXES)
def test_invalid_boxes_specs_are_refused_before_the_instances(built, bad):
    assert _call(built, [], [], _cells(built), _boxes(built, **bad))[0] == -1


@pytest.mark.parametrize("cells,boxes", BAD_PAIRS)
def test_invalid_pairs_of_specs_are_refused_before_the_instances(built, cells, boxes):
    assert _call(built, [], [], _cells(built, **cells), _boxes(built, **boxes))[0] == -1


def test_null_specs_are_refused(built):
    L = built.api_lib()
    assert _call(built, [], [], _cells(built), _boxes(built), null_boxes=True)[0] == -1
    assert L.h264bsdmiOutputCellBoxes(0, None, 0, None, None, ctypes.byref(_boxes(built)), None, None, None, None, None, None) == -1
    assert L.h264bsdmiOutputCellBoxes(0, None, 0, None, None, None, None, None, None, None, None, None) == -1


def test_every_refusal_is_minus_one_and_nothing_is_written_or_popped(built):
    """an instance in capture mode has no pixels: every call that names it is refused, whatever else is wrong with it; the sentinels
    stay, and the instance's output queue is what an untouched twin's is"""
    a, keep_a = _capture_until_output(built)
    b, keep_b = _capture_until_output(built)
    untouched = (-1, [SENTINEL]) + ([SENTINEL],) * 4
    region = (0, 0, 0, 16, 16)
    for kw in GOOD:
        assert _call(built, [a], [region], _cells(built), _boxes(built, **kw)) == untouched
    for bad in BAD_BOXES:
        assert _call(built, [a], [region], _cells(built), _boxes(built, **bad)) == untouched, bad
    for cells, boxes in BAD_PAIRS:
        assert _call(built, [a], [region], _cells(built, **cells), _boxes(built, **boxes)) == untouched, (cells, boxes)
    for bad in [(1, 0, 0, 16, 16), (0, 0, 0, 0, 16), (0, 16385, 0, 16, 16), (0, 0, -16385, 16, 16)]:        # what the cell maps refuse in regions
        assert _call(built, [a], [bad], _cells(built), _boxes(built)) == untouched, bad
    assert _call(built, [a], [region], _cells(built), _boxes(built), null_got=True)[0] == -1
    assert _call(built, [a], [region] * 2, _cells(built), _boxes(built), null_regions=True)[0] == -1
    res = _call(built, [a, a], [region, (1, 0, 0, 16, 16)], _cells(built), _boxes(built))
    assert res[0] == -1 and res[1] == [SENTINEL] * 2 and res[2] == [SENTINEL] * 2
    info = a.next_output_info()
    assert info is not None and info == b.next_output_info()
    a.close()
    b.close()


@pytest.mark.parametrize("kw", [dict(source="yuv"), dict(cell=12), dict(against="previous"), dict(planes=()), dict(planes=("sum",)),
                                dict(against=None, planes=("sum",), threshold=1), dict(against=None, planes=("sum",), keep=True),
                                dict(threshold=256), dict(grid=(0, 4)), dict(grid=(4, 4097)), dict(regions=[(0, 0, 0, 0, 8)]),
                                dict(regions=[(1, 0, 0, 8, 8)]),
                                dict(plane="ssd"), dict(planes=("sad", "dsum"), plane="dsum"), dict(planes=("dsum",)), dict(plane="max"),
                                dict(channel=3), dict(channel=-1), dict(channel=1.0), dict(planes=("count",), channel=1), dict(source="y", channel=1),
                                dict(sense="over"), dict(connectivity=6), dict(connectivity="8"), dict(level=-1), dict(level=2 ** 32),
                                dict(level=1.5), dict(min_cells=0), dict(max_boxes=0), dict(max_boxes=513), dict(max_boxes=8.0)])
def test_pull_boxes_refuses_bad_arguments(built, kw):
    """before any device work: what pull_cells refuses, under pull_boxes' own name, and what the boxes add"""
    a, keep = _capture_until_output(built)
    args = dict(regions=[(0, 0, 0, 8, 8)], source="ycbcr")
    args.update(kw)
    with pytest.raises(ValueError, match="pull_boxes"):
        built.pull_boxes([a], **args)
    a.close()


def test_a_grid_above_the_cap_names_the_cap(built):
    a, keep = _capture_until_output(built)
    with pytest.raises(ValueError, match="pull_boxes.*16384"):
        built.pull_boxes([a], regions=[(0, 0, 0, 1920, 1080)], cell=8)
    with pytest.raises(ValueError, match="pull_boxes.*16384"):
        built.pull_boxes([a], regions=[(0, 0, 0, 8, 8)], grid=(129, 128))
    with pytest.raises(ValueError, match="pull_cells"):              # pull_cells keeps its own name in the shared checks
        built.pull_cells([a], regions=[(0, 0, 0, 8, 8)], cell=12)
    a.close()


class _Maps:
    def __init__(self, got):
        self.got = got


def test_views_sums_and_regions_on_a_hand_filled_buffer(built):
    import torch
    R, M = 3, 4
    buf = np.zeros((R, 1 + M, 8), np.int64)
    buf[0, 0, :4] = (6, 4, 40, 2)                                  # found above M: four written
    buf[0, 1:] = [(10 * k, 20 * k + 1, 16, 32, k + 1, 255, 7 + k, k) for k in range(M)]
    buf[0, 4, 6:] = (0xFFFFFFFF, 0xF)                              # sum 0xFFFFFFFFF: the low word is a negative int32
    buf[1] = 0x5A5A5A5A                                            # got 0: untouched, never read
    buf[2, 0, :4] = (1, 1, 3, 0)
    buf[2, 1] = (0, 0, 90, 60, 3, 9, 27, 0)
    boxes = torch.from_numpy(buf.astype(np.uint32).view(np.int32).reshape(R, 1 + M, 8).copy())
    cb = built.CellBoxes(_Maps([1, 0, 1]), boxes, [1, 0, 1])
    assert tuple(cb.header.shape) == (R, 8) and tuple(cb.records.shape) == (R, M, 8)
    assert cb.header[0].tolist() == [6, 4, 40, 2, 0, 0, 0, 0] and cb.records[0, 2].tolist() == [20, 41, 16, 32, 3, 255, 9, 2]
    sums = cb.sums()
    assert sums.dtype == torch.int64 and tuple(sums.shape) == (R, M)
    assert sums[0].tolist() == [7, 8 + (1 << 32), 9 + (2 << 32), 0xFFFFFFFFF] and sums[2].tolist() == [27, 0, 0, 0]
    assert cb.found == [6, 0, 1]
    assert cb.regions() == [(1, 0, 1, 16, 32), (1, 10, 21, 16, 32), (1, 20, 41, 16, 32), (1, 30, 61, 16, 32), (1, 0, 0, 90, 60)]
    assert cb.regions(pad=3)[1] == (1, 7, 18, 22, 38) and cb.regions(pad=3)[-1] == (1, -3, -3, 96, 66)
    assert cb.cells.got == [1, 0, 1] and cb.boxes is boxes


# ---- the model ----
def _scipy_slice(fg, values, connectivity, M):
    from scipy import ndimage
    structure = np.ones((3, 3), int) if connectivity == 8 else None
    lab, n = ndimage.label(fg, structure=structure)
    out = []
    for k, sl in enumerate(ndimage.find_objects(lab)[:M]):
        inside = lab[sl] == k + 1
        out.append((sl[1].start, sl[0].start, sl[1].stop - sl[1].start, sl[0].stop - sl[0].start, int(inside.sum()), int(values[sl][inside].max()),
                    int(values[sl][inside].sum())))
    return n, out


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("density", [0.3, 0.5, 0.6])
def test_model_equals_scipy_label_and_find_objects(connectivity, density):
    """scipy numbers its labels in raster order of their first cell too: the order, the rectangles, the cells, the peaks and the sums"""
    pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(int(density * 10) + connectivity)
    rows, cols, M = 37, 53, 512
    values = np.where(rng.random((rows, cols)) < density, rng.integers(1, 1000, (rows, cols)), 0)
    reach = np.ones((rows, cols), bool)
    got = bm.boxes(values, reach, (0, 0, cols, rows), (0, 0, cols, rows), 1, M, connectivity=connectivity)
    n, want = _scipy_slice(values > 0, values, connectivity, M)
    assert got[0].tolist() == [n, min(n, M), int((values > 0).sum()), 0, 0, 0, 0, 0] and n > 3
    assert [tuple(r[:7]) for r in got[1:1 + min(n, M)].tolist()] == want
    assert not got[1 + min(n, M):].any() and not got[1:, 7].any()


def test_model_min_cells_drops_before_numbering_and_m_truncates():
    v = np.zeros((6, 9), np.int64)
    v[0, 0] = 5                          # one cell
    v[0, 3:6] = (7, 9, 8)                # three
    v[2, 1], v[3, 2] = 4, 6              # two through a diagonal
    v[5, 8] = 1                          # one
    reach = np.ones_like(v, bool)
    geo = ((0, 0, 9, 6), (0, 0, 9, 6), 1)
    s = bm.boxes(v, reach, *geo, 8)
    assert s[0].tolist()[:4] == [4, 4, 7, 0]
    assert s[1:5].tolist() == [[0, 0, 1, 1, 1, 5, 5, 0], [3, 0, 3, 1, 3, 9, 24, 0], [1, 2, 2, 2, 2, 6, 10, 0], [8, 5, 1, 1, 1, 1, 1, 0]]
    s4 = bm.boxes(v, reach, *geo, 8, connectivity=4)
    assert s4[0].tolist()[:4] == [5, 5, 7, 0] and s4[3].tolist() == [1, 2, 1, 1, 1, 4, 4, 0] and s4[4].tolist() == [2, 3, 1, 1, 1, 6, 6, 0]
    s = bm.boxes(v, reach, *geo, 8, min_cells=2)
    assert s[0].tolist()[:4] == [2, 2, 7, 2] and s[1].tolist() == [3, 0, 3, 1, 3, 9, 24, 0] and s[2].tolist() == [1, 2, 2, 2, 2, 6, 10, 0] and not s[3:].any()
    s = bm.boxes(v, reach, *geo, 1, min_cells=2)                   # M = 1: found stays 2, one written, the first in raster order
    assert s.shape == (2, 8) and s[0].tolist()[:4] == [2, 1, 7, 2] and s[1].tolist() == [3, 0, 3, 1, 3, 9, 24, 0]
    s = bm.boxes(v, reach, *geo, 8, level=6)                       # value > 6: 7, 9, 8 only
    assert s[0].tolist()[:4] == [1, 1, 3, 0]
    s = bm.boxes(np.zeros((6, 9), np.int64), reach, *geo, 8)
    assert not s.any()


def test_model_below_never_takes_unreached_cells_and_rectangles_are_clipped():
    """window 90 x 60, box (-9, 10, 30, 20) at cell 8 on a 5 x 6 grid: column 0 lies outside the window, the box ends inside column 3
    (x = 21) and inside row 2 (y = 30); every value is 0, which passes BELOW 1"""
    window, box, cell, grid = (2, 2, 90, 60), (-9, 10, 30, 20), 8, (5, 6)
    reach = bm.reached(window, box, cell, grid)
    assert reach.astype(int).tolist() == [[0, 1, 1, 1, 0, 0]] * 3 + [[0] * 6] * 2
    s = bm.boxes(np.zeros(grid, np.int64), reach, window, box, cell, 4, sense=bm.BELOW, level=1)
    assert s[0].tolist()[:4] == [1, 1, 9, 0]
    assert s[1].tolist() == [0, 10, 21, 20, 9, 0, 0, 0]            # x from the window's edge, not -1; w to the box's end, not 24
    v = np.full(grid, 50, np.int64)
    v[1, 2] = 3
    s = bm.boxes(v, reach, window, box, cell, 4, sense=bm.BELOW, level=50)
    assert s[0].tolist()[:4] == [1, 1, 1, 0] and s[1].tolist() == [7, 18, 8, 8, 1, 3, 3, 0]
    assert not bm.boxes(v, reach, window, box, cell, 4, sense=bm.BELOW, level=0).any()
    big = np.full((128, 128), 64 * 255 * 255, np.int64)
    s = bm.boxes(big, np.ones((128, 128), bool), (0, 0, 1024, 1024), (0, 0, 1024, 1024), 8, 2)
    total = 16384 * 64 * 255 * 255
    assert total > 2 ** 32 and s[1].tolist() == [0, 0, 1024, 1024, 16384, 64 * 255 * 255, total & 0xFFFFFFFF, total >> 32]
