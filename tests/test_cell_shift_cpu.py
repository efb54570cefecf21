"""No GPU: the symbol of the cell shift (declared, exported, mirrored), the struct and the constants against the header, what
h264bsdmiOutputCellShift refuses before it looks at a device (through the built library, on parser-only instances), the argument errors
of pull_flow, the plane order and the views of CellShift on a hand-filled buffer, and the numpy model (tests/flow_model.py): the
vectorised form against the cell-by-cell records of tests/shift_model.py, which is the interface's definition."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import flow_model as fm
import shift_model as shm
from conftest import ROOT
from test_tensor_output import _capture_until_output

SENTINEL = 0xA5A5A5A5
CONSTANTS = dict(H264BSDMI_FLOW_COUNT=1, H264BSDMI_FLOW_DX=2, H264BSDMI_FLOW_DY=4, H264BSDMI_FLOW_BEST=8, H264BSDMI_FLOW_STILL=16,
                 H264BSDMI_FLOW_TIES=32)
SYMBOL = "h264bsdmiOutputCellShift"


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_symbol_is_declared_exported_and_mirrored(built):
    text = open(os.path.join(ROOT, "include", "h264bsd_mi355x.h")).read()
    built.lib()
    assert re.search(r"\bint\s+" + SYMBOL + r"\s*\(", text)
    assert SYMBOL in built.EXPORTED_SYMBOLS
    assert SYMBOL in _exported(built.LIB_PATH) and SYMBOL in _exported(built.capi.BENCH_LIB_PATH)
    for attr in ("pull_flow", "CellShiftSpec", "CellShift"):
        assert hasattr(built, attr)
    assert tuple(int(v) for v in built.__version__.split(".")) >= (0, 10, 0)
    doc = text[text.index("/* Cell shift:"):text.index(SYMBOL + "(")]
    assert "THE DEFINITION" in doc and "min(cell, w - j cell)" in doc and "Cell 4 is left out on purpose" in doc
    assert "need no H264BSDMI_SHIFT_MAX_SIDE cap" in doc


def test_spec_layout_and_constants_match_the_header(built, tmp_path):
    fields = [f[0] for f in built.CellShiftSpec._fields_]
    assert fields == ["data", "cols", "rows", "cell", "radius", "planes", "crop", "keep_after"]
    src = tmp_path / "spec.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "h264bsd_mi355x.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(h264bsdmi_cell_shift_spec));\n' +
                   "".join(f'    printf("%zu\\n", offsetof(h264bsdmi_cell_shift_spec, {f}));\n' for f in fields) +
                   "".join(f'    printf("%u\\n", (unsigned){c});\n' for c in CONSTANTS) + "    return 0;\n}\n")
    exe = tmp_path / "spec"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(built.CellShiftSpec)] + [getattr(built.CellShiftSpec, f).offset for f in fields] + list(CONSTANTS.values())
    assert built.capi.FLOW_PLANES == fm.PLANES == {k.split("_")[-1].lower(): v for k, v in CONSTANTS.items()}
    assert built.capi.FLOW_CELL_SIZES == fm.CELLS == (8, 16, 32, 64)


def _spec(built, **kw):
    s = dict(data=0x1000, cols=6, rows=5, cell=8, radius=4, planes=63, crop=1, keep_after=0)
    s.update(kw)
    return built.CellShiftSpec(s["data"], s["cols"], s["rows"], s["cell"], s["radius"], s["planes"], s["crop"], s["keep_after"])


def _call(built, decoders, regions, spec, null_regions=False, null_got=False, n_regions=None):
    """(rc, got, current, kept, picId, keptPicId) of one raw call; the output arrays start as SENTINEL"""
    L = built.api_lib()
    n, K = len(decoders), len(regions) if n_regions is None else n_regions
    got = (ctypes.c_uint32 * max(K, 1))(*([SENTINEL] * max(K, 1)))
    per = [(ctypes.c_uint32 * max(n, 1))(*([SENTINEL] * max(n, 1))) for _ in range(4)]
    dec = (ctypes.c_void_p * max(n, 1))(*[d._st for d in decoders])
    regs = (built.Region * max(len(regions), 1))(*[built.Region(*r) for r in regions])
    rc = L.h264bsdmiOutputCellShift(n, dec, K, None if null_regions else regs, ctypes.byref(spec), None, None if null_got else got, *per)
    return (rc, list(got)) + tuple(list(a) for a in per)


def test_an_empty_call_with_a_valid_spec_is_accepted_and_launches_nothing(built):
    for cell in fm.CELLS:
        for kw in (dict(), dict(radius=0), dict(radius=16, keep_after=1), dict(planes=1), dict(planes=32), dict(cols=4096, rows=4096),
                   dict(cols=1, rows=1), dict(data=0x1004), dict(crop=0)):
            res = _call(built, [], [], _spec(built, cell=cell, **kw))
            assert res[0] == 0 and res[1] == [SENTINEL], (cell, kw)
    assert _call(built, [], [], _spec(built), null_regions=True, null_got=True)[0] == 0        # regions == NULL, nRegions == n == 0


BAD_SPEC = [dict(data=0), dict(data=0x1002), dict(data=0x1001), dict(cols=0), dict(rows=0), dict(cols=4097), dict(rows=4097),
            dict(cols=2 ** 32 - 1), dict(cell=0), dict(cell=4), dict(cell=12), dict(cell=128), dict(cell=2 ** 31), dict(radius=17),
            dict(radius=2 ** 32 - 1), dict(planes=0), dict(planes=64), dict(planes=2 ** 31 | 1), dict(crop=2), dict(keep_after=2)]


@pytest.mark.parametrize("bad", BAD_SPEC)
def test_invalid_specs_are_refused_before_the_instances(built, bad):
    assert _call(built, [], [], _spec(built, **bad))[0] == -1
    assert built.api_lib().h264bsdmiOutputCellShift(0, None, 0, None, None, None, None, None, None, None, None) == -1      # no spec at all


def test_every_refusal_is_minus_one_and_nothing_is_written_or_popped(built):
    """an instance in capture mode has no pixels: every call that names it is refused; the sentinels stay, and the instance's output
    queue is what an untouched twin's is.  A region may be larger than the region shift's 4096: the refusal is not for its size"""
    a, keep_a = _capture_until_output(built)
    b, keep_b = _capture_until_output(built)
    spec = _spec(built)
    untouched = (-1, [SENTINEL]) + ([SENTINEL],) * 4
    for good in [(0, 0, 0, 16, 16), (0, -5, 3, 17, 31), (0, 16384, -16384, 16384, 16384)]:
        assert _call(built, [a], [good], spec) == untouched
    for bad in [(1, 0, 0, 16, 16), (0, 0, 0, 0, 16), (0, 0, 0, 16, 16385), (0, 16385, 0, 16, 16), (0, 0, -16385, 16, 16)]:
        assert _call(built, [a], [bad], spec) == untouched, bad
    for bad in BAD_SPEC:
        assert _call(built, [a], [(0, 0, 0, 16, 16)], _spec(built, **bad)) == untouched, bad
    assert _call(built, [a], [(0, 0, 0, 16, 16)] * 2, spec, null_regions=True)[0] == -1      # regions == NULL with nRegions != n
    assert _call(built, [a], [(0, 0, 0, 16, 16)], spec, null_got=True)[0] == -1
    assert _call(built, [a], [(0, 0, 0, 16, 16)], spec, n_regions=65536)[0] == -1
    res = _call(built, [a, a], [(0, 0, 0, 16, 16), (1, 0, 0, 16, 16)], spec)
    assert res[0] == -1 and res[1] == [SENTINEL] * 2 and res[2] == [SENTINEL] * 2
    info = a.next_output_info()
    assert info is not None and info == b.next_output_info()
    a.close()
    b.close()


@pytest.mark.parametrize("kw", [dict(cell=4), dict(cell=12), dict(cell=128), dict(radius=17), dict(radius=-1), dict(radius=2.0), dict(radius=True),
                                dict(planes=()), dict(planes=("sad",)), dict(planes=("dx", "surface")), dict(grid=(0, 4)), dict(grid=(4, 4097)),
                                dict(grid=7), dict(grid=(2.0, 2)), dict(regions=[(0, 0, 0, 0, 8)]), dict(regions=[(1, 0, 0, 8, 8)]),
                                dict(regions=[(0, 0, 0, 8, 8)] * 65536)])
def test_pull_flow_refuses_bad_arguments(built, kw, monkeypatch):
    """before any library call: the entry point is taken away for the test, so a refusal that came too late would not be a ValueError"""
    a, keep = _capture_until_output(built)
    monkeypatch.setattr(built.capi, "_kept_pull", lambda *args, **kws: pytest.fail("the library was called"))
    args = dict(regions=[(0, 0, 0, 8, 8)])
    args.update(kw)
    with pytest.raises(ValueError, match="pull_flow"):
        built.pull_flow([a], **args)
    a.close()


class _Buffer:
    """what CellShift needs of a tensor: slicing"""

    def __init__(self, a):
        self.a = a

    def __getitem__(self, k):
        return self.a[k]


@pytest.mark.parametrize("names", [("dx",), ("ties",), ("dx", "dy", "best"), ("still", "best"), ("ties", "still", "best", "dy", "dx", "count")])
def test_plane_order_views_and_gain_on_a_hand_filled_buffer(built, names):
    """map p of a slice is filled with p: the planes in ascending bit order whatever order they were named in"""
    bits = fm.plane_bits(names)
    P = bin(bits).count("1")
    R, rows, cols = 2, 3, 4
    maps = np.broadcast_to(np.arange(P, dtype=np.int32)[None, :, None, None] * 10, (R, P, rows, cols)).copy()
    maps[1] += 100
    cs = built.CellShift(_Buffer(maps), 16, 4, bits, [1, 1], [1], [1], [7], [6])
    at = 0
    for name, bit in built.capi.FLOW_PLANES.items():
        view = getattr(cs, name)
        if not bits & bit:
            assert view is None, name
            continue
        assert view.shape == (R, rows, cols) and (view[0] == 10 * at).all() and (view[1] == 10 * at + 100).all(), name
        at += 1
    assert at == P and (cs.got, cs.current, cs.kept, cs.pic_id, cs.kept_pic_id) == ([1, 1], [1], [1], [7], [6])
    if bits & 8 and bits & 16:
        assert cs.gain.shape == (R, rows, cols) and (cs.gain == 10).all()           # still is the map behind best
    else:
        with pytest.raises(ValueError, match="gain"):
            cs.gain


# ---- the model: the vectorised form against the cell-by-cell records, which are the definition ----
W, H = 112, 80
WINDOW = (2, 3, 93, 61)                                 # at no macroblock edge
MODEL_BOXES = [(0, 0, 93, 61), (13, 11, 37, 23), (-9, 10, 30, 20), (70, -5, 40, 20), (5, 50, 9, 30), (-40, 0, 30, 30), (95, 3, 10, 10), (200, 200, 8, 8)]


@pytest.fixture(scope="module")
def pair():
    rng = np.random.default_rng(31)
    kept = rng.integers(0, 256, (H, W), dtype=np.uint8)
    cur = np.roll(kept, (2, -1), axis=(0, 1))
    cur[40:, :] = rng.integers(0, 256, (H - 40, W), dtype=np.uint8)
    cur[:8, :40] = 90
    kept[:8, :40] = 90                                  # a flat corner: ties
    return kept, cur


@pytest.mark.parametrize("radius", [0, 1, 3, 16])
@pytest.mark.parametrize("cell", fm.CELLS)
def test_the_two_forms_of_the_model_are_equal(pair, cell, radius):
    """windows at no macroblock edge; boxes with negative origins, boxes that leave and miss the window, widths that are no multiple of
    4 or of the cell; grids smaller and larger than the box"""
    kept, cur = pair
    boxes = MODEL_BOXES if radius < 16 else MODEL_BOXES[1:4] + MODEL_BOXES[-1:]
    for box in boxes:
        for grid in (fm.default_grid([(box[3], box[2])], cell), (5, 6), (1, 2)):
            if radius == 16 and grid == (5, 6) and cell == 8:
                continue                                # (the slow form at its slowest; the other two grids cover it)
            a = fm.maps(kept, cur, WINDOW, box, cell, grid, radius)
            b = fm.maps_fast(kept, cur, WINDOW, box, cell, grid, radius)
            assert np.array_equal(a, b), (box, grid, np.argwhere(a != b)[:4])
            assert a.shape == (6,) + tuple(grid)


def test_model_geometry_ties_and_the_record_of_nothing(pair):
    kept, cur = pair
    m = fm.maps(kept, cur, WINDOW, (13, 11, 37, 23), 8, (5, 6), 3)
    assert m[0, 0].tolist() == [64, 64, 64, 64, 40, 0] and m[0, :, 0].tolist() == [64, 64, 56, 0, 0]     # a last column 5 wide, a last row 7 tall
    assert (m[5][m[0] == 0] == 49).all() and not m[1:5][:, m[0] == 0].any()
    r = shm.record(kept, cur, WINDOW, (13 + 8, 11 + 8, 8, 8), 3)
    assert m[:, 1, 1].tolist() == [r.count, r.dx, r.dy, r.best, r.still, r.ties] and (r.dx, r.dy, r.best) == (-1, 2, 0)
    miss = fm.maps(kept, cur, WINDOW, (200, 200, 8, 8), 8, (2, 2), 16)
    assert not miss[:5].any() and (miss[5] == 33 * 33).all()
    flat = fm.maps(kept, cur, (0, 0, 40, 8), (0, 0, 40, 8), 8, (1, 5), 3)
    assert (flat[5] == 49).all() and not flat[1:5].any()                                                    # every displacement ties: (0, 0)
    small = fm.maps(kept, cur, WINDOW, (13, 11, 37, 23), 8, (2, 3), 3)
    assert np.array_equal(small, m[:, :2, :3])
    assert np.array_equal(fm.select(m, fm.plane_bits(("ties", "dx"))), m[[1, 5]])
