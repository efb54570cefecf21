"""GPU: h264bsdmiOutputCellShift / pull_flow through the product library.  The pictures are chosen (tests/pcm_pictures.py, as in
test_gpu_region_shift.py), so both the kept and the current picture are known exactly, and every map is compared with
tests/flow_model.py element for element.  Every call writes into a buffer that starts as a pattern: the whole slice is written, and an
untouched slice stays untouched.  The golden stream runs beside a twin decoder and is compared with the merged siblings, pull_shift and
pull_cells."""
import os
import re

import numpy as np
import pytest

import flow_model as fm
import pcm_pictures as pp
from conftest import ROOT
from test_gpu_region_change import Pair
from test_gpu_region_shift import CROP, H, SHIFT, W, Chosen, _picture, _shifted
from test_gpu_tensor_colour import Feed

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
ALL = ("count", "dx", "dy", "best", "still", "ties")
BOXES = [None, (-9, 10, 30, 20), (50, -7, 25, 19), (13, 11, 37, 23), (200, 200, 8, 8)]     # None: the whole window


@pytest.fixture(autouse=True, scope="module")
def _through_the_product_library(built):
    built.use_product_library(True)
    yield
    built.use_product_library(False)


@pytest.fixture(autouse=True)
def _no_device_errors(built):
    yield
    assert built.device_errors() == 0


def _pull(built, decs, regions, cell, grid, radius, planes=ALL, **kw):
    """pull_flow into a buffer that starts as FILL -> (CellShift, maps as int64 on the host)"""
    import torch
    K = len(decs) if regions is None else len(regions)
    out = torch.full((K, len(set(planes)), grid[0], grid[1]), FILL, dtype=torch.int32, device="cuda")
    cs = built.pull_flow(decs, regions, cell=cell, grid=grid, radius=radius, planes=planes, out=out, **kw)
    assert cs.maps is out
    return cs, out.cpu().numpy().astype(np.int64)


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, [(tuple(k), int(got[tuple(k)]), int(want[tuple(k)])) for k in np.argwhere(got != want)[:6]])


@pytest.fixture(scope="module", params=[False, True], ids=["coded", "cropped"])
def small(request, built, _through_the_product_library):
    rng = np.random.default_rng(5)
    K = rng.integers(0, 256, (H, W), dtype=np.uint8)
    c = Chosen(built, [K, _shifted(K, *SHIFT)], crop=CROP["crop"] if request.param else None)
    c.window = CROP["window"] if request.param else (0, 0, W, H)
    yield c
    c.close()


@pytest.mark.parametrize("radius", [0, 1, 3, 16])
@pytest.mark.parametrize("cell", fm.CELLS)
def test_whole_windows_of_a_shifted_pair_equal_the_model(built, small, cell, radius):
    """radius 16 exceeds the cell and a macroblock; cell 64 exceeds the picture's height: one partial cell.  The guard: where the search
    can see the shift every cell of the coded window answers it, and in the cropped window 35 of 40 cells of 8"""
    ww, wh = small.window[2:]
    grid = fm.default_grid([(wh, ww)], cell)
    want = fm.maps_fast(small.lumas[0], small.lumas[1], small.window, (0, 0, ww, wh), cell, grid, radius)
    if radius >= 3:
        found = int(((want[1] == SHIFT[0]) & (want[2] == SHIFT[1])).sum())
        if small.window == (0, 0, W, H):
            assert found == grid[0] * grid[1] == {8: 48, 16: 12, 32: 4, 64: 1}[cell]
        elif cell == 8:
            assert (found, grid[0] * grid[1]) == (35, 40)
    if radius <= 3 and cell >= 16:                      # the definition itself, where it is quick
        assert np.array_equal(want, fm.maps(small.lumas[0], small.lumas[1], small.window, (0, 0, ww, wh), cell, grid, radius))
    cs, got = _pull(built, [small.dec], None, cell, grid, radius)
    assert cs.got == [1] and cs.current == [1] and cs.kept == [1]
    _same(got[0], want, (cell, radius))
    for k, name in enumerate(ALL):
        assert np.array_equal(getattr(cs, name).cpu().numpy()[0], want[k]), name
    assert np.array_equal(cs.gain.cpu().numpy()[0], want[4] - want[3])
    default = built.pull_flow([small.dec], cell=cell, radius=radius, planes=ALL, crop=True)      # the default grid is the window's
    assert tuple(default.maps.shape) == (1, 6) + grid
    _same(default.maps.cpu().numpy().astype(np.int64)[0], want, "default grid")


@pytest.mark.parametrize("cell,grid,radius", [(8, (4, 6), 3), (16, (2, 3), 3), (8, (4, 9), 16), (32, (2, 1), 1)])
def test_boxes_in_one_call_equal_the_model(built, small, cell, grid, radius):
    """the whole window, boxes with negative origins that leave the window, width 37 (the masked last dword, a last cell 5 wide), one
    that misses (ties = D D everywhere); the grid is smaller than the largest box and larger than the smallest"""
    ww, wh = small.window[2:]
    boxes = [b or (0, 0, ww, wh) for b in BOXES]
    assert grid[0] * cell < wh or grid[1] * cell < ww
    assert grid[0] * cell > 8 and grid[1] * cell > 8
    want = [fm.maps_fast(small.lumas[0], small.lumas[1], small.window, b, cell, grid, radius) for b in boxes]
    if radius == 3:
        for k, b in enumerate(boxes):
            assert np.array_equal(want[k], fm.maps(small.lumas[0], small.lumas[1], small.window, b, cell, grid, radius)), b
    assert not want[4][:5].any() and (want[4][5] == (2 * radius + 1) ** 2).all()
    if cell == 8 and radius == 3:
        assert want[3][0, 0].tolist() == [64, 64, 64, 64, 40, 0][:grid[1]]
    cs, got = _pull(built, [small.dec], [(0,) + b for b in boxes], cell, grid, radius)
    assert cs.got == [1] * len(boxes)
    for k, b in enumerate(boxes):
        _same(got[k], want[k], (b, cell, grid, radius))


def test_ties_on_a_checkerboard_and_on_a_flat_pair(built):
    """kept: the one-sample checkerboard, current: the same moved by (1, 0): every cell finds a perfect match at several
    displacements, and which one the rule names depends on the window's edge: all three levels of the rule decide somewhere"""
    x, y = np.arange(W)[None, :], np.arange(H)[:, None]
    board = (((x + y) & 1) * 200).astype(np.uint8)
    c = Chosen(built, [board, _shifted(board, 1, 0)])
    for cell in (8, 16):
        grid = fm.default_grid([(H, W)], cell)
        want = fm.maps(board, c.lumas[1], (0, 0, W, H), (0, 0, W, H), cell, grid, 3)
        assert not want[3].any()
        assert set(zip(want[1].ravel().tolist(), want[2].ravel().tolist())) == {(-1, 0), (1, 0), (0, -1)}
        assert want[5].min() == 6 and want[5].max() == 24
        _same(_pull(built, [c.dec], None, cell, grid, 3)[1][0], want, ("board", cell))
    c.close()
    flat = np.full((H, W), 77, np.uint8)
    c = Chosen(built, [flat, flat])
    for cell, radius in ((8, 3), (16, 16)):
        grid = fm.default_grid([(H, W)], cell)
        got = _pull(built, [c.dec], None, cell, grid, radius)[1][0]
        assert not got[1:5].any() and (got[5] == (2 * radius + 1) ** 2).all() and got[0].sum() == W * H
    c.close()


def test_more_than_one_rectangle_each_way(built):
    """two of the kernel's rectangles and a partial one wide and high; the content moves by a different shift in each quadrant"""
    kernel = open(os.path.join(ROOT, "h264bsd_amd", "csrc", "kernels", "k_cell_shift.hip.h")).read()
    RW, RH = (int(v) for v in re.search(r"FLOW_RECT_W = (\d+), FLOW_RECT_H = (\d+);", kernel).groups())
    BW, BH = 2 * RW + 32, 2 * RH + 16
    rng = np.random.default_rng(17)
    K = rng.integers(0, 256, (BH, BW), dtype=np.uint8)
    C = K.copy()
    shifts = {(0, 0): (2, 1), (0, 1): (-3, 0), (1, 0): (0, -2), (1, 1): (1, 3)}
    for (qi, qj), s in shifts.items():
        ys, xs = slice(qi * BH // 2, (qi + 1) * BH // 2), slice(qj * BW // 2, (qj + 1) * BW // 2)
        C[ys, xs] = _shifted(K, *s)[ys, xs]
    c = Chosen(built, [K, C])
    for cell, radius in ((16, 3), (8, 1)):
        grid = fm.default_grid([(BH, BW)], cell)
        assert grid[1] * cell > 2 * RW and grid[0] * cell > 2 * RH
        want = fm.maps_fast(K, C, (0, 0, BW, BH), (0, 0, BW, BH), cell, grid, radius)
        if radius == 3:                                 # well inside each quadrant its shift is found
            for (qi, qj), s in shifts.items():
                i, j = (qi * BH // 2 + BH // 4) // cell, (qj * BW // 2 + BW // 4) // cell
                assert (want[1, i, j], want[2, i, j], want[3, i, j]) == (s[0], s[1], 0)
        _same(_pull(built, [c.dec], None, cell, grid, radius)[1][0], want, ("rectangles", cell, radius))
    # a box whose origin is negative: the rectangles' edges are at no multiple of anything in the frame
    box, grid = (-21, -13, 150, 120), (6, 9)
    want = fm.maps_fast(K, C, (0, 0, BW, BH), box, 16, grid, 3)
    _same(_pull(built, [c.dec], [(0,) + box], 16, grid, 3)[1][0], want, "negative origin")
    c.close()


@pytest.mark.parametrize("planes", [("dx",), ("ties",), ("ties", "dx"), ALL])
def test_plane_subsets_follow_the_bits(built, small, planes):
    ww, wh = small.window[2:]
    grid = fm.default_grid([(wh, ww)], 8)
    want = fm.maps_fast(small.lumas[0], small.lumas[1], small.window, (0, 0, ww, wh), 8, grid, 3)
    cs, got = _pull(built, [small.dec], None, 8, grid, 3, planes=planes)
    _same(got[0], fm.select(want, fm.plane_bits(planes)), planes)
    assert [name for name in ALL if getattr(cs, name) is not None] == [name for name in ALL if name in planes]
    if not ("best" in planes and "still" in planes):
        with pytest.raises(ValueError):
            cs.gain


def _luma(pair, frame):
    w, h = pair.frame_size
    return frame[:w * h].reshape(h, w)


def test_against_the_merged_siblings_on_real_content(built):
    """two decoders on the 640x360 stream at different pictures: every cell of 32 at radius 4 is what pull_shift gives for the cell as
    a region, field for field, and still is pull_cells' luma sad against the kept picture"""
    pairs = [Pair(built, "test_640x360"), Pair(built, "test_640x360")]
    for p, ahead in zip(pairs, (1, 3)):
        p.advance(ahead)
        p.keep()
        p.advance(2)
    decs = [p.dec for p in pairs]
    cell, grid = 32, (12, 20)
    cs, got = _pull(built, decs, None, cell, grid, 4)
    assert cs.got == [1, 1] and cs.kept == [1, 1] and cs.kept_pic_id == [p.kept_id for p in pairs] and cs.pic_id == [p.pic_id for p in pairs]
    regions = [(d, j * cell, i * cell, min(cell, 640 - j * cell), min(cell, 360 - i * cell)) for d in range(2) for i in range(grid[0]) for j in range(grid[1])]
    sh = built.pull_shift(decs, regions, radius=4)
    assert sh.got == [1] * len(regions)
    for k, name in enumerate(ALL):
        sib = getattr(sh, name).cpu().numpy().astype(np.int64).reshape(2, grid[0], grid[1])
        _same(got[:, k], sib, ("pull_shift", name))
    cells = built.pull_cells(decs, cell=cell, grid=grid, source="y", planes=("sad",), against="kept")
    _same(got[:, 4], cells.sad.cpu().numpy().astype(np.int64)[:, 0], "pull_cells sad")
    assert got[:, 4].any() and (got[:, 3] <= got[:, 4]).all()
    want = fm.maps_fast(_luma(pairs[0], pairs[0].kept), _luma(pairs[0], pairs[0].frame), pairs[0].window(True), (0, 0, 640, 360), cell, grid, 4)
    _same(got[0], want, "model")
    for p in pairs:
        p.close()


def test_three_instances_mixed_regions_and_the_keep_chain(built):
    """three decoders of different picture sizes in one call, regions interleaved; one has no kept picture: got 0, its slices stay the
    pattern.  keep=True: the second call compares with the first call's pictures"""
    rng = np.random.default_rng(29)
    sizes = [(64, 48), (96, 80), (48, 32)]
    lumas = [[rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(3)] for w, h in sizes]
    a, b = Chosen(built, lumas[0]), Chosen(built, lumas[1])
    fresh = Feed(built, pp.pcm_stream([_picture(Y) for Y in lumas[2]]))       # a current picture, nothing kept
    assert fresh.step() and fresh.dec.next_output_info() is not None
    decs = [a.dec, fresh.dec, b.dec]
    regions = [(2, 0, 0, 96, 80), (0, -5, 3, 40, 30), (1, 0, 0, 48, 32), (2, 10, -4, 50, 33), (0, 0, 0, 64, 48), (1, 3, 3, 20, 20)]
    cell, grid, radius = 8, (5, 7), 2
    cs, got = _pull(built, decs, regions, cell, grid, radius, keep=True)
    assert cs.got == [1, 1, 0, 1, 1, 0] and cs.current == [1, 1, 1] and cs.kept == [1, 0, 1]
    first_ids = cs.pic_id
    for k, (d, *box) in enumerate(regions):
        if d == 1:
            assert (got[k] == FILL).all()
            continue
        w, h = sizes[0 if d == 0 else 1]
        ls = lumas[0 if d == 0 else 1]
        _same(got[k], fm.maps_fast(ls[0], ls[1], (0, 0, w, h), tuple(box), cell, grid, radius), ("first", k))
    # the chain: everyone's kept picture is now the current one of the first call; a and b decode on, fresh stays
    a.next()
    b.next()
    cs, got = _pull(built, decs, regions, cell, grid, radius)
    assert cs.got == [1] * 6 and cs.kept == [1, 1, 1] and cs.kept_pic_id == first_ids
    pics = {0: (lumas[0][1], lumas[0][2], sizes[0]), 1: (lumas[2][0], lumas[2][0], sizes[2]), 2: (lumas[1][1], lumas[1][2], sizes[1])}
    for k, (d, *box) in enumerate(regions):
        kept, cur, (w, h) = pics[d]
        want = fm.maps_fast(kept, cur, (0, 0, w, h), tuple(box), cell, grid, radius)
        _same(got[k], want, ("second", k))
        if d == 1:
            assert not want[1:5].any()                  # the same picture twice: (0, 0), best 0
    for c in (a, b, fresh):
        c.close()


def test_raw_calls_that_must_be_refused_write_nothing(built, small):
    import ctypes
    import torch
    L = built.api_lib()
    out = torch.full((2, 6, 3, 4), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    S = 0xA5A5A5A5

    def call(decs, regs, data=None, cols=4, rows=3, cell=16, radius=1, planes=63, crop=1, keep_after=0):
        spec = built.CellShiftSpec(out.data_ptr() if data is None else data, cols, rows, cell, radius, planes, crop, keep_after)
        arrays = [(ctypes.c_uint32 * 2)(S, S) for _ in range(5)]
        regions = (built.Region * 2)(*[built.Region(*r) for r in regs])
        rc = L.h264bsdmiOutputCellShift(len(decs), (ctypes.c_void_p * len(decs))(*decs), 2, regions, ctypes.byref(spec), None, *arrays)
        return rc, [list(a) for a in arrays]

    good = [(0, 0, 0, 16, 16), (0, 10, 10, 8, 8)]
    untouched = (-1, [[S, S]] * 5)
    d = small.dec._st
    assert call([d, d], good) == untouched                               # repeated instances
    for bad in (dict(radius=17), dict(cell=4), dict(cell=24), dict(cols=0), dict(rows=4097), dict(planes=0), dict(planes=64), dict(crop=2),
                dict(keep_after=2), dict(data=out.data_ptr() + 2), dict(data=0)):
        assert call([d], good, **bad) == untouched, bad
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    rc, arrays = call([d], good)
    assert rc == 0 and arrays[0] == [1, 1]
    torch.cuda.synchronize()
    for k, r in enumerate(good):
        _same(out[k].cpu().numpy().astype(np.int64), fm.maps(small.lumas[0], small.lumas[1], small.window, r[1:], 16, (3, 4), 1), ("raw", k))
