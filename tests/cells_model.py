"""numpy model of h264bsdmiOutputCellMaps (include/h264bsd_mi355x.h): the slice of one box, [P, rows, cols] int64.

The planes are stats_model.channels() of the I420 coded frame (PICTURE), or of two of them (CHANGE: the current picture and the kept
one).  maps() computes the slice directly: the box's grid, rows * cell x cols * cell luma positions from the box's origin, is cut out
of the planes padded with "not valid" (outside the box, outside the window), reshaped to [rows, cell, cols, cell] and reduced over the
two cell axes.  maps_by_records() computes the same cell by cell through stats_model.record / change_model.record at bins 0, which
is the interface's definition of a cell; tests/test_cell_maps_cpu.py holds the two against each other.

Map order: "count" if asked, then per requested plane in the order of PLANES[mode] the C channel maps.  DSUM is signed here; the
device writes it as an i32 in two's complement, which torch's int32 reads back signed."""
import numpy as np

import change_model
import stats_model
from stats_model import CHANNELS  # noqa: F401

PICTURE, CHANGE = 0, 1
PLANES = ({"count": 1, "sum": 2, "sumsq": 4, "min": 8, "max": 16}, {"count": 1, "sad": 2, "ssd": 4, "dsum": 8, "dmax": 16, "above": 32})
CELLS = (4, 8, 16, 32, 64)


def plane_bits(mode, names):
    return sum({PLANES[mode][n] for n in names})


def n_maps(mode, C, bits):
    return (bits & 1) + C * bin(bits >> 1).count("1")


def default_grid(sizes, cell):
    """(rows, cols) for boxes / windows of the (h, w) in sizes"""
    return max([-(-h // cell) for h, _ in sizes] + [1]), max([-(-w // cell) for _, w in sizes] + [1])


def _grid_cut(planes, window, box, cell, grid):
    """([C, rows * cell, cols * cell] int64 values, [rows * cell, cols * cell] bool valid) of the box's grid"""
    C, H, W = planes.shape
    wx, wy, ww, wh = window
    x, y, w, h = box
    rows, cols = grid
    v = np.arange(rows * cell)[:, None]
    u = np.arange(cols * cell)[None, :]
    valid = (u < w) & (v < h) & (x + u >= 0) & (x + u < ww) & (y + v >= 0) & (y + v < wh)
    Y = np.clip(wy + y + v, 0, H - 1)
    X = np.clip(wx + x + u, 0, W - 1)
    return planes[:, Y, X].astype(np.int64), valid


def _cells(a, cell, grid):
    rows, cols = grid
    return a.reshape(a.shape[:-2] + (rows, cell, cols, cell))


def maps(mode, bits, cur, kept, window, box, cell, grid, threshold=(0, 0, 0)):
    """the slice [P, rows, cols] int64.  cur, kept: [C, H, W] planes (kept: None in PICTURE mode); window (x0, y0, w, h) in the coded
    frame; box (x, y, w, h) relative to the window; grid (rows, cols)"""
    C = cur.shape[0]
    a, valid = _grid_cut(cur, window, box, cell, grid)
    out = []
    count = _cells(valid.astype(np.int64), cell, grid).sum((-3, -1))
    if bits & 1:
        out.append(count[None])
    vm = valid[None]
    if mode == PICTURE:
        if bits & 2:
            out.append(_cells(np.where(vm, a, 0), cell, grid).sum((-3, -1)))
        if bits & 4:
            out.append(_cells(np.where(vm, a * a, 0), cell, grid).sum((-3, -1)))
        if bits & 8:
            out.append(_cells(np.where(vm, a, 255), cell, grid).min((-3, -1)))
        if bits & 16:
            out.append(_cells(np.where(vm, a, 0), cell, grid).max((-3, -1)))
    else:
        b, _ = _grid_cut(kept, window, box, cell, grid)
        d = np.where(vm, a - b, 0)
        ad = np.abs(d)
        thr = np.asarray(list(threshold)[:C], np.int64)[:, None, None]
        if bits & 2:
            out.append(_cells(ad, cell, grid).sum((-3, -1)))
        if bits & 4:
            out.append(_cells(d * d, cell, grid).sum((-3, -1)))
        if bits & 8:
            out.append(_cells(d, cell, grid).sum((-3, -1)))
        if bits & 16:
            out.append(_cells(ad, cell, grid).max((-3, -1)))
        if bits & 32:
            out.append(_cells((ad > thr).astype(np.int64), cell, grid).sum((-3, -1)))
    res = np.concatenate(out, 0)
    assert res.shape == (n_maps(mode, C, bits),) + tuple(grid)
    return res


def cell_box(box, cell, i, j):
    """the box of cell (i, j) of the grid over `box`; w or h <= 0: beyond the box"""
    x, y, w, h = box
    return x + j * cell, y + i * cell, min(cell, w - j * cell), min(cell, h - i * cell)


def maps_by_records(mode, bits, cur, kept, window, box, cell, grid, threshold=(0, 0, 0)):
    """the same slice, every cell from the sibling's record of cell_box()"""
    C = cur.shape[0]
    rows, cols = grid
    res = np.zeros((n_maps(mode, C, bits), rows, cols), np.int64)
    for i in range(rows):
        for j in range(cols):
            cb = cell_box(box, cell, i, j)
            if cb[2] <= 0 or cb[3] <= 0:
                cb = (0, 0, 1, 1)
                window_ij = (0, 0, 0, 0)             # nothing of it is inside: the record of a box that misses the window
            else:
                window_ij = window
            if mode == PICTURE:
                r = stats_model.record(cur, window_ij, cb, 0)
                fields = [(2, r.sum), (4, r.sumsq), (8, r.min), (16, r.max)]
            else:
                r = change_model.record(cur, kept, window_ij, cb, 0, threshold)
                fields = [(2, r.sad), (4, r.ssd), (8, r.sum), (16, r.max), (32, r.above)]
            at = 0
            if bits & 1:
                res[at, i, j] = r.count
                at += 1
            for bit, val in fields:
                if bits & bit:
                    res[at:at + C, i, j] = val
                    at += C
    return res
