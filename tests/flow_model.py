"""numpy model of h264bsdmiOutputCellShift (include/h264bsd_mi355x.h): the slice of one box, [6, rows, cols] int64 in the order of the
bits: count, dx, dy, best, still, ties.

kept, cur: [H, W] uint8 luma planes of two coded frames; window (x0, y0, w, h) in the coded frame; box (x, y, w, h) relative to the
window.  maps() IS the definition: cell (i, j) holds the fields of shift_model.record for the box (x + j cell, y + i cell,
min(cell, w - j cell), min(cell, h - i cell)), and a cell the box does not reach at all is the record of nothing.  maps_fast() is the
same quantity computed the other way round — one |kept - cur(+dx, +dy)| plane per displacement over box ∩ window, summed per cell with
np.add.reduceat, then the argmin under the tie rule for all cells at once; it is compared only against maps() (tests/
test_cell_shift_cpu.py) and exists so that the larger GPU cases stay in seconds."""
import numpy as np

import shift_model as shm

PLANES = {"count": 1, "dx": 2, "dy": 4, "best": 8, "still": 16, "ties": 32}
CELLS = (8, 16, 32, 64)


def plane_bits(names):
    return sum({PLANES[n] for n in names})


def select(maps6, bits):
    """the maps of the set bits, in ascending order, as the call lays them out"""
    return maps6[[k for k in range(6) if bits >> k & 1]]


def default_grid(sizes, cell):
    """(rows, cols) that cover the largest of the (h, w)"""
    return (max([-(-h // cell) for h, _ in sizes] + [1]), max([-(-w // cell) for _, w in sizes] + [1]))


def maps(kept, cur, window, box, cell, grid, R):
    rows, cols = grid
    x, y, w, h = box
    D = 2 * R + 1
    out = np.zeros((6, rows, cols), np.int64)
    out[5] = D * D
    for i in range(rows):
        for j in range(cols):
            cw, ch = min(cell, w - j * cell), min(cell, h - i * cell)
            if cw <= 0 or ch <= 0:
                continue                                # beyond the box: the formula applied to nothing
            r = shm.record(kept, cur, window, (x + j * cell, y + i * cell, cw, ch), R)
            out[:, i, j] = (r.count, r.dx, r.dy, r.best, r.still, r.ties)
    return out


def _edges(origin, lo, hi, cell, n):
    """the cells 0 .. n-1 along one axis, [origin + k cell, origin + (k + 1) cell) ∩ [lo, hi): (first cell that is not empty, the
    starts of the cells that are not empty relative to lo, their lengths)"""
    a = np.clip(origin + cell * np.arange(n), lo, hi)
    b = np.clip(origin + cell * (np.arange(n) + 1), lo, hi)
    full = np.nonzero(b > a)[0]
    if full.size == 0:
        return 0, np.zeros(0, np.int64), np.zeros(0, np.int64)
    assert (np.diff(full) == 1).all()
    return int(full[0]), (a[full] - lo).astype(np.int64), (b[full] - a[full]).astype(np.int64)


def maps_fast(kept, cur, window, box, cell, grid, R):
    rows, cols = grid
    wx, wy, ww, wh = window
    x, y, w, h = box
    D = 2 * R + 1
    out = np.zeros((6, rows, cols), np.int64)
    out[5] = D * D
    x0, x1, y0, y1 = max(x, 0), min(x + w, ww), max(y, 0), min(y + h, wh)
    if x1 <= x0 or y1 <= y0:
        return out
    j0, xs, xl = _edges(x, x0, x1, cell, cols)
    i0, ys, yl = _edges(y, y0, y1, cell, rows)
    if xs.size == 0 or ys.size == 0:
        return out
    # the box may reach beyond the grid: only the part the grid's cells cover is summed
    xe, ye = int(xs[-1] + xl[-1]), int(ys[-1] + yl[-1])
    t = kept[wy + y0:wy + y0 + ye, wx + x0:wx + x0 + xe].astype(np.int64)
    sad = np.zeros((D, D, ys.size, xs.size), np.int64)
    for dy in range(-R, R + 1):
        rr = wy + np.clip(np.arange(y0, y0 + ye) + dy, 0, wh - 1)
        for dx in range(-R, R + 1):
            cc = wx + np.clip(np.arange(x0, x0 + xe) + dx, 0, ww - 1)
            d = np.abs(t - cur[rr[:, None], cc[None, :]].astype(np.int64))
            sad[dy + R, dx + R] = np.add.reduceat(np.add.reduceat(d, ys, axis=0), xs, axis=1)
    dyi, dxi = np.meshgrid(np.arange(D), np.arange(D), indexing="ij")
    rank = ((dxi - R) ** 2 + (dyi - R) ** 2) << 12 | dyi << 6 | dxi               # the tie rule as one number, as the kernel's key
    key = (sad << 32 | rank[:, :, None, None]).reshape(D * D, ys.size, xs.size).min(axis=0)
    best = key >> 32
    sub = (slice(i0, i0 + ys.size), slice(j0, j0 + xs.size))
    out[0][sub] = yl[:, None] * xl[None, :]
    out[1][sub] = (key & 63) - R
    out[2][sub] = (key >> 6 & 63) - R
    out[3][sub] = best
    out[4][sub] = sad[R, R]
    out[5][sub] = (sad == best[None, None]).sum(axis=(0, 1))
    return out
