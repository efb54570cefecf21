"""The numpy model of h264bsdmiOutputCellBoxes (test infrastructure): one map [rows, cols] of a cell-map slice, which cells box ∩
window reaches, and the boxes spec -> the boxes slice [1 + M, 8] as the header of include/h264bsd_mi355x.h defines it.  A plain
sequential union–find with the smaller raster index as root; the surviving roots in ascending order are the numbering.  Written from
the definition; it shares nothing with the kernel."""
import numpy as np

ABOVE, BELOW = 0, 1
MAX_CELLS, MAX_BOXES = 16384, 512


def reached(window, box, cell, grid):
    """[rows, cols] bool: box ∩ window reaches cell (i, j) — cells_model's count above 0.  window (left, top, w, h) in the coded frame,
    box (x, y, w, h) relative to the window"""
    rows, cols = grid
    x, y, w, h = box
    bx0, bx1, by0, by1 = max(x, 0), min(x + w, window[2]), max(y, 0), min(y + h, window[3])
    j, i = np.arange(cols), np.arange(rows)
    cx = np.minimum(x + (j + 1) * cell, bx1) > np.maximum(x + j * cell, bx0)
    cy = np.minimum(y + (i + 1) * cell, by1) > np.maximum(y + i * cell, by0)
    return cy[:, None] & cx[None, :] & (bx1 > bx0) & (by1 > by0)


def foreground(values, reach, sense, level):
    v = np.asarray(values).astype(np.int64) & 0xFFFFFFFF
    return reach & ((v < level) if sense == BELOW else (v > level))


def labels(fg, connectivity):
    """[rows, cols] int64: the raster index of the first cell of each foreground cell's component, -1 for background"""
    rows, cols = fg.shape
    parent = np.arange(rows * cols)

    def find(a):
        root = a
        while parent[root] != root:
            root = parent[root]
        while parent[a] != root:
            parent[a], a = root, parent[a]
        return root

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    back = [(0, -1), (-1, 0)] + ([(-1, -1), (-1, 1)] if connectivity == 8 else [])
    for i in range(rows):
        for j in range(cols):
            if not fg[i, j]:
                continue
            for di, dj in back:
                a, b = i + di, j + dj
                if 0 <= a and 0 <= b < cols and fg[a, b]:
                    union(i * cols + j, a * cols + b)
    out = np.full((rows, cols), -1, np.int64)
    for i in range(rows):
        for j in range(cols):
            if fg[i, j]:
                out[i, j] = find(i * cols + j)
    return out


def boxes(values, reach, window, box, cell, max_boxes, sense=ABOVE, level=0, connectivity=8, min_cells=1):
    """the slice [1 + max_boxes, 8] int64 (unsigned words) of one region: values [rows, cols] the chosen map, reach = reached(...)"""
    assert connectivity in (4, 8) and 1 <= max_boxes <= MAX_BOXES and min_cells >= 1 and values.size <= MAX_CELLS
    v = np.asarray(values).astype(np.int64) & 0xFFFFFFFF
    fg = foreground(v, reach, sense, level)
    lab = labels(fg, connectivity)
    roots, counts = np.unique(lab[lab >= 0], return_counts=True)            # ascending: the numbering
    keep = roots[counts >= min_cells]
    out = np.zeros((1 + max_boxes, 8), np.int64)
    out[0, :4] = len(keep), min(len(keep), max_boxes), int(fg.sum()), len(roots) - len(keep)
    x, y, w, h = box
    bx0, bx1, by0, by1 = max(x, 0), min(x + w, window[2]), max(y, 0), min(y + h, window[3])
    for k, root in enumerate(keep[:max_boxes]):
        ii, jj = np.nonzero(lab == root)
        x0, x1 = max(x + int(jj.min()) * cell, bx0), min(x + (int(jj.max()) + 1) * cell, bx1)
        y0, y1 = max(y + int(ii.min()) * cell, by0), min(y + (int(ii.max()) + 1) * cell, by1)
        vals = v[ii, jj]
        total = int(vals.sum())
        out[1 + k] = (x0 & 0xFFFFFFFF, y0 & 0xFFFFFFFF, x1 - x0, y1 - y0, len(ii), int(vals.min() if sense == BELOW else vals.max()),
                      total & 0xFFFFFFFF, total >> 32)
    return out
