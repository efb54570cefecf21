"""The background spread of h264bsdmiBlendCurrentPicturesSpread in numpy (test infrastructure): background_model.Background with a
third frame V, one byte per sample of the I420 coded frame, and the three planes of the cell maps' SPREAD mode on cells_model's geometry.

Per sample, with the current sample c, the kept byte hi and the spread byte V from before the call, d = |c - hi|:
    a luma sample is moving when d > max(hold, V); a chroma sample when one of the four luma samples it covers is (chroma V never gates)
    S = 256 hi + lo is updated as Background.blend updates it under that mask
    A = min(255, gain d);  V' = clamp(V + sign(A - V), lowest, highest);  update "none": no byte of V changes, "all": every sample
    takes V', "still": only the samples that are not moving
V is None while it is not valid (before the first spread blend, after a plain keep) and then reads as `lowest`; where the model starts,
S = T, V = lowest and nothing is moving."""
import numpy as np

import background_model as bm
import cells_model as clm

UPDATES = ("none", "all", "still")
SPREAD = 2                                                      # H264BSDMI_CELLS_SPREAD
PLANES = {"count": 1, "fore": 2, "excess": 4, "spread": 8}      # name -> H264BSDMI_CELL_*, in the order of the maps


def plane_bits(names):
    return sum({PLANES[n] for n in names})


def step(V, d, gain, lowest, highest):
    """V' of int arrays V and d = |c - hi|"""
    V, d = np.asarray(V, np.int64), np.asarray(d, np.int64)
    A = np.minimum(255, gain * d)
    return np.clip(V + np.sign(A - V), lowest, highest)


class Spread(bm.Background):
    """hi, lo and V of one instance.  keep() and blend() are Background's plain calls: a keep invalidates V, a plain blend leaves it;
    blend_spread() is the new call and returns (blended, moving luma samples) as blend() does"""

    def __init__(self, W, H):
        super().__init__(W, H)
        self.V = None

    def keep(self, cur):
        super().keep(cur)
        self.V = None

    def blend_spread(self, cur, shift, hold=255, moving_shift=None, gain=2, lowest=2, highest=255, update="all"):
        assert 1 <= gain <= 8 and 0 <= lowest <= highest <= 255 and update in UPDATES
        assert 0 <= shift <= 7 and 0 <= hold <= 255 and (moving_shift is None or 0 <= moving_shift <= 7 or moving_shift == bm.FROZEN)
        cur = np.asarray(cur, np.uint8)
        assert cur.shape == (self.W * self.H * 3 // 2,)
        if self.hi is None:
            super().keep(cur)                               # the model starts: S = T, V = lowest, nothing is moving
            self.V = np.full(cur.shape, lowest, np.uint8)
            return 0, 0
        if moving_shift is None:
            moving_shift = shift
        V = np.full(cur.shape, lowest, np.int64) if self.V is None else self.V.astype(np.int64)
        n = self.W * self.H
        d = np.abs(cur.astype(np.int64) - self.hi.astype(np.int64))
        luma = (d[:n] > np.maximum(hold, V[:n])).reshape(self.H, self.W)
        chroma = luma.reshape(self.H // 2, 2, self.W // 2, 2).any(axis=(1, 3)).reshape(-1)
        moving = np.concatenate([luma.reshape(-1), chroma, chroma])
        S = self.state()
        k = np.where(moving, 0 if moving_shift == bm.FROZEN else moving_shift, shift)
        S2 = bm.update(S, bm.target(cur), k)
        if moving_shift == bm.FROZEN:
            S2 = np.where(moving, S, S2)
        assert S2.min() >= bm.S_MIN and S2.max() <= bm.S_MAX
        self.hi, self.lo = (S2 >> 8).astype(np.uint8), (S2 & 255).astype(np.uint8)
        if update != "none":
            V2 = step(V, d, gain, lowest, highest)
            V = np.where(moving, V, V2) if update == "still" else V2
        self.V = V.astype(np.uint8)
        self.last_moving = moving
        return 1, int(luma.sum())


def maps(bits, cur, kept, spread, window, box, cell, grid, threshold=(0, 0, 0)):
    """the slice [P, rows, cols] int64 of SPREAD mode.  cur, kept, spread: [C, H, W] planes (stats_model.channels of the three I420
    frames); window, box, grid as cells_model.maps"""
    C = cur.shape[0]
    a, valid = clm._grid_cut(cur, window, box, cell, grid)
    b, _ = clm._grid_cut(kept, window, box, cell, grid)
    v, _ = clm._grid_cut(spread, window, box, cell, grid)
    vm = valid[None]
    d = np.where(vm, np.abs(a - b), 0)
    t = np.maximum(np.asarray(list(threshold)[:C], np.int64)[:, None, None], v)
    out = []
    if bits & 1:
        out.append(clm._cells(valid.astype(np.int64), cell, grid).sum((-3, -1))[None])
    if bits & 2:
        out.append(clm._cells((vm & (d > t)).astype(np.int64), cell, grid).sum((-3, -1)))
    if bits & 4:
        out.append(clm._cells(np.where(vm, np.maximum(0, d - t), 0), cell, grid).sum((-3, -1)))
    if bits & 8:
        out.append(clm._cells(np.where(vm, v, 0), cell, grid).sum((-3, -1)))
    res = np.concatenate(out, 0)
    assert res.shape == (clm.n_maps(SPREAD, C, bits),) + tuple(grid)
    return res


def maps_by_samples(bits, cur, kept, spread, window, box, cell, grid, threshold=(0, 0, 0)):
    """the same slice by a direct loop over the samples of every cell's box"""
    C, H, W = cur.shape
    wx, wy, ww, wh = window
    rows, cols = grid
    res = np.zeros((clm.n_maps(SPREAD, C, bits), rows, cols), np.int64)
    for i in range(rows):
        for j in range(cols):
            x, y, w, h = clm.cell_box(box, cell, i, j)
            count, fore, excess, busy = 0, [0] * C, [0] * C, [0] * C
            for yy in range(y, y + max(h, 0)):
                for xx in range(x, x + max(w, 0)):
                    if not (0 <= xx < ww and 0 <= yy < wh):
                        continue
                    count += 1
                    for c in range(C):
                        V = int(spread[c, wy + yy, wx + xx])
                        t = max(int(threshold[c]), V)
                        d = abs(int(cur[c, wy + yy, wx + xx]) - int(kept[c, wy + yy, wx + xx]))
                        fore[c] += d > t
                        excess[c] += max(0, d - t)
                        busy[c] += V
            at = 0
            if bits & 1:
                res[at, i, j] = count
                at += 1
            for bit, val in ((2, fore), (4, excess), (8, busy)):
                if bits & bit:
                    res[at:at + C, i, j] = val
                    at += C
    return res
