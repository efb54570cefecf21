"""No GPU: what tests/test_gpu_saturated_motion.py is FOR, held on the CPU.  k_cell_shift and k_region_shift keep their SADs in packed
16-bit sums that may take SHIFT_FOLD = 64 v_qsad_pk_u16_u8 of at most 1020 each; how many they really take is decided by the item walks
of the two kernels, restated here in plain Python from their headers (the constants are read from the headers, so a change there is
seen).  The restatement reproduces the tables of docs/PARITY.md ("Chosen content: the shift, flow and corner pulls"), and the cases of
the GPU file are held to their reach: a packed sum that takes exactly SHIFT_FOLD instructions of saturated content, unpackings inside
the row loop, the one-line mutant `pending > SHIFT_FOLD` wrapping on the chosen pairs and not on noise, segments of 32 dwords in
k_region_shift and none longer, corner energies above 2^32 per band and whole, perfect-square radicands of 2^49 and more, box sums at 0
and 6375.  No family of cases can be dropped from the GPU file without a test here failing."""
import math
import os
import re

import numpy as np
import pytest

import corners_model as cm
import flow_model as fm
import matches_model as mm
import test_gpu_saturated_motion as sat
from conftest import ROOT
from test_gpu_region_shift import SHIFT as NOISE_SHIFT
from test_gpu_region_shift import _shifted

KERNELS = os.path.join(ROOT, "h264bsd_amd", "csrc", "kernels")


def _constants(header, names):
    text = open(os.path.join(KERNELS, header)).read()
    return {n: int(re.search(r"\b" + n + r" = (\d+)\b", text).group(1)) for n in names}


K = _constants("k_region_shift.hip.h", ["SHIFT_QUADS", "SHIFT_QUADS_FROM", "SHIFT_MAX_RADIUS", "SHIFT_ROWS", "SHIFT_COLS4", "SHIFT_FOLD", "SHIFT_SPLIT"])
K.update(_constants("k_cell_shift.hip.h", ["FLOW_RECT_W", "FLOW_RECT_H", "FLOW_MIN_SHIFT", "FLOW_MAX_SHIFT", "FLOW_SURF_WORDS", "FLOW_SPLIT"]))
K.update(_constants("k_region_stats.hip.h", ["STATS_MAX_PARTIALS"]))
FOLD = K["SHIFT_FOLD"]
RADII = range(K["SHIFT_MAX_RADIUS"] + 1)


def test_the_constants_are_the_ones_the_tables_were_made_with():
    assert K == dict(SHIFT_QUADS=3, SHIFT_QUADS_FROM=4, SHIFT_MAX_RADIUS=16, SHIFT_ROWS=32, SHIFT_COLS4=64, SHIFT_FOLD=64, SHIFT_SPLIT=1024,
                     FLOW_RECT_W=64, FLOW_RECT_H=64, FLOW_MIN_SHIFT=3, FLOW_MAX_SHIFT=6, FLOW_SURF_WORDS=4096, FLOW_SPLIT=512,
                     STATS_MAX_PARTIALS=1024)
    assert FOLD * 1020 == 65280 <= 65535 < (FOLD + 1) * 1020


def pairs_of(R):
    """(QUADS, Q3, P): the quads a thread takes, the threads per row of the surface, the (row, thread) pairs of a surface"""
    D = 2 * R + 1
    quads = K["SHIFT_QUADS"] if R >= K["SHIFT_QUADS_FROM"] else 1
    q3 = ((D + 3) // 4 + quads - 1) // quads
    return quads, q3, D * q3


# ---- k_cell_shift: the item walk ----
def kernel_rule(pending, width):
    return pending + width > FOLD


def mutant_rule(pending, width):
    return pending > FOLD


def flow_shares(window, box, cell, grid, R):
    """every (cell, share) the kernel walks for one region: dict(G, rows: the template rows of the share in the coded frame, width:
    u1 - u0, the dwords of a row, x: the samples [xa, xb) of the row's FULL dwords, the ones that go through v_qsad_pk_u16_u8).
    The walk is the same for every (dy, quads) pair of the surface"""
    wx, wy, ww, wh = window
    rows, cols = grid
    ox, oy = wx + box[0], wy + box[1]
    x0, x1, y0, y1 = max(ox, wx), min(ox + box[2], wx + ww), max(oy, wy), min(oy + box[3], wy + wh)
    D = 2 * R + 1
    n, (_, _, P) = D * D, pairs_of(R)
    RW, RH = K["FLOW_RECT_W"] // cell, K["FLOW_RECT_H"] // cell
    out = []
    if x1 <= x0 or y1 <= y0:
        return out
    for i0 in range(0, rows, RH):
        for j0 in range(0, cols, RW):
            nj, ni = min(RW, cols - j0), min(RH, rows - i0)
            rectx, recty = ox + j0 * cell, oy + i0 * cell
            rx0, rx1, ry0, ry1 = max(x0, rectx), min(x1, rectx + nj * cell), max(y0, recty), min(y1, recty + ni * cell)
            if rx1 <= rx0 or ry1 <= ry0:
                continue
            SX, SY = rectx + ((rx0 - rectx) >> 2 << 2), ry0
            gc = min(ni * nj, K["FLOW_SURF_WORDS"] // n)
            G = min(max((K["FLOW_SPLIT"] + gc * P - 1) // (gc * P), 1), cell)
            for c in range(ni * nj):
                ci, cj = divmod(c, nj)
                cellx, celly = rectx + cj * cell, recty + ci * cell
                cx0, cx1, cy0, cy1 = max(rx0, cellx), min(rx1, cellx + cell), max(ry0, celly), min(ry1, celly + cell)
                if cx1 <= cx0 or cy1 <= cy0:
                    continue
                ba, bb = cx0 - SX, cx1 - SX
                u0, u1 = ba >> 2, (bb + 3) >> 2
                assert (cellx - SX) % 4 == 0 and u1 - u0 <= cell // 4          # a cell starts on a dword of the staged template
                fa = u0 + (1 if ba & 3 else 0)                                  # the full dwords [fa, fb): the first and the last may be masked
                fb = max(fa, u1 - (1 if bb & 3 else 0))
                for g in range(G):
                    out.append(dict(G=G, gc=gc, rows=list(range(cy0 + g, cy1, G)), width=u1 - u0, x=(SX + 4 * fa, SX + 4 * fb)))
    return out


def fold_walk(share, rule):
    """the row loop of one item under `rule`: (the rows of every packed sum's lifetime, unpackings inside the loop, of those behind
    which more rows follow).  The last lifetime ends at the item's closing fold and may be empty"""
    lives, pending, live, inside, mid = [], 0, [], 0, 0
    for k, y in enumerate(share["rows"]):
        live.append(y)
        pending += share["width"]
        if rule(pending, share["width"]):
            lives.append(live)
            live, pending, inside = [], 0, inside + 1
            mid += k + 1 < len(share["rows"])
    lives.append(live)
    return lives, inside, mid


def instructions(share, live):
    return len(live) * (share["x"][1] - share["x"][0]) // 4


def flow_reach(window, box, cell, grid, R, rule=kernel_rule):
    """(the most instructions a packed sum takes, unpackings inside the loop per pair of the surface, of those in mid-item, G)"""
    shares = flow_shares(window, box, cell, grid, R)
    walks = [(s, fold_walk(s, rule)) for s in shares]
    most = max(instructions(s, live) for s, (lives, _, _) in walks for live in lives)
    return most, sum(w[1] for _, w in walks), sum(w[2] for _, w in walks), max(s["G"] for s in shares)


FULL = ((0, 0, 4096, 4096), (64, 64, 64, 64))             # one full rectangle well inside a window


def test_the_fold_table_of_a_full_rectangle():
    """docs/PARITY.md: the fold only runs for cells of 32 from radius 8 and of 64 from radius 6 on, and then a packed sum takes exactly
    SHIFT_FOLD instructions; the third figure of an entry is the unpackings inside the row loop per cell and pair of the surface"""
    table = {}
    for cell in fm.CELLS:
        for R in RADII:
            grid = (64 // cell, 64 // cell)
            most, inside, mid, G = flow_reach(FULL[0], FULL[1], cell, grid, R)
            assert most <= FOLD
            table[cell, R] = (G, most, inside // (grid[0] * grid[1]))
    quiet = [(cell, R) for cell in fm.CELLS for R in RADII if cell < 32 or R < 6]
    assert all(table[k][1] <= 32 and table[k][2] == 0 for k in quiet), {k: table[k] for k in quiet if table[k][1] > 32 or table[k][2]}
    # between the radii the public tests run: cells of 32 come close at radius 6 and 7, cells of 64 already fold there
    assert {(c, R): table[c, R] for c in (32, 64) for R in (6, 7)} == {(32, 6): (5, 56, 0), (32, 7): (5, 56, 0), (64, 6): (20, 64, 4), (64, 7): (18, 64, 10)}
    for R in range(8, 17):
        assert table[32, R][1] == table[64, R][1] == FOLD and table[32, R][2] > 0 and table[64, R][2] > 0
    assert {(c, R): table[c, R] for c in (32, 64) for R in (8, 12, 16)} == {
        (32, 8): (4, 64, 4), (32, 12): (2, 64, 4), (32, 16): (2, 64, 4), (64, 8): (16, 64, 16), (64, 12): (7, 64, 14), (64, 16): (6, 64, 12)}
    # the mutant: 72 and 80 instructions, from radius 12 on (at radius 8 a share has too few rows to get there)
    mutant = {(c, R): flow_reach(FULL[0], FULL[1], c, (64 // c, 64 // c), R, mutant_rule)[0] for c in (32, 64) for R in (8, 12, 16)}
    assert mutant == {(32, 8): 64, (32, 12): 72, (32, 16): 72, (64, 8): 64, (64, 12): 80, (64, 16): 80}
    assert 72 * 1020 == 73440 > 65535 and 80 * 1020 == 81600 and 72 * 4 * 85 < 65535 and 80 * 4 * 225 > 65535


def _rowsums(kept, cur, window, R):
    """[D D, H, W + 1] prefix sums along x of |kept - cur(+dx, +dy)|, the current picture clamped at the window: frame coordinates"""
    wx, wy, ww, wh = window
    H, W = kept.shape
    out = np.zeros(((2 * R + 1) ** 2, H, W + 1), np.int64)
    ys, xs = np.arange(H), np.arange(W)
    k = 0
    for dy in range(-R, R + 1):
        rr = np.clip(ys + dy, wy, wy + wh - 1)
        for dx in range(-R, R + 1):
            cc = np.clip(xs + dx, wx, wx + ww - 1)
            out[k, :, 1:] = np.abs(kept.astype(np.int64) - cur[rr[:, None], cc[None, :]]).cumsum(axis=1)
            k += 1
    return out


def largest_packed_sum(kept, cur, window, box, cell, grid, R, rule):
    """the largest value any packed 16-bit sum of a displacement inside the surface would have to hold before it is unpacked"""
    pre = _rowsums(kept, cur, window, R)
    most = 0
    for s in flow_shares(window, box, cell, grid, R):
        xa, xb = s["x"]
        if xb <= xa:
            continue
        per_row = pre[:, :, xb] - pre[:, :, xa]
        for live in fold_walk(s, rule)[0]:
            if live:
                most = max(most, int(per_row[:, live].sum(axis=1).max()))
    return most


def _flow_calls():
    """(pair, cell, radius, window, boxes, grid) of every call of the GPU file"""
    window = (0, 0, sat.FW, sat.FH)
    boxes = [b or window for b in sat.FLOW_BOXES]
    return [(p, c, r, window, boxes, fm.default_grid([(b[3], b[2]) for b in boxes], c)) for p, c, r in sat.FLOW_CASES]


def test_the_flow_set_is_the_one_asked_for():
    assert set(sat.PAIRS) == {"sat", "sat-reversed", "dark-bright"}
    assert {(p, c, r) for p in sat.PAIRS for c in (32, 64) for r in (8, 12, 16)} <= set(sat.FLOW_CASES)
    assert {("sat", c, r) for c in fm.CELLS for r in (0, 3, 4)} <= set(sat.FLOW_CASES)
    assert None in sat.FLOW_BOXES and (-21, -13, 150, 120) in sat.FLOW_BOXES and (3, 5, 69, 70) in sat.FLOW_BOXES
    assert (sat.FW, sat.FH) == (80, 80)
    assert {pairs_of(r)[0] for _, _, r in sat.FLOW_CASES} == {1, 3}                 # both instantiations
    for name in sat.PAIRS:
        kept, cur = sat.pair(name, sat.FW, sat.FH)
        d = np.abs(kept.astype(int) - cur.astype(int))
        assert (d.min(), d.max()) == ((255, 255) if name.startswith("sat") else (225, 255))
    kept, cur = sat.pair("dark-bright", sat.FW, sat.FH)
    assert len(np.unique(kept)) == 16 and len(np.unique(cur)) == 16


def test_the_flow_cases_reach_the_fold():
    """on the pictures and boxes of the GPU file, per (cell, radius) of the deep set: some packed sum takes exactly SHIFT_FOLD
    instructions on full dwords (65280 on `sat`), none takes more, and the unpacking runs inside the row loop — at radius 12 and 16
    with rows still to come.  The boxes at odd origins bring masked first and last dwords beside full ones in one row"""
    seen = {}
    for p, c, r, window, boxes, grid in _flow_calls():
        if (c, r) in seen:
            continue
        reach = [flow_reach(window, b, c, grid, r) for b in boxes]
        seen[c, r] = (max(x[0] for x in reach), sum(x[1] for x in reach), sum(x[2] for x in reach))
        for b in boxes[1:]:
            shares = flow_shares(window, b, c, grid, r)
            assert any(0 < s["x"][1] - s["x"][0] < 4 * s["width"] for s in shares), (c, r, b)      # masked and full dwords in one row
    for c, r in ((c, r) for c in (32, 64) for r in (8, 12, 16)):
        most, inside, mid = seen[c, r]
        assert most == FOLD and inside > 0 and (mid > 0) == (r >= 12), (c, r, seen[c, r])
    for (c, r), (most, inside, mid) in seen.items():
        assert most <= FOLD
        if c < 32 or r < 8:
            assert inside == 0 and most <= 32, (c, r)
    kept, cur = sat.pair("sat", sat.FW, sat.FH)
    window = (0, 0, sat.FW, sat.FH)
    assert largest_packed_sum(kept, cur, window, window, 64, (2, 2), 8, kernel_rule) == 65280


@pytest.mark.parametrize("cell,radius", [(32, 12), (32, 16), (64, 12), (64, 16)])
def test_the_altered_rule_wraps_on_the_chosen_pairs_and_not_on_noise(cell, radius):
    """`pending > SHIFT_FOLD` in place of `pending + (u1 - u0) > SHIFT_FOLD`: 72 or 80 instructions into one packed sum.  Every chosen
    pair then needs more than 16 bits; the noise pair of tests/test_gpu_cell_shift.py, which runs the same cells at radius 16, does not"""
    window = (0, 0, sat.FW, sat.FH)
    grid = fm.default_grid([(sat.FH, sat.FW)], cell)
    for name in sat.PAIRS:
        kept, cur = sat.pair(name, sat.FW, sat.FH)
        assert largest_packed_sum(kept, cur, window, window, cell, grid, radius, kernel_rule) <= 65535, name
        assert largest_packed_sum(kept, cur, window, window, cell, grid, radius, mutant_rule) > 65535, name
    W, H = 64, 48
    noise = np.random.default_rng(5).integers(0, 256, (H, W), dtype=np.uint8)
    grid = fm.default_grid([(H, W)], cell)
    worst = largest_packed_sum(noise, _shifted(noise, *NOISE_SHIFT), (0, 0, W, H), (0, 0, W, H), cell, grid, 16, mutant_rule)
    assert 0 < worst < 40000, worst


# ---- k_region_shift: the segments ----
def band_count(n_regs, tallest):
    return 1 if n_regs >= K["STATS_MAX_PARTIALS"] else min(K["STATS_MAX_PARTIALS"] // n_regs, max(tallest, 1))


def shift_tiles(box, S):
    """the (th, tw) of every tile of template a box inside the window is walked in, by S row bands"""
    x, y, w, h = box
    x0, x1, y0, y1 = x, x + w, y, y + h
    mby0, rows = y0 >> 4, ((y1 + 15) >> 4) - (y0 >> 4)
    out = []
    for band in range(S):
        r0, r1 = mby0 + rows * band // S, mby0 + rows * (band + 1) // S
        ya, yb = max(y0, 16 * r0), min(y1, 16 * r1)
        for ys in range(ya, yb, K["SHIFT_ROWS"]):
            for xs in range(x0, x1, 4 * K["SHIFT_COLS4"]):
                out.append((min(K["SHIFT_ROWS"], yb - ys), min(4 * K["SHIFT_COLS4"], x1 - xs)))
    return out


def segment_length(th, tw4, R):
    G = (K["SHIFT_SPLIT"] + pairs_of(R)[2] - 1) // pairs_of(R)[2]
    L = 1
    while L < K["SHIFT_COLS4"] and 2 * L * 4 * G <= th * tw4:
        L *= 2
    return L, G


def longest_packed_segment(th, tw, R):
    """the most v_qsad_pk_u16_u8 a packed sum takes in a tile: the dwords of its longest segment, the masked last one of a row left out"""
    tw4 = (tw + 3) >> 2
    L, _ = segment_length(th, tw4, R)
    full = tw4 - (1 if tw & 3 else 0)
    return max(min(u0 + L, full) - u0 for u0 in range(0, tw4, L) if u0 < full) if full else 0


def test_the_segment_table_and_the_rule_that_keeps_it():
    """docs/PARITY.md: the longest segment of a 32 x 256 tile per radius; no tile at any radius gives a longer one than 32 dwords, half
    of what SHIFT_FOLD allows — the rule is `2 L * 4 G <= th * tw4` with G = ceil(SHIFT_SPLIT / P)"""
    table = [segment_length(32, 64, R)[0] for R in RADII]
    assert table == [1, 1] + [4] * 4 + [8] * 2 + [16] * 4 + [32] * 5
    assert segment_length(32, 64, 1) == (1, 342)                               # what the saturated largest frame of the sibling file runs
    for R in RADII:
        for th in range(1, K["SHIFT_ROWS"] + 1):
            for tw4 in (1, 2, 3, 7, 8, 16, 31, 32, 33, 48, 63, 64):
                assert segment_length(th, tw4, R)[0] <= 32 <= FOLD // 2
    assert 32 * 1020 == 32640


def _shift_calls():
    """(n_regs, boxes) of the two calls the GPU file makes per (pair, radius, surface)"""
    return [sat.SHIFT_BOXES, sat.SHIFT_BOXES + [sat.SHIFT_PAD[0]] * sat.SHIFT_PAD[1]]


def test_the_shift_cases_walk_segments_of_32_dwords():
    assert set(sat.SHIFT_PAIRS) == {"sat", "dark-bright"} and set(sat.SHIFT_RADII) == {1, 4, 8, 12, 16} and (sat.SW, sat.SH) == (288, 48)
    assert set(sat.SHIFT_BOXES) == {(0, 0, 288, 48), (0, 0, 256, 32), (16, 16, 256, 16), (3, 5, 253, 40)}
    assert {pairs_of(r)[0] for r in sat.SHIFT_RADII} == {1, 3}
    banded, single = _shift_calls()
    tallest = max(((b[1] + b[3] + 15) >> 4) - (b[1] >> 4) for b in banded)
    assert (band_count(len(banded), tallest), band_count(len(single), tallest)) == (3, 1)
    # with a band per macroblock row a tile has 16 rows: half the template, segments of 16 dwords at the most
    assert max(th for b in banded for th, _ in shift_tiles(b, 3)) == 16
    assert max(longest_packed_segment(th, tw, R) for b in banded for th, tw in shift_tiles(b, 3) for R in sat.SHIFT_RADII) == 16
    # one band per region: the 32 x 256 tile, and at radius 12 and 16 segments of 32 full dwords
    assert (32, 256) in shift_tiles((0, 0, 256, 32), 1) and (32, 256) in shift_tiles((0, 0, 288, 48), 1)
    longest = {R: max(longest_packed_segment(th, tw, R) for b in single for th, tw in shift_tiles(b, 1)) for R in sat.SHIFT_RADII}
    assert longest == {1: 1, 4: 4, 8: 16, 12: 32, 16: 32}
    # the box at (3, 5), 253 wide: a masked last dword (253 = 4 * 63 + 1) at the end of a row of full ones
    assert any(tw & 3 for th, tw in shift_tiles((3, 5, 253, 40), 1))
    # a single band by geometry, and bands that meet in the scratch with sums of 255 x 16 x 288 each
    assert len({th for th, _ in shift_tiles((16, 16, 256, 16), 3)}) == 1


# ---- k_corner_points: the energy and the square root ----
def _energy(win, box):
    return cm.Window(win).points(box, 3)[1]


def test_the_corner_pictures_reach_what_the_random_ones_do_not():
    assert set(sat.CORNER_PICTURES) == {"columns", "dots", "wide-columns", "quadrant"} and set(sat.COLUMN_PICTURES) == {"columns", "wide-columns"}
    assert {(s, b, n) for s in (cm.MIN_EIGEN, cm.HARRIS) for b in (3, 5) for n in (1, 3)} <= set(sat.CORNER_PARAMS)
    assert (0, 0, 288, 48) in sat.CORNER_BOXES and (0, 16, 288, 16) in sat.CORNER_BOXES
    assert band_count(len(sat.CORNER_BOXES), 3) == 3 and band_count(2 + sat.CORNER_PAD[1], 3) == 1
    # the pictures the existing device tests run: all below 2^32
    noise = lambda seed, w, h: np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    x, y = np.meshgrid(np.arange(64), np.arange(48))
    board = ((((x // 8) + (y // 8)) & 1) * 255).astype(np.uint8)
    existing = (_energy(noise(11, 144, 80), (0, 0, 144, 80)), _energy(noise(5, 64, 48), (0, 0, 64, 48)), _energy(board, (0, 0, 64, 48)))
    assert existing == (1531708032, 404770244, 1146520800) and max(existing) < 2 ** 32
    # two-sample columns: above 2^32 in the whole window and in one band of 16 rows
    wide = sat.corner_picture("wide-columns")
    assert _energy(wide, (0, 0, 288, 48)) == 14282611200 > 3 * 2 ** 32 and _energy(wide, (0, 16, 288, 16)) == 4760870400 > 2 ** 32
    assert all(_energy(sat.corner_picture(n), (0, 0, 288, 48)) < 2 ** 32 for n in sat.CORNER_PICTURES if n != "wide-columns")
    # the extremes of the model's own test, at this size: A at its largest, the most negative Harris score, a radicand that is a
    # perfect square of 2^49 and more, whose root must come out exactly
    A, B, C = cm.tensor(wide, 5)
    assert A.max() == 25 * 1020 * 1020 and not B.any() and not C.any()
    assert cm.scores(wide, cm.HARRIS, 5).min() == -(25 * 1020 * 1020) ** 2
    radicand = (A - B) * (A - B) + 4 * C * C
    assert int(radicand.max()) == (25 * 1020 * 1020) ** 2 >= 2 ** 49 and math.isqrt(int(radicand.max())) ** 2 == int(radicand.max())
    for name in sat.COLUMN_PICTURES:
        for block in (3, 5):
            A, B, C = cm.tensor(sat.corner_picture(name), block)
            assert A.max() > 0 and not B.any() and not C.any()                 # the radicand is A A: a root one too small scores 1 everywhere
            assert not cm.scores(sat.corner_picture(name), cm.MIN_EIGEN, block).any()
            assert cm.scores(sat.corner_picture(name), cm.HARRIS, block).max() <= 0
            for score in (cm.MIN_EIGEN, cm.HARRIS):
                assert cm.Window(sat.corner_picture(name), score, block).points((0, 0, 288, 48), 1)[2] == []
    # the pictures that do have points: their largest MIN_EIGEN score, far below the 2^26 of the kernel's header
    best = {n: max(int(cm.scores(sat.corner_picture(n), cm.MIN_EIGEN, b).max()) for b in (3, 5)) for n in ("dots", "quadrant")}
    assert best == {"dots": 5202000, "quadrant": 13005000} and max(best.values()) < 2 ** 26
    for n in ("dots", "quadrant"):
        assert len(cm.Window(sat.corner_picture(n), cm.HARRIS, 5).points((0, 0, 288, 48), 1)[2]) > 0


# ---- k_point_describe: the box sums ----
def test_the_match_points_compare_box_sums_at_their_ends():
    kept = sat.match_picture()
    assert kept.shape == (80, 80) and set(np.unique(kept)) == {0, 255} and len(sat.MATCH_POINTS) == sat.MATCH_K == len(set(sat.MATCH_POINTS))
    assert all(0 <= x < 80 and 0 <= y < 80 for x, y in sat.MATCH_POINTS)
    bp, bq = sat.match_sums(kept, sat.MATCH_POINTS)
    assert min(bp.min(), bq.min()) == 0 and max(bp.max(), bq.max()) == 6375 == 25 * 255
    counts = (int(((bp == 0) | (bq == 0)).sum()), int(((bp == 6375) | (bq == 6375)).sum()), int((bp == bq).sum()))
    assert min(counts) >= 256, counts
    # the quick form of the model, which the GPU file compares with, is the definition on these pictures
    kp = mm.points_record(sat.MATCH_POINTS, sat.MATCH_K)
    args = (kept, 255 - kept, (0, 0, 80, 80), (0, 0, 80, 80), kp, kp, sat.MATCH_K)
    assert mm.record(*args, max_distance=256, ratio=256, mutual_only=0) == mm.record_fast(*args, max_distance=256, ratio=256, mutual_only=0)
