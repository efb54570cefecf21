"""GPU parity of the one-vector inter kernel (k_recon_inter_lb: a 4x4 block per lane, four macroblocks per wavefront, chunks binned by
interpolation class) on hand-built jobs whose one-vector LIST is laid out on purpose: kernels vs CPU oracle, byte for byte.
Every picture is two intra pictures (slots 0 and 1: noise, so every tap of every filter matters) and one P picture in which chosen
macroblocks carry one motion vector each and all the others are zero-motion copies (they go to k_copy, not to the list).  What the
list then holds is the test: its length (group remainder, chunk remainder, more than one chunk), the bins of its entries (one class
alone, all ten in turn), where the reference windows lie, which coefficient blocks there are and in which arithmetic."""
import struct

import numpy as np
import pytest

from jobgen import build_job, z_of
from replay_compare import run_and_compare

pytestmark = pytest.mark.gpu

QPC = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 29,
       30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39]
FJ_CODED_WIDE = 1 << 27
CLASSES = ["whole", "hor", "ver", "diag", "centre"]
CLASS_FRACTIONS = {                                            # (fx, fy) of the luma quarter-sample position
    "whole": [(0, 0)],
    "hor": [(1, 0), (2, 0), (3, 0)],
    "ver": [(0, 1), (0, 2), (0, 3)],
    "diag": [(1, 1), (3, 1), (1, 3), (3, 3)],
    "centre": [(2, 2), (2, 1), (2, 3), (1, 2), (3, 2)],
}
RESIDUALS = ["none", "luma", "cdc", "cac", "all", "wide_sat"]


def class_of(mv):
    fx, fy = mv[0] & 3, mv[1] & 3
    return "whole" if (fx | fy) == 0 else "hor" if fy == 0 else "ver" if fx == 0 else "diag" if fx != 2 and fy != 2 else "centre"


def _levels(rng, ac_only=False):
    """a block of one to three levels of magnitude <= 3: with the quantisers below the parser's 16-bit bound holds by a wide margin"""
    c = np.zeros(16, dtype=np.int16)
    for _ in range(int(rng.integers(1, 4))):
        c[int(rng.integers(1 if ac_only else 0, 16))] = rng.choice([-3, -2, -1, 1, 2, 3])
    return c


def _residual(rng, kind):
    """(coded bits, coefficient blocks in the order of framejob.h, qp_y or None) of one macroblock"""
    blocks, coded, qp = [], 0, None
    if kind == "none":
        return 0, [], None
    if kind == "wide_sat":
        # qp 51: one DC level of +-9 per luma block is a residual of +-504 for every sample of it (inside [-512, 511], far outside what
        # a sample can absorb: the sum clips to 0 or 255), and 9 x (23 << 8) breaks the 16-bit bound: FJ_CODED_WIDE.  Chroma: the DC
        # levels (64, 0, 0, 0) at QPc 39 give +-448 in all four blocks of a plane
        for z in range(16):
            if z % 3 != 1:
                c = np.zeros(16, dtype=np.int16); c[0] = 9 if z % 2 else -9
                blocks.append(c); coded |= 1 << z
        cdc = np.zeros(16, dtype=np.int16); cdc[0], cdc[4] = 64, -64
        blocks.append(cdc); coded |= 1 << 25
        return coded, blocks, 51
    luma = {"luma": sorted(rng.choice(16, int(rng.integers(1, 6)), replace=False)), "all": range(16)}.get(kind, [])
    for z in luma:
        blocks.append(_levels(rng)); coded |= 1 << int(z)
    if kind in ("cdc", "cac", "all"):
        cdc = np.zeros(16, dtype=np.int16); cdc[:8] = rng.integers(-6, 7, 8)
        blocks.append(cdc); coded |= 1 << 25
    ac = {"cac": sorted(rng.choice(8, int(rng.integers(1, 5)), replace=False)), "all": range(8)}.get(kind, [])
    for k in ac:
        blocks.append(_levels(rng, ac_only=True)); coded |= 1 << (16 + int(k))
    return coded, blocks, int(rng.integers(10, 31))


def _buffer_of(view):
    while view.base is not None:
        view = view.base
    return view


_intra = {}


def _intra_pictures(lib, wmb, hmb):
    if (wmb, hmb) not in _intra:
        rng = np.random.default_rng(1000 * wmb + hmb)
        _intra[(wmb, hmb)] = [build_job(lib, rng, wmb, hmb, 0, 3, []), build_job(lib, rng, wmb, hmb, 1, 3, [])]
    return _intra[(wmb, hmb)]


def p_picture(lib, seed, wmb, hmb, entries):
    """entries: [(macroblock address, (mvx, mvy) in quarter samples, reference slot, residual kind)] in ascending address order — the
    one-vector list of the picture; every other macroblock copies slot 0 in place"""
    rng = np.random.default_rng(seed)
    n = wmb * hmb
    by_mb = {a: (mv, slot, kind) for a, mv, slot, kind in entries}
    assert len(by_mb) == len(entries)

    def patch(recs, mvs, first_extra):
        coefs = _buffer_of(recs)[128 + n * 32 + n * 64:].view(np.int16)
        nb = first_extra
        for a in range(n):
            r = recs[a]
            r[0], r[4] = 0, 1 << 4                                  # inter, one 16x16 partition
            r[8:12] = 0
            if a not in by_mb:
                mvs[a] = (0, 0); r[16:20] = 0
                continue
            mv, slot, kind = by_mb[a]
            mvs[a] = mv; r[16:20] = slot
            coded, blocks, qp = _residual(rng, kind)
            if qp is not None:
                r[1], r[2] = qp, QPC[qp]
            struct.pack_into("<I", r, 8, coded)
            struct.pack_into("<I", r, 12, nb)
            for blk in blocks:
                coefs[16 * nb:16 * nb + 16] = blk; nb += 1

    job = build_job(lib, rng, wmb, hmb, 2, 3, [0, 1], p_inter=1.0, patch=patch, extra_blocks=25 * len(entries) + 1)
    # the finished job must hold the list this test is about
    n_gen, n_uni = struct.unpack_from("<I", job, 72)[0], struct.unpack_from("<I", job, 84)[0]
    assert n_gen == n_uni == len(entries), (n_gen, n_uni, len(entries))
    return job


def run(built, seed, wmb, hmb, entries, stages=3, n_streams=2):
    lib = built.lib()
    job = p_picture(lib, seed, wmb, hmb, entries)
    run_and_compare(built, _intra_pictures(lib, wmb, hmb) + [job], n_streams=n_streams, stages=stages)
    return job


def gen_entries(job):
    off, n = struct.unpack_from("<I", job, 68)[0], struct.unpack_from("<I", job, 72)[0]
    return [struct.unpack_from("<HBBhhII", job, off + 16 * i) for i in range(n)]      # mb, uniform, slot, mvx, mvy, coef word, coded


def vector(rng, cls, i, reach=24):
    """a vector of the class, its whole part within +-reach samples, the fraction the i-th of the class"""
    fx, fy = CLASS_FRACTIONS[cls][i % len(CLASS_FRACTIONS[cls])]
    if cls == "whole" and i % 2 == 0:
        # whole luma samples: one component at half a chroma sample, or the macroblock would be a copy when it has no coefficients
        wx, wy = int(rng.integers(-reach, reach + 1)), int(rng.integers(-reach, reach + 1))
        return (4 * (2 * (wx // 2) + 1), 4 * wy) if i % 4 else (4 * wx, 4 * (2 * (wy // 2) + 1))
    if cls == "whole":
        return 4 * (2 * int(rng.integers(-reach // 2, reach // 2)) + 1), 4 * (2 * int(rng.integers(-reach // 2, reach // 2)) + 1)
    return 4 * int(rng.integers(-reach, reach + 1)) + fx, 4 * int(rng.integers(-reach, reach + 1)) + fy


def addresses(rng, n, length):
    return sorted(int(a) for a in rng.choice(n, length, replace=False))


# ---- list lengths: the group remainder (1, 3, 4, 5), the chunk remainder and more than one chunk (17, 63, 64, 65) ----
@pytest.mark.parametrize("wmb,hmb,length", [(1, 1, 1), (2, 2, 1), (2, 2, 3), (2, 2, 4), (3, 2, 5), (5, 4, 17), (11, 6, 63), (11, 6, 64), (11, 6, 65)])
def test_list_lengths_with_every_bin_in_turn(built, wmb, hmb, length):
    """entry i is of class i mod 5, uncoded and coded in turns of five (the coded ones with each residual kind in turn): all ten bins
    within the first ten entries, so every group of four is mixed, WIDE macroblocks share groups with packed ones, both reference
    slots occur"""
    rng = np.random.default_rng(100 + length)
    entries = [(a, vector(rng, CLASSES[i % 5], i // 5 + i, reach=8 * wmb), i % 2, RESIDUALS[1 + i % 5] if (i // 5) % 2 else "none")
               for i, a in enumerate(addresses(rng, wmb * hmb, length))]
    job = run(built, 200 + length, wmb, hmb, entries)
    if length >= 17:
        got = gen_entries(job)
        bins = {(class_of((e[3], e[4])), bool(e[6] & 0x03FFFFFF)) for e in got}
        assert len(bins) == 10, sorted(bins)
        assert any(e[6] & FJ_CODED_WIDE for e in got) and any(e[6] & 0x03FFFFFF and not e[6] & FJ_CODED_WIDE for e in got)
        assert {e[2] for e in got} == {0, 1}


# ---- every class alone in a list, with and without coefficients ----
@pytest.mark.parametrize("coded", [False, True], ids=["uncoded", "coded"])
@pytest.mark.parametrize("cls", CLASSES)
def test_one_class_alone(built, cls, coded):
    """3x2, six entries (a full group and a remainder of two) of one bin: every letter of the class occurs, the class pass runs with all
    slots and no other pass runs"""
    rng = np.random.default_rng(300 + CLASSES.index(cls) + 10 * coded)
    entries = [(a, vector(rng, cls, i, reach=12), i % 2, ["luma", "cac", "all"][i % 3] if coded else "none") for i, a in enumerate(range(6))]
    job = run(built, 400 + CLASSES.index(cls), 3, 2, entries)
    assert {(class_of((e[3], e[4])), bool(e[6] & 0x03FFFFFF)) for e in gen_entries(job)} == {(cls, coded)}


# ---- all 16 luma and all 64 chroma fractions ----
@pytest.mark.parametrize("base", [(0, 0), (-3, 5), (13, -9)], ids=["still", "near", "far"])
def test_every_fraction(built, base):
    """11x6, 64 entries: vector i = 8 * base + (i mod 8, i div 8): every chroma eighth-sample fraction once, every luma quarter-sample
    fraction four times; far: windows of the macroblocks near the borders leave the picture"""
    rng = np.random.default_rng(500)
    addrs = addresses(rng, 66, 64)
    entries = [(a, (8 * base[0] + i % 8, 8 * base[1] + i // 8), i % 2, ["none", "cac"][(i // 3) % 2] if i else "luma") for i, a in enumerate(addrs)]
    run(built, 501, 11, 6, entries)


# ---- where the windows lie ----
def test_windows_across_every_edge_and_corner(built):
    """3x2 (48 x 32 samples): every macroblock with vectors that push its windows across the left, right, upper and lower edge, across
    each corner, and wholly outside the picture; fractions of every class (the clamped gather feeds all of them)"""
    rng = np.random.default_rng(600)
    pushes = [(-40, 0), (40, 0), (0, -40), (0, 40), (-40, -40), (40, -40), (-40, 40), (40, 40), (-400, 300), (700, -500), (-9, 3), (5, -7)]
    jobs_run = 0
    for start in (0, 6):                                            # two pictures of six entries: each macroblock with two of the pushes
        entries = []
        for a in range(6):
            px, py = pushes[start + a]
            fx, fy = CLASS_FRACTIONS[CLASSES[(a + start) % 5]][a % 3 % len(CLASS_FRACTIONS[CLASSES[(a + start) % 5]])]
            entries.append((a, (4 * px + fx + (4 if (fx | fy) == 0 else 0), 4 * py + fy), a % 2, ["none", "all"][a % 2]))
        run(built, 601 + start, 3, 2, entries)
        jobs_run += 1
    assert jobs_run == 2


@pytest.mark.parametrize("rel", [11, 12, 15])
def test_window_start_in_its_first_tile(built, rel):
    """5x4: windows inside the picture whose first column is column rel of a tile — at 11 the 21 columns end in the second tile (the
    third is not fetched), from 12 on they reach the third; from the left and from the right end of a row, all classes"""
    rng = np.random.default_rng(700 + rel)
    entries = []
    for i, a in enumerate([0, 4, 5, 9, 10, 14, 15, 19]):
        mbx = a % 5
        whole_x = (rel + 2) if mbx == 0 else (rel + 2 - 32)         # xi = 16 * mbx + whole_x - 2 = rel (mod 16), inside the picture
        cls = CLASSES[i % 5]
        fx, fy = CLASS_FRACTIONS[cls][i % len(CLASS_FRACTIONS[cls])]
        whole_y = int(rng.integers(-2, 3)) + (8 if a < 10 else -8)
        if cls == "whole":
            whole_y = 2 * (whole_y // 2) + 1                          # half a chroma sample: not a copy macroblock
        entries.append((a, (4 * whole_x + fx, 4 * whole_y + fy), i % 2, ["none", "luma"][i % 2]))
    run(built, 710 + rel, 5, 4, entries)


# ---- residual cases ----
@pytest.mark.parametrize("kind", RESIDUALS)
def test_residual_kinds(built, kind):
    """2x2, four entries (one full group) of one residual kind: no coefficients, luma only, chroma DC only, chroma DC and AC, all 25
    blocks, and FJ_CODED_WIDE with a residual that saturates every sample it touches"""
    rng = np.random.default_rng(800 + RESIDUALS.index(kind))
    entries = [(a, vector(rng, CLASSES[(a + 1) % 5], a, reach=10), a % 2, kind) for a in range(4)]
    job = run(built, 810 + RESIDUALS.index(kind), 2, 2, entries)
    got = gen_entries(job)
    if kind == "wide_sat":
        assert all(e[6] & FJ_CODED_WIDE for e in got)
    elif kind != "none":
        assert all(e[6] & 0x03FFFFFF and not e[6] & FJ_CODED_WIDE for e in got)


def test_full_pipeline_with_the_filter_on_top(built):
    """5x4, 17 mixed entries through all stages (k_dbk and the per-picture kernels read what the list kernel wrote), four streams"""
    rng = np.random.default_rng(900)
    entries = [(a, vector(rng, CLASSES[i % 5], i, reach=20), i % 2, RESIDUALS[i % 5]) for i, a in enumerate(addresses(rng, 20, 17))]
    run(built, 901, 5, 4, entries, stages=7, n_streams=4)
