"""GPU parity of the quadrant inter kernel (k_recon_inter_lq: the 8x8 quadrants of a chunk of list entries binned by interpolation class, 16
quadrants per wavefront, a 4x4 block per lane) on hand-built jobs whose QUADRANT list is laid out on purpose: kernels vs CPU oracle, byte
for byte.  In the manner of test_gpu_inter_lane_blocks.py (whose helpers it uses): every picture is two noise intra pictures (slots 0, 1)
and one P picture in which chosen macroblocks carry one motion vector and one reference slot per 8x8 quadrant, with the FJ_PARTS_* bits to
match; all the others are zero-motion copies.  What the list then holds is the test: its length (group remainder, chunk remainder, more
than one chunk), the bins of its quadrants, the partition shapes, where the windows lie, which coefficient blocks there are."""
import struct

import numpy as np
import pytest

import test_gpu_inter_lane_blocks as lb
from jobgen import build_job
from replay_compare import run_and_compare

pytestmark = pytest.mark.gpu

CHUNK = 8                                                      # INTER_LQ_CHUNK (kernels/k_recon_inter_lanes.hip.h)
CLASSES, CLASS_FRACTIONS, RESIDUALS, FJ_CODED_WIDE = lb.CLASSES, lb.CLASS_FRACTIONS, lb.RESIDUALS, lb.FJ_CODED_WIDE
FJ_PARTS_8x8, FJ_PARTS_16x8, FJ_PARTS_8x16 = 0, 2, 3


def quadrant_mask(q):
    """the bits of the coded word that reach quadrant q: its luma blocks (H.264 block order), its chroma block per plane, the chroma DC"""
    return (0xF << (4 * q)) | (0x00110000 << q) | (1 << 25)


def _residual(rng, kind):
    if kind.startswith("only_q"):                              # every coded block lies in one quadrant: three luma blocks, one Cr AC block
        q = int(kind[-1])
        coded, blocks = 0, []
        for z in (4 * q, 4 * q + 1, 4 * q + 3):
            blocks.append(lb._levels(rng)); coded |= 1 << z
        blocks.append(lb._levels(rng, ac_only=True)); coded |= 1 << (20 + q)
        return coded, blocks, int(rng.integers(10, 31))
    return lb._residual(rng, kind)


def p_picture(lib, seed, wmb, hmb, entries):
    """entries: [(macroblock address, four (mvx, mvy) in quarter samples, four reference slots, residual kind)] in ascending address order,
    quadrants in raster order — the quadrant list of the picture; every other macroblock copies slot 0 in place"""
    rng = np.random.default_rng(seed)
    n = wmb * hmb
    by_mb = {a: (mv, slots, kind) for a, mv, slots, kind in entries}
    assert len(by_mb) == len(entries)

    def patch(recs, mvs16, first_extra):
        coefs = lb._buffer_of(recs)[128 + n * 32 + n * 64:].view(np.int16)
        mvs = mvs16.reshape(n, 4, 4, 2)
        nb = first_extra
        for a in range(n):
            r = recs[a]
            r[0], r[4] = 0, 1 << 4                                  # inter, one 16x16 partition
            r[8:12] = 0
            if a not in by_mb:
                mvs[a] = (0, 0); r[16:20] = 0
                continue
            mv, slots, kind = by_mb[a]
            mv = [tuple(v) for v in mv]
            assert len(set(mv)) > 1 or len(set(slots)) > 1, "a macroblock with one vector and one slot is no quadrant entry"
            for q in range(4):
                mvs[a, 2 * (q >> 1):2 * (q >> 1) + 2, 2 * (q & 1):2 * (q & 1) + 2] = mv[q]
                r[16 + q] = slots[q]
            pairs = lambda i, j: mv[i] == mv[j] and slots[i] == slots[j]
            parts = FJ_PARTS_16x8 if pairs(0, 1) and pairs(2, 3) else FJ_PARTS_8x16 if pairs(0, 2) and pairs(1, 3) else FJ_PARTS_8x8
            r[4] = parts << 4
            coded, blocks, qp = _residual(rng, kind)
            if qp is not None:
                r[1], r[2] = qp, lb.QPC[qp]
            struct.pack_into("<I", r, 8, coded)
            struct.pack_into("<I", r, 12, nb)
            for blk in blocks:
                coefs[16 * nb:16 * nb + 16] = blk; nb += 1

    job = build_job(lib, rng, wmb, hmb, 2, 3, [0, 1], p_inter=1.0, patch=patch, extra_blocks=25 * len(entries) + 1)
    # the finished job must hold the list this test is about: quadrant entries only
    n_gen, n_uni, n_quad = (struct.unpack_from("<I", job, o)[0] for o in (72, 84, 100))
    assert (n_gen, n_uni, n_quad) == (len(entries), 0, len(entries)), (n_gen, n_uni, n_quad, len(entries))
    return job


def run(built, seed, wmb, hmb, entries, stages=3, n_streams=2):
    lib = built.lib()
    job = p_picture(lib, seed, wmb, hmb, entries)
    run_and_compare(built, lb._intra_pictures(lib, wmb, hmb) + [job], n_streams=n_streams, stages=stages)
    return job


def quadrants(job):
    """[(macroblock, quadrant, (mvx, mvy), slot, coded word)] of the finished job's quadrant list, in list order"""
    gen_off, rec_off, mvx_off = (struct.unpack_from("<I", job, o)[0] for o in (68, 20, 104))
    n_uni, n_quad = struct.unpack_from("<I", job, 84)[0], struct.unpack_from("<I", job, 100)[0]
    out = []
    for i in range(n_uni, n_uni + n_quad):
        mb, uniform, _, idx, _, coded = struct.unpack_from("<HBBIII", job, gen_off + 16 * i)
        assert uniform == 2
        for q in range(4):
            mv = struct.unpack_from("<hh", job, mvx_off + 64 * idx + 4 * ((q >> 1) * 8 + (q & 1) * 2))
            out.append((mb, q, mv, job[rec_off + 32 * mb + 16 + q], coded))
    return out


def bins(job):
    return {(lb.class_of(mv), bool(coded & quadrant_mask(q))) for _, q, mv, _, coded in quadrants(job)}


def vector(rng, cls, i, reach=24):
    """a vector of the class, its whole part within +-reach samples, the fraction the i-th of the class"""
    fx, fy = CLASS_FRACTIONS[cls][i % len(CLASS_FRACTIONS[cls])]
    return 4 * int(rng.integers(-reach, reach + 1)) + fx, 4 * int(rng.integers(-reach, reach + 1)) + fy


# ---- list lengths: the group remainder (a group is 4 entries' quadrants), the chunk remainder and more than one chunk ----
@pytest.mark.parametrize("wmb,hmb,length", [(1, 1, 1), (2, 2, 1), (2, 2, 3), (2, 2, 4), (3, 2, 5), (5, 4, 17), (11, 6, CHUNK - 1), (11, 6, CHUNK), (11, 6, CHUNK + 1)])
def test_list_lengths_with_every_bin_in_turn(built, wmb, hmb, length):
    """quadrant q of entry i is of class (i + q) mod 5: the quadrants of a macroblock are in four classes, every group is mixed; coded and
    uncoded entries in turns of three (the coded ones with each residual kind in turn, WIDE among them), both reference slots"""
    rng = np.random.default_rng(1100 + length)
    entries = [(a, [vector(rng, CLASSES[(i + q) % 5], i + q, reach=8 * wmb) for q in range(4)], [(i + q) % 2 for q in range(4)],
                RESIDUALS[1 + i % 5] if (i // 3) % 2 else "none") for i, a in enumerate(lb.addresses(rng, wmb * hmb, length))]
    job = run(built, 1200 + length, wmb, hmb, entries)
    if length >= 17:
        assert len(bins(job)) == 10, sorted(bins(job))
        coded = {c for *_, c in quadrants(job)}
        assert any(c & FJ_CODED_WIDE for c in coded) and any(c & 0x03FFFFFF and not c & FJ_CODED_WIDE for c in coded)
    assert {s for _, _, _, s, _ in quadrants(job)} == {0, 1}


# ---- every class alone in a list, with and without coefficients ----
@pytest.mark.parametrize("coded", [False, True], ids=["uncoded", "coded"])
@pytest.mark.parametrize("cls", CLASSES)
def test_one_class_alone(built, cls, coded):
    """3x2, six entries (one full group and a remainder of eight quadrants) of one bin: all 24 quadrants of the class, with different
    whole-sample parts and every letter of the class; coded: all 25 blocks, so every quadrant is coded"""
    rng = np.random.default_rng(1300 + CLASSES.index(cls) + 10 * coded)
    entries = [(a, [vector(rng, cls, a + q, reach=12) for q in range(4)], [(a + q) % 2 for q in range(4)], "all" if coded else "none") for a in range(6)]
    job = run(built, 1400 + CLASSES.index(cls), 3, 2, entries)
    assert bins(job) == {(cls, coded)}


# ---- partition shapes ----
@pytest.mark.parametrize("shape", ["16x8", "8x16", "four_vectors", "equal_classes", "slots_only"])
def test_partition_shapes(built, shape):
    """3x2, six entries of one shape: 16x8 and 8x16 (two quadrants share a vector and a slot), four different vectors, four vectors of one
    class that differ in their whole-sample parts, and one vector whose quadrants refer to different slots"""
    rng = np.random.default_rng(1500 + len(shape))
    entries = []
    for a in range(6):
        v = [vector(rng, CLASSES[(a + q) % 5], a + q, reach=12) for q in range(4)]
        slots = [(a + q) % 2 for q in range(4)]
        if shape == "16x8":
            v, slots = [v[0], v[0], v[2], v[2]], [slots[0], slots[0], slots[2], slots[2]]
        elif shape == "8x16":
            v, slots = [v[0], v[1], v[0], v[1]], [slots[0], slots[1], slots[0], slots[1]]
        elif shape == "equal_classes":
            fx, fy = CLASS_FRACTIONS[CLASSES[a % 5]][a % len(CLASS_FRACTIONS[CLASSES[a % 5]])]
            v = [(4 * (3 * q - 5 + a) + fx, 4 * (7 - 4 * q) + fy) for q in range(4)]
        elif shape == "slots_only":
            v, slots = [v[0]] * 4, [[0, 1, 1, 0], [1, 0, 0, 1], [0, 0, 0, 1]][a % 3]
        entries.append((a, v, slots, ["none", "all", "luma"][a % 3]))
    job = run(built, 1510 + len(shape), 3, 2, entries)
    got = quadrants(job)
    per_mb = [got[4 * i:4 * i + 4] for i in range(6)]
    if shape == "16x8":
        assert all(m[0][2:4] == m[1][2:4] and m[2][2:4] == m[3][2:4] and m[0][2:4] != m[2][2:4] for m in per_mb)
    elif shape == "8x16":
        assert all(m[0][2:4] == m[2][2:4] and m[1][2:4] == m[3][2:4] and m[0][2:4] != m[1][2:4] for m in per_mb)
    elif shape == "four_vectors":
        assert all(len({x[2] for x in m}) == 4 for m in per_mb)
    elif shape == "equal_classes":
        assert all(len({lb.class_of(x[2]) for x in m}) == 1 and len({x[2] for x in m}) == 4 for m in per_mb)
    else:
        assert all(len({x[2] for x in m}) == 1 and len({x[3] for x in m}) == 2 for m in per_mb)


# ---- all 16 luma and all 64 chroma fractions ----
@pytest.mark.parametrize("base", [(0, 0), (-3, 5), (13, -9)], ids=["still", "near", "far"])
def test_every_fraction(built, base):
    """11x6, 64 entries: quadrant k = 4 * i + q has the vector 8 * base + (k mod 8, k div 8 mod 8): every chroma eighth-sample fraction four
    times, every luma quarter-sample fraction sixteen times; far: windows of the quadrants near the borders leave the picture"""
    rng = np.random.default_rng(1600)
    addrs = lb.addresses(rng, 66, 64)
    entries = [(a, [(8 * base[0] + (4 * i + q) % 8, 8 * base[1] + (4 * i + q) // 8 % 8) for q in range(4)], [(i + q) % 2 for q in range(4)],
                ["none", "cac"][(i // 3) % 2] if i else "luma") for i, a in enumerate(addrs)]
    job = run(built, 1601, 11, 6, entries)
    assert {(mv[0] & 7, mv[1] & 7) for _, _, mv, _, _ in quadrants(job)} == {(x, y) for x in range(8) for y in range(8)}


# ---- where the windows lie ----
def test_windows_across_every_edge_and_corner(built):
    """3x2 (48 x 32 samples): per quadrant, vectors that push its windows across the left, right, upper and lower edge, across each corner
    and wholly outside the picture; the right and lower quadrants of a macroblock are pushed the opposite way; fractions of every class"""
    pushes = [(-40, 0), (40, 0), (0, -40), (0, 40), (-40, -40), (40, -40), (-40, 40), (40, 40), (-400, 300), (700, -500), (-9, 3), (5, -7)]
    for start in (0, 6):                                            # two pictures of six entries: each macroblock with two of the pushes
        entries = []
        for a in range(6):
            px, py = pushes[start + a]
            v = []
            for q in range(4):
                cls = CLASSES[(a + start + q) % 5]
                fx, fy = CLASS_FRACTIONS[cls][(a + q) % len(CLASS_FRACTIONS[cls])]
                v.append((4 * (-px if q & 1 else px) + fx, 4 * (-py if q >> 1 else py) + fy))
            entries.append((a, v, [(a + q) % 2 for q in range(4)], ["none", "all"][a % 2]))
        job = run(built, 1701 + start, 3, 2, entries)
        assert len(quadrants(job)) == 24


@pytest.mark.parametrize("rel", [3, 4, 11, 12, 15])
def test_window_start_in_its_first_tile(built, rel):
    """5x4: windows inside the picture whose first column is column rel of a tile — up to 3 the 13 columns end in the first tile (the second
    is not fetched), from 4 on they reach the second; 11, 12, 15: as for the 21-column window; from both ends of a row, all classes"""
    rng = np.random.default_rng(1800 + rel)
    entries = []
    for i, a in enumerate([0, 4, 5, 9, 10, 14, 15, 19]):
        mbx, v = a % 5, []
        for q in range(4):
            xi = rel + (16 if mbx == 0 else 48)                     # first window column: rel (mod 16), the window inside the picture
            whole_x = xi + 2 - 8 * (q & 1) - 16 * mbx               # xi = 16 * mbx + 8 * (q & 1) + whole_x - 2
            cls = CLASSES[(i + q) % 5]
            fx, fy = CLASS_FRACTIONS[cls][(i + q) % len(CLASS_FRACTIONS[cls])]
            whole_y = int(rng.integers(-2, 3)) + (8 if a < 10 else -8)
            v.append((4 * whole_x + fx, 4 * whole_y + fy))
        entries.append((a, v, [(i + q) % 2 for q in range(4)], ["none", "luma"][i % 2]))
    job = run(built, 1810 + rel, 5, 4, entries)
    assert all((16 * (mb % 5) + 8 * (q & 1) + (mv[0] >> 2) - 2) % 16 == rel and 0 <= 16 * (mb % 5) + 8 * (q & 1) + (mv[0] >> 2) - 2 <= 80 - 13
               for mb, q, mv, _, _ in quadrants(job))


# ---- residual cases ----
@pytest.mark.parametrize("kind", RESIDUALS + ["only_q0", "only_q3", "wide_among_packed"])
def test_residual_kinds(built, kind):
    """2x2, four entries (one full group): the six kinds of test_gpu_inter_lane_blocks.py (FJ_CODED_WIDE with saturation among them), a
    macroblock whose coded blocks all lie in one quadrant (its other three are binned as not coded), and a group in which one macroblock
    is WIDE and the others packed"""
    rng = np.random.default_rng(1900 + len(kind))
    kinds = ["luma", "wide_sat", "all", "cac"] if kind == "wide_among_packed" else [kind] * 4
    entries = [(a, [vector(rng, CLASSES[(a + q + 1) % 5], a + q, reach=10) for q in range(4)], [(a + q) % 2 for q in range(4)], kinds[a]) for a in range(4)]
    job = run(built, 1910 + len(kind), 2, 2, entries)
    got = quadrants(job)
    coded = [c for *_, c in got[::4]]
    if kind == "wide_sat":
        assert all(c & FJ_CODED_WIDE for c in coded)
    elif kind == "wide_among_packed":
        assert [bool(c & FJ_CODED_WIDE) for c in coded] == [False, True, False, False] and all(c & 0x03FFFFFF for c in coded)
    elif kind.startswith("only_q"):
        want = int(kind[-1])
        assert all(bool(c & quadrant_mask(q)) == (q == want) for _, q, _, _, c in got)
    elif kind != "none":
        assert all(c & 0x03FFFFFF and not c & FJ_CODED_WIDE for c in coded)


def test_full_pipeline_with_the_filter_on_top(built):
    """5x4, 17 mixed entries through all stages (k_dbk and the per-picture kernels read what the list kernel wrote), four streams"""
    rng = np.random.default_rng(2000)
    entries = [(a, [vector(rng, CLASSES[(i + q) % 5], i + q, reach=20) for q in range(4)], [(i + q) % 2 for q in range(4)], RESIDUALS[i % 5])
               for i, a in enumerate(lb.addresses(rng, 20, 17))]
    job = run(built, 2001, 5, 4, entries, stages=7, n_streams=4)
    assert len(bins(job)) >= 8
