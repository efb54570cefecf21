"""GPU: saturated pictures through pull_flow, pull_shift, pull_corners and pull_matches, through the product library.  The four kernels
behind them state bounds on their intermediate sums — the packed 16-bit SADs of k_cell_shift and k_region_shift (SHIFT_FOLD instructions
of at most 1020 each), the 64-bit energy of k_corner_points and its exact square root, the u16 box sums of k_point_describe — and the
pictures here are chosen so that those bounds are REACHED: every picture is an all-I_PCM stream (tests/pcm_pictures.py), every expected
value an exact integer of the models, and the `sat` pair has closed forms beside them.  Which item of which kernel each case reaches, and
that no case can be dropped without losing one, is held on the CPU by tests/test_saturated_motion_reach.py, which reads the lists below."""
import numpy as np
import pytest

import corners_model as cm
import flow_model as fm
import matches_model as mm
import shift_model as shm
from test_gpu_cell_shift import ALL
from test_gpu_cell_shift import _pull as _pull_flow
from test_gpu_cell_shift import _same as _same_maps
from test_gpu_corner_points import Chosen as ChosenCurrent
from test_gpu_corner_points import _check as _check_corners
from test_gpu_corner_points import _pull as _pull_corners
from test_gpu_point_matches import _pull as _pull_matches
from test_gpu_point_matches import _same as _same_matches
from test_gpu_region_shift import Chosen
from test_gpu_region_shift import _pull as _pull_shift
from test_gpu_region_shift import _same as _same_record

pytestmark = pytest.mark.gpu

FW, FH = 80, 80             # 5 x 5 macroblocks: one full 64 x 64 rectangle of k_cell_shift and a partial one each way
SW, SH = 288, 48            # 18 x 3 macroblocks: a 32 x 256 tile of k_region_shift, three bands; a band of two-sample columns above 2^32
MW, MH = 80, 80             # 16 x 16 blocks of 5 x 5 samples for the descriptors

PAIRS = ("sat", "sat-reversed", "dark-bright")


def pair(name, w, h):
    """(kept, current) luma planes"""
    if name == "sat":
        return np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)
    if name == "sat-reversed":
        return np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8)
    assert name == "dark-bright"
    rng = np.random.default_rng(41)
    return rng.integers(0, 16, (h, w), dtype=np.uint8), rng.integers(240, 256, (h, w), dtype=np.uint8)


# ---- pull_flow ----
FLOW_BOXES = [None, (-21, -13, 150, 120), (3, 5, 69, 70)]               # None: the whole window; the others start and end inside a dword
FLOW_DEEP = [(cell, radius) for cell in (32, 64) for radius in (8, 12, 16)]     # where the fold runs: on every pair
FLOW_SHALLOW = [(cell, radius) for cell in fm.CELLS for radius in (0, 3, 4)]    # both instantiations, no fold: on `sat`
FLOW_CASES = [(p, c, r) for p in PAIRS for c, r in FLOW_DEEP] + [("sat", c, r) for c, r in FLOW_SHALLOW]

# ---- pull_shift ----
SHIFT_PAIRS = ("sat", "dark-bright")
SHIFT_RADII = (1, 4, 8, 12, 16)
SHIFT_BOXES = [(0, 0, SW, SH), (0, 0, 256, 32), (16, 16, 256, 16), (3, 5, 253, 40)]
SHIFT_PAD = ((5, 7, 1, 1), 512)                                         # with 512 of these behind the boxes every region is ONE band: tiles of 32 rows

# ---- pull_corners ----
CORNER_PICTURES = ("columns", "dots", "wide-columns", "quadrant")
COLUMN_PICTURES = ("columns", "wide-columns")
CORNER_BOXES = [(0, 0, SW, SH), (0, 16, SW, 16), (3, 5, 253, 40), (-9, 10, 30, 20)]
CORNER_PARAMS = [(score, block, nms) for score in (cm.MIN_EIGEN, cm.HARRIS) for block in (3, 5) for nms in (1, 3)]
CORNER_PAD = ((5, 7, 9, 9), 512)


def corner_picture(name, w=SW, h=SH):
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    on = {"columns": x & 1, "dots": (x & 1) & (y & 1), "wide-columns": (x >> 1) & 1, "quadrant": (x >= w // 2) & (y >= h // 2)}[name]
    return (on.astype(bool) * 255).astype(np.uint8)


# ---- pull_matches ----
def match_picture(w=MW, h=MH):
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    return ((((x // 5) + (y // 5)) & 1) * 255).astype(np.uint8)


MATCH_K = 64
# the four corners of the window (the clamp in two directions) and 60 points at every phase of the blocks
MATCH_POINTS = [(0, 0), (MW - 1, 0), (0, MH - 1), (MW - 1, MH - 1)] + [(1 + 10 * (k % 8) + k // 8, 2 + 10 * (k // 8) + k % 3) for k in range(4, MATCH_K)]


def match_sums(win, points):
    """(B(p), B(q)) of every test of every point: [len(points), 256] each"""
    B = mm.box_sums(win.astype(np.int64))
    x, y = np.array([p[0] for p in points])[:, None] + mm.REACH, np.array([p[1] for p in points])[:, None] + mm.REACH
    return B[y + mm.PATTERN[None, :, 1], x + mm.PATTERN[None, :, 0]], B[y + mm.PATTERN[None, :, 3], x + mm.PATTERN[None, :, 2]]


@pytest.fixture(autouse=True, scope="module")
def _through_the_product_library(built):
    built.use_product_library(True)
    yield
    built.use_product_library(False)


@pytest.fixture(autouse=True)
def _no_device_errors(built):
    yield
    assert built.device_errors() == 0


class _Decoders:
    """the decoders of the pictures asked for, opened once"""

    def __init__(self, built, make):
        self.built, self.make, self.open = built, make, {}

    def __call__(self, name):
        if name not in self.open:
            self.open[name] = self.make(self.built, name)
        return self.open[name]

    def close(self):
        for c in self.open.values():
            c.close()


@pytest.fixture(scope="module")
def flow_pairs(built, _through_the_product_library):
    d = _Decoders(built, lambda b, name: Chosen(b, list(pair(name, FW, FH))))
    yield d
    d.close()


@pytest.fixture(scope="module")
def shift_pairs(built, _through_the_product_library):
    def make(b, name):
        c = Chosen(b, list(pair(name, SW, SH)))
        c.models = {}                                       # per radius: the records of SHIFT_BOXES and of the pad
        return c

    d = _Decoders(built, make)
    yield d
    d.close()


@pytest.fixture(scope="module")
def corner_pictures(built, _through_the_product_library):
    d = _Decoders(built, lambda b, name: ChosenCurrent(b, [corner_picture(name)]))
    yield d
    d.close()


@pytest.mark.parametrize("name,cell,radius", FLOW_CASES)
def test_flow_of_saturated_pairs_equals_the_model(built, flow_pairs, name, cell, radius):
    """the three boxes as three regions of one call, all six planes, on a grid that covers the largest box: cells of 32 and 64 at radius
    8 and more unpack their packed sums on the way, and on `sat` a packed sum reaches 64 x 1020 = 65280 exactly"""
    c = flow_pairs(name)
    window = (0, 0, FW, FH)
    boxes = [b or window for b in FLOW_BOXES]
    grid = fm.default_grid([(b[3], b[2]) for b in boxes], cell)
    want = [fm.maps_fast(c.lumas[0], c.lumas[1], window, b, cell, grid, radius) for b in boxes]
    D = 2 * radius + 1
    for w in want:
        if name in ("sat", "sat-reversed"):                 # the closed forms, beside the model
            assert np.array_equal(w[3], 255 * w[0]) and np.array_equal(w[4], 255 * w[0]) and not w[1].any() and not w[2].any() and (w[5] == D * D).all()
        else:                                               # large, unequal sums: the argmin decides among them
            full = w[0] == cell * cell
            assert (w[3][full] >= 225 * cell * cell).all() and (w[4][full] <= 255 * cell * cell).all()
            assert radius == 0 or (w[5][full] < D * D).all()
    assert want[0][0].max() == cell * cell                  # a full cell, and with it a full row of dwords
    cs, got = _pull_flow(built, [c.dec], [(0,) + b for b in boxes], cell, grid, radius)
    assert cs.got == [1] * len(boxes)
    for k, b in enumerate(boxes):
        _same_maps(got[k], want[k], (name, cell, radius, b))
    for k, plane in enumerate(ALL):
        assert np.array_equal(getattr(cs, plane).cpu().numpy(), np.stack([w[k] for w in want])), plane


def _shift_model(c, radius):
    if radius not in c.models:
        window = (0, 0, SW, SH)
        c.models[radius] = [shm.record(c.lumas[0], c.lumas[1], window, b, radius) for b in SHIFT_BOXES + [SHIFT_PAD[0]]]
    return c.models[radius]


@pytest.mark.parametrize("surface", [True, False], ids=["surface", "header"])
@pytest.mark.parametrize("radius", SHIFT_RADII)
@pytest.mark.parametrize("name", SHIFT_PAIRS)
def test_shift_of_saturated_pairs_equals_the_model(built, shift_pairs, name, radius, surface):
    """the four boxes in one call: three bands each, the bands' partial surfaces of saturated sums meet in the scratch.  Then the same
    boxes with 512 one-sample regions behind them: one band per region, so the two boxes of 32 rows and more are walked in tiles of
    32 x 256 samples, the segments at their longest (32 dwords from radius 12 on), every packed sum of `sat` 1020 per instruction"""
    c = shift_pairs(name)
    want = _shift_model(c, radius)
    D = 2 * radius + 1
    for w, b in zip(want, SHIFT_BOXES):
        assert w.count == b[2] * b[3]
        if name == "sat":
            assert w.best == w.still == 255 * w.count and (w.dx, w.dy) == (0, 0) and w.ties == D * D
        else:
            assert w.best >= 225 * w.count and w.ties < D * D
    sh = _pull_shift(built, [c.dec], [(0,) + b for b in SHIFT_BOXES], radius, surface)
    assert sh.got == [1] * len(SHIFT_BOXES)
    for k, b in enumerate(SHIFT_BOXES):
        _same_record(sh, k, want[k], surface, (name, radius, "bands", b))
    regions = [(0,) + b for b in SHIFT_BOXES] + [(0,) + SHIFT_PAD[0]] * SHIFT_PAD[1]
    sh = _pull_shift(built, [c.dec], regions, radius, surface)
    assert sh.got == [1] * len(regions)
    host = built.RegionShift(sh.records.cpu(), radius, surface, sh.got, sh.current, sh.kept, sh.pic_id, sh.kept_pic_id)
    for k in range(len(SHIFT_BOXES)):
        _same_record(host, k, want[k], surface, (name, radius, "one band", SHIFT_BOXES[k]))
    pad = want[-1].bytes(surface)
    raw = host.records.numpy()
    assert all(bytes(raw[k]) == pad for k in range(len(SHIFT_BOXES), len(regions)))


@pytest.mark.parametrize("score,block,nms", CORNER_PARAMS)
@pytest.mark.parametrize("name", CORNER_PICTURES)
def test_corners_of_extreme_pictures_equal_the_model(built, corner_pictures, name, score, block, nms):
    """the worst pictures of the model's own extremes test, and one bright quadrant.  Pure columns have B = C = 0: the MIN_EIGEN
    radicand is A A exactly, the root must be A and every score 0; every Harris score is negative.  Two-sample columns carry an energy
    above 2^32 in the whole window (three bands through the scratch) and in the one band of rows 16 .. 31 alone"""
    c = corner_pictures(name)
    m = c.model(score, block)
    K = 64
    cp = _pull_corners(built, [c.dec], [(0,) + b for b in CORNER_BOXES], K, score=score, block=block, nms=nms)
    assert cp.got == [1] * len(CORNER_BOXES)
    if name in COLUMN_PICTURES:                             # without the model's help
        assert cp.found.tolist() == [0] * len(CORNER_BOXES) and cp.written.tolist() == [0] * len(CORNER_BOXES)
    for k, b in enumerate(CORNER_BOXES):
        assert int(cp.energy[k]) == m.points(b, nms)[1], (name, b)
    if name == "wide-columns":
        assert int(cp.energy[0]) == 1020 * 1020 * (SW - 2) * SH > 2 ** 32 and int(cp.energy[1]) == 1020 * 1020 * (SW - 2) * 16 > 2 ** 32
    _check_corners(cp, [m.record(b, nms, K) for b in CORNER_BOXES], (name, score, block, nms))


@pytest.mark.parametrize("name", ["wide-columns", "quadrant"])
def test_corners_when_every_region_is_one_band(built, corner_pictures, name):
    """more regions than the scratch has partials for: band_count gives S = 1, the whole window's workgroup walks all three macroblock
    rows itself and closes the record with an energy above 2^32 that never went through a partial"""
    c = corner_pictures(name)
    boxes = CORNER_BOXES[:2] + [CORNER_PAD[0]] * CORNER_PAD[1]
    for score in (cm.MIN_EIGEN, cm.HARRIS):
        m = c.model(score, 3)
        cp = _pull_corners(built, [c.dec], [(0,) + b for b in boxes], 16, score=score, block=3, nms=3)
        assert cp.got == [1] * len(boxes)
        wants = [m.record(b, 3, 16) for b in CORNER_BOXES[:2]] + [m.record(CORNER_PAD[0], 3, 16)] * CORNER_PAD[1]
        _check_corners(cp, wants, (name, score, "one band"))
        assert int(cp.energy[0]) == m.points(boxes[0], 3)[1] and (int(cp.energy[0]) > 2 ** 32) == (name == "wide-columns")


def test_matches_on_blocks_of_0_and_255(built):
    """5 x 5 blocks of 0 / 255 against their complement: where a 5 x 5 box sum lies on a block it is 0 or 6375, the ends of the u16
    sums, and between blocks of equal phase two sums are equal, where the strict comparison gives 0 on both sides.  The complement
    inverts every other bit, so the distances are large: max_distance 256 and no ratio test, so that the slots are all filled"""
    kept = match_picture()
    cur = 255 - kept
    window = box = (0, 0, MW, MH)
    for win in (kept, cur):
        bp, bq = match_sums(win, MATCH_POINTS)
        assert ((bp == 0) | (bq == 0)).sum() >= 256 and ((bp == 6375) | (bq == 6375)).sum() >= 256 and (bp == bq).sum() >= 256
        assert ((bp == 0) & (bq == 6375)).any() and ((bp == 6375) & (bq == 0)).any()
    kp = cp = mm.points_record(MATCH_POINTS, MATCH_K)
    kw = dict(max_distance=256, ratio=256, mutual=False)
    want = mm.record_fast(kept, cur, window, box, kp, cp, MATCH_K, max_distance=256, ratio=256, mutual_only=0)
    w = mm.Record(want, MATCH_K)
    assert w.kept_valid == w.current_valid == w.accepted == MATCH_K and max(s[1] for s in w.slots) > 64
    c = Chosen(built, [kept, cur])
    m, got = _pull_matches(built, [c.dec], [kp], [cp], None, MATCH_K, **kw)
    assert m.got == [1]
    _same_matches(got[0], want, MATCH_K, "blocks")
    same = mm.record_fast(cur, cur, window, box, kp, cp, MATCH_K, max_distance=256, ratio=256, mutual_only=0)
    assert all(s[1] == 0 for s in mm.Record(same, MATCH_K).slots)
    assert built.keep_pictures([c.dec])[0] == [1]           # the complement on both sides: every slot finds itself at distance 0
    m, got = _pull_matches(built, [c.dec], [kp], [cp], None, MATCH_K, **kw)
    _same_matches(got[0], same, MATCH_K, "blocks, the same picture")
    c.close()
