"""GPU: h264bsdmiOutputCornerPoints / pull_corners through the product library.  The pictures are chosen (tests/pcm_pictures.py: all-I_PCM
streams carry any picture verbatim), so the current picture is known exactly, and every record is compared with tests/corners_model.py
byte for byte: nothing is skipped and nothing tolerated."""
import ctypes

import numpy as np
import pytest

import corners_model as cm
import pcm_pictures as pp
import shift_model as shm
from test_gpu_tensor_colour import Feed

pytestmark = pytest.mark.gpu

W, H = 64, 48                                           # 4 x 3 macroblocks: a whole-window region runs three bands, one macroblock row each
CROP = dict(crop=(1, 2, 2, 2), window=(2, 4, 58, 40))   # frame_crop offsets in chroma samples: the window is at no macroblock edge
BW, BH = 144, 80                                        # 9 x 5 macroblocks: wider than two tiles of 64, taller than two of 32
SHIFT = (3, -2)
FILL = 0x5A
SCORES = [cm.MIN_EIGEN, cm.HARRIS]


@pytest.fixture(autouse=True, scope="module")
def _through_the_product_library(built):
    built.use_product_library(True)
    yield
    built.use_product_library(False)


@pytest.fixture(autouse=True)
def _no_device_errors(built):
    yield
    assert built.device_errors() == 0


def _picture(Y):
    return (Y, np.full((Y.shape[0] // 2, Y.shape[1] // 2), 128, np.uint8), np.full((Y.shape[0] // 2, Y.shape[1] // 2), 128, np.uint8))


class Chosen:
    """a decoder whose pictures are `lumas`, the first of them current; the models of its window, one per (score, block)"""

    def __init__(self, built, lumas, crop=None, window=None):
        self.lumas = lumas
        self.feed = Feed(built, pp.pcm_stream([_picture(Y) for Y in lumas], crop=crop))
        self.dec = self.feed.dec
        self.window = window or (0, 0, lumas[0].shape[1], lumas[0].shape[0])
        self.models = {}
        self.next()

    def next(self):
        assert self.feed.step()
        assert self.dec.next_output_info() is not None

    def model(self, score, block, picture=0):
        x, y, w, h = self.window
        if (score, block, picture) not in self.models:
            self.models[score, block, picture] = cm.Window(self.lumas[picture][y:y + h, x:x + w], score, block)
        return self.models[score, block, picture]

    def close(self):
        self.feed.close()


def _pull(built, decs, regions, K, **kw):
    """pull_corners into a record buffer that starts as FILL: the call writes whole records, zeros included"""
    import torch
    R = len(decs) if regions is None else len(regions)
    out = torch.full((R, built.corners_record_bytes(K)), FILL, dtype=torch.uint8, device="cuda")
    cp = built.pull_corners(decs, regions, max_points=K, out=out, **kw)
    assert cp.records is out and tuple(out.shape) == (R, cm.record_bytes(K))
    return cp


def _same(cp, host, k, want, what=None):
    """record k (host: the records on the host) against the model's bytes"""
    got = bytes(host[k])
    if got != want:
        g, w = np.frombuffer(got, "<u4"), np.frombuffer(want, "<u4")
        at = int(np.nonzero(g != w)[0][0])
        raise AssertionError((what, k, "header", g[:8].tolist(), w[:8].tolist(), "first difference at word", at, g[at:at + 8].tolist(), w[at:at + 8].tolist()))


def _check(cp, wants, what=None):
    host = cp.records.cpu().numpy()
    for k, want in enumerate(wants):
        _same(cp, host, k, want, what)


def _boxes(ww, wh):
    return [(0, 0, ww, wh), (5, 7, 1, 1), (13, 11, 37, 23), (-9, 10, 30, 20), (50, -7, 25, 19), (200, 200, 8, 8),
            (0, 0, 8, 8), (ww - 8, 0, 8, 8), (0, wh - 8, 8, 8), (ww - 8, wh - 8, 8, 8)]


@pytest.fixture(scope="module", params=[False, True], ids=["coded", "cropped"])
def small(request, built, _through_the_product_library):
    Y = np.random.default_rng(5).integers(0, 256, (H, W), dtype=np.uint8)
    c = Chosen(built, [Y], crop=CROP["crop"] if request.param else None, window=CROP["window"] if request.param else None)
    yield c
    c.close()


@pytest.fixture(scope="module")
def large(built, _through_the_product_library):
    Y = np.random.default_rng(11).integers(0, 256, (BH, BW), dtype=np.uint8)
    c = Chosen(built, [Y])
    yield c
    c.close()


@pytest.mark.parametrize("nms", [1, 3, 7])
@pytest.mark.parametrize("block", [3, 5])
@pytest.mark.parametrize("score", SCORES)
def test_boxes_of_a_random_picture_equal_the_model(built, small, score, block, nms):
    """the whole window (three macroblock rows: three bands, whose halos cross the seams), one sample, a box across macroblock edges,
    boxes that leave the window on each side, one that misses it (the empty record), the four corners (the replication in two
    directions); K = 64 is fewer than the whole window's candidates at nms 1 and more than any box's at nms 7"""
    ww, wh = small.window[2:]
    assert small.dec.cropping_params()[0] == (small.window != (0, 0, W, H))
    boxes = _boxes(ww, wh)
    m = small.model(score, block)
    cp = _pull(built, [small.dec], [(0,) + b for b in boxes], 64, score=score, block=block, nms=nms)
    assert cp.got == [1] * len(boxes) and cp.current == [1]
    _check(cp, [m.record(b, nms, 64) for b in boxes], (score, block, nms))
    assert m.record(boxes[5], nms, 64) == bytes(cm.record_bytes(64))
    whole = m.points(boxes[0], nms)
    assert whole[1] > 0 and (len(whole[2]) > 64) == (nms == 1)
    # ... and through the views
    k = 2
    count, energy, pts = m.points(boxes[k], nms)
    n = min(len(pts), 64)
    assert (int(cp.count[k]), int(cp.found[k]), int(cp.written[k]), int(cp.energy[k])) == (count, len(pts), n, energy)
    assert cp.x[k, :n].tolist() == [p[0] for p in pts[:n]] and cp.y[k, :n].tolist() == [p[1] for p in pts[:n]]
    assert cp.score[k, :n].tolist() == [p[2] for p in pts[:n]] and cp.points(k) == pts[:n]
    assert cp.x.dtype == cp.y.dtype == __import__("torch").int32 and cp.score.dtype == cp.energy.dtype == __import__("torch").int64


@pytest.mark.parametrize("score", SCORES)
def test_the_checkerboard_is_all_ties(built, score):
    """8 x 8 squares of 0 / 255: every candidate has ONE score, so the suppression, the order of the record, the cut at K and the merge
    of the bands are decided by raster position alone"""
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    c = Chosen(built, [((((x // 8) + (y // 8)) & 1) * 255).astype(np.uint8)])
    m = c.model(score, 3)
    pts = m.points((0, 0, W, H), 3)[2]
    assert len(pts) == 35 and len({p[2] for p in pts}) == 1 and pts[0][2] > 0
    for nms in (1, 3, 7):
        for K in (16, 64):                                         # 16: the cut falls among equal scores
            boxes = [(0, 0, W, H), (4, 4, 40, 30), (7, 7, 1, 1), (8, 8, 50, 40)]
            cp = _pull(built, [c.dec], [(0,) + b for b in boxes], K, score=score, nms=nms)
            _check(cp, [m.record(b, nms, K) for b in boxes], ("checkerboard", score, nms, K))
    c.close()


@pytest.mark.parametrize("score", SCORES)
def test_tiles_truncation_merge_and_tail(built, large, score):
    """144 x 80, the whole window as ONE region: five bands, each of several tiles in a row.  K = 256 at nms 1: more candidates than K,
    the best K stand; K = 16: every band brings more than the record holds; K = 256 at nms 7: fewer than K, a tail of zeros"""
    m = large.model(score, 3)
    found = {nms: len(m.points((0, 0, BW, BH), nms)[2]) for nms in (1, 7)}
    assert found[1] > 256 and 16 < found[7] < 256
    for nms, K in ((1, 256), (1, 16), (7, 256), (7, 16)):
        cp = _pull(built, [large.dec], None, K, score=score, nms=nms)
        assert cp.got == [1] and int(cp.found[0]) == found[nms] and int(cp.written[0]) == min(found[nms], K)
        _check(cp, [m.record((0, 0, BW, BH), nms, K)], ("large", score, nms, K))
    cp = _pull(built, [large.dec], None, 64, score=score, nms=3, block=5)
    _check(cp, [large.model(score, 5).record((0, 0, BW, BH), 3, 64)], ("large block 5", score))


@pytest.mark.parametrize("score", SCORES)
def test_many_small_regions_close_their_own_records(built, large, score):
    """1100 regions in one call: one band each, the workgroup closes its record without the scratch.  Boxes taller than a tile of 32 rows
    and wider than one of 64 (32 for Harris) columns among them, and boxes that leave the window"""
    regions = [(0, (7 * k) % 140 - 6, (5 * k) % 76 - 4, 9 + 13 * (k % 8), 6 + 17 * (k % 5)) for k in range(1100)]
    assert max(r[3] for r in regions) > 64 and max(r[4] for r in regions) > 32
    m = large.model(score, 3)
    cp = _pull(built, [large.dec], regions, 32, score=score, nms=3)
    assert cp.got == [1] * len(regions)
    seen = {}
    wants = [seen.setdefault(r, m.record(r[1:], 3, 32)) if r not in seen else seen[r] for r in regions]
    _check(cp, wants, ("many", score))
    assert any(np.frombuffer(w, "<u4")[1] > 32 for w in wants) and any(np.frombuffer(w, "<u4")[0] == 0 or np.frombuffer(w, "<u4")[1] == 0 for w in wants)


@pytest.mark.parametrize("score", SCORES)
def test_min_score_is_strict(built, large, score):
    m = large.model(score, 3)
    pts = m.points((0, 0, BW, BH), 3)[2]
    values = sorted({p[2] for p in pts}, reverse=True)
    assert len(values) > 8
    between = (values[4] + values[5]) // 2                        # between two candidate scores
    assert values[5] <= between < values[4]
    for min_score, n in ((between, sum(p[2] > between for p in pts)), (values[0], 0), (values[0] - 1, sum(p[2] == values[0] for p in pts))):
        want = m.record((0, 0, BW, BH), 3, 64, min_score)
        # raising min_score only removes candidates whose score it reaches: those that remain were maxima before
        assert np.frombuffer(want, "<u4")[1] == n
        cp = _pull(built, [large.dec], None, 64, score=score, nms=3, min_score=min_score)
        _check(cp, [want], ("min_score", score, min_score))


def test_two_sizes_in_one_call_and_a_decoder_without_a_picture(built, small, large):
    """regions of a 64 x 48 and a 144 x 80 instance interleaved, and of one that has decoded nothing: got = 0 there and the record is
    still the fill"""
    idle = built.Decoder(1)
    decs = [small.dec, idle, large.dec]
    sw, sh = small.window[2:]
    regions = [(0, 0, 0, sw, sh), (2, 0, 0, BW, BH), (1, 0, 0, 16, 16), (2, 100, 50, 60, 40), (0, -3, 20, 30, 40), (1, 5, 5, 8, 8), (2, 64, 32, 1, 1)]
    for score in SCORES:
        cp = _pull(built, decs, regions, 48, score=score, nms=2, block=5)
        assert cp.got == [1, 1, 0, 1, 1, 0, 1] and cp.current == [1, 0, 1]
        host = cp.records.cpu().numpy()
        for k, r in enumerate(regions):
            if r[0] == 1:
                assert (host[k] == FILL).all()
            else:
                _same(cp, host, k, (small if r[0] == 0 else large).model(score, 5).record(r[1:], 2, 48), (score, r))
    whole = _pull(built, decs, None, 8)                            # whole windows: one record per decoder
    assert whole.got == [1, 0, 1] and bool((whole.records[1] == FILL).all())
    host = whole.records.cpu().numpy()
    _same(whole, host, 0, small.model(cm.MIN_EIGEN, 3).record((0, 0, sw, sh), 3, 8), "whole windows")
    _same(whole, host, 2, large.model(cm.MIN_EIGEN, 3).record((0, 0, BW, BH), 3, 8), "whole windows")
    idle.close()


@pytest.mark.parametrize("score", SCORES)
def test_points_of_boxes_are_the_windows_points_in_the_boxes(built, large, score):
    """candidates(box) = candidates(window) ∩ box, on the device alone: K is large enough to hold them all"""
    rng = np.random.default_rng(17)
    boxes = [(int(rng.integers(-10, BW - 4)), int(rng.integers(-10, BH - 4)), int(rng.integers(1, 90)), int(rng.integers(1, 60))) for _ in range(24)]
    whole = _pull(built, [large.dec], None, 256, score=score, nms=4)
    assert int(whole.found[0]) <= 256
    every = whole.points(0)
    cp = _pull(built, [large.dec], [(0,) + b for b in boxes], 256, score=score, nms=4)
    for k, (x, y, w, h) in enumerate(boxes):
        assert cp.points(k) == [p for p in every if x <= p[0] < x + w and y <= p[1] < y + h], (k, boxes[k])
        assert int(cp.found[k]) == int(cp.written[k]) == len(cp.points(k))


def test_back_to_back_calls_share_the_scratch(built, large):
    """two banded calls on one stream without a wait between them, then a third: each must find the tickets zero and wait for the scratch"""
    import torch
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        first = _pull(built, [large.dec], None, 64, score=cm.HARRIS, nms=2, stream=st)
        second = _pull(built, [large.dec], None, 32, score=cm.MIN_EIGEN, nms=5, stream=st)
        third = _pull(built, [large.dec], [(0, 0, 0, BW, BH), (0, 10, 10, 50, 60)], 16, nms=1, stream=st)
    st.synchronize()
    _check(first, [large.model(cm.HARRIS, 3).record((0, 0, BW, BH), 2, 64)], "first")
    _check(second, [large.model(cm.MIN_EIGEN, 3).record((0, 0, BW, BH), 5, 32)], "second")
    _check(third, [large.model(cm.MIN_EIGEN, 3).record(b, 1, 16) for b in ((0, 0, BW, BH), (10, 10, 50, 60))], "third")


def test_corner_regions_feed_the_region_shift(built):
    """the loop the feature closes: points of picture 0, boxes of 9 x 9 around them, the picture kept, and on picture 1 — picture 0 moved
    by (3, -2) — pull_shift on those boxes answers (3, -2) alone, for every point.  The points are asked for in a box whose margin is
    half a side plus the radius, so every box lies inside the window with the search's reach to spare; that the definition answers so
    for this picture is asserted on the model first"""
    SIDE, RADIUS = 9, 4
    margin = SIDE // 2 + RADIUS
    Y = np.random.default_rng(23).integers(0, 256, (H, W), dtype=np.uint8)
    moved = Y[np.clip(np.arange(H) - SHIFT[1], 0, H - 1)[:, None], np.clip(np.arange(W) - SHIFT[0], 0, W - 1)[None, :]]
    c = Chosen(built, [Y, moved])
    asked = [(0, margin, margin, W - 2 * margin, H - 2 * margin)]
    cp = _pull(built, [c.dec], asked, 24, nms=5)
    _check(cp, [c.model(cm.MIN_EIGEN, 3).record(asked[0][1:], 5, 24)], "points")
    boxes = cp.regions(SIDE, asked)
    pts = cp.points(0)
    assert len(boxes) == int(cp.written[0]) >= 8
    assert boxes == [(0, p[0] - SIDE // 2, p[1] - SIDE // 2, SIDE, SIDE) for p in pts]
    assert all(b[1] >= RADIUS and b[2] >= RADIUS and b[1] + SIDE + RADIUS <= W and b[2] + SIDE + RADIUS <= H for b in boxes)
    for b in boxes:
        want = shm.record(Y, moved, (0, 0, W, H), b[1:], RADIUS)
        assert (want.dx, want.dy, want.best, want.ties) == (SHIFT[0], SHIFT[1], 0, 1), b
    assert built.keep_pictures([c.dec])[0] == [1]
    c.next()
    sh = built.pull_shift([c.dec], boxes, radius=RADIUS)
    assert sh.got == [1] * len(boxes)
    assert sh.dx.tolist() == [SHIFT[0]] * len(boxes) and sh.dy.tolist() == [SHIFT[1]] * len(boxes) and sh.ties.tolist() == [1] * len(boxes)
    assert sh.moved(boxes) == [(0, b[1] + SHIFT[0], b[2] + SHIFT[1], SIDE, SIDE) for b in boxes]
    st = built.pull_stats([c.dec], boxes, source="y", bins=0)    # and the statistics take them as well
    assert st.got == [1] * len(boxes)
    with pytest.raises(ValueError):
        cp.regions(SIDE, None)
    with pytest.raises(ValueError):
        cp.regions(SIDE, asked * 2)
    with pytest.raises(ValueError):
        cp.regions(0, asked)
    c.close()


def test_raw_calls_that_must_be_refused_write_nothing(built, small):
    import torch
    L = built.api_lib()
    stride = built.corners_record_bytes(8)
    out = torch.full((2, stride + 8), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    S = 0xA5A5A5A5
    good = dict(data=out.data_ptr(), score=0, block=3, nms=3, max_points=8, crop=1, zero=0, min_score=0)

    def call(decs, regs, **kw):
        f = dict(good)
        f.update(kw)
        spec = built.CornersSpec(*[f[k[0]] for k in built.CornersSpec._fields_])
        arrays = [(ctypes.c_uint32 * 2)(S, S) for _ in range(3)]
        regions = (built.Region * 2)(*[built.Region(*r) for r in regs])
        rc = L.h264bsdmiOutputCornerPoints(len(decs), (ctypes.c_void_p * len(decs))(*decs), 2, regions, ctypes.byref(spec), None, *arrays)
        return rc, [list(a) for a in arrays]

    regs = [(0, 0, 0, 16, 16), (0, 10, 10, 8, 8)]
    untouched = (-1, [[S, S]] * 3)
    d = small.dec._st
    assert call([d, d], regs) == untouched                               # repeated instances
    for bad in (dict(score=2), dict(block=4), dict(nms=0), dict(nms=8), dict(max_points=0), dict(max_points=257), dict(crop=2), dict(zero=1),
                dict(score=1, min_score=2 ** 63), dict(data=out.data_ptr() + 4)):
        assert call([d], regs, **bad) == untouched, bad
    assert call([d], [regs[0], (0, 0, 0, 0, 8)]) == untouched
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    rc, arrays = call([d], regs)
    assert rc == 0 and arrays == [[1, 1], [1, S], [arrays[2][0], S]]
    torch.cuda.synchronize()
    assert bool((out.view(-1)[2 * stride:] == FILL).all())
    m = small.model(cm.MIN_EIGEN, 3)
    host = out.view(-1)[:2 * stride].view(2, stride).cpu().numpy()
    for k, r in enumerate(regs):
        _same(None, host, k, m.record(r[1:], 3, 8), ("raw", r))
