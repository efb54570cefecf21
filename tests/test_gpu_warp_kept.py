"""GPU: warped kept pictures — h264bsdmiWarpKeptPictures / warp_kept — through the product library.  The pictures are chosen
(tests/pcm_pictures.py), so every current picture is known exactly; the state is read back with pull_kept(fraction=True) and every
comparison is an equality with tests/warp_model.py, byte for byte.  A workgroup of the kernel owns a block of 64 x 16 luma samples and
gathers the source samples from the tiles; a variant that staged a block's source box in LDS when it was at most 96 x 40 samples was
measured slower and is not shipped.  The transforms stay on both sides of that rule and at its edge all the same (a horizontal scale of
1.5 gives boxes of exactly 96 columns, 1.5 + 1/64 of 97; a vertical scale of 2.55 gives 40 rows in the first row of blocks and 41
further down): they are what a second path would have to agree on.  The 208 x 112 pictures have several blocks each way, the last one
of a row half empty."""
import ctypes
import math

import numpy as np
import pytest

import background_model as bm
import cells_model as clm
import corners_model as cm
import matches_model as mm
import model_fit_model as fm
import pcm_pictures as pp
import stats_model as sm
import warp_model as wm
from test_gpu_background import Scene, _random_pictures, _same_state
from test_gpu_region_shift import _picture, _shifted
from test_gpu_tensor_colour import Feed

pytestmark = pytest.mark.gpu

ONE = wm.ONE
SIZES = {"16x16": (16, 16, None), "80x48": (80, 48, None), "48x32-cropped": (48, 32, (1, 2, 2, 1)), "208x112": (208, 112, None)}
MODES = {"replicate": wm.REPLICATE, "current": wm.CURRENT}


@pytest.fixture(autouse=True, scope="module")
def _through_the_product_library(built):
    built.use_product_library(True)
    yield
    built.use_product_library(False)


@pytest.fixture(autouse=True)
def _no_device_errors(built):
    yield
    assert built.device_errors() == 0


def _about_the_centre(w, h, lin, shift=(0.0, 0.0)):
    """the map output -> source with the linear part lin = (a, b, d, e) as floats that keeps the window's centre, then moves by shift"""
    a, b, d, e = lin
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    return tuple(int(round(v * ONE)) for v in (a, b, cx - a * cx - b * cy + shift[0], d, e, cy - d * cx - e * cy + shift[1]))


def _turned(w, h, degrees, scale, shift):
    c, s = scale * math.cos(math.radians(degrees)), scale * math.sin(math.radians(degrees))
    return _about_the_centre(w, h, (c, -s, s, c), shift)


def transforms(w, h):
    """name -> a b c d e f for a window w x h: small and large source boxes of a block, and the edge of the rule above"""
    return {
        "identity": wm.IDENTITY,
        "shift +3 -2": wm.translation(3, -2), "shift -4 +6": wm.translation(-4, 6), "shift +1 +1": wm.translation(1, 1),
        "half +x +y": wm.translation(0.5, 0.5), "half -x": wm.translation(-0.5, 0), "half -y": wm.translation(0, -0.5), "half +1.5 -2.5": wm.translation(1.5, -2.5),
        "odd fraction": wm.translation(-2.30078125, 1.7109375),
        "turn +3 x0.97": _turned(w, h, 3, 0.97, (2.25, -1.5)), "turn -3 x1.03": _turned(w, h, -3, 1.03, (-3.125, 0.75)),
        "quarter turn": (0, ONE, 0, -ONE, 0, (h - 1) << 16), "quarter turn back": (0, -ONE, (w - 1) << 16, ONE, 0, 0),
        "half turn": wm.half_turn(w, h),
        "zoom x4": _about_the_centre(w, h, (0.25, 0, 0, 0.25)), "zoom x1/4": _about_the_centre(w, h, (4, 0, 0, 4)),
        "shear": _about_the_centre(w, h, (1, 0.25, -0.125, 1)),
        "edge 96 columns": (3 * ONE // 2, 0, 0, 0, ONE, 0), "edge 97 columns": (3 * ONE // 2 + ONE // 64, 0, 0, 0, ONE, 0),
        "edge 40 rows": (ONE, 0, 0, 0, 167117, 0), "edge 41 rows": (ONE, 0, 0, 0, 170394, 0),        # 2.55 and 2.6
        "far away": wm.translation(3 * w, -2 * h), "largest": (wm.MAX_COEFFICIENT, -wm.MAX_COEFFICIENT, 2 ** 31 - 1, wm.MAX_COEFFICIENT, wm.MAX_COEFFICIENT, -2 ** 31),
    }


class WarpScene(Scene):
    """test_gpu_background's decoder over chosen pictures, with the model that knows the warp; warp(): the call on the decoder and on
    the model, their answers compared"""

    def __init__(self, built, pictures, crop=None):
        super().__init__(built, pictures, crop)
        self.model = wm.Background(self.W, self.H)
        self.kept_id = 0

    def blend(self, stream=None, **kw):
        self.kept_id = 100 + self.t
        return super().blend(stream, **kw)

    def keep(self):
        self.kept_id = 100 + self.t
        super().keep()

    def warp(self, coef, outside="replicate", crop=True, stream=None, current=True):
        window = self.window if crop else (0, 0, self.W, self.H)
        want = self.model.warp(coef, MODES[outside], window, self.frame if current else None)
        warped, ids, counts = self.built.warp_kept([self.dec], coefficients=[coef], outside=outside, crop=crop, count_outside=True, stream=stream)
        if stream is not None:
            stream.synchronize()
        assert (warped, ids) == ([want[0]], [self.kept_id]), (warped, ids, want)
        assert counts.dtype.is_floating_point is False and counts.cpu().tolist() == [want[1]], (counts.cpu().tolist(), want, coef, outside)
        return want


def _checkerboard(W, H):
    x, y = np.arange(W)[None, :], np.arange(H)[:, None]
    board = lambda xs, ys: (((xs + ys) & 1) * 255).astype(np.uint8)
    return (board(x, y), board(x[:, :W // 2], y[:H // 2]), 255 - board(x[:, :W // 2], y[:H // 2]))


@pytest.mark.parametrize("state", ["kept", "blended", "saturated"])
@pytest.mark.parametrize("size", list(SIZES))
def test_every_transform_equals_the_model_byte_for_byte(built, size, state):
    """kept: after a plain keep — lo is not valid, reads as 128, is not written and stays 0x80; blended: after three blends — lo valid
    and busy; both go through all the transforms one after the other, each on what the last one left, the outside mode alternating.
    saturated: hi 255 beside 0 in a checkerboard on all three planes, kept again before every transform"""
    W, H, crop = SIZES[size]
    if state == "saturated":
        sc = WarpScene(built, [_checkerboard(W, H)], crop=crop)
        sc.next()
    else:
        sc = WarpScene(built, _random_pictures(W, H, 4, seed=W + len(state)), crop=crop)
        for _ in range(3 if state == "blended" else 1):
            sc.next()
            sc.blend(shift=2) if state == "blended" else sc.keep()
        sc.next()
    w, h = sc.window[2:]
    assert state != "blended" or (sc.model.lo_valid and (sc.model.lo != 0x80).any())
    for k, (name, coef) in enumerate(transforms(w, h).items()):
        for outside in (("replicate", "current") if state == "saturated" else (("replicate", "current")[k & 1],)):
            if state == "saturated":
                sc.keep()
            want = sc.warp(coef, outside)
            assert want[0] == 1 and (want[1] == w * h) == (name in ("far away", "largest")) and (want[1] > 0 or "turn" in name or name in ("identity", "zoom x4"))
            sc.check((size, state, name, outside))
    assert sc.model.lo_valid == (state == "blended") and (state == "blended" or (sc.model.lo == 0x80).all())
    sc.close()


def test_the_coded_frame_as_the_window_of_a_cropped_stream(built):
    """crop=False: the window is the coded frame, the map is in its samples"""
    W, H, crop = SIZES["48x32-cropped"]
    sc = WarpScene(built, _random_pictures(W, H, 3, seed=5), crop=crop)
    for _ in range(2):
        sc.next()
        sc.blend(shift=1)
    for coef, outside in ((wm.translation(2.5, -1.25), "replicate"), (_turned(W, H, 5, 1.0, (0, 0)), "current")):
        sc.warp(coef, outside, crop=False)
        sc.check(("coded frame", outside))
    sc.close()


def test_warps_blends_and_keeps_in_sequence(built):
    """warp, warp; warp, blend, warp; warp, keep, warp: the spare buffers change places with the live ones each time, and a blend and
    a keep write the live ones"""
    W, H = 80, 48
    sc = WarpScene(built, _random_pictures(W, H, 6, seed=71))
    sc.next()
    sc.blend(shift=2)
    t = transforms(W, H)
    for step in ("warp", "warp", "blend", "warp", "warp", "blend", "blend", "warp", "keep", "warp", "blend", "warp"):
        if step == "warp":
            sc.warp(t["turn +3 x0.97"], "current")
        else:
            sc.next()
            sc.blend(shift=3, hold=40, moving_shift=1) if step == "blend" else sc.keep()
        sc.check(step)
    sc.close()


def test_a_batch_of_three_sizes_with_different_maps(built):
    """one launch for decoders of 16 x 16, 80 x 48 and 48 x 32 (cropped).  A NaN row of theta leaves its decoder out; a decoder without a
    kept picture and, under "current", one without a current picture are left alone and report 0"""
    scenes = [WarpScene(built, _random_pictures(W, H, 4, seed=80 + W), crop=crop) for W, H, crop in (SIZES["16x16"], SIZES["80x48"], SIZES["48x32-cropped"])]
    a, b, c = scenes
    decs = [s.dec for s in scenes]
    for s in (a, c):
        for _ in range(2):
            s.next()
            s.blend(shift=2)
    b.next()                                                    # a current picture, nothing kept
    nan = float("nan")
    theta = np.array([[[nan] * 3] * 2, [[1, 0, 2], [0, 1, 1]], [[0.98, -0.05, 1.5], [0.05, 0.98, -2.25]]])
    rows = built.warp_coefficients(theta)
    assert rows[0] is None and rows[1].tolist() == [ONE, 0, -2 * ONE, 0, ONE, -ONE]
    want_c = c.model.warp(rows[2], wm.REPLICATE, c.window, c.frame)
    warped, ids, counts = built.warp_kept(decs, theta=theta, count_outside=True)
    assert (warped, ids) == ([0, 0, 1], [0, 0, 101]) and counts.cpu().tolist() == [0, 0, want_c[1]] and want_c[1] > 0
    assert built.pull_kept([b.dec]) == [None]
    for s in (a, c):
        s.check("first call")
    b.keep()
    a.decode()                                                  # decoded, not popped: no current picture
    maps = [wm.translation(0.5, -0.5), _turned(80, 48, -2, 1.01, (1, 1)), wm.half_turn(*c.window[2:])]
    want = [s.model.warp(m, wm.CURRENT, s.window, None if s is a else s.frame) for s, m in zip(scenes, maps)]
    warped, ids, counts = built.warp_kept(decs, coefficients=np.array(maps, np.int32), outside="current", count_outside=True)
    assert (warped, ids) == ([0, 1, 1], [101, 100, 101]) and want[0] == (0, 0) and counts.cpu().tolist() == [0, want[1][1], want[2][1]]
    want = [s.model.warp(m, wm.REPLICATE, s.window, None) for s, m in zip(scenes, maps)]
    assert built.warp_kept(decs, coefficients=[np.array(m) for m in maps]) == ([1, 1, 1], [101, 100, 101])        # no current picture is needed
    for s in scenes:
        s.check("batch")
    assert built.warp_kept([], coefficients=[]) == ([], []) and built.warp_kept(decs, coefficients=[None] * 3) == ([0, 0, 0], [0, 0, 0])
    with pytest.raises(ValueError, match="warp_kept"):
        built.warp_kept([a.dec, a.dec], coefficients=[wm.IDENTITY] * 2)
    for s in scenes:
        s.check("after the refusals")
        s.close()


def test_a_warp_on_a_side_stream_then_a_comparison_on_another(built):
    """the ordering of launches that touch kept pictures: pull_change on a second stream reads the warped picture, the readback on a
    third the same bytes"""
    import torch
    import change_model as chm
    from test_gpu_region_change import _equal
    W, H = 208, 112
    sc = WarpScene(built, _random_pictures(W, H, 3, seed=91))
    s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    sc.next()
    sc.blend(stream=s1, shift=2)
    cur = sc.next()
    records = []
    for name in ("turn -3 x1.03", "quarter turn", "half +x +y"):
        sc.warp(transforms(W, H)[name], "replicate", stream=s1)
        want = chm.record(sm.channels(cur, W, H, "y"), sm.channels(sc.model.hi, W, H, "y"), (0, 0, W, H), (0, 0, W, H), 0, (4, 0, 0))
        records.append((built.pull_change([sc.dec], None, source="y", threshold=4, stream=s2), want))
    sc.check("streams", stream=s3)
    torch.cuda.synchronize()
    for ch, want in records:
        _equal(ch, 0, want)
    sc.close()


def test_the_consumers_see_a_moved_camera_taken_out(built):
    """the next picture is the kept one moved by a whole (even) number of samples, new content at the borders: against the kept
    picture as it lies everything changed; after warp_kept(outside="current") nothing did"""
    W, H, move = 80, 48, (4, -2)
    kept = _random_pictures(W, H, 1, seed=95)[0]
    fresh = _random_pictures(W, H, 1, seed=96)[0]
    cur = []
    for q, (k, f) in enumerate(zip(kept, fresh)):
        d = 1 if q == 0 else 2
        p = f.copy()
        hh, ww = k.shape
        ys, xs = np.mgrid[0:hh, 0:ww]
        sy, sx = ys - move[1] // d, xs - move[0] // d           # the content moves by `move`
        ok = (sy >= 0) & (sy < hh) & (sx >= 0) & (sx < ww)
        p[ok] = k[sy[ok], sx[ok]]
        cur.append(p)
    sc = WarpScene(built, [kept, tuple(cur)])
    sc.next()
    sc.keep()
    sc.next()
    names = ("sad", "above")
    before = built.pull_change([sc.dec], None, source="ycbcr")
    cells = built.pull_cells([sc.dec], None, cell=8, grid=(6, 10), source="ycbcr", planes=names, against="kept")
    assert (before.sad[0].cpu().numpy() > 0).all() and (cells.maps[0].cpu().numpy() != 0).any()
    coef = built.warp_coefficients(np.array([[[1, 0, move[0]], [0, 1, move[1]]]], np.float64))[0]
    assert coef.tolist() == list(wm.translation(-move[0], -move[1]))
    want = sc.warp(coef, "current")
    assert want[1] == W * H - (W - abs(move[0])) * (H - abs(move[1]))
    sc.check("moved")
    assert np.array_equal(sc.model.hi, sc.frame)
    after = built.pull_change([sc.dec], None, source="ycbcr")
    cells = built.pull_cells([sc.dec], None, cell=8, grid=(6, 10), source="ycbcr", planes=names, against="kept")
    assert after.kept_pic_id == [100] and (after.sad[0].cpu().numpy() == 0).all() and (cells.maps[0].cpu().numpy() == 0).all()
    sc.close()


def test_corners_matches_model_and_warp_chained_leave_only_what_moved(built):
    """a textured picture and its copy moved by (5, -3) with a bright square pasted in.  On the MODELS alone, before the device is
    asked: 35 usable pairs, all of them inliers of the translation fit at tolerance 0 and every one moved by exactly (5, -3).  So
    warp_coefficients(theta) is that translation, the warped background equals the current picture outside the square, and pull_boxes
    finds the square and nothing else"""
    W, H, K, move = 64, 48, 64, (5, -3)
    kept = np.random.default_rng(1).integers(0, 256, (H, W), dtype=np.uint8)
    cur = _shifted(kept, *move).copy()
    cur[16:24, 32:40] = 255
    box = (0, 0, W, H)
    kp, cp = cm.Window(kept).record(box, 3, K), cm.Window(cur).record(box, 3, K)
    wt = fm.Record(fm.record(mm.record_fast(kept, cur, box, box, kp, cp, K), kp, cp, K, model=fm.TRANSLATION, tolerance=0), K)
    assert (wt.usable, wt.inliers, wt.found) == (35, 35, 1)
    assert (wt.sums[2] - wt.sums[0], wt.sums[3] - wt.sums[1]) == (move[0] * wt.inliers, move[1] * wt.inliers)

    feed = Feed(built, pp.pcm_stream([_picture(kept), _picture(cur)]))
    assert feed.step() and feed.dec.next_output_info() is not None
    c0 = built.pull_corners([feed.dec], max_points=K)
    assert built.keep_pictures([feed.dec])[0] == [1]
    assert feed.step() and feed.dec.next_output_info() is not None
    c1 = built.pull_corners([feed.dec], max_points=K)
    g = built.pull_model([feed.dec], built.pull_matches([feed.dec], c0, c1), c0, c1, model="translation", tolerance=0)
    theta = g.theta("translation")
    rows = built.warp_coefficients(theta)
    assert rows[0].tolist() == [ONE, 0, -move[0] * ONE, 0, ONE, -move[1] * ONE]
    unregistered = built.pull_boxes([feed.dec], None, cell=8, grid=(6, 8))
    assert unregistered.cells.maps[0].cpu().numpy().astype(bool).sum() > 40                 # nearly every cell changed
    model = wm.Background(W, H)
    model.keep(pp.i420(_picture(kept)))
    want = model.warp(rows[0], wm.CURRENT, box, pp.i420(_picture(cur)))
    warped, ids, counts = built.warp_kept([feed.dec], theta=theta, outside="current", count_outside=True)
    assert (warped, counts.cpu().tolist()) == ([1], [want[1]]) and ids == built.pull_change([feed.dec], None).kept_pic_id
    hi, lo = built.pull_kept([feed.dec], fraction=True)[0]
    _same_state(hi, lo, model, "chain")
    changed = model.hi[:W * H].reshape(H, W) != cur
    assert changed[16:24, 32:40].any() and not changed[:16].any() and not changed[24:].any() and not changed[:, :32].any() and not changed[:, 40:].any()
    boxes = built.pull_boxes([feed.dec], None, cell=8, grid=(6, 8))
    assert boxes.found == [1] and boxes.regions() == [(0, 32, 16, 8, 8)]
    feed.close()
