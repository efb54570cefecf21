"""GPU: the background spread — h264bsdmiBlendCurrentPicturesSpread / blend_pictures(spread=...), h264bsdmiOutputKeptSpread /
pull_kept(spread=True) and the SPREAD mode of the cell maps and cell boxes / pull_cells, pull_boxes(against="spread") — through the
product library.  The pictures are chosen (tests/pcm_pictures.py), so every current picture is known exactly; the state is read back
with pull_kept(fraction=True, spread=True) and every comparison is an equality with tests/spread_model.py, whose arithmetic
tests/test_spread_model_cpu.py pins without a GPU."""
import numpy as np
import pytest

import background_model as bm
import boxes_model as bxm
import cells_model as clm
import pcm_pictures as pp
import spread_model as spm
import stats_model as sm
import warp_model as wm
from test_gpu_background import SIZES, Scene, _model_shift, _random_pictures
from test_gpu_cell_maps import Pair, _cropped

pytestmark = pytest.mark.gpu

S32 = 0x5A5A5A5A
SPREAD_PLANES = ("count", "fore", "excess", "spread")


@pytest.fixture(autouse=True, scope="module")
def _through_the_product_library(built):
    built.use_product_library(True)
    yield
    built.use_product_library(False)


@pytest.fixture(autouse=True)
def _no_device_errors(built):
    yield
    assert built.device_errors() == 0


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:6].ravel(), got[got != want][:6], want[got != want][:6])


class SpreadScene(Scene):
    """test_gpu_background's decoder over chosen pictures with the model that knows the spread.  spread(): the new call on the decoder
    and on the model, their answers compared; check(): hi, lo and V read back (V: None exactly where the model's is not valid)"""

    def __init__(self, built, pictures, crop=None):
        super().__init__(built, pictures, crop)
        self.model = spm.Spread(self.W, self.H)

    def spread(self, spec, stream=None, **kw):
        want = self.model.blend_spread(self.frame, kw.get("shift", 4), kw.get("hold", 255), _model_shift(kw.get("moving_shift")), **spec)
        kept, blended, ids, moving = self.built.blend_pictures([self.dec], count_moving=True, stream=stream, spread=spec, **kw)
        if stream is not None:
            stream.synchronize()
        assert (kept, blended, ids) == ([1], [want[0]], [100 + self.t])
        assert moving.cpu().tolist() == [want[1]], (moving.cpu().tolist(), want, kw, spec)
        return want

    def check(self, what=None, stream=None):
        hi, lo, V = self.built.pull_kept([self.dec], fraction=True, spread=True, stream=stream)[0]
        if stream is not None:
            stream.synchronize()
        _same(hi, self.model.hi, (what, "hi"))
        _same(lo, self.model.lo, (what, "lo"))
        assert (V is None) == (self.model.V is None), what
        if V is not None:
            _same(V, self.model.V, (what, "V"))


def _noisy_pictures(W, H, count, seed, amplitudes=(2, 9, 30)):
    """a base picture and `count` pictures around it whose noise grows from the left third to the right one, in all three planes:
    the spread gets different values in different places"""
    rng = np.random.default_rng(seed)
    base = _random_pictures(W, H, 1, seed=seed + 1)[0]
    out = []
    for _ in range(count):
        pic = []
        for p in base:
            h, w = p.shape
            amp = np.asarray(amplitudes)[np.minimum(np.arange(w) * 3 // w, 2)][None, :]
            pic.append(np.clip(p.astype(np.int64) + rng.integers(-1, 2, (h, w)) * rng.integers(0, 2, (h, w)) * amp, 0, 255).astype(np.uint8))
        out.append(tuple(pic))
    return out


@pytest.mark.parametrize("update", ["all", "still", "none"])
@pytest.mark.parametrize("size", list(SIZES))
def test_six_random_pictures_blend_as_the_model_does(built, size, update):
    """one macroblock (16 live lanes), 15 macroblocks (a workgroup step that is not full), a cropped stream; gain 1, 2 and 8 with
    moving_shift 0, 3 and frozen; the first call starts the model: blended = 0, V = lowest, nothing is moving"""
    W, H, crop = SIZES[size]
    for gain in (1, 2, 8):
        for moving_shift in (0, 3, "frozen"):
            spec = dict(gain=gain, lowest=gain, highest=255 if gain != 2 else 6, update=update)
            pictures = _random_pictures(W, H, 6, seed=W + gain) if gain != 2 else _noisy_pictures(W, H, 6, seed=W + gain)
            sc = SpreadScene(built, pictures, crop=crop)
            assert built.pull_kept([sc.dec], fraction=True, spread=True) == [None]
            moving = 0
            for t in range(6):
                sc.next()
                blended, count = sc.spread(spec, shift=3, hold=4 * gain, moving_shift=moving_shift)
                assert blended == (1 if t else 0)
                moving += count
                sc.check((size, update, gain, moving_shift, t))
                if t == 0:
                    assert (sc.model.V == gain).all() and count == 0
            assert moving > 0
            assert update == "still" or (update == "none") == bool((sc.model.V == gain).all())
            sc.close()


def test_the_saturated_pair_climbs_one_step_a_call_to_255(built):
    """black and white alternating with shift 0: hi is the picture before, d = 255 at every call, A = 255 at gain 8, so V is t after
    call t; every luma sample is moving while V < 255, none from then on, and mode 2 then finds no foreground at all"""
    W = H = 16
    calls = 256
    sc = SpreadScene(built, [pp.flat(W, H, v, v, v) for v in [0] + [255 if t & 1 else 0 for t in range(1, calls + 1)]])
    spec = dict(gain=8, lowest=0, highest=255, update="all")
    sc.next()
    sc.spread(spec, shift=0, hold=0)
    for t in range(1, calls + 1):
        sc.next()
        if t in (100, 256):                              # the current picture against the state of call t - 1: d = 255, V = t - 1
            cells = built.pull_cells([sc.dec], None, cell=4, source="ycbcr", planes=SPREAD_PLANES, against="spread")
            assert cells.got == [1] and int(cells.count.sum()) == W * H
            assert int(cells.fore.sum()) == (3 * W * H if t == 100 else 0) and int(cells.excess.sum()) == 3 * W * H * (256 - t)
            assert int(cells.spread.sum()) == 3 * W * H * (t - 1)
        _, moving = sc.spread(spec, shift=0, hold=0)
        assert moving == (W * H if t <= 255 else 0) and (sc.model.V == min(t, 255)).all()
        if t % 64 == 0 or t >= 254:
            sc.check(t)
    sc.close()


@pytest.mark.parametrize("moving_shift", [None, 0, "frozen"])
def test_with_lowest_and_highest_zero_it_is_the_plain_blend_of_a_twin(built, moving_shift):
    """two decoders over the same stream, one with blend_pictures(spread=dict(lowest=0, highest=0)), one with plain blend_pictures:
    identical hi, lo and moving counts, whatever gain and update say"""
    W, H = 80, 48
    pictures = _noisy_pictures(W, H, 5, seed=5)
    a, b = SpreadScene(built, pictures), Scene(built, pictures)
    for t in range(5):
        a.next(), b.next()
        kw = dict(shift=2, hold=(0, 3, 9, 40, 255)[t], moving_shift=moving_shift)
        assert a.spread(dict(gain=1 + t, lowest=0, highest=0, update=spm.UPDATES[t % 3]), **kw) == b.blend(**kw)
        ga, gb = built.pull_kept([a.dec], fraction=True, spread=True)[0], built.pull_kept([b.dec], fraction=True, spread=True)[0]
        assert gb[2] is None and not bool(ga[2].any())
        for x, y in zip(ga[:2], gb[:2]):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())
        a.check(t), b.check(t)
    a.close(), b.close()


@pytest.mark.parametrize("how", ["keep_pictures", "pull_change", "pull_cells"])
def test_a_plain_keep_between_two_spread_blends_invalidates_the_spread(built, how):
    """after it pull_kept(spread=True) gives None for the spread, pull_cells(against="spread") got = 0 and an untouched slice, and the
    next spread blend reads V as its `lowest`; a plain blend in between leaves V as it is"""
    import torch
    W, H = 80, 48
    sc = SpreadScene(built, _noisy_pictures(W, H, 7, seed=21))
    spec = dict(gain=4, lowest=1, highest=255, update="all")
    for _ in range(3):
        sc.next()
        sc.spread(spec, shift=3, hold=2)
    assert len(np.unique(sc.model.V)) > 2
    sc.next()
    before = sc.model.V.copy()
    sc.blend(shift=3)                                        # Scene.blend: the plain call on both
    sc.check("a plain blend")
    assert np.array_equal(sc.model.V, before)
    sc.next()
    if how == "keep_pictures":
        sc.keep()
    elif how == "pull_change":
        ch = built.pull_change([sc.dec], None, source="y", keep=True)
        assert ch.got == [1]
        sc.model.keep(sc.frame)
    else:
        cm = built.pull_cells([sc.dec], None, cell=16, planes=("sad",), against="kept", keep=True)
        assert cm.got == [1]
        sc.model.keep(sc.frame)
    sc.check(how)
    hi, lo, V = built.pull_kept([sc.dec], fraction=True, spread=True)[0]
    assert V is None and sc.model.V is None and bool((lo == 0x80).all())
    assert len(built.pull_kept([sc.dec], spread=True)[0]) == 2 and built.pull_kept([sc.dec], spread=True)[0][1] is None
    sc.next()
    out = torch.full((1, 2, 3, 5), S32, dtype=torch.int32, device="cuda")
    cells = built.pull_cells([sc.dec], None, cell=16, planes=("count", "fore"), against="spread", out=out)
    torch.cuda.synchronize()
    assert cells.got == [0] and cells.current == [1] and cells.kept == [1] and bool((out == S32).all())
    spec = dict(gain=4, lowest=7, highest=255, update="still")
    assert sc.spread(spec, shift=3, hold=2)[0] == 1
    sc.check((how, "the spread blend after it"))
    assert sc.model.V.min() >= 7 and sc.model.V.max() <= 8
    sc.close()


def test_a_batch_of_three_sizes_one_of_them_never_blended_with_spread(built):
    """a decoder whose model starts in this call, one with three spread blends behind it, one that only ever saw plain blends (its
    spread is not valid: it reads as lowest), one without a current picture, one without anything"""
    spec = dict(gain=2, lowest=3, highest=200, update="all")
    nothing = built.Decoder(1)
    fresh = SpreadScene(built, _noisy_pictures(80, 48, 1, seed=41))
    going = SpreadScene(built, _noisy_pictures(16, 16, 4, seed=42))
    plain = SpreadScene(built, _noisy_pictures(48, 32, 4, seed=43), crop=SIZES["48x32-cropped"][2])
    idle = SpreadScene(built, _noisy_pictures(16, 16, 3, seed=44))
    fresh.next()
    for _ in range(3):
        going.next()
        going.spread(spec, shift=2, hold=1)
        plain.next()
        plain.blend(shift=2)
    for _ in range(2):
        idle.next()
        idle.spread(spec, shift=2, hold=1)
    going.next(), plain.next()
    idle.decode()                                            # decoded, not popped: no current picture
    decs = [nothing, fresh.dec, going.dec, plain.dec, idle.dec]
    want = [sc.model.blend_spread(sc.frame, 2, 1, 0, **spec) for sc in (fresh, going, plain)]
    kept, blended, ids, moving = built.blend_pictures(decs, shift=2, hold=1, moving_shift=0, count_moving=True, spread=spec)
    assert (kept, blended, ids) == ([0, 1, 1, 1, 0], [0, 0, 1, 1, 0], [0, 100, 103, 103, 101])
    assert moving.cpu().tolist() == [0, want[0][1], want[1][1], want[2][1], 0] and want[1][1] > 0 and want[2][1] > 0
    got = built.pull_kept(decs, fraction=True, spread=True)
    assert got[0] is None
    for sc, g in zip((fresh, going, plain, idle), got[1:]):
        for x, m, name in zip(g, (sc.model.hi, sc.model.lo, sc.model.V), ("hi", "lo", "V")):
            _same(x, m, (sc.W, sc.H, name))
    assert built.blend_pictures([], spread=spec) == ([], [], []) and built.pull_kept([], spread=True) == []
    nothing.close(), fresh.close(), going.close(), plain.close(), idle.close()


def test_calls_on_other_streams_give_the_same_bytes(built):
    """spread blends on one torch stream alternating with mode-2 maps on another (the ordering of launches that touch kept pictures),
    the readback on a third: the state and the maps are the model's, as on the default stream"""
    import torch
    W, H = 80, 48
    sc = SpreadScene(built, _noisy_pictures(W, H, 6, seed=61))
    s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    spec = dict(gain=3, lowest=1, highest=255, update="still")
    pending = []
    for t in range(6):
        cur = sc.next()
        if t:
            planes = [sm.channels(f, W, H, "ycbcr") for f in (cur, sc.model.hi, sc.model.V)]
            want = spm.maps(15, *planes, (0, 0, W, H), (0, 0, W, H), 8, (6, 10), (2, 1, 1))
            pending.append((built.pull_cells([sc.dec], None, cell=8, source="ycbcr", planes=SPREAD_PLANES, against="spread", threshold=[2, 1, 1],
                                             stream=s2), want))
        sc.spread(spec, stream=s1, shift=3, hold=2, moving_shift=1)
    sc.check("streams", stream=s3)
    torch.cuda.synchronize()
    for cells, want in pending:
        assert cells.got == [1] and np.array_equal(cells.maps[0].cpu().numpy().astype(np.int64), want)
    sc.close()


# ---- mode 2 of the cell maps

class SpreadPair(Pair):
    """test_gpu_cell_maps' decoder and twin with the spread model beside them: blend() is a spread blend of the current picture on both"""

    def __init__(self, built, *names):
        super().__init__(built, *names)
        self.model = None

    def blend(self, spec, **kw):
        if self.model is None:
            self.model = spm.Spread(*self.size())
        want = self.model.blend_spread(self.frame, kw.get("shift", 4), kw.get("hold", 255), kw.get("moving_shift"), **spec)
        assert self.built.blend_pictures([self.dec], spread=spec, **kw)[:2] == ([1], [want[0]])

    def want(self, names, source, crop, box, cell, grid, threshold=(0, 0, 0)):
        W, H = self.size()
        window = self.window(crop)
        box = (0, 0) + window[2:] if box is None else box
        planes = [sm.channels(f, W, H, source) for f in (self.frame, self.model.hi, self.model.V)]
        return spm.maps(spm.plane_bits(names), *planes, window, box, cell, grid, threshold)


@pytest.fixture(scope="module")
def cropped_pair(built):
    """the 90 x 60 window at (2, 2) of a 96 x 64 coded frame: pictures 0 and 1 blended with spread, picture 2 current.  V is lowest or
    one above after the one update the stream has room for; the threshold lies below it in one channel, in it in another, above it in
    the third"""
    built.use_product_library(True)
    pair = SpreadPair(built, _cropped())
    for _ in range(2):
        pair.advance(1)
        pair.blend(dict(gain=2, lowest=4, highest=255, update="all"), shift=1, hold=3)
    pair.advance(1)
    assert pair.window(True) == (2, 2, 90, 60) and pair.size() == (96, 64) and set(np.unique(pair.model.V)) == {4, 5}
    yield pair
    pair.close()


@pytest.mark.parametrize("source", ["y", "ycbcr"])
@pytest.mark.parametrize("cell", [4, 8, 16, 64])
def test_mode_2_on_the_cropped_synthetic_stream(built, cropped_pair, cell, source):
    """all four planes; the plain path (4, 8) and the QUAD path (16, 64); crop on and off; whole windows, a box with a negative odd
    origin that leaves the window, and a grid larger than the box"""
    pair = cropped_pair
    thr = (3, 5, 9)
    for crop in (True, False):
        size = pair.window(crop)[2:]
        rows, cols = clm.default_grid([(size[1], size[0])], cell)
        grid = (rows + 1, cols + 2)
        boxes = [(0, 0) + size, (-3, -5, 61, 41), (size[0] - 21, 7, 40, 33)]
        regions = [(0,) + b for b in boxes]
        cells = built.pull_cells([pair.dec], regions, cell=cell, grid=grid, source=source, planes=SPREAD_PLANES, against="spread",
                                 threshold=list(thr)[:1 if source == "y" else 3], crop=crop)
        assert cells.got == [1, 1, 1] and cells.kept == [1] and cells.pic_id == [pair.pic_id] and tuple(cells.maps.shape[2:]) == grid
        for k, b in enumerate(boxes):
            want = pair.want(SPREAD_PLANES, source, crop, b, cell, grid, thr)
            got = cells.maps[k].cpu().numpy().astype(np.int64)
            assert np.array_equal(got, want), (source, crop, cell, b, np.argwhere(got != want)[:4], got[got != want][:4], want[got != want][:4])
            assert want[1].any() and not want[:, -1, :].any() and not want[:, :, -1].any()     # foreground somewhere; nothing beyond the box
        whole = built.pull_cells([pair.dec], None, cell=cell, source=source, planes=SPREAD_PLANES, against="spread", crop=crop)
        assert tuple(whole.maps.shape[2:]) == (rows, cols)
        assert np.array_equal(whole.maps[0].cpu().numpy().astype(np.int64), pair.want(SPREAD_PLANES, source, crop, None, cell, (rows, cols)))


@pytest.mark.parametrize("names, P", [(("excess",), 3), (("count", "spread"), 4), (("fore", "spread"), 6)])
def test_a_plane_subset_writes_its_slice_and_nothing_behind_it(built, cropped_pair, names, P):
    import torch
    pair = cropped_pair
    grid = (8, 12)
    out = torch.full((3, P, 8, 12), S32, dtype=torch.int32, device="cuda")
    cells = built.pull_cells([pair.dec], [(0, -3, 5, 61, 41)], cell=8, grid=grid, source="ycbcr", planes=names, against="spread", threshold=[2, 2, 2],
                             out=out[1:2])
    torch.cuda.synchronize()
    assert cells.got == [1] and bool((out[0] == S32).all()) and bool((out[2] == S32).all())
    assert np.array_equal(out[1].cpu().numpy().astype(np.int64), pair.want(names, "ycbcr", True, (-3, 5, 61, 41), 8, grid, (2, 2, 2)))
    for name in SPREAD_PLANES:
        assert (getattr(cells, name) is None) == (name not in names)


def test_two_moving_squares_over_a_noisy_half(built):
    """a scene whose right half flickers by up to 24 and whose left half is quiet; after twelve spread blends two squares of + 60
    appear, one in either half.  pull_boxes(against="spread", plane="fore") finds exactly the two squares; against="kept" with the
    same floor marks the noisy half as well.  Both are held against the numpy models of the maps and of the boxes"""
    W, H, cell = 128, 64, 8
    rng = np.random.default_rng(71)
    base = rng.integers(60, 120, (H, W))
    flat_c = np.full((H // 2, W // 2), 128, np.uint8)

    def picture(squares):
        Y = base + np.where(np.arange(W)[None, :] >= W // 2, rng.integers(-24, 25, (H, W)), rng.integers(-1, 2, (H, W)))
        for x, y in squares:
            Y[y:y + 16, x:x + 16] += 90
        return np.clip(Y, 0, 255).astype(np.uint8), flat_c, flat_c

    squares = [(16, 24), (96, 16)]
    sc = SpreadScene(built, [picture([]) for _ in range(40)] + [picture(squares)])
    spec = dict(gain=2, lowest=2, highest=255, update="all")
    for _ in range(40):
        sc.next()
        sc.spread(spec, shift=4, hold=2)
    sc.check("the scene")
    cur = sc.next()
    window, box, grid = (0, 0, W, H), (0, 0, W, H), (H // cell, W // cell)
    reach = bxm.reached(window, box, cell, grid)
    planes = [sm.channels(f, W, H, "y") for f in (cur, sc.model.hi, sc.model.V)]
    kw = dict(cell=cell, source="y", threshold=4, level=cell * cell // 2, max_boxes=32)
    found = {}
    for against, plane, want_map in (("spread", "fore", spm.maps(2, *planes, window, box, cell, grid, (4, 0, 0))[0]),
                                     ("kept", "above", clm.maps(clm.CHANGE, 32, planes[0], planes[1], window, box, cell, grid, (4, 0, 0))[0])):
        cb = built.pull_boxes([sc.dec], None, planes=(plane,), against=against, plane=plane, **kw)
        assert cb.cells.got == [1]
        assert np.array_equal(getattr(cb.cells, plane)[0, 0].cpu().numpy().astype(np.int64), want_map), against
        want = bxm.boxes(want_map, reach, window, box, cell, 32, bxm.ABOVE, kw["level"])
        assert np.array_equal(cb.host()[0], want), (against, cb.host()[0][:4], want[:4])
        found[against] = [tuple(int(v) for v in r[:4]) for r in want[1:1 + int(want[0, 1])]]
    assert found["spread"] == [(96, 16, 16, 16), (16, 24, 16, 16)]
    assert len(found["kept"]) >= 2 and (16, 24, 16, 16) in found["kept"] and any(x + w == W and w >= W // 2 - cell for x, _, w, _ in found["kept"])
    sc.close()


def test_a_warp_moves_the_kept_picture_and_leaves_the_spread_where_it_lies(built):
    """warp_kept by a whole-sample translation after spread blends: hi and lo move as tests/warp_model.py says, V is byte-identical
    and still valid"""
    W, H = 80, 48
    sc = SpreadScene(built, _noisy_pictures(W, H, 5, seed=81))
    spec = dict(gain=4, lowest=1, highest=255, update="all")
    for _ in range(4):
        sc.next()
        sc.spread(spec, shift=3, hold=2)
    before = sc.model.V.copy()
    S = sc.model.state()
    S2, outside = wm.warp_state(S, W, H, wm.translation(6, -4))
    warped, ids, counts = built.warp_kept([sc.dec], coefficients=[wm.translation(6, -4)], crop=False, count_outside=True)
    assert warped == [1] and ids == [103] and counts.cpu().tolist() == [outside]
    sc.model.hi, sc.model.lo = (S2 >> 8).astype(np.uint8), (S2 & 255).astype(np.uint8)
    assert not np.array_equal(sc.model.state(), S)
    sc.check("behind the warp")
    assert np.array_equal(sc.model.V, before) and len(np.unique(before)) > 2
    sc.next()
    sc.spread(spec, shift=3, hold=2)
    sc.check("a spread blend behind the warp")
    sc.close()
