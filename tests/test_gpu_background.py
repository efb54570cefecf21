"""GPU: the background model — h264bsdmiBlendCurrentPictures / blend_pictures and h264bsdmiOutputKeptPictures / pull_kept — through the
product library.  The pictures are chosen (tests/pcm_pictures.py: all-I_PCM streams carry any picture verbatim), so every current
picture is known exactly; the state is read back with pull_kept(fraction=True) and every comparison is an equality with
tests/background_model.py.  The bundled stream runs beside a twin decoder, as in test_gpu_region_change.py."""
import ctypes

import numpy as np
import pytest

import background_model as bm
import cells_model as clm
import change_model as cm
import pcm_pictures as pp
import shift_model as shm
import stats_model as sm
from test_gpu_region_change import Pair, _equal
from test_gpu_region_shift import _same

pytestmark = pytest.mark.gpu

SIZES = {"16x16": (16, 16, None), "80x48": (80, 48, None), "48x32-cropped": (48, 32, (1, 2, 2, 1))}


@pytest.fixture(autouse=True, scope="module")
def _through_the_product_library(built):
    built.use_product_library(True)
    yield
    built.use_product_library(False)


@pytest.fixture(autouse=True)
def _no_device_errors(built):
    yield
    assert built.device_errors() == 0


def _random_pictures(W, H, count, seed):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H // 2, W // 2), dtype=np.uint8),
             rng.integers(0, 256, (H // 2, W // 2), dtype=np.uint8)) for _ in range(count)]


class Scene:
    """a decoder over a stream of chosen pictures (picIds from 100) and the model of its kept picture.  next(): one more picture decoded
    and popped; blend() / keep(): the call on the decoder and on the model, their answers compared; check(): the state read back"""

    def __init__(self, built, pictures, crop=None):
        self.built = built
        self.H, self.W = pictures[0][0].shape
        self.frames = [pp.i420(p) for p in pictures]
        self.data = pp.pcm_stream(pictures, crop=crop)
        self.buf = ctypes.create_string_buffer(self.data, len(self.data))
        self.off, self.t = 0, -1
        self.dec = built.Decoder(1)
        self.model = bm.Background(self.W, self.H)
        self.window = (0, 0, self.W, self.H)
        if crop:
            self.window = (2 * crop[0], 2 * crop[2], self.W - 2 * (crop[0] + crop[1]), self.H - 2 * (crop[2] + crop[3]))

    def decode(self):
        """one more picture decoded, not popped: there is no current picture"""
        while self.off < len(self.data):
            r, rb = self.dec.decode(ctypes.addressof(self.buf) + self.off, len(self.data) - self.off, pic_id=100 + self.t + 1)
            self.off += rb
            assert r < self.built.H264BSD_ERROR
            if r == self.built.H264BSD_PIC_RDY:
                self.t += 1
                return
        raise AssertionError("the stream has no more pictures")

    def next(self):
        self.decode()
        assert self.dec.next_output_info()[1] == 100 + self.t
        return self.frames[self.t]

    @property
    def frame(self):
        return self.frames[self.t]

    def blend(self, stream=None, **kw):
        want = self.model.blend(self.frame, kw.get("shift", 4), kw.get("hold", 255), _model_shift(kw.get("moving_shift")))
        kept, blended, ids, moving = self.built.blend_pictures([self.dec], count_moving=True, stream=stream, **kw)
        if stream is not None:
            stream.synchronize()
        assert (kept, blended, ids) == ([1], [want[0]], [100 + self.t])
        assert moving.dtype.is_floating_point is False and moving.cpu().tolist() == [want[1]], (moving.cpu().tolist(), want, kw)
        return want

    def keep(self):
        assert self.built.keep_pictures([self.dec]) == ([1], [100 + self.t])
        self.model.keep(self.frame)

    def check(self, what=None, stream=None):
        hi, lo = self.built.pull_kept([self.dec], fraction=True, stream=stream)[0]
        if stream is not None:
            stream.synchronize()
        _same_state(hi, lo, self.model, what)

    def close(self):
        self.dec.close()


def _model_shift(moving_shift):
    return bm.FROZEN if moving_shift == "frozen" else moving_shift


def _same_state(hi, lo, model, what=None):
    hi, lo = hi.cpu().numpy(), lo.cpu().numpy()
    assert hi.dtype == np.uint8 and hi.shape == model.hi.shape == lo.shape
    assert np.array_equal(hi, model.hi), (what, "hi", np.argwhere(hi != model.hi)[:6].ravel())
    assert np.array_equal(lo, model.lo), (what, "lo", np.argwhere(lo != model.lo)[:6].ravel())


@pytest.mark.parametrize("shift", [0, 1, 4, 7])
@pytest.mark.parametrize("size", list(SIZES))
def test_six_random_pictures_blend_as_the_model_does(built, size, shift):
    """one macroblock (a quarter wavefront), 15 macroblocks (the last wavefront partly idle), a cropped stream; the first blend
    starts the model: it reports blended = 0 and leaves what a keep leaves"""
    W, H, crop = SIZES[size]
    sc = Scene(built, _random_pictures(W, H, 6, seed=W + shift), crop=crop)
    assert built.pull_kept([sc.dec], fraction=True) == [None]
    for t in range(6):
        sc.next()
        assert sc.blend(shift=shift)[0] == (1 if t else 0)
        sc.check((size, shift, t))
        if t == 0:
            assert np.array_equal(sc.model.hi, sc.frame) and (sc.model.lo == 0x80).all()
    assert shift == 0 or (sc.model.lo != 0x80).any()
    alone = built.pull_kept([sc.dec])[0]
    assert np.array_equal(alone.cpu().numpy(), sc.model.hi)
    sc.close()


@pytest.mark.parametrize("k", range(8))
def test_pictures_alternating_black_and_white_reach_both_ends_of_the_difference(built, k):
    W, H = 80, 48
    sc = Scene(built, [pp.flat(W, H, v, v, v) for v in (0, 255, 0, 255, 255, 0)])
    extremes = set()
    for t in range(6):
        sc.next()
        if t:
            d = bm.target(sc.frame) - sc.model.state()
            extremes |= {int(d.min()), int(d.max())}
        sc.blend(shift=k)
        sc.check((k, t))
    assert -65280 in extremes or 65280 in extremes
    sc.close()


def _gated_pictures(W, H):
    """a base picture and two that differ from it: small luma noise on a third of the samples, other chroma, and single luma samples
    far off at each of the four positions of a 2 x 2 block on tile borders and frame corners — by 128 in the first picture and by 64
    in the second (moving at hold 0 and 16) and, where the base is forced to 0, by 255 (moving at hold 254, never at 255)"""
    rng = np.random.default_rng(11)
    base = _random_pictures(W, H, 1, seed=12)[0]
    Y0 = base[0].copy()
    far = [(15, 15), (16, 15), (31, 16), (32, 33), (0, 0), (W - 1, H - 1), (47, 16), (16, 31)]
    full = [(14, 14), (17, 15), (33, 16), (30, 33)]
    assert {(x & 1, y & 1) for x, y in far} == {(0, 0), (1, 1), (1, 0), (0, 1)} == {(x & 1, y & 1) for x, y in full}
    for x, y in full:
        Y0[y, x] = 0
    out = [(Y0, base[1], base[2])]
    for p in range(2):
        noise = rng.integers(-3, 4, (H, W)) * (rng.integers(0, 3, (H, W)) == 0)
        Y = np.clip(Y0.astype(np.int64) + noise, 0, 255).astype(np.uint8)
        for x, y in far:
            Y[y, x] = Y0[y, x] ^ (0x40 if p else 0x80)
        for x, y in full:
            Y[y, x] = 255
        Cb, Cr = (np.clip(c.astype(np.int64) + rng.integers(-40, 41, c.shape), 0, 255).astype(np.uint8) for c in base[1:])
        out.append((Y, Cb, Cr))
    return out


@pytest.mark.parametrize("moving_shift", [0, 3, "frozen"])
@pytest.mark.parametrize("hold", [0, 16, 254, 255])
def test_the_hold_mask_and_the_moving_count(built, hold, moving_shift):
    """the moving count equals the model's and pull_change's `above` of the whole coded frame taken just before the blend"""
    W, H = 80, 48
    sc = Scene(built, _gated_pictures(W, H))
    sc.next()
    sc.blend(shift=2, hold=hold, moving_shift=moving_shift)
    counts = []
    for t in (1, 2):
        sc.next()
        above = int(built.pull_change([sc.dec], None, source="y", threshold=hold, crop=False).above[0, 0])
        luma, moving = bm.moving_masks(sc.frame, sc.model.hi, W, H, hold)
        assert moving[W * H:].sum() >= 2 * (luma.sum() > 0)
        _, count = sc.blend(shift=2, hold=hold, moving_shift=moving_shift)
        assert count == above == int(luma.sum())
        counts.append(count)
        sc.check((hold, moving_shift, t))
    assert (hold == 255) == (counts == [0, 0]) and (hold != 254 or 0 < counts[0] <= 4) and (hold != 0 or counts[0] > W * H // 8)
    sc.close()


@pytest.mark.parametrize("how", ["keep_pictures", "pull_change"])
def test_a_plain_keep_between_two_blends_resets_the_fraction(built, how):
    W, H = 80, 48
    sc = Scene(built, _random_pictures(W, H, 5, seed=21))
    for _ in range(3):
        sc.next()
        sc.blend(shift=3)
    assert (sc.model.lo != 0x80).any()
    sc.next()
    if how == "keep_pictures":
        sc.keep()
    else:
        ch = built.pull_change([sc.dec], None, source="y", keep=True)
        assert ch.got == [1] and ch.kept_pic_id == [102]
        sc.model.keep(sc.frame)
    sc.check(how)
    assert (sc.model.lo == 0x80).all() and np.array_equal(sc.model.hi, sc.frame)
    sc.next()
    assert sc.blend(shift=3)[0] == 1
    sc.check((how, "the blend after it"))
    sc.close()


def test_the_first_blend_equals_a_keep_and_shift_0_is_a_keep(built):
    """two decoders over the same stream: one blends (the model starts; then shift 0), the other keeps; the kept pictures and the
    change records against the following picture are the same bytes"""
    W, H = 80, 48
    pictures = _random_pictures(W, H, 4, seed=31)
    a, b = Scene(built, pictures), Scene(built, pictures)
    for t in range(3):
        a.next(), b.next()
        spec = dict(shift=0) if t else dict(shift=5, hold=9, moving_shift=6)
        assert built.blend_pictures([a.dec], **spec)[:2] == ([1], [1 if t else 0])
        b.keep()
        got_a, got_b = built.pull_kept([a.dec], fraction=True)[0], built.pull_kept([b.dec], fraction=True)[0]
        for x, y in zip(got_a, got_b):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())
        assert np.array_equal(got_a[0].cpu().numpy(), b.model.hi) and bool((got_a[1] == 0x80).all())
    a.next(), b.next()
    regions = [(0, 0, 0, W, H), (0, 5, 7, 33, 21)]
    ra = built.pull_change([a.dec], regions, source="ycbcr", bins=32, threshold=[3, 2, 1])
    rb = built.pull_change([b.dec], regions, source="ycbcr", bins=32, threshold=[3, 2, 1])
    assert ra.got == rb.got == [1, 1] and ra.kept_pic_id == rb.kept_pic_id == [102]
    assert np.array_equal(ra.records.cpu().numpy(), rb.records.cpu().numpy()) and int(ra.sad[0, 0]) > 0
    a.close(), b.close()


def test_a_batch_mixes_instances_and_leaves_the_others_as_they_are(built):
    """no sequence at all; a current picture and nothing kept; a kept picture of another size that is blended into; a kept picture but
    no current one"""
    nothing = built.Decoder(1)
    fresh = Scene(built, _random_pictures(80, 48, 1, seed=41))
    fresh.next()
    going = Scene(built, _random_pictures(16, 16, 3, seed=42))
    idle = Scene(built, _random_pictures(48, 32, 3, seed=43))
    for sc in (going, idle):
        for _ in range(2):
            sc.next()
            sc.blend(shift=2)
    going.next()
    idle.decode()                                            # decoded, not popped: no current picture
    decs = [nothing, fresh.dec, going.dec, idle.dec]
    want = going.model.blend(going.frame, 2, 10, 0)
    fresh.model.blend(fresh.frame, 2, 10, 0)
    kept, blended, ids, moving = built.blend_pictures(decs, shift=2, hold=10, moving_shift=0, count_moving=True)
    assert (kept, blended, ids) == ([0, 1, 1, 0], [0, 0, 1, 0], [0, 100, 102, 101])
    assert want[1] > 0 and moving.cpu().tolist() == [0, 0, want[1], 0]
    got = built.pull_kept(decs, fraction=True)
    assert got[0] is None
    for sc, g in zip((fresh, going, idle), got[1:]):
        _same_state(g[0], g[1], sc.model, (sc.W, sc.H))
    assert built.pull_kept([]) == [] and built.blend_pictures([]) == ([], [], [])
    nothing.close(), fresh.close(), going.close(), idle.close()


def test_the_consumers_of_the_kept_picture_see_the_high_bytes(built):
    """after three blends pull_change (y, and ycbcr with a histogram), pull_cells(against="kept") and pull_shift on the next picture
    equal their numpy models fed the model's hi frame as the kept picture"""
    W, H = 80, 48
    base = _random_pictures(W, H, 1, seed=51)[0]
    rng = np.random.default_rng(52)
    pictures = [tuple(np.clip(p.astype(np.int64) + rng.integers(-30, 31, p.shape), 0, 255).astype(np.uint8) for p in base) for _ in range(5)]
    sc = Scene(built, pictures)
    for _ in range(4):
        sc.next()
        sc.blend(shift=2, hold=20, moving_shift=5)
    sc.check()
    assert (sc.model.lo != 0x80).any() and not any(np.array_equal(sc.model.hi, f) for f in sc.frames)
    cur = sc.next()
    window, boxes = (0, 0, W, H), [(0, 0, W, H), (13, 11, 37, 23), (-9, 10, 30, 20)]
    regions = [(0,) + b for b in boxes]
    for source, bins, thr in (("y", 0, (6, 0, 0)), ("ycbcr", 64, (6, 3, 2))):
        C = 1 if source == "y" else 3
        planes = sm.channels(cur, W, H, source), sm.channels(sc.model.hi, W, H, source)
        ch = built.pull_change([sc.dec], regions, source=source, bins=bins, threshold=list(thr)[:C])
        assert ch.got == [1, 1, 1] and ch.kept_pic_id == [103]
        for k, b in enumerate(boxes):
            _equal(ch, k, cm.record(planes[0], planes[1], window, b, bins, thr), (source, b))
    planes = sm.channels(cur, W, H, "ycbcr"), sm.channels(sc.model.hi, W, H, "ycbcr")
    names = ("count", "sad", "dsum", "above")
    cells = built.pull_cells([sc.dec], regions, cell=8, grid=(6, 10), source="ycbcr", planes=names, against="kept", threshold=[6, 3, 2])
    assert cells.got == [1, 1, 1]
    for k, b in enumerate(boxes):
        want = clm.maps(clm.CHANGE, clm.plane_bits(clm.CHANGE, names), planes[0], planes[1], window, b, 8, (6, 10), (6, 3, 2))
        assert np.array_equal(cells.maps[k].cpu().numpy().astype(np.int64), want), b
    luma = lambda f: f[:W * H].reshape(H, W)
    sh = built.pull_shift([sc.dec], regions, radius=2, surface=True)
    assert sh.got == [1, 1, 1]
    for k, b in enumerate(boxes):
        _same(sh, k, shm.record(luma(sc.model.hi), luma(cur), window, b, 2), True, b)
    sc.close()


def test_six_pictures_of_the_bundled_stream_with_frozen_movers(built):
    """test_640x360.h264: coded height 368 and a crop; the twin decoder gives the I420 coded frames"""
    pair = Pair(built, "test_640x360")
    W, H = 640, 368
    model = bm.Background(W, H)
    counts = []
    for t in range(6):
        pic_id = pair.advance(1)
        assert pair.size() == (W, H)
        want = model.blend(pair.frame, 3, 12, bm.FROZEN)
        kept, blended, ids, moving = built.blend_pictures([pair.dec], shift=3, hold=12, moving_shift="frozen", count_moving=True)
        assert (kept, blended, ids) == ([1], [1 if t else 0], [pic_id]) and moving.cpu().tolist() == [want[1]]
        counts.append(want[1])
        hi, lo = built.pull_kept([pair.dec], fraction=True)[0]
        _same_state(hi, lo, model, t)
    assert any(0 < c < W * H for c in counts)
    pair.close()


def test_calls_on_other_streams_give_the_same_bytes(built):
    """blends on one torch stream alternating with comparisons on another (the ordering of launches that touch kept pictures), and the
    readback on a third: the state is the model's, as on the default stream"""
    import torch
    W, H = 80, 48
    sc = Scene(built, _random_pictures(W, H, 5, seed=61))
    s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    records = []
    for t in range(5):
        cur = sc.next()
        if t:
            want = cm.record(sm.channels(cur, W, H, "y"), sm.channels(sc.model.hi, W, H, "y"), (0, 0, W, H), (0, 0, W, H), 0, (4, 0, 0))
            records.append((built.pull_change([sc.dec], None, source="y", threshold=4, stream=s2), want))
        sc.blend(stream=s1, shift=3, hold=30, moving_shift=1)
    sc.check("streams", stream=s3)
    torch.cuda.synchronize()
    for ch, want in records:
        _equal(ch, 0, want)
    sc.close()
