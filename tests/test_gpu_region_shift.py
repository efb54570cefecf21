"""GPU: h264bsdmiOutputRegionShift / pull_shift through the product library.  The pictures are chosen (tests/pcm_pictures.py: all-I_PCM
streams carry any picture verbatim), so both the kept and the current picture are known exactly, and every record is compared with
tests/shift_model.py byte for byte.  The golden streams run beside a twin decoder, as in test_gpu_region_change.py."""
import ctypes

import numpy as np
import pytest

import pcm_pictures as pp
import shift_model as shm
from test_gpu_region_change import Pair
from test_gpu_tensor_colour import Feed

pytestmark = pytest.mark.gpu

W, H = 64, 48                                           # 4 x 3 macroblocks
CROP = dict(crop=(1, 2, 2, 2), window=(2, 4, 58, 40))   # frame_crop offsets in chroma samples: the window is at no macroblock edge
SHIFT = (3, -2)
RADII = [0, 1, 3, 16]
FILL = 0x5A


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


def _shifted(K, sx, sy):
    """C(u, v) = K(clamp(u - sx), clamp(v - sy)): the content moves by (sx, sy), replicated at the frame's border"""
    h, w = K.shape
    return K[np.clip(np.arange(h) - sy, 0, h - 1)[:, None], np.clip(np.arange(w) - sx, 0, w - 1)[None, :]]


class Chosen:
    """a decoder whose kept picture is lumas[0] and whose current picture is lumas[1]"""

    def __init__(self, built, lumas, crop=None):
        self.built, self.lumas = built, lumas
        self.feed = Feed(built, pp.pcm_stream([_picture(Y) for Y in lumas], crop=crop))
        self.dec = self.feed.dec
        self.next()
        assert built.keep_pictures([self.dec])[0] == [1]
        self.next()

    def next(self):
        assert self.feed.step()
        assert self.dec.next_output_info() is not None

    def close(self):
        self.feed.close()


def _same(sh, k, want, surface, what=None):
    """record k of a RegionShift against a model record, byte for byte, and through the views"""
    got = bytes(sh.records[k].cpu().numpy())
    assert got == want.bytes(surface), (what, k, np.frombuffer(got, "<u4")[:8], np.frombuffer(want.bytes(surface), "<u4")[:8])
    u32 = lambda t: int(t[k]) & 0xFFFFFFFF
    assert (u32(sh.count), int(sh.dx[k]), int(sh.dy[k]), u32(sh.best), u32(sh.still), u32(sh.ties)) == \
           (want.count, want.dx, want.dy, want.best, want.still, want.ties)
    if surface:
        assert np.array_equal(sh.surface[k].cpu().numpy().astype(np.int64) & 0xFFFFFFFF, want.surface)
    else:
        assert sh.surface is None


def _pull(built, decs, regions, radius, surface, **kw):
    """pull_shift into a record buffer that starts as FILL: the call writes whole records, pads included"""
    import torch
    K = len(decs) if regions is None else len(regions)
    out = torch.full((K, built.shift_record_bytes(radius, surface)), FILL, dtype=torch.uint8, device="cuda")
    sh = built.pull_shift(decs, regions, radius=radius, surface=surface, out=out, **kw)
    assert sh.records is out
    return sh


@pytest.fixture(scope="module", params=[False, True], ids=["coded", "cropped"])
def small(request, built, _through_the_product_library):
    rng = np.random.default_rng(5)
    K = rng.integers(0, 256, (H, W), dtype=np.uint8)
    c = Chosen(built, [K, _shifted(K, *SHIFT)], crop=CROP["crop"] if request.param else None)
    c.window = CROP["window"] if request.param else (0, 0, W, H)
    c.models = {}
    yield c
    c.close()


def _boxes(ww, wh):
    return [(0, 0, ww, wh), (5, 7, 1, 1), (13, 11, 37, 23), (-9, 10, 30, 20), (50, -7, 25, 19), (200, 200, 8, 8),
            (0, 0, 8, 8), (ww - 8, 0, 8, 8), (0, wh - 8, 8, 8), (ww - 8, wh - 8, 8, 8)]


@pytest.mark.parametrize("surface", [True, False])
@pytest.mark.parametrize("radius", RADII)
def test_boxes_of_a_shifted_pair_equal_the_model(built, small, radius, surface):
    """the whole window, one sample, a box across macroblock edges, boxes that leave the window, one that misses it, the four corners
    (the clamp in two directions); R = 16 exceeds a macroblock and a third of the picture's height"""
    ww, wh = small.window[2:]
    boxes = _boxes(ww, wh)
    assert small.dec.cropping_params()[0] == (small.window != (0, 0, W, H))
    if radius not in small.models:
        small.models[radius] = [shm.record(small.lumas[0], small.lumas[1], small.window, b, radius) for b in boxes]
    want = small.models[radius]
    sh = _pull(built, [small.dec], [(0,) + b for b in boxes], radius, surface)
    assert sh.got == [1] * len(boxes) and sh.current == [1] and sh.kept == [1]
    assert tuple(sh.records.shape) == (len(boxes), shm.record_bytes(radius, surface))
    for k, b in enumerate(boxes):
        _same(sh, k, want[k], surface, (radius, surface, b))
    assert want[5].count == 0 and want[5].ties == (2 * radius + 1) ** 2
    if radius >= 3:                                      # the guard: the box well inside finds the shift, exactly and alone
        assert (want[2].dx, want[2].dy, want[2].best, want[2].ties) == (SHIFT[0], SHIFT[1], 0, 1)
    if radius == 0:
        assert all(w.best == w.still and w.ties == 1 for w in want)


def test_both_band_paths_and_back_to_back_calls(built, small):
    """one whole-window region: three macroblock rows, S == 3, through the scratch and the tickets — twice in a row on one stream
    without a wait between them, at two radii (the second launch must find the tickets zero and wait for the scratch).  1024 regions
    of 16 x 16 in one call: S == 1, every workgroup closes its own record"""
    import torch
    ww, wh = small.window[2:]
    whole = (0, 0, ww, wh)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        first = _pull(built, [small.dec], None, 3, True, stream=st)
        second = _pull(built, [small.dec], None, 1, True, stream=st)
    st.synchronize()
    _same(first, 0, shm.record(small.lumas[0], small.lumas[1], small.window, whole, 3), True, "bands")
    _same(second, 0, shm.record(small.lumas[0], small.lumas[1], small.window, whole, 1), True, "bands again")
    regions = [(0, (7 * k) % (ww - 15), (5 * k) % (wh - 15), 16, 16) for k in range(1024)]
    many = _pull(built, [small.dec], regions, 2, True)
    assert many.got == [1] * 1024
    host = built.RegionShift(many.records.cpu(), 2, True, many.got, many.current, many.kept, many.pic_id, many.kept_pic_id)
    seen = {}
    for k, r in enumerate(regions):
        if r not in seen:
            seen[r] = shm.record(small.lumas[0], small.lumas[1], small.window, r[1:], 2)
        _same(host, k, seen[r], True, ("many", r))


def test_ties_go_to_the_nearest_then_the_smallest(built):
    """a flat pair: every displacement is a minimum, the answer is (0, 0).  A pair with period 4 horizontally, the current picture the
    kept one moved by 2: dx = -2 and dx = 2 are both exact, equally far, on the same row: the rule names dx = -2"""
    flat = np.full((H, W), 77, np.uint8)
    rng = np.random.default_rng(9)
    per = np.tile(rng.integers(0, 256, (H, 4), dtype=np.uint8), (1, W // 4))
    for lumas, box, want_d, want_ties in (([flat, flat], (0, 0, W, H), (0, 0), 81), ([per, np.roll(per, 2, axis=1)], (16, 9, 30, 21), (-2, 0), 2)):
        c = Chosen(built, lumas)
        want = shm.record(lumas[0], lumas[1], (0, 0, W, H), box, 4)
        assert (want.dx, want.dy) == want_d and want.ties == want_ties and want.best == 0
        for surface in (True, False):
            _same(_pull(built, [c.dec], [(0,) + box], 4, surface), 0, want, surface, ("ties", want_d))
        c.close()


def test_sums_above_2_31_on_the_largest_frame(built):
    """kept all 0, current all 255 on the largest legal frame (256 x 144 macroblocks); the largest box the limit allows inside it is
    4096 x 2304, at R = 1 every SAD is 255 x 9,437,184 = 2,406,481,920 > 2^31; 16 column chunks per band.  And a box whose width is no
    multiple of the chunk or of 4"""
    BW, BH = 4096, 2304
    lumas = [np.zeros((BH, BW), np.uint8), np.full((BH, BW), 255, np.uint8)]
    c = Chosen(built, lumas)
    boxes = [(0, 0, BW, BH), (3, 5, 1001, 40)]
    assert built.capi.SHIFT_MAX_SIDE == 4096
    for surface in (True, False):
        sh = _pull(built, [c.dec], [(0,) + b for b in boxes], 1, surface)
        for k, b in enumerate(boxes):
            want = shm.record(lumas[0], lumas[1], (0, 0, BW, BH), b, 1)
            assert want.best == 255 * want.count and want.ties == 9 and (want.dx, want.dy) == (0, 0)
            _same(sh, k, want, surface, ("big", b))
    assert 255 * BW * BH > 2 ** 31
    c.close()


def _luma(pair, frame):
    w, h = pair.frame_size
    return frame[:w * h].reshape(h, w)


def test_keep_chains_four_consecutive_pictures(built):
    """keep=True: call t searches the picture of call t - 1 in the picture of call t; the first call has nothing to compare with,
    leaves its record untouched and starts the chain"""
    pair = Pair(built, "test_640x360")
    for t in range(4):
        pic_id = pair.advance(1)
        sh = _pull(built, [pair.dec], None, 2, True, keep=True)
        assert sh.current == [1] and sh.pic_id == [pic_id]
        if t == 0:
            assert sh.got == [0] and sh.kept == [0] and sh.kept_pic_id == [0] and bool((sh.records == FILL).all())
        else:
            assert sh.got == [1] and sh.kept == [1] and sh.kept_pic_id == [pic_id - 1]
            want = shm.record(_luma(pair, pair.kept), _luma(pair, pair.frame), pair.window(True), (0, 0, 640, 360), 2)
            assert want.still > 0
            _same(sh, 0, want, True, t)
        pair.kept_now()
    pair.close()


def test_two_instances_of_different_sizes_and_the_sibling_sad(built):
    """640x360 and 1920x1080 in one call, 12 random boxes each at R = 2, regions interleaved; still is pull_change's luma sad"""
    pairs = [Pair(built, "test_640x360"), Pair(built, "test_1920x1080")]
    for p in pairs:
        p.advance(2)
        p.keep()
        p.advance(2)
    rng = np.random.default_rng(3)
    regions = []
    for k in range(24):
        i = k & 1
        ww, wh = pairs[i].window(True)[2:]
        w, h = int(rng.integers(1, 200)), int(rng.integers(1, 120))
        regions.append((i, int(rng.integers(-20, ww - 10)), int(rng.integers(-20, wh - 10)), w, h))
    decs = [p.dec for p in pairs]
    sh = _pull(built, decs, regions, 2, True)
    ch = built.pull_change(decs, regions, source="y", bins=0)
    assert sh.got == ch.got == [1] * 24 and sh.kept == [1, 1] and sh.kept_pic_id == [p.kept_id for p in pairs]
    assert sh.pic_id == [p.pic_id for p in pairs]
    for k, r in enumerate(regions):
        p = pairs[r[0]]
        want = shm.record(_luma(p, p.kept), _luma(p, p.frame), p.window(True), r[1:], 2)
        _same(sh, k, want, True, r)
        assert int(sh.still[k]) == int(ch.sad[k, 0]) and int(sh.count[k]) == int(ch.count[k])
    for p in pairs:
        p.close()


def test_moved_regions_follow_the_content(built, small):
    ww, wh = small.window[2:]
    regions = [(0, 13, 11, 37, 23), (0, 20, 15, 16, 16)]
    sh = built.pull_shift([small.dec], regions, radius=4)
    moved = sh.moved(regions)
    assert moved == [(0, 13 + SHIFT[0], 11 + SHIFT[1], 37, 23), (0, 20 + SHIFT[0], 15 + SHIFT[1], 16, 16)]
    res = built.pull_regions([small.dec], moved, (16, 16))
    assert res[1] == [1, 1]
    again = built.pull_shift([small.dec], moved, radius=1)               # and pull_shift takes them as well
    assert again.got == [1, 1]
    with pytest.raises(ValueError):
        sh.moved(regions[:1])
    with pytest.raises(ValueError):
        sh.moved(None)
    whole = built.pull_shift([small.dec], None, radius=4)                # whole windows: the caller names them
    assert whole.moved([(0, 0, 0, ww, wh)]) == [(0, int(whole.dx[0]), int(whole.dy[0]), ww, wh)]


def test_raw_calls_that_must_be_refused_write_nothing(built, small):
    import torch
    L = built.api_lib()
    stride = built.shift_record_bytes(1, True)
    out = torch.full((2, stride + 8), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    S = 0xA5A5A5A5
    fresh = Feed(built, pp.pcm_stream([_picture(small.lumas[0])]))      # a current picture, nothing kept
    assert fresh.step() and fresh.dec.next_output_info() is not None

    def call(decs, regs, data=None, radius=1, surface=1, crop=1, keep_after=0):
        spec = built.ShiftSpec(out.data_ptr() if data is None else data, radius, surface, crop, keep_after)
        arrays = [(ctypes.c_uint32 * 2)(S, S) for _ in range(5)]
        regions = (built.Region * 2)(*[built.Region(*r) for r in regs])
        rc = L.h264bsdmiOutputRegionShift(len(decs), (ctypes.c_void_p * len(decs))(*decs), 2, regions, ctypes.byref(spec), None, *arrays)
        return rc, [list(a) for a in arrays]

    good = [(0, 0, 0, 16, 16), (0, 10, 10, 8, 8)]
    untouched = (-1, [[S, S]] * 5)
    d = small.dec._st
    assert call([d, d], good) == untouched                               # repeated instances
    assert call([d], good, radius=17) == untouched
    assert call([d], good, surface=2) == untouched
    assert call([d], good, crop=2) == untouched
    assert call([d], good, keep_after=2) == untouched
    assert call([d], good, data=out.data_ptr() + 4) == untouched         # misaligned data
    assert call([d], [(0, 0, 0, 4097, 16), good[1]]) == untouched
    assert call([d], [good[0], (0, 0, 0, 16, 4097)]) == untouched
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    # an instance without a kept picture: got 0, its record untouched; the other region's record is written
    rc, arrays = call([d, fresh.dec._st], [good[0], (1, 0, 0, 16, 16)])
    assert rc == 0 and arrays[0] == [1, 0] and arrays[1] == [1, 1] and arrays[2] == [1, 0]
    torch.cuda.synchronize()
    assert bool((out.view(-1)[stride:] == FILL).all())
    rec = built.RegionShift(out.view(-1)[:2 * stride].view(2, stride), 1, True, [1, 0], [1, 1], [1, 0], [0, 0], [0, 0])
    _same(rec, 0, shm.record(small.lumas[0], small.lumas[1], small.window, good[0][1:], 1), True, "raw")
    fresh.close()
