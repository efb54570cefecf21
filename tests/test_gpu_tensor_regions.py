"""GPU: h264bsdmiOutputTensorRegions / pull_regions — boxes of pictures that have been popped already, each resampled into its own
slice of one tensor.  Expected values come from a twin decoder's host picture through the oracle's conversion (REFERENCE) or
tests/colour_model.py (BT.709 full range, bilinear chroma) and the float64 model of tests/region_model.py (pad, crop, resample);
from the tensor kernels themselves only where equality with them is the point."""
import ctypes

import numpy as np
import pytest

import region_model as gm
import resize_model as rm
from h264writer import StreamWriter
from test_gpu_tensor_colour import Feed, _geometry
from test_gpu_tensor_resize import (FILTERS, IMAGENET_MEAN, IMAGENET_STD, _check, _check_shares, _finish, _hwc, _source, _streams,
                                    _tol, _torch_dtype)

pytestmark = pytest.mark.gpu

PAD = (0.25, 114 / 255, 1.0)


@pytest.fixture(autouse=True, scope="module")
def _through_the_product_library(built):
    built.use_product_library(True)
    yield
    built.use_product_library(False)


@pytest.fixture(autouse=True)
def _no_device_errors(built):
    yield
    assert built.device_errors() == 0


class IdFeed(Feed):
    """a Feed whose pictures carry their decode index as picId"""

    def __init__(self, built, data, reorder=False):
        super().__init__(built, data)
        if reorder:
            self.dec.close()
            self.dec = built.Decoder(0)
        self.n = 0

    def step(self):
        while self.off < len(self.data):
            r, rb = self.dec.decode(ctypes.addressof(self.buf) + self.off, len(self.data) - self.off, pic_id=100 + self.n)
            self.off += rb
            assert r < self.built.H264BSD_ERROR
            if r == self.built.H264BSD_PIC_RDY:
                self.n += 1
                return True
        return False


def _norm(dt):
    return (IMAGENET_MEAN, IMAGENET_STD) if dt != "u8" else ((0, 0, 0), (1, 1, 1))


def _regions(built, decs, regions, dt, lay, ch, size, filt, colour, fit="stretch", pad=PAD, crop=True, **kw):
    mode, aa = FILTERS[filt]
    mean, std = _norm(dt)
    col = {} if colour == "reference" else dict(colour="bt709", colour_range="full", chroma="bilinear")
    return built.pull_regions(decs, regions, size, layout=lay, dtype=_torch_dtype(dt), channels=ch, mean=mean, std=std, crop=crop,
                              mode=mode, antialias=aa, fit=fit, pad=pad, **col, **kw)


def _border_values(dt, ch, pad):
    """the letterbox border as the tensor holds it, per output channel (alpha included)"""
    import torch
    mean, std = _norm(dt)
    C = 1 if ch == "Y" else 3
    want = torch.tensor([rm.pad_value(pad[c], dt, mean[c], std[c]) for c in range(C)], dtype=torch.float32).to(_torch_dtype(dt)).double().numpy()
    return np.append(want, 255.0 if dt == "u8" else 1.0) if ch in ("RGBA", "BGRA") else want


class Sources:
    """the converted windows of the pictures the twins popped, computed once per (decoder, colour, channels, crop)"""

    def __init__(self, pics, decs):
        self.pics, self.decs, self.memo = pics, decs, {}

    def get(self, i, colour, ch, crop=True):
        kind = "Y" if ch == "Y" else "BGR" if ch in ("BGR", "BGRA") else "RGB"
        key = (i, colour, kind, crop)
        if key not in self.memo:
            self.memo[key] = _source(self.pics[i][0], _geometry(self.decs[i], crop), colour, kind)
        return self.memo[key]


def _check_region(g, v, box, dt, ch, size, filt, colour, fit, pad, rect, what, shares=None):
    """g: [H, W, C'] float64 of one slice; v: the converted window; box: (x, y, w, h).  The rectangle is the model's, its inside the
    model's resampled crop, the border the normalised pad exactly; a box wholly outside is one value per channel"""
    mean, std = _norm(dt)
    ref = colour == "reference"
    want_rect, inner = gm.region(v, box, size, filt, fit, gm.sample_pad(pad, ref), fma=ref)
    assert rect == want_rect, (what, rect, want_rect)
    left, top, iw, ih = want_rect
    got_inner = g[top:top + ih, left:left + iw]
    # (a box wholly outside the picture is one pad value per channel: decided, but it says nothing about the resampling's rounding)
    _check(got_inner, _finish(inner, colour, dt, ch, mean, std), dt, _tol(colour, dt, std), what=what, half_up=ref,
           shares=None if gm.whole_outside(box, v.shape[1], v.shape[0]) else shares)
    border = np.ones(g.shape[:2], bool)
    border[top:top + ih, left:left + iw] = False
    if border.any():
        assert (g[border] == _border_values(dt, ch, pad)[None, :]).all(), (what, "border")
    if gm.whole_outside(box, v.shape[1], v.shape[0]):
        flat = got_inner.reshape(-1, got_inner.shape[2])
        assert (flat == flat[0][None, :]).all(), (what, "a box outside the picture is one value per channel")
        if not ref or dt == "u8":      # REF floats: (floor(255 pad + 0.5) / 255 - mean) / std, held to the model above
            assert (flat[0] == _border_values(dt, ch, pad)).all(), (what, flat[0])


def _open(built, names, cls=Feed):
    return [cls(built, d) for d in names], [cls(built, d) for d in names]


def _pop_all(feeds, refs):
    """one picture decoded and popped everywhere: the feeds by h264bsdmiNextOutputInfo, the twins to the host"""
    for f in feeds + refs:
        assert f.step()
    pics = [r.dec.next_output_picture() for r in refs]
    for f in feeds:
        assert f.dec.next_output_info() is not None
    return pics


CONFIGS = [("f32", "NCHW", "RGB", (64, 48)), ("u8", "NHWC", "RGBA", (57, 33)), ("f16", "NCHW", "BGR", (256, 128)),
           ("f32", "NHWC", "Y", (8, 8)), ("u8", "NCHW", "Y", (96, 96)), ("f16", "NHWC", "BGRA", (57, 33)),
           ("f32", "NHWC", "RGB", (128, 256)), ("u8", "NCHW", "RGB", (8, 8))]
# (decoder, x, y, w, h): odd origins and sizes inside, boxes that end on the window's right and bottom edge (the chroma clamp),
# small boxes (upscaling) and whole windows (downscaling); windows 640x360, 1920x1080, 1920x1080 (no regions), 90x60
INSIDE = [(0, 33, 21, 101, 77), (0, 640 - 151, 360 - 99, 151, 99), (0, 101, 51, 16, 12), (0, 0, 0, 640, 360),
          (1, 1001, 333, 399, 201), (1, 1920 - 64, 1080 - 128, 64, 128), (1, 0, 0, 1920, 1080), (1, 7, 1079, 25, 1),
          (3, 5, 7, 31, 23), (3, 90 - 45, 60 - 33, 45, 33), (3, 0, 0, 90, 60), (3, 89, 59, 1, 1)]


@pytest.mark.parametrize("colour", ["reference", "bt709"])
@pytest.mark.parametrize("filt", ["bilinear", "bilinear_aa", "bicubic_aa"])
def test_regions_inside_match_the_model(built, filt, colour):
    """one call over four streams of different frame sizes, several regions per instance and none for one of them, stretch and
    letterbox, every configuration of CONFIGS — on ONE popped picture per instance: the call pops nothing"""
    feeds, refs = _open(built, _streams())
    pics = _pop_all(feeds, refs)
    src = Sources(pics, [r.dec for r in refs])
    shares = {}
    for k, (dt, lay, ch, size) in enumerate(CONFIGS):
        for fit in ("stretch", "letterbox"):
            t, got, boxes, cur, ids = _regions(built, [f.dec for f in feeds], INSIDE, dt, lay, ch, size, filt, colour, fit)
            assert got == [1] * len(INSIDE) and cur == [1] * 4 and ids == [p[1] for p in pics]
            for r, (i, x, y, w, h) in enumerate(INSIDE):
                _check_region(_hwc(t[r], lay), src.get(i, colour, ch), (x, y, w, h), dt, ch, size, filt, colour, fit, PAD, boxes[r],
                              what=("regions", filt, colour, k, fit, r, dt), shares=shares)
    _check_shares(shares, ("regions", filt, colour))
    for f in feeds + refs:
        f.close()


# window-relative boxes for a ww x wh window: across each edge, across two corners, around the window, wholly outside on each side
def _edge_boxes(ww, wh):
    return [(-9, 11, 31, 21), (ww - 13, 5, 41, 17), (21, -7, 25, 19), (11, wh - 8, 23, 15), (-6, -11, 29, 31), (ww - 10, wh - 9, 35, 27),
            (-5, -3, ww + 11, wh + 8), (ww, 3, 20, 20), (-40, 5, 40, 9), (3, wh + 5, 12, 30), (7, -25, 30, 25), (-16384, -16384, 64, 64)]


@pytest.mark.parametrize("colour", ["reference", "bt709"])
@pytest.mark.parametrize("filt", ["bilinear", "bilinear_aa", "bicubic_aa"])
def test_regions_across_the_edges_read_the_pad(built, filt, colour):
    """boxes over each edge, over corners and wholly outside, on 640x360 and on the cropped synthetic stream with crop=True (what
    lies outside the cropping window is pad) and crop=False (the coded frame is the picture)"""
    names = ["test_640x360", _streams()[3]]
    feeds, refs = _open(built, names)
    pics = _pop_all(feeds, refs)
    src = Sources(pics, [r.dec for r in refs])
    for crop in (True, False):
        regions = []
        for i, r in enumerate(refs):
            geo = _geometry(r.dec, crop)
            regions += [(i,) + b for b in _edge_boxes(geo[4], geo[5])]
        assert _geometry(refs[1].dec, crop)[4:] == ((90, 60) if crop else (96, 64))
        for k, (dt, lay, ch, size) in enumerate([("f32", "NCHW", "RGB", (40, 56)), ("u8", "NHWC", "BGRA", (33, 17)),
                                                 ("f16", "NHWC", "Y", (64, 64)), ("f16", "NCHW", "BGR", (16, 24))]):
            for fit in ("stretch", "letterbox"):
                t, got, boxes, _, _ = _regions(built, [f.dec for f in feeds], regions, dt, lay, ch, size, filt, colour, fit, crop=crop)
                assert got == [1] * len(regions)
                for r, (i, x, y, w, h) in enumerate(regions):
                    _check_region(_hwc(t[r], lay), src.get(i, colour, ch, crop), (x, y, w, h), dt, ch, size, filt, colour, fit, PAD,
                                  boxes[r], what=(crop, k, fit, r))
    for f in feeds + refs:
        f.close()


@pytest.mark.parametrize("colour", ["reference", "bt709"])
def test_the_whole_window_is_pull_tensor_bit_for_bit(built, colour):
    """the whole window as one region against pull_tensor of a twin with the same arguments: both go through the same tap
    arithmetic — the two antialiased filters with stretch, all three with letterbox (bilinear stretch is k_tensor_resize's own
    arithmetic in pull_tensor)"""
    import torch
    names = ["test_640x360", _streams()[3], "test_1920x1080"]
    feeds = [Feed(built, d) for d in names]
    for f in feeds:
        assert f.step() and f.dec.next_output_info() is not None
    wins = [_geometry(f.dec, True)[4:] for f in feeds]
    regions = [(i, 0, 0, w, h) for i, (w, h) in enumerate(wins)]
    col = {} if colour == "reference" else dict(colour="bt709", colour_range="full", chroma="bilinear")
    for dt, lay, ch, size in [("f16", "NCHW", "RGB", (224, 224)), ("u8", "NHWC", "BGRA", (96, 160)), ("f32", "NHWC", "Y", (57, 333))]:
        mean, std = _norm(dt)
        for filt, fit in [("bilinear_aa", "stretch"), ("bicubic_aa", "stretch"), ("bilinear", "letterbox"), ("bilinear_aa", "letterbox"),
                          ("bicubic_aa", "letterbox")]:
            twins = [Feed(built, d) for d in names]
            for tw in twins:
                assert tw.step()
            mode, aa = FILTERS[filt]
            want, got2, _, _, _, wboxes = built.pull_tensor([tw.dec for tw in twins], size=size, layout=lay, dtype=_torch_dtype(dt),
                                                            channels=ch, mean=mean, std=std, mode=mode, antialias=aa, fit=fit, pad=PAD,
                                                            return_boxes=True, **col)
            t, got, boxes, _, _ = _regions(built, [f.dec for f in feeds], regions, dt, lay, ch, size, filt, colour, fit)
            torch.cuda.synchronize()
            assert got == got2 == [1] * 3 and boxes == wboxes
            assert torch.equal(t, want), (dt, lay, ch, filt, fit, [int((t[i] != want[i]).sum()) for i in range(3)])
            for tw in twins:
                tw.close()
    for f in feeds:
        f.close()


@pytest.mark.parametrize("colour", ["reference", "bt709"])
def test_identity_scale_is_the_slice_of_the_full_size_pull(built, colour):
    """FILTER_BILINEAR, stretch, output size = box size, odd origins: the slice of a twin's size=None pull; u8 equal, floats within
    the tolerance of the resize tests"""
    import torch
    feed, twin = Feed(built, "test_640x360"), Feed(built, "test_640x360")
    assert feed.step() and twin.step() and feed.dec.next_output_info() is not None
    col = {} if colour == "reference" else dict(colour="bt709", colour_range="full", chroma="bilinear")
    boxes = [(0, 33, 21, 48, 40), (0, 591, 319, 48, 40), (0, 1, 1, 48, 40), (0, 592, 320, 48, 40)]
    full = {}
    for dt, lay, ch in [("u8", "NHWC", "RGBA"), ("f32", "NCHW", "RGB"), ("f16", "NHWC", "Y"), ("u8", "NCHW", "BGR")]:
        mean, std = _norm(dt)
        tw = Feed(built, "test_640x360")
        assert tw.step()
        whole = built.pull_tensor([tw.dec], size=None, layout=lay, dtype=_torch_dtype(dt), channels=ch, mean=mean, std=std, **col)[0]
        t, got, rects, _, _ = _regions(built, [feed.dec], boxes, dt, lay, ch, (40, 48), "bilinear", colour)
        torch.cuda.synchronize()
        assert got == [1] * 4 and rects == [(0, 0, 48, 40)] * 4
        w = _hwc(whole[0], lay)
        for r, (_, x, y, bw, bh) in enumerate(boxes):
            g, want = _hwc(t[r], lay), w[y:y + bh, x:x + bw]
            if dt == "u8":
                assert (g == want).all(), (dt, lay, ch, r)
            else:
                _check(g, want, dt, _tol(colour, dt, std), what=(dt, lay, ch, r), half_up=colour == "reference")
        tw.close()
    feed.close()
    twin.close()


def _one(built, dec, regions=((0, 33, 21, 101, 77), (0, -9, 300, 64, 128)), **kw):
    import torch
    res = built.pull_regions([dec], list(regions), (64, 32), dtype=torch.float32, mean=IMAGENET_MEAN, std=IMAGENET_STD, mode="bilinear",
                             antialias=True, fit="letterbox", pad=PAD, **kw)
    torch.cuda.synchronize()
    return res


def _expect_one(frame, dec, t, boxes, regions=((0, 33, 21, 101, 77), (0, -9, 300, 64, 128))):
    v = _source(frame, _geometry(dec, True), "reference", "RGB")
    for r, (_, x, y, w, h) in enumerate(regions):
        _check_region(_hwc(t[r], "NCHW"), v, (x, y, w, h), "f32", "RGB", (64, 32), "bilinear_aa", "reference", "letterbox", PAD, boxes[r], what=r)


def test_lifetime_of_the_current_picture(built):
    """nothing current before a pop and after a decode call; current after a pop by each kind of output call, with its picId; the
    call pops nothing: twice the same tensor, and the next pop gives the next picture"""
    import torch
    feed, twin = IdFeed(built, "test_640x360"), IdFeed(built, "test_640x360")
    sentinel = torch.full((2, 3, 64, 32), -7.0, dtype=torch.float32, device="cuda")

    def nothing_current():
        out = sentinel.clone()
        t, got, boxes, cur, ids = _one(built, feed.dec, out=out)
        assert got == [0, 0] and boxes == [None, None] and cur == [0] and ids == [0]
        assert torch.equal(out, sentinel)

    nothing_current()                                   # nothing decoded yet
    pops = [lambda d: d.next_output_picture()[1], lambda d: d.next_output_picture_device()[1], lambda d: d.next_output_info()[1],
            lambda d: built.pull_tensor([d], size=(8, 8))[2][0], lambda d: built.pull_batch([d])[1][0],
            lambda d: d.next_output_picture_converted(built.FMT_RGBA)[1]]
    for k, pop in enumerate(pops):
        assert feed.step() and twin.step()
        nothing_current()                               # decoded, not popped
        frame, pid = twin.dec.next_output_picture()[:2]
        assert pop(feed.dec) == pid == 100 + k
        t, got, boxes, cur, ids = _one(built, feed.dec)
        assert got == [1, 1] and cur == [1] and ids == [pid]
        _expect_one(frame, twin.dec, t, boxes)
        again = _one(built, feed.dec)
        assert torch.equal(t, again[0]) and again[1:] == (got, boxes, cur, ids)
        assert feed.dec.next_output_info() is None      # the regions popped nothing, and there is no second picture
        assert _one(built, feed.dec)[3] == [1]          # an empty pop changes nothing
    feed.dec.flush_buffer()
    nothing_current()                                   # h264bsdFlushBuffer
    feed.close()
    twin.close()


def test_regions_follow_output_reordering(built):
    """a stream whose output order differs from its decode order: the regions are those of the picture popped, whichever frame
    buffer it lies in, while later pictures have been decoded around it"""
    from synth_configs import CONFIGS as SYNTH
    data = StreamWriter(**SYNTH["poc0_display_reorder"]).build()
    feed, twin = IdFeed(built, data, reorder=True), IdFeed(built, data, reorder=True)
    regions = ((0, 3, 5, 41, 33), (0, -4, 30, 30, 50))
    order = []

    def drain():
        while True:
            pic = twin.dec.next_output_picture()
            info = feed.dec.next_output_info()
            assert (pic is None) == (info is None)
            if pic is None:
                return
            assert info[1] == pic[1]
            t, got, boxes, cur, ids = _one(built, feed.dec, regions)
            assert got == [1, 1] and ids == [pic[1]]
            _expect_one(pic[0], twin.dec, t, boxes, regions)
            order.append(pic[1])

    while feed.step():
        assert twin.step()
        drain()
    feed.dec.flush_buffer()
    twin.dec.flush_buffer()
    drain()
    assert len(order) == 12 and order != sorted(order) and sorted(order) == list(range(100, 112))
    feed.close()
    twin.close()


def test_regions_on_a_busy_side_stream_are_fenced_against_the_next_decode(built):
    """regions enqueued on a side stream that is still busy, the next pictures decoded and pulled at once (the frame-buffer slots
    come round again): the regions are those of the picture that was current, the later pictures equal the twins'"""
    import torch
    name, N = "test_1920x1080", 3
    feeds, twins = [Feed(built, name) for _ in range(N)], [Feed(built, name) for _ in range(N)]
    side = torch.cuda.Stream()
    regions = [(i, x, y, w, h) for i in range(N) for (x, y, w, h) in ((101, 55, 1501, 901), (-20, 700, 400, 400), (1500, 3, 333, 777))]
    kw = dict(dtype=torch.float16, mean=IMAGENET_MEAN, std=IMAGENET_STD, mode="bilinear", antialias=True, fit="letterbox", pad=PAD,
              colour="bt709", chroma="bilinear")
    big = torch.randn(4096, 4096, device="cuda")
    for rnd in range(2):
        for f in feeds + twins:
            assert f.step() and f.dec.next_output_info() is not None
        out = torch.empty((len(regions), 3, 256, 128), dtype=torch.float16, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(20):
                big = (big @ big).clamp_(-1, 1)             # keeps the side stream busy while the host runs ahead
        _, got, _, cur, _ = built.pull_regions([f.dec for f in feeds], regions, (256, 128), out=out, stream=side, **kw)
        assert got == [1] * len(regions) and cur == [1] * N
        later = []
        for _ in range(8):
            for f in feeds:
                assert f.step()
            later.append(built.pull_tensor([f.dec for f in feeds], size=(64, 64), dtype=torch.float16)[0])
        want = built.pull_regions([t.dec for t in twins], regions, (256, 128), stream=torch.cuda.default_stream(), **kw)[0]
        torch.cuda.synchronize()
        assert torch.equal(out, want), rnd
        for k in range(8):
            for t in twins:
                assert t.step()
            w = built.pull_tensor([t.dec for t in twins], size=(64, 64), dtype=torch.float16)[0]
            torch.cuda.synchronize()
            assert torch.equal(later[k], w), (rnd, k)
    for f in feeds + twins:
        f.close()


def test_4096_regions_over_16_instances_in_one_call(built):
    """seeded boxes (some over the edges) into 32 x 32 u8, every region against the model; a second call right behind the first
    (both halves of the staging ring) with other boxes"""
    import torch
    N, K = 16, 4096
    feeds = [Feed(built, "test_640x360") for _ in range(N)]
    ref = Feed(built, "test_640x360")
    for f in feeds:
        assert f.step() and f.dec.next_output_info() is not None
    assert ref.step()
    v = _source(ref.dec.next_output_picture()[0], _geometry(ref.dec, True), "reference", "RGB")
    rng = np.random.default_rng(4096)
    calls = []
    for c in range(2):
        w, h = rng.integers(1, 200, K), rng.integers(1, 200, K)
        x, y = rng.integers(-40, 640 + 20, K), rng.integers(-40, 360 + 20, K)
        regions = [(int(i), int(a), int(b), int(p), int(q)) for i, a, b, p, q in zip(rng.integers(0, N, K), x, y, w, h)]
        calls.append((regions, built.pull_regions([f.dec for f in feeds], regions, 32, dtype=torch.uint8, mode="bilinear", antialias=True,
                                                  pad=PAD)))
    torch.cuda.synchronize()
    for c, (regions, (t, got, boxes, cur, _)) in enumerate(calls):
        assert got == [1] * K and cur == [1] * N and boxes == [(0, 0, 32, 32)] * K
        g = t.cpu().double().numpy().transpose(0, 2, 3, 1)
        for r, (_, x, y, w, h) in enumerate(regions):
            _check_region(g[r], v, (x, y, w, h), "u8", "RGB", (32, 32), "bilinear_aa", "reference", "stretch", PAD, boxes[r], what=(c, r))
    for f in feeds + [ref]:
        f.close()


def test_raw_c_call_with_null_outputs_and_the_librarys_stream(built):
    """box, current, picId and stream NULL, resize and colour NULL ({FILTER_BILINEAR, FIT_STRETCH}, REFERENCE): the call waits"""
    import torch
    feed, twin = Feed(built, "test_640x360"), Feed(built, "test_640x360")
    empty = Feed(built, "test_640x360")
    assert feed.step() and twin.step() and feed.dec.next_output_info() is not None
    frame = twin.dec.next_output_picture()[0]
    regions = [(0, 33, 21, 101, 77), (1, 0, 0, 64, 64), (0, 600, -10, 80, 60)]
    out = torch.full((3, 48, 64, 3), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    spec = built.TensorSpec(out.data_ptr(), 64, 48, built.capi.LAYOUTS["NHWC"], 0, built.capi.CHANNELS["RGB"][0], 1, 1,
                            (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1))
    got = (ctypes.c_uint32 * 3)(9, 9, 9)
    rc = built.api_lib().h264bsdmiOutputTensorRegions(2, (ctypes.c_void_p * 2)(feed.dec._st, empty.dec._st), 3,
                                                      (built.Region * 3)(*[built.Region(*r) for r in regions]), ctypes.byref(spec),
                                                      None, None, None, got, None, None, None)
    assert rc == 0 and list(got) == [1, 0, 1]
    g = out.cpu().double().numpy()                      # no synchronisation: the call waited
    v = _source(frame, _geometry(twin.dec, True), "reference", "RGB")
    for r in (0, 2):
        _check_region(g[r], v, regions[r][1:], "u8", "RGB", (48, 64), "bilinear", "reference", "stretch", (0, 0, 0), (0, 0, 64, 48), what=r)
    assert (g[1] == 7).all()
    for f in (feed, twin, empty):
        f.close()
