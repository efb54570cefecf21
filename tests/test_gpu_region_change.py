"""GPU: h264bsdmiKeepCurrentPictures / keep_pictures and h264bsdmiOutputRegionChange / pull_change through the product library.  Beside
every decoder runs a twin, a second device decoder fed the same bytes; both pop in lock-step, the twin through
h264bsdNextOutputPicture, whose I420 coded frames are what tests/change_model.py compares.  Everything is an integer: every comparison
is an equality."""
import ctypes

import numpy as np
import pytest

import change_model as cm
import stats_model as sm
from conftest import stream_bytes
from h264writer import StreamWriter
from synth_configs import CONFIGS

pytestmark = pytest.mark.gpu

SOURCES = ["y", "ycbcr", "rgb"]
FIELDS = ("sad", "ssd", "sum", "max", "above")


@pytest.fixture(autouse=True, scope="module")
def _through_the_product_library(built):
    built.use_product_library(True)
    yield
    built.use_product_library(False)


@pytest.fixture(autouse=True)
def _no_device_errors(built):
    yield
    assert built.device_errors() == 0


def _data(name):
    return StreamWriter(**CONFIGS[name]).build() if name in CONFIGS else stream_bytes(name)


class Pair:
    """a decoder and its twin, fed the same NAL units (of one stream, or of several one after the other).  step(): one more picture
    decoded by both; pop(): the next output picture of both, current in the decoder, as the I420 coded frame from the twin -> picId;
    keep(): the decoder's current picture becomes its kept one, and the twin's frame the model's"""

    def __init__(self, built, *names):
        self.built = built
        self.data = b"".join(_data(n) for n in names)
        self.bufs = [ctypes.create_string_buffer(self.data, len(self.data)) for _ in range(2)]
        self.off = self.n = 0
        self.dec, self.twin = built.Decoder(1), built.Decoder(1)
        self.frame = self.frame_size = self.kept = self.kept_size = None
        self.pic_id = self.kept_id = 0

    def step(self):
        stall = 0
        while self.off < len(self.data) and stall <= 3:
            left = len(self.data) - self.off
            r, rb = self.dec.decode(ctypes.addressof(self.bufs[0]) + self.off, left, pic_id=100 + self.n)
            assert (r, rb) == self.twin.decode(ctypes.addressof(self.bufs[1]) + self.off, left, pic_id=100 + self.n)
            self.off += rb
            stall = stall + 1 if rb == 0 else 0
            if r == self.built.H264BSD_PIC_RDY:
                self.n += 1
                return True
        return False

    def pop(self):
        info, pic = self.dec.next_output_info(), self.twin.next_output_picture()
        assert info is not None and pic is not None and info[1:] == pic[1:]
        self.frame, self.frame_size, self.pic_id = np.array(pic[0], copy=True), self.size(), info[1]
        return info[1]

    def advance(self, pictures):
        for _ in range(pictures):
            assert self.step()
            pic_id = self.pop()
        return pic_id

    def keep(self, stream=None):
        assert self.built.keep_pictures([self.dec], stream=stream) == ([1], [self.pic_id])
        self.kept_now()

    def kept_now(self):
        self.kept, self.kept_size, self.kept_id = self.frame, self.frame_size, self.pic_id

    def size(self):
        return 16 * self.dec.pic_width(), 16 * self.dec.pic_height()

    def window(self, crop):
        W, H = self.size()
        flag, left, cw, top, ch = self.dec.cropping_params()
        return (left, top, cw, ch) if crop and flag else (0, 0, W, H)

    def planes(self, source):
        assert self.kept is not None and self.kept_size == self.frame_size
        return sm.channels(self.frame, *self.frame_size, source), sm.channels(self.kept, *self.kept_size, source)

    def want(self, source, crop, box, bins, threshold=(0, 0, 0), planes=None):
        cur, kept = planes or self.planes(source)
        return cm.record(cur, kept, self.window(crop), box, bins, threshold)

    def close(self):
        self.dec.close()
        self.twin.close()


def _equal(ch, k, want, what=None):
    """record k of a RegionChange against a model record"""
    assert int(ch.count[k]) == want.count, (what, k, int(ch.count[k]), want.count)
    assert not ch.records[k, 4:8].any()
    for name in FIELDS:
        got = getattr(ch, name)[k].cpu().numpy().astype(np.int64)
        assert np.array_equal(got, getattr(want, name)), (what, k, name, got, getattr(want, name))
    if want.hist is None:
        assert ch.hist is None
    else:
        got = ch.hist[k].cpu().numpy().astype(np.int64)
        assert np.array_equal(got, want.hist), (what, k, "hist", np.argwhere(got != want.hist)[:4])
        assert (got.sum(1) == want.count).all()


# (x, y, w, h) in a 640-wide window of 360 (cropped: the last macroblock row is cut in the middle) or 368 rows: the whole window,
# one sample, one aligned macroblock, odd everything across a tile corner, leaving the window on each side (negative origins
# included), outside it on either side
BOXES = [(0, 0, 640, 360), (5, 7, 1, 1), (32, 48, 16, 16), (13, 11, 37, 23), (-9, 10, 30, 20), (601, 3, 81, 17), (20, -7, 25, 19),
         (11, 338, 23, 45), (700, 50, 20, 20), (-40, 5, 40, 9)]


@pytest.mark.parametrize("later", [1, 3])
@pytest.mark.parametrize("source", SOURCES)
def test_the_kept_picture_survives_decoding_and_equals_the_model(built, source, later):
    """keep at picture 2 of the 640x360 stream, decode and pop 1 or 3 more pictures (the DPB goes round: the kept picture's frame buffer
    is decoded into again), compare: every bins, crop on (640 x 360) and off (the 640 x 368 coded frame), three thresholds"""
    pair = Pair(built, "test_640x360")
    kept_id = pair.advance(3)
    pair.keep()
    pic_id = pair.advance(later)
    planes = pair.planes(source)
    mixed = 0
    for crop in (True, False):
        rows = 360 if crop else 368
        assert pair.window(crop) == (0, 0, 640, rows)
        boxes = [(0, 0, 640, rows)] + BOXES[1:]             # the whole window of this crop setting first
        regions = [(0,) + b for b in boxes]
        for bins in (0, 16, 256):
            for t in (0, 7, 255):
                thr = (t, t, t) if bins != 16 else (t, 7, 0)
                ch = built.pull_change([pair.dec], regions, source=source, bins=bins, threshold=list(thr)[:ch_n(source)], crop=crop)
                assert ch.got == [1] * len(boxes) and ch.current == [1] and ch.kept == [1]
                assert ch.pic_id == [pic_id] and ch.kept_pic_id == [kept_id]
                assert tuple(ch.records.shape) == (len(boxes), cm.record_bytes(source, bins))
                for k, b in enumerate(boxes):
                    want = pair.want(source, crop, b, bins, thr, planes)
                    _equal(ch, k, want, (source, later, crop, bins, t, b))
                    mixed += int(any(0 < a < want.count for a in want.above))
                whole = pair.want(source, crop, boxes[0], bins, thr, planes)
                assert whole.sad.all() and whole.count == 640 * rows           # the guard: these two pictures differ in every channel
                assert int(ch.count[8]) == 0 and int(ch.count[9]) == 0 and not ch.records[8].any()
    assert mixed > 0                                                           # ... and `above` is neither nothing nor everything somewhere
    pair.close()


def ch_n(source):
    return 1 if source == "y" else 3


@pytest.mark.parametrize("source", SOURCES)
def test_keep_then_compare_without_decoding_is_all_zero(built, source):
    pair = Pair(built, "plain_ip")
    pic_id = pair.advance(2)
    pair.keep()
    ch = built.pull_change([pair.dec], [(0, 0, 0, 96, 80), (0, 3, 5, 30, 17)], source=source, bins=256)
    assert ch.got == [1, 1] and ch.kept == [1] and ch.pic_id == ch.kept_pic_id == [pic_id]
    assert [int(c) for c in ch.count] == [96 * 80, 30 * 17]
    for name in FIELDS:
        assert not getattr(ch, name).any(), name
    hist = ch.hist.cpu().numpy()
    assert (hist[:, :, 0] == ch.count.cpu().numpy()[:, None]).all() and not hist[:, :, 1:].any()
    assert bool(np.isinf(ch.psnr().cpu().numpy()).all()) and not ch.mse().any()
    pair.close()


def test_keep_after_chains_five_consecutive_pictures(built):
    """keep=True: call t gives the difference to the picture of call t - 1; the first call has nothing to compare with, leaves its
    record untouched and starts the chain"""
    import torch
    pair = Pair(built, "test_640x360")
    stride = built.change_record_bytes("ycbcr", 64)
    for t in range(5):
        pic_id = pair.advance(1)
        out = torch.full((1, stride), 0x5A, dtype=torch.uint8, device="cuda")
        ch = built.pull_change([pair.dec], None, source="ycbcr", bins=64, threshold=[4, 2, 2], keep=True, out=out)
        assert ch.current == [1] and ch.pic_id == [pic_id] and ch.records is out
        if t == 0:
            assert ch.got == [0] and ch.kept == [0] and ch.kept_pic_id == [0] and bool((out == 0x5A).all())
        else:
            assert ch.got == [1] and ch.kept == [1] and ch.kept_pic_id == [pic_id - 1]
            want = pair.want("ycbcr", True, (0, 0, 640, 360), 64, (4, 2, 2))
            assert want.sad[0] > 0
            _equal(ch, 0, want, t)
            mse = ch.mse()[0].cpu().numpy()
            assert np.allclose(mse, want.ssd / want.count) and np.allclose(ch.psnr()[0].cpu().numpy(), 10 * np.log10(255.0 ** 2 / mse))
        pair.kept_now()
    pair.close()


def test_both_band_paths_equal_the_model(built):
    """one whole-window region: 23 row bands meet in the engine's scratch, twice in a row on the same scratch (the tickets were zeroed
    by the first launch).  1,040 one-macroblock regions (and their edge relatives): one workgroup per region writes its record."""
    pair = Pair(built, "test_640x360")
    pair.advance(2)
    pair.keep()
    pair.advance(2)
    for source, bins, thr in (("ycbcr", 256, (3, 1, 1)), ("rgb", 32, (9, 9, 9)), ("y", 0, (12, 0, 0))):
        planes = pair.planes(source)
        want = pair.want(source, True, (0, 0, 640, 360), bins, thr, planes)
        first = built.pull_change([pair.dec], None, source=source, bins=bins, threshold=list(thr)[:ch_n(source)])
        again = built.pull_change([pair.dec], None, source=source, bins=bins, threshold=list(thr)[:ch_n(source)])
        _equal(first, 0, want, ("bands", source))
        assert bytes(first.records.cpu().numpy()) == bytes(again.records.cpu().numpy())
        regions = [(0, 16 * (k % 40), 16 * (k // 40), 16, 16) for k in range(920)]                      # every macroblock of the window
        regions += [(0, 16 * (k % 40) - 5, 16 * (k // 4) + 3, 16, 16) for k in range(120)]              # ... and boxes across four of them
        many = built.pull_change([pair.dec], regions, source=source, bins=bins, threshold=list(thr)[:ch_n(source)])
        assert many.got == [1] * 1040
        many = built.RegionChange(many.records.cpu(), ch_n(source), bins, many.got, many.current, many.kept, many.pic_id, many.kept_pic_id)
        for k, r in enumerate(regions):
            _equal(many, k, pair.want(source, True, r[1:], bins, thr, planes), ("many", source, r))
        assert int(many.sad[:920].sum(0)[0]) == int(want.sad[0])
    pair.close()


def test_eight_instances_of_different_sizes_in_one_call(built):
    """regions name the instances in mixed order; instance 2 has a current picture and no kept one, instance 5 a kept picture and no
    current one: their records stay as they were"""
    import torch
    names = ["test_640x360", "plain_ip", "multi_ref", "vga_multi_slice", "fmo_explicit", "aso", "high_qp", "multi_slice_idc012"]
    pairs = [Pair(built, n) for n in names]
    for i, p in enumerate(pairs):
        p.advance(1 + i % 2)
        if i != 2:
            p.keep()
        p.advance(1 + i % 3)
    assert pairs[5].step()                                   # decoded on, not popped: no current picture
    decs = [p.dec for p in pairs]
    regions = []
    for i in (3, 0, 7, 2, 5, 1, 6, 4, 0, 5, 3, 2):
        W, H = pairs[i].window(True)[2:]
        regions += [(i, 0, 0, W, H), (i, W // 3, -2, W // 2 + 1, H // 2 + 3)]
    stride = built.change_record_bytes("ycbcr", 16)
    out = torch.full((len(regions), stride), 0x5A, dtype=torch.uint8, device="cuda")
    ch = built.pull_change(decs, regions, source="ycbcr", bins=16, threshold=[5, 5, 5], out=out)
    assert ch.current == [1, 1, 1, 1, 1, 0, 1, 1] and ch.kept == [1, 1, 0, 1, 1, 1, 1, 1]
    assert ch.pic_id == [0 if i == 5 else p.pic_id for i, p in enumerate(pairs)]
    assert ch.kept_pic_id == [0 if i == 2 else p.kept_id for i, p in enumerate(pairs)]
    assert ch.got == [0 if r[0] in (2, 5) else 1 for r in regions]
    rec = built.RegionChange(out.cpu(), 3, 16, ch.got, ch.current, ch.kept, ch.pic_id, ch.kept_pic_id)
    for k, r in enumerate(regions):
        if ch.got[k]:
            _equal(rec, k, pairs[r[0]].want("ycbcr", True, r[1:], 16, (5, 5, 5)), r)
        else:
            assert bool((rec.records[k] == 0x5A).all())
    for p in pairs:
        p.close()


def test_two_streams_order_themselves_without_host_waits(built):
    """keep on stream A, compare on stream B, keep again on A, compare on B; the instance decodes on in between and nothing is waited
    for until the end: the comparisons see the pictures kept just before them"""
    import torch
    twin = Pair(built, "test_640x360")                      # the frames first, from a pair of its own
    frames = []
    for _ in range(4):
        twin.advance(1)
        frames.append(twin.frame)
    twin.close()
    data = _data("test_640x360")
    buf = ctypes.create_string_buffer(data, len(data))
    dec, off = built.Decoder(1), 0

    def picture(k):
        nonlocal off
        r = stall = 0
        while r != built.H264BSD_PIC_RDY and stall <= 3:
            r, rb = dec.decode(ctypes.addressof(buf) + off, len(data) - off, pic_id=100 + k)
            off += rb
            stall = stall + 1 if rb == 0 else 0
        assert r == built.H264BSD_PIC_RDY
        assert dec.next_output_info()[1] == 100 + k

    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    picture(0)
    assert built.keep_pictures([dec], stream=a) == ([1], [100])
    picture(1)
    first = built.pull_change([dec], None, source="ycbcr", bins=256, stream=b)
    assert built.keep_pictures([dec], stream=a) == ([1], [101])
    picture(2)
    picture(3)
    second = built.pull_change([dec], None, source="ycbcr", bins=256, stream=b)
    assert first.got == second.got == [1] and first.kept_pic_id == [100] and second.kept_pic_id == [101] and second.pic_id == [103]
    a.synchronize()
    b.synchronize()
    planes = [sm.channels(f, 640, 368, "ycbcr") for f in frames]
    _equal(first, 0, cm.record(planes[1], planes[0], (0, 0, 640, 360), (0, 0, 640, 360), 256), "first")
    _equal(second, 0, cm.record(planes[3], planes[1], (0, 0, 640, 360), (0, 0, 640, 360), 256), "second")
    dec.close()


def test_a_sequence_of_another_size_drops_the_kept_picture(built):
    """multi_ref and aso are 5 x 4 macroblocks with different parameter sets, plain_ip is 6 x 5: the kept picture outlives the
    activation of a sequence of its own size and goes with the first of another"""
    pair = Pair(built, "multi_ref", "aso", "plain_ip")
    pair.advance(3)
    pair.keep()
    kept_id = pair.kept_id
    pair.advance(12 - 3 + 2)                                 # into aso: the same coded size
    assert pair.size() == (80, 64)
    ch = built.pull_change([pair.dec], None, source="ycbcr", bins=16)
    assert ch.got == [1] and ch.kept == [1] and ch.kept_pic_id == [kept_id]
    _equal(ch, 0, pair.want("ycbcr", True, (0, 0, 80, 64), 16), "same size")
    pair.advance(10 - 2 + 2)                                 # into plain_ip
    assert pair.size() == (96, 80)
    ch = built.pull_change([pair.dec], None, source="ycbcr", bins=16)
    assert ch.got == [0] and ch.current == [1] and ch.kept == [0] and ch.kept_pic_id == [0]
    pair.keep()                                              # a new kept picture of the new size
    pair.advance(1)
    ch = built.pull_change([pair.dec], None, source="y", bins=0)
    assert ch.got == [1] and ch.kept == [1]
    _equal(ch, 0, pair.want("y", True, (0, 0, 96, 80), 0), "new size")
    pair.close()


def test_the_kept_picture_outlives_a_flush_and_a_miss_keeps_it(built):
    pair = Pair(built, "plain_ip")
    pair.advance(2)
    pair.keep()
    kept_id = pair.kept_id
    assert pair.step()                                       # no current picture now
    assert built.keep_pictures([pair.dec]) == ([0], [kept_id])
    pair.pop()
    built.api_lib().h264bsdFlushBuffer(pair.dec._st)
    built.api_lib().h264bsdFlushBuffer(pair.twin._st)
    ch = built.pull_change([pair.dec], None)
    assert ch.got == [0] and ch.current == [0] and ch.kept == [1] and ch.kept_pic_id == [kept_id]
    pair.close()


def test_raw_calls_that_need_a_live_decoder_are_refused_and_write_nothing(built):
    import torch
    pair = Pair(built, "plain_ip")
    pair.advance(2)
    pair.keep()
    pair.advance(1)
    L = built.api_lib()
    stride = built.change_record_bytes("y", 0)
    out = torch.full((2, stride + 8), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    regs = (built.Region * 2)(built.Region(0, 0, 0, 96, 80), built.Region(0, 10, 10, 16, 16))
    S = 0xA5A5A5A5

    def call(decs, data, thr=(0, 0, 0)):
        spec = built.ChangeSpec(data, 0, 0, 1, (ctypes.c_uint32 * 3)(*thr), 0)
        arrays = [(ctypes.c_uint32 * 2)(S, S) for _ in range(5)]
        rc = L.h264bsdmiOutputRegionChange(len(decs), (ctypes.c_void_p * len(decs))(*decs), 2, regs, ctypes.byref(spec), None, *arrays)
        return rc, [list(a) for a in arrays]

    untouched = (-1, [[S, S]] * 5)
    assert call([pair.dec._st, pair.dec._st], out.data_ptr()) == untouched           # repeated instances
    assert call([pair.dec._st], out.data_ptr(), thr=(256, 0, 0)) == untouched
    assert call([pair.dec._st], out.data_ptr(), thr=(0, 0, 256)) == untouched
    assert call([pair.dec._st], out.data_ptr() + 4) == untouched                     # misaligned data
    kept = (ctypes.c_uint32 * 2)(S, S)
    assert L.h264bsdmiKeepCurrentPictures(2, (ctypes.c_void_p * 2)(pair.dec._st, pair.dec._st), None, kept, None) == -1 and list(kept) == [S, S]
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())
    rc, arrays = call([pair.dec._st], out.data_ptr())                                # and the accepted call, on the library's own stream
    assert rc == 0 and arrays[0] == [1, 1] and arrays[1][0] == 1 and arrays[2][0] == 1
    ch = built.RegionChange(out.view(-1)[:2 * stride].view(2, stride), 1, 0, [1, 1], [1], [1], [0], [0])
    _equal(ch, 0, pair.want("y", True, (0, 0, 96, 80), 0))
    _equal(ch, 1, pair.want("y", True, (10, 10, 16, 16), 0))
    pair.close()
