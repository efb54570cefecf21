"""GPU: h264bsdmiOutputRegionStats / pull_stats through the product library.  Beside every decoder runs a twin, a second device
decoder fed the same bytes; both pop in lock-step, the twin through h264bsdNextOutputPicture, whose I420 coded frame is what
tests/stats_model.py reduces.  Everything is an integer: every comparison is an equality."""
import ctypes
import random

import numpy as np
import pytest

import stats_model as sm
from conftest import stream_bytes
from h264writer import StreamWriter
from synth_configs import CONFIGS

pytestmark = pytest.mark.gpu

SOURCES = ["y", "ycbcr", "rgb"]


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
    """a decoder and its twin, fed the same NAL units.  step(): one more picture decoded by both; pop(): the next output picture of
    both, current in the decoder, as the I420 coded frame from the twin -> picId"""

    def __init__(self, built, name):
        self.built = built
        self.data = _data(name)
        self.bufs = [ctypes.create_string_buffer(self.data, len(self.data)) for _ in range(2)]
        self.off = self.n = 0
        self.dec, self.twin = built.Decoder(1), built.Decoder(1)
        self.frame, self._planes = None, {}

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
        self.frame, self._planes = pic[0], {}
        return info[1]

    def advance(self, pictures):
        for _ in range(pictures):
            assert self.step()
            pic_id = self.pop()
        return pic_id

    def size(self):
        return 16 * self.dec.pic_width(), 16 * self.dec.pic_height()

    def window(self, crop):
        W, H = self.size()
        flag, left, cw, top, ch = self.dec.cropping_params()
        return (left, top, cw, ch) if crop and flag else (0, 0, W, H)

    def planes(self, source):
        if source not in self._planes:
            self._planes[source] = sm.channels(self.frame, *self.size(), source)
        return self._planes[source]

    def want(self, source, crop, box, bins):
        return sm.record(self.planes(source), self.window(crop), box, bins)

    def close(self):
        self.dec.close()
        self.twin.close()


def _equal(st, k, want, what=None):
    """record k of a RegionStats against a model record"""
    assert int(st.count[k]) == want.count, (what, k, int(st.count[k]), want.count)
    assert not st.records[k, 4:8].any()
    for name in ("sum", "sumsq", "min", "max"):
        got = getattr(st, name)[k].cpu().numpy().astype(np.int64)
        assert np.array_equal(got, getattr(want, name)), (what, k, name, got, getattr(want, name))
    if want.hist is None:
        assert st.hist is None
    else:
        got = st.hist[k].cpu().numpy().astype(np.int64)
        assert np.array_equal(got, want.hist), (what, k, "hist", np.argwhere(got != want.hist)[:4])
        assert (got.sum(1) == want.count).all()


# (x, y, w, h) in a 640-wide window of 360 (cropped: the last macroblock row is cut in the middle) or 368 rows: the whole window,
# one sample, one aligned macroblock, odd everything across a tile corner, leaving the window on each side (negative origins
# included), outside it on either side
BOXES = [(0, 0, 640, 360), (5, 7, 1, 1), (32, 48, 16, 16), (13, 11, 37, 23), (-9, 10, 30, 20), (601, 3, 81, 17), (20, -7, 25, 19),
         (11, 338, 23, 45), (700, 50, 20, 20), (-40, 5, 40, 9)]


@pytest.mark.parametrize("pictures", [0, 3])
@pytest.mark.parametrize("source", SOURCES)
def test_every_source_and_bins_equal_the_model(built, source, pictures):
    """picture 0 (intra) and picture 3 (P) of the 640x360 stream, crop on (640 x 360) and off (the 640 x 368 coded frame)"""
    pair = Pair(built, "test_640x360")
    pair.advance(1 + pictures)
    for crop in (True, False):
        rows = 360 if crop else 368
        assert pair.window(crop) == (0, 0, 640, rows)
        boxes = [(0, 0, 640, rows)] + BOXES[1:]             # the whole window of this crop setting first
        regions = [(0,) + b for b in boxes]
        for bins in sm.BINS:
            st = built.pull_stats([pair.dec], regions, source=source, bins=bins, crop=crop)
            assert st.got == [1] * len(boxes) and st.current == [1] and st.pic_id == [100 + pictures]
            assert tuple(st.records.shape) == (len(boxes), sm.record_bytes(source, bins))
            for k, b in enumerate(boxes):
                _equal(st, k, pair.want(source, crop, b, bins), (source, pictures, crop, bins, b))
            assert int(st.count[8]) == 0 and int(st.count[9]) == 0 and int(st.count[0]) == 640 * rows
    pair.close()


def test_both_merge_paths_at_the_same_shapes(built):
    """one region of 23 macroblock rows: 23 row bands meet in the engine's scratch.  1,100 regions (random boxes over 4 instances of
    three sizes, instances repeated, a fixed seed): one workgroup per region writes its record, and the item ring grows past its
    first 256.  The whole window is in both calls: the same record."""
    names = ["test_640x360", "plain_ip", "multi_ref", "test_640x360"]
    pairs = [Pair(built, n) for n in names]
    for i, p in enumerate(pairs):
        p.advance(2 + i)
    decs = [p.dec for p in pairs]
    rng = random.Random(5)
    regions = [(0, 0, 0, 640, 360)]
    while len(regions) < 1100:
        i = rng.randrange(4)
        W, H = pairs[i].window(True)[2:]
        w, h = rng.randint(1, W), rng.randint(1, H)
        regions.append((i, rng.randint(-20, W - 1), rng.randint(-20, H - 1), w, h))
    for source, bins in (("ycbcr", 256), ("rgb", 16), ("y", 0)):
        one = built.pull_stats(decs[:1], regions[:1], source=source, bins=bins)
        _equal(one, 0, pairs[0].want(source, True, regions[0][1:], bins), ("bands", source))
        many = built.pull_stats(decs, regions, source=source, bins=bins)
        assert many.got == [1] * 1100 and many.current == [1] * 4
        rec = many.records.cpu()
        assert bytes(rec[0].numpy()) == bytes(one.records[0].cpu().numpy())
        many = built.RegionStats(rec, 1 if source == "y" else 3, bins, many.got, many.current, many.pic_id)
        for k, r in enumerate(regions):
            _equal(many, k, pairs[r[0]].want(source, True, r[1:], bins), ("many", source, r))
    for p in pairs:
        p.close()


def test_no_regions_means_every_whole_window(built):
    names = ["test_640x360", "plain_ip", "multi_ref", "vga_multi_slice"]
    pairs = [Pair(built, names[i % 4]) for i in range(8)]
    for i, p in enumerate(pairs):
        p.advance(1 + i % 3)
    decs = [p.dec for p in pairs]
    for crop in (True, False):
        explicit = [(i,) + (0, 0) + p.window(crop)[2:] for i, p in enumerate(pairs)]
        a = built.pull_stats(decs, None, source="ycbcr", bins=64, crop=crop)
        b = built.pull_stats(decs, explicit, source="ycbcr", bins=64, crop=crop)
        assert a.got == b.got == [1] * 8 and a.pic_id == b.pic_id
        assert bytes(a.records.cpu().numpy()) == bytes(b.records.cpu().numpy())
        for i, p in enumerate(pairs):
            _equal(a, i, p.want("ycbcr", crop, explicit[i][1:], 64), (i, crop))
    for p in pairs:
        p.close()


def test_agrees_with_reductions_of_a_tensor_pull(built):
    """without the model: Y against the u8 luma pull of the same picture, RGB against the u8 REFERENCE pull of the next one"""
    import torch
    pair = Pair(built, "test_640x360")
    for source, channels in (("y", "Y"), ("rgb", "RGB")):
        assert pair.step() and pair.twin.next_output_picture() is not None
        t, got, ids, _, _ = built.pull_tensor([pair.dec], dtype=torch.uint8, channels=channels, size=None)        # pops: now current
        assert got == [1] and tuple(t.shape[2:]) == (360, 640)
        v = t[0].cpu().numpy().astype(np.int64).reshape(t.shape[1], -1)
        st = built.pull_stats([pair.dec], None, source=source, bins=256)
        assert st.got == [1] and st.pic_id == ids and int(st.count[0]) == 640 * 360
        assert np.array_equal(st.sum[0].cpu().numpy(), v.sum(1)) and np.array_equal(st.sumsq[0].cpu().numpy(), (v * v).sum(1))
        assert np.array_equal(st.min[0].cpu().numpy(), v.min(1)) and np.array_equal(st.max[0].cpu().numpy(), v.max(1))
        assert np.array_equal(st.hist[0].cpu().numpy(), np.stack([np.bincount(c, minlength=256) for c in v]))
        box = (0, 101, 77, 203, 131)
        sub = t[0, :, 77:77 + 131, 101:101 + 203].cpu().numpy().astype(np.int64).reshape(t.shape[1], -1)
        st = built.pull_stats([pair.dec], [box], source=source, bins=32)
        assert np.array_equal(st.sum[0].cpu().numpy(), sub.sum(1))
        assert np.array_equal(st.hist[0].cpu().numpy(), np.stack([np.bincount(c >> 3, minlength=32) for c in sub]))
    pair.close()


def test_an_instance_without_a_current_picture_leaves_its_records_untouched(built):
    import torch
    pair, idle = Pair(built, "plain_ip"), Pair(built, "plain_ip")
    pic_id = pair.advance(2)
    regions = [(0, 0, 0, 96, 80), (1, 0, 0, 96, 80), (0, 3, 3, 20, 20), (1, 5, 5, 1, 1)]
    out = torch.full((4, built.stats_record_bytes("ycbcr", 16)), 0x5A, dtype=torch.uint8, device="cuda")
    st = built.pull_stats([pair.dec, idle.dec], regions, source="ycbcr", bins=16, out=out)
    assert st.got == [1, 0, 1, 0] and st.current == [1, 0] and st.pic_id == [pic_id, 0] and st.records is out
    assert (out[1] == 0x5A).all() and (out[3] == 0x5A).all()
    _equal(st, 0, pair.want("ycbcr", True, regions[0][1:], 16))
    _equal(st, 2, pair.want("ycbcr", True, regions[2][1:], 16))
    out.fill_(0x5A)
    st = built.pull_stats([idle.dec], None, source="y", bins=0, out=out[:1, :32].contiguous())
    assert st.got == [0] and st.current == [0] and (st.records == 0x5A).all()
    pair.close()
    idle.close()


def test_lifetime_of_the_current_picture(built):
    """the call pops nothing and may be repeated; the picture stops being current at the next decode"""
    pair = Pair(built, "multi_ref")
    pic_id = pair.advance(3)
    a = built.pull_stats([pair.dec], None, source="rgb", bins=128)
    b = built.pull_stats([pair.dec], None, source="rgb", bins=128)
    assert a.got == b.got == [1] and a.pic_id == b.pic_id == [pic_id]
    assert bytes(a.records.cpu().numpy()) == bytes(b.records.cpu().numpy())
    _equal(a, 0, pair.want("rgb", True, (0, 0) + pair.window(True)[2:], 128))
    assert pair.step()
    c = built.pull_stats([pair.dec], None, source="rgb", bins=128)
    assert c.got == [0] and c.current == [0] and c.pic_id == [0]
    assert pair.pop() == pic_id + 1
    _equal(built.pull_stats([pair.dec], None, source="y", bins=16), 0, pair.want("y", True, (0, 0) + pair.window(True)[2:], 16))
    pair.close()


def test_two_side_streams_with_row_bands_then_decode(built):
    """two calls back to back on two streams, both with row bands (they share the engine's scratch, one behind the other), then the
    same instances decode on at once: both records are right, and the next pictures are bit-exact (the twin pulls them as well)"""
    import torch
    pairs = [Pair(built, "test_640x360"), Pair(built, "vga_multi_slice")]
    for p in pairs:
        p.advance(2)
    decs = [p.dec for p in pairs]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = built.pull_stats(decs, None, source="ycbcr", bins=256, stream=s1)
    b = built.pull_stats(decs, [(1, 0, 0, 640, 480), (0, -3, -3, 400, 300)], source="rgb", bins=32, stream=s2)
    wants = [p.want("ycbcr", True, (0, 0) + p.window(True)[2:], 256) for p in pairs]
    wants_b = [pairs[1].want("rgb", True, (0, 0, 640, 480), 32), pairs[0].want("rgb", True, (-3, -3, 400, 300), 32)]
    for p in pairs:
        assert p.step()
    s1.synchronize()
    s2.synchronize()
    for k in range(2):
        _equal(a, k, wants[k], ("s1", k))
        _equal(b, k, wants_b[k], ("s2", k))
    for p in pairs:
        got, want = p.dec.next_output_picture(), p.twin.next_output_picture()
        assert got is not None and got[1:] == want[1:] and np.array_equal(got[0], want[0])
    for p in pairs:
        p.close()


def test_a_raw_call_on_the_librarys_own_stream(built):
    """stream NULL: the call waits; current and picId may be NULL"""
    import torch
    pair = Pair(built, "plain_ip")
    pair.advance(2)
    L = built.api_lib()
    stride = built.stats_record_bytes("ycbcr", 16)
    out = torch.zeros((2, stride), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    regs = (built.Region * 2)(built.Region(0, 0, 0, 96, 80), built.Region(0, 90, 70, 16, 16))
    spec = built.StatsSpec(out.data_ptr(), 1, 16, 1)
    got = (ctypes.c_uint32 * 2)()
    assert L.h264bsdmiOutputRegionStats(1, (ctypes.c_void_p * 1)(pair.dec._st), 2, regs, ctypes.byref(spec), None, got, None, None) == 0
    assert list(got) == [1, 1]
    st = built.RegionStats(out, 3, 16, [1, 1], [1], [0])
    _equal(st, 0, pair.want("ycbcr", True, (0, 0, 96, 80), 16))
    _equal(st, 1, pair.want("ycbcr", True, (90, 70, 16, 16), 16))
    assert int(st.count[1]) == 6 * 10
    pair.close()
