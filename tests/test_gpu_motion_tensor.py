"""GPU: h264bsdmiSetMotionExport / h264bsdmiOutputMotionRegions / pull_motion through the product library.  Beside every device
decoder runs a twin in capture mode on the same bytes; its frame jobs give the expected side information (tests/motion_model.py
side_info: which job speaks for a frame buffer, validity, ages) and the expected tensor (motion_region).  The picture that a pull
reads is identified through the twin: both pop in lock-step, the twin's h264bsdmiNextOutputInfo names the frame buffer, and the
picIds (the decode index) must agree.

Error bounds.  NEAREST without units / per_picture: a vector component is mx / 4, exact in fp32 — equality.  With per_picture and
UNITS_OUTPUT the kernel makes at most three fp32 roundings (v / max(age, 1); (float) iw / (float) w; their product): relative
3 * 2^-24 < 2^-22 against float64; the model reproduces that operation order in numpy float32 (f32_steps), so NEAREST is ALSO
held to equality with it.  AREA: the kernel forms edges, weights and sums in double like the model and rounds the mean to fp32
once; per_picture's per-block division before it and the two roundings of the unit scaling after it make four, 4 * 2^-24 max|v|
over the footprint.  What is asserted is the bound of a kernel that sums the T blocks under a footprint in fp32, T roundings of
partial sums and one per weight, numerator and denominator: (T + 4) 2^-23 max|value in the footprint|, T = the most blocks a
footprint of the region can touch.  It is at least 5 * 2^-23 max|v|, so the double-precision kernel has to meet it everywhere; no
absolute term, no case excluded.
F16: the model's fp32 value converted by torch (round to nearest even), equality."""
import ctypes

import numpy as np
import pytest

import motion_model as mm
from conftest import stream_bytes
from h264writer import StreamWriter
from synth_configs import CONFIGS

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _through_the_product_library(built):
    built.use_product_library(True)
    yield
    built.use_product_library(False)


@pytest.fixture(autouse=True)
def _no_device_errors(built):
    yield
    assert built.device_errors() == 0


class Pair:
    """a device decoder with motion export and its capture twin, fed the same NAL units; pictures carry their decode index as
    picId.  step(): one more picture decoded by both (errors of damaged streams are skipped, as the reference harness does);
    pop(): the next output picture of both -> (frame buffer, picId) or None"""

    def __init__(self, built, data, reorder=False, motion=True, copy_elision=None):
        self.built = built
        self.data = data if isinstance(data, bytes) else stream_bytes(data)
        self.bufs = [ctypes.create_string_buffer(self.data, len(self.data)) for _ in range(2)]
        self.off = 0
        self.n = 0
        self.jobs, self.starts = [], set()
        self.dec = built.Decoder(0 if reorder else 1, motion=motion, copy_elision=copy_elision)
        self.twin = built.Decoder(0 if reorder else 1, capture=self.jobs.append)

    def step(self):
        stall = 0
        while self.off < len(self.data) and stall <= 3:
            left = len(self.data) - self.off
            r, rb = self.dec.decode(ctypes.addressof(self.bufs[0]) + self.off, left, pic_id=100 + self.n)
            r2, rb2 = self.twin.decode(ctypes.addressof(self.bufs[1]) + self.off, left, pic_id=100 + self.n)
            assert (r, rb) == (r2, rb2)
            self.off += rb
            stall = stall + 1 if rb == 0 else 0
            if r == self.built.H264BSD_HDRS_RDY:
                self.starts.add(len(self.jobs))
            if r == self.built.H264BSD_PIC_RDY:
                self.n += 1
                return True
        return False

    def pop(self):
        a, b = self.dec.next_output_info(), self.twin.next_output_info()
        assert (a is None) == (b is None)
        if a is None:
            return None
        assert a == b                                   # the same frame buffer, picId, isIdr, numErrMbs
        return b[0], b[1]

    def side(self, slot):
        return mm.side_of_slot(self.jobs, slot, self.starts)

    def window(self, crop):
        W, H = 16 * self.dec.pic_width(), 16 * self.dec.pic_height()
        flag, left, cw, top, ch = self.dec.cropping_params()
        return (left, top, cw, ch) if crop and flag else (0, 0, W, H)

    def close(self):
        self.dec.close()
        self.twin.close()


def _hwc(t, k, layout):
    v = t[k].cpu()
    return (v.permute(1, 2, 0) if layout == "NCHW" else v).double().numpy()


def _f16(x):
    import torch
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(torch.float16).double().numpy()


def _check_native(built, pair, slot, pic_id, what):
    """the native grid of the uncropped frame, NEAREST, SOURCE, all four planes: equal to the model, fp32 and fp16"""
    import torch
    side = pair.side(slot)
    window = pair.window(False)
    size = mm.native_size(window)
    rect, want, _ = mm.motion_region(side, window, (0, 0, window[2], window[3]), size)
    for dtype in (torch.float32, torch.float16):
        t, got, boxes, cur, ids = built.pull_motion([pair.dec], crop=False, dtype=dtype, planes=("mv", "valid", "age", "qp"))
        assert tuple(t.shape) == (1, 5, size[0], size[1]) and got == [1] and cur == [1] and ids == [pic_id], what
        assert boxes == [rect]
        g = _hwc(t, 0, "NCHW")
        assert np.array_equal(g, want if dtype == torch.float32 else _f16(want)), (what, dtype, np.abs(g - want).max())
    return side


@pytest.mark.parametrize("name,count", [("test_640x360", None), ("test_1920x1080", 12)])
def test_native_grid_equals_the_model_on_the_bundled_streams(built, name, count):
    """every picture of the 640x360 stream and the first 12 of the 1080p stream, copy elision on (the default for a decoder bound to
    a device; the twin captures WITHOUT it: elided macroblocks keep their records)"""
    pair = Pair(built, name)
    k = moving = 0
    while (count is None or k < count) and pair.step():
        slot, pic_id = pair.pop()
        assert pic_id == 100 + k
        side = _check_native(built, pair, slot, pic_id, (name, k))
        assert k > 0 or not side.valid.any()
        moving += int(side.mv.any())
        assert pair.pop() is None
        k += 1
    assert k >= (count or 30) and moving > 0
    pair.close()


def test_copy_elision_changes_nothing(built):
    """the same pictures with copy elision on and off: the same tensors (the 1080p stream elides most of its P_Skip copies)"""
    import torch
    on, off = Pair(built, "test_1920x1080", copy_elision=True), Pair(built, "test_1920x1080", copy_elision=False)
    for k in range(6):
        assert on.step() and off.step()
        slot, pic_id = on.pop()
        assert off.pop() == (slot, pic_id)
        a = built.pull_motion([on.dec], crop=False, dtype=torch.float32, planes=("mv", "valid", "age", "qp"))[0]
        b = built.pull_motion([off.dec], crop=False, dtype=torch.float32, planes=("mv", "valid", "age", "qp"))[0]
        assert torch.equal(a, b)
        _check_native(built, on, slot, pic_id, ("elision", k))
    on.close()
    off.close()


def _synthetic(name):
    import test_damaged_streams as tds
    return StreamWriter(**CONFIGS[name]).build() if name in CONFIGS else tds.stream_of(name)


SYNTHETIC = ["multi_ref", "everything", "redundant_slices", "redundant_fmo", "damaged_3", "damaged_14", "redundant_514",
             "redundant_521", "damaged_bundled_640x360"]


def test_native_grid_equals_the_model_on_synthetic_and_damaged_streams(built):
    """Streams of tests/h264writer.py and damaged ones (tests/damage.py), with output reordering on (h264bsdInit(.., 0)), every
    popped picture pulled and compared.  Together they must contain, checked here from the twin's jobs: partitions below 8x8,
    more than one reference age inside one picture, a FJ_MB_CONCEAL_P and an intra macroblock inside a P picture, pop order !=
    decode order, and a redundant-slice picture rendered as several jobs with a deblock-only job last (redo_split).  (Long skip
    runs with elided copies: the bundled 1080p stream, test_copy_elision_changes_nothing.)"""
    seen = dict(sub8=0, ages=0, conceal_p=0, intra_in_p=0, reordered=0, several_jobs=0)
    for name in SYNTHETIC:
        pair = Pair(built, _synthetic(name), reorder=True)
        order = []
        while pair.step():
            while True:
                p = pair.pop()
                if p is None:
                    break
                slot, pic_id = p
                order.append(pic_id)
                s = _check_native(built, pair, slot, pic_id, (name, pic_id))
                quads = s.mv.reshape(s.mv.shape[0] // 2, 2, s.mv.shape[1] // 2, 2, 2)
                seen["sub8"] += int((quads != quads[:, :1, :, :1]).any())
                seen["ages"] += int(len(np.unique(s.age[s.valid])) > 1)
                seen["conceal_p"] += int(s.valid.any() and (s.kind == 5).any())
                seen["intra_in_p"] += int(s.valid.any() and np.isin(s.kind, (1, 2, 3)).any())
        heads = [built.job_header(j) for j in pair.jobs]
        seen["several_jobs"] += sum(1 for a, b in zip(heads, heads[1:]) if a["ghost"] and b["dbk_only"] and not b["ghost"])
        seen["reordered"] += int(order != sorted(order))
        pair.close()
    assert all(seen.values()), seen


# (x, y, w, h) in the 640x360 cropping window (368 coded rows): odd origins and sizes, negative origin, reaching outside on every
# side, wholly outside, the whole window, one sample
BOXES = [(33, 21, 101, 77), (-9, 10, 30, 20), (601, 3, 81, 17), (20, -7, 25, 19), (11, 338, 23, 45), (-10, -10, 660, 380),
         (700, 50, 20, 20), (-40, 5, 40, 9), (0, 0, 640, 360), (639, 359, 1, 1), (128, 64, 256, 128)]
SIZES = [(17, 29), (64, 48), (8, 8), (45, 80), (56, 56)]


def _pulled_pair(built, name="test_640x360", pictures=5, **kw):
    pair = Pair(built, name, **kw)
    for _ in range(pictures):
        assert pair.step()
        slot, pic_id = pair.pop()
    return pair, slot, pic_id


@pytest.mark.parametrize("fit", ["stretch", "letterbox"])
@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
def test_regions_lie_over_the_pixels_of_a_region_pull(built, fit, layout):
    """crop on: the same boxes through pull_regions and pull_motion — the same output rectangles; NEAREST equal to the model,
    everything outside the rectangle and every sample outside the window zero in every plane"""
    import torch
    pair, slot, pic_id = _pulled_pair(built)
    side, window = pair.side(slot), pair.window(True)
    assert window == (0, 0, 640, 360) and side.valid.shape[0] == 92
    regions = [(0,) + b for b in BOXES]
    for size in SIZES:
        pix = built.pull_regions([pair.dec], regions, size, layout=layout, dtype=torch.float32, fit=fit)
        t, got, boxes, cur, ids = built.pull_motion([pair.dec], regions, size, layout=layout, dtype=torch.float32, fit=fit,
                                                    planes=("qp", "age", "valid", "mv"))
        assert (got, boxes, cur, ids) == (pix[1], pix[2], pix[3], pix[4]) and ids == [pic_id]
        for k, b in enumerate(BOXES):
            rect, want, _ = mm.motion_region(side, window, b, size, fit=fit)
            assert boxes[k] == rect
            g = _hwc(t, k, layout)
            assert np.array_equal(g, want), (size, b, np.abs(g - want).max())
            left, top, iw, ih = rect
            border = np.ones(size, bool)
            border[top:top + ih, left:left + iw] = False
            assert not g[border].any()
        assert not _hwc(t, 6, layout).any() and not _hwc(t, 7, layout).any()        # wholly outside
    pair.close()


@pytest.mark.parametrize("fit", ["stretch", "letterbox"])
def test_nearest_with_output_units_per_picture(built, fit):
    """at most three fp32 roundings: relative 2^-22 against the float64 model, and equality with the model that repeats the
    kernel's operation order in numpy float32"""
    import torch
    pair, slot, pic_id = _pulled_pair(built, "test_640x360", pictures=7)
    side, window = pair.side(slot), pair.window(True)
    regions = [(0,) + b for b in BOXES]
    for size in SIZES:
        for opts in (dict(units="output"), dict(per_picture=True), dict(units="output", per_picture=True)):
            t = built.pull_motion([pair.dec], regions, size, dtype=torch.float32, fit=fit, planes=("mv", "valid", "age", "qp"), **opts)[0]
            for k, b in enumerate(BOXES):
                _, want, _ = mm.motion_region(side, window, b, size, fit=fit, **opts)
                _, same, _ = mm.motion_region(side, window, b, size, fit=fit, f32_steps=True, **opts)
                g = _hwc(t, k, "NCHW")
                assert (np.abs(g - want) <= 2.0 ** -22 * np.abs(want)).all(), (size, b, opts)
                assert np.array_equal(g, same), (size, b, opts)
    pair.close()


@pytest.mark.parametrize("fit", ["stretch", "letterbox"])
def test_area_is_within_the_bound(built, fit):
    """(T + 4) 2^-23 max|value in the footprint| for the vectors (module docstring); VALID, AGE and QP are means of small integers
    with weights the kernel and the model form alike in double: the same bound with their largest value (1, 255, 51)"""
    import torch
    pair, slot, pic_id = _pulled_pair(built, pictures=7)
    side, window = pair.side(slot), pair.window(True)
    regions = [(0,) + b for b in BOXES]
    for size in SIZES:
        for opts in (dict(), dict(units="output", per_picture=True)):
            t, got, boxes, _, _ = built.pull_motion([pair.dec], regions, size, dtype=torch.float32, fit=fit, sampler="area",
                                                    planes=("mv", "valid", "age", "qp"), **opts)
            for k, b in enumerate(BOXES):
                rect, want, scale = mm.motion_region(side, window, b, size, fit=fit, sampler="area", **opts)
                assert boxes[k] == rect
                bound = (mm.footprint_blocks(b, rect, window) + 4) * 2.0 ** -23
                g = _hwc(t, k, "NCHW")
                d = np.abs(g - want)
                print("area", size, b, opts, "largest error / bound of dx, dy",
                      [float((d[..., c][scale[..., c] > 0] / (bound * scale[..., c][scale[..., c] > 0])).max(initial=0.0)) for c in (0, 1)])
                assert (d[..., 0] <= bound * scale[..., 0]).all() and (d[..., 1] <= bound * scale[..., 1]).all(), (size, b, opts)
                assert (d[..., 2] <= bound).all() and (d[..., 3] <= bound * 255).all() and (d[..., 4] <= bound * 51).all(), (size, b, opts)
    pair.close()


def test_many_decoders_of_three_sizes_in_one_call(built):
    """24 decoders of three frame sizes, several regions each, one of them without a picture (got = 0: slice untouched); the pull
    may be repeated; the picture stops being current at the next decode"""
    import torch
    names = ["test_640x360", "multi_ref", "vga_multi_slice"]
    datas = [stream_bytes(names[0]), StreamWriter(**CONFIGS[names[1]]).build(), StreamWriter(**CONFIGS[names[2]]).build()]
    pairs = [Pair(built, datas[i % 3]) for i in range(24)]
    slots = {}
    for i, p in enumerate(pairs):
        if i == 5:
            continue                                       # never decodes: no current picture
        for _ in range(2 + i % 3):
            assert p.step()
            slots[i] = p.pop()
    regions, size = [], (24, 40)
    for i, p in enumerate(pairs):
        W, H = (16 * p.dec.pic_width(), 16 * p.dec.pic_height()) if i != 5 else (64, 64)
        regions += [(i, 0, 0, W, H), (i, -3, 5, W // 2 + 1, H // 3), (i, W // 2, H // 2, W, H)]
    decs = [p.dec for p in pairs]
    out = torch.full((len(regions), 5, size[0], size[1]), -7.0, dtype=torch.float32, device="cuda")
    t, got, boxes, cur, ids = built.pull_motion(decs, regions, size, dtype=torch.float32, planes=("mv", "valid", "age", "qp"), out=out)
    assert cur == [0 if i == 5 else 1 for i in range(24)]
    for k, r in enumerate(regions):
        i = r[0]
        if i == 5:
            assert got[k] == 0 and boxes[k] is None and (t[k] == -7.0).all()
            continue
        assert got[k] == 1 and ids[i] == slots[i][1]
        _, want, _ = mm.motion_region(pairs[i].side(slots[i][0]), pairs[i].window(True), r[1:], size)
        assert np.array_equal(_hwc(t, k, "NCHW"), want), r
    again = built.pull_motion(decs, regions, size, dtype=torch.float32, planes=("mv", "valid", "age", "qp"), out=out.clone())
    assert torch.equal(again[0], t) and again[1:] == (got, boxes, cur, ids)
    assert pairs[0].step()                                  # instance 0 decodes: nothing is current any more
    t2, got2, _, cur2, _ = built.pull_motion(decs[:2], [(0, 0, 0, 64, 64), (1, 0, 0, 64, 64)], size, dtype=torch.float32)
    assert got2 == [0, 1] and cur2 == [0, 1]
    for p in pairs:
        p.close()


def test_a_pull_on_a_callers_stream_is_fenced_against_the_next_decode(built):
    """pull on a torch stream and decode on at once, picture after picture: every tensor is its own picture's, although the next
    pictures are decoded into the same frame buffers while the caller's stream may still be reading"""
    import torch
    pair = Pair(built, "test_1920x1080")
    st = torch.cuda.Stream()
    outs, wants = [], []
    for k in range(10):
        assert pair.step()
        slot, pic_id = pair.pop()
        with torch.cuda.stream(st):
            t = built.pull_motion([pair.dec], crop=False, dtype=torch.float32, planes=("mv", "valid", "age", "qp"), stream=st)[0]
        outs.append(t)
        window = pair.window(False)
        wants.append(mm.motion_region(pair.side(slot), window, (0, 0, window[2], window[3]), mm.native_size(window))[1])
    st.synchronize()
    for k, (t, want) in enumerate(zip(outs, wants)):
        assert np.array_equal(_hwc(t, 0, "NCHW"), want), k
    pair.close()


def test_a_new_sequence_of_another_size_starts_the_ages_from_nothing(built):
    """two streams of different sizes one after the other in one decoder: the side information follows the new size, and the first
    P pictures of the second sequence have no age older than the sequence"""
    a = StreamWriter(**CONFIGS["multi_ref"]).build()
    b = StreamWriter(**dict(CONFIGS["multi_ref"], wmb=7, hmb=6, seed=77)).build()
    pair = Pair(built, a + b)
    k, sizes = 0, set()
    first_of_b = len(mm.side_info(built.capture_stream(a)[0]))
    while pair.step():
        slot, pic_id = pair.pop()
        side = _check_native(built, pair, slot, pic_id, ("concat", k))
        sizes.add(side.valid.shape)
        if k >= first_of_b:
            assert side.age.max() <= k - first_of_b
        k += 1
    assert sizes == {(16, 20), (24, 28)} and k == 2 * first_of_b
    pair.close()


def test_without_motion_export_a_pull_is_refused(built):
    """export off (the default): -1 whatever the instance has decoded, also beside an instance that has it on; the switch itself
    is refused once the instance has decoded"""
    plain, slot, pic_id = _pulled_pair(built, motion=False)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        built.pull_motion([plain.dec], size=(8, 8))
    moving, _, _ = _pulled_pair(built)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        built.pull_motion([moving.dec, plain.dec], size=(8, 8))
    assert built.pull_motion([moving.dec], size=(8, 8))[1] == [1]
    L = built.api_lib()
    assert L.h264bsdmiSetMotionExport(plain.dec._st, 1) == -1
    assert L.h264bsdmiSetMotionExport(moving.dec._st, 0) == -1
    assert plain.dec.next_output_info() is None and plain.step() and plain.pop() is not None      # nothing was disturbed
    plain.close()
    moving.close()
