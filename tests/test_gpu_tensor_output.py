"""GPU: h264bsdmiNextOutputTensorBatch / pull_tensor — the next pictures of many decoder instances as one device tensor,
held to the host API's pictures and the CPU oracle's colour conversion."""
import ctypes

import numpy as np
import pytest

from conftest import STREAMS, stream_bytes

pytestmark = pytest.mark.gpu

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
COMBOS = [("NCHW", "RGB"), ("NCHW", "BGR"), ("NCHW", "Y"), ("NHWC", "RGB"), ("NHWC", "BGR"), ("NHWC", "RGBA"), ("NHWC", "BGRA"),
          ("NHWC", "Y")]


@pytest.fixture(autouse=True, scope="module")
def _through_the_product_library(built):
    built.use_product_library(True)
    yield
    built.use_product_library(False)


@pytest.fixture(autouse=True)
def _no_device_errors(built):
    yield
    assert built.device_errors() == 0


class Feed:
    """one decoder instance and its private copy of a stream, advanced picture by picture"""

    def __init__(self, built, name, no_output_reordering=0):
        self.built = built
        self.data = stream_bytes(name)
        self.buf = ctypes.create_string_buffer(self.data, len(self.data))
        self.off = 0
        self.dec = built.Decoder(no_output_reordering)

    def step(self):
        """decode up to the next completed picture; False at the end of the stream"""
        while self.off < len(self.data):
            r, rb = self.dec.decode(ctypes.addressof(self.buf) + self.off, len(self.data) - self.off)
            self.off += rb
            assert r < self.built.H264BSD_ERROR
            if r == self.built.H264BSD_PIC_RDY:
                return True
        return False

    def close(self):
        self.dec.close()


def _geometry(dec, crop):
    W, H = 16 * dec.pic_width(), 16 * dec.pic_height()
    flag, left, cw, top, ch = dec.cropping_params()
    return (W, H, left, top, cw, ch) if crop and flag else (W, H, 0, 0, W, H)


def _oracle_rgba(frame, geo):
    """[h, w, 4] uint8 (R, G, B, 255) of a host I420 frame: pyoracle.oracle_convert, sliced to the window"""
    from oracle import pyoracle
    W, H, x0, y0, w, h = geo
    full = pyoracle.oracle_convert(0, W, H, frame).reshape(H, W)[y0:y0 + h, x0:x0 + w]
    return np.ascontiguousarray(full).view(np.uint8).reshape(h, w, 4)


def _oracle_luma(frame, geo):
    W, H, x0, y0, w, h = geo
    return frame[: W * H].reshape(H, W)[y0:y0 + h, x0:x0 + w]


def _expected_u8(rgba, luma, layout, channels):
    order = {"RGB": [0, 1, 2], "BGR": [2, 1, 0], "RGBA": [0, 1, 2, 3], "BGRA": [2, 1, 0, 3]}
    hwc = luma[:, :, None] if channels == "Y" else rgba[:, :, order[channels]]
    return np.array(hwc.transpose(2, 0, 1) if layout == "NCHW" else hwc)


def _normalise(rgb_hwc_u8, mean, std):
    """numpy float32 reference (v / 255 - mean) / std, [h, w, 3]"""
    return (rgb_hwc_u8.astype(np.float32) / np.float32(255) - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)


F16_STATS = {"elements": 0, "decided": 0, "undecided_differ": 0}       # summed over the _f16_close calls of a test (which resets it)


def _f16_rule(got, want32):
    """tests/rounding_model.py's float16 rule in torch, on the tensors' device: (within, decided, wrong) — got within one float16
    ulp of want32 rounded to float16 (the bound this comparison always had), where the rounding is decided, and where got is not
    want32 rounded to nearest even.

    eps.  want32 and the kernel evaluate the same three fp32 operations, (b / 255 - mean) / std, on the same operands.  With IEEE
    division both are the same number (test_float_without_resize_matches_numpy asserts that for float32); an evaluation whose last
    operation is not correctly rounded is still within one fp32 ulp of it, 2^(floor(log2 |v|) - 23).  That ulp is eps: got may
    differ from the rounded want32 only where want32 is that close to a midpoint of two float16 values.  The midpoints of float16
    are fp32 numbers and lie within a factor 2 of want32, so every difference below is exact in fp32.  (tests/test_rounding_model.py
    holds this function to rounding_model.f16_expected on every float16 value.)"""
    import torch
    want = want32.to(torch.float16).float()
    a = want.abs().clamp_min(2.0 ** -14)
    e = torch.frexp(a)[1].float() - 1                                   # floor(log2 a), exactly
    ulp = torch.exp2(e - 10)
    within = (got.float() - want).abs() <= ulp
    out = ulp / 2                                                       # to the midpoint away from zero
    inw = torch.where((want.abs() == torch.exp2(e)) & (want.abs() > 2.0 ** -14), ulp / 4, ulp / 2)   # a power of two: the finer side
    m = torch.where(want < 0, -want32, want32)                          # want32 on want's side of zero
    eps = torch.exp2(torch.frexp(want32.abs().clamp_min(2.0 ** -126))[1].float() - 24)
    decided = ((m - (want.abs() + out)).abs() > eps) & ((m - (want.abs() - inw)).abs() > eps)
    return within, decided, got.float() != want


def _f16_close(got, want32):
    """got (float16) equals want32 rounded to float16 wherever that rounding is decided (_f16_rule), and within one unit in the
    last place elsewhere"""
    import torch
    within, decided, wrong = _f16_rule(got, want32)
    ok, n_dec, n_und = torch.stack([(within & ~(decided & wrong)).all().long(), decided.sum(), (wrong & ~decided).sum()]).tolist()
    F16_STATS["elements"] += got.numel()
    F16_STATS["decided"] += n_dec
    F16_STATS["undecided_differ"] += n_und
    return bool(ok)


def _f16_stats(what):
    """prints the decided share of the _f16_close calls since the last report and requires rounding_model's floor of it"""
    import rounding_model as rd
    share = F16_STATS["decided"] / max(F16_STATS["elements"], 1)
    print(f"{what} f16: decided {share:.6f} of {F16_STATS['elements']}, undecided that differ {F16_STATS['undecided_differ']}")
    rd.check_share([share], "f16", what)
    for k in F16_STATS:
        F16_STATS[k] = 0


@pytest.mark.parametrize("crop", [True, False])
@pytest.mark.parametrize("name", STREAMS)
def test_u8_without_resize_is_bit_exact(built, name, crop):
    """every picture of 3 instances per layout / channel combination, pulled round by round, equals the oracle's conversion of
    the host API's picture (the luma plane for Y); metadata equals the host API's"""
    import torch
    groups = [[Feed(built, name) for _ in range(3)] for _ in COMBOS]
    ref = Feed(built, name)
    n_pics = 0
    while ref.step():
        for g in groups:
            for f in g:
                assert f.step()
        while True:
            pic = ref.dec.next_output_picture()
            outs = [built.pull_tensor([f.dec for f in g], layout=lay, dtype=torch.uint8, channels=ch, crop=crop)
                    for g, (lay, ch) in zip(groups, COMBOS)]
            torch.cuda.synchronize()
            if pic is None:
                assert all(o[1] == [0, 0, 0] for o in outs)
                break
            frame, pid, idr, err = pic
            geo = _geometry(ref.dec, crop)
            rgba, luma = _oracle_rgba(frame, geo), _oracle_luma(frame, geo)
            for (t, got, ids, idrs, errs), (lay, ch) in zip(outs, COMBOS):
                assert got == [1, 1, 1] and ids == [pid] * 3 and idrs == [idr] * 3 and errs == [err] * 3
                want = torch.from_numpy(_expected_u8(rgba, luma, lay, ch)).cuda()
                for k in range(3):
                    assert torch.equal(t[k], want), (n_pics, lay, ch, k)
            n_pics += 1
    assert n_pics == 73
    for f in [f for g in groups for f in g] + [ref]:
        f.close()


@pytest.mark.parametrize("dtype,layout", [("float32", "NCHW"), ("float16", "NCHW"), ("float32", "NHWC"), ("float16", "NHWC")])
def test_float_without_resize_matches_numpy(built, dtype, layout):
    """ImageNet mean / std: f32 exactly (rgb / 255 - mean) / std in numpy float32 (the same fp32 operations in the same order), f16
    that value rounded to f16"""
    import torch
    name = "test_640x360"
    feeds = [Feed(built, name) for _ in range(2)]
    ref = Feed(built, name)
    seen = 0
    while seen < 8 and ref.step():
        for f in feeds:
            assert f.step()
        while True:
            pic = ref.dec.next_output_picture()
            t, got, ids, _, _ = built.pull_tensor([f.dec for f in feeds], layout=layout, dtype=getattr(torch, dtype),
                                                  mean=IMAGENET_MEAN, std=IMAGENET_STD)
            torch.cuda.synchronize()
            if pic is None:
                assert got == [0, 0]
                break
            assert got == [1, 1] and ids == [pic[1]] * 2
            want = _normalise(_oracle_rgba(pic[0], _geometry(ref.dec, True))[:, :, :3], IMAGENET_MEAN, IMAGENET_STD)
            want = torch.from_numpy(np.ascontiguousarray(want.transpose(2, 0, 1) if layout == "NCHW" else want))
            for k in range(2):
                g = t[k].cpu()
                assert torch.equal(g, want if dtype == "float32" else want.to(torch.float16))
            seen += 1
    assert seen == 8
    for f in feeds + [ref]:
        f.close()


def _interp_ref(rgba, size):
    import torch
    import torch.nn.functional as F
    x = torch.from_numpy(np.ascontiguousarray(rgba[:, :, :3].transpose(2, 0, 1))).float()[None]
    return F.interpolate(x, size=size, mode="bilinear", align_corners=False, antialias=False)[0]      # [3, H, W], 0..255


@pytest.mark.parametrize("names,size", [
    (["test_640x360", "test_1920x1080", "test_640x360", "test_1920x1080_fullRange"], (224, 224)),
    (["test_640x360", "test_1920x1080", "test_640x360", "test_1920x1080_fullRange"], (257, 333)),
    (["test_640x360", "test_640x360"], (720, 1280)),
])
def test_resize_matches_torch_bilinear(built, names, size):
    """instances of different frame sizes in one call, resized (down, to odd sizes, up): f32 within 1e-4 of torch's bilinear
    interpolation of the oracle RGB in the 0..255 domain, U8 within 1"""
    import torch
    import rounding_model as rd
    shares = []
    feeds = {dt: [Feed(built, n, 1) for n in names] for dt in ("f32", "u8")}
    refs = [Feed(built, n, 1) for n in names]
    for rnd in range(3):
        for r in refs:
            assert r.step()
        for fs in feeds.values():
            for f in fs:
                assert f.step()
        pics = [r.dec.next_output_picture() for r in refs]
        t32, got32, ids32, _, _ = built.pull_tensor([f.dec for f in feeds["f32"]], size=size, dtype=torch.float32)
        t8, got8, _, _, _ = built.pull_tensor([f.dec for f in feeds["u8"]], size=size, dtype=torch.uint8)
        torch.cuda.synchronize()
        assert tuple(t32.shape) == (len(names), 3) + size
        for k, (p, r) in enumerate(zip(pics, refs)):
            assert p is not None
            assert got32[k] == 1 and got8[k] == 1 and ids32[k] == p[1]
            want = _interp_ref(_oracle_rgba(p[0], _geometry(r.dec, True)), size)
            assert float((t32[k].cpu() * 255 - want).abs().max()) <= 1e-4, (rnd, k)
            assert int((t8[k].cpu().int() - torch.round(want).int()).abs().max()) <= 1, (rnd, k)
            # the rounding itself (k_tensor_resize's own halves-up tail): exact wherever torch's value is further from a
            # half-integer than the 1e-4 the float32 pull of the same kernel is held to above
            shares.append(rd.check_u8(t8[k].cpu().double().numpy(), want.double().numpy(), 1e-4, True, what=("stretch bilinear", size, rnd, k)))
    if size != (720, 1280):         # 640 -> 1280: weights 1/4 and 3/4 pile values onto exact halves; the rule holds, the share does not count
        rd.check_share(shares, "u8", ("stretch bilinear reference", size))
    for f in [f for fs in feeds.values() for f in fs] + refs:
        f.close()


def test_got_mask_leaves_other_slices_untouched(built):
    """instances with nothing to give — drained, only headers parsed, nothing parsed — get got = 0 and their slices of a
    sentinel-filled tensor stay as they were"""
    import torch
    name = "test_640x360"
    drained, ready, headers, fresh = Feed(built, name), Feed(built, name, 1), Feed(built, name), Feed(built, name)
    while drained.step():
        while drained.dec.next_output_picture() is not None:
            pass
    while drained.dec.next_output_picture() is not None:
        pass
    assert ready.step()
    r, rb = headers.dec.decode(ctypes.addressof(headers.buf), len(headers.data))     # the SPS only
    assert r != built.H264BSD_PIC_RDY
    decs = [drained.dec, ready.dec, headers.dec, fresh.dec]
    out = torch.full((4, 3, 360, 640), 77, dtype=torch.uint8, device="cuda")
    t, got, ids, _, _ = built.pull_tensor(decs, size=(360, 640), dtype=torch.uint8, out=out)
    torch.cuda.synchronize()
    assert t.data_ptr() == out.data_ptr()
    assert got == [0, 1, 0, 0]
    for k in (0, 2, 3):
        assert bool((out[k] == 77).all())
    assert not bool((out[1] == 77).all())
    for f in (drained, ready, headers, fresh):
        f.close()


def _pull_c(built, decs, spec_kw, stream):
    L = built.api_lib()
    n = len(decs)
    s = dict(layout=0, dtype=0, channels=0, crop=1, resize=0)
    s.update(spec_kw)
    spec = built.TensorSpec(s["data"], s["width"], s["height"], s["layout"], s["dtype"], s["channels"], s["crop"], s["resize"],
                            (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1))
    got, ids = (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
    rc = L.h264bsdmiNextOutputTensorBatch(n, (ctypes.c_void_p * n)(*[d._st for d in decs]), ctypes.byref(spec), stream, got, ids, None, None)
    return rc, list(got), list(ids)


def test_all_or_nothing(built):
    """a batch that cannot be served — windows that differ without resize, an instance named twice — returns < 0 and pops nothing:
    the next pull of every instance yields the picture it would have yielded"""
    import torch
    names = ["test_640x360", "test_1920x1080"]
    feeds, twins = [Feed(built, n, 1) for n in names], [Feed(built, n, 1) for n in names]
    for f in feeds + twins:
        assert f.step()
    out = torch.zeros((2, 3, 360, 640), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc, _, _ = _pull_c(built, [f.dec for f in feeds], dict(data=out.data_ptr(), width=640, height=360), None)
    assert rc < 0
    with pytest.raises(RuntimeError):
        built.pull_tensor([f.dec for f in feeds], dtype=torch.uint8)
    rc, _, _ = _pull_c(built, [feeds[0].dec, feeds[0].dec], dict(data=out.data_ptr(), width=640, height=360), None)
    assert rc < 0
    for f, t in zip(feeds, twins):
        a = built.pull_tensor([f.dec], dtype=torch.uint8)
        b = built.pull_tensor([t.dec], dtype=torch.uint8)
        torch.cuda.synchronize()
        assert a[1] == b[1] == [1] and a[2] == b[2]
        assert torch.equal(a[0], b[0])
    for f in feeds + twins:
        f.close()


@pytest.mark.parametrize("on_torch_stream", [True, False])
def test_pull_is_asynchronous_and_slots_are_protected(built, on_torch_stream):
    """A pull enqueued on a non-default torch stream (or, asynchronous=False, on the library's own stream) is followed, without any
    synchronisation, by decoding and h264bsdmiFlushAsync of further pictures on every instance (1080p, no output reordering, so that
    frame-buffer slots are recycled).  After synchronising, the pulled tensor still equals the oracle's picture.  This shows that
    later ticks wait for the pull's fence in the cases exercised here; a test cannot prove that no race exists."""
    import torch
    name = "test_1920x1080"
    N = 4
    feeds = [Feed(built, name, no_output_reordering=1) for _ in range(N)]
    ref = Feed(built, name, no_output_reordering=1)
    L = built.api_lib()
    side = torch.cuda.Stream()
    for rnd in range(3):
        for f in feeds + [ref]:
            assert f.step()
        pic = ref.dec.next_output_picture()
        assert pic is not None
        out = torch.empty((N, 3, 1080, 1920), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        if on_torch_stream:
            t, got, ids, _, _ = built.pull_tensor([f.dec for f in feeds], dtype=torch.uint8, out=out, stream=side)
        else:
            rc, got, ids = _pull_c(built, [f.dec for f in feeds], dict(data=out.data_ptr(), width=1920, height=1080), None)
            assert rc == 0
        assert got == [1] * N and ids == [pic[1]] * N
        for _ in range(8):                              # the pulled picture's slot comes round again
            for f in feeds + [ref]:
                assert f.step()
            assert L.h264bsdmiFlushAsync() == 0
            ref.dec.next_output_picture()
        torch.cuda.synchronize()
        want = torch.from_numpy(_expected_u8(_oracle_rgba(pic[0], _geometry(ref.dec, True)), None, "NCHW", "RGB")).cuda()
        for k in range(N):
            assert torch.equal(out[k], want), (rnd, k)
    for f in feeds + [ref]:
        f.close()


def test_256_instances_every_picture(built):
    """256 instances of the 1080p stream, one pull_tensor per round (f16 NCHW, ImageNet normalisation) over all 73 pictures.
    Pictures 0, 1 and 72 are compared in full with the oracle; every picture of every instance is compared on the device with the
    same normalisation done in torch on next_output_picture_device(FMT_RGBA, crop=True) of a second set of 256 instances."""
    import torch
    name = "test_1920x1080"
    N = 256
    data = stream_bytes(name)
    mine = [built.Decoder() for _ in range(N)]
    other = [built.Decoder() for _ in range(N)]
    drv = built.BatchDriver(mine + other, [data] * (2 * N))
    ref = Feed(built, name)
    mean = torch.tensor(IMAGENET_MEAN, device="cuda").view(3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device="cuda").view(3, 1, 1)
    out = torch.empty((N, 3, 1080, 1920), dtype=torch.float16, device="cuda")
    n_pics = 0
    F16_STATS.update(dict.fromkeys(F16_STATS, 0))
    while True:
        ready = drv.step()
        if not ready:
            break
        assert len(ready) == 2 * N and ref.step()
        while True:
            t, got, ids, _, _ = built.pull_tensor(mine, dtype=torch.float16, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=out)
            pic = ref.dec.next_output_picture()
            if pic is None:
                assert got == [0] * N
                break
            assert got == [1] * N and len(set(ids)) == 1          # (BatchDriver numbers the pictures it feeds itself)
            for k, d in enumerate(other):
                p = d.next_output_picture_device(built.FMT_RGBA, crop=True)
                assert p is not None and p[1] == ids[k]
                want = (p[0][:, :, :3].permute(2, 0, 1).float() / 255 - mean) / std
                assert _f16_close(t[k], want), (n_pics, k)
            if n_pics in (0, 1, 72):
                want = _normalise(_oracle_rgba(pic[0], _geometry(ref.dec, True))[:, :, :3], IMAGENET_MEAN, IMAGENET_STD)
                want = torch.from_numpy(np.ascontiguousarray(want.transpose(2, 0, 1))).cuda()
                for k in (0, 1, 127, 255):
                    assert _f16_close(t[k], want), (n_pics, k)
            n_pics += 1
    assert n_pics == 73
    _f16_stats("256 instances, every picture")
    for d in mine + other:
        d.close()
    ref.close()
