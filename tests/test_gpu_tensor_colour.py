"""GPU: h264bsdmiNextOutputTensorBatchColour / pull_tensor(colour=...) — the tensor pull in the stream's colour space, held to the
float64 model of tests/colour_model.py applied to the host API's picture of a twin decoder."""
import ctypes

import numpy as np
import pytest

import colour_model as cm
import rounding_model as rd
from conftest import stream_bytes
from h264writer import BitWriter, StreamWriter, nal

pytestmark = pytest.mark.gpu

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
DTYPES = {"u8": "uint8", "f16": "float16", "f32": "float32"}
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
    """one decoder instance (no output reordering: one picture out per picture in) and its private copy of a stream"""

    def __init__(self, built, data):
        self.built = built
        self.data = data if isinstance(data, bytes) else stream_bytes(data)
        self.buf = ctypes.create_string_buffer(self.data, len(self.data))
        self.off = 0
        self.dec = built.Decoder(1)

    def step(self):
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


def _torch_dtype(dt):
    import torch
    return getattr(torch, DTYPES[dt])


def _check(got, want, dt, std=IMAGENET_STD, what=""):
    """got: a tensor slice, want: the model's float64 values of the same shape.  f16: within one f16 ulp of the model, plus the
    fp32 evaluation's absolute error (1e-6 / |std|), which only matters near 0, where the f16 ulp is finer than fp32's at 1 — and
    equal to the model rounded to nearest even wherever the model lies further than that error from a midpoint of two float16
    values (tests/rounding_model.py); the decided share is printed and must reach rounding_model.F16_FLOOR"""
    g = got.cpu().double().numpy()
    assert g.shape == want.shape, what
    d = np.abs(g - want)
    if dt == "u8":
        assert d.max() <= 1, (what, d.max())
        assert (d == 0).mean() >= 0.999, (what, (d == 0).mean())
    elif dt == "f32":
        assert d.max() <= 1e-5 / min(abs(s) for s in std), (what, d.max())
    else:
        eps = 1e-6 / min(abs(s) for s in std)
        rd.check_share([rd.check_f16(g, want, eps, eps, what=what)], "f16", what)


def _pull(built, decs, dt, lay, ch, crop, size, **colour):
    import torch
    kw = dict(mean=IMAGENET_MEAN, std=IMAGENET_STD) if dt != "u8" else {}
    return built.pull_tensor(decs, size=size, layout=lay, dtype=_torch_dtype(dt), channels=ch, crop=crop, **kw, **colour)


def _pull_c(built, fn, decs, dt, lay, ch, crop, size, colour=None, **colour_args):
    """one call of the C entry point `fn`, into a fresh tensor; returns (tensor, got)"""
    import torch
    L = built.api_lib()
    n = len(decs)
    C = dict(RGB=3, BGR=3, RGBA=4, BGRA=4, Y=1)[ch]
    H, W = size if size is not None else _geometry(decs[0], crop)[5:3:-1]
    out = torch.full((n, C, H, W) if lay == "NCHW" else (n, H, W, C), 7, dtype=_torch_dtype(dt), device="cuda")
    torch.cuda.synchronize()
    mean, std = (IMAGENET_MEAN, IMAGENET_STD) if dt != "u8" else ((0, 0, 0), (1, 1, 1))
    spec = built.TensorSpec(out.data_ptr(), W, H, built.capi.LAYOUTS[lay], list(DTYPES).index(dt), built.capi.CHANNELS[ch][0],
                            1 if crop else 0, 0 if size is None else 1, (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std))
    got = (ctypes.c_uint32 * n)()
    VP = ctypes.c_void_p * n
    if fn == "old":
        rc = L.h264bsdmiNextOutputTensorBatch(n, VP(*[d._st for d in decs]), ctypes.byref(spec), None, got, None, None, None)
    else:
        cs = None if colour is None else ctypes.byref(built.ColourSpec(colour, *[colour_args.get(k, 0) for k in ("range", "chroma", "unspecified")]))
        rc = L.h264bsdmiNextOutputTensorBatchColour(n, VP(*[d._st for d in decs]), ctypes.byref(spec), cs, None, got, None, None, None)
    assert rc == 0
    return out, list(got)


@pytest.mark.parametrize("size", [None, (224, 224)])
@pytest.mark.parametrize("dt", ["u8", "f16", "f32"])
def test_null_and_reference_colour_are_the_old_entry_point(built, dt, size):
    """colour = NULL and matrix = REFERENCE through the new entry point give the old entry point's bytes, for every layout x channels"""
    import torch
    for lay, ch in COMBOS:
        feeds = [Feed(built, "test_640x360") for _ in range(3)]
        for rnd in range(2):
            for f in feeds:
                assert f.step()
            a, ga = _pull_c(built, "old", [feeds[0].dec], dt, lay, ch, True, size)
            b, gb = _pull_c(built, "new", [feeds[1].dec], dt, lay, ch, True, size, None)
            c, gc = _pull_c(built, "new", [feeds[2].dec], dt, lay, ch, True, size, 0)
            torch.cuda.synchronize()
            assert ga == gb == gc == [1]
            assert torch.equal(a, b) and torch.equal(a, c), (lay, ch, rnd)
        for f in feeds:
            f.close()


# (dtype, layout, channels, crop, size): every dtype, layout and channel mode, crop on and off, resize on and off
CONFIGS = [("u8", "NCHW", "RGB", True, None), ("u8", "NHWC", "BGRA", False, None), ("u8", "NHWC", "Y", True, (224, 224)),
           ("u8", "NCHW", "BGR", False, (257, 333)), ("f16", "NCHW", "RGB", True, None), ("f16", "NHWC", "RGBA", True, (224, 224)),
           ("f16", "NCHW", "Y", False, None), ("f16", "NHWC", "BGR", False, (720, 1280)), ("f32", "NHWC", "RGB", True, None),
           ("f32", "NCHW", "BGR", True, (224, 224)), ("f32", "NHWC", "Y", True, (131, 97)), ("f32", "NCHW", "RGB", False, (360, 640))]


@pytest.mark.parametrize("chroma", ["nearest", "bilinear"])
@pytest.mark.parametrize("rng", ["limited", "full"])
@pytest.mark.parametrize("matrix", ["bt601", "bt709", "bt2020"])
def test_explicit_colour_matches_the_model(built, matrix, rng, chroma):
    """3 pictures of the 640x360 stream per configuration, against the model of the twin decoder's host picture"""
    name = "test_640x360"
    feeds = [Feed(built, name) for _ in CONFIGS]
    ref = Feed(built, name)
    for rnd in range(3):
        assert ref.step()
        for f in feeds:
            assert f.step()
        frame, pid = ref.dec.next_output_picture()[:2]
        outs = [_pull(built, [f.dec], dt, lay, ch, crop, size, colour=matrix, colour_range=rng, chroma=chroma)
                for f, (dt, lay, ch, crop, size) in zip(feeds, CONFIGS)]
        for (t, got, ids, _, _), (dt, lay, ch, crop, size) in zip(outs, CONFIGS):
            assert got == [1] and ids == [pid]
            want = cm.expected(frame, _geometry(ref.dec, crop), matrix, rng == "full", chroma, dt, lay, ch, IMAGENET_MEAN, IMAGENET_STD, size)
            _check(t[0], want, dt, what=(rnd, dt, lay, ch, crop, size))
    for f in feeds + [ref]:
        f.close()


@pytest.mark.parametrize("dt,lay", [("u8", "NCHW"), ("f32", "NHWC"), ("f16", "NCHW")])
def test_crop_window_clamps_bilinear_chroma(built, dt, lay):
    """1080p, crop on: the last rows of the window take their chroma from the window only (the coded rows below the crop hold
    other samples, so a kernel that reads them fails there); without crop the same rows see the coded rows"""
    import torch
    name = "test_1920x1080"
    feeds = [Feed(built, name) for _ in range(3)]
    ref = Feed(built, name)
    for rnd in range(2):
        for f in feeds + [ref]:
            assert f.step()
        frame = ref.dec.next_output_picture()[0]
        geo = _geometry(ref.dec, True)
        assert geo[5] == 1080 and geo[1] == 1088
        t, got, _, _, _ = _pull(built, [f.dec for f in feeds[:2]], dt, lay, "RGB", True, None, colour="bt709", chroma="bilinear")
        full, _, _, _, _ = _pull(built, [feeds[2].dec], dt, lay, "RGB", False, None, colour="bt709", chroma="bilinear")
        torch.cuda.synchronize()
        assert got == [1, 1]
        want = cm.expected(frame, geo, "bt709", False, "bilinear", dt, lay, "RGB", IMAGENET_MEAN, IMAGENET_STD)
        for k in range(2):
            _check(t[k], want, dt, what=(rnd, k))
        rows = (slice(None), slice(1076, 1080)) if lay == "NCHW" else (slice(1076, 1080),)
        _check(t[0][rows], want[rows], dt, what=(rnd, "last rows"))
        want_full = cm.expected(frame, _geometry(ref.dec, False), "bt709", False, "bilinear", dt, lay, "RGB", IMAGENET_MEAN, IMAGENET_STD)
        _check(full[0], want_full, dt, what=(rnd, "uncropped"))
    for f in feeds + [ref]:
        f.close()


def _write_sps(wmb, hmb, full, mc, crop=None):
    """the SPS StreamWriter writes (its default configuration), with a VUI that carries video_signal_type and colour_description"""
    bw = BitWriter()
    bw.u(8, 66); bw.u(8, 0xC0); bw.u(8, 40)
    bw.ue(0)                                           # sps_id
    bw.ue(0)                                           # log2_max_frame_num - 4
    bw.ue(2)                                           # poc_type
    bw.ue(1)                                           # num_ref_frames
    bw.u(1, 0)                                         # gaps
    bw.ue(wmb - 1); bw.ue(hmb - 1)
    bw.u(1, 1); bw.u(1, 1)                             # frame_mbs_only, direct_8x8_inference
    bw.u(1, 1 if crop else 0)
    for v in crop or ():
        bw.ue(v)
    bw.u(1, 1)                                         # vui_parameters_present
    bw.u(1, 0); bw.u(1, 0)                             # aspect_ratio_info, overscan_info
    bw.u(1, 1)                                         # video_signal_type_present
    bw.u(3, 5); bw.u(1, full); bw.u(1, 1)              # video_format, video_full_range_flag, colour_description_present
    bw.u(8, 1); bw.u(8, 1); bw.u(8, mc)                # colour_primaries, transfer_characteristics, matrix_coefficients
    bw.u(1, 0); bw.u(1, 0); bw.u(1, 0); bw.u(1, 0)     # chroma_loc, timing, nal_hrd, vcl_hrd
    bw.u(1, 0)                                         # pic_struct_present
    bw.u(1, 0)                                         # bitstream_restriction
    bw.trailing()
    return nal(3, 7, bw.bytes())


def _synthetic(mc, full, crop=None, seed=3, wmb=6, hmb=4):
    data = StreamWriter(wmb=wmb, hmb=hmb, n_pics=3, seed=seed).build()
    pps = data.index(b"\x00\x00\x00\x01", 4)
    assert data[4] & 0x1F == 7 and data[pps + 4] & 0x1F == 8
    return _write_sps(wmb, hmb, full, mc, crop) + data[pps:]


@pytest.mark.parametrize("mc,full,named", [(1, 1, "bt709"), (5, 0, "bt601"), (9, 1, "bt2020"), (2, 0, None)])
def test_auto_takes_the_streams_matrix_and_range(built, mc, full, named):
    """synthetic streams whose VUI names a matrix and range: AUTO equals the explicit matrix and range byte for byte, and the model;
    matrix_coefficients 2 falls back to `unspecified`"""
    import torch
    data = _synthetic(mc, full, crop=(1, 2, 1, 1))
    auto, expl, ref = Feed(built, data), Feed(built, data), Feed(built, data)
    assert auto.step() and expl.step() and ref.step()
    assert ref.dec.video_range() == full and ref.dec.matrix_coefficients() == mc
    matrix = named or "fcc"
    for rnd in range(3):
        frame = ref.dec.next_output_picture()[0]
        a = _pull(built, [auto.dec], "f32", "NCHW", "RGB", True, None, colour="auto", unspecified="fcc", chroma="bilinear")
        b = _pull(built, [expl.dec], "f32", "NCHW", "RGB", True, None, colour=matrix, colour_range="full" if full else "limited",
                  chroma="bilinear")
        torch.cuda.synchronize()
        assert a[1] == b[1] == [1]
        assert torch.equal(a[0], b[0]), rnd
        geo = _geometry(ref.dec, True)
        assert geo[2:] == (2, 2, 90, 60)
        _check(a[0][0], cm.expected(frame, geo, matrix, bool(full), "bilinear", "f32", "NCHW", "RGB", IMAGENET_MEAN, IMAGENET_STD), "f32")
        if rnd < 2:
            assert auto.step() and expl.step() and ref.step()
    for f in (auto, expl, ref):
        f.close()


def test_auto_range_of_the_golden_streams(built):
    """test_1920x1080_fullRange signals full range: AUTO equals explicit FULL; test_1920x1080 does not: AUTO equals LIMITED"""
    import torch
    for name, rng in (("test_1920x1080_fullRange", "full"), ("test_1920x1080", "limited")):
        auto, expl = Feed(built, name), Feed(built, name)
        for rnd in range(2):
            assert auto.step() and expl.step()
            assert auto.dec.video_range() == (rng == "full")
            a = _pull(built, [auto.dec], "u8", "NHWC", "RGB", True, None, colour="bt709", chroma="bilinear")
            b = _pull(built, [expl.dec], "u8", "NHWC", "RGB", True, None, colour="bt709", colour_range=rng, chroma="bilinear")
            torch.cuda.synchronize()
            assert a[1] == b[1] == [1] and torch.equal(a[0], b[0]), (name, rnd)
        auto.close()
        expl.close()


@pytest.mark.parametrize("size", [None, (40, 56)])
def test_one_call_mixes_colour_spaces(built, size):
    """one AUTO call over a BT.709 full-range instance and a BT.601 limited-range one: each gets its own conversion"""
    import torch
    specs = [(1, 1, "bt709"), (5, 0, "bt601"), (1, 1, "bt709")]
    datas = [_synthetic(mc, full, seed=7 + k) for k, (mc, full, _) in enumerate(specs)]
    feeds, refs = [Feed(built, d) for d in datas], [Feed(built, d) for d in datas]
    for rnd in range(3):
        for f in feeds + refs:
            assert f.step()
        frames = [r.dec.next_output_picture()[0] for r in refs]
        t, got, _, _, _ = _pull(built, [f.dec for f in feeds], "f16" if rnd % 2 else "u8", "NCHW", "RGB", False, size,
                                colour="auto", chroma="bilinear")
        torch.cuda.synchronize()
        assert got == [1, 1, 1]
        dt = "f16" if rnd % 2 else "u8"
        for k, ((mc, full, m), r) in enumerate(zip(specs, refs)):
            want = cm.expected(frames[k], _geometry(r.dec, False), m, bool(full), "bilinear", dt, "NCHW", "RGB", IMAGENET_MEAN,
                               IMAGENET_STD, size)
            _check(t[k], want, dt, what=(rnd, k))
    for f in feeds + refs:
        f.close()


def test_pull_on_a_torch_stream_is_ordered_before_later_decoding(built):
    """a colour pull enqueued on a torch side stream, followed without synchronisation by more decoding and h264bsdmiFlushAsync of the
    same instances (1080p: frame-buffer slots come round again), gives what a synchronous pull of twin instances gives"""
    import torch
    name = "test_1920x1080"
    N = 3
    feeds, twins = [Feed(built, name) for _ in range(N)], [Feed(built, name) for _ in range(N)]
    L = built.api_lib()
    side = torch.cuda.Stream()
    kw = dict(colour="bt709", colour_range="full", chroma="bilinear")
    for rnd in range(2):
        for f in feeds + twins:
            assert f.step()
        out = torch.empty((N, 3, 1080, 1920), dtype=torch.float16, device="cuda")
        torch.cuda.synchronize()
        _, got, _, _, _ = built.pull_tensor([f.dec for f in feeds], dtype=torch.float16, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=out,
                                            stream=side, **kw)
        assert got == [1] * N
        for _ in range(8):                              # the pulled picture's slot comes round again
            for f in feeds:
                assert f.step()
            assert L.h264bsdmiFlushAsync() == 0
            for f in feeds:
                f.dec.next_output_picture()
        sync, got2, _, _, _ = built.pull_tensor([t.dec for t in twins], dtype=torch.float16, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                                                stream=torch.cuda.default_stream(), **kw)
        torch.cuda.synchronize()
        assert got2 == [1] * N
        assert torch.equal(out, sync), rnd
        for _ in range(8):
            for t in twins:
                assert t.step()
                t.dec.next_output_picture()
    for f in feeds + twins:
        f.close()
