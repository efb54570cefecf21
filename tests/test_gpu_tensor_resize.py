"""GPU: h264bsdmiNextOutputTensorBatchResize / pull_tensor(mode=..., antialias=..., fit=...) — antialiased and letterboxed tensor
pulls, held to the float64 models of tests/resize_model.py (weights, letterbox) and tests/colour_model.py (colour) applied to the host
API's picture of a twin decoder; the reference colour to the CPU oracle's conversion."""
import ctypes

import numpy as np
import pytest

import colour_model as cm
import resize_model as rm
import rounding_model as rd
from conftest import stream_bytes
from h264writer import StreamWriter
from test_gpu_tensor_colour import Feed, _geometry, _write_sps
from test_gpu_tensor_output import _oracle_rgba

pytestmark = pytest.mark.gpu

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
DTYPES = {"u8": "uint8", "f16": "float16", "f32": "float32"}
FILTERS = {"bilinear": ("bilinear", False), "bilinear_aa": ("bilinear", True), "bicubic_aa": ("bicubic", True)}


@pytest.fixture(autouse=True, scope="module")
def _through_the_product_library(built):
    built.use_product_library(True)
    yield
    built.use_product_library(False)


@pytest.fixture(autouse=True)
def _no_device_errors(built):
    yield
    assert built.device_errors() == 0


def _synthetic(wmb, hmb, crop=None, seed=3, n_pics=12):
    """a BT.709 full-range stream of wmb x hmb macroblocks (cropped when crop = (left, right, top, bottom) in crop units)"""
    data = StreamWriter(wmb=wmb, hmb=hmb, n_pics=n_pics, seed=seed).build()
    pps = data.index(b"\x00\x00\x00\x01", 4)
    return _write_sps(wmb, hmb, 1, 1, crop) + data[pps:]


def _streams():
    """the decoders of different frame sizes that share each call: 640x360, 1080p, 1080p full range, a cropped synthetic stream"""
    return ["test_640x360", "test_1920x1080", "test_1920x1080_fullRange", _synthetic(6, 4, crop=(1, 2, 1, 1))]


def _torch_dtype(dt):
    import torch
    return getattr(torch, DTYPES[dt])


def _source(frame, geo, colour, ch):
    """[h, w, C] float64 of a picture's window: REF the oracle's 8-bit R, G, B (or luma), otherwise the model's colour in [0, 1]"""
    if colour == "reference":
        W, H, x0, y0, w, h = geo
        if ch == "Y":
            return np.asarray(frame[: W * H], np.float64).reshape(H, W)[y0:y0 + h, x0:x0 + w, None]
        rgb = _oracle_rgba(frame, geo)[:, :, :3].astype(np.float64)
        return rgb[:, :, ::-1] if ch in ("BGR", "BGRA") else rgb
    return cm.colour_hwc(frame, geo, "bt709", True, "bilinear", "Y" if ch == "Y" else ch)


def _finish(v, colour, dt, ch, mean, std):
    """the values the tensor holds, [h, w, C'] float64: the output scale of include/h264bsd_mi355x.h, alpha appended.  U8: the value
    on the 0 .. 255 scale after the clamp and BEFORE the rounding, which is _check's (REF halves up, otherwise halves to even)"""
    C = v.shape[2]
    m, s = np.asarray(mean[:C], np.float64), np.asarray(std[:C], np.float64)
    if colour == "reference":
        out = np.clip(v, 0, 255) if dt == "u8" else (v / 255 - m) / s
    else:
        out = np.clip(np.round(255 * v, 9), 0, 255) if dt == "u8" else (v - m) / s
    if ch in ("RGBA", "BGRA"):
        out = np.concatenate([out, np.full(out.shape[:2] + (1,), 255.0 if dt == "u8" else 1.0)], axis=2)
    return out


def _tol(colour, dt, std):
    """f32 (and the fp32 part of f16): REF 2e-3 on the 0..255 scale, colour 1e-5 on the [0, 1] scale, scaled by 1 / std.  U8: the
    same number on the 0..255 scale (std is 1), the eps of the rounding rule: what the float32 pull of the same configuration is
    held to, so a uint8 value further than this from a half-integer cannot legitimately round the other way"""
    base = 2e-3 / 255 if colour == "reference" else 1e-5
    return base * (255 if dt == "u8" else 1) / min(abs(x) for x in std)


def _tol_bilinear_ref(dt, std):
    """the tighter bound of the reference colour's bilinear without antialiasing: 1e-4 on the 0..255 scale"""
    return 1e-4 / 255 * (255 if dt == "u8" else 1) / min(abs(x) for x in std)


def _check(got, want, dt, tol, what="", half_up=False, shares=None):
    """got: [h, w, C'] float64 from the tensor, want: _finish's.  f32 within tol.  U8 and f16 under tests/rounding_model.py's rule
    with eps = tol: equal to want rounded (U8: halves up when half_up, the reference colour, else to even; f16: to nearest even)
    wherever want lies further than tol from a rounding boundary, elsewhere U8 within 1 and f16 within one f16 ulp + tol.  The decided
    share is printed and appended to shares[dt] for the caller's rd.check_share"""
    assert got.shape == want.shape, what
    if dt == "f32":
        d = np.abs(got - want)
        assert d.max() <= tol, (what, d.max(), tol)
        return
    share = rd.check_u8(got, want, tol, half_up, what) if dt == "u8" else rd.check_f16(got, want, tol, tol, what)
    if shares is not None:
        shares.setdefault(dt, []).append(share)


def _check_shares(shares, what):
    for dt in ("u8", "f16"):
        rd.check_share(shares.get(dt), dt, what)


def _hwc(t, lay):
    g = t.cpu().double().numpy()
    return g.transpose(1, 2, 0) if lay == "NCHW" else g


def _pull(built, decs, dt, lay, ch, size, filt, colour, fit="stretch", pad=(0.0, 0.0, 0.0), **kw):
    mode, aa = FILTERS[filt]
    norm = dict(mean=IMAGENET_MEAN, std=IMAGENET_STD) if dt != "u8" else {}
    col = {} if colour == "reference" else dict(colour="bt709", colour_range="full", chroma="bilinear")
    return built.pull_tensor(decs, size=size, layout=lay, dtype=_torch_dtype(dt), channels=ch, crop=True, mode=mode, antialias=aa,
                             fit=fit, pad=pad, return_boxes=True, **norm, **col, **kw)


STRETCH = [("f32", "NCHW", "RGB", (224, 224)), ("u8", "NHWC", "RGBA", (257, 333)), ("f16", "NCHW", "BGR", (720, 1280)),
           ("f32", "NHWC", "Y", (8, 8)), ("u8", "NCHW", "Y", (224, 224)), ("f16", "NHWC", "BGRA", (257, 333)),
           ("f32", "NHWC", "RGB", (720, 1280)), ("u8", "NCHW", "RGB", (8, 8))]


@pytest.mark.parametrize("colour", ["reference", "bt709"])
@pytest.mark.parametrize("filt", ["bilinear", "bilinear_aa", "bicubic_aa"])
def test_stretch_matches_the_model(built, filt, colour):
    """four decoders of different frame sizes per call, every configuration of STRETCH, against torch's weights (antialiased, or
    bilinear without antialiasing: k_tensor_resize) applied in float64 to the oracle's (REF) or the colour model's values of the
    twin decoders' host pictures; uint8 and float16 pinned in their rounding (_check)"""
    names = _streams()
    shares = {}
    feeds, refs = [Feed(built, d) for d in names], [Feed(built, d) for d in names]
    for k, (dt, lay, ch, size) in enumerate(STRETCH):
        for f in feeds + refs:
            assert f.step()
        pics = [r.dec.next_output_picture() for r in refs]
        t, got, ids, _, _, boxes = _pull(built, [f.dec for f in feeds], dt, lay, ch, size, filt, colour)
        assert got == [1] * 4 and ids == [p[1] for p in pics]
        assert boxes == [(0, 0, size[1], size[0])] * 4
        std = IMAGENET_STD if dt != "u8" else (1, 1, 1)
        for i, (p, r) in enumerate(zip(pics, refs)):
            v = rm.resample_hwc(_source(p[0], _geometry(r.dec, True), colour, ch), size, filt, fma=colour == "reference")
            want = _finish(v, colour, dt, ch, IMAGENET_MEAN, std)
            tol = _tol_bilinear_ref(dt, std) if colour == "reference" and filt == "bilinear" else _tol(colour, dt, std)
            # 720 x 1280 is a rational scale of every stream (1/2, 3/2): values pile onto exact halves; the rule holds, the share does not count
            _check(_hwc(t[i], lay), want, dt, tol, what=("stretch", filt, colour, k, i, dt, lay, ch, size), half_up=colour == "reference",
                   shares=shares if size != (720, 1280) else None)
    _check_shares(shares, ("stretch", filt, colour))
    for f in feeds + refs:
        f.close()


@pytest.mark.parametrize("colour", ["reference", "bt709"])
@pytest.mark.parametrize("filt", ["bilinear", "bilinear_aa", "bicubic_aa"])
def test_letterbox_mixes_aspect_ratios(built, filt, colour):
    """one call over 16:9 (1080p) and a 3:2 synthetic stream into 320 x 320 and 256 x 512: the boxes are the model's, the inner
    rectangle is the window resampled to (ih, iw), the border is the normalised pad exactly"""
    import torch
    names = ["test_1920x1080", _synthetic(6, 4, seed=11), "test_640x360"]
    feeds, refs = [Feed(built, d) for d in names], [Feed(built, d) for d in names]
    pad = (0.25, 114 / 255, 1.0)
    shares = {}
    for k, (dt, lay, ch, size) in enumerate([("f32", "NCHW", "RGB", (320, 320)), ("u8", "NHWC", "BGR", (256, 512)),
                                             ("f16", "NHWC", "RGBA", (320, 320)), ("f32", "NHWC", "Y", (256, 512))]):
        for f in feeds + refs:
            assert f.step()
        pics = [r.dec.next_output_picture() for r in refs]
        t, got, _, _, _, boxes = _pull(built, [f.dec for f in feeds], dt, lay, ch, size, filt, colour, fit="letterbox", pad=pad)
        assert got == [1] * 3
        std = IMAGENET_STD if dt != "u8" else (1, 1, 1)
        mean = IMAGENET_MEAN if dt != "u8" else (0, 0, 0)
        for i, (p, r) in enumerate(zip(pics, refs)):
            geo = _geometry(r.dec, True)
            left, top, iw, ih = rm.letterbox(size[1], size[0], geo[4], geo[5])
            assert boxes[i] == (left, top, iw, ih), (k, i)
            g = _hwc(t[i], lay)
            v = rm.resample_hwc(_source(p[0], geo, colour, ch), (ih, iw), filt, fma=colour == "reference")
            tol = _tol_bilinear_ref(dt, std) if colour == "reference" and filt == "bilinear" else _tol(colour, dt, std)
            _check(g[top:top + ih, left:left + iw], _finish(v, colour, dt, ch, mean, std), dt, tol, what=("letterbox", filt, colour, k, i, dt),
                   half_up=colour == "reference", shares=shares)
            border = np.ones(g.shape[:2], bool)
            border[top:top + ih, left:left + iw] = False
            assert border.any()
            C = 1 if ch == "Y" else 3
            want = [rm.pad_value(pad[c], dt, mean[c], std[c]) for c in range(C)]
            want = torch.tensor(want, dtype=torch.float32).to(_torch_dtype(dt)).double().numpy()
            if ch in ("RGBA", "BGRA"):
                want = np.append(want, 255.0 if dt == "u8" else 1.0)
            assert (g[border] == want[None, :]).all(), (k, i, np.unique(g[border], axis=0)[:4], want)
    _check_shares(shares, ("letterbox", filt, colour))
    for f in feeds + refs:
        f.close()


def _pull_c(built, fn, decs, dt, lay, ch, size, colour, resize, box=None):
    """one call of the C entry point `fn` ("colour" or "resize"), into a fresh tensor; returns (tensor, got)"""
    import torch
    L = built.api_lib()
    n = len(decs)
    C = dict(RGB=3, BGR=3, RGBA=4, BGRA=4, Y=1)[ch]
    H, W = size
    out = torch.full((n, C, H, W) if lay == "NCHW" else (n, H, W, C), 7, dtype=_torch_dtype(dt), device="cuda")
    torch.cuda.synchronize()
    mean, std = (IMAGENET_MEAN, IMAGENET_STD) if dt != "u8" else ((0, 0, 0), (1, 1, 1))
    spec = built.TensorSpec(out.data_ptr(), W, H, built.capi.LAYOUTS[lay], list(DTYPES).index(dt), built.capi.CHANNELS[ch][0], 1, 1,
                            (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std))
    got = (ctypes.c_uint32 * n)()
    VP = ctypes.c_void_p * n
    cs = None if colour is None else ctypes.byref(colour)
    if fn == "colour":
        rc = L.h264bsdmiNextOutputTensorBatchColour(n, VP(*[d._st for d in decs]), ctypes.byref(spec), cs, None, got, None, None, None)
    else:
        rc = L.h264bsdmiNextOutputTensorBatchResize(n, VP(*[d._st for d in decs]), ctypes.byref(spec), cs,
                                                    None if resize is None else ctypes.byref(resize), None, got, None, None, None, box)
    assert rc == 0
    torch.cuda.synchronize()
    return out, list(got)


@pytest.mark.parametrize("colour", [None, (3, 2, 1, 0)])
@pytest.mark.parametrize("dt", ["u8", "f16", "f32"])
def test_null_and_bilinear_stretch_are_the_colour_entry_point(built, dt, colour):
    """resize = NULL and {FILTER_BILINEAR, FIT_STRETCH} give h264bsdmiNextOutputTensorBatchColour's bytes, on twin decoders"""
    import torch
    cs = None if colour is None else built.ColourSpec(*colour)
    for lay, ch in [("NCHW", "RGB"), ("NHWC", "BGRA"), ("NCHW", "Y")]:
        feeds = [Feed(built, "test_640x360") for _ in range(3)]
        for rnd in range(2):
            for f in feeds:
                assert f.step()
            box = (ctypes.c_uint32 * 4)()
            a, ga = _pull_c(built, "colour", [feeds[0].dec], dt, lay, ch, (224, 224), cs, None)
            b, gb = _pull_c(built, "resize", [feeds[1].dec], dt, lay, ch, (224, 224), cs, None)
            c, gc = _pull_c(built, "resize", [feeds[2].dec], dt, lay, ch, (224, 224), cs, built.ResizeSpec(0, 0, (ctypes.c_float * 3)(1, 1, 1)),
                            box)
            assert ga == gb == gc == [1] and list(box) == [0, 0, 224, 224]
            assert torch.equal(a, b) and torch.equal(a, c), (lay, ch, rnd)
        for f in feeds:
            f.close()


def test_got_mask_slices_stay_untouched_and_boxes_are_zero(built):
    """an instance without a picture (no stream fed yet) leaves its slice of a sentinel tensor untouched, border included"""
    import torch
    feed, empty = Feed(built, "test_640x360"), Feed(built, "test_640x360")
    assert feed.step()
    out = torch.full((2, 3, 96, 160), -5.0, dtype=torch.float32, device="cuda")
    _, got, _, _, _, boxes = built.pull_tensor([empty.dec, feed.dec], size=(96, 160), dtype=torch.float32, out=out, mode="bicubic",
                                               antialias=True, fit="letterbox", pad=(0.5, 0.5, 0.5), return_boxes=True)
    torch.cuda.synchronize()
    assert got == [0, 1] and boxes == [None, (0, 3, 160, 90)]
    assert (out[0] == -5).all()
    assert (out[1, :, :3] == 0.5).all() and (out[1, :, 93:] == 0.5).all() and (out[1] != -5).all()
    feed.close()
    empty.close()


def test_refused_batch_pops_nothing(built):
    """a repeated instance refuses the whole call: nothing is popped, and the next good call gives the same picture as a twin's"""
    import torch
    a, twin = Feed(built, "test_640x360"), Feed(built, "test_640x360")
    assert a.step() and twin.step()
    with pytest.raises(RuntimeError):
        built.pull_tensor([a.dec, a.dec], size=(64, 64), mode="bicubic", antialias=True, fit="letterbox")
    x = built.pull_tensor([a.dec], size=(64, 64), mode="bicubic", antialias=True, fit="letterbox")
    y = built.pull_tensor([twin.dec], size=(64, 64), mode="bicubic", antialias=True, fit="letterbox")
    torch.cuda.synchronize()
    assert x[1] == y[1] == [1] and x[2] == y[2] and torch.equal(x[0], y[0])
    a.close()
    twin.close()


def test_pull_on_a_torch_stream_is_ordered_before_later_decoding(built):
    """an antialiased letterbox pull enqueued on a torch side stream, followed without synchronisation by more decoding and
    h264bsdmiFlushAsync of the same instances (frame-buffer slots come round again), gives what a synchronous pull of twins gives"""
    import torch
    name = "test_1920x1080"
    N = 3
    feeds, twins = [Feed(built, name) for _ in range(N)], [Feed(built, name) for _ in range(N)]
    L = built.api_lib()
    side = torch.cuda.Stream()
    kw = dict(size=(320, 320), dtype=torch.float16, mean=IMAGENET_MEAN, std=IMAGENET_STD, mode="bilinear", antialias=True,
              fit="letterbox", pad=(0.5, 0.5, 0.5), colour="bt709", chroma="bilinear")
    for rnd in range(2):
        for f in feeds + twins:
            assert f.step()
        out = torch.empty((N, 3, 320, 320), dtype=torch.float16, device="cuda")
        torch.cuda.synchronize()
        _, got, _, _, _ = built.pull_tensor([f.dec for f in feeds], out=out, stream=side, **kw)
        assert got == [1] * N
        for _ in range(8):
            for f in feeds:
                assert f.step()
            assert L.h264bsdmiFlushAsync() == 0
            for f in feeds:
                f.dec.next_output_picture()
        sync, got2, _, _, _ = built.pull_tensor([t.dec for t in twins], stream=torch.cuda.default_stream(), **kw)
        torch.cuda.synchronize()
        assert got2 == [1] * N
        assert torch.equal(out, sync), rnd
        for _ in range(8):
            for t in twins:
                assert t.step()
                t.dec.next_output_picture()
    for f in feeds + twins:
        f.close()


def test_256_1080p_instances_in_one_call(built):
    """256 x 1080p, BILINEAR_AA to 224 x 224 f16 ImageNet-normalised in one call: every slice equals the model of the picture"""
    import torch
    N = 256
    decs = [built.Decoder(no_output_reordering=1) for _ in range(N)]
    data = stream_bytes("test_1920x1080")
    drv = built.BatchDriver(decs, [data] * N)
    ref = Feed(built, "test_1920x1080")
    for rnd in range(2):
        assert len(drv.step()) == N
        assert ref.step()
        frame = ref.dec.next_output_picture()[0]
        t, got, _, _, _ = built.pull_tensor(decs, size=224, dtype=torch.float16, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                                            mode="bilinear", antialias=True)
        torch.cuda.synchronize()
        assert got == [1] * N
        want = _finish(rm.resample_hwc(_source(frame, _geometry(ref.dec, True), "reference", "RGB"), (224, 224), "bilinear_aa"),
                       "reference", "f16", "RGB", IMAGENET_MEAN, IMAGENET_STD)
        first = t[0]
        _check(_hwc(first, "NCHW"), want, "f16", _tol("reference", "f16", IMAGENET_STD), what=("256 x 1080p", rnd), half_up=True)
        for i in range(1, N):
            assert torch.equal(t[i], first), (rnd, i)
    for d in decs:
        d.close()
    ref.close()
