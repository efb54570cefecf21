"""GPU: h264bsdmiOutputTensorRemap / pull_remap — current pictures sampled through coordinate maps, each map into its own slice of
one tensor.  Expected values come from a twin decoder's host picture through the oracle's conversion (REFERENCE) or
tests/colour_model.py (BT.709 full range, bilinear chroma) and the float64 model of tests/remap_model.py; from the other tensor
kernels where equality with them is the point (identity, integer translations, rotation by 90 degrees)."""
import numpy as np
import pytest

import region_model as gm
import remap_model as mm
from h264writer import StreamWriter
from test_gpu_tensor_colour import Feed, _geometry
from test_gpu_tensor_regions import PAD, IdFeed, Sources, _border_values, _norm, _open, _pop_all
from test_gpu_tensor_resize import (IMAGENET_MEAN, IMAGENET_STD, STRETCH, _check, _check_shares, _finish, _hwc, _source, _streams,
                                    _synthetic, _tol, _torch_dtype)

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (9, 33), (40, 64)]         # (H, W): 8 x 8, 33 x 9 (ragged in both tile directions), 64 x 40
CONFIGS = [("f32", "NCHW", "RGB"), ("f16", "NHWC", "BGRA"), ("u8", "NHWC", "Y"), ("u8", "NCHW", "RGB"), ("f16", "NCHW", "Y"),
           ("f32", "NHWC", "BGRA")]


@pytest.fixture(autouse=True, scope="module")
def _through_the_product_library(built):
    built.use_product_library(True)
    yield
    built.use_product_library(False)


@pytest.fixture(autouse=True)
def _no_device_errors(built):
    yield
    assert built.device_errors() == 0


def _col(colour):
    return {} if colour == "reference" else dict(colour="bt709", colour_range="full", chroma="bilinear")


def _dev(m):
    import torch
    return torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).cuda()


def _remap(built, decs, maps, dt, lay, ch, colour, mode="bilinear", border="constant", pad=PAD, **kw):
    """maps: numpy [H, W, 2] arrays or device tensors"""
    import torch
    mean, std = _norm(dt)
    maps = [m if isinstance(m, torch.Tensor) else _dev(m) for m in maps]
    torch.cuda.synchronize()                # the maps are complete on every stream
    res = built.pull_remap(decs, maps, layout=lay, dtype=_torch_dtype(dt), channels=ch, mean=mean, std=std, mode=mode, border=border,
                           pad=pad, **_col(colour), **kw)
    torch.cuda.synchronize()
    return res


def _check_map(g, v, m, dt, ch, colour, mode, border, pad, what, shares=None):
    """g: [H, W, C'] float64 of one slice; v: the converted window; m: the float32 map.  f32 within the project's tolerance of the
    model; U8 and f16 under tests/rounding_model.py's rule (test_gpu_tensor_resize._check): U8 equal to the model rounded (REF halves
    up, otherwise to even) except where the model's own value lies within 2e-3 of a rounding boundary (there within 1), f16 equal
    to the model rounded to nearest even except within the tolerance of a midpoint; the padded pixels (non-finite coordinates) the
    normalised pad exactly"""
    mean, std = _norm(dt)
    ref = colour == "reference"
    s, padded = mm.remap(v, m, mode, border, gm.sample_pad(pad, ref), fma=ref)
    want = _finish(s, colour, dt, ch, mean, std)
    border_values = _border_values(dt, ch, pad)
    want[padded] = border_values
    # U8: 2e-3 on the 0..255 scale for both colours — what this comparison has always held the matrix colours to (_tol gives 2.55e-3)
    _check(g, want, dt, 2e-3 if dt == "u8" else _tol(colour, dt, std), what=what, half_up=ref, shares=shares)
    if padded.any():
        assert (g[padded] == border_values[None, :]).all(), (what, "padded")


def _identity(h, w, dx=0, dy=0):
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.stack([j + dx, i + dy], axis=-1).astype(np.float32)


@pytest.mark.parametrize("colour", ["reference", "bt709"])
def test_identity_map_is_pull_tensor_bit_for_bit(built, colour):
    """mx = j, my = i at the window's size against pull_tensor(mode="bilinear") of a twin at that size, every dtype x layout x
    channels of STRETCH, on 640x360 and on the cropped synthetic stream"""
    import torch
    for name in ("test_640x360", _streams()[3]):
        feed = Feed(built, name)
        assert feed.step()
        _, _, _, _, w, h = _geometry(feed.dec, True)
        ident = _dev(_identity(h, w))
        for k, (dt, lay, ch, _) in enumerate(STRETCH):
            mean, std = _norm(dt)
            twin = Feed(built, name)
            assert twin.step()
            want, got2 = built.pull_tensor([twin.dec], size=(h, w), layout=lay, dtype=_torch_dtype(dt), channels=ch, mean=mean, std=std,
                                           mode="bilinear", **_col(colour))[:2]
            t, got, cur, ids = _remap(built, [feed.dec], [ident], dt, lay, ch, colour, pop=k == 0)
            assert got == got2 == [1] and cur == [1]
            assert torch.equal(t, want), (name if isinstance(name, str) else "synthetic", dt, lay, ch, int((t != want).sum()))
            for border in ("replicate",):
                t2 = _remap(built, [feed.dec], [ident], dt, lay, ch, colour, border=border)[0]
                assert torch.equal(t2, want), (dt, lay, ch, border)
            twin.close()
        feed.close()


@pytest.mark.parametrize("colour", ["reference", "bt709"])
def test_integer_translations_are_pull_regions_bit_for_bit(built, colour):
    """negative offsets and overhang on all four sides: the same box through pull_regions at scale 1 (bilinear, stretch, same pad)"""
    import torch
    names = ["test_640x360", _streams()[3]]
    feeds = [Feed(built, d) for d in names]
    for f in feeds:
        assert f.step() and f.dec.next_output_info() is not None
    decs = [f.dec for f in feeds]
    for (H, W) in SIZES:
        offsets = []
        for i, f in enumerate(feeds):
            _, _, _, _, w, h = _geometry(f.dec, True)
            offsets += [(i, dx, dy) for dx, dy in ((-5, -3), (w - W // 2, h - H // 2), (-W + 2, 7), (11, -H + 1), (w - 3, -2), (3, h - 1),
                                                   (17, 9), (-W - 4, 5), (w, h))]
        maps = [_identity(H, W, dx, dy) for _, dx, dy in offsets]
        regions = [(i, dx, dy, W, H) for i, dx, dy in offsets]
        for dt, lay, ch in CONFIGS[:4]:
            mean, std = _norm(dt)
            want, gotr = built.pull_regions(decs, regions, (H, W), layout=lay, dtype=_torch_dtype(dt), channels=ch, mean=mean, std=std,
                                            mode="bilinear", fit="stretch", pad=PAD, **_col(colour))[:2]
            t, got, _, _ = _remap(built, decs, maps, dt, lay, ch, colour, instances=[i for i, _, _ in offsets])
            assert got == gotr == [1] * len(offsets)
            assert torch.equal(t, want), ((H, W), dt, lay, ch, [int((t[r] != want[r]).sum()) for r in range(len(offsets))])
    for f in feeds:
        f.close()


@pytest.mark.parametrize("colour", ["reference", "bt709"])
def test_rotation_by_90_degrees_is_rot90_of_the_region(built, colour):
    """affine_maps of a quarter turn about a box: torch.rot90 of the region pull of that box, exactly"""
    import torch
    feed = Feed(built, "test_640x360")
    assert feed.step() and feed.dec.next_output_info() is not None
    for x, y, bw, bh in ((101, 51, 33, 9), (600, 340, 64, 40), (-3, -2, 8, 8)):
        theta = [[[0, -1, x + bw - 1], [1, 0, y]]]          # output (i, j) of bw rows x bh columns <- source (x + bw - 1 - i, y + j)
        maps = built.affine_maps(theta, (bw, bh))
        for dt, lay, ch in CONFIGS[:4]:
            mean, std = _norm(dt)
            box = built.pull_regions([feed.dec], [(0, x, y, bw, bh)], (bh, bw), layout=lay, dtype=_torch_dtype(dt), channels=ch, mean=mean,
                                     std=std, mode="bilinear", pad=PAD, **_col(colour))[0]
            t, got, _, _ = _remap(built, [feed.dec], maps, dt, lay, ch, colour)
            dims = (2, 3) if lay == "NCHW" else (1, 2)
            assert got == [1] and torch.equal(t, torch.rot90(box, 1, dims)), ((x, y, bw, bh), dt, lay, ch)
    feed.close()


@pytest.mark.parametrize("colour", ["reference", "bt709"])
@pytest.mark.parametrize("border", ["constant", "replicate"])
def test_barrel_distortion_matches_the_model(built, border, colour):
    """fractional coordinates that reach 5 samples outside the window, both filters, on 640x360 and the cropped synthetic stream"""
    names = ["test_640x360", _streams()[3]]
    feeds, refs = _open(built, names)
    pics = _pop_all(feeds, refs)
    src = Sources(pics, [r.dec for r in refs])
    wins = [_geometry(r.dec, True)[4:] for r in refs]
    shares = {"bilinear": {}, "nearest": {}}
    for (H, W) in SIZES:
        maps = [mm.barrel(H, W, w, h) for (w, h) in wins]
        assert all(m[:, :, 0].min() < -4.5 and m[:, :, 0].max() > w + 3.5 for m, (w, h) in zip(maps, wins))
        for mode in ("bilinear", "nearest"):
            for dt, lay, ch in CONFIGS:
                t, got, cur, ids = _remap(built, [f.dec for f in feeds], maps, dt, lay, ch, colour, mode, border)
                assert got == [1, 1] and cur == [1, 1] and ids == [p[1] for p in pics]
                for i in range(2):
                    _check_map(_hwc(t[i], lay), src.get(i, colour, ch), maps[i], dt, ch, colour, mode, border, PAD,
                               what=("remap", mode, colour, (H, W), border, dt, lay, ch, i), shares=shares[mode])
    for mode in shares:
        _check_shares(shares[mode], ("remap", mode, border, colour))
    for f in feeds + refs:
        f.close()


def _special_map(H, W, w, h):
    """fractional coordinates inside, then one run of special x values along a row and of special y values along a column"""
    rng = np.random.default_rng(7)
    m = np.stack([rng.uniform(0, w - 1, (H, W)), rng.uniform(0, h - 1, (H, W))], axis=-1).astype(np.float32)

    def specials(n):
        return [np.nan, np.inf, -np.inf, 1e30, -1e30, -1, -0.5, n - 1, n - 0.5, n, 0.5, 10.5, n - 1.5, -1e-8, -0.3, n - 1 + 1e-3]

    xs, ys = specials(w), specials(h)
    m[1, :len(xs), 0] = xs
    m[2, :len(xs), 0] = xs
    m[2, :len(xs), 1] = h - 1                       # the special x values on the window's last row
    m[3:3 + min(len(ys), H - 3), 3, 1] = ys[:H - 3]
    m[0, :len(ys), 1] = ys
    m[0, :len(ys), 0] = np.arange(len(ys)) + 0.5
    m[4, 4] = (np.nan, np.nan)
    m[4, 5] = (-1, -1)
    m[4, 6] = (w, h)
    m[4, 7] = (-0.5, -0.5)
    m[4, 8] = (w - 0.5, h - 0.5)
    m[4, 9] = (w - 1, h - 1)
    m[4, 10] = (1e30, -1e30)
    m[4, 11] = (np.inf, 3)
    return m


@pytest.mark.parametrize("colour", ["reference", "bt709"])
def test_special_values(built, colour):
    """NaN, the infinities, +-1e30, exactly -1, -0.5, W - 1, W - 0.5, W and x.5 positions in one map: the model's values, the padded
    pixels the normalised pad exactly, no device error"""
    feeds, refs = _open(built, ["test_640x360", _streams()[3]])
    pics = _pop_all(feeds, refs)
    src = Sources(pics, [r.dec for r in refs])
    wins = [_geometry(r.dec, True)[4:] for r in refs]
    maps = [_special_map(9, 33, w, h) for (w, h) in wins]
    for border in ("constant", "replicate"):
        for mode in ("bilinear", "nearest"):
            for dt, lay, ch in CONFIGS[:4]:
                t, got, _, _ = _remap(built, [f.dec for f in feeds], maps, dt, lay, ch, colour, mode, border)
                assert got == [1, 1]
                for i in range(2):
                    _check_map(_hwc(t[i], lay), src.get(i, colour, ch), maps[i], dt, ch, colour, mode, border, PAD,
                               what=(mode, border, dt, lay, ch, i))
    assert built.device_errors() == 0
    for f in feeds + refs:
        f.close()


def test_four_frame_sizes_share_one_map_and_one_decoder_takes_two(built):
    """four decoders of different frame sizes through ONE map, two more maps on the first, and a decoder without a current picture: got = 0 and
    its slice's sentinel bytes intact; current / picId as the region call reports them; the call repeated gives identical bytes"""
    import torch
    feeds, refs = _open(built, ["test_640x360", _streams()[3], _synthetic(8, 5, seed=5), _synthetic(11, 7, crop=(0, 1, 2, 0), seed=9)])
    pics = _pop_all(feeds, refs)
    assert len({_geometry(r.dec, True)[4:] for r in refs}) == 4
    idle = Feed(built, "test_640x360")
    assert idle.step()                                   # decoded, not popped: no current picture
    src = Sources(pics, [r.dec for r in refs])
    H, W = 40, 64
    shared = mm.barrel(H, W, 96, 64, reach=3.0)          # over the smallest window, and the top-left corner of the others
    own = [_identity(H, W, 301, 155) * np.float32(1.0) + np.float32(0.25), mm.barrel(H, W, 640, 360)]
    d_shared, d_own = _dev(shared), [_dev(m) for m in own]
    maps = [d_shared, d_shared, d_own[0], d_shared, d_shared, d_shared, d_own[1]]
    np_maps = [shared, shared, own[0], shared, shared, shared, own[1]]
    inst = [0, 1, 0, 2, 4, 3, 0]
    decs = [f.dec for f in feeds] + [idle.dec]
    for dt, lay, ch, colour in (("f32", "NCHW", "RGB", "reference"), ("u8", "NHWC", "BGRA", "bt709"), ("f16", "NHWC", "Y", "bt709")):
        C = dict(RGB=3, BGRA=4, Y=1)[ch]
        sentinel = torch.full((7, C, H, W) if lay == "NCHW" else (7, H, W, C), 7, dtype=_torch_dtype(dt), device="cuda")
        out = sentinel.clone()
        t, got, cur, ids = _remap(built, decs, maps, dt, lay, ch, colour, instances=inst, out=out)
        assert got == [1, 1, 1, 1, 0, 1, 1] and cur == [1, 1, 1, 1, 0] and ids == [p[1] for p in pics] + [0]
        regions = built.pull_regions(decs, [(i, 0, 0, 8, 8) for i in range(5)], 8)
        assert regions[3:] == (cur, ids)
        assert torch.equal(out[4], sentinel[4])
        for r, i in enumerate(inst):
            if i != 4:
                _check_map(_hwc(t[r], lay), src.get(i, colour, ch), np_maps[r], dt, ch, colour, "bilinear", "constant", PAD, what=(dt, r))
        again = _remap(built, decs, maps, dt, lay, ch, colour, instances=inst, out=sentinel.clone())
        assert torch.equal(again[0], out) and again[1:] == (got, cur, ids)
    for f in feeds + refs + [idle]:
        f.close()


def test_remap_on_a_busy_side_stream_is_fenced_against_the_next_decode(built):
    """a remap enqueued on a side stream that is still busy, the next pictures of every instance decoded and pulled at once (the
    frame-buffer slots come round again): the tensor is the one twins give with the library's own stream"""
    import torch
    name, N = "test_640x360", 3
    feeds, twins = [Feed(built, name) for _ in range(N)], [Feed(built, name) for _ in range(N)]
    side = torch.cuda.Stream()
    maps = _dev(np.stack([mm.barrel(40, 64, 640, 360), _identity(40, 64, 300, 200) + np.float32(0.5), mm.barrel(40, 64, 320, 180)]))
    kw = dict(dtype=torch.float16, mean=IMAGENET_MEAN, std=IMAGENET_STD, pad=PAD, colour="bt709", chroma="bilinear")
    big = torch.randn(2048, 2048, device="cuda")
    for rnd in range(2):
        for f in feeds + twins:
            assert f.step() and f.dec.next_output_info() is not None
        out = torch.empty((N, 3, 40, 64), dtype=torch.float16, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(20):
                big = (big @ big).clamp_(-1, 1)             # keeps the side stream busy while the host runs ahead
        _, got, cur, _ = built.pull_remap([f.dec for f in feeds], maps, out=out, stream=side, **kw)
        assert got == [1] * N and cur == [1] * N
        later = []
        for _ in range(8):
            for f in feeds:
                assert f.step()
            later.append(built.pull_tensor([f.dec for f in feeds], size=(64, 64), dtype=torch.float16)[0])
        want = built.pull_remap([t.dec for t in twins], maps, stream=torch.cuda.default_stream(), **kw)[0]
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


def test_24_decoders_in_one_call(built):
    """23 decoders on 640x360 and one on 1080p through one shared 64 x 40 map: the first and the 1080p slice against the model, the
    other 640x360 slices equal to the first"""
    import torch
    names = ["test_640x360"] * 23 + ["test_1920x1080"]
    feeds = [Feed(built, d) for d in names]
    refs = [Feed(built, "test_640x360"), Feed(built, "test_1920x1080")]
    for f in feeds:
        assert f.step()
    for r in refs:
        assert r.step()
    pics = [r.dec.next_output_picture() for r in refs]
    m = mm.barrel(40, 64, 700, 420, reach=4.0)           # beyond 640x360 on the right and below, inside 1080p
    t, got, cur, ids = _remap(built, [f.dec for f in feeds], [_dev(m)] * 24, "f16", "NCHW", "RGB", "reference", pop=True)
    assert got == [1] * 24 and cur == [1] * 24 and ids == [pics[0][1]] * 23 + [pics[1][1]]
    for r, k in ((0, 0), (1, 23)):
        v = _source(pics[r][0], _geometry(refs[r].dec, True), "reference", "RGB")
        _check_map(_hwc(t[k], "NCHW"), v, m, "f16", "RGB", "reference", "bilinear", "constant", PAD, what=k)
    for k in range(1, 23):
        assert torch.equal(t[k], t[0]), k
    assert not torch.equal(t[23], t[0])
    for f in feeds + refs:
        f.close()


def test_pop_returns_the_pictures_in_output_order(built):
    """pop=True on a stream whose output order differs from its decode order: every call pops the next picture in OUTPUT order and
    samples it, whichever frame buffer it lies in"""
    from synth_configs import CONFIGS as SYNTH
    data = StreamWriter(**SYNTH["poc0_display_reorder"]).build()
    feed, twin = IdFeed(built, data, reorder=True), IdFeed(built, data, reorder=True)
    order = []
    m = None

    def drain():
        nonlocal m
        while True:
            pic = twin.dec.next_output_picture()
            if pic is None:
                assert feed.dec.next_output_info() is None
                return
            if m is None:
                _, _, _, _, w, h = _geometry(twin.dec, True)
                m = mm.barrel(9, 33, w, h)
            t, got, cur, ids = _remap(built, [feed.dec], [m], "f32", "NCHW", "RGB", "reference", pop=True)
            assert got == [1] and cur == [1] and ids == [pic[1]]
            v = _source(pic[0], _geometry(twin.dec, True), "reference", "RGB")
            _check_map(_hwc(t[0], "NCHW"), v, m, "f32", "RGB", "reference", "bilinear", "constant", PAD, what=pic[1])
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
