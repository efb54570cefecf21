"""GPU: the pixel-consuming kernels on pictures whose samples the test chose (tests/pcm_pictures.py: all-I_PCM streams), through the
product library.

The cube: two 4096 x 2048 pictures that hold every (Y, Cb, Cr) triple once.  Every path that applies the reference's integer BT.601
conversion must give, for all 2^24 triples, the bytes of pyoracle.oracle_convert — which tests/test_pcm_pictures.py pins to the
reference's formula and to the compiled reference on the same pictures — never those of a sibling kernel.  The matrix colours are held
to tests/colour_model.py in float64 on the same triples.  Saturated pictures (all 0, all 255) of the largest legal frame take the
integer statistics to their extremes and the fold loops into their second pass; hard 0 / 255 edges take the resampling kernels past
0 and 255."""
import numpy as np
import pytest

import cells_model as clm
import change_model as chm
import colour_model as cm
import pcm_pictures as pp
import resize_model as rm
import stats_model as sm
import test_gpu_tensor_resize as tr
from oracle import pyoracle
from test_gpu_cell_maps import CHANGE_PLANES, PICTURE_PLANES
from test_gpu_cell_maps import _equal as _cells_equal
from test_gpu_region_change import _equal as _change_equal
from test_gpu_region_stats import _equal as _stats_equal
from test_gpu_tensor_colour import COMBOS, IMAGENET_MEAN, IMAGENET_STD, Feed, _check

pytestmark = pytest.mark.gpu

CW, CH = 4096, 2048                     # the cube pictures
BW, BH = 4096, 2304                     # the largest legal frame: 256 x 144 = 36864 macroblocks
N_BIG = BW * BH
SMALL = dict(W=144, H=80, crop=(1, 2, 1, 3), window=(2, 2, 138, 72))      # 9 x 5 macroblocks, cropped: no cell or tile is aligned
ORDER = dict(RGB=[0, 1, 2], BGR=[2, 1, 0], RGBA=[0, 1, 2, 3], BGRA=[2, 1, 0, 3])


@pytest.fixture(autouse=True, scope="module")
def _through_the_product_library(built):
    built.use_product_library(True)
    yield
    built.use_product_library(False)


@pytest.fixture(autouse=True)
def _no_device_errors(built):
    yield
    assert built.device_errors() == 0


# ------------------------------------------------------------------------------------------------ the cube and who holds it
class Cube:
    """the two pictures, their coded frames, the stream (idc 0: every picture is a filtered one for the engine), and the expected
    bytes: conv[p][fmt], uint32 per pixel, from the oracle"""

    def __init__(self):
        self.pics = pp.cube_pictures()
        self.frames = [pp.i420(p) for p in self.pics]
        self.data = pp.pcm_stream(self.pics, idc=0)
        self.conv = [[pyoracle.oracle_convert(fmt, CW, CH, f) for fmt in range(3)] for f in self.frames]
        self._planes = {}

    def planes(self, p, source):
        if (p, source) not in self._planes:
            self._planes[p, source] = sm.channels(self.frames[p], CW, CH, source)
        return self._planes[p, source]


@pytest.fixture(scope="module")
def cube():
    return Cube()


@pytest.fixture(scope="module")
def cube_dev(cube):
    """(rgba [2, H, W, 4], luma [2, H, W]) uint8 on the device: what the tensor pulls are compared with, where they lie"""
    import torch
    rgba = torch.from_numpy(np.stack([c[0].view(np.uint8).reshape(CH, CW, 4) for c in cube.conv])).cuda()
    luma = torch.from_numpy(np.stack([p[0] for p in cube.pics])).cuda()
    return rgba, luma


def _pop(feed, pictures):
    for _ in range(pictures):
        assert feed.step()
        assert feed.dec.next_output_info() is not None


@pytest.fixture(scope="module")
def current(built, cube, _through_the_product_library):
    """decoders positioned on the cube: on[p] has picture p as its current picture; `changed` has picture 1 as its current and
    picture 0 as its kept picture.  Nothing the tests call on them pops a picture."""
    feeds = [Feed(built, cube.data) for _ in range(3)]
    _pop(feeds[0], 1)
    _pop(feeds[1], 2)
    _pop(feeds[2], 1)
    assert built.keep_pictures([feeds[2].dec])[0] == [1]
    _pop(feeds[2], 1)

    class Current:
        on = [feeds[0].dec, feeds[1].dec]
        changed = feeds[2].dec
    yield Current
    for f in feeds:
        f.close()


def _same(got, want, what):
    """two device tensors, equal; on failure: how many elements differ and where the first ones are"""
    import torch
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    if not torch.equal(got, want):
        ne = got != want
        at = ne.nonzero()[:6]
        raise AssertionError((what, int(ne.sum()), at.tolist(), got[ne][:6].tolist(), want[ne][:6].tolist()))


def _same_np(got, want, what):
    """two uint32 pictures, equal; on failure: how many pixels differ, and the first ones with their position"""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        at = np.flatnonzero(got != want)
        raise AssertionError((what, at.size, [(int(i % CW), int(i // CW), hex(int(got[i])), hex(int(want[i]))) for i in at[:6]]))


def _u8_want(cube_dev, p, lay, ch):
    rgba, luma = cube_dev
    t = luma[p][:, :, None] if ch == "Y" else rgba[p][:, :, ORDER[ch]]
    return t.permute(2, 0, 1) if lay == "NCHW" else t


def _float_want(cube, p, lay, ch):
    """(b / 255 - mean) / std of the oracle's 8-bit values in float64, alpha 1"""
    if ch == "Y":
        v = cube.pics[p][0].astype(np.float64)[:, :, None]
    else:
        v = cube.conv[p][0].view(np.uint8).reshape(CH, CW, 4)[:, :, ORDER[ch][:3]].astype(np.float64)
    C = v.shape[2]
    out = (v / 255 - np.asarray(IMAGENET_MEAN[:C])) / np.asarray(IMAGENET_STD[:C])
    if ch in ("RGBA", "BGRA"):
        out = np.concatenate([out, np.ones(out.shape[:2] + (1,))], axis=2)
    return np.ascontiguousarray(out.transpose(2, 0, 1)) if lay == "NCHW" else out


# ------------------------------------------------------------------------------------------------ 2a: the reference's integer BT.601
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_cube_through_the_converted_output_entry_points(built, cube, fmt):
    """h264bsdNextOutputPictureRGBA / BGRA / YCbCrA, h264bsdmiNextOutputPictureDevice in the same format and the stateless
    h264bsdConvertTo*: all 2^24 triples against the oracle"""
    host, dev = Feed(built, cube.data), Feed(built, cube.data)
    for p in range(2):
        assert host.step() and dev.step()
        want = cube.conv[p][fmt]
        pic = host.dec.next_output_picture_converted(fmt)
        assert pic is not None
        _same_np(pic[0], want, ("host", fmt, p))
        t = dev.dec.next_output_picture_device(fmt)
        assert t is not None and tuple(t[0].shape) == (CH, CW, 4)
        _same_np(t[0].cpu().numpy().reshape(-1).view(np.uint32), want, ("device", fmt, p))
        _same_np(built.convert(fmt, CW, CH, cube.frames[p]), want, ("stateless", fmt, p))
    host.close()
    dev.close()


@pytest.fixture(scope="module")
def cube_jobs(built, cube):
    """the frame jobs of cube picture 0, 1, 0: three ticks, so that both cube pictures have a next tick to be converted in"""
    jobs, _, info = built.capture_stream(pp.pcm_stream(cube.pics + cube.pics[:1], idc=0))
    assert len(jobs) == 3 and (info["width_mbs"], info["height_mbs"]) == (CW // 16, CH // 16)
    return jobs


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_cube_through_the_replay_conversions(built, cube, cube_jobs, fmt):
    """The conversion launch (rep.convert) and the hosted conversion (set_convert, trailing=False) of both cube pictures on two
    replay streams, each against the oracle.  The stream has idc 0, so every tick launches k_frame_dbk, consecutive pictures lie
    in different frame buffers, and rep.convert_timings() reports no conversion launch in the hosted runs (asserted): the hosted
    bytes are the work of the conversion wavefronts inside k_frame_dbk, not of k_convert_rest, which only runs in a tick without
    k_frame_dbk."""
    heads = [pyoracle.blob_header(j) for j in cube_jobs]
    assert all(h["any_deblock"] for h in heads) and heads[0]["cur_slot"] != heads[1]["cur_slot"] != heads[2]["cur_slot"]
    errs_before = built.device_error_events()              # (the replay runs in the harness library: its own engine and counter)
    rep = built.Replay(cube_jobs, n_streams=2)
    try:
        for k in range(2):
            want = cube.conv[k][fmt]
            rep.set_convert(fmt, trailing=False)
            rep.run(0, k + 2); rep.sync()
            _, launches = rep.convert_timings()
            assert launches == 0
            for s in range(2):
                _same_np(rep.fetch_converted(s, CW * CH), want, ("hosted", fmt, k, s))
            rep.set_convert(-1)
            rep.run(0, k + 1)
            rep.convert(heads[k]["cur_slot"], fmt)
            for s in range(2):
                _same_np(rep.fetch_converted(s, CW * CH), want, ("launch", fmt, k, s))
            assert np.array_equal(rep.fetch(1, heads[k]["cur_slot"]), cube.frames[k])
        assert built.device_error_events() == errs_before
    finally:
        rep.close()


@pytest.mark.parametrize("resized", [False, True])
def test_cube_through_the_reference_colour_of_pull_tensor_u8(built, cube, cube_dev, resized):
    """pull_tensor(colour="reference") in uint8, every channel order in both layouts; resized: the same pull with size = (2048, 4096),
    which takes k_tensor_resize and its fp32 map of the reference's coefficients at identity scale.  Exact."""
    import torch
    feeds = [Feed(built, cube.data) for _ in COMBOS]
    for p in range(2):
        for f, (lay, ch) in zip(feeds, COMBOS):
            assert f.step()
            t, got, _, _, _ = built.pull_tensor([f.dec], size=(CH, CW) if resized else None, layout=lay, dtype=torch.uint8, channels=ch)
            assert got == [1]
            _same(t[0], _u8_want(cube_dev, p, lay, ch), (resized, lay, ch, p))
    for f in feeds:
        f.close()


@pytest.mark.parametrize("resized", [False, True])
@pytest.mark.parametrize("dt,lay,ch", [("f32", "NCHW", "RGB"), ("f16", "NHWC", "BGRA"), ("f32", "NHWC", "Y"), ("f16", "NCHW", "BGR")])
def test_cube_through_the_reference_colour_of_pull_tensor_floats(built, cube, dt, lay, ch, resized):
    """float32 and float16 with the ImageNet mean and std, under test_gpu_tensor_colour's _check against (b / 255 - mean) / std of
    the oracle's bytes in float64"""
    import torch
    feed = Feed(built, cube.data)
    for p in range(2):
        assert feed.step()
        t, got, _, _, _ = built.pull_tensor([feed.dec], size=(CH, CW) if resized else None, layout=lay, dtype=getattr(torch, tr.DTYPES[dt]),
                                            channels=ch, mean=IMAGENET_MEAN, std=IMAGENET_STD)
        assert got == [1]
        _check(t[0], _float_want(cube, p, lay, ch), dt, what=(dt, lay, ch, resized, p))
    feed.close()


def test_cube_through_pull_regions_at_identity_scale(built, cube_dev, current):
    """eight 4096 x 256 boxes per picture, two decoders in one call, size = the box: k_tensor_roi at scale 1, uint8, exact"""
    import torch
    regions = [(p, 0, 256 * k, CW, 256) for p in range(2) for k in range(8)]
    for lay, ch in (("NHWC", "RGBA"), ("NCHW", "BGR")):
        t, got, boxes, cur, _ = built.pull_regions(current.on, regions, size=(256, CW), layout=lay, dtype=torch.uint8, channels=ch)
        assert got == [1] * 16 and cur == [1, 1] and boxes == [(0, 0, CW, 256)] * 16
        for r, (p, _, y, _, _) in enumerate(regions):
            want = _u8_want(cube_dev, p, lay, ch)
            want = want[:, y:y + 256] if lay == "NCHW" else want[y:y + 256]
            _same(t[r], want, (lay, ch, r))


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_cube_through_pull_remap_with_an_identity_map(built, cube_dev, current, mode):
    """the identity map over each of the eight 4096 x 256 strips, one map shared by both pictures per call: k_tensor_remap, uint8,
    exact (integer coordinates: every bilinear weight is 0 or 1)"""
    import torch
    j, i = torch.meshgrid(torch.arange(CW, dtype=torch.float32), torch.arange(256, dtype=torch.float32), indexing="xy")
    for k in range(8):
        m = torch.stack([j, i + 256.0 * k], dim=-1).contiguous().cuda()
        t, got, cur, _ = built.pull_remap(current.on, [m, m], instances=[0, 1], layout="NHWC", dtype=torch.uint8, channels="RGB", mode=mode)
        assert got == [1, 1] and cur == [1, 1]
        for p in range(2):
            _same(t[p], _u8_want(cube_dev, p, "NHWC", "RGB")[256 * k:256 * (k + 1)], (mode, k, p))


def _tiling():
    """33 boxes that tile the 4096 x 2048 window: 11 columns x 3 rows, odd origins and sizes, one-sample-wide columns"""
    xs = [0, 1, 130, 515, 1024, 1777, 2048, 2049, 3000, 3583, 4095, 4096]
    ys = [0, 777, 1025, 2048]
    boxes = [(xs[a], ys[b], xs[a + 1] - xs[a], ys[b + 1] - ys[b]) for b in range(3) for a in range(11)]
    assert len(boxes) == 33 and sum(w * h for _, _, w, h in boxes) == CW * CH
    return boxes


WINDOW = (0, 0, CW, CH)
BOX_SETS = {"window": [WINDOW], "tiling": _tiling()}


@pytest.mark.parametrize("boxes", ["window", "tiling"])
@pytest.mark.parametrize("p", [0, 1])
@pytest.mark.parametrize("source", ["rgb", "ycbcr"])
def test_cube_statistics(built, cube, current, source, p, boxes):
    """pull_stats at 256 bins against stats_model.record: the whole window (one region: the banded path) and the 33-box tiling"""
    regions = [(0,) + b for b in BOX_SETS[boxes]]
    st = built.pull_stats([current.on[p]], regions, source=source, bins=256)
    assert st.got == [1] * len(regions)
    host = built.capi.RegionStats(st.records.cpu(), 3, 256, st.got, st.current, st.pic_id)
    for k, b in enumerate(BOX_SETS[boxes]):
        _stats_equal(host, k, sm.record(cube.planes(p, source), WINDOW, b, 256), (source, p, b))


@pytest.mark.parametrize("boxes", ["window", "tiling"])
def test_cube_change_statistics(built, cube, current, boxes):
    """pull_change(source="rgb", bins=256, threshold=(0, 127, 254)) of cube picture 1 against kept picture 0, against
    change_model.record, with the same box sets"""
    regions = [(0,) + b for b in BOX_SETS[boxes]]
    thr = (0, 127, 254)
    ch = built.pull_change([current.changed], regions, source="rgb", bins=256, threshold=thr)
    assert ch.got == [1] * len(regions) and ch.kept == [1]
    host = built.capi.RegionChange(ch.records.cpu(), 3, 256, ch.got, ch.current, ch.kept, ch.pic_id, ch.kept_pic_id)
    for k, b in enumerate(BOX_SETS[boxes]):
        _change_equal(host, k, chm.record(cube.planes(1, "rgb"), cube.planes(0, "rgb"), WINDOW, b, 256, thr), b)


@pytest.mark.parametrize("what", ["picture0", "picture1", "change"])
@pytest.mark.parametrize("cell", [4, 8, 16, 64])
def test_cube_cell_maps(built, cube, current, cell, what):
    """pull_cells(source="rgb") against cells_model.maps, all planes: PICTURE mode on both pictures and CHANGE mode (picture 1
    against kept picture 0), at cell sizes that take the QUAD kernels (4, 8) and the others (16, 64).  This is the path in which the
    compiler once fused the clamp of two pixels (docs/EXPERIMENTS.md, "Cell maps")."""
    grid = clm.default_grid([(CH, CW)], cell)
    if what == "change":
        thr = (0, 127, 254)
        got = built.pull_cells([current.changed], None, cell=cell, source="rgb", planes=CHANGE_PLANES, against="kept", threshold=thr)
        want = clm.maps(clm.CHANGE, clm.plane_bits(clm.CHANGE, CHANGE_PLANES), cube.planes(1, "rgb"), cube.planes(0, "rgb"), WINDOW, WINDOW,
                        cell, grid, thr)
    else:
        p = int(what[-1])
        got = built.pull_cells([current.on[p]], None, cell=cell, source="rgb", planes=PICTURE_PLANES)
        want = clm.maps(clm.PICTURE, clm.plane_bits(clm.PICTURE, PICTURE_PLANES), cube.planes(p, "rgb"), None, WINDOW, WINDOW, cell, grid)
    assert got.got == [1]
    _cells_equal(got, 0, want, (cell, what))


# ------------------------------------------------------------------------------------------------ 2b: the matrix colours
def _matrix_bound(matrix, full):
    """M: a bound of the magnitude of every term and partial sum of the kernel's chain on the 255 scale, from the model's
    coefficients: |k0| 255 + (|k1| + |k2|) 128, the largest over the three channels (k3 <= 0 <= k0 Y and |k3| < 255 k0, so
    |k0 Y + k3| <= 255 k0)"""
    kr, kb = cm.KR_KB[matrix]
    kg = 1 - kr - kb
    sy, sc = (1 / 255, 1 / 255) if full else (1 / 219, 1 / 224)
    rows = [(0.0, 2 * (1 - kr)), (2 * kb * (1 - kb) / kg, 2 * kr * (1 - kr) / kg), (2 * (1 - kb), 0.0)]
    return max(255 * (sy * 255 + (a + b) * sc * 128) for a, b in rows)


@pytest.mark.parametrize("p", [0, 1])
@pytest.mark.parametrize("rng", ["limited", "full"])
@pytest.mark.parametrize("matrix", ["bt601", "bt709", "bt2020"])
def test_cube_through_the_matrix_colours(built, cube, matrix, rng, p):
    """pull_tensor(colour=matrix, colour_range=rng, chroma="nearest") on all 2^24 triples against colour_model in float64.
    float32: test_gpu_tensor_colour's _check as it stands.  uint8: |d| <= 1 everywhere, and d != 0 only where the model's 255 v
    lies within eps of a half-integer.

    eps.  The kernel computes v = med3(fma(k2, Cr', fma(k1, Cb', fma(k0, Y, k3))), 0, 255) in fp32 (tc_value, k_tensor_out.hip.h)
    on exact 8-bit operands, with k0 .. k3 the model's coefficients on the 255 scale folded in double and rounded to fp32 once
    (colour_item, engine.hip).  That is 7 roundings: 4 of coefficients, each a relative 2^-24 of a term, and 3 of FMA results, each
    a relative 2^-24 of a partial sum.  No term or partial sum exceeds M = max over channels of |k0| 255 + (|k1| + |k2|) 128
    (_matrix_bound: at most 572, BT.2020 limited range, blue), and the clamp and the model's own float64 noise (< 1e-9, the
    rounding to 9 places in colour_model.output) add nothing larger.  So |v - 255 v_model| <= eps = 7 x 2^-24 x M + 1e-9
    <= 2.39e-4, and rint() of the two can differ only where 255 v_model is that close to a half-integer."""
    import torch
    M = _matrix_bound(matrix, rng == "full")
    assert 255 < M < 572
    eps = 7 * 2.0 ** -24 * M + 1e-9
    geo = (CW, CH, 0, 0, CW, CH)
    v = cm.colour_hwc(cube.frames[p], geo, matrix, rng == "full", "nearest", "RGB")
    a, b = Feed(built, cube.data), Feed(built, cube.data)
    for f in (a, b):
        _pop(f, p)
        assert f.step()
    kw = dict(colour=matrix, colour_range=rng, chroma="nearest", layout="NHWC", channels="RGB")
    t8, got8, _, _, _ = built.pull_tensor([a.dec], dtype=torch.uint8, **kw)
    t32, got32, _, _, _ = built.pull_tensor([b.dec], dtype=torch.float32, mean=IMAGENET_MEAN, std=IMAGENET_STD, **kw)
    assert got8 == got32 == [1]
    _check(t32[0], cm.output(v, "f32", IMAGENET_MEAN, IMAGENET_STD), "f32", what=(matrix, rng, p))
    x = np.round(255 * v, 9)
    d = t8[0].cpu().numpy().astype(np.float64) - np.rint(x)
    band = np.abs(x - np.floor(x) - 0.5) <= eps
    print(f"matrix colours: {matrix} {rng} picture {p}: eps {eps:.3e}, {int(band.sum())} of {band.size} values inside the band, "
          f"{int((d != 0).sum())} of them differ from the model")
    assert np.abs(d).max() <= 1, np.abs(d).max()
    assert not (d != 0)[~band].any(), (int((d != 0)[~band].sum()), x[(d != 0) & ~band][:6])
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 2c: extremes of the integer statistics
class Big:
    """two streams of two 4096 x 2304 pictures, all (0, 0, 0) then all (255, 255, 255) and the reverse; a decoder on each, the
    first picture kept and the second current.  planes[v][source]: the model's channel planes of the picture of value v."""

    def __init__(self, built):
        zero, full = pp.flat(BW, BH, 0, 0, 0), pp.flat(BW, BH, 255, 255, 255)
        self.feeds = []
        for pics in ((zero, full), (full, zero)):
            f = Feed(built, pp.pcm_stream(list(pics), idc=0))
            _pop(f, 1)
            assert built.keep_pictures([f.dec])[0] == [1]
            _pop(f, 1)
            self.feeds.append(f)
        self.frames = {0: pp.i420(zero), 255: pp.i420(full)}
        self._planes, self._records = {}, {}

    def planes(self, v, source):
        if (v, source) not in self._planes:
            self._planes[v, source] = sm.channels(self.frames[v], BW, BH, source)
        return self._planes[v, source]

    def record(self, kind, order, source, box, bins):
        """the model's record of a box (cached: the 1 x 1 boxes repeat); order 0: 0 then 255, order 1: 255 then 0"""
        key = (kind, order, source, box, bins)
        if key not in self._records:
            cur, kept = self.planes((255, 0)[order], source), self.planes((0, 255)[order], source)
            w = (0, 0, BW, BH)
            self._records[key] = sm.record(cur, w, box, bins) if kind == "stats" else chm.record(cur, kept, w, box, bins, (254, 254, 254))
        return self._records[key]


@pytest.fixture(scope="module")
def big(built, _through_the_product_library):
    b = Big(built)
    yield b
    for f in b.feeds:
        f.close()


def _big_regions(layout):
    """first / last: 1024 regions, the whole window as region 0 / region 1023 and 1023 boxes of 1 x 1 spread over the picture;
    single: the whole window alone"""
    whole = (0, 0, BW, BH)
    ones = [((37 * k) % BW, (53 * k) % BH, 1, 1) for k in range(1023)]
    return {"first": [whole] + ones, "last": ones + [whole], "single": [whole]}[layout]


@pytest.mark.parametrize("layout", ["first", "last", "single"])
@pytest.mark.parametrize("bins", [0, 256])
@pytest.mark.parametrize("source", ["y", "ycbcr"])
def test_saturated_largest_frame_statistics(built, big, source, bins, layout):
    """pull_stats of the all-255 picture of 256 x 144 macroblocks, exact against the model and in closed form: sum 255 N, sumsq
    65025 N, min = max = 255, hist[255] = N with N = 4096 x 2304 = 9,437,184.
    first / last: the call has 1024 regions = STATS_MAX_PARTIALS, which forces S == 1 (one band per region), so ONE workgroup walks
    all 36864 macroblocks of the whole-window region: 36864 > 4 x 8192 = 4 wavefronts x STATS_FOLD, the only shape at which the
    fold loop of k_region_stats makes a second pass.  single: the whole window alone, which takes the banded path."""
    boxes = _big_regions(layout)
    st = built.pull_stats([big.feeds[0].dec], [(0,) + b for b in boxes], source=source, bins=bins)
    assert st.got == [1] * len(boxes)
    C = sm.CHANNELS[source]
    host = built.capi.RegionStats(st.records.cpu(), C, bins, st.got, st.current, st.pic_id)
    for k, b in enumerate(boxes):
        _stats_equal(host, k, big.record("stats", 0, source, b, bins), (source, bins, layout, k))
    k = boxes.index((0, 0, BW, BH))
    assert int(host.count[k]) == N_BIG
    assert host.sum[k].tolist() == [255 * N_BIG] * C and host.sumsq[k].tolist() == [65025 * N_BIG] * C
    assert host.min[k].tolist() == host.max[k].tolist() == [255] * C
    if bins:
        assert host.hist[k][:, 255].tolist() == [N_BIG] * C and int(host.hist[k].sum()) == C * N_BIG


@pytest.mark.parametrize("layout", ["first", "last", "single"])
@pytest.mark.parametrize("bins", [0, 256])
@pytest.mark.parametrize("source", ["y", "ycbcr"])
def test_saturated_largest_frame_change(built, big, source, bins, layout):
    """pull_change between the all-0 and the all-255 picture of 256 x 144 macroblocks, in both orders: |d| = 255 on every sample.
    Exact against the model and in closed form with N = 9,437,184: sad 255 N, ssd 65025 N, sum +255 N (0 kept, 255 current) and
    -255 N (the reverse: a negative 64-bit sum), max 255, above = N at threshold 254 and 0 at threshold 255, hist[255] = N and
    hist[0] = 0 (bin 0 is closed as count - rest).
    first / last: 1024 regions = STATS_MAX_PARTIALS force S == 1, so one workgroup walks all 36864 macroblocks of the whole-window
    region: 36864 > 4 x 8192 = 4 wavefronts x CHANGE_FOLD, the only shape at which the fold loop of k_region_change makes a second
    pass.  single: the whole window alone, which takes the banded path."""
    boxes = _big_regions(layout)
    C = sm.CHANNELS[source]
    k = boxes.index((0, 0, BW, BH))
    for order, sign in ((0, 1), (1, -1)):
        ch = built.pull_change([big.feeds[order].dec], [(0,) + b for b in boxes], source=source, bins=bins, threshold=254)
        assert ch.got == [1] * len(boxes) and ch.kept == [1]
        host = built.capi.RegionChange(ch.records.cpu(), C, bins, ch.got, ch.current, ch.kept, ch.pic_id, ch.kept_pic_id)
        for r, b in enumerate(boxes):
            _change_equal(host, r, big.record("change", order, source, b, bins), (source, bins, layout, order, r))
        assert int(host.count[k]) == N_BIG
        assert host.sad[k].tolist() == [255 * N_BIG] * C and host.ssd[k].tolist() == [65025 * N_BIG] * C
        assert host.sum[k].tolist() == [sign * 255 * N_BIG] * C
        assert host.max[k].tolist() == [255] * C and host.above[k].tolist() == [N_BIG] * C
        if bins:
            assert host.hist[k][:, 255].tolist() == [N_BIG] * C and host.hist[k][:, 0].tolist() == [0] * C
    top = built.pull_change([big.feeds[0].dec], [(0, 0, 0, BW, BH)], source=source, bins=0, threshold=255)
    assert top.above[0].tolist() == [0] * C and top.max[0].tolist() == [255] * C


def _small_feed(built, pics):
    return Feed(built, pp.pcm_stream(pics, crop=SMALL["crop"], idc=0))


SWEEP = sorted({0, 255, 127, 128} | {v for B in (16, 32, 64, 128, 256) for v in (256 // B - 1, 256 // B)})


@pytest.mark.parametrize("source", ["y", "ycbcr", "rgb"])
def test_histogram_bin_boundaries(built, source):
    """flat pictures of 9 x 5 macroblocks (cropped to 138 x 72 at (2, 2)) whose value v = Y = Cb = Cr sits on each side of two bin
    boundaries of every bins setting — the first (256 / bins - 1 and 256 / bins) and the middle one (127, 128) — and at 0 and 255:
    pull_stats, and pull_change against the kept all-0 picture (|d| = v for y and ycbcr), for every bins, against the models"""
    assert SWEEP == [0, 1, 2, 3, 4, 7, 8, 15, 16, 127, 128, 255]
    W, H = SMALL["W"], SMALL["H"]
    feed = _small_feed(built, [pp.flat(W, H, v, v, v) for v in SWEEP])
    boxes = [(0, 0, 138, 72), (1, 3, 67, 33), (-5, 60, 200, 40)]
    regions = [(0,) + b for b in boxes]
    kept = None
    for v in SWEEP:
        _pop(feed, 1)
        planes = sm.channels(pp.i420(pp.flat(W, H, v, v, v)), W, H, source)
        if kept is None:
            assert built.keep_pictures([feed.dec])[0] == [1]
            kept = planes
        for bins in (16, 32, 64, 128, 256):
            st = built.pull_stats([feed.dec], regions, source=source, bins=bins)
            thr = (v, 0, 255)
            ch = built.pull_change([feed.dec], regions, source=source, bins=bins, threshold=thr[:sm.CHANNELS[source]])
            assert st.got == ch.got == [1] * 3
            for k, b in enumerate(boxes):
                _stats_equal(st, k, sm.record(planes, SMALL["window"], b, bins), (source, v, bins, b))
                _change_equal(ch, k, chm.record(planes, kept, SMALL["window"], b, bins, thr), (source, v, bins, b))
            if source != "rgb":
                assert int(st.hist[0, 0, v >> (8 - int(np.log2(bins)))]) == 138 * 72 == int(ch.hist[0, 0, v >> (8 - int(np.log2(bins)))])
    feed.close()


@pytest.mark.parametrize("source", ["y", "ycbcr", "rgb"])
def test_saturated_cell_maps(built, source):
    """a saturated pair on the cropped 9 x 5 macroblock picture (window 138 x 72 at (2, 2): partial cells at the right and bottom
    edge at every cell size): all 0, all 255, all 0.  PICTURE maps of the 255 picture and CHANGE maps in both orders, all planes, every
    cell size, against cells_model.maps; at cell 64 the `sum of d` map goes from +255 x 4096 to -255 x 4096 as int32."""
    W, H = SMALL["W"], SMALL["H"]
    pics = [pp.flat(W, H, 0, 0, 0), pp.flat(W, H, 255, 255, 255), pp.flat(W, H, 0, 0, 0)]
    planes = [sm.channels(pp.i420(p), W, H, source) for p in pics]
    feed = _small_feed(built, pics)
    _pop(feed, 1)
    window, box = SMALL["window"], (0, 0, 138, 72)
    for cur in (1, 2):
        assert built.keep_pictures([feed.dec])[0] == [1]
        _pop(feed, 1)
        for cell in clm.CELLS:
            grid = clm.default_grid([(72, 138)], cell)
            got = built.pull_cells([feed.dec], None, cell=cell, source=source, planes=CHANGE_PLANES, against="kept", threshold=254)
            want = clm.maps(clm.CHANGE, clm.plane_bits(clm.CHANGE, CHANGE_PLANES), planes[cur], planes[cur - 1], window, box, cell, grid,
                            (254, 254, 254))
            assert got.got == [1]
            _cells_equal(got, 0, want, (source, cur, cell))
            if source != "rgb":
                full = 255 * min(cell, 64) ** 2 * (1 if cur == 1 else -1)
                assert int(got.dsum[0, 0, 0, 0]) == full and (cell != 64 or abs(full) == 255 * 4096)
            pic = built.pull_cells([feed.dec], None, cell=cell, source=source, planes=PICTURE_PLANES)
            _cells_equal(pic, 0, clm.maps(clm.PICTURE, clm.plane_bits(clm.PICTURE, PICTURE_PLANES), planes[cur], None, window, box, cell, grid),
                         (source, cur, cell, "picture"))
    feed.close()


# ------------------------------------------------------------------------------------------------ 2d: resampling at hard edges
SCALES = (1 / 3.7, 1 / 2, 1 / 1.5, 1.3)
EDGE_PICTURES = {"9x5": (144, 80, (1, 2, 1, 3), (2, 2, 138, 72)), "20x12": (320, 192, None, (0, 0, 320, 192))}


@pytest.mark.parametrize("filt", ["bilinear", "bilinear_aa", "bicubic_aa"])
@pytest.mark.parametrize("name", ["9x5", "20x12"])
def test_resampling_at_hard_edges(built, name, filt):
    """steps() pictures — hard 0 / 255 edges, one-sample lines, a checkerboard — through pull_tensor(size=...) at scales 1 / 3.7,
    1 / 2, 1 / 1.5 and 1.3 per axis, stretched and letterboxed, uint8 and float32, reference colour and BT.709 full range, against
    resize_model with the comparison and the tolerances of test_gpu_tensor_resize.py (imported).  Bicubic: the model's unclamped
    values leave [0, 255] ([0, 1]) on these inputs (asserted), so the clamp of the uint8 output is exercised on both sides."""
    W, H, crop, window = EDGE_PICTURES[name]
    geo = (W, H) + window
    w, h = window[2:]
    cases = [(s, fit, dt, colour) for s in SCALES for fit in ("stretch", "letterbox") for dt in ("u8", "f32") for colour in ("reference", "bt709")]
    pics = [pp.steps(W, H, seed=k) for k in range(len(cases))]
    feed = Feed(built, pp.pcm_stream(pics, crop=crop, idc=0))
    pad = (0.25, 114 / 255, 1.0)
    for pic, (s, fit, dt, colour) in zip(pics, cases):
        assert feed.step()
        lay, ch = ("NCHW", "RGB") if dt == "f32" else ("NHWC", "BGRA")
        size = (round(h * s), round(w * s)) if fit == "stretch" else (round(h * s * 1.25), round(w * s))
        t, got, _, _, _, boxes = tr._pull(built, [feed.dec], dt, lay, ch, size, filt, colour, fit=fit, pad=pad)
        assert got == [1]
        std = IMAGENET_STD if dt != "u8" else (1, 1, 1)
        mean = IMAGENET_MEAN if dt != "u8" else (0, 0, 0)
        left, top, iw, ih = rm.letterbox(size[1], size[0], w, h) if fit == "letterbox" else (0, 0, size[1], size[0])
        assert boxes == [(left, top, iw, ih)], (s, fit)
        v = rm.resample_hwc(tr._source(pp.i420(pic), geo, colour, ch), (ih, iw), filt, fma=colour == "reference")
        if filt == "bicubic_aa":
            assert v.min() < 0 and v.max() > (255 if colour == "reference" else 1), (s, fit, v.min(), v.max())
        tol = tr._tol_bilinear_ref(dt, std) if colour == "reference" and filt == "bilinear" else tr._tol(colour, dt, std)
        g = tr._hwc(t[0], lay)
        tr._check(g[top:top + ih, left:left + iw], tr._finish(v, colour, dt, ch, mean, std), dt, tol, what=(name, filt, s, fit, dt, colour),
                  half_up=colour == "reference")
        if fit == "letterbox":
            import torch
            border = np.ones(g.shape[:2], bool)
            border[top:top + ih, left:left + iw] = False
            assert border.any()
            want = [rm.pad_value(pad[c], dt, mean[c], std[c]) for c in range(3)]
            want = torch.tensor(want, dtype=torch.float32).to(tr._torch_dtype(dt)).double().numpy()
            if ch == "BGRA":
                want = np.append(want, 255.0)
            assert (g[border] == want[None, :]).all(), (s, dt, colour)
    feed.close()
