"""No GPU: the stride formula, what h264bsdmiOutputRegionStats refuses before it looks at a device (through the built library, on
parser-only instances), and the numpy model (tests/stats_model.py) against itself."""
import ctypes

import numpy as np
import pytest

import stats_model as sm
from test_tensor_output import _capture_until_output

SENTINEL = 0xA5A5A5A5
LIMIT = 16384


@pytest.mark.parametrize("source", ["y", "ycbcr", "rgb"])
@pytest.mark.parametrize("bins", [0, 16, 32, 64, 128, 256])
def test_record_bytes_is_the_formula(built, source, bins):
    C = 1 if source == "y" else 3
    assert built.stats_record_bytes(source, bins) == 8 + 24 * C + 4 * C * bins == sm.record_bytes(source, bins)
    assert built.stats_record_bytes(source, bins) % 8 == 0


def test_record_bytes_refuses_other_names(built):
    for source, bins in (("yuv", 256), ("y", 8), ("rgb", 48), ("ycbcr", 512)):
        with pytest.raises(ValueError):
            built.stats_record_bytes(source, bins)


def _spec(built, **kw):
    s = dict(data=0x1000, source=1, bins=256, crop=1)
    s.update(kw)
    return built.StatsSpec(*[s[f[0]] for f in built.StatsSpec._fields_])


def _call(built, decoders, regions, spec, null_regions=False, null_got=False, n_regions=None):
    """(rc, got, current, picId) of one raw call; the output arrays start as SENTINEL"""
    L = built.api_lib()
    n, K = len(decoders), len(regions) if n_regions is None else n_regions
    got = (ctypes.c_uint32 * max(K, 1))(*([SENTINEL] * max(K, 1)))
    cur, ids = (ctypes.c_uint32 * max(n, 1))(*([SENTINEL] * max(n, 1))), (ctypes.c_uint32 * max(n, 1))(*([SENTINEL] * max(n, 1)))
    dec = (ctypes.c_void_p * max(n, 1))(*[d._st for d in decoders])
    regs = (built.Region * max(len(regions), 1))(*[built.Region(*r) for r in regions])
    rc = L.h264bsdmiOutputRegionStats(n, dec, K, None if null_regions else regs, ctypes.byref(spec), None,
                                      None if null_got else got, cur, ids)
    return rc, list(got), list(cur), list(ids)


def test_an_empty_call_with_a_valid_spec_is_accepted(built):
    for source in (0, 1, 2):
        for bins in sm.BINS:
            for crop in (0, 1):
                rc, got, cur, ids = _call(built, [], [], _spec(built, source=source, bins=bins, crop=crop))
                assert rc == 0 and got == [SENTINEL], (source, bins, crop)
    assert _call(built, [], [], _spec(built), null_regions=True, null_got=True)[0] == 0       # regions == NULL, nRegions == n == 0


BAD_SPEC = [dict(data=0), dict(data=0x1004), dict(data=0x1001), dict(source=3), dict(source=2 ** 32 - 1), dict(bins=8), dict(bins=1),
            dict(bins=48), dict(bins=255), dict(bins=512), dict(crop=2)]


@pytest.mark.parametrize("bad", BAD_SPEC)
def test_invalid_specs_are_refused_before_the_instances(built, bad):
    assert _call(built, [], [], _spec(built, **bad))[0] == -1
    assert built.api_lib().h264bsdmiOutputRegionStats(0, None, 0, None, None, None, None, None, None) == -1      # no spec at all


BAD_REGIONS = [(1, 0, 0, 16, 16), (2 ** 32 - 1, 0, 0, 16, 16), (0, 0, 0, 0, 16), (0, 0, 0, 16, 0), (0, 0, 0, LIMIT + 1, 16),
               (0, 0, 0, 16, LIMIT + 1), (0, LIMIT + 1, 0, 16, 16), (0, -LIMIT - 1, 0, 16, 16), (0, 0, LIMIT + 1, 16, 16),
               (0, 0, -LIMIT - 1, 16, 16), (0, -2 ** 31, 0, 16, 16)]


def test_every_refusal_is_minus_one_and_nothing_is_written_or_popped(built):
    """an instance in capture mode has no pixels: every call that names it is refused, whatever else is wrong with it; the
    sentinels stay, and the instance's output queue is what an untouched twin's is"""
    a, keep_a = _capture_until_output(built)
    b, keep_b = _capture_until_output(built)
    spec = _spec(built)
    untouched = (-1, [SENTINEL], [SENTINEL], [SENTINEL])
    for good in [(0, 0, 0, 16, 16), (0, -5, 3, 17, 31), (0, LIMIT, -LIMIT, LIMIT, LIMIT)]:
        for kw in (dict(), dict(source=0, bins=0), dict(source=2, bins=16, crop=0)):
            assert _call(built, [a], [good], _spec(built, **kw)) == untouched
    for bad in BAD_REGIONS:
        assert _call(built, [a], [bad], spec) == untouched, bad
    for bad in BAD_SPEC:
        assert _call(built, [a], [(0, 0, 0, 16, 16)], _spec(built, **bad)) == untouched, bad
    assert _call(built, [a], [(0, 0, 0, 16, 16)], spec, null_regions=True) == untouched      # whole windows, but capture mode
    assert _call(built, [a], [(0, 0, 0, 16, 16)] * 2, spec, null_regions=True)[0] == -1      # regions == NULL with nRegions != n
    assert _call(built, [], [(0, 0, 0, 16, 16)], spec, null_regions=True)[0] == -1           # likewise, n == 0
    assert _call(built, [a], [(0, 0, 0, 16, 16)], spec, null_got=True)[0] == -1
    assert _call(built, [a], [(0, 0, 0, 16, 16)], spec, n_regions=65536)[0] == -1
    assert _call(built, [a], [], spec)[0] == -1                                              # the instances are checked as in the region pull
    rc, got, cur, ids = _call(built, [a, a], [(0, 0, 0, 16, 16), (1, 0, 0, 16, 16)], spec)
    assert rc == -1 and got == [SENTINEL] * 2 and cur == [SENTINEL] * 2
    info = a.next_output_info()
    assert info is not None and info == b.next_output_info()
    a.close()
    b.close()


@pytest.mark.parametrize("kw", [dict(source="yuv"), dict(bins=8), dict(bins=48), dict(regions=[(0, 0, 0, 0, 8)]),
                                dict(regions=[(0, 0, 0, 8, LIMIT + 1)]), dict(regions=[(0, 0.5, 0, 8, 8)]), dict(regions=[(1, 0, 0, 8, 8)]),
                                dict(regions=[(0, 0, 0, 8, 8)] * 65536)])
def test_pull_stats_refuses_bad_arguments(built, kw):
    """before any device work: names that are not in the tables, regions that are not five host integers in range"""
    a, keep = _capture_until_output(built)
    args = dict(regions=[(0, 0, 0, 8, 8)])
    args.update(kw)
    with pytest.raises(ValueError):
        built.pull_stats([a], **args)
    a.close()


# ---- the model against itself ----
W, H = 48, 40
WINDOW = (2, 4, 40, 30)
MODEL_BOXES = [(0, 0, 40, 30), (0, 0, 1, 1), (14, 12, 16, 16), (3, 5, 21, 13), (-7, 2, 12, 9), (33, -3, 20, 10), (5, 25, 9, 30), (-4, -4, 50, 40)]


@pytest.fixture(scope="module")
def planes():
    rng = np.random.default_rng(7)
    i420 = rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8)
    return {"y": sm.channels(i420, W, H, "y"), "ycbcr": sm.channels(i420, W, H, "ycbcr"), "i420": i420}


@pytest.mark.parametrize("source", ["y", "ycbcr"])
def test_model_histograms_sum_to_count_and_agree_with_the_extrema(planes, source):
    for box in MODEL_BOXES:
        r = sm.record(planes[source], WINDOW, box, 256)
        x0, x1 = max(box[0], 0), min(box[0] + box[2], WINDOW[2])
        y0, y1 = max(box[1], 0), min(box[1] + box[3], WINDOW[3])
        assert r.count == (x1 - x0) * (y1 - y0) > 0
        for c in range(planes[source].shape[0]):
            assert r.hist[c].sum() == r.count
            nz = np.nonzero(r.hist[c])[0]
            assert (nz[0], nz[-1]) == (r.min[c], r.max[c])
            assert r.sum[c] == (np.arange(256) * r.hist[c]).sum() and r.sumsq[c] == (np.arange(256) ** 2 * r.hist[c]).sum()
        for bins in (16, 32, 64, 128):
            coarse = sm.record(planes[source], WINDOW, box, bins)
            assert np.array_equal(coarse.hist, r.hist.reshape(r.hist.shape[0], bins, 256 // bins).sum(2))
            assert (coarse.count, list(coarse.sum), list(coarse.min)) == (r.count, list(r.sum), list(r.min))
        assert sm.record(planes[source], WINDOW, box, 0).hist is None


def test_model_pairs_chroma_in_coded_frame_coordinates(planes):
    """a 1 x 1 box at window position (u, v) reads chroma sample ((x0 + u) >> 1, (y0 + v) >> 1) of the coded frame"""
    i420 = planes["i420"]
    cb = i420[W * H:W * H * 5 // 4].reshape(H // 2, W // 2)
    for u, v in ((0, 0), (1, 1), (7, 2), (39, 29)):
        r = sm.record(planes["ycbcr"], WINDOW, (u, v, 1, 1), 0)
        X, Y = WINDOW[0] + u, WINDOW[1] + v
        assert r.count == 1 and r.sum[0] == i420[Y * W + X] and r.sum[1] == cb[Y >> 1, X >> 1]


def test_model_rgb_is_the_reference_conversion(built, planes):
    rgb = sm.channels(planes["i420"], W, H, "rgb")
    assert rgb.shape == (3, H, W)
    Y, cb, cr = [p.astype(np.int64) for p in planes["ycbcr"]]
    want = np.clip((298 * (Y - 16) + 409 * (cr - 128) + 128) >> 8, 0, 255)
    assert np.array_equal(rgb[0], want)
    want = np.clip((298 * (Y - 16) + 516 * (cb - 128) + 128) >> 8, 0, 255)
    assert np.array_equal(rgb[2], want)


@pytest.mark.parametrize("box", [(40, 0, 5, 5), (0, 30, 5, 5), (-5, 0, 5, 5), (0, -9, 40, 9), (100, 100, 1, 1)])
def test_model_box_outside_the_window_is_the_empty_record(planes, box):
    r = sm.record(planes["ycbcr"], WINDOW, box, 16)
    assert r.count == 0 and not r.sum.any() and not r.sumsq.any() and not r.hist.any()
    assert list(r.min) == [255] * 3 and list(r.max) == [0] * 3
