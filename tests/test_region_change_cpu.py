"""No GPU: the two symbols of kept pictures and change statistics (declared, exported, mirrored), the stride formula, what
h264bsdmiKeepCurrentPictures and h264bsdmiOutputRegionChange refuse before they look at a device (through the built library, on
parser-only instances), and the numpy model (tests/change_model.py) against itself."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import change_model as cm
import stats_model as sm
from conftest import ROOT
from test_tensor_output import _capture_until_output

SENTINEL = 0xA5A5A5A5
LIMIT = 16384
SYMBOLS = ("h264bsdmiKeepCurrentPictures", "h264bsdmiOutputRegionChange")


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_symbols_are_declared_exported_and_mirrored(built):
    text = open(os.path.join(ROOT, "include", "h264bsd_mi355x.h")).read()
    built.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text)
        assert name in built.EXPORTED_SYMBOLS
        assert name in _exported(built.LIB_PATH) and name in _exported(built.capi.BENCH_LIB_PATH)
    for name in ("keep_pictures", "pull_change", "change_record_bytes", "ChangeSpec", "RegionChange"):
        assert hasattr(built, name)
    assert tuple(int(v) for v in built.__version__.split(".")) >= (0, 4, 0)


def test_change_spec_layout_matches_the_ctypes_mirror(built, tmp_path):
    fields = [f[0] for f in built.ChangeSpec._fields_]
    src = tmp_path / "spec.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "h264bsd_mi355x.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(h264bsdmi_change_spec));\n' +
                   "".join(f'    printf("%zu\\n", offsetof(h264bsdmi_change_spec, {f}));\n' for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "spec"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(built.ChangeSpec)] + [getattr(built.ChangeSpec, f).offset for f in fields]


@pytest.mark.parametrize("source", ["y", "ycbcr", "rgb"])
@pytest.mark.parametrize("bins", [0, 16, 32, 64, 128, 256])
def test_record_bytes_is_the_formula(built, source, bins):
    C = 1 if source == "y" else 3
    assert built.change_record_bytes(source, bins) == 8 + 32 * C + 4 * C * bins == cm.record_bytes(source, bins)
    assert built.change_record_bytes(source, bins) % 8 == 0


def test_record_bytes_refuses_other_names(built):
    for source, bins in (("yuv", 256), ("y", 8), ("rgb", 48), ("ycbcr", 512)):
        with pytest.raises(ValueError):
            built.change_record_bytes(source, bins)


def _spec(built, **kw):
    s = dict(data=0x1000, source=1, bins=256, crop=1, threshold=(0, 0, 0), keep_after=0)
    s.update(kw)
    return built.ChangeSpec(s["data"], s["source"], s["bins"], s["crop"], (ctypes.c_uint32 * 3)(*s["threshold"]), s["keep_after"])


def _call(built, decoders, regions, spec, null_regions=False, null_got=False, n_regions=None, null_dec=False):
    """(rc, got, current, kept, picId, keptPicId) of one raw call; the output arrays start as SENTINEL"""
    L = built.api_lib()
    n, K = len(decoders), len(regions) if n_regions is None else n_regions
    got = (ctypes.c_uint32 * max(K, 1))(*([SENTINEL] * max(K, 1)))
    per = [(ctypes.c_uint32 * max(n, 1))(*([SENTINEL] * max(n, 1))) for _ in range(4)]
    dec = (ctypes.c_void_p * max(n, 1))(*[d._st for d in decoders])
    regs = (built.Region * max(len(regions), 1))(*[built.Region(*r) for r in regions])
    rc = L.h264bsdmiOutputRegionChange(n, None if null_dec else dec, K, None if null_regions else regs, ctypes.byref(spec), None,
                                       None if null_got else got, *per)
    return (rc, list(got)) + tuple(list(a) for a in per)


def _keep(built, decoders, null_kept=False, null_dec=False, n=None):
    L = built.api_lib()
    n = len(decoders) if n is None else n
    kept, ids = (ctypes.c_uint32 * max(n, 1))(*([SENTINEL] * max(n, 1))), (ctypes.c_uint32 * max(n, 1))(*([SENTINEL] * max(n, 1)))
    dec = (ctypes.c_void_p * max(n, 1))(*[d._st for d in decoders])
    rc = L.h264bsdmiKeepCurrentPictures(n, None if null_dec else dec, None, None if null_kept else kept, ids)
    return rc, list(kept), list(ids)


def test_an_empty_call_with_a_valid_spec_is_accepted(built):
    for source in (0, 1, 2):
        for bins in sm.BINS:
            for keep_after in (0, 1):
                res = _call(built, [], [], _spec(built, source=source, bins=bins, threshold=(255, 0, 7), keep_after=keep_after))
                assert res[0] == 0 and res[1] == [SENTINEL], (source, bins, keep_after)
    assert _call(built, [], [], _spec(built), null_regions=True, null_got=True)[0] == 0        # regions == NULL, nRegions == n == 0
    assert _keep(built, []) == (0, [SENTINEL], [SENTINEL])                                       # n == 0 returns 0 ...
    assert _keep(built, [], null_kept=True, null_dec=True)[0] == 0                               # ... whatever else is NULL


BAD_SPEC = [dict(data=0), dict(data=0x1004), dict(data=0x1001), dict(source=3), dict(source=2 ** 32 - 1), dict(bins=8), dict(bins=1),
            dict(bins=48), dict(bins=255), dict(bins=512), dict(crop=2), dict(threshold=(256, 0, 0)), dict(threshold=(0, 256, 0)),
            dict(threshold=(0, 0, 2 ** 32 - 1)), dict(keep_after=2)]


@pytest.mark.parametrize("bad", BAD_SPEC)
def test_invalid_specs_are_refused_before_the_instances(built, bad):
    assert _call(built, [], [], _spec(built, **bad))[0] == -1
    assert built.api_lib().h264bsdmiOutputRegionChange(0, None, 0, None, None, None, None, None, None, None, None) == -1      # no spec at all


BAD_REGIONS = [(1, 0, 0, 16, 16), (2 ** 32 - 1, 0, 0, 16, 16), (0, 0, 0, 0, 16), (0, 0, 0, 16, 0), (0, 0, 0, LIMIT + 1, 16),
               (0, 0, 0, 16, LIMIT + 1), (0, LIMIT + 1, 0, 16, 16), (0, -LIMIT - 1, 0, 16, 16), (0, 0, LIMIT + 1, 16, 16),
               (0, 0, -LIMIT - 1, 16, 16), (0, -2 ** 31, 0, 16, 16)]


def test_every_refusal_is_minus_one_and_nothing_is_written_or_popped(built):
    """an instance in capture mode has no pixels: every call that names it is refused, whatever else is wrong with it; the
    sentinels stay, and the instance's output queue is what an untouched twin's is"""
    a, keep_a = _capture_until_output(built)
    b, keep_b = _capture_until_output(built)
    spec = _spec(built)
    untouched = (-1, [SENTINEL]) + ([SENTINEL],) * 4
    for good in [(0, 0, 0, 16, 16), (0, -5, 3, 17, 31), (0, LIMIT, -LIMIT, LIMIT, LIMIT)]:
        for kw in (dict(), dict(source=0, bins=0), dict(source=2, bins=16, crop=0, keep_after=1)):
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
    assert _call(built, [a], [], spec, null_dec=True)[0] == -1
    res = _call(built, [a, a], [(0, 0, 0, 16, 16), (1, 0, 0, 16, 16)], spec)
    assert res[0] == -1 and res[1] == [SENTINEL] * 2 and res[2] == [SENTINEL] * 2 and res[3] == [SENTINEL] * 2
    # the keep call: capture mode, repeated instances, dec NULL, kept NULL
    assert _keep(built, [a]) == (-1, [SENTINEL], [SENTINEL])
    assert _keep(built, [a, b]) == (-1, [SENTINEL] * 2, [SENTINEL] * 2)
    assert _keep(built, [a, a])[0] == -1
    assert _keep(built, [a], null_dec=True)[0] == -1 and _keep(built, [a], null_kept=True)[0] == -1
    info = a.next_output_info()
    assert info is not None and info == b.next_output_info()
    a.close()
    b.close()


@pytest.mark.parametrize("kw", [dict(source="yuv"), dict(bins=8), dict(threshold=256), dict(threshold=-1), dict(threshold=(1, 2)),
                                dict(threshold=1.5), dict(regions=[(0, 0, 0, 0, 8)]), dict(regions=[(1, 0, 0, 8, 8)]),
                                dict(regions=[(0, 0, 0, 8, 8)] * 65536)])
def test_pull_change_refuses_bad_arguments(built, kw):
    """before any device work: names that are not in the tables, thresholds and regions out of range"""
    a, keep = _capture_until_output(built)
    args = dict(regions=[(0, 0, 0, 8, 8)], source="ycbcr")
    args.update(kw)
    with pytest.raises(ValueError):
        built.pull_change([a], **args)
    a.close()


# ---- the model against itself ----
W, H = 48, 40
WINDOW = (2, 4, 40, 30)
MODEL_BOXES = [(0, 0, 40, 30), (0, 0, 1, 1), (14, 12, 16, 16), (3, 5, 21, 13), (-7, 2, 12, 9), (33, -3, 20, 10), (5, 25, 9, 30), (-4, -4, 50, 40)]


@pytest.fixture(scope="module")
def frames():
    rng = np.random.default_rng(11)
    return [rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8) for _ in range(2)]


@pytest.mark.parametrize("source", ["y", "ycbcr"])
def test_model_identical_frames_give_all_zero(frames, source):
    p = sm.channels(frames[0], W, H, source)
    for box in MODEL_BOXES:
        for bins in (16, 256):
            r = cm.record(p, p.copy(), WINDOW, box, bins)
            assert r.count > 0
            for f in (r.sad, r.ssd, r.sum, r.max, r.above):
                assert not f.any()
            assert (r.hist[:, 0] == r.count).all() and not r.hist[:, 1:].any()


def test_model_a_hand_made_pair_of_samples():
    """two samples: d = +3 and -10"""
    cur = np.array([[[10, 20]]], np.uint8)
    kept = np.array([[[7, 30]]], np.uint8)
    r = cm.record(cur, kept, (0, 0, 2, 1), (0, 0, 2, 1), 16, threshold=(3,))
    assert (r.count, int(r.sad[0]), int(r.ssd[0]), int(r.sum[0]), int(r.max[0]), int(r.above[0])) == (2, 13, 109, -7, 10, 1)
    assert list(r.hist[0]) == [2] + [0] * 15
    r = cm.record(cur, kept, (0, 0, 2, 1), (0, 0, 2, 1), 256, threshold=(2,))
    assert int(r.above[0]) == 2 and r.hist[0][3] == 1 and r.hist[0][10] == 1 and r.hist[0].sum() == 2
    r = cm.record(cur, kept, (0, 0, 2, 1), (1, 0, 5, 5), 0)                  # the second sample only
    assert (r.count, int(r.sad[0]), int(r.sum[0])) == (1, 10, -10) and r.hist is None


@pytest.mark.parametrize("source", ["y", "ycbcr"])
def test_model_histograms_sum_to_count_and_agree_with_the_moments(frames, source):
    a, b = [sm.channels(f, W, H, source) for f in frames]
    for box in MODEL_BOXES:
        r = cm.record(a, b, WINDOW, box, 256, threshold=(40, 0, 254))
        back = cm.record(b, a, WINDOW, box, 256, threshold=(40, 0, 254))
        assert r.count > 0
        for c in range(a.shape[0]):
            assert r.hist[c].sum() == r.count
            assert r.sad[c] == (np.arange(256) * r.hist[c]).sum() and r.ssd[c] == (np.arange(256) ** 2 * r.hist[c]).sum()
            assert np.nonzero(r.hist[c])[0][-1] == r.max[c]
            assert r.above[c] == r.hist[c][(40, 0, 254)[c] + 1:].sum()
        assert np.array_equal(r.sum, -back.sum) and np.array_equal(r.sad, back.sad) and np.array_equal(r.hist, back.hist)
        for bins in (16, 32, 64, 128):
            coarse = cm.record(a, b, WINDOW, box, bins)
            assert np.array_equal(coarse.hist, r.hist.reshape(r.hist.shape[0], bins, 256 // bins).sum(2))


@pytest.mark.parametrize("box", [(40, 0, 5, 5), (0, 30, 5, 5), (-5, 0, 5, 5), (0, -9, 40, 9), (100, 100, 1, 1)])
def test_model_box_outside_the_window_is_all_zero(frames, box):
    a, b = [sm.channels(f, W, H, "ycbcr") for f in frames]
    r = cm.record(a, b, WINDOW, box, 16)
    assert r.count == 0 and not r.hist.any()
    for f in (r.sad, r.ssd, r.sum, r.max, r.above):
        assert not f.any()
