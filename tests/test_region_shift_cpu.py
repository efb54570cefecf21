"""No GPU: the symbol of the region shift (declared, exported, mirrored), the stride formula, what h264bsdmiOutputRegionShift refuses
before it looks at a device (through the built library, on parser-only instances), and the numpy model (tests/shift_model.py) against
itself.  A parser-only instance is refused whatever its regions are, so here both sides of the 4096 limit return -1; that a side of
4096 passes the check is shown in C by tests/test_region_shift_host.py, where an accepted call reaches a recording sink, and on the
device by tests/test_gpu_region_shift.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import change_model as cm
import shift_model as shm
from conftest import ROOT
from test_tensor_output import _capture_until_output

SENTINEL = 0xA5A5A5A5
LIMIT = 16384
SYMBOL = "h264bsdmiOutputRegionShift"


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_the_symbol_is_declared_exported_and_mirrored(built):
    text = open(os.path.join(ROOT, "include", "h264bsd_mi355x.h")).read()
    built.lib()
    assert re.search(r"\bint\s+" + SYMBOL + r"\s*\(", text)
    assert SYMBOL in built.EXPORTED_SYMBOLS
    assert SYMBOL in _exported(built.LIB_PATH) and SYMBOL in _exported(built.capi.BENCH_LIB_PATH)
    for name in ("pull_shift", "shift_record_bytes", "ShiftSpec", "RegionShift"):
        assert hasattr(built, name)
    assert re.search(r"#define\s+H264BSDMI_SHIFT_MAX_RADIUS\s+16\b", text) and re.search(r"#define\s+H264BSDMI_SHIFT_MAX_SIDE\s+4096\b", text)
    assert (built.capi.SHIFT_MAX_RADIUS, built.capi.SHIFT_MAX_SIDE) == (16, 4096)
    assert tuple(int(v) for v in built.__version__.split(".")) >= (0, 7, 0)


def test_shift_spec_layout_matches_the_ctypes_mirror(built, tmp_path):
    fields = [f[0] for f in built.ShiftSpec._fields_]
    src = tmp_path / "spec.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "h264bsd_mi355x.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(h264bsdmi_shift_spec));\n' +
                   "".join(f'    printf("%zu\\n", offsetof(h264bsdmi_shift_spec, {f}));\n' for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "spec"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(built.ShiftSpec)] + [getattr(built.ShiftSpec, f).offset for f in fields]


@pytest.mark.parametrize("radius", [0, 1, 16])
def test_record_bytes_is_the_headers_formula(built, radius):
    D = 2 * radius + 1
    assert built.shift_record_bytes(radius, False) == 32 == shm.record_bytes(radius, False)
    assert built.shift_record_bytes(radius, True) == 32 + 4 * (D * D + 1) == shm.record_bytes(radius, True)
    assert built.shift_record_bytes(radius, True) % 8 == 0
    for bad in (-1, 17, 1.0, None):
        with pytest.raises(ValueError):
            built.shift_record_bytes(bad, True)


def _spec(built, **kw):
    s = dict(data=0x1000, radius=4, surface=1, crop=1, keep_after=0)
    s.update(kw)
    return built.ShiftSpec(s["data"], s["radius"], s["surface"], s["crop"], s["keep_after"])


def _call(built, decoders, regions, spec, null_regions=False, null_got=False, n_regions=None, null_dec=False):
    """(rc, got, current, kept, picId, keptPicId) of one raw call; the output arrays start as SENTINEL"""
    L = built.api_lib()
    n, K = len(decoders), len(regions) if n_regions is None else n_regions
    got = (ctypes.c_uint32 * max(K, 1))(*([SENTINEL] * max(K, 1)))
    per = [(ctypes.c_uint32 * max(n, 1))(*([SENTINEL] * max(n, 1))) for _ in range(4)]
    dec = (ctypes.c_void_p * max(n, 1))(*[d._st for d in decoders])
    regs = (built.Region * max(len(regions), 1))(*[built.Region(*r) for r in regions])
    rc = L.h264bsdmiOutputRegionShift(n, None if null_dec else dec, K, None if null_regions else regs, ctypes.byref(spec), None,
                                      None if null_got else got, *per)
    return (rc, list(got)) + tuple(list(a) for a in per)


def test_an_empty_call_with_a_valid_spec_is_accepted(built):
    for radius in (0, 1, 16):                                  # radius 16 passes ...
        for surface in (0, 1):
            for keep_after in (0, 1):
                res = _call(built, [], [], _spec(built, radius=radius, surface=surface, crop=surface, keep_after=keep_after))
                assert res[0] == 0 and res[1] == [SENTINEL], (radius, surface, keep_after)
    assert _call(built, [], [], _spec(built, radius=17))[0] == -1                              # ... and 17 does not
    assert _call(built, [], [], _spec(built), null_regions=True, null_got=True)[0] == 0        # regions == NULL, nRegions == n == 0


BAD_SPEC = [dict(data=0), dict(data=0x1004), dict(data=0x1001), dict(radius=17), dict(radius=2 ** 32 - 1), dict(surface=2), dict(crop=2),
            dict(keep_after=2), dict(surface=2 ** 31)]


@pytest.mark.parametrize("bad", BAD_SPEC)
def test_invalid_specs_are_refused_before_the_instances(built, bad):
    assert _call(built, [], [], _spec(built, **bad))[0] == -1
    assert built.api_lib().h264bsdmiOutputRegionShift(0, None, 0, None, None, None, None, None, None, None, None) == -1       # no spec at all


BAD_REGIONS = [(1, 0, 0, 16, 16), (2 ** 32 - 1, 0, 0, 16, 16), (0, 0, 0, 0, 16), (0, 0, 0, 16, 0), (0, 0, 0, LIMIT + 1, 16),
               (0, 0, 0, 16, LIMIT + 1), (0, LIMIT + 1, 0, 16, 16), (0, -LIMIT - 1, 0, 16, 16), (0, 0, LIMIT + 1, 16, 16),
               (0, 0, -LIMIT - 1, 16, 16), (0, -2 ** 31, 0, 16, 16), (0, 0, 0, 4097, 16), (0, 0, 0, 16, 4097), (0, 0, 0, LIMIT, LIMIT)]


def test_every_refusal_is_minus_one_and_nothing_is_written_or_popped(built):
    """an instance in capture mode has no pixels: every call that names it is refused, whatever else is wrong with it; the
    sentinels stay, and the instance's output queue is what an untouched twin's is"""
    a, keep_a = _capture_until_output(built)
    b, keep_b = _capture_until_output(built)
    spec = _spec(built)
    untouched = (-1, [SENTINEL]) + ([SENTINEL],) * 4
    for good in [(0, 0, 0, 16, 16), (0, -5, 3, 17, 31), (0, LIMIT, -LIMIT, 4096, 4096)]:
        for kw in (dict(), dict(radius=0, surface=0), dict(radius=16, crop=0, keep_after=1)):
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
    info = a.next_output_info()
    assert info is not None and info == b.next_output_info()
    a.close()
    b.close()


@pytest.mark.parametrize("kw", [dict(radius=17), dict(radius=-1), dict(radius=1.5), dict(regions=[(0, 0, 0, 0, 8)]), dict(regions=[(1, 0, 0, 8, 8)]),
                                dict(regions=[(0, 0, 0, 4097, 8)]), dict(regions=[(0, 0, 0, 8, 4097)]), dict(regions=[(0, 0, 0, 8, 8)] * 65536)])
def test_pull_shift_refuses_bad_arguments(built, kw):
    """before any device work: a radius or a region out of range"""
    a, keep = _capture_until_output(built)
    args = dict(regions=[(0, 0, 0, 8, 8)])
    args.update(kw)
    with pytest.raises(ValueError):
        built.pull_shift([a], **args)
    a.close()


# ---- the model against itself ----
W, H = 64, 48


def _shifted(K, sx, sy):
    return K[np.clip(np.arange(H) - sy, 0, H - 1)[:, None], np.clip(np.arange(W) - sx, 0, W - 1)[None, :]]


@pytest.mark.parametrize("R", [3, 5])
def test_model_finds_the_shift_it_was_given(R):
    K = np.random.default_rng(21).integers(0, 256, (H, W), dtype=np.uint8)
    box = (R + 4, R + 1, W - 2 * R - 9, H - 2 * R - 3)                 # at least R inside the window
    for sx, sy in ((0, 0), (3, -2), (-R, R)):
        r = shm.record(K, _shifted(K, sx, sy), (0, 0, W, H), box, R)
        assert (r.dx, r.dy, r.best, r.ties) == (sx, sy, 0, 1) and r.count == box[2] * box[3] and r.D == 2 * R + 1
        assert r.surface[sy + R, sx + R] == 0 and r.still == r.surface[R, R] and len(r.bytes(True)) == shm.record_bytes(R, True)
        assert (r.still == 0) == ((sx, sy) == (0, 0))


def test_model_flat_pair_answers_zero_with_every_displacement_tied():
    a, b = np.full((H, W), 90, np.uint8), np.full((H, W), 97, np.uint8)
    for box in ((0, 0, W, H), (5, 5, 9, 9), (-3, 40, 20, 20)):
        r = shm.record(a, b, (0, 0, W, H), box, 4)
        assert (r.dx, r.dy, r.ties) == (0, 0, 81) and r.best == r.still == 7 * r.count and (r.surface == r.best).all()


def test_model_still_is_the_change_models_luma_sad():
    rng = np.random.default_rng(4)
    kept, cur = (rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(2))
    window = (2, 4, 58, 40)
    for box in ((0, 0, 58, 40), (13, 11, 37, 23), (-9, 10, 30, 20), (50, -7, 25, 19), (0, 0, 1, 1)):
        r = shm.record(kept, cur, window, box, 2)
        c = cm.record(cur[None], kept[None], window, box, 0)
        assert r.count == c.count and r.still == int(c.sad[0])


def test_model_clamps_at_the_window_and_a_miss_is_the_formula_on_nothing():
    rng = np.random.default_rng(6)
    kept, cur = (rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(2))
    window = (2, 4, 58, 40)
    r = shm.record(kept, cur, window, (0, 0, 1, 1), 1)                # the window's corner: up and left replicate the corner sample
    d = abs(int(kept[4, 2]) - int(cur[4, 2]))
    assert r.surface[0, 0] == r.surface[0, 1] == r.surface[1, 0] == r.surface[1, 1] == d
    assert r.surface[1, 2] == abs(int(kept[4, 2]) - int(cur[4, 3])) and r.surface[2, 1] == abs(int(kept[4, 2]) - int(cur[5, 2]))
    r = shm.record(kept, cur, window, (200, 200, 8, 8), 3)
    assert (r.count, r.dx, r.dy, r.best, r.still, r.ties) == (0, 0, 0, 0, 0, 49) and not r.surface.any()
    assert r.bytes(False) == np.array([0, 7, 0, 0, 0, 0, 49, 0], "<u4").tobytes()
