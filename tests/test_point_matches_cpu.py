"""No GPU: the pattern of the descriptor (the generator of the header against its pins and against h264bsdmiDescriptorPattern), the
symbols of the point matches (declared, exported, mirrored), the struct and the constants against the header, what
h264bsdmiOutputPointMatches refuses before it looks at a device (through the built library, on parser-only instances), the argument
errors of pull_matches, the views of PointMatches on a hand-filled buffer, and the numpy model (tests/matches_model.py): the vectorised
form against the one written straight from the definition, the tie rules and the accept rule at its boundaries."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import matches_model as mm
from conftest import ROOT
from test_tensor_output import _capture_until_output

SENTINEL = 0xA5A5A5A5
CONSTANTS = dict(H264BSDMI_MATCH_VALID=1, H264BSDMI_MATCH_MUTUAL=2, H264BSDMI_MATCH_ACCEPTED=4, H264BSDMI_MATCHES_MAX_POINTS=256)
SYMBOL = "h264bsdmiOutputPointMatches"


# ---- the pattern ----
def test_the_generator_reproduces_the_pins():
    tests, dropped = mm.generate_pattern()
    assert dropped == 0 and len(tests) == 256
    assert tests[:3] == [(-6, 5, 4, -1), (0, -10, -10, -4), (-7, -10, -6, 1)] and tests[-1] == (-2, -2, -4, -11)
    flat = [v for t in tests for v in t]
    assert sum(flat) == 86 and sum(abs(v) for v in flat) == 4464 and min(flat) >= -12 and max(flat) <= 12


def test_256_distinct_tests_none_degenerate():
    tests = [tuple(t) for t in mm.PATTERN.tolist()]
    assert all(t[:2] != t[2:] for t in tests)
    assert len(set(tests) | {t[2:] + t[:2] for t in tests}) == 512


def test_the_exported_pattern_is_the_generator(built):
    got = built.descriptor_pattern()
    assert got.dtype == np.int8 and got.shape == (256, 4) and np.array_equal(got.astype(np.int64), mm.PATTERN)
    header = open(os.path.join(ROOT, "h264bsd_amd", "csrc", "descriptor_pattern.h")).read()
    numbers = [int(v) for v in re.findall(r"-?\d+", header[header.index("DESCRIPTOR_PATTERN_VALUES") + 25:header.rindex("#endif")])]
    assert numbers == mm.PATTERN.ravel().tolist()              # written out as numbers, once: api.c and the kernel include it
    for user in ("api.c", os.path.join("kernels", "k_point_matches.hip.h")):
        text = open(os.path.join(ROOT, "h264bsd_amd", "csrc", user)).read()
        assert "descriptor_pattern.h" in text and "DESCRIPTOR_PATTERN_VALUES" in text


# ---- the symbols, the struct ----
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_symbols_are_declared_exported_and_mirrored(built):
    text = open(os.path.join(ROOT, "include", "h264bsd_mi355x.h")).read()
    built.lib()
    assert re.search(r"\bint\s+" + SYMBOL + r"\s*\(", text) and re.search(r"const signed char \*h264bsdmiDescriptorPattern\(void\);", text)
    for sym in (SYMBOL, "h264bsdmiDescriptorPattern"):
        assert sym in built.EXPORTED_SYMBOLS
        assert sym in _exported(built.LIB_PATH) and sym in _exported(built.capi.BENCH_LIB_PATH)
    for attr in ("pull_matches", "MatchesSpec", "PointMatches", "matches_record_bytes", "descriptor_pattern"):
        assert hasattr(built, attr)
    assert tuple(int(v) for v in built.__version__.split(".")) >= (0, 11, 0)
    doc = text[text.index("/* Point matches:"):text.index(SYMBOL + "(")]
    assert "THE DEFINITION" in doc and "0x9E3779B9" in doc and "best * 256 < ratio * second" in doc and "(-2, -2, -4, -11)" in doc


FIELDS = ["data", "kept_points", "current_points", "max_points", "max_distance", "ratio", "max_move", "mutual_only", "crop", "keep_after", "zero"]


def test_spec_layout_and_constants_match_the_header(built, tmp_path):
    assert [f[0] for f in built.MatchesSpec._fields_] == FIELDS
    src = tmp_path / "spec.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "h264bsd_mi355x.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(h264bsdmi_matches_spec));\n' +
                   "".join(f'    printf("%zu\\n", offsetof(h264bsdmi_matches_spec, {f}));\n' for f in FIELDS) +
                   "".join(f'    printf("%u\\n", (unsigned){c});\n' for c in CONSTANTS) + "    return 0;\n}\n")
    exe = tmp_path / "spec"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(built.MatchesSpec)] + [getattr(built.MatchesSpec, f).offset for f in FIELDS] + list(CONSTANTS.values())
    assert built.capi.MATCH_FLAGS == dict(valid=mm.VALID, mutual=mm.MUTUAL, accepted=mm.ACCEPTED)
    assert built.capi.MATCHES_MAX_POINTS == 256


def test_matches_record_bytes(built):
    assert [built.matches_record_bytes(k) for k in (1, 7, 64, 256)] == [112, 592, 5152, 20512] == [mm.record_bytes(k) for k in (1, 7, 64, 256)]
    for bad in (0, 257, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="matches_record_bytes"):
            built.matches_record_bytes(bad)


# ---- the refusals of the header, without a device ----
def _spec(built, **kw):
    s = dict(data=0x1000, kept_points=0x2000, current_points=0x3000, max_points=64, max_distance=64, ratio=205, max_move=0, mutual_only=1,
             crop=1, keep_after=0, zero=0)
    s.update(kw)
    return built.MatchesSpec(*[s[f] for f in FIELDS])


def _call(built, decoders, regions, spec, null_regions=False, null_got=False, n_regions=None):
    """(rc, got, current, kept, picId, keptPicId) of one raw call; the output arrays start as SENTINEL"""
    L = built.api_lib()
    n, K = len(decoders), len(regions) if n_regions is None else n_regions
    got = (ctypes.c_uint32 * max(K, 1))(*([SENTINEL] * max(K, 1)))
    per = [(ctypes.c_uint32 * max(n, 1))(*([SENTINEL] * max(n, 1))) for _ in range(4)]
    dec = (ctypes.c_void_p * max(n, 1))(*[d._st for d in decoders])
    regs = (built.Region * max(len(regions), 1))(*[built.Region(*r) for r in regions])
    rc = L.h264bsdmiOutputPointMatches(n, dec, K, None if null_regions else regs, ctypes.byref(spec), None, None if null_got else got, *per)
    return (rc, list(got)) + tuple(list(a) for a in per)


def test_an_empty_call_with_a_valid_spec_is_accepted_and_launches_nothing(built):
    for kw in (dict(), dict(max_points=1), dict(max_points=256), dict(max_distance=0), dict(max_distance=256), dict(ratio=1), dict(ratio=256),
               dict(max_move=1), dict(max_move=65535), dict(mutual_only=0), dict(crop=0), dict(keep_after=1), dict(data=0x1008),
               dict(current_points=0x2000)):
        res = _call(built, [], [], _spec(built, **kw))
        assert res[0] == 0 and res[1] == [SENTINEL], kw
    assert _call(built, [], [], _spec(built), null_regions=True, null_got=True)[0] == 0        # regions == NULL, nRegions == n == 0


BAD_SPEC = [dict(data=0), dict(data=0x1004), dict(data=0x1001), dict(kept_points=0), dict(kept_points=0x2004), dict(current_points=0),
            dict(current_points=0x3002), dict(max_points=0), dict(max_points=257), dict(max_points=2 ** 32 - 1), dict(max_distance=257),
            dict(max_distance=2 ** 31), dict(ratio=0), dict(ratio=257), dict(max_move=65536), dict(max_move=2 ** 32 - 1), dict(mutual_only=2),
            dict(crop=2), dict(keep_after=2), dict(zero=1)]


@pytest.mark.parametrize("bad", BAD_SPEC)
def test_invalid_specs_are_refused_before_the_instances(built, bad):
    assert _call(built, [], [], _spec(built, **bad))[0] == -1
    assert built.api_lib().h264bsdmiOutputPointMatches(0, None, 0, None, None, None, None, None, None, None, None) == -1      # no spec at all


def test_every_refusal_is_minus_one_and_nothing_is_written_or_popped(built):
    """an instance in capture mode has no pixels: every call that names it is refused; the sentinels stay, and the instance's output
    queue is what an untouched twin's is.  The regions are the region shift's: a side above 4096 is refused"""
    a, keep_a = _capture_until_output(built)
    b, keep_b = _capture_until_output(built)
    spec = _spec(built)
    untouched = (-1, [SENTINEL]) + ([SENTINEL],) * 4
    for good in [(0, 0, 0, 16, 16), (0, -5, 3, 17, 31), (0, 16384, -16384, 4096, 4096)]:
        assert _call(built, [a], [good], spec) == untouched
    for bad in [(1, 0, 0, 16, 16), (0, 0, 0, 0, 16), (0, 0, 0, 16, 4097), (0, 0, 0, 4097, 16), (0, 16385, 0, 16, 16), (0, 0, -16385, 16, 16)]:
        assert _call(built, [a], [bad], spec) == untouched, bad
    for bad in BAD_SPEC:
        assert _call(built, [a], [(0, 0, 0, 16, 16)], _spec(built, **bad)) == untouched, bad
    assert _call(built, [a], [(0, 0, 0, 16, 16)] * 2, spec, null_regions=True)[0] == -1      # regions == NULL with nRegions != n
    assert _call(built, [a], [(0, 0, 0, 16, 16)], spec, null_got=True)[0] == -1
    assert _call(built, [a], [(0, 0, 0, 16, 16)], spec, n_regions=65536)[0] == -1
    res = _call(built, [a, a], [(0, 0, 0, 16, 16), (1, 0, 0, 16, 16)], spec)
    assert res[0] == -1 and res[1] == [SENTINEL] * 2 and res[2] == [SENTINEL] * 2
    info = a.next_output_info()
    assert info is not None and info == b.next_output_info()
    a.close()
    b.close()


class _Points:
    """what pull_matches looks at of a tensor of point records before the library is called"""

    def __init__(self, shape, ptr=0x1000, cuda=True, contiguous=True, dtype=None):
        import torch
        self.shape, self._ptr, self.is_cuda, self._contiguous, self.dtype = shape, ptr, cuda, contiguous, dtype or torch.uint8

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return self._contiguous

    def data_ptr(self):
        return self._ptr


@pytest.mark.parametrize("kw", [dict(max_distance=257), dict(max_distance=-1), dict(max_distance=2.0), dict(max_distance=True), dict(ratio=0),
                                dict(ratio=257), dict(ratio=0.8), dict(max_move=-1), dict(max_move=65536), dict(max_move=None),
                                dict(regions=[(0, 0, 0, 0, 8)]), dict(regions=[(1, 0, 0, 8, 8)]), dict(regions=[(0, 0, 0, 4097, 8)]),
                                dict(regions=[(0, 0, 0, 8, 8)] * 65536), dict(kept_points="records"), dict(kept_points=None)])
def test_pull_matches_refuses_bad_arguments(built, kw, monkeypatch):
    """before any library call: the entry point is taken away for the test, so a refusal that came too late would not be a ValueError"""
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(torch, "Tensor", _Points)               # the stand-in passes for a tensor: no device is needed to refuse
    a, keep = _capture_until_output(built)
    monkeypatch.setattr(built.capi, "_kept_pull", lambda *args, **kws: pytest.fail("the library was called"))
    monkeypatch.setattr(built.capi, "_out_and_stream", lambda *args, **kws: pytest.fail("an output was allocated"))
    args = dict(kept_points=_Points((1, 32 + 16 * 8)), current_points=_Points((1, 32 + 16 * 8)), regions=[(0, 0, 0, 8, 8)])
    with pytest.raises(pytest.fail.Exception, match="an output was allocated"):
        built.pull_matches([a], **args)                         # the arguments as they stand pass every check
    args.update(kw)
    with pytest.raises(ValueError, match="pull_matches"):
        built.pull_matches([a], **args)
    a.close()


def test_pull_matches_refuses_point_records_that_do_not_fit(built, monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(torch, "Tensor", _Points)               # the stand-in passes for a tensor: no device is needed to refuse
    a, keep = _capture_until_output(built)
    monkeypatch.setattr(built.capi, "_kept_pull", lambda *args, **kws: pytest.fail("the library was called"))
    monkeypatch.setattr(built.capi, "_out_and_stream", lambda *args, **kws: pytest.fail("an output was allocated"))
    good = _Points((1, 32 + 16 * 8))
    for bad in (_Points((1, 32 + 16 * 8), cuda=False), _Points((1, 32 + 16 * 8), contiguous=False), _Points((1, 32 + 16 * 8), ptr=0x1004),
                _Points((1, 32 + 16 * 8), dtype=torch.int32), _Points((2, 32 + 16 * 8)), _Points((1, 32 + 16 * 8 + 8)), _Points((1, 32)),
                _Points((1, 32 + 16 * 257)), _Points((32 + 16 * 8,)), _Points((1, 32 + 16 * 7))):
        for args in ((bad, good), (good, bad)):
            with pytest.raises(ValueError, match="pull_matches"):
                built.pull_matches([a], *args, regions=[(0, 0, 0, 8, 8)])
    a.close()


def test_views_of_a_hand_filled_record(built):
    torch = pytest.importorskip("torch")
    K, R = 3, 2
    recs = []
    for r in range(R):
        slots = [(1, 5 + r, 9, 7), (-1, 257, 257, 0), (0, 0, 257, 5)]
        recs.append(struct.pack("<IIIIiiII", 2, 3, 2, 1, -7 - r, 4, 0, 0) + b"".join(struct.pack("<iIII", *s) for s in slots) +
                    bytes(range(96)) + bytes(range(100, 196)))
    m = built.PointMatches(torch.tensor(np.frombuffer(b"".join(recs), np.uint8).reshape(R, -1).copy()), K, [1, 1], [1], [1], [7], [6])
    assert m.kept_valid.tolist() == [2, 2] and m.current_valid.tolist() == [3, 3] and m.accepted.tolist() == [2, 2] and m.mutual.tolist() == [1, 1]
    assert m.sum_dx.tolist() == [-7, -8] and m.sum_dy.tolist() == [4, 4]
    assert m.j.tolist() == [[1, -1, 0]] * 2 and m.best.tolist() == [[5, 257, 0], [6, 257, 0]] and m.second.tolist() == [[9, 257, 257]] * 2
    assert m.flags.tolist() == [[7, 0, 5]] * 2
    assert tuple(m.kept_descriptors.shape) == (R, K, 32) and m.kept_descriptors[1, 2].tolist() == list(range(64, 96))
    assert m.current_descriptors[0, 0].tolist() == list(range(100, 132))
    pts = lambda ps: torch.tensor(np.frombuffer(mm.points_record(ps, K) * R, np.uint8).reshape(R, -1).copy())
    kp, cp = pts([(10, 20), (0, 0), (30, 40)]), pts([(33, 38), (12, 19), (0, 0)])
    assert m.pairs(1, kp, cp) == [(10, 20, 12, 19, 6), (30, 40, 33, 38, 0)]
    assert m.moved(29, [(0, 0, 0, 64, 48), (0, 0, 0, 64, 48)], cp) == [(0, -2, 5, 29, 29), (0, 19, 24, 29, 29)] * 2
    with pytest.raises(ValueError, match="moved"):
        m.moved(29, None, cp)
    with pytest.raises(ValueError, match="pairs"):
        m.pairs(0, kp[:1], cp)


# ---- the model: the vectorised form against the definition ----
W, H = 64, 48
WINDOWS = [(0, 0, W, H), (2, 4, 58, 40)]                      # the coded frame; a window at no macroblock edge


def _edge_points(ww, wh):
    """the four corners, the middle of each edge, 13, 14 and 15 samples from each border, the interior"""
    pts = [(0, 0), (ww - 1, 0), (0, wh - 1), (ww - 1, wh - 1), (ww // 2, 0), (ww // 2, wh - 1), (0, wh // 2), (ww - 1, wh // 2)]
    for d in (13, 14, 15):
        pts += [(d, wh // 2), (ww - 1 - d, wh // 2), (ww // 2, d), (ww // 2, wh - 1 - d), (d, d), (ww - 1 - d, wh - 1 - d)]
    return pts + [(ww // 2, wh // 2), (ww // 2 + 3, wh // 2 - 2)]


@pytest.fixture(scope="module")
def pictures():
    rng = np.random.default_rng(41)
    kept = rng.integers(0, 256, (H, W), dtype=np.uint8)
    cur = np.roll(kept, (2, -3), axis=(0, 1))
    cur[30:, :] = rng.integers(0, 256, (H - 30, W), dtype=np.uint8)
    return kept, cur


@pytest.mark.parametrize("window", WINDOWS)
def test_the_two_forms_agree_on_random_pictures(pictures, window):
    """points on all four corners and edges of the window, around the reach of the descriptor, in the interior; invalid slots: outside
    the box, outside the window, negative, 2^31 - 1, beyond `written`; boxes that cut the points and one that misses the window"""
    kept, cur = pictures
    ww, wh = window[2:]
    pts = _edge_points(ww, wh)
    K = len(pts) + 6
    kp = mm.points_record(pts + [(ww, 3), (3, wh), (-1, 5), (2 ** 31 - 1, 2 ** 31 - 1), (-2 ** 31, 0)], K)
    cp = mm.points_record([(min(x + 3, ww - 1), max(y - 2, 0)) for x, y in pts] + [(5, 5)], K, written=len(pts))      # (5, 5): beyond written
    for box in [(0, 0, ww, wh), (10, 5, 30, 25), (-9, -9, 40, 30), (ww - 5, wh - 5, 50, 50), (200, 200, 8, 8)]:
        for kw in (dict(), dict(max_move=5), dict(max_move=3, mutual_only=0), dict(ratio=256, max_distance=256), dict(max_distance=0, ratio=1)):
            a, b = mm.record(kept, cur, window, box, kp, cp, K, **kw), mm.record_fast(kept, cur, window, box, kp, cp, K, **kw)
            assert a == b, (box, kw)
    whole = mm.Record(mm.record(kept, cur, window, (0, 0, ww, wh), kp, cp, K), K)
    assert whole.kept_valid == len(pts) and whole.current_valid == len(pts) and whole.slots[len(pts)] == (-1, 257, 257, 0)
    assert not whole.kept_descriptors[len(pts):].any() and not whole.current_descriptors[len(pts):].any()
    assert whole.kept_descriptors[:len(pts)].any(axis=1).all()
    miss = mm.Record(mm.record(kept, cur, window, (200, 200, 8, 8), kp, cp, K), K)
    assert (miss.kept_valid, miss.current_valid, miss.accepted, miss.mutual, miss.sum_dx, miss.sum_dy) == (0,) * 6
    assert miss.slots == [(-1, 257, 257, 0)] * K and not miss.kept_descriptors.any()


def test_the_descriptor_is_the_definition_at_a_corner(pictures):
    """bit 0 of the descriptor of the window's first sample, by hand: test (-6, 5, 4, -1), every sample clamped"""
    kept, _ = pictures
    win = kept[4:44, 2:60].astype(np.int64)
    p = sum(int(win[min(max(5 + dv, 0), 39), min(max(-6 + du, 0), 57)]) for dv in range(-2, 3) for du in range(-2, 3))
    q = sum(int(win[min(max(-1 + dv, 0), 39), min(max(4 + du, 0), 57)]) for dv in range(-2, 3) for du in range(-2, 3))
    assert (mm.descriptor(win, 0, 0)[0] & 1) == (1 if p < q else 0) and p != q
    assert np.array_equal(mm.box_sums(win)[12 + 5, 12 - 6], p)
    assert mm.box_sums(np.full((9, 7), 255, np.int64)).max() == 6375


def test_a_flat_picture_pins_the_tie_rules():
    flat = np.full((H, W), 77, np.uint8)
    pts = [(5, 5), (20, 9), (40, 30), (63, 47), (0, 0)]
    K = 7
    kp, cp = mm.points_record(pts + [(64, 0)], K), mm.points_record(pts[::-1], K)
    for ratio in (1, 205, 255, 256):
        for mutual_only in (0, 1):
            a = mm.record(flat, flat, WINDOWS[0], (0, 0, W, H), kp, cp, K, ratio=ratio, mutual_only=mutual_only)
            assert a == mm.record_fast(flat, flat, WINDOWS[0], (0, 0, W, H), kp, cp, K, ratio=ratio, mutual_only=mutual_only)
            r = mm.Record(a, K)
            assert not r.kept_descriptors.any() and not r.current_descriptors.any()            # no sum is below another
            assert [s[:3] for s in r.slots[:5]] == [(0, 0, 0)] * 5                               # every distance is 0: the smallest j
            assert [bool(s[3] & mm.MUTUAL) for s in r.slots[:5]] == [True, False, False, False, False] and r.mutual == 1
            want = 0 if ratio < 256 else 1 if mutual_only else 5
            assert r.accepted == want and [bool(s[3] & mm.ACCEPTED) for s in r.slots[:5]] == [ratio == 256 and (i == 0 or not mutual_only) for i in range(5)]
            assert r.slots[5] == (-1, 257, 257, 0) and r.slots[6] == (-1, 257, 257, 0)
            # the accepted slots all go to current slot 0, the point (0, 0)
            assert (r.sum_dx, r.sum_dy) == ((0, 0) if not want else (-5, -5) if want == 1 else (-sum(p[0] for p in pts), -sum(p[1] for p in pts)))


def test_every_boundary_of_the_accept_rule(pictures):
    """best == max_distance is accepted and best == max_distance + 1 is not; best * 256 == ratio * second is not accepted and one
    256th more is: on a pair of points whose best and second are known from the model itself (the boundary is then placed on them)"""
    kept, cur = pictures
    K = 4
    kp, cp = mm.points_record([(20, 12), (40, 20)], K), mm.points_record([(17, 14), (37, 22), (50, 10)], K)
    args = (kept, cur, WINDOWS[0], (0, 0, W, H), kp, cp, K)
    free = mm.Record(mm.record(*args, max_distance=256, ratio=256, mutual_only=0), K)
    assert free.accepted == 2 and [s[0] for s in free.slots[:2]] == [0, 1]                       # the content moved by (-3, 2)
    best, second = free.slots[0][1], free.slots[0][2]
    assert 0 < best < second < 257
    for max_distance, want in ((best, True), (best - 1, False)):
        a = mm.record(*args, max_distance=max_distance, ratio=256, mutual_only=0)
        assert a == mm.record_fast(*args, max_distance=max_distance, ratio=256, mutual_only=0)
        assert bool(mm.Record(a, K).slots[0][3] & mm.ACCEPTED) == want
    # around best * 256 == ratio * second: the distances read off the model, the ratio solved for
    for i in range(2):
        b, s = free.slots[i][1], free.slots[i][2]
        edge = -(-b * 256 // s)                            # the smallest ratio with best * 256 <= ratio * second
        for ratio in (edge - 1, edge, edge + 1):
            if not 1 <= ratio <= 255:
                continue
            a = mm.record(*args, max_distance=256, ratio=ratio, mutual_only=0)
            assert a == mm.record_fast(*args, max_distance=256, ratio=ratio, mutual_only=0)
            assert bool(mm.Record(a, K).slots[i][3] & mm.ACCEPTED) == (b * 256 < ratio * s), (i, ratio)
    # equality itself, on distances chosen for it: best 0 never fails the test unless second is 0 as well
    assert mm._accept(64, 128, True, 64, 128, 1) is False and mm._accept(64, 128, True, 64, 129, 1) is True
    assert mm._accept(0, 0, True, 0, 255, 1) is False and mm._accept(0, 1, True, 0, 1, 1) is True and mm._accept(0, 0, False, 0, 256, 1) is False
    assert mm._accept(65, 257, True, 64, 256, 0) is False and mm._accept(64, 257, True, 64, 256, 0) is True
