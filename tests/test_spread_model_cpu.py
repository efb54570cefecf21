"""No GPU: the background spread's numpy model (tests/spread_model.py) — every statement below follows from the rule in the header and
is asserted exactly, so that a kernel cannot pass the GPU tests by agreeing with a wrong model — and the surface of the feature: the
symbols (declared, exported, mirrored), the struct and the constants against the header, the argument errors of the Python calls."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import background_model as bm
import pcm_pictures as pp
import spread_model as spm
import stats_model as sm
from conftest import ROOT

W = H = 16
N = W * H * 3 // 2


def _random_frames(count, seed, W=W, H=H):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8) for _ in range(count)]


@pytest.mark.parametrize("moving_shift", [None, 0, 3, bm.FROZEN])
@pytest.mark.parametrize("hold", [0, 1, 16, 100, 254, 255])
@pytest.mark.parametrize("shift", range(8))
def test_with_lowest_and_highest_zero_it_is_the_plain_blend(shift, hold, moving_shift):
    """V is 0 everywhere, max(hold, V) = hold: hi, lo and the moving count are Background.blend's byte for byte"""
    plain, spread = bm.Background(W, H), spm.Spread(W, H)
    for t, cur in enumerate(_random_frames(5, seed=shift * 1000 + hold)):
        update = spm.UPDATES[t % 3]
        assert plain.blend(cur, shift, hold, moving_shift) == spread.blend_spread(cur, shift, hold, moving_shift, gain=1 + t, lowest=0, highest=0, update=update)
        assert np.array_equal(plain.hi, spread.hi) and np.array_equal(plain.lo, spread.lo)
        assert spread.V.dtype == np.uint8 and not spread.V.any()


@pytest.mark.parametrize("update", ["all", "still"])
@pytest.mark.parametrize("gain, lowest, highest", [(1, 0, 255), (2, 2, 255), (8, 10, 40), (3, 7, 7)])
def test_a_call_moves_v_by_at_most_one_and_keeps_it_in_its_range(gain, lowest, highest, update):
    m = spm.Spread(W, H)
    before = None
    for cur in _random_frames(12, seed=gain):
        m.blend_spread(cur, 3, 20, 5, gain=gain, lowest=lowest, highest=highest, update=update)
        assert m.V.min() >= lowest and m.V.max() <= highest
        if before is not None:
            assert np.abs(m.V.astype(np.int64) - before).max() <= 1
        before = m.V.astype(np.int64)
    assert highest == lowest or (m.V != lowest).any()


@pytest.mark.parametrize("lowest", [0, 3])
def test_a_constant_picture_brings_v_to_lowest_in_exactly_v0_minus_lowest_calls(lowest):
    """d = 0 from the second call on, so A = 0 and V falls by one a call: from V0 it is at `lowest` after V0 - lowest calls, not sooner"""
    cur = pp.i420(pp.flat(W, H, 90, 60, 200))
    m = spm.Spread(W, H)
    m.blend_spread(cur, 0, gain=1, lowest=lowest)
    V0 = 37
    m.V[:] = V0
    for call in range(1, V0 - lowest + 1):
        assert (m.V > lowest).all()
        m.blend_spread(cur, 0, gain=1, lowest=lowest)
        assert (m.V == V0 - call).all()
    assert (m.V == lowest).all()
    m.blend_spread(cur, 0, gain=1, lowest=lowest)
    assert (m.V == lowest).all()


@pytest.mark.parametrize("gain, a, highest", [(1, 5, 255), (2, 9, 255), (8, 40, 255), (4, 30, 50), (8, 1, 255)])
def test_alternating_pictures_take_v_to_the_gained_amplitude_in_exactly_that_many_steps(gain, a, highest):
    """pictures m + a, m - a, ... around a background that shift 7 holds at m: d = a at every call, A = min(255, gain a) is constant, so
    V climbs one a call from 0 to min(A, highest) and stays; from then on nothing is moving at hold 0 (a <= gain a <= V, or V = highest
    >= a in these cases)"""
    mid = 100
    goal = min(255, gain * a, highest)
    m = spm.Spread(W, H)
    m.blend_spread(pp.i420(pp.flat(W, H, mid, mid, mid)), 7, gain=gain, lowest=0, highest=highest)
    assert not m.V.any()
    for call in range(1, goal + 3):
        v = mid + a if call & 1 else mid - a
        _, moving = m.blend_spread(pp.i420(pp.flat(W, H, v, v, v)), 7, 0, bm.FROZEN, gain=gain, lowest=0, highest=highest)
        assert (m.hi == mid).all()                       # the sum of the excursions over goal + 2 calls stays far below 128 * 2^7
        assert (m.V == min(call, goal)).all()
        assert moving == (W * H if call - 1 < a else 0)  # V from before the call is call - 1: moving while a > V
    assert goal >= a
    _, moving = m.blend_spread(pp.i420(pp.flat(W, H, mid + a, mid, mid)), 7, 0, gain=gain, lowest=0, highest=highest)
    assert moving == 0


def test_update_none_changes_no_byte_of_v():
    m = spm.Spread(W, H)
    frames = _random_frames(6, seed=5)
    for cur in frames[:3]:
        m.blend_spread(cur, 2, 10, gain=2, lowest=1)
    before = m.V.copy()
    assert len(np.unique(before)) > 1                    # (one step a call from lowest: a sample with a small d has stopped)
    for cur in frames[3:]:
        assert m.blend_spread(cur, 2, 10, gain=8, lowest=40, highest=90, update="none")[0] == 1
        assert np.array_equal(m.V, before)
    fresh = spm.Spread(W, H)
    fresh.blend_spread(frames[0], 2, lowest=9, update="none")
    assert (fresh.V == 9).all()                          # the model starts: V = lowest


def test_update_still_changes_no_byte_under_the_moving_mask():
    """the mask is the one of the S update: luma by its own test, chroma by the four luma samples over it"""
    m = spm.Spread(W, H)
    frames = _random_frames(8, seed=6)
    m.blend_spread(frames[0], 2)
    seen_moving = seen_still = 0
    for cur in frames[1:]:
        before, hi = m.V.copy(), m.hi.copy()
        m.blend_spread(cur, 2, 60, 4, gain=2, lowest=2, update="still")
        moving = m.last_moving
        luma = moving[:W * H].reshape(H, W)
        assert np.array_equal(moving[W * H:W * H * 5 // 4].reshape(H // 2, W // 2), luma.reshape(H // 2, 2, W // 2, 2).any(axis=(1, 3)))
        assert np.array_equal(moving[W * H * 5 // 4:], moving[W * H:W * H * 5 // 4])
        assert np.array_equal(m.V[moving], before[moving])
        d = np.abs(cur.astype(np.int64) - hi)
        assert np.array_equal(m.V[~moving], spm.step(before, d, 2, 2, 255)[~moving])
        seen_moving += int(moving.sum())
        seen_still += int((m.V[~moving] != before[~moving]).sum())
    assert seen_moving and seen_still


def test_a_plain_keep_invalidates_v_and_a_plain_blend_leaves_it():
    m = spm.Spread(W, H)
    frames = _random_frames(5, seed=7)
    m.blend_spread(frames[0], 2)
    m.blend_spread(frames[1], 2, gain=4)
    before = m.V.copy()
    m.blend(frames[2], 2)
    assert np.array_equal(m.V, before)
    m.keep(frames[3])
    assert m.V is None
    twin = spm.Spread(W, H)
    twin.keep(frames[3])
    twin.V = np.full(N, 6, np.uint8)
    assert m.blend_spread(frames[4], 2, 3, gain=2, lowest=6) == twin.blend_spread(frames[4], 2, 3, gain=2, lowest=6)     # it reads as lowest
    assert np.array_equal(m.V, twin.V) and np.array_equal(m.hi, twin.hi)


BOXES = [(0, 0, 40, 24), (-7, -5, 30, 20), (21, 9, 40, 40), (3, 2, 11, 5), (-50, 0, 20, 20)]


@pytest.mark.parametrize("source", ["y", "ycbcr"])
@pytest.mark.parametrize("cell", [4, 8, 16])
def test_the_spread_planes_of_a_cell_are_the_loop_over_its_samples(cell, source):
    """boxes with negative origins, boxes that leave the window, a box that misses it, a grid larger than the box; a window inside
    the coded frame"""
    Wf, Hf = 48, 32
    cur, kept = _random_frames(2, seed=8, W=Wf, H=Hf)
    kept = np.clip(cur.astype(np.int64) + np.random.default_rng(9).integers(-20, 21, cur.shape), 0, 255).astype(np.uint8)
    spread = np.random.default_rng(10).integers(0, 24, cur.shape, dtype=np.uint8)
    planes = [sm.channels(f, Wf, Hf, source) for f in (cur, kept, spread)]
    thr = (6, 3, 2)
    for window in ((0, 0, Wf, Hf), (2, 4, 40, 26)):
        for box in BOXES:
            grid = (-(-box[3] // cell) + 1, -(-box[2] // cell) + 1)
            for bits in (15, 1 | 4, 2 | 8):
                a = spm.maps(bits, *planes, window, box, cell, grid, thr)
                b = spm.maps_by_samples(bits, *planes, window, box, cell, grid, thr)
                assert np.array_equal(a, b), (window, box, bits)
    full = spm.maps(15, *planes, (0, 0, Wf, Hf), BOXES[0], cell, (-(-24 // cell), -(-40 // cell)), thr)
    C = planes[0].shape[0]
    assert full[0].sum() == 40 * 24 and full[1:1 + C].sum() > 0 and (full[1 + C:1 + 2 * C] >= full[1:1 + C]).all()       # an excess is at least 1 a sample
    assert full[1 + 2 * C:].sum() == sum(int(planes[2][c, :24, :40].sum()) for c in range(C))
    assert not spm.maps(15, *planes, (0, 0, Wf, Hf), BOXES[4], cell, (2, 2), thr).any()


# ---- the surface

SYMBOLS = ("h264bsdmiBlendCurrentPicturesSpread", "h264bsdmiOutputKeptSpread")
CONSTANTS = dict(H264BSDMI_SPREAD_NONE=0, H264BSDMI_SPREAD_ALL=1, H264BSDMI_SPREAD_STILL=2, H264BSDMI_CELLS_SPREAD=2, H264BSDMI_CELL_FORE=2,
                 H264BSDMI_CELL_EXCESS=4, H264BSDMI_CELL_SPREADSUM=8)


def test_the_symbols_are_declared_exported_and_mirrored(built):
    text = open(os.path.join(ROOT, "include", "h264bsd_mi355x.h")).read()
    built.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", built.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text) and name in built.EXPORTED_SYMBOLS and name in exported
    assert hasattr(built, "SpreadSpec") and tuple(int(v) for v in built.__version__.split(".")) >= (0, 14, 0)
    assert "unresampled and still valid" in text           # what a warp does to the spread is said in the header


def test_the_spread_spec_and_the_constants_match_the_header(built, tmp_path):
    fields = [f[0] for f in built.SpreadSpec._fields_]
    assert fields == ["gain", "lowest", "highest", "update"]
    src = tmp_path / "spec.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "h264bsd_mi355x.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(h264bsdmi_spread_spec));\n' +
                   "".join(f'    printf("%zu\\n", offsetof(h264bsdmi_spread_spec, {f}));\n' for f in fields) +
                   "".join(f'    printf("%u\\n", (unsigned){c});\n' for c in CONSTANTS) + "    return 0;\n}\n")
    exe = tmp_path / "spec"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(built.SpreadSpec)] + [getattr(built.SpreadSpec, f).offset for f in fields] + list(CONSTANTS.values())
    assert built.capi.SPREAD_UPDATES == {name: k for k, name in enumerate(spm.UPDATES)}
    assert built.capi.CELL_SPREAD_PLANES == spm.PLANES and built.capi.CELL_AGAINST == {None: 0, "kept": 1, "spread": spm.SPREAD}
    assert len(built.capi.CELL_PLANES) == 2                # the pair of the two older modes stays a pair


@pytest.mark.parametrize("spread", [dict(gain=0), dict(gain=9), dict(lowest=-1), dict(lowest=5, highest=4), dict(highest=256), dict(update="moving"),
                                    dict(update=1), dict(gain=2.0), dict(rate=3), "all", 2])
def test_blend_pictures_refuses_a_wrong_spread_before_any_call(built, spread):
    with pytest.raises(ValueError, match="blend_pictures: spread"):
        built.blend_pictures([], spread=spread)


@pytest.mark.parametrize("who", ["pull_cells", "pull_boxes"])
@pytest.mark.parametrize("kw", [dict(keep=True), dict(source="rgb"), dict(planes=("sad",)), dict(planes=("fore", "above")), dict(against="previous"),
                                dict(against="Spread"), dict(against=2)])
def test_the_cell_pulls_refuse_what_the_spread_mode_has_not(built, who, kw):
    args = dict(against="spread", planes=("fore",))
    args.update(kw)
    with pytest.raises(ValueError, match=who):
        getattr(built, who)([], **args)


def test_the_raw_calls_refuse_a_wrong_spread_spec_on_parser_only_instances(built):
    """before any instance is looked at: -1, nothing written"""
    L = built.api_lib()
    blend = built.BlendSpec(3, 10, 3, None)
    out = [(ctypes.c_uint32 * 1)(0xA5A5A5A5) for _ in range(3)]
    dec = (ctypes.c_void_p * 1)(None)
    for bad in ((0, 0, 255, 1), (9, 0, 255, 1), (1, 6, 5, 1), (1, 0, 256, 1), (1, 256, 256, 1), (1, 0, 255, 3), (0xFFFFFFFF, 0, 255, 1)):
        assert L.h264bsdmiBlendCurrentPicturesSpread(1, dec, ctypes.byref(blend), ctypes.byref(built.SpreadSpec(*bad)), None, *out) == -1
    assert L.h264bsdmiBlendCurrentPicturesSpread(1, dec, ctypes.byref(blend), None, None, *out) == -1
    assert L.h264bsdmiBlendCurrentPicturesSpread(1, dec, None, ctypes.byref(built.SpreadSpec(1, 0, 255, 1)), None, *out) == -1
    assert L.h264bsdmiBlendCurrentPicturesSpread(0, None, None, None, None, None, None, None) == 0
    assert L.h264bsdmiOutputKeptSpread(1, dec, None, None, out[0], None) == -1 and L.h264bsdmiOutputKeptSpread(0, None, None, None, None, None) == 0
    assert all(o[0] == 0xA5A5A5A5 for o in out)
