"""tests/pcm_pictures.py: an all-I_PCM stream decodes to exactly the planes it was given (host parser + CPU oracle, and the compiled
reference where it exists), the cube pictures hold every (Y, Cb, Cr) triple, and the oracle's colour conversion — the checker the GPU
tests of chosen content compare against — is the reference's formula on all of them."""
import hashlib
import os

import numpy as np
import pytest

import pcm_pictures as pp
from oracle import pyoracle

HAVE_REF = os.path.exists(pyoracle.REF_SO)


def _random(W, H, lo, hi, seed):
    r = np.random.default_rng(seed)
    return (r.integers(lo, hi, (H, W), dtype=np.uint8), r.integers(lo, hi, (H // 2, W // 2), dtype=np.uint8),
            r.integers(lo, hi, (H // 2, W // 2), dtype=np.uint8))


def _start_code(W, H):
    """the luma plane starts with 00 00 01, and every plane holds runs of 00 00 0x"""
    Y, Cb, Cr = _random(W, H, 0, 256, 5)
    Y.reshape(-1)[:8] = (0, 0, 1, 0, 0, 0, 1, 0)
    Cb.reshape(-1)[:6] = (0, 0, 3, 0, 0, 2)
    Cr.reshape(-1)[-3:] = (0, 0, 0)
    return Y, Cb, Cr


CONTENT = {"zero": lambda W, H: pp.flat(W, H, 0, 0, 0), "low": lambda W, H: _random(W, H, 0, 4, 1), "start_code": _start_code,
           "random": lambda W, H: _random(W, H, 0, 256, 2), "steps": lambda W, H: pp.steps(W, H)}
SIZES = [(1, 1, None), (3, 2, None), (9, 5, (1, 2, 1, 3))]


@pytest.mark.parametrize("idc", [0, 1])
@pytest.mark.parametrize("wmb,hmb,crop", SIZES)
def test_decode_equals_planes(built, wmb, hmb, crop, idc):
    """three or more pictures per stream, every content kind: the decoded coded frame is concat(Y, Cb, Cr) byte for byte"""
    W, H = 16 * wmb, 16 * hmb
    pics = [CONTENT[k](W, H) for k in ("zero", "low", "start_code", "random", "steps", "zero")]
    data = pp.pcm_stream(pics, crop=crop, idc=idc)
    frames = pp.decode_oracle(data)
    assert len(frames) == len(pics)
    for k, (f, p) in enumerate(zip(frames, pics)):
        assert np.array_equal(f, pp.i420(p)), (k, np.flatnonzero(f != pp.i420(p))[:8])
    if not HAVE_REF:
        pytest.skip("oracle/_ref is absent: the compiled reference's half is left out")
    import synth
    _, ref = synth.decode_reference(data, 1)
    assert [r[0] for r in ref] == [hashlib.sha1(pp.i420(p).tobytes()).hexdigest() for p in pics]


def test_cropping_is_what_the_parser_reports(built):
    data = pp.pcm_stream([pp.flat(144, 80, 1, 2, 3)], crop=(1, 2, 1, 3))
    _, _, info = built.capture_stream(data)
    assert (info["width_mbs"], info["height_mbs"]) == (9, 5) and info["cropping"] == (1, 2, 138, 2, 72)


@pytest.fixture(scope="module")
def cube():
    return pp.cube_pictures()


def test_cube_covers_every_triple(cube):
    counts = np.zeros(1 << 24, np.int64)
    for p in cube:
        assert p[0].shape == (2048, 4096)
        counts += np.bincount(pp.triples(p).reshape(-1), minlength=1 << 24)
    assert counts.min() == 1 and counts.max() == 1


def test_cube_stream_decodes_to_the_cube(built, cube):
    frames = pp.decode_oracle(pp.pcm_stream(cube, idc=0))
    assert len(frames) == 2
    for f, p in zip(frames, cube):
        assert np.array_equal(f, pp.i420(p))


def test_oracle_conversion_is_the_reference_formula_on_the_cube(cube):
    """oracle_convert in its three formats equals the formula written out in numpy for all 2^24 triples, and where the compiled
    reference exists its h264bsdConvertTo* give the same"""
    ref = pyoracle.RefDecoder() if HAVE_REF else None
    for p in cube:
        frame = pp.i420(p)
        for fmt in range(3):
            want = pp.formula_convert(fmt, p).reshape(-1)
            assert np.array_equal(pyoracle.oracle_convert(fmt, 4096, 2048, frame), want), fmt
            if ref is not None:
                assert np.array_equal(ref.convert(fmt, 4096, 2048, frame), want), fmt
    if ref is None:
        pytest.skip("oracle/_ref is absent: the compiled reference's half is left out")


def test_steps_has_hard_edges_lines_and_a_checkerboard():
    Y, Cb, Cr = pp.steps(144, 80)
    assert set(np.unique(Y)) == {0, 255} and (Cb == 128).all() and (Cr == 128).all()
    assert (Y[0, 36:72] == (np.arange(36, 72) & 1) * 255).all() or (Y[0, 36:72] == ((np.arange(36, 72) + 1) & 1) * 255).all()
    d = np.abs(np.diff(Y[0, :36].astype(int)))
    assert d.max() == 255
