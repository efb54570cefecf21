"""No GPU: the model of h264bsdmiOutputPointModel (tests/model_fit_model.py) — the form written straight from the definition in Python
integers against the vectorised int64 form, on random records and on every hand-built case the device test uses
(tests/model_fit_cases.py) —, PointModel.theta against numpy.linalg.lstsq on the inlier pairs, the symbols, the struct and the constants
against the header, what the C call refuses before it looks at a device, the argument errors of pull_model, model_record_bytes."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import matches_model as mm
import model_fit_cases as fc
import model_fit_model as fm
from conftest import ROOT

SYMBOL = "h264bsdmiOutputPointModel"
CONSTANTS = dict(H264BSDMI_MODEL_TRANSLATION=0, H264BSDMI_MODEL_SIMILARITY=1, H264BSDMI_MODEL_USABLE=1, H264BSDMI_MODEL_INLIER=2,
                 H264BSDMI_MODEL_MAX_POINTS=256)
FIELDS = ["data", "matches", "kept_points", "current_points", "max_points", "model", "tolerance", "max_scale", "min_inliers", "zero"]
CASES = fc.cases()
PLAIN_MAX = 65                 # the plain form walks n^3 / 2 tests in Python: up to this many pairs a case


# ---- the two forms of the model ----
@pytest.mark.parametrize("case", [c for c in CASES if c.K <= PLAIN_MAX], ids=lambda c: c.name)
def test_both_forms_agree_on_the_hand_built_cases(case):
    assert fm.record(case.mrec, case.krec, case.crec, case.K, **case.kw) == fm.record_fast(case.mrec, case.krec, case.crec, case.K, **case.kw)


def test_both_forms_agree_on_random_records():
    rng = np.random.default_rng(7)
    seen = set()
    for trial in range(120):
        K = int(rng.integers(1, 25))
        n = int(rng.integers(0, K + 1))
        span = int(rng.choice([4, 30, 2000, fm.COORD_MAX + 1]))            # crowded (ties, equal points) to the whole range
        base = [(int(rng.integers(0, span)), int(rng.integers(0, span))) for _ in range(n)]
        shift = (int(rng.integers(0, 3)), int(rng.integers(0, 3)))
        pairs = [(p, (min(p[0] + shift[0], fm.COORD_MAX), min(p[1] + shift[1], fm.COORD_MAX)) if rng.integers(0, 3) else
                  (int(rng.integers(0, span)), int(rng.integers(0, span)))) for p in base]
        model = int(rng.integers(0, 2))
        kw = dict(model=model, tolerance=int(rng.choice([0, 1, 2, 5, 255])), max_scale=int(rng.choice([0, 256, 300, 4096])) if model else 0,
                  min_inliers=int(rng.integers(1 + model, 6)))
        recs = fm.inputs(K, pairs)
        want = fm.record(*recs, K, **kw)
        assert want == fm.record_fast(*recs, K, **kw), (trial, K, kw)
        r = fm.Record(want, K)
        seen.add((model, r.found))
        assert r.zero == (0, 0) and r.usable == n and (r.found or (r.inliers == 0 and r.a == r.b == -1 and not any(r.sums)))
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_the_cases_are_what_they_say():
    by = {c.name: fm.Record(fm.record_fast(c.mrec, c.krec, c.crec, c.K, **c.kw), c.K) for c in CASES}
    assert {c.K for c in CASES} >= set(fc.SIZES)
    for K in fc.SIZES:
        m = (3 * K + 4) // 5
        r = by[f"full_similarity_K{K}"]
        assert r.usable == K and r.found == (K >= 2) and r.inliers >= (m if K >= 2 and m >= 2 else 0)
        r = by[f"full_translation_K{K}"]
        assert r.usable == K and r.found == 1 and r.inliers >= m and r.b == -1
    assert by["usable_0_model0"].head() == (0, 0, 0, 0, -1, -1, (0, 0)) and by["usable_1_model1"].head() == (1, 0, 0, 0, -1, -1, (0, 0))
    assert by["usable_1_model0"].head() == (1, 1, 1, 1, 0, -1, (0, 0)) and by["usable_2_model1"].head() == (2, 1, 2, 1, 0, 1, (0, 0))
    assert by["kept_equal_similarity"].hypotheses == 0 and by["current_equal_similarity"].hypotheses == 0
    assert by["kept_equal_translation"].hypotheses == 5 and by["current_equal_translation"].found == 1
    for motion in ("rot90", "rot180", "scale2", "half", "translation"):
        assert by[f"two_motions_{motion}_6_4_tol0"].inliers == 6 and by[f"two_motions_{motion}_4_6_tol0"].inliers == 6
        tie = by[f"two_motions_{motion}_5_5_tol0"]
        assert tie.inliers == 5 and tie.a == 0                              # slot 0 belongs to the first motion: the tie goes there
        assert by[f"two_motions_{motion}_5_5_swapped"].inliers == 5 and by[f"two_motions_{motion}_5_5_swapped"].a == 0
    for name, r in by.items():
        if name.startswith("boundary_"):
            assert r.inliers == 9 and r.usable == 11, name                  # 5 exact + 4 on the boundary; 2 one step beyond
        if name.startswith("scale_gate_") and name != "scale_gate_among_many":
            assert r.usable == 2 and r.hypotheses == (0 if "beyond" in name else 1), name
    assert by["sums_256_at_16383_translation"].sums[4] == 256 * 16383 ** 2 > 2 ** 32 and by["sums_256_at_16383_translation"].inliers == 256
    assert by["sums_256_near_16383_similarity"].inliers == 256 and by["sums_256_near_16383_similarity"].sums[11] > 2 ** 36
    for bad in (-1, 16384, fc.INT_MIN, fc.INT_MAX):
        assert by[f"coordinate_{bad}_model1"].usable == 12 and by[f"coordinate_{bad}_model1"].inliers == 12
    assert by["bad_j_K16"].usable == 10 and by["bad_j_K20"].usable == 10            # j = 18 is a slot at K = 20, but behind `written`
    assert by["flags"].usable == 16 - 3
    assert by["written_0_None_K16"].usable == 0 and by["written_None_0_K16"].usable == 0 and by["written_4294967295_4294967295_K24"].usable == 16
    assert by["written_9_None_K16"].usable == 9 and 0 < by["written_None_9_K16"].usable < 16
    assert any(by[f"random_records_K{K}"].found for K in (7, 64, 256))
    for c in CASES:
        if c.name.endswith("_min_inliers_above"):
            assert by[c.name].head()[2:] == (0, 0, -1, -1, (0, 0)) and not any(by[c.name].sums) and not any(f & fm.INLIER for f in by[c.name].flags)
            assert by[c.name[:-6] + "_at"].found == 1 or c.name.startswith("usable_1")


# ---- theta ----
def _lstsq(pairs, kind):
    P = np.array(pairs, np.float64)
    x, y, u, v = P.T
    one, zero = np.ones_like(x), np.zeros_like(x)
    if kind == "translation":
        return np.array([[1, 0, (u - x).mean()], [0, 1, (v - y).mean()]])
    if kind == "similarity":                                               # u = a x - b y + tx, v = b x + a y + ty
        A = np.concatenate([np.stack([x, -y, one, zero], 1), np.stack([y, x, zero, one], 1)])
        a, b, tx, ty = np.linalg.lstsq(A, np.concatenate([u, v]), rcond=None)[0]
        return np.array([[a, -b, tx], [b, a, ty]])
    A = np.stack([x, y, one], 1)
    return np.stack([np.linalg.lstsq(A, u, rcond=None)[0], np.linalg.lstsq(A, v, rcond=None)[0]])


def _point_model(built, torch, cases):
    """a PointModel over the model's records of cases of one K, on the CPU"""
    K = cases[0].K
    recs = np.frombuffer(b"".join(fm.record_fast(c.mrec, c.krec, c.crec, K, **c.kw) for c in cases), np.uint8).reshape(len(cases), -1).copy()
    as_tensor = lambda field: torch.tensor(np.frombuffer(b"".join(getattr(c, field) for c in cases), np.uint8).reshape(len(cases), -1).copy())
    return built.PointModel(torch.tensor(recs), K, "similarity", as_tensor("mrec")), as_tensor("krec"), as_tensor("crec")


def test_theta_is_the_least_squares_fit_of_the_inlier_pairs(built):
    """against numpy.linalg.lstsq on the pairs PointModel.pairs lists.  The bound: coordinates below 2^13, a design matrix of condition
    below 10^4, float64: 2^-52 x 10^4 x 10^4 = 2 x 10^-8 in a translation; 10^-6 absolute, 10^-9 relative"""
    torch = pytest.importorskip("torch")
    cases = [c for c in CASES if c.K == 16 and (c.name.startswith(("two_motions_", "boundary_")) or c.name == "flags") and "min_inliers" not in c.name]
    assert len(cases) > 40
    g, kp, cp = _point_model(built, torch, cases)
    assert g.found.tolist() == [1] * len(cases)
    thetas = {kind: g.theta(kind) for kind in ("translation", "similarity", "affine")}
    for r, c in enumerate(cases):
        want = fm.Record(fm.record_fast(c.mrec, c.krec, c.crec, c.K, **c.kw), c.K)
        pairs = g.pairs(r, kp, cp)
        assert len(pairs) == want.inliers == int(g.inliers[r]) and g.inlier_slots(r) == [i for i in range(c.K) if want.flags[i] & fm.INLIER]
        assert len(g.pairs(r, kp, cp, inliers=False)) == want.usable - want.inliers
        assert g.sums[r].tolist() == want.sums and (int(g.a[r]), int(g.b[r])) == (want.a, want.b)
        for kind, theta in thetas.items():
            assert theta.dtype == np.float64 and theta.shape == (len(cases), 2, 3)
            assert np.allclose(theta[r], _lstsq(pairs, kind), rtol=1e-9, atol=1e-6), (c.name, kind, theta[r], _lstsq(pairs, kind))
    exact = next(r for r, c in enumerate(cases) if c.name == "two_motions_rot90_6_4_tol0")
    assert np.allclose(thetas["similarity"][exact], [[0, -1, 5000], [1, 0, 100]], atol=1e-9) and np.allclose(thetas["affine"][exact], [[0, -1, 5000], [1, 0, 100]], atol=1e-6)
    with pytest.raises(ValueError, match="theta"):
        g.theta("homography")


def test_theta_is_nan_where_nothing_was_found_or_the_moments_are_singular(built):
    torch = pytest.importorskip("torch")
    K = 7                                                                   # a stride that is no multiple of 8
    line = [((100 + 10 * k, 200 + 20 * k), (140 + 10 * k, 225 + 20 * k)) for k in range(5)]          # collinear kept points
    cases = [fc.Case("one", K, dict(model=fm.TRANSLATION, tolerance=0), *fm.inputs(K, [((5, 6), (9, 4))])),
             fc.Case("line", K, dict(model=fm.TRANSLATION, tolerance=0), *fm.inputs(K, line)),
             fc.Case("none", K, dict(model=fm.SIMILARITY, tolerance=0), *fm.inputs(K, [])),
             fc.Case("above", K, dict(model=fm.TRANSLATION, tolerance=0, min_inliers=6), *fm.inputs(K, line)),
             fc.Case("same", K, dict(model=fm.TRANSLATION, tolerance=0), *fm.inputs(K, [((5, 6), (9, 4))] * 3))]
    g, _, _ = _point_model(built, torch, cases)
    assert g.found.tolist() == [1, 1, 0, 0, 1] and g.inliers.tolist() == [1, 5, 0, 0, 3]
    alone, _, _ = _point_model(built, torch, cases[1:2])                    # one record of an odd stride: the sums are still read
    assert alone.sums.tolist() == [fm.Record(fm.record(*cases[1][3:], K, **cases[1].kw), K).sums] and np.array_equal(alone.theta("translation")[0], [[1, 0, 40], [0, 1, 25]])
    t, s, a = g.theta("translation"), g.theta("similarity"), g.theta("affine")
    assert np.array_equal(t[0], [[1, 0, 4], [0, 1, -2]]) and np.array_equal(t[1], [[1, 0, 40], [0, 1, 25]]) and np.array_equal(t[4], t[0])
    assert np.isnan(t[2]).all() and np.isnan(t[3]).all()
    assert np.isnan(s[0]).all() and np.isnan(s[4]).all() and np.allclose(s[1], [[1, 0, 40], [0, 1, 25]], atol=1e-9)      # one point; a line is enough
    assert np.isnan(a[0]).all() and np.isnan(a[1]).all() and np.isnan(a[2:]).all()                                     # collinear: singular


# ---- the symbols, the struct ----
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_symbols_are_declared_exported_and_mirrored(built):
    text = open(os.path.join(ROOT, "include", "h264bsd_mi355x.h")).read()
    built.lib()
    assert re.search(r"\bint\s+" + SYMBOL + r"\s*\(", text)
    assert SYMBOL in built.EXPORTED_SYMBOLS and SYMBOL in _exported(built.LIB_PATH) and SYMBOL in _exported(built.capi.BENCH_LIB_PATH)
    for attr in ("pull_model", "ModelSpec", "PointModel", "model_record_bytes"):
        assert hasattr(built, attr)
    assert tuple(int(v) for v in built.__version__.split(".")) >= (0, 12, 0)
    doc = text[text.index("/* Point model:"):text.index(SYMBOL + "(")]
    assert "THE DEFINITION" in doc and "tolerance^2 |p_b - p_a|^2" in doc and "Σ(uu + vv)" in doc and "then the smallest a, then the smallest b" in doc
    assert "point_model" in open(os.path.join(ROOT, "h264bsd_amd", "csrc", "engine.h")).read().split("point_matches)(")[1]     # the third member, at the end


def test_spec_layout_and_constants_match_the_header(built, tmp_path):
    assert [f[0] for f in built.ModelSpec._fields_] == FIELDS
    src = tmp_path / "spec.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "h264bsd_mi355x.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(h264bsdmi_model_spec));\n' +
                   "".join(f'    printf("%zu\\n", offsetof(h264bsdmi_model_spec, {f}));\n' for f in FIELDS) +
                   "".join(f'    printf("%u\\n", (unsigned){c});\n' for c in CONSTANTS) + "    return 0;\n}\n")
    exe = tmp_path / "spec"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(built.ModelSpec)] + [getattr(built.ModelSpec, f).offset for f in FIELDS] + list(CONSTANTS.values())
    assert built.capi.MODEL_FLAGS == dict(usable=fm.USABLE, inlier=fm.INLIER) and built.capi.MODEL_KINDS == dict(translation=0, similarity=1)


def test_model_record_bytes(built):
    assert [built.model_record_bytes(k) for k in (1, 7, 64, 256)] == [132, 156, 384, 1152] == [fm.record_bytes(k) for k in (1, 7, 64, 256)]
    for bad in (0, 257, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="model_record_bytes"):
            built.model_record_bytes(bad)


# ---- the refusals of the header, without a device ----
def _spec(built, **kw):
    s = dict(data=0x1000, matches=0x2000, kept_points=0x3000, current_points=0x4000, max_points=64, model=1, tolerance=2, max_scale=0,
             min_inliers=2, zero=(0, 0, 0))
    s.update(kw)
    return built.ModelSpec(*[s[f] if f != "zero" else (ctypes.c_uint32 * 3)(*s[f]) for f in FIELDS])


def _call(built, decoders, n_records, spec):
    dec = (ctypes.c_void_p * max(len(decoders), 1))(*[d._st if d is not None else None for d in decoders])
    return built.api_lib().h264bsdmiOutputPointModel(len(decoders), dec, n_records, ctypes.byref(spec) if spec is not None else None, None)


GOOD_SPEC = [dict(), dict(max_points=1), dict(max_points=256), dict(model=0, min_inliers=1), dict(model=0, min_inliers=256), dict(tolerance=0),
             dict(tolerance=255), dict(max_scale=256), dict(max_scale=4096), dict(min_inliers=256), dict(data=0x1008), dict(matches=0x3000)]
BAD_SPEC = [dict(data=0), dict(data=0x1004), dict(matches=0), dict(matches=0x2001), dict(kept_points=0), dict(kept_points=0x3004),
            dict(current_points=0), dict(current_points=0x4002), dict(max_points=0), dict(max_points=257), dict(max_points=2 ** 32 - 1),
            dict(model=2), dict(model=2 ** 31), dict(tolerance=256), dict(max_scale=255), dict(max_scale=1), dict(max_scale=4097),
            dict(model=0, min_inliers=1, max_scale=256), dict(min_inliers=0), dict(min_inliers=1), dict(model=0, min_inliers=0),
            dict(min_inliers=257), dict(zero=(1, 0, 0)), dict(zero=(0, 1, 0)), dict(zero=(0, 0, 1))]


def test_an_empty_call_with_a_valid_spec_is_accepted(built):
    for kw in GOOD_SPEC:
        assert _call(built, [], 0, _spec(built, **kw)) == 0, kw


@pytest.mark.parametrize("bad", BAD_SPEC, ids=str)
def test_invalid_specs_are_refused(built, bad):
    assert _call(built, [], 0, _spec(built, **bad)) == -1
    assert _call(built, [], 0, None) == -1


def test_instances_that_are_refused(built):
    """no device is reached: a capture-mode instance has none, and everything else is refused before it is looked at"""
    a, b = built.Decoder(capture="discard"), built.Decoder(capture="discard")
    spec = _spec(built)
    assert _call(built, [], 1, spec) == -1                                  # n == 0 with records
    assert _call(built, [a], 1, spec) == -1 and _call(built, [a], 0, spec) == -1 and _call(built, [a, b], 3, spec) == -1      # capture mode
    assert _call(built, [None], 1, spec) == -1 and _call(built, [a, a], 1, spec) == -1
    assert _call(built, [], 65536, spec) == -1
    assert built.api_lib().h264bsdmiOutputPointModel(1, None, 1, ctypes.byref(spec), None) == -1
    a.close()
    b.close()


class _Records:
    """what pull_model looks at of a tensor of records before the library is called"""

    def __init__(self, shape, ptr=0x1000, cuda=True, contiguous=True, dtype=None):
        import torch
        self.shape, self._ptr, self.is_cuda, self._contiguous, self.dtype = shape, ptr, cuda, contiguous, dtype or torch.uint8

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return self._contiguous

    def data_ptr(self):
        return self._ptr


def _args(K=8, R=2):
    return dict(matches=_Records((R, 32 + 80 * K)), kept_points=_Records((R, 32 + 16 * K)), current_points=_Records((R, 32 + 16 * K)))


BAD_ARGS = [dict(model="affine"), dict(model=1), dict(tolerance=-1), dict(tolerance=256), dict(tolerance=2.0), dict(tolerance=True),
            dict(max_scale=255), dict(max_scale=4097), dict(max_scale=1.5), dict(model="translation", max_scale=256), dict(min_inliers=0),
            dict(min_inliers=1), dict(min_inliers=257), dict(model="translation", min_inliers=0), dict(min_inliers=2.0),
            dict(matches="records"), dict(matches=None), dict(matches=_Records((2, 32 + 80 * 8), cuda=False)),
            dict(matches=_Records((2, 32 + 80 * 8), contiguous=False)), dict(matches=_Records((2, 32 + 80 * 8), ptr=0x1004)),
            dict(matches=_Records((2, 32 + 80 * 8 + 16))), dict(matches=_Records((2, 32))), dict(matches=_Records((2, 32 + 80 * 257))),
            dict(matches=_Records((32 + 80 * 8,))), dict(matches=_Records((65536, 32 + 80 * 8))), dict(matches=_Records((2, 32 + 80 * 7))),
            dict(kept_points=_Records((3, 32 + 16 * 8))), dict(current_points=_Records((2, 32 + 16 * 9))), dict(kept_points=None),
            dict(current_points=_Records((2, 32 + 16 * 8), ptr=0x1002))]


@pytest.mark.parametrize("kw", BAD_ARGS, ids=lambda kw: ",".join(kw))
def test_pull_model_refuses_bad_arguments(built, kw, monkeypatch):
    """before any library call: the call is taken away for the test, so a refusal that came too late would not be a ValueError"""
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(torch, "Tensor", _Records)              # the stand-in passes for a tensor: no device is needed to refuse
    monkeypatch.setattr(built.capi, "_model_call", lambda *args, **kws: pytest.fail("the library was called"))
    monkeypatch.setattr(built.capi, "_out_and_stream", lambda *args, **kws: pytest.fail("an output was allocated"))
    a = built.Decoder(capture="discard")
    with pytest.raises(pytest.fail.Exception, match="an output was allocated"):
        built.pull_model([a], **_args())                        # the arguments as they stand pass every check
    with pytest.raises(pytest.fail.Exception, match="an output was allocated"):
        built.pull_model([a], **dict(_args(), model="translation", min_inliers=1, tolerance=255))
    with pytest.raises(ValueError, match="pull_model"):
        built.pull_model([a], **dict(_args(), **kw))
    a.close()


def test_pull_model_refuses_decoders_and_what_the_c_call_refuses(built, monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(torch, "Tensor", _Records)
    a = built.Decoder(capture="discard")
    monkeypatch.setattr(built.capi, "_out_and_stream", lambda *args, **kws: pytest.fail("an output was allocated"))
    for decoders in ([], [a, a], ["decoder"]):
        with pytest.raises(ValueError, match="pull_model"):
            built.pull_model(decoders, **_args())

    class _Stream:
        cuda_stream = 0
    monkeypatch.setattr(built.capi, "_out_and_stream", lambda who, out, shape, dtype, stream, aligned=False: (_Records(shape, ptr=0x9000), _Stream()))
    with pytest.raises(ValueError, match="pull_model.*refused"):           # a capture-mode instance: -1 from the library itself
        built.pull_model([a], **_args())
    a.close()
    with pytest.raises(ValueError, match="pull_model"):
        built.pull_model([a], **_args())                                    # closed
