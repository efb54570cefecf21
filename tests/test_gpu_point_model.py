"""GPU: h264bsdmiOutputPointModel / pull_model through the product library.  The call reads no picture: the three input records are
built by hand (tests/model_fit_cases.py) and uploaded, one idle Decoder names the device, the output buffer starts as a fill pattern and
every record is compared with tests/model_fit_model.py byte for byte.  The vectorised form of the model is used; the CPU suite
(tests/test_point_model_cpu.py) holds it equal to the form written from the definition on these same cases.  One test chains two
pull_corners calls and pull_matches on chosen pictures into the model and the found transform into pull_remap."""
import ctypes

import numpy as np
import pytest

import corners_model as cm
import matches_model as mm
import model_fit_cases as fc
import model_fit_model as fm
import pcm_pictures as pp
from test_gpu_region_shift import H, SHIFT, W, _picture, _shifted
from test_gpu_tensor_colour import Feed

pytestmark = pytest.mark.gpu

FILL = 0x5A
CASES = fc.cases()
MODEL_NAMES = {fm.TRANSLATION: "translation", fm.SIMILARITY: "similarity"}


@pytest.fixture(autouse=True, scope="module")
def _through_the_product_library(built):
    built.use_product_library(True)
    yield
    built.use_product_library(False)


@pytest.fixture(autouse=True)
def _no_device_errors(built):
    yield
    assert built.device_errors() == 0


@pytest.fixture(scope="module")
def idle(built, _through_the_product_library):
    """a decoder that was never fed anything: it only names the device"""
    d = built.Decoder()
    yield d
    d.close()


def _records(recs):
    import torch
    return torch.tensor(np.frombuffer(b"".join(recs), np.uint8).reshape(len(recs), -1).copy(), device="cuda")


def _pull(built, decs, K, kw, recs, stream=None):
    """pull_model of hand-built records [(mrec, krec, crec)] into a buffer that starts as FILL -> (PointModel, the records' bytes)"""
    import torch
    out = torch.full((len(recs), fm.record_bytes(K)), FILL, dtype=torch.uint8, device="cuda")
    g = built.pull_model(decs, _records([r[0] for r in recs]), _records([r[1] for r in recs]), _records([r[2] for r in recs]),
                         model=MODEL_NAMES[kw["model"]], tolerance=kw["tolerance"], max_scale=kw.get("max_scale", 0),
                         min_inliers=kw.get("min_inliers"), out=out, stream=stream)
    assert g.records is out and g.max_points == K
    if stream is not None:
        stream.synchronize()
    return g, [bytes(r) for r in out.cpu().numpy()]


def _same(got, want, K, what):
    if got != want:
        g, w = fm.Record(got, K), fm.Record(want, K)
        bad = [(i, g.flags[i], w.flags[i]) for i in range(K) if g.flags[i] != w.flags[i]][:6]
        sums = [(k, g.sums[k], w.sums[k]) for k in range(fm.SUMS) if g.sums[k] != w.sums[k]][:4]
        pytest.fail(f"{what}: header {g.head()} for {w.head()}; sums {sums}; flags {bad}")


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_hand_built_case_equals_the_model(built, idle, case):
    want = fm.record_fast(case.mrec, case.krec, case.crec, case.K, **case.kw)
    g, got = _pull(built, [idle], case.K, case.kw, [(case.mrec, case.krec, case.crec)])
    _same(got[0], want, case.K, case.name)
    w = fm.Record(want, case.K)
    assert (int(g.usable[0]), int(g.hypotheses[0]), int(g.inliers[0]), int(g.found[0]), int(g.a[0]), int(g.b[0])) == w.head()[:6]
    assert g.sums[0].tolist() == w.sums and g.flags[0].tolist() == w.flags
    assert g.inlier_slots(0) == [i for i in range(case.K) if w.flags[i] & fm.INLIER]


def test_many_records_of_different_sizes_in_one_call(built, idle):
    """300 records, a different number of pairs each and one of them full: a workgroup that finishes early sits beside one that runs long"""
    K = 64
    kw, recs = fc.many_records(300, K, full=7)
    g, got = _pull(built, [idle], K, kw, recs)
    want = [fm.record_fast(*r, K, **kw) for r in recs]
    assert fm.Record(want[7], K).usable == K and len({fm.Record(w, K).usable for w in want}) == K + 1
    for r in range(len(recs)):
        _same(got[r], want[r], K, ("many", r))
    assert int(g.found.sum()) == sum(fm.Record(w, K).found for w in want) > 250


def test_records_beyond_the_count_are_untouched_and_refused_calls_write_nothing(built, idle):
    import torch
    L = built.api_lib()
    K = 7
    pairs = [((10, 20), (30, 45)), ((14, 23), (34, 48)), ((40, 41), (60, 66)), ((7, 9), (100, 3))]
    recs = [fm.inputs(K, pairs[:n]) for n in (4, 3, 2)]
    m, kp, cp = (_records([r[k] for r in recs]) for k in range(3))
    out = torch.full((3, fm.record_bytes(K)), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def call(decs, n_records, **kw):
        s = dict(data=out.data_ptr(), matches=m.data_ptr(), kept_points=kp.data_ptr(), current_points=cp.data_ptr(), max_points=K, model=1,
                 tolerance=1, max_scale=0, min_inliers=2, zero=(ctypes.c_uint32 * 3)())
        s.update(kw)
        spec = built.ModelSpec(*[s[f[0]] for f in built.ModelSpec._fields_])
        return L.h264bsdmiOutputPointModel(len(decs), (ctypes.c_void_p * max(len(decs), 1))(*decs), n_records, ctypes.byref(spec), None)

    d = idle._st
    assert call([d, d], 3) == -1 and call([], 3) == -1 and call([d], 65536) == -1
    for bad in (dict(max_points=0), dict(max_points=257), dict(model=2), dict(tolerance=256), dict(max_scale=255), dict(max_scale=4097),
                dict(min_inliers=1), dict(min_inliers=257), dict(zero=(ctypes.c_uint32 * 3)(0, 0, 1)), dict(data=out.data_ptr() + 4), dict(data=0),
                dict(matches=0), dict(kept_points=kp.data_ptr() + 2), dict(current_points=0)):
        assert call([d], 3, **bad) == -1, bad
    assert call([d], 0) == 0
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    assert call([d], 2) == 0                                               # no stream: complete on return
    got = [bytes(r) for r in out.cpu().numpy()]
    for r in range(2):
        _same(got[r], fm.record(*recs[r], K, model=fm.SIMILARITY, tolerance=1), K, ("raw", r))
    assert got[2] == bytes([FILL]) * fm.record_bytes(K)


def test_a_caller_stream_gives_what_no_stream_gives(built, idle):
    import torch
    K = 64
    kw, recs = fc.many_records(40, K, full=3)
    _, plain = _pull(built, [idle], K, kw, recs)
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    with torch.cuda.stream(side):
        _, streamed = _pull(built, [idle], K, kw, recs, stream=side)
    assert streamed == plain == [fm.record_fast(*r, K, **kw) for r in recs]


def test_several_decoders_name_the_device_and_need_no_picture(built, idle):
    other = built.Decoder()
    c = next(c for c in CASES if c.name == "two_motions_rot90_6_4_tol0")
    _, got = _pull(built, [other, idle], c.K, c.kw, [(c.mrec, c.krec, c.crec)])
    _same(got[0], fm.record(c.mrec, c.krec, c.crec, c.K, **c.kw), c.K, "two decoders")
    with pytest.raises(ValueError, match="pull_model"):
        _pull(built, [idle, idle], c.K, c.kw, [(c.mrec, c.krec, c.crec)])
    other.close()


def test_corners_matches_and_model_chained_then_the_picture_registered(built):
    """pull_corners x 2 -> pull_matches -> pull_model on chosen pictures (the shifted pair of test_gpu_region_shift.py: noise moved by
    (3, -2)) equals the corners model chained into the matches model chained into this model, byte for byte.  On the MODELS alone, before
    the device is asked (seed 1): 40 usable pairs, of which the translation fit at tolerance 0 keeps 39, every one moved by exactly
    (3, -2), and leaves one mismatch out.  So theta is that move, and affine_maps(theta) -> pull_remap(nearest) of the current picture
    equals the kept picture wherever the map stays inside the window"""
    import torch
    K = 64
    kept = np.random.default_rng(1).integers(0, 256, (H, W), dtype=np.uint8)
    cur = _shifted(kept, *SHIFT)
    window = box = (0, 0, W, H)
    kp, cp = cm.Window(kept).record(box, 3, K), cm.Window(cur).record(box, 3, K)
    mrec = mm.record_fast(kept, cur, window, box, kp, cp, K)
    want_t = fm.record(mrec, kp, cp, K, model=fm.TRANSLATION, tolerance=0)
    want_s = fm.record_fast(mrec, kp, cp, K, model=fm.SIMILARITY, tolerance=1, max_scale=512)
    wt, ws = fm.Record(want_t, K), fm.Record(want_s, K)
    assert (wt.usable, wt.inliers, wt.found) == (40, 39, 1) and ws.found and ws.inliers >= wt.inliers, (wt.head(), ws.head())
    assert (wt.sums[2] - wt.sums[0], wt.sums[3] - wt.sums[1]) == (SHIFT[0] * wt.inliers, SHIFT[1] * wt.inliers)      # every inlier moved by SHIFT

    feed = Feed(built, pp.pcm_stream([_picture(kept), _picture(cur)]))
    assert feed.step() and feed.dec.next_output_info() is not None
    c0 = built.pull_corners([feed.dec], max_points=K)
    assert built.keep_pictures([feed.dec])[0] == [1]
    same_place = built.affine_maps([[[1, 0, 0], [0, 1, 0]]], (H, W))
    first = built.pull_remap([feed.dec], same_place, channels="Y", dtype=torch.uint8, mode="nearest")[0].cpu().numpy().reshape(H, W)
    assert np.array_equal(first, kept)
    assert feed.step() and feed.dec.next_output_info() is not None
    c1 = built.pull_corners([feed.dec], max_points=K)
    assert bytes(c0.records[0].cpu().numpy()) == kp and bytes(c1.records[0].cpu().numpy()) == cp
    m = built.pull_matches([feed.dec], c0, c1)
    assert bytes(m.records[0].cpu().numpy()) == mrec
    out = torch.full((1, fm.record_bytes(K)), FILL, dtype=torch.uint8, device="cuda")
    gt = built.pull_model([feed.dec], m, c0, c1, model="translation", tolerance=0, out=out)
    _same(bytes(out[0].cpu().numpy()), want_t, K, "chained translation")
    gs = built.pull_model([feed.dec], m.records, c0.records, c1.records, model="similarity", tolerance=1, max_scale=512)
    _same(bytes(gs.records[0].cpu().numpy()), want_s, K, "chained similarity")
    assert len(gt.pairs(0, c0, c1)) == 39 and len(gt.pairs(0, c0, c1, inliers=False)) == 1
    assert all((xc - xk, yc - yk) == SHIFT for xk, yk, xc, yc in gt.pairs(0, c0, c1))
    theta = gt.theta("translation")
    assert np.array_equal(theta, [[[1, 0, SHIFT[0]], [0, 1, SHIFT[1]]]])
    assert np.allclose(gs.theta("similarity"), theta, atol=0.25)           # tolerance 1 over 64 x 48 samples: the similarity is the move, nearly

    moved = built.pull_remap([feed.dec], built.affine_maps(theta, (H, W)), channels="Y", dtype=torch.uint8, mode="nearest")[0].cpu().numpy().reshape(H, W)
    inside = np.s_[-SHIFT[1]:H, 0:W - SHIFT[0]]                            # (j + 3, i - 2) lies in the window
    assert np.array_equal(moved[inside], kept[inside]) and np.array_equal(moved[inside], first[inside])
    assert not np.array_equal(built.pull_remap([feed.dec], same_place, channels="Y", dtype=torch.uint8, mode="nearest")[0].cpu().numpy().reshape(H, W)[inside], kept[inside])
    feed.close()
