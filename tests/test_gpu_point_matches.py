"""GPU: h264bsdmiOutputPointMatches / pull_matches through the product library.  The pictures are chosen (tests/pcm_pictures.py, as in
test_gpu_region_shift.py), so both the kept and the current picture are known exactly, and every record is compared with
tests/matches_model.py byte for byte.  Every call writes into a buffer that starts as a pattern: the whole record is written, and an
untouched record stays the pattern.  The point records are built by hand and uploaded, except where two pull_corners calls are chained
into the matching."""
import numpy as np
import pytest

import corners_model as cm
import matches_model as mm
import pcm_pictures as pp
from test_gpu_region_shift import CROP, H, SHIFT, W, Chosen, _picture, _shifted
from test_gpu_tensor_colour import Feed

pytestmark = pytest.mark.gpu

FILL = 0x5A


@pytest.fixture(autouse=True, scope="module")
def _through_the_product_library(built):
    built.use_product_library(True)
    yield
    built.use_product_library(False)


@pytest.fixture(autouse=True)
def _no_device_errors(built):
    yield
    assert built.device_errors() == 0


def _records(recs):
    """point records (bytes, one per region) as a device tensor"""
    import torch
    return torch.tensor(np.frombuffer(b"".join(recs), np.uint8).reshape(len(recs), -1).copy(), device="cuda")


def _pull(built, decs, kpts, cpts, regions, K, **kw):
    """pull_matches of hand-built point records into a record buffer that starts as FILL -> (PointMatches, the records' bytes)"""
    import torch
    R = len(decs) if regions is None else len(regions)
    out = torch.full((R, mm.record_bytes(K)), FILL, dtype=torch.uint8, device="cuda")
    m = built.pull_matches(decs, _records(kpts), _records(cpts), regions, out=out, **kw)
    assert m.records is out and m.max_points == K
    return m, [bytes(r) for r in out.cpu().numpy()]


def _same(got, want, K, what):
    if got != want:
        g, w = mm.Record(got, K), mm.Record(want, K)
        head = lambda r: (r.kept_valid, r.current_valid, r.accepted, r.mutual, r.sum_dx, r.sum_dy)
        bad = [(i, g.slots[i], w.slots[i]) for i in range(K) if g.slots[i] != w.slots[i]][:4]
        dk = np.nonzero((g.kept_descriptors != w.kept_descriptors).any(axis=1))[0][:6].tolist()
        dc = np.nonzero((g.current_descriptors != w.current_descriptors).any(axis=1))[0][:6].tolist()
        pytest.fail(f"{what}: header {head(g)} for {head(w)}; slots {bad}; kept descriptors {dk}; current descriptors {dc}")


def _model_kw(kw):
    """pull_matches' arguments as the model's"""
    return dict(max_distance=kw.get("max_distance", 64), ratio=kw.get("ratio", 205), max_move=kw.get("max_move", 0),
                mutual_only=1 if kw.get("mutual", True) else 0)


@pytest.fixture(scope="module", params=[False, True], ids=["coded", "cropped"])
def small(request, built, _through_the_product_library):
    rng = np.random.default_rng(5)
    K = rng.integers(0, 256, (H, W), dtype=np.uint8)
    c = Chosen(built, [K, _shifted(K, *SHIFT)], crop=CROP["crop"] if request.param else None)
    c.window = CROP["window"] if request.param else (0, 0, W, H)
    yield c
    c.close()


def _descriptor_points(window):
    """the four window corners, each edge, 13, 14 and 15 samples from each border, x or y = 0 and 15 mod 16 in the coded frame, the
    interior"""
    wx, wy, ww, wh = window
    pts = [(0, 0), (ww - 1, 0), (0, wh - 1), (ww - 1, wh - 1), (ww // 2, 0), (ww // 2, wh - 1), (0, wh // 2), (ww - 1, wh // 2)]
    for d in (13, 14, 15):
        pts += [(d, wh // 2), (ww - 1 - d, wh // 2), (ww // 2, d), (ww // 2, wh - 1 - d), (d, d), (ww - 1 - d, wh - 1 - d), (d, wh - 1 - d)]
    pts += [(16 - wx, 21), (31 - wx, 21), (32 - wx, 9), (47 - wx, 30), (20, 16 - wy), (20, 31 - wy), (33, 32 - wy), (16 - wx, 16 - wy), (31 - wx, 31 - wy)]
    return pts + [(ww // 2, wh // 2), (ww // 2 + 3, wh // 2 - 2), (29, 19)]


def test_descriptors_at_every_clamp_and_tile_edge_equal_the_definition(built, small):
    """a patch of 29 x 29 around each point crosses the tiles of 16 and all four clamps of the window; both descriptor blocks, the slots
    and the header equal the model in the form written straight from the definition"""
    ww, wh = small.window[2:]
    pts = _descriptor_points(small.window)
    assert all(0 <= x < ww and 0 <= y < wh for x, y in pts)
    K = 64
    assert len(pts) <= K
    kp = mm.points_record(pts, K)
    cp = mm.points_record([(min(max(x + SHIFT[0], 0), ww - 1), min(max(y + SHIFT[1], 0), wh - 1)) for x, y in pts], K)
    box = (0, 0, ww, wh)
    want = mm.record(small.lumas[0], small.lumas[1], small.window, box, kp, cp, K)
    assert want == mm.record_fast(small.lumas[0], small.lumas[1], small.window, box, kp, cp, K)
    w = mm.Record(want, K)
    assert w.kept_valid == w.current_valid == len(pts) and w.accepted >= 20      # the shifted pair: the interior points find themselves
    m, got = _pull(built, [small.dec], [kp], [cp], None, K)
    assert m.got == [1] and m.current == [1] and m.kept == [1]
    _same(got[0], want, K, "descriptors")
    assert np.array_equal(m.kept_descriptors[0].cpu().numpy(), w.kept_descriptors)
    assert np.array_equal(m.current_descriptors[0].cpu().numpy(), w.current_descriptors)
    assert (int(m.kept_valid[0]), int(m.current_valid[0]), int(m.accepted[0]), int(m.mutual[0]), int(m.sum_dx[0]), int(m.sum_dy[0])) == \
           (w.kept_valid, w.current_valid, w.accepted, w.mutual, w.sum_dx, w.sum_dy)
    assert [tuple(v) for v in zip(m.j[0].tolist(), m.best[0].tolist(), m.second[0].tolist(), m.flags[0].tolist())] == w.slots
    pairs = m.pairs(0, _records([kp]), _records([cp]))
    assert len(pairs) == w.accepted and all(p[4] == w.slots[i][1] for p, i in zip(pairs, [i for i in range(K) if w.slots[i][3] & mm.ACCEPTED]))
    assert len(m.moved(29, [(0,) + box], _records([cp]))) == w.accepted


def _some_points(rng, n, ww, wh):
    return [(int(rng.integers(0, ww)), int(rng.integers(0, wh))) for _ in range(n)]


@pytest.mark.parametrize("K", [1, 7, 64, 256])
def test_slots_of_every_kind_equal_the_model(built, small, K):
    """written of 0, below K, equal to K and 0xFFFFFFFF; points outside the box, outside the window, negative and 2^31 - 1; an empty
    kept side and an empty current side; a box that misses the window; K = 256 with duplicate and dense points.  One call, one region
    per case"""
    ww, wh = small.window[2:]
    rng = np.random.default_rng(100 + K)
    if K == 256:
        dense = [(20 + i % 16, 10 + i // 16) for i in range(200)]               # adjacent samples: descriptors a few bits apart
        full = dense + dense[:40] + _some_points(rng, 16, ww, wh)               # and duplicates: distance 0, the smallest j
    else:
        full = _some_points(rng, K, ww, wh)
    moved = [(min(max(x + SHIFT[0], 0), ww - 1), min(max(y + SHIFT[1], 0), wh - 1)) for x, y in full]
    odd = ([(ww, 5), (5, wh), (-1, 5), (5, -1), (2 ** 31 - 1, 2 ** 31 - 1), (-2 ** 31, -2 ** 31), (2 ** 31 - 1, 3)] * K)[:K]
    mixed = [p if i % 3 else o for i, (p, o) in enumerate(zip(full, odd))]
    whole, inner, miss = (0, 0, ww, wh), (10, 5, 30, 25), (200, 200, 8, 8)
    cases = [(mm.points_record(full, K), mm.points_record(moved, K), whole),                            # written == K
             (mm.points_record(full, K, written=0xFFFFFFFF), mm.points_record(moved, K, written=K + 1), whole),
             (mm.points_record(full, K, written=K // 2), mm.points_record(moved, K, written=(K + 1) // 2), whole),
             (mm.points_record(full, K, written=0), mm.points_record(moved, K), whole),                 # an empty kept side
             (mm.points_record(full, K), mm.points_record(moved, K, written=0), whole),                 # an empty current side
             (mm.points_record(mixed, K), mm.points_record(moved, K), whole),
             (mm.points_record(full, K), mm.points_record(mixed, K, written=0xFFFFFFFF), inner),        # outside the box
             (mm.points_record(full, K), mm.points_record(moved, K), (-9, -9, 40, 30)),
             (mm.points_record(full, K), mm.points_record(moved, K), miss)]
    kw = dict(mutual=K != 7, max_distance=80)
    want = [mm.record_fast(small.lumas[0], small.lumas[1], small.window, box, kp, cp, K, **_model_kw(kw)) for kp, cp, box in cases]
    if K <= 7:
        for (kp, cp, box), w in zip(cases, want):
            assert w == mm.record(small.lumas[0], small.lumas[1], small.window, box, kp, cp, K, **_model_kw(kw))
    assert mm.Record(want[3], K).kept_valid == 0 and mm.Record(want[4], K).current_valid == 0 and mm.Record(want[4], K).kept_valid == K
    assert mm.Record(want[4], K).slots == [(-1, 257, 257, mm.VALID)] * K and want[8][:32 + 16 * K] == bytes(32) + bytes.fromhex("ffffffff010100000101000000000000") * K
    assert not any(want[8][32 + 16 * K:])
    if K == 256:
        assert mm.Record(want[0], K).slots[200][:3] == mm.Record(want[0], K).slots[0][:3]       # a duplicate point: the same answer
    m, got = _pull(built, [small.dec], [c[0] for c in cases], [c[1] for c in cases], [(0,) + c[2] for c in cases], K, **kw)
    assert m.got == [1] * len(cases)
    for k in range(len(cases)):
        _same(got[k], want[k], K, ("slots", K, k))


def test_the_flat_picture_pins_the_ties(built):
    flat = np.full((H, W), 77, np.uint8)
    c = Chosen(built, [flat, flat])
    pts = [(5, 5), (20, 9), (40, 30), (63, 47), (0, 0)]
    K = 7
    kp, cp = mm.points_record(pts + [(64, 0)], K), mm.points_record(pts[::-1], K)
    for kw in (dict(ratio=256, mutual=True), dict(ratio=256, mutual=False), dict(ratio=255, mutual=False), dict()):
        want = mm.record(flat, flat, (0, 0, W, H), (0, 0, W, H), kp, cp, K, **_model_kw(kw))
        w = mm.Record(want, K)
        assert [s[:3] for s in w.slots[:5]] == [(0, 0, 0)] * 5 and w.mutual == 1
        assert w.accepted == (0 if kw.get("ratio") != 256 else 1 if kw["mutual"] else 5)
        _same(_pull(built, [c.dec], [kp], [cp], None, K, **kw)[1][0], want, K, ("flat", kw))
    c.close()


def test_max_move_the_accept_boundaries_and_mutual_only(built, small):
    """the content moved by SHIFT = (3, -2): max_move 1 sees no true pair, 5 sees them all, 0 does not gate; max_distance at the best
    of a slot and one below it; the ratio around best * 256 == ratio * second of a slot; mutual_only on and off"""
    ww, wh = small.window[2:]
    rng = np.random.default_rng(77)
    K = 64
    # 40 distinct points whose patches meet no clamp in either picture: [14, 41) x [16, 26) lies that deep in both windows
    pts = [(14 + int(k) % 27, 16 + int(k) // 27) for k in rng.choice(27 * 10, 40, replace=False)]
    kp = mm.points_record(pts, K)
    cp = mm.points_record([(x + SHIFT[0], y + SHIFT[1]) for x, y in pts[::-1]] + [(x + 1, y) for x, y in pts[:12]] + [(x, y + 1) for x, y in pts[:12]], K)
    args = (small.lumas[0], small.lumas[1], small.window, (0, 0, ww, wh), kp, cp, K)
    free = mm.Record(mm.record_fast(*args, max_distance=256, ratio=256, mutual_only=0), K)
    truth = [i for i in range(40) if free.slots[i][0] == 39 - i]
    assert len(truth) >= 36 and all(free.slots[i][1] == 0 for i in truth)          # the interior of a pure shift: distance 0
    cases = [dict(max_move=0), dict(max_move=1), dict(max_move=5), dict(max_move=5, mutual=False), dict(max_move=2, mutual=False, ratio=256, max_distance=256),
             dict(mutual=False), dict(mutual=False, ratio=256), dict(max_distance=0), dict(max_distance=0, ratio=256, mutual=False)]
    # second-best distances of the true pairs give the ratio's boundary: best 0 passes any ratio; a slot with best > 0 (a clamped patch
    # or a gated search) gives both sides of best * 256 == ratio * second
    gated = mm.Record(mm.record_fast(*args, max_distance=256, ratio=256, max_move=1, mutual_only=0), K)
    i1 = next(i for i in range(40) if 0 < gated.slots[i][1] < gated.slots[i][2] < 257)
    b, s = gated.slots[i1][1], gated.slots[i1][2]
    edge = -(-b * 256 // s)
    cases += [dict(max_move=1, mutual=False, max_distance=256, ratio=r) for r in (edge - 1, edge, edge + 1) if 1 <= r <= 256]
    cases += [dict(max_move=1, mutual=False, ratio=256, max_distance=d) for d in (b - 1, b, b + 1)]
    for kw in cases:
        want = mm.record_fast(*args, **_model_kw(kw))
        w = mm.Record(want, K)
        if kw == dict(max_move=1):
            assert not any(w.slots[i][0] == 39 - i for i in range(40))
        if kw == dict(max_move=5):
            assert sum(1 for i in range(40) if w.slots[i][0] == 39 - i and w.slots[i][3] & mm.ACCEPTED) >= 30
        if kw.get("max_move") == 1 and "ratio" in kw and kw["ratio"] != 256:
            assert bool(w.slots[i1][3] & mm.ACCEPTED) == (b * 256 < kw["ratio"] * s)
        if kw.get("max_move") == 1 and kw.get("ratio") == 256 and "max_distance" in kw:
            assert bool(w.slots[i1][3] & mm.ACCEPTED) == (b <= kw["max_distance"])
        _same(_pull(built, [small.dec], [kp], [cp], None, K, **kw)[1][0], want, K, ("rules", kw))


def test_instances_regions_streams_and_the_keep_chain(built):
    """two decoders of different sizes in one call, several regions per decoder in mixed order, one decoder without a kept picture
    (got 0, its records stay the pattern), a caller's stream; keep=True: the second call compares with the first call's pictures"""
    import torch
    rng = np.random.default_rng(29)
    sizes = [(64, 48), (96, 80), (48, 32)]
    lumas = [[rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(3)] for w, h in sizes]
    a, b = Chosen(built, lumas[0]), Chosen(built, lumas[1])
    fresh = Feed(built, pp.pcm_stream([_picture(Y) for Y in lumas[2]]))       # a current picture, nothing kept
    assert fresh.step() and fresh.dec.next_output_info() is not None
    decs = [a.dec, fresh.dec, b.dec]
    regions = [(2, 0, 0, 96, 80), (0, -5, 3, 40, 30), (1, 0, 0, 48, 32), (2, 10, -4, 50, 33), (0, 0, 0, 64, 48), (1, 3, 3, 20, 20)]
    K = 7

    def inside(d, x, y, w, h):
        """K points, the first five in box ∩ window, the others anywhere in the window"""
        ww, wh = sizes[(0, 2, 1)[d]]
        x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, ww), min(y + h, wh)
        return [(x0 + px % (x1 - x0), y0 + py % (y1 - y0)) for px, py in _some_points(rng, 5, ww, wh)] + _some_points(rng, K - 5, ww, wh)

    kps = [mm.points_record(inside(*r), K) for r in regions]
    cps = [mm.points_record(inside(*r), K) for r in regions]
    kw = dict(max_distance=200, ratio=256, mutual=False)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        m, got = _pull(built, decs, kps, cps, regions, K, keep=True, stream=stream, **kw)
    stream.synchronize()
    assert m.got == [1, 1, 0, 1, 1, 0] and m.current == [1, 1, 1] and m.kept == [1, 0, 1]
    first_ids = m.pic_id
    for k, (d, *box) in enumerate(regions):
        if d == 1:
            assert got[k] == bytes([FILL]) * mm.record_bytes(K)
            continue
        w, h = sizes[0 if d == 0 else 1]
        ls = lumas[0 if d == 0 else 1]
        want = mm.record(ls[0], ls[1], (0, 0, w, h), tuple(box), kps[k], cps[k], K, **_model_kw(kw))
        assert mm.Record(want, K).kept_valid >= 5 and mm.Record(want, K).accepted >= 1
        _same(got[k], want, K, ("first", k))
    # the chain: everyone's kept picture is now the current one of the first call; a and b decode on, fresh stays
    a.next()
    b.next()
    m, got = _pull(built, decs, kps, cps, regions, K, **kw)
    assert m.got == [1] * 6 and m.kept == [1, 1, 1] and m.kept_pic_id == first_ids
    pics = {0: (lumas[0][1], lumas[0][2], sizes[0]), 1: (lumas[2][0], lumas[2][0], sizes[2]), 2: (lumas[1][1], lumas[1][2], sizes[1])}
    for k, (d, *box) in enumerate(regions):
        kept, cur, (w, h) = pics[d]
        _same(got[k], mm.record(kept, cur, (0, 0, w, h), tuple(box), kps[k], cps[k], K, **_model_kw(kw)), K, ("second", k))
    # the same records on both sides of the same picture: every valid slot finds itself at distance 0
    m, got = _pull(built, [fresh.dec], [kps[2]], [kps[2]], None, K, **kw)
    w = mm.Record(got[0], K)
    assert w.kept_valid == w.current_valid == K and all(s[1] == 0 for s in w.slots) and (w.sum_dx, w.sum_dy) == (0, 0)
    for c in (a, b, fresh):
        c.close()


BW, BH, MOVE = 176, 144, (40, 25)


def _smoothed_pair(seed):
    """kept: noise under a 5 x 5 mean, stretched to the full range; current: the same moved by MOVE, perturbed by +-2"""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, 256, (BH + 8, BW + 8)).astype(np.float64)
    c = np.pad(n.cumsum(axis=0).cumsum(axis=1), ((1, 0), (1, 0)))
    s = (c[5:, 5:] - c[:-5, 5:] - c[5:, :-5] + c[:-5, :-5])[:BH, :BW] / 25
    kept = np.floor((s - s.min()) / (s.max() - s.min()) * 255 + 0.5).astype(np.uint8)
    cur = _shifted(kept, *MOVE).astype(np.int64) + rng.integers(-2, 3, (BH, BW))
    return kept, np.clip(cur, 0, 255).astype(np.uint8)


def test_corner_points_chained_into_matches_beyond_the_radius(built):
    """the reason for the call: the content moves by (40, 25), which pull_shift at radius 16 cannot reach.  Two pull_corners calls are
    passed straight on; the record equals the corners model chained into the matches model.  On the MODEL alone, before the device is
    asked: at least 16 slots are accepted, and at least 3/4 of them moved within Chebyshev 1 of (40, 25) (seed 1: 41 of 41)"""
    K = 64
    kept, cur = _smoothed_pair(1)
    window = box = (0, 0, BW, BH)
    kp, cp = cm.Window(kept).record(box, 3, K), cm.Window(cur).record(box, 3, K)
    want = mm.record_fast(kept, cur, window, box, kp, cp, K)
    w = mm.Record(want, K)
    ks, cs = mm.slots(kp, K, window, box), mm.slots(cp, K, window, box)
    accepted = [i for i in range(K) if w.slots[i][3] & mm.ACCEPTED]
    near = [i for i in accepted if max(abs(cs[w.slots[i][0]][0] - ks[i][0] - MOVE[0]), abs(cs[w.slots[i][0]][1] - ks[i][1] - MOVE[1])) <= 1]
    assert len(accepted) >= 16 and 4 * len(near) >= 3 * len(accepted), (len(accepted), len(near))
    assert w.accepted == len(accepted) and abs(w.sum_dx - MOVE[0] * w.accepted) <= w.accepted and abs(w.sum_dy - MOVE[1] * w.accepted) <= w.accepted

    import torch
    feed = Feed(built, pp.pcm_stream([_picture(kept), _picture(cur)]))
    assert feed.step() and feed.dec.next_output_info() is not None
    c0 = built.pull_corners([feed.dec], max_points=K)
    assert built.keep_pictures([feed.dec])[0] == [1]
    assert feed.step() and feed.dec.next_output_info() is not None
    c1 = built.pull_corners([feed.dec], max_points=K)
    assert bytes(c0.records[0].cpu().numpy()) == kp and bytes(c1.records[0].cpu().numpy()) == cp
    out = torch.full((1, mm.record_bytes(K)), FILL, dtype=torch.uint8, device="cuda")
    m = built.pull_matches([feed.dec], c0, c1, keep=True, out=out)
    assert m.got == [1] and m.kept == [1]
    _same(bytes(out[0].cpu().numpy()), want, K, "beyond the radius")
    pairs = m.pairs(0, c0, c1)
    assert len(pairs) == len(accepted) and pairs[0][:4] == ks[accepted[0]][:2] + cs[w.slots[accepted[0]][0]][:2]
    boxes = m.moved(29, [(0,) + box], c1)
    assert len(boxes) == len(accepted) and boxes[0] == (0, pairs[0][2] - 14, pairs[0][3] - 14, 29, 29)
    with pytest.raises(ValueError, match="pull_matches"):
        built.pull_matches([feed.dec], c0, built.pull_corners([feed.dec], max_points=32))
    feed.close()


def test_raw_calls_that_must_be_refused_write_nothing(built, small):
    import ctypes
    import torch
    L = built.api_lib()
    K = 7
    out = torch.full((2, mm.record_bytes(K)), FILL, dtype=torch.uint8, device="cuda")
    pts = _records([mm.points_record([(20, 20), (30, 12)], K)] * 2)
    torch.cuda.synchronize()
    S = 0xA5A5A5A5

    def call(decs, regs, **kw):
        s = dict(data=out.data_ptr(), kept_points=pts.data_ptr(), current_points=pts.data_ptr(), max_points=K, max_distance=64, ratio=205,
                 max_move=0, mutual_only=1, crop=1, keep_after=0, zero=0)
        s.update(kw)
        spec = built.MatchesSpec(*[s[f[0]] for f in built.MatchesSpec._fields_])
        arrays = [(ctypes.c_uint32 * 2)(S, S) for _ in range(5)]
        regions = (built.Region * 2)(*[built.Region(*r) for r in regs])
        rc = L.h264bsdmiOutputPointMatches(len(decs), (ctypes.c_void_p * len(decs))(*decs), 2, regions, ctypes.byref(spec), None, *arrays)
        return rc, [list(a) for a in arrays]

    good = [(0, 0, 0, 58, 40), (0, 10, 10, 30, 20)]
    untouched = (-1, [[S, S]] * 5)
    d = small.dec._st
    assert call([d, d], good) == untouched                               # repeated instances
    for bad in (dict(max_points=0), dict(max_points=257), dict(max_distance=257), dict(ratio=0), dict(ratio=257), dict(max_move=65536),
                dict(mutual_only=2), dict(crop=2), dict(keep_after=2), dict(zero=1), dict(data=out.data_ptr() + 4), dict(data=0),
                dict(kept_points=0), dict(current_points=pts.data_ptr() + 2)):
        assert call([d], good, **bad) == untouched, bad
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    rc, arrays = call([d], good)
    assert rc == 0 and arrays[0] == [1, 1]
    torch.cuda.synchronize()
    rec = mm.points_record([(20, 20), (30, 12)], K)
    for k, r in enumerate(good):
        _same(bytes(out[k].cpu().numpy()), mm.record(small.lumas[0], small.lumas[1], small.window, r[1:], rec, rec, K), K, ("raw", k))
