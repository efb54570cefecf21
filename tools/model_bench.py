#!/usr/bin/env python3
"""What the point model costs (h264bsdmiOutputPointModel / pull_model) beside the call it follows and the route a caller had without it.

N instances decode the 1080p golden stream through BatchDriver; pull_corners of the whole windows at K points, the pictures are kept,
two more are popped, pull_corners again and pull_matches of the two.  The timed calls (HIP events on a torch stream around the work; per
figure [median, min, max] in ms over --reps after --warmup calls of the same shape), for each K of --points:
  matches_k<K>_ms             the pull_matches call that precedes the model, on the pictures;
  model_<m>_k<K>_ms           pull_model, m = translation and similarity, on FULLY POPULATED records made by hand — every slot an
                              accepted match with both points in range, 70 % of them under one rotation + scale + shift, the rest
                              anywhere in the window —, N records: K usable pairs each, K (K - 1) / 2 hypotheses a record;
  model_<m>_matched_k<K>_ms   the same call on the records pull_matches gave for the pictures; usable_matched_k<K> is the mean number
                              of usable pairs a record there;
  torch_<m>_k<K>_ms           (not with --kernel-only) the same consensus in torch on the device over the hand-made records: int64
                              tensors [N, hypotheses of a chunk, K], the running best kept as count << 20 | reversed index; inliers, a
                              and b are first checked EQUAL to the call's.
Prints one JSON line.

usage: model_bench.py [--streams 256] [--reps 20] [--warmup 2] [--points 64,256] [--kernel-only]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                    # noqa: E402  (torch's HIP runtime first: capi._share_torch_hip_runtime)
import h264bsd_amd as h                         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=256)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--points", default="64,256")
ap.add_argument("--kernel-only", action="store_true")
args = ap.parse_args()
points = [int(k) for k in args.points.split(",")]

data = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "test_1920x1080.h264"), "rb").read()
N, W, H = args.streams, 1920, 1080
L = h.api_lib()
decs = [h.Decoder(no_output_reordering=1) for _ in range(N)]
drv = h.BatchDriver(decs, [data] * N)
TOLERANCE = 2


def next_round():
    assert len(drv.step()) == N
    assert L.h264bsdmiFlush() == 0
    for d in decs:
        assert d.next_output_info() is not None


def timed(call, reps, warmup):
    st = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for rep in range(warmup + reps):
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            e0.record(st)
            call(st)
            e1.record(st)
        st.synchronize()
        if rep >= warmup:
            ms.append(e0.elapsed_time(e1))
    ms.sort()
    return [round(ms[len(ms) // 2], 4), round(ms[0], 4), round(ms[-1], 4)]


def populated(K, rng):
    """N hand-made records of each kind with every slot a usable pair -> (matches, kept points, current points) as device tensors, and
    the pairs [N, K, 4] int64 in slot order"""
    kept = np.stack([rng.integers(200, W - 200, (N, K)), rng.integers(200, H - 200, (N, K))], axis=2)
    c, s = 1.05 * np.cos(0.05), 1.05 * np.sin(0.05)
    moved = np.stack([c * kept[..., 0] - s * kept[..., 1] + 31.0, s * kept[..., 0] + c * kept[..., 1] - 17.0], axis=2)
    moved = np.rint(moved + rng.uniform(-1.0, 1.0, moved.shape)).astype(np.int64)
    anywhere = np.stack([rng.integers(0, W, (N, K)), rng.integers(0, H, (N, K))], axis=2)
    cur = np.where(rng.random((N, K, 1)) < 0.7, moved, anywhere)
    assert cur.min() >= 0 and cur.max() <= 16383
    j = np.stack([rng.permutation(K) for _ in range(N)])
    m = np.zeros((N, 8 + 20 * K), np.int32)
    m[:, 8:8 + 4 * K:4], m[:, 11:8 + 4 * K:4] = j, 7
    pts = np.zeros((2, N, 8 + 4 * K), np.int32)
    pts[:, :, 2] = K
    pts[0, :, 8::4], pts[0, :, 9::4] = kept[..., 0], kept[..., 1]
    rows = np.arange(N)[:, None]
    pts[1, rows, 8 + 4 * j], pts[1, rows, 9 + 4 * j] = cur[..., 0], cur[..., 1]
    dev = lambda a: torch.tensor(a.view(np.uint8).reshape(N, -1), device="cuda")
    return dev(m), dev(pts[0]), dev(pts[1]), torch.tensor(np.concatenate([kept, cur], axis=2), device="cuda")


def torch_route(P, model, tolerance, chunk):
    """(inliers, a, b) [N] of the consensus over the pairs P [N, K, 4], every pair usable, no scale gate"""
    K, T2 = P.shape[1], tolerance * tolerance
    if model == "translation":
        d = P[..., 2:] - P[..., :2]
        e = d[:, None, :, :] - d[:, :, None, :]
        counts = ((e * e).sum(3) <= T2).sum(2)
        a = counts.argmax(1)                    # (ties: torch's argmax names no order; the check below tolerates none, the data has none)
        return counts.gather(1, a[:, None])[:, 0], a, torch.full_like(a, -1)
    ia, ib = torch.triu_indices(K, K, 1, device="cuda")
    best = torch.full((P.shape[0],), -1, dtype=torch.int64, device="cuda")
    for at in range(0, ia.numel(), chunk):
        A, B = P[:, ia[at:at + chunk]], P[:, ib[at:at + chunk]]
        Pv, Qv = B[..., :2] - A[..., :2], B[..., 2:] - A[..., 2:]
        PP, QQ = (Pv * Pv).sum(2), (Qv * Qv).sum(2)
        dp, dq = P[:, None, :, :2] - A[:, :, None, :2], P[:, None, :, 2:] - A[:, :, None, 2:]
        px, py, qx, qy = Pv[..., 0:1], Pv[..., 1:2], Qv[..., 0:1], Qv[..., 1:2]
        re = (dq[..., 0] * px - dq[..., 1] * py) - (qx * dp[..., 0] - qy * dp[..., 1])
        im = (dq[..., 0] * py + dq[..., 1] * px) - (qx * dp[..., 1] + qy * dp[..., 0])
        counts = (re * re + im * im <= T2 * PP[..., None]).sum(2)
        counts = torch.where((PP > 0) & (QQ > 0), counts, torch.full_like(counts, -1))
        index = (1 << 20) - 1 - (at + torch.arange(A.shape[1], device="cuda"))       # the first hypothesis wins a tie
        best = torch.maximum(best, (counts * (1 << 20) + index).max(1).values)
    h_ = (1 << 20) - 1 - best % (1 << 20)
    return best >> 20, ia[h_], ib[h_]


res = {"streams": N, "reps": args.reps, "points": points, "tolerance": TOLERANCE}
next_round()
c0 = {K: h.pull_corners(decs, max_points=K) for K in points}
assert h.keep_pictures(decs)[0] == [1] * N
next_round()
next_round()                                    # two pictures on: more than noise between them
rng = np.random.default_rng(3)
for K in points:
    c1 = h.pull_corners(decs, max_points=K)
    mout = torch.empty((N, h.matches_record_bytes(K)), dtype=torch.uint8, device="cuda")
    res[f"matches_k{K}_ms"] = timed(lambda st: h.pull_matches(decs, c0[K], c1, out=mout, stream=st), args.reps, args.warmup)
    m = h.pull_matches(decs, c0[K], c1, out=mout)
    mrec, krec, crec, P = populated(K, rng)
    out = torch.empty((N, h.model_record_bytes(K)), dtype=torch.uint8, device="cuda")
    for model in ("translation", "similarity"):
        call = lambda st, a=(mrec, krec, crec): h.pull_model(decs[:1], *a, model=model, tolerance=TOLERANCE, out=out, stream=st)
        res[f"model_{model}_k{K}_ms"] = timed(call, args.reps, args.warmup)
        g = h.pull_model(decs[:1], mrec, krec, crec, model=model, tolerance=TOLERANCE, out=out)
        torch.cuda.synchronize()
        assert bool((g.usable == K).all()) and bool((g.found == 1).all())
        res[f"inliers_{model}_k{K}"] = round(float(g.inliers.float().mean()), 2)
        mine = (g.inliers.long().clone(), g.a.long().clone(), g.b.long().clone())
        real = lambda st: h.pull_model(decs[:1], m, c0[K], c1, model=model, tolerance=TOLERANCE, out=out, stream=st)
        res[f"model_{model}_matched_k{K}_ms"] = timed(real, args.reps, args.warmup)
        res[f"usable_matched_k{K}"] = round(float(h.pull_model(decs[:1], m, c0[K], c1, model=model, tolerance=TOLERANCE).usable.float().mean()), 2)
        if args.kernel_only:
            continue
        chunk = max(1, (1 << 24) // (N * K))                                # 16 Mi elements a tensor
        theirs = torch_route(P, model, TOLERANCE, chunk)
        assert bool((theirs[0] == mine[0]).all()), (model, K, "inliers")
        if model == "similarity":
            assert bool((theirs[1] == mine[1]).all()) and bool((theirs[2] == mine[2]).all()), (model, K, "a, b")
        res[f"torch_{model}_k{K}_ms"] = timed(lambda st: torch_route(P, model, TOLERANCE, chunk), 3, 1)
res["device_errors"] = h.device_errors()
print(json.dumps(res))
