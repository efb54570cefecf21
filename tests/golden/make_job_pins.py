#!/usr/bin/env python3
"""The pins of frame-job assembly (h264bsd_amd/csrc/hd_core.c: fj_finalize_ex and the code around it that makes the ghost, redo and
concealment jobs): the bytes of every finished job of every fixture stream, of a set of hand-built jobs, and the hand-made jobs
that must be refused.  tests/test_job_pins.py holds the tree to job_pins.json; this file is the generator and holds the one set
both use.

The pins never come from the code under test: the generator is given a checkout of the commit BEFORE the change under review, with
its library built, and imports h264bsd_amd from there (the streams and jobgen are this tree's):

    mkdir parent && git archive HEAD~ | tar -x -C parent && python3 -c "import sys; sys.path.insert(0, 'parent'); import h264bsd_amd; h264bsd_amd.build()"
    python3 tests/golden/make_job_pins.py parent "$(git rev-parse --short HEAD~)"

Streams: the three bundled ones, every synth_configs.CONFIGS stream, every test_damaged_streams.NAMES stream; each is captured
without and with copy elision, and pinned as [jobs of the first capture, SHA-256 over all jobs of the first then of the second].
Hand-built jobs (tests/jobgen.build_job through h264bsdmiJobFinalize: dense vectors in FRONT of the coefficients, which the parser
never produces) are pinned as the SHA-256 of the finished job up to total_bytes."""
import ctypes
import hashlib
import json
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PINS = os.path.join(HERE, "job_pins.json")
BUNDLED = ["test_640x360", "test_1920x1080", "test_1920x1080_fullRange"]

SIZES = [(1, 1), (2, 1), (1, 3), (3, 2), (5, 4), (11, 9)]
# (name, reference slots, arguments of build_job): intra only, the defaults, nearly all inter with short vectors (copy runs, uniform
# neighbours for the deblocking proof), nothing filtered, partitioned vectors far outside the picture
VARIANTS = [("intra", [], {}), ("mixed", [0], {}), ("inter", [0, 1, 2], dict(p_inter=0.97, mv_range=16)),
            ("nodbk", [0, 1], dict(any_deblock=False)), ("pcm", [1, 2], dict(p_inter=0.5, p_pcm=0.25))]
REJECTIONS = ["mv_off + 64 n > capacity", "dense vectors in front of the coefficients run into them", "coef_idx + blocks > n_coef_blocks",
              "capacity one byte short of total_bytes", "mv_off behind coef_off but inside the finished job"]


def streams():
    """[(name, bytes)]: bundled, synth_*, dmg_*"""
    sys.path[:0] = [p for p in (os.path.join(ROOT, "tests"),) if p not in sys.path]
    from h264writer import StreamWriter
    from synth_configs import CONFIGS
    import test_damaged_streams as dmg
    out = [(n, open(os.path.join(HERE, n + ".h264"), "rb").read()) for n in BUNDLED]
    out += [("synth_" + n, StreamWriter(**cfg).build()) for n, cfg in CONFIGS.items()]
    out += [("dmg_" + n, dmg.stream_of(n)) for n in dmg.NAMES]
    return out


def _count(stats, h264bsd_amd, full, lean):
    """what kinds of jobs the set holds (the test asserts lower bounds, so that the pin cannot silently stop covering a path)"""
    for jf, jl in zip(full, lean):
        h, hl = h264bsd_amd.job_header(jf), h264bsd_amd.job_header(jl)
        r = np.frombuffer(jf, np.uint8, h["n_mbs"] * 32, h["rec_off"]).reshape(-1, 32)
        kind, pred = r[:, 0], r[:, 4]
        n_ci = int((kind == 4).sum())
        for key, hit in (("jobs", True), ("ghost", h["ghost"]), ("dbk_only", h["dbk_only"]), ("conceal_i", n_ci), ("conceal_i_dbk_only", n_ci and h["dbk_only"]),
                         ("conceal_p", (kind == 5).any()), ("phase2", (pred & 0x80).any()), ("ipcm", (kind == 3).any()), ("stale", (kind == 6).any()),
                         ("mvx", h["n_mvx"]), ("quad", h["n_gen_quad"])):
            stats[key] = stats.get(key, 0) + bool(hit)
        stats["max_conceal_i"] = max(stats.get("max_conceal_i", 0), n_ci)
        stats["elided"] = stats.get("elided", 0) + h["n_copy_mbs"] - hl["n_copy_mbs"]


def stream_pins(h264bsd_amd, named):
    """({name: [jobs, sha256]}, stats over all streams, stats over the bundled and damaged streams alone)"""
    pins, stats, stats_bd = {}, {}, {}
    for name, data in named:
        full = h264bsd_amd.capture_stream(data)[0]
        lean = h264bsd_amd.capture_stream(data, copy_elision=True)[0]
        assert len(full) == len(lean)
        sha = hashlib.sha256()
        for j in full + lean:
            sha.update(bytes(j))
        pins[name] = [len(full), sha.hexdigest()]
        _count(stats, h264bsd_amd, full, lean)
        if not name.startswith("synth_"):
            _count(stats_bd, h264bsd_amd, full, lean)
    return pins, stats, stats_bd


class _Tap:
    """stands in for the library in build_job: keeps the job as it was handed to h264bsdmiJobFinalize"""

    def __init__(self, lib):
        self.lib = lib

    def h264bsdmiJobFinalize(self, ptr, cap, nblk):
        self.raw, self.cap, self.nblk = ctypes.string_at(ptr.value, cap), cap, nblk
        return self.lib.h264bsdmiJobFinalize(ptr, cap, nblk)


def _build_job(lib, k, size, variant):
    sys.path[:0] = [p for p in (os.path.join(ROOT, "tests"),) if p not in sys.path]
    from jobgen import build_job
    _, refs, kw = variant
    return build_job(lib, np.random.default_rng(9000 + k), size[0], size[1], 3, 4, refs, **kw)


def _copy_runs(w, h):
    """patch of build_job: whole-sample one-vector macroblocks without coefficients on both sides of a row end — a displaced pair (a
    copy run must not cross the row end) and ten with zero motion (it may, and splits at FJ_COPY_RUN); random jobs hardly ever hold either"""
    def patch(recs, mvs):
        for addrs, mv, slot in ((range(w - 1, w + 1), (8, -16), 1), (range(2 * w - 1, min(w * h, 2 * w + 9)), (0, 0), 2)):
            for a in addrs:
                recs[a, 0], recs[a, 4], recs[a, 8:12], recs[a, 16:20], mvs[a] = 0, 0, 0, slot, mv
    return patch


def hand_built(lib):
    """{name: sha256 of the finished job}: every size x every variant, and the copy runs at the sizes with two rows and columns; seeds fixed"""
    todo = [(s, v) for s in SIZES for v in VARIANTS]
    todo += [(s, ("runs", [0, 1, 2], dict(p_inter=0.9, patch=_copy_runs(*s)))) for s in SIZES if min(s) >= 2]
    return {f"{size[0]}x{size[1]}_{variant[0]}": hashlib.sha256(_build_job(lib, k, size, variant)).hexdigest() for k, (size, variant) in enumerate(todo)}


def rejections(lib):
    """[(what, return code, return code of the nearest edit that must be accepted)] of REJECTIONS: a valid 5x4 job as build_job hands
    it over (vectors | coefficients, a generous capacity), one field edited each, so that each reaches the check its name says and
    no earlier one; the unedited job first, which must be accepted"""
    tap = _Tap(lib)
    good = _build_job(tap, 100, (5, 4), VARIANTS[1])
    n, mv_off, coef_off = struct.unpack_from("<I", tap.raw, 12)[0], struct.unpack_from("<I", tap.raw, 24)[0], struct.unpack_from("<I", tap.raw, 36)[0]
    total = len(good)
    recs = np.frombuffer(tap.raw, np.uint8, n * 32, 128).reshape(n, 32)
    coded = np.frombuffer(recs[:, 8:12].tobytes(), np.uint32)
    owner = int(np.flatnonzero((coded & 0x03FFFFFF) != 0)[-1])              # a macroblock that owns coefficient blocks

    def run(edit=None, cap=tap.cap):
        buf = ctypes.create_string_buffer(tap.raw, tap.cap)
        if edit:
            struct.pack_into("<I", buf, *edit)
        rc = lib.h264bsdmiJobFinalize(ctypes.cast(buf, ctypes.c_void_p), cap, tap.nblk)
        return rc, bytes(buf[:total])

    rc, again = run()
    assert rc == 0 and again == good
    lvl_off = (coef_off + tap.nblk * 32 + 31) & ~31
    assert mv_off < coef_off < lvl_off < total
    behind = (tap.cap - 64 * n) & ~31                  # dense vectors at the tail of the buffer, where the parser keeps them
    assert behind >= total
    edits = [  # (the edit, the capacity), the same for the accepted neighbour
        # the first check of fj_finalize_ex: the vectors end 32 bytes behind the buffer / end inside it
        (((24, tap.cap - 64 * n + 32), tap.cap), ((24, behind), tap.cap)),
        # its second check: the vectors start in front of coef_off and end 32 bytes inside the coefficients / the job as it is
        (((24, mv_off + 32), tap.cap), (None, tap.cap)),
        # fj_coefs_inside: the last macroblock with blocks starts at the end of the section / the job as it is
        (((128 + 32 * owner + 12, tap.nblk), tap.cap), (None, tap.cap)),
        # total_bytes > cap (the vectors lie in front: the first check passes) / a capacity of exactly total_bytes
        ((None, total - 1), (None, total)),
        # the last check: the vectors start at lvl_off, inside the finished job / right behind it
        (((24, lvl_off), tap.cap), ((24, total), tap.cap))]
    return [(what, run(*bad)[0], run(*ok)[0]) for what, (bad, ok) in zip(REJECTIONS, edits)]


def collect(h264bsd_amd, named=None):
    pins, stats, stats_bd = stream_pins(h264bsd_amd, streams() if named is None else named)
    return dict(streams=pins, stats=stats, stats_bundled_damaged=stats_bd, hand_built=hand_built(h264bsd_amd.lib()), rejections=rejections(h264bsd_amd.lib()))


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit("usage: make_job_pins.py <built checkout of the commit the pins are taken from> <its name>")
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import h264bsd_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(h264bsd_amd.__file__))) == os.path.abspath(sys.argv[1])
    got = collect(h264bsd_amd)
    assert all(rc == -1 and ok == 0 for _, rc, ok in got["rejections"]), got["rejections"]
    with open(PINS, "w") as f:
        json.dump({"recorded_from": sys.argv[2], "streams": got["streams"], "hand_built": got["hand_built"]}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{PINS}: {len(got['streams'])} streams and {len(got['hand_built'])} hand-built jobs from {sys.argv[2]}, {os.path.getsize(PINS)} bytes\n{got['stats']}",
          file=sys.stderr)
