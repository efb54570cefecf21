"""Robustness of the host parser: arbitrarily damaged streams must end in error codes and concealed pictures, never
in a crash or a hang.  Runs in a child process so that a memory fault shows up as a failed test instead of killing
pytest.  (tests/fuzz_asan/ is the same idea under ASan/UBSan, with every frame job also rendered by the oracle.)"""
import subprocess

import pytest
import sys
import textwrap

from conftest import ROOT

CHILD = textwrap.dedent("""
    import ctypes, sys
    sys.path.insert(0, %r)
    import numpy as np
    import h264bsd_amd
    data = np.frombuffer(open(%r + "/tests/golden/test_640x360.h264", "rb").read(), dtype=np.uint8)
    rng = np.random.default_rng(int(sys.argv[1]))
    n_cases, pics, errors = 0, 0, 0
    for case in range(int(sys.argv[2])):
        d = data.copy()
        kind = case %% 4
        if kind == 0:                                   # random byte flips
            idx = rng.integers(0, d.size, rng.integers(1, 40)); d[idx] = rng.integers(0, 256, idx.size)
        elif kind == 1:                                 # truncation
            d = d[: int(rng.integers(10, d.size))]
        elif kind == 2:                                 # a burst of garbage
            s = int(rng.integers(0, d.size - 600)); d[s:s + 500] = rng.integers(0, 256, 500)
        else:                                           # bit flips inside the first slices
            idx = rng.integers(30, 4000, 8); d[idx] ^= (1 << rng.integers(0, 8, idx.size)).astype(np.uint8)
        jobs = []
        dec = h264bsd_amd.Decoder(capture=jobs.append)
        buf = ctypes.create_string_buffer(d.tobytes(), d.size)
        base, off, guard, stuck = ctypes.addressof(buf), 0, 0, 0
        while off < d.size and guard < 5000:
            guard += 1
            r, rb = dec.decode(base + off, d.size - off)
            assert 0 <= r <= 5 and rb <= d.size - off
            if r >= 3:
                errors += 1
            if rb == 0:
                stuck += 1
                if stuck > 3:
                    off += 1                          # a caller's resync step after repeated "call me again"
                    stuck = 0
            else:
                stuck = 0
            off += rb
        pics += len(jobs)
        dec.close()
        n_cases += 1
    print("OK", n_cases, pics, errors)
""") % (ROOT, ROOT)


def test_damaged_streams_never_crash(tmp_path, built):
    script = tmp_path / "fuzz_child.py"
    script.write_text(CHILD)
    for seed in (1, 2):
        out = subprocess.run([sys.executable, str(script), str(seed), "60"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, f"seed {seed}: rc={out.returncode}\n{out.stderr[-1500:]}"
        tag, n, pics, errors = out.stdout.split()[-4:]
        assert tag == "OK" and int(n) == 60 and int(errors) > 0


REPEAT_CHILD = textwrap.dedent("""
    import ctypes, sys
    sys.path.insert(0, %r)
    import h264bsd_amd
    data = open(%r + "/tests/golden/test_640x360.h264", "rb").read()
    starts = []
    i = data.find(b"\\x00\\x00\\x00\\x01")
    while i >= 0:
        starts.append(i)
        i = data.find(b"\\x00\\x00\\x00\\x01", i + 4)
    starts.append(len(data))
    worst = 0
    for k in range(len(starts) - 1):
        nal = data[starts[k]:starts[k + 1]]
        if nal[4] & 31 != 1 or k < 8:
            continue
        for frac in (0.25, 0.5, 0.75):
            cut = nal[: max(8, int(len(nal) * frac))]
            d = data[:starts[k]] + cut * 400 + data[starts[k + 1]:starts[k + 3]]
            jobs = []
            dec = h264bsd_amd.Decoder(capture=jobs.append)
            buf = ctypes.create_string_buffer(d, len(d))
            base, off, stuck, guard = ctypes.addressof(buf), 0, 0, 0
            while off < len(d) and guard < 5000:
                guard += 1
                r, rb = dec.decode(base + off, len(d) - off)
                stuck = stuck + 1 if rb == 0 else 0
                if stuck > 3:
                    off += 1; stuck = 0
                off += rb
            dec.close()
            for j in jobs:
                h = h264bsd_amd.job_header(j)
                assert h["n_coef_blocks"] <= 27 * h["n_mbs"] + 2 + 27, (k, frac, h["n_coef_blocks"])
                worst = max(worst, h["n_coef_blocks"])
        if k > 14:
            break
    print("OK", worst)
""") % (ROOT, ROOT)


def test_repeated_truncated_slices_stay_inside_the_coefficient_section(tmp_path, built):
    """A slice NAL unit cut short and repeated 400 times: its macroblocks are decoded, rolled back and decoded again.
    The coefficient blocks of rolled-back macroblocks are reclaimed (hd_core.c mark_slice_corrupted, hd_mb.c decode_mb)
    and the section is bounds-checked (next_block) — round 1 overran the pinned staging buffer here."""
    script = tmp_path / "repeat_child.py"
    script.write_text(REPEAT_CHILD)
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.split()[-2] == "OK", out.stderr[-1500:]


def test_sanitizer_harness_builds_and_runs(tmp_path):
    """tests/fuzz_asan/run.sh compiles the host parser + oracle with AddressSanitizer and UBSan and feeds them mutated
    streams; the harness had silently stopped linking once (a new engine entry point without a stub), so a short run is
    part of the suite: it must build, finish, and report no sanitizer finding."""
    import os
    import shutil
    import subprocess
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TMPDIR=str(tmp_path))
    r = subprocess.run(["bash", os.path.join(root, "tests", "fuzz_asan", "run.sh"),
                        os.path.join(root, "tests", "golden", "test_640x360.h264"), "40", "3"],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    assert "cases 40" in r.stdout and "ERROR: AddressSanitizer" not in r.stdout and "runtime error" not in r.stdout.replace("left shift of negative", "")
    # the bundled streams have one slice per picture: redundant slices, slice groups and several slices per picture come
    # from the bitstream writer (this stream + seed once read coefficient blocks past the end of a job: a record that
    # survived its slice's roll-back had lost them to the reclaim in mark_slice_corrupted)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from synth_configs import SWEEP_FINDS
    from h264writer import StreamWriter
    from damage import damage
    cfg, dmg = SWEEP_FINDS["redundant_flipped_106936"]
    stream = tmp_path / "redundant.h264"
    stream.write_bytes(damage(StreamWriter(**cfg).build(), **dmg))
    r = subprocess.run([os.path.join(str(tmp_path), "h264bsd_fuzz_asan"), str(stream), "150", "3"],
                       capture_output=True, text=True, timeout=900, env=dict(env, ASAN_OPTIONS="detect_leaks=0"))
    out = "\n".join(ln for ln in (r.stdout + r.stderr).splitlines() if "left shift of negative" not in ln)   # (mirrors the reference's arithmetic)
    assert "cases 150" in out and "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-1500:]


@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_batch_calls_under_sanitizers(tmp_path, sanitizer):
    """The threaded host paths — parser pool, h264bsdmiDecodePictureBatch, h264bsdmiNextOutputPictureBatch and
    h264bsdmiPullAndDecodePictureBatch with its look-ahead pulls — under ThreadSanitizer and under Address/UB/LeakSanitizer, bound to a
    device stand-in (tests/fuzz_asan/mock_engine.c) whose pictures are the running number of the job decoded into a frame buffer: every
    pull must hand out the successor of the instance's previous picture, no report from the sanitizer."""
    import os
    import shutil
    import subprocess
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import host_program
    exe = host_program.build("batch_tsan", str(tmp_path), sanitizer)
    r = subprocess.run([exe, os.path.join(root, "tests", "golden", "test_640x360.h264"), "12", "6"], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", TSAN_OPTIONS="halt_on_error=0"))
    out = "\n".join(ln for ln in (r.stdout + r.stderr).splitlines() if "left shift of negative" not in ln)   # (mirrors the reference's arithmetic)
    if "FATAL: ThreadSanitizer" in out and "unexpected memory mapping" in out:
        pytest.skip("ThreadSanitizer cannot run in this container (address space layout)")
    assert r.returncode == 0 and "ok: 12 instances x 2 styles, 1752 pictures pulled" in out, out[-2000:]
    assert "WARNING: ThreadSanitizer" not in out and "ERROR: AddressSanitizer" not in out and "ERROR: LeakSanitizer" not in out and "runtime error" not in out, out[-2000:]
