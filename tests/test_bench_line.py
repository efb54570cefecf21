"""bench.py's plain line and --dump-outputs: the timed steps are the ones asked for, the line carries the headline only, and
the dumped arrays are the reference's pictures (the frame buffers as the last timed step left them)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


@pytest.mark.gpu
def test_gpu_bench_plain_line_and_dump(built, golden, tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--streams", "8", "--steps", "3", "--warmup", "1",
                          "--ramp-seconds", "0", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["higher_is_better"] is True and res["dtype"] == "u8"
    assert abs(res["value"] - 8 * 73 * 8160 * 1000 / res["ms_per_step"]) < 1e-6 * res["value"]
    for key in ("roofline", "staggered", "argb", "desynchronised", "end_to_end", "cpu_baseline", "lock_step_4_stream_groups"):
        assert key not in res, key                                       # behind --full
    g = golden["test_1920x1080"]
    pics = np.load(tmp_path / "last_pictures.npy")
    streams = np.load(tmp_path / "last_pictures_streams.npy")
    sums = np.load(tmp_path / "slot_checksums.npy")
    assert pics.dtype == np.float32 and streams.dtype == np.float64 and sums.dtype == np.float64
    assert pics.shape == (3, 8160 * 384) and sums.shape[1:] == (8, 2)
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64 << 20
    assert len(set(streams.tolist())) == 3 and all(0 <= s < 8 for s in streams)
    for p in pics:
        assert hashlib.sha256(p.astype(np.uint8).tobytes()).hexdigest() == g["frame_sha256"][-1]
    got = sums[..., 0].astype(np.uint64) | (sums[..., 1].astype(np.uint64) << np.uint64(32))
    assert (got[:, 0] == got[:, 1:].T).all()                               # every stream holds the same pictures
    assert int(np.uint64(g["frame_checksum64"][-1])) in got[:, 0].tolist()
