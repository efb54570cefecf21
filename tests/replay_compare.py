"""What the GPU tests on hand-built frame jobs share (test_gpu_random_jobs.py, test_gpu_structured_jobs.py): the bit-exact comparison
of a replayed sequence with the CPU oracle, the fixture that sets the row bands of the per-picture kernels and puts the default
back, and the recipe of the random sequences, which the CPU tests of tests/test_structured_jobs.py rebuild as well."""
import numpy as np
import pytest

from oracle import pyoracle
from jobgen import build_job


def run_and_compare(built, jobs, n_streams=2, stages=7):
    rep = built.Replay(jobs, n_streams=n_streams)
    rep.set_stages(stages)
    dpb = pyoracle.OracleDpb(jobs[0])
    try:
        for i, job in enumerate(jobs):
            rep.run(i, 1)
            want = dpb.decode(job, deblock=bool(stages & 4))
            cur = pyoracle.blob_header(job)["cur_slot"]
            for s in range(n_streams):
                got = rep.fetch(s, cur)
                if not np.array_equal(got, want):
                    d = np.nonzero(got != want)[0]
                    h = pyoracle.blob_header(job)
                    W = h["width_mbs"] * 16
                    i0 = int(d[0])
                    where = f"luma x={i0 % W} y={i0 // W}" if i0 < W * h["height_mbs"] * 16 else f"chroma byte {i0 - W * h['height_mbs'] * 16}"
                    pytest.fail(f"picture {i} stream {s}: {d.size} bytes differ, first at {where}: got {got[i0]} want {want[i0]}")
    finally:
        rep.close()


RANDOM_PIPELINE = [(1, 6, 5), (2, 11, 7), (3, 1, 1), (4, 1, 9), (5, 9, 1), (6, 20, 12), (7, 5, 4)]      # (seed, wmb, hmb)


def random_pipeline_jobs(lib, seed, wmb, hmb):
    """the five pictures of test_random_pictures_full_pipeline"""
    rng = np.random.default_rng(seed)
    jobs = [build_job(lib, rng, wmb, hmb, 0, 4, [])]                       # intra / PCM only
    jobs.append(build_job(lib, rng, wmb, hmb, 1, 4, [0]))
    jobs.append(build_job(lib, rng, wmb, hmb, 2, 4, [0, 1]))
    jobs.append(build_job(lib, rng, wmb, hmb, 3, 4, [0, 1, 2], p_inter=0.9))
    jobs.append(build_job(lib, rng, wmb, hmb, 0, 4, [1, 2, 3], p_inter=0.97, mv_range=64))
    return jobs


# ---- row bands of the two per-picture kernels (k_frame_dbk / k_frame_intra, kernels.hip.h): a picture split over several
# workgroups with the hand-over through HBM must give the same samples as one workgroup ----
DEFAULT_TAIL = (17, 9, 8, 0, 9, 12, 320)       # TailConfig (csrc/tick_plan.h)


@pytest.fixture
def tail(built):
    def set_(*cfg):
        built.set_tail(*cfg)
    yield set_
    built.set_tail(*DEFAULT_TAIL)
