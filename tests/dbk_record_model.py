"""What k_dbk has to leave in the deblocking scratch for one frame job (test infrastructure of tests/test_gpu_dbk_records.py): the
48-byte record and the flag byte of every macroblock, from the CPU oracle's boundary strengths and a numpy model of the threshold
values.  The record layout is the one of h264bsd_amd/csrc/kernels/common.hip.h (DBK_REC_BYTES, DBKF_*):

  bytes 0..15   strength nibbles: byte 8 * dir + 2 * e + kh holds segment 2 * kh (low) and 2 * kh + 1 (high) of edge e
  bytes 16..39  six dwords {alpha, beta, tc0 for bS 1, tc0 for bS 2}: classes luma left / top / inner, chroma left / top / inner
  bytes 40..45  tc0 for bS 3 of the six classes
  byte 46       FJ_DBK_* flags, LEFT / TOP only where that neighbour exists;  byte 47: 1 where any strength is non-zero
  flag byte     DBKF_ANY | DBKF_LEFT | DBKF_TOP | DBKF_INNER, from the nibbles

Conventions the oracle does not share are the kernel's (its comments say so): a macroblock edge has strengths only where the
record's FJ_DBK_LEFT / FJ_DBK_TOP is set AND the neighbour exists; a macroblock is filtered where its dbk byte is non-zero and it
is not FJ_MB_ABSENT; the thresholds of an edge whose neighbour does not exist are computed with the macroblock's own QP.  (The
kernel gives the inner edges of a filtered macroblock their strengths whether FJ_DBK_INNER is set or not, the oracle only where it
is set: tests/jobgen.py sets it wherever it sets anything, expected() refuses a job that does not.)"""
import struct

import numpy as np

import h264bsd_amd
from oracle import pyoracle

DBKF_ANY, DBKF_LEFT, DBKF_TOP, DBKF_INNER = 1, 2, 4, 8
FJ_DBK_LEFT, FJ_DBK_TOP, FJ_DBK_INNER = 1, 2, 4
FJ_MB_ABSENT = 255

# Tables 8-16 (alpha', beta') and 8-17 (tC0' for bS 1, 2, 3) of the standard, by indexA / indexB
ALPHA = np.array([0] * 16 + [4, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 17, 20, 22, 25, 28, 32, 36, 40, 45, 50, 56, 63, 71, 80, 90, 101, 113, 127, 144,
                             162, 182, 203, 226, 255, 255])
BETA = np.array([0] * 16 + [2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15, 16, 16, 17, 17,
                            18, 18])
TC0 = np.array([[0, 0, 0]] * 17 + [[0, 0, 1]] * 4 + [[0, 1, 1]] * 2 + [[1, 1, 1]] * 4 + [[1, 1, 2]] * 4 + [[1, 2, 3]] * 2 + [[2, 2, 3], [2, 2, 4],
               [2, 3, 4], [2, 3, 4], [3, 3, 5], [3, 4, 6], [3, 4, 6], [4, 5, 7], [4, 5, 8], [4, 6, 9], [5, 7, 10], [6, 8, 11], [6, 8, 13], [7, 10, 14],
               [8, 11, 16], [9, 12, 18], [10, 13, 20], [11, 15, 23], [13, 17, 25]])
QPC = np.array(list(range(30)) + [29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39])
assert len(ALPHA) == len(BETA) == len(TC0) == len(QPC) == 52


def expected(job):
    """dict of arrays over the macroblocks of a finished frame job: listed, filtered (bool), rec [n, 48] (bytes 0..47 as k_dbk writes them
    for a listed, filtered macroblock), flag [n] (the flag byte of every macroblock; 0 off the list and where nothing is filtered)"""
    h = h264bsd_amd.job_header(job)
    n, w = h["n_mbs"], h["width_mbs"]
    recs = np.frombuffer(job, dtype=np.uint8, count=n * 32, offset=h["rec_off"]).reshape(n, 32)
    kind, dbk = recs[:, 0], recs[:, 5].astype(int)
    qp = recs[:, 1].astype(int)
    a_off, b_off, cqp = recs[:, 6].view(np.int8).astype(int), recs[:, 7].view(np.int8).astype(int), recs[:, 20].view(np.int8).astype(int)
    listed = np.zeros(n, dtype=bool)
    listed[[struct.unpack_from("<H", job, h["dbk_off"] + 2 * i)[0] for i in range(h["n_dbk"])]] = True
    filtered = (dbk != 0) & (kind != FJ_MB_ABSENT)
    assert ((dbk & FJ_DBK_INNER) != 0)[filtered].all(), "a filtered macroblock without FJ_DBK_INNER: kernel and oracle differ there (module docstring)"
    mb = np.arange(n)
    has_left, has_top = mb % w != 0, mb >= w
    f_left, f_top = ((dbk & FJ_DBK_LEFT) != 0) & has_left, ((dbk & FJ_DBK_TOP) != 0) & has_top
    bs = pyoracle.strengths(job).astype(np.uint8).copy()             # [n][dir][e][k]
    bs[~f_left, 0, 0, :] = 0
    bs[~f_top, 1, 0, :] = 0
    bs[~filtered] = 0
    rec = np.zeros((n, 48), dtype=np.uint8)
    flat = bs.reshape(n, 32)
    rec[:, 0:16] = flat[:, 0::2] | (flat[:, 1::2] << 4)
    left, top = rec[:, 0:2].any(axis=1), rec[:, 8:10].any(axis=1)
    inner = rec[:, 2:8].any(axis=1) | rec[:, 10:16].any(axis=1)
    any_ = left | top | inner
    flag = (any_ * DBKF_ANY + left * DBKF_LEFT + top * DBKF_TOP + inner * DBKF_INNER).astype(np.uint8)
    flag[~(listed & filtered)] = 0
    # thresholds: qPav of the two sides (chroma: QPc of both with the CURRENT macroblock's offset), the current macroblock's filter offsets
    other = [np.where(has_left, qp[np.maximum(mb - 1, 0)], qp), np.where(has_top, qp[np.maximum(mb - w, 0)], qp), qp]
    for c in range(6):
        a, b = qp, other[c % 3]
        if c >= 3:
            a, b = QPC[np.clip(a + cqp, 0, 51)], QPC[np.clip(b + cqp, 0, 51)]
        qpav = (a + b + 1) >> 1
        ia, ib = np.clip(qpav + a_off, 0, 51), np.clip(qpav + b_off, 0, 51)
        rec[:, 16 + 4 * c] = ALPHA[ia]
        rec[:, 17 + 4 * c] = BETA[ib]
        rec[:, 18 + 4 * c] = TC0[ia, 0]
        rec[:, 19 + 4 * c] = TC0[ia, 1]
        rec[:, 40 + c] = TC0[ia, 2]
    rec[:, 46] = f_left * FJ_DBK_LEFT + f_top * FJ_DBK_TOP + (dbk & FJ_DBK_INNER)
    rec[:, 47] = any_
    rec[~filtered, 46:48] = 0
    return dict(listed=listed, filtered=filtered, rec=rec, flag=flag)


def compare(exp, got_rec, got_flag):
    """None, or what differs first: listed filtered macroblocks byte for byte, listed unfiltered ones in bytes 46..47 and the flag byte,
    the others in the flag byte"""
    n = exp["flag"].shape[0]
    if not np.array_equal(got_flag, exp["flag"]):
        a = int(np.nonzero(got_flag != exp["flag"])[0][0])
        return f"flag byte of macroblock {a}: got {int(got_flag[a])} want {int(exp['flag'][a])} (listed {bool(exp['listed'][a])}, filtered {bool(exp['filtered'][a])})"
    for a in range(n):
        if not exp["listed"][a]:
            continue
        lo = 0 if exp["filtered"][a] else 46
        if not np.array_equal(got_rec[a, lo:], exp["rec"][a, lo:]):
            i = lo + int(np.nonzero(got_rec[a, lo:] != exp["rec"][a, lo:])[0][0])
            return f"macroblock {a} byte {i}: got {int(got_rec[a, i])} want {int(exp['rec'][a, i])}; record {got_rec[a].tolist()} want {exp['rec'][a].tolist()}"
    return None
