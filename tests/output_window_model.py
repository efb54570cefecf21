"""Device-resident output and narrow-picture conversion (test infrastructure for tests/test_gpu_output_windows.py): the cases, the
expected bytes and a classifier of which code a case reaches.

want() slices the chosen pictures themselves (tests/pcm_pictures.py: an all-I_PCM stream carries them verbatim) and, for the converted
formats, pp.formula_convert — the reference's formula in numpy.  Nothing here comes from a kernel or from the decoder under test.

reach() mirrors, by hand, the branch conditions of k_output (kernels/k_pixels_io.hip.h) and the grid sink_fetch_device (engine.hip)
launches it on; pairs() mirrors conv_pic (kernels/convert.hip.h).  tests/test_gpu_output_windows.py asserts on the CPU that the cases
reach what they were chosen for, and that the two source lines mirrored here still read as they did."""
import collections

import numpy as np

import pcm_pictures as pp

Case = collections.namedtuple("Case", "wmb hmb crop window uncropped")

# (wmb, hmb), frame_crop offsets (left, right, top, bottom) in chroma samples or None, the window (x0, y0, w, h) in luma samples;
# uncropped: the case is also pulled with crop=False (the window is then the coded frame)
CASES = [
    Case(1, 1, (0, 7, 0, 7), (0, 0, 2, 2), False),          # smallest window: one chroma sample per plane; sample path
    Case(1, 1, (7, 0, 7, 0), (14, 14, 2, 2), False),        # last corner of a tile
    Case(1, 1, (3, 4, 0, 0), (6, 0, 2, 16), False),         # two columns
    Case(1, 1, (0, 6, 0, 0), (0, 0, 4, 16), False),         # quad path, one quad per row
    Case(1, 1, (1, 1, 1, 1), (2, 2, 12, 12), False),        # quad path, x0 = 2 (mod 4)
    Case(2, 1, (1, 0, 0, 0), (2, 0, 30, 16), False),        # sample path across a tile seam
    Case(2, 1, (0, 1, 0, 3), (0, 0, 30, 10), False),        # sample path, x0 = 0
    Case(2, 2, (7, 7, 7, 7), (14, 14, 4, 4), True),         # one quad over four luma tiles; chroma pair over the seam
    Case(3, 2, (1, 1, 0, 0), (2, 0, 44, 32), False),        # quads straddling luma seams; chroma pairs straddling
    Case(3, 2, (2, 0, 1, 0), (4, 2, 44, 30), False),        # aligned quads, y0 != 0, h not a multiple of 16
    Case(9, 5, (1, 2, 1, 3), (2, 2, 138, 72), True),        # sample path, several trips
    Case(9, 5, (1, 1, 0, 0), (2, 0, 140, 80), False),       # quads straddling, more than one workgroup
    Case(9, 5, (3, 0, 0, 0), (6, 0, 138, 80), False),       # sample path, x0 = 2 (mod 4)
    Case(3, 1, (0, 0, 0, 0), (0, 0, 48, 16), True),         # cropping flag set, whole frame
    Case(3, 1, None, (0, 0, 48, 16), False),                # no cropping in the SPS
]
SMALL = CASES[10]                                           # the 9 x 5 stream the tensor-pull suites use
BIG = Case(120, 68, (1, 1, 0, 4), (2, 0, 1916, 1080), False)     # the I420 quad loop's second trip
NARROW = [(1, 1), (2, 1), (1, 3), (2, 9), (1, 17), (3, 2), (4, 3)]      # (wmb, hmb) of the conversion cases

CONV_BATCH = 8                                              # CONV_BATCH_N, kernels/convert.hip.h
K_OUTPUT_BRANCH = "if (w & 3u) {"                           # k_output, kernels/k_pixels_io.hip.h
K_OUTPUT_GRID = "dim3((n + 255) / 256 < 2048 ? (n + 255) / 256 + 1 : 2048)"          # sink_fetch_device, engine.hip
K_OUTPUT_ITEMS = "const uint32_t n = fmt == 3 ? w * h * 3 / 8 : w * h / 4;"


def case_id(c):
    return f"{c.wmb}x{c.hmb}-" + ("none" if c.crop is None else ".".join(str(v) for v in c.crop))


def coded_window(c):
    return (0, 0, 16 * c.wmb, 16 * c.hmb)


def pictures(c, n, tag=0):
    """n pictures of case c, uniformly random over 0..255 in all three planes; one fixed seed per (case, tag, picture index)"""
    W, H = 16 * c.wmb, 16 * c.hmb
    out = []
    for k in range(n):
        rng = np.random.default_rng([c.wmb, c.hmb, W * (c.window[1] + 1) + c.window[0], c.window[2], tag, k])
        out.append(tuple(rng.integers(0, 256, shape, dtype=np.uint8) for shape in ((H, W), (H // 2, W // 2), (H // 2, W // 2))))
    return out


def want(fmt, picture, window):
    """the bytes h264bsdmiNextOutputPictureDevice hands out for the window (x0, y0, w, h) of `picture`: fmt 3 a tight I420 picture
    (flat uint8), fmt 0..2 [h, w] uint32"""
    Y, Cb, Cr = picture
    x0, y0, w, h = window
    if fmt == 3:
        c = lambda p: p[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2].reshape(-1)
        return np.concatenate([Y[y0:y0 + h, x0:x0 + w].reshape(-1), c(Cb), c(Cr)])
    return np.ascontiguousarray(pp.formula_convert(fmt, picture)[y0:y0 + h, x0:x0 + w]).astype(np.uint32)


def where(fmt, window, i):
    """flat element i of want(fmt, ., window) as (plane, x, y) in window coordinates (chroma planes in chroma samples)"""
    _, _, w, h = window
    if fmt != 3:
        return ("pixel", i % w, i // w)
    if i < w * h:
        return ("Y", i % w, i // w)
    j, nc = i - w * h, (w // 2) * (h // 2)
    return ("Cr" if j >= nc else "Cb", (j % nc) % (w // 2), (j % nc) // (w // 2))


Reach = collections.namedtuple("Reach", "kernel path items grid trips luma_seam chroma_seam one_chroma_sample")


def reach(fmt, window, coded):
    """what the pull of `window` of a coded frame of `coded` = (W, H) samples runs.  kernel: k_detile or k_output; path: one of
    sample_i420, sample_conv, quad_i420, quad_conv; items: loop items of the path; grid: workgroups of 256 lanes; trips: the most
    trips a lane makes; luma_seam: a lane's four luma samples lie in two tiles; chroma_seam: a lane's two chroma samples do"""
    x0, y0, w, h = window
    if fmt == 3 and window == (0, 0) + tuple(coded):
        return Reach("k_detile", None, 0, 512, 0, False, False, False)
    n = w * h * 3 // 8 if fmt == 3 else w * h // 4
    grid = (n + 255) // 256 + 1 if (n + 255) // 256 < 2048 else 2048
    sample, qw = bool(w & 3), w >> 2
    if sample:
        items = w * h + 2 * (w >> 1) * (h >> 1) if fmt == 3 else w * h
    else:
        items = qw * h + 2 * ((w >> 1) >> 1) * (h >> 1) if fmt == 3 else qw * h
    starts = [x0 + 4 * q for q in range(qw)]
    luma_seam = not sample and any(x >> 4 != (x + 3) >> 4 for x in starts)
    if fmt == 3:                                            # the pair (x0 / 2 + 2 q, + 1) of a chroma row
        chroma_seam = not sample and any((x0 // 2 + 2 * q) >> 3 != (x0 // 2 + 2 * q + 1) >> 3 for q in range((w >> 1) >> 1))
    else:                                                   # the two chroma samples under a quad
        chroma_seam = not sample and any((x >> 1) >> 3 != ((x + 3) >> 1) >> 3 for x in starts)
    return Reach("k_output", ("sample" if sample else "quad") + ("_i420" if fmt == 3 else "_conv"), items, grid, -(-items // (grid * 256)),
                 luma_seam, chroma_seam, fmt == 3 and (w >> 1) * (h >> 1) == 1)


def pairs(wmb, hmb):
    """(ppr, magic, tile pairs) of conv_pic for a picture of wmb x hmb macroblocks"""
    ppr = (wmb + 1) >> 1
    return ppr, 0 if ppr == 1 else 0xFFFFFFFF // ppr + 1, ppr * hmb
