"""GPU: exact ties through the resampling tensor pulls.  The reference colour rounds halves UP and the matrix colours round halves
to EVEN (include/h264bsd_mi355x.h), and the two differ only on a tie — which the band rule of tests/rounding_model.py never decides.
So here the input is chosen such that fp32 is exact and the outputs ARE ties, and equality is asserted on every one of them.

The picture (tie_picture): 64 x 48, all I_PCM, chroma 128; luma v where x % 4 is 0 or 1 and v + 2 where it is 2 or 3, v constant in
bands of 8 rows (BANDS: v = 0, v + 2 = 255, even and odd v).

- bilinear_aa, 2 : 1 down along x: the taps of an inner output column are 4 source columns weighted 1/8, 3/8, 3/8, 1/8 (triangle
  values 1/4, 3/4, 3/4, 1/4, sum 2.0, norm 0.5), so the value is v + 0.5 or v + 1.5.  At scale 1 along y the taps are 1 and 0.
- bilinear without antialiasing, 2 : 1 up along x: the weights are 1/4 and 3/4: a + (b - a) / 4, a tie where b - a = 2.
- remap, bilinear: the sample position x + 1/4 (even rows) or x + 3/4 (odd rows) gives the same blend.  (x + 1/2 would give
  (a + b) / 2, which this picture never makes a tie in luma: neighbouring columns differ by 0 or 2.)
Every weight is a multiple of 1/8 and every operand an 8-bit integer, so the kernels' fp32 sums and the model's float64 sums are
the same exact numbers.  The first and last output columns and rows of an antialiased axis have fewer taps, weights over 1.75: fp32
is not exact there (over a flat band float64 happens to give k + 0.5 where fp32 gives k + 0.50000003), so outputs whose weights
are not all multiples of 1/8 are left out (_exact); the letterboxed rows that mix two bands are whatever the model says.  Which
outputs are ties is read off the MODEL (x * 8 % 8 == 4, asserted to be at least a quarter of the outputs), so a change to the
picture cannot turn a test into a no-op.

Expected: reference colour floor(x + 0.5) on every channel (its R, G, B of a grey triple are integers, so the operands stay 8-bit;
where R(v + 2) - R(v) is 3 or 0 the RGB outputs are no ties, the Y outputs are).  Matrix colour: channel Y of BT.709 FULL range,
where colour_item (engine.hip) folds k0 = (float)(1 * (1.0 / 255) * 255.0) = 1.0f exactly and k3 = (float)(0.0 * 255 + 0.0) = 0, so
the value under the uint8 scale is Y itself: np.rint(x), 0.5 -> 0, 1.5 -> 2, 254.5 -> 254.

bicubic_aa is left out here, and only here: its normalisation 1 / sum of the Keys weights is no power of two, so fp32 is not exact
and no output is a guaranteed tie."""
import numpy as np
import pytest

import colour_model as cm
import pcm_pictures as pp
import region_model as gm
import remap_model as mm
import resize_model as rm
import test_gpu_tensor_resize as tr
from test_gpu_tensor_colour import Feed

pytestmark = pytest.mark.gpu

W, H = 64, 48
BANDS = (0, 253, 100, 101, 38, 89)         # (the last four: R(v + 2) - R(v) = 2 in the reference colour)
GEO = (W, H, 0, 0, W, H)
# (colour, channels, layout): the reference colour on luma and on R, G, B; a matrix colour on luma
KINDS = [("reference", "Y", "NCHW"), ("reference", "RGB", "NHWC"), ("bt709", "Y", "NHWC")]


@pytest.fixture(autouse=True, scope="module")
def _through_the_product_library(built):
    built.use_product_library(True)
    yield
    built.use_product_library(False)


@pytest.fixture(autouse=True)
def _no_device_errors(built):
    yield
    assert built.device_errors() == 0


def tie_picture():
    x, y = np.arange(W)[None, :], np.arange(H)[:, None]
    luma = np.asarray(BANDS)[y // 8] + np.where(x % 4 < 2, 0, 2)
    assert luma.min() == 0 and luma.max() == 255 and {v & 1 for v in BANDS} == {0, 1}
    return luma.astype(np.uint8), np.full((H // 2, W // 2), 128, np.uint8), np.full((H // 2, W // 2), 128, np.uint8)


def _feed(built, n_pics):
    return Feed(built, pp.pcm_stream([tie_picture()] * n_pics))


def _source(colour, ch):
    """[48, 64, C] float64 on the 0 .. 255 scale: the oracle's 8-bit values (REF), or the luma samples themselves (BT.709 full range,
    channel Y: the colour model's 255 v, asserted)"""
    frame = pp.i420(tie_picture())
    if colour == "reference":
        return tr._source(frame, GEO, colour, ch)
    assert ch == "Y"
    luma = np.asarray(tie_picture()[0], np.float64)[:, :, None]
    assert (np.round(255 * cm.colour_hwc(frame, GEO, "bt709", True, "bilinear", "Y"), 9) == luma).all()
    return luma


def _col(colour):
    return {} if colour == "reference" else dict(colour="bt709", colour_range="full", chroma="bilinear")


def _exact(n_in, n_out, filt, fma=False):
    """per output index: every weight of the model is a multiple of 1/8, so the kernel's fp32 weights and sums are exact"""
    return ((rm.weights(n_in, n_out, filt, fma) * 8) % 1 == 0).all(axis=1)


def _assert_ties(got, x, colour, what, exact=None):
    """got: [h, w, C] float64 of the uint8 tensor, x: the model on the 0 .. 255 scale, exact: [h, w] bool, where fp32 is exact
    (default: everywhere).  Every exact tie of the model equals floor(x + 0.5) (REF) or np.rint(x) (halves to even); there are
    enough of them, going both ways for the matrix colour"""
    assert got.shape == x.shape, what
    assert x.min() >= 0 and x.max() <= 255
    ties = (x * 8) % 8 == 4                             # float64, exact: x is a sum of 8-bit integers weighted by multiples of 1/8
    if exact is not None:
        ties &= exact[:, :, None]
    assert ((x[ties] * 2) % 2 == 1).all()
    want = np.floor(x + 0.5) if colour == "reference" else np.rint(x)
    print(f"{what}: ties {ties.mean():.3f} of {ties.size}, ties that differ {int((got != want)[ties].sum())}")
    assert ties.mean() >= 0.25, (what, ties.mean())
    if colour != "reference":                           # halves to even go down as often as up: both are present
        down, up = want[ties] < x[ties], want[ties] > x[ties]
        assert down.mean() >= 0.25 and up.mean() >= 0.25, (what, down.mean(), up.mean())
    assert (got[ties] == want[ties]).all(), (what, int((got != want)[ties].sum()), x[ties & (got != want)][:6], got[ties & (got != want)][:6])
    assert np.abs(got - want).max() <= 1, what


def _torch_u8():
    import torch
    return torch.uint8


@pytest.mark.parametrize("colour,ch,lay", KINDS)
@pytest.mark.parametrize("fit,size", [("stretch", (48, 32)), ("letterbox", (32, 32))])
def test_bilinear_aa_two_to_one_down(built, fit, size, colour, ch, lay):
    """k_tensor_aa: 64 x 48 to 32 x 48 stretched (the y taps are the identity) and letterboxed into 32 x 32 (inner 32 x 24: the
    rows that stay inside a band of 8 are ties)"""
    feed = _feed(built, 1)
    assert feed.step()
    t, got, _, _, _, boxes = built.pull_tensor([feed.dec], size=size, layout=lay, dtype=_torch_u8(), channels=ch, mode="bilinear",
                                               antialias=True, fit=fit, pad=(0.25, 0.5, 1.0), return_boxes=True, **_col(colour))
    left, top, iw, ih = rm.letterbox(size[1], size[0], W, H) if fit == "letterbox" else (0, 0, size[1], size[0])
    assert got == [1] and boxes == [(left, top, iw, ih)] and (iw, ih) == ((32, 24) if fit == "letterbox" else (32, 48))
    x = rm.resample_hwc(_source(colour, ch), (ih, iw), "bilinear_aa")
    if fit == "stretch" and ch == "Y":                  # every inner column of every row: v + 0.5 or v + 1.5
        assert ((x[:, 1:-1, 0] - np.asarray(BANDS, np.float64)[np.arange(H) // 8][:, None]) % 1 == 0.5).all()
    exact = _exact(H, ih, "bilinear_aa")[:, None] & _exact(W, iw, "bilinear_aa")[None, :]
    assert exact[1:-1, 1:-1].all() and not exact[:, 0].any()
    _assert_ties(tr._hwc(t[0], lay)[top:top + ih, left:left + iw], x, colour, ("aa", fit, colour, ch), exact)
    feed.close()


@pytest.mark.parametrize("colour,ch,lay", KINDS)
def test_bilinear_aa_regions(built, colour, ch, lay):
    """k_tensor_roi: one box that covers the window (into 32 x 48) and an interior box on a multiple of 4 (40 x 32 at (8, 8), into
    20 x 32), both 2 : 1 along x only"""
    feed = _feed(built, 1)
    assert feed.step() and feed.dec.next_output_info() is not None
    v = _source(colour, ch)
    for box, size in (((0, 0, 64, 48), (48, 32)), ((8, 8, 40, 32), (32, 20))):
        t, got, rects, _, _ = built.pull_regions([feed.dec], [(0,) + box], size, layout=lay, dtype=_torch_u8(), channels=ch, mode="bilinear",
                                                 antialias=True, fit="stretch", **_col(colour))
        assert got == [1] and rects == [(0, 0, size[1], size[0])]
        rect, x = gm.region(v, box, size, "bilinear_aa", "stretch", gm.sample_pad((0, 0, 0), colour == "reference"))
        exact = _exact(box[3], size[0], "bilinear_aa")[:, None] & _exact(box[2], size[1], "bilinear_aa")[None, :]
        _assert_ties(tr._hwc(t[0], lay), x, colour, ("roi", box, colour, ch), exact)
    feed.close()


@pytest.mark.parametrize("colour,ch,lay", KINDS)
@pytest.mark.parametrize("fit,size", [("stretch", (48, 128)), ("letterbox", (112, 128))])
def test_bilinear_two_to_one_up(built, fit, size, colour, ch, lay):
    """bilinear without antialiasing: k_tensor_resize (stretch, 64 x 48 to 128 x 48) and TA_BILINEAR of k_tensor_aa (letterbox
    into 128 x 112, inner 128 x 96): a tie wherever the two source columns of an output differ by 2"""
    feed = _feed(built, 1)
    assert feed.step()
    t, got, _, _, _, boxes = built.pull_tensor([feed.dec], size=size, layout=lay, dtype=_torch_u8(), channels=ch, mode="bilinear",
                                               antialias=False, fit=fit, pad=(0.25, 0.5, 1.0), return_boxes=True, **_col(colour))
    left, top, iw, ih = rm.letterbox(size[1], size[0], W, H) if fit == "letterbox" else (0, 0, size[1], size[0])
    assert got == [1] and boxes == [(left, top, iw, ih)] and (iw, ih) == ((128, 96) if fit == "letterbox" else (128, 48))
    x = rm.resample_hwc(_source(colour, ch), (ih, iw), "bilinear", fma=colour == "reference")
    ref = colour == "reference"
    exact = _exact(H, ih, "bilinear", ref)[:, None] & _exact(W, iw, "bilinear", ref)[None, :]
    assert exact.all()                                  # 1/4 and 3/4, 0 and 1 at the ends
    _assert_ties(tr._hwc(t[0], lay)[top:top + ih, left:left + iw], x, colour, ("bilinear", fit, colour, ch), exact)
    feed.close()


@pytest.mark.parametrize("colour,ch,lay", KINDS)
@pytest.mark.parametrize("border", ["constant", "replicate"])
def test_remap_quarter_positions(built, border, colour, ch, lay):
    """k_tensor_remap, bilinear: every sample at x + 1/4 (even rows) or x + 3/4 (odd rows) on a row of the picture"""
    import torch
    feed = _feed(built, 1)
    assert feed.step() and feed.dec.next_output_info() is not None
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    m = np.stack([j + np.where(i % 2, 0.75, 0.25), i], axis=-1).astype(np.float32)
    maps = [torch.from_numpy(m).cuda()]
    torch.cuda.synchronize()
    t, got, _, _ = built.pull_remap([feed.dec], maps, layout=lay, dtype=_torch_u8(), channels=ch, mode="bilinear", border=border,
                                    pad=(0, 0, 0), **_col(colour))
    torch.cuda.synchronize()
    assert got == [1]
    ref = colour == "reference"
    x, padded = mm.remap(_source(colour, ch), m, "bilinear", border, (0.0, 0.0, 0.0), fma=ref)        # pad 0: the same on either scale
    assert not padded.any()
    _assert_ties(tr._hwc(t[0], lay), np.clip(x, 0, 255), colour, ("remap", border, colour, ch))
    feed.close()
