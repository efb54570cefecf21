/* kernels/k_tensor_roi.hip.h — k_tensor_roi: boxes of pictures that have been popped already, each resampled into its own slice of the
 * caller's tensor (h264bsdmiOutputTensorRegions), one launch per call, grid.y = one item per region.  Included by engine.hip AFTER
 * k_tensor_aa.hip.h: the kernel is ta_tile_body<..., BOX = true> of that header, where the scheme and what BOX switches are
 * described; like the other tensor headers, not part of the kernel sources that key the committed counter tables (srchash.py).
 *
 * A region is "convert the picture, pad it, crop it, resample the crop": the item holds the picture's source WINDOW (x0, y0, w, h of
 * the TensorItem: it decides what is picture and what is pad, and it bounds the neighbours of the bilinear chroma exactly as in a
 * pull of the whole window) and the BOX (bx, by relative to the window, signed, any parity; bw x bh), whose size is the n_in of the
 * tap arithmetic.  k_tensor_aa has one rectangle for both and needs it even.  The pad around the picture is under the scale of the
 * converted samples (spad; engine.hip, fold_pad): REF the 8-bit floor(255 pad + 0.5), otherwise 255 pad (U8) or (pad - mean) / std.
 * All three filters run through the taps: FILTER_BILINEAR is torch's antialias=False coordinate over the taps floor(f),
 * floor(f) + 1, as in k_tensor_aa's letterbox. */
#pragma once
namespace h264k {

/* one region: t the TensorItem of the picture (window, colour map) with dst = the region's slice; the box relative to the window;
 * the inner rectangle of the output it fills */
struct RoiItem { TensorItem t; int32_t bx, by; uint32_t bw, bh, left, top, iw, ih; };
/* pad: outside the inner rectangle, per output channel, under the output scale; spad: the picture's pad under the scale of the
 * converted samples */
struct RoiArgs { const RoiItem *items; uint32_t width, height, chroma, filter; float mean[3], std[3], pad[3], spad[3]; };

template <int DT, int LAYOUT, int C, bool REF>
__global__ __launch_bounds__(256) void k_tensor_roi(RoiArgs a)
{
    ta_tile_body<DT, LAYOUT, C, REF, true>(a);
}

} // namespace h264k
