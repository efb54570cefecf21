/* kernels/k_tensor_roi.hip.h — k_tensor_roi: boxes of pictures that have been popped already, each resampled into its own slice of the
 * caller's tensor (h264bsdmiOutputTensorRegions), one launch per call, grid.y = one item per region.  Included by engine.hip AFTER
 * k_tensor_aa.hip.h, whose scheme it follows and whose helpers it uses (ta_taps, ta_filter; tc_chroma_seg, tc_value and the element
 * encoders of k_tensor_out.hip.h); like them, not part of the kernel sources that key the committed counter tables (srchash.py).
 *
 * A region is "convert the picture, pad it, crop it, resample the crop": the item holds the picture's source WINDOW (x0, y0, w, h of
 * the TensorItem: it decides what is picture and what is pad, and it bounds the neighbours of the bilinear chroma exactly as in a
 * pull of the whole window) and the BOX (bx, by relative to the window, signed, any parity; bw x bh), whose size is the n_in of the
 * tap arithmetic.  k_tensor_aa has one rectangle for both and needs it even.
 *
 * Per output tile of 32 x 8 the source band follows from the taps of the tile's first and last inner column and row, in absolute
 * frame coordinates that may be negative or lie beyond the frame.  It is walked in chunks of 8 rows x 320 columns that start on a
 * multiple of 8 columns, as in k_tensor_aa.  A segment of 8 samples whose row or columns miss the window altogether is filled with
 * the pad and forms no address; one that straddles the window's left or right edge is loaded whole (it lies in the window's
 * 8-aligned hull, which the coded frame contains: its width is a multiple of 16), converted, and the samples outside are replaced by
 * the pad.  The pad is under the scale of the converted samples (engine.hip): REF the 8-bit floor(255 pad + 0.5), otherwise 255 pad
 * (U8) or (pad - mean) / std.  A tile whose band misses the window loads nothing and takes the pad itself, so that a box outside the
 * picture is the pad exactly.  All three filters run through the taps: FILTER_BILINEAR is torch's antialias=False coordinate over
 * the taps floor(f), floor(f) + 1, as in k_tensor_aa's letterbox. */
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
    constexpr int NC = tc_nc<C>();
    typedef typename ToElem<DT>::T E;
    __shared__ float sbuf[TAA_RC][TAA_SC][NC];
    __shared__ float hbuf[TAA_RC][TAA_COLS][NC];
    __shared__ TaTap tcol[TAA_COLS], trow[TAA_ROWS];
    const RoiItem ri = a.items[blockIdx.y];
    const TensorItem &it = ri.t;
    const uint32_t W = a.width, H = a.height, filter = a.filter, tid = threadIdx.x;
    const int wmb = (int)it.wmb;
    const int wx0 = (int)it.x0, wy0 = (int)it.y0, wx1 = wx0 + (int)it.w, wy1 = wy0 + (int)it.h;     /* the window, absolute */
    const int x0 = wx0 + ri.bx, y0 = wy0 + ri.by;                                                   /* the box's origin, absolute */
    const bool bil = !REF && a.chroma == TC_BILINEAR;
    const uint32_t chi = (it.x0 + it.w) / 2u - 1u, rlo = it.y0 / 2u, rhi = (it.y0 + it.h) / 2u - 1u, ccw = it.wmb * 8u;
    const float invs_x = filter == TA_BILINEAR ? 1.0f : (float)(1.0 / fmax((double)ri.bw / (double)ri.iw, 1.0));
    const float invs_y = filter == TA_BILINEAR ? 1.0f : (float)(1.0 / fmax((double)ri.bh / (double)ri.ih, 1.0));
    const uint32_t nux = (W + TAA_COLS - 1u) / TAA_COLS, units = nux * ((H + TAA_ROWS - 1u) / TAA_ROWS);
    const uint32_t col = tid % TAA_COLS, row = tid / TAA_COLS;
    const size_t plane = (size_t)W * H;
    E *dst = reinterpret_cast<E *>(it.dst);
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int tx = (int)((u % nux) * TAA_COLS), ty = (int)((u / nux) * TAA_ROWS);
        /* the tile's inner columns and rows, tile-relative [c_lo, c_hi) x [r_lo, r_hi) */
        const int c_lo = min(max((int)ri.left - tx, 0), TAA_COLS), c_hi = min(max((int)(ri.left + ri.iw) - tx, 0), TAA_COLS);
        const int r_lo = min(max((int)ri.top - ty, 0), TAA_ROWS), r_hi = min(max((int)(ri.top + ri.ih) - ty, 0), TAA_ROWS);
        const bool inner = (int)col >= c_lo && (int)col < c_hi && (int)row >= r_lo && (int)row < r_hi;
        float acc[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) acc[c] = 0.0f;
        if (c_lo < c_hi && r_lo < r_hi) {
            if ((int)tid >= c_lo && (int)tid < c_hi)
                ta_taps<REF>(tcol[tid], filter, (uint32_t)(tx + (int)tid - (int)ri.left), ri.iw, ri.bw, invs_x);
            else if (tid >= TAA_COLS && (int)tid - TAA_COLS >= r_lo && (int)tid - TAA_COLS < r_hi)
                ta_taps<REF>(trow[tid - TAA_COLS], filter, (uint32_t)(ty + (int)tid - TAA_COLS - (int)ri.top), ri.ih, ri.bh, invs_y);
            __syncthreads();
            const TaTap mc = (int)col >= c_lo && (int)col < c_hi ? tcol[col] : TaTap{ 0, 0, 0.0f, 0.0f };
            const TaTap mr = (int)row >= r_lo && (int)row < r_hi ? trow[row] : TaTap{ 0, 0, 0.0f, 0.0f };
            const int bx0 = x0 + tcol[c_lo].lo, bx1 = x0 + tcol[c_hi - 1].lo + tcol[c_hi - 1].n;      /* the source band, absolute */
            const int by0 = y0 + trow[r_lo].lo, by1 = y0 + trow[r_hi - 1].lo + trow[r_hi - 1].n;
            if (bx1 <= wx0 || bx0 >= wx1 || by1 <= wy0 || by0 >= wy1) {        /* nothing of the picture: the pad itself */
#pragma unroll
                for (int c = 0; c < NC; c++) acc[c] = a.spad[c];
            } else {
                const int xs = bx0 & ~7;
                for (int yc = by0; yc < by1; yc += TAA_RC) {
                    const int nr = min(TAA_RC, by1 - yc);
                    float hacc[NC];
#pragma unroll
                    for (int c = 0; c < NC; c++) hacc[c] = 0.0f;
                    for (int cs = xs; cs < bx1; cs += TAA_SC) {
                        const int ng = (min(cs + TAA_SC, bx1) - cs + 7) / 8;
                        for (int g = (int)tid; g < nr * ng; g += 256) {
                            const int rr = g / ng, gx = g % ng;
                            const int sx = cs + 8 * gx, sy = yc + rr;
                            if (sy < wy0 || sy >= wy1 || sx + TO_SEG <= wx0 || sx >= wx1) {
#pragma unroll
                                for (int k = 0; k < TO_SEG; k++)
#pragma unroll
                                    for (int c = 0; c < NC; c++) sbuf[rr][8 * gx + k][c] = a.spad[c];
                                continue;
                            }
                            const unsigned long long yv = *reinterpret_cast<const unsigned long long *>(it.src + luma_at(wmb, sx, sy));
                            float cb[TO_SEG], cr[TO_SEG];
                            if constexpr (NC == 3) {
                                const uint32_t cy = (uint32_t)sy >> 1, nb = (sy & 1) ? min(cy + 1u, rhi) : max(cy, rlo + 1u) - 1u;
                                tc_chroma_seg(cb, it.src, wmb, 0, (uint32_t)sx, (uint32_t)sy, ccw, bil, nb, chi);
                                tc_chroma_seg(cr, it.src, wmb, 1, (uint32_t)sx, (uint32_t)sy, ccw, bil, nb, chi);
                            }
#pragma unroll
                            for (int k = 0; k < TO_SEG; k++) {
                                const float y = (float)(uint32_t)((yv >> (8 * k)) & 255u);
                                const bool in = sx + k >= wx0 && sx + k < wx1;
                                float p[NC];
                                if constexpr (NC == 1) p[0] = __builtin_amdgcn_fmed3f(fmaf(it.k[0][0], y, it.k[0][3]), it.lo[0], it.hi[0]);
                                else {
#pragma unroll
                                    for (int c = 0; c < 3; c++) p[c] = tc_value(it, c, y, cb[k], cr[k]);
                                }
#pragma unroll
                                for (int c = 0; c < NC; c++) sbuf[rr][8 * gx + k][c] = !in ? a.spad[c] : REF ? __builtin_truncf(p[c]) : p[c];
                            }
                        }
                        __syncthreads();
                        if ((int)row < nr && mc.n) {
                            const int xa = max(x0 + mc.lo, cs), xb = min(x0 + mc.lo + mc.n, cs + TAA_SC);
                            for (int x = xa; x < xb; x++) {
                                const float w = ta_filter(filter, ((float)(x - x0 - mc.lo) - mc.cr) * invs_x);
#pragma unroll
                                for (int c = 0; c < NC; c++) hacc[c] = fmaf(w, sbuf[row][x - cs][c], hacc[c]);
                            }
                        }
                        __syncthreads();
                    }
#pragma unroll
                    for (int c = 0; c < NC; c++) hbuf[row][col][c] = hacc[c] * mc.norm;
                    __syncthreads();
                    if (mr.n) {
                        const int ya = max(y0 + mr.lo, yc), yb = min(y0 + mr.lo + mr.n, yc + nr);
                        for (int y = ya; y < yb; y++) {
                            const float w = ta_filter(filter, ((float)(y - y0 - mr.lo) - mr.cr) * invs_y) * mr.norm;
#pragma unroll
                            for (int c = 0; c < NC; c++) acc[c] = fmaf(w, hbuf[y - yc][col][c], acc[c]);
                        }
                    }
                }
            }
            __syncthreads();        /* tcol / trow / hbuf are the next tile's */
        }
        const uint32_t ox = (uint32_t)tx + col, oy = (uint32_t)ty + row;
        if (ox >= W || oy >= H) continue;
        const size_t pix = (size_t)oy * W + ox;
#pragma unroll
        for (int c = 0; c < C; c++) {
            E e;
            if (c == 3) e = tc_alpha<DT>();
            else if (!inner) {
                if constexpr (DT == TO_U8) e = (E)(uint32_t)a.pad[c];
                else e = to_enc<DT>(a.pad[c]);
            } else if constexpr (REF) {
                if constexpr (DT == TO_U8) e = (E)(int)(__builtin_amdgcn_fmed3f(acc[c], 0.0f, 255.0f) + 0.5f);
                else e = to_enc<DT>((acc[c] / 255.0f - a.mean[c]) / a.std[c]);
            } else {
                e = tc_enc<DT>(DT == TO_U8 ? __builtin_amdgcn_fmed3f(acc[c], 0.0f, 255.0f) : acc[c]);
            }
            if constexpr (LAYOUT == TO_NCHW) dst[c * plane + pix] = e;
            else dst[pix * C + c] = e;
        }
    }
}

} // namespace h264k
