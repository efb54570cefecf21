/* kernels/k_tensor_aa.hip.h — k_tensor_aa: the separable, table-driven resampler of h264bsdmiNextOutputTensorBatchResize (torch's
 * bilinear / bicubic with antialias=True, and letterboxing), and ta_tile_body, the tile body it shares with k_tensor_roi
 * (k_tensor_roi.hip.h, included after this header).  Included by engine.hip AFTER k_tensor_out.hip.h (whose item, window, segment and
 * element helpers it uses); like it, not part of the kernel sources that key the committed counter tables (srchash.py).
 *
 * Weights (include/h264bsd_mi355x.h): output index i of an inner size n_out over a source window of n_in samples, scale = n_in / n_out,
 * center = scale (i + 0.5), support = (interp / 2) max(scale, 1); taps xmin = max((int)(center - support + 0.5), 0) .. xmax =
 * min((int)(center + support + 0.5), n_in), tap x weighted filter((x - center + 0.5) / max(scale, 1)), normalised by the sum of the
 * taps; triangle 1 - |t| (interp 2) or Keys' cubic with a = -0.5 (interp 4).  FILTER_BILINEAR (letterbox only; stretch takes
 * k_tensor_resize) is the same machinery with torch's antialias=False coordinate f = max((i + 0.5) scale - 0.5, 0), computed in fp32 as
 * tcr_coord does, and the triangle over the taps floor(f) and floor(f) + 1 (the second one dropped at the last source sample).  The
 * tap bounds and centres are computed in fp64 per tile, once per output column and row; a weight is evaluated in fp32 from the tap's
 * offset to its centre, so that it keeps full precision however large the source coordinate.
 *
 * What is interpolated is what k_tensor_resize interpolates: REF, the reference's 8-bit R, G, B (or luma) through the item's map,
 * truncated; otherwise the unquantised colour already under the output scale (255 v for U8, (v - mean) / std for floats).  REF floats
 * are then (v / 255 - mean[c]) / std[c]; U8 is clamped to [0, 255] (bicubic may overshoot) and rounded as k_tensor_resize rounds
 * (REF halves up, otherwise rint).  Pixels outside the inner rectangle of a picture are the call's pad, already under the output
 * scale (engine.hip, fold_pad); alpha is 255 / 1.0.  k_tensor_remap's tail is this one, statement for statement: the equalities
 * between the families rest on the two staying the same. */
#pragma once
namespace h264k {

/* one picture: the TensorItem of k_tensor_out / k_tensor_resize and the inner rectangle of the output it fills */
struct AaItem { TensorItem t; uint32_t left, top, iw, ih; };
/* pad: the value written outside the inner rectangle, per output channel, under the output scale (U8: an integer) */
struct AaArgs { const AaItem *items; uint32_t width, height, chroma, filter; float mean[3], std[3], pad[3]; };

enum { TA_BILINEAR = 0, TA_BILINEAR_AA = 1, TA_BICUBIC_AA = 2 };
constexpr int TAA_COLS = 32, TAA_ROWS = 8;      /* output tile of one workgroup and step */
constexpr int TAA_RC = 8, TAA_SC = 320;         /* source rows x columns converted into LDS at a time (TAA_SC: a multiple of 8) */

/* the taps of one output column or row: the first one (relative to the window), their count, the centre's offset from the first
 * one and the reciprocal of the sum of the weights */
struct TaTap { int lo, n; float cr, norm; };

__device__ __forceinline__ float ta_filter(uint32_t filter, float t)
{
    t = fabsf(t);
    if (filter == TA_BICUBIC_AA)
        return t < 1.0f ? fmaf(fmaf(1.5f, t, -2.5f), t * t, 1.0f) : t < 2.0f ? fmaf(fmaf(fmaf(-0.5f, t, 2.5f), t, -4.0f), t, 2.0f) : 0.0f;
    return fmaxf(1.0f - t, 0.0f);
}

template <bool REF>
__device__ __forceinline__ void ta_taps(TaTap &tp, uint32_t filter, uint32_t o, uint32_t n_out, uint32_t n_in, float invs)
{
    int lo, hi;
    float cr;
    if (filter == TA_BILINEAR) {
        float l;
        tcr_coord<REF>(o, (float)n_in / (float)n_out, lo, l);
        hi = min(lo + 2, (int)n_in);
        cr = l;
    } else {
        const double scale = (double)n_in / (double)n_out, center = scale * ((double)o + 0.5);
        const double support = (filter == TA_BICUBIC_AA ? 2.0 : 1.0) * fmax(scale, 1.0);
        lo = max((int)(center - support + 0.5), 0);
        hi = min((int)(center + support + 0.5), (int)n_in);
        cr = (float)(center - 0.5 - (double)lo);
    }
    float s = 0.0f;
    for (int j = 0; j < hi - lo; j++) s += ta_filter(filter, ((float)j - cr) * invs);
    tp.lo = lo;
    tp.n = hi - lo;
    tp.cr = cr;
    tp.norm = 1.0f / s;
}

/* The tile body of k_tensor_aa (BOX = false) and k_tensor_roi (BOX = true, k_tensor_roi.hip.h).
 *
 * A workgroup takes an output tile of 32 columns x 8 rows of one item at a time.  From the taps of its first and last inner
 * column and row (computed by 40 lanes into LDS) it knows the source band it reads, and walks it in chunks of 8 source rows x 320
 * source columns that start on a multiple of 8 columns: each chunk is converted once, 8 horizontally adjacent pixels per lane and
 * slot from one 8-byte luma load and word loads of chroma (tc_seg), into LDS; then lane (r, c) accumulates the horizontal taps of
 * output column c over source row r of the chunk in registers (a wider band than 320 columns takes several chunks and keeps the
 * partial sums).  The row's sums go to LDS, and lane (r, c) adds the vertical taps of output pixel (r, c) that fall in the chunk's
 * rows.  So LDS is bounded whatever the scale (34 KB for 3 channels), a source pixel is converted once per tile that reads it, and
 * extreme downscaling only lengthens the walk.  Tiles or lanes outside the inner rectangle write the pad and read nothing.
 *
 * BOX switches three things.  (1) The n_in and the origin of the tap arithmetic: the item's box (bx, by relative to the window,
 * signed, any parity; bw x bh) instead of the window itself, so the band is in absolute frame coordinates that may be negative or lie
 * beyond the frame.  (2) The window tests: a tile whose band misses the window loads nothing and takes spad itself (a box outside
 * the picture is the pad exactly); a segment of 8 samples whose row or columns miss the window is filled with spad and forms no
 * address.  (3) The per-sample patch: a segment that straddles the window's left or right edge is loaded whole (it lies in the
 * window's 8-aligned hull, which the coded frame contains: its width is a multiple of 16), converted, and the samples outside are
 * replaced by spad.  Without BOX none of the tests exists: the band of a window lies inside it. */
template <int DT, int LAYOUT, int C, bool REF, bool BOX, typename Args>
__device__ __forceinline__ void ta_tile_body(const Args &a)
{
    constexpr int NC = tc_nc<C>();
    typedef typename ToElem<DT>::T E;
    __shared__ float sbuf[TAA_RC][TAA_SC][NC];
    __shared__ float hbuf[TAA_RC][TAA_COLS][NC];
    __shared__ TaTap tcol[TAA_COLS], trow[TAA_ROWS];
    const auto ai = a.items[blockIdx.y];
    const TensorItem &it = ai.t;
    const uint32_t W = a.width, H = a.height, filter = a.filter, tid = threadIdx.x;
    const int wmb = (int)it.wmb;
    const int wx0 = (int)it.x0, wy0 = (int)it.y0, wx1 = wx0 + (int)it.w, wy1 = wy0 + (int)it.h;     /* the window, absolute */
    int x0 = wx0, y0 = wy0;                             /* the origin and the size of what the taps run over, absolute */
    uint32_t n_x = it.w, n_y = it.h;
    if constexpr (BOX) { x0 += ai.bx; y0 += ai.by; n_x = ai.bw; n_y = ai.bh; }
    const TcWin win = tc_win<REF>(it, a.chroma);
    const float invs_x = filter == TA_BILINEAR ? 1.0f : (float)(1.0 / fmax((double)n_x / (double)ai.iw, 1.0));
    const float invs_y = filter == TA_BILINEAR ? 1.0f : (float)(1.0 / fmax((double)n_y / (double)ai.ih, 1.0));
    const uint32_t nux = (W + TAA_COLS - 1u) / TAA_COLS, units = nux * ((H + TAA_ROWS - 1u) / TAA_ROWS);
    const uint32_t col = tid % TAA_COLS, row = tid / TAA_COLS;
    const size_t plane = (size_t)W * H;
    E *dst = reinterpret_cast<E *>(it.dst);
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int tx = (int)((u % nux) * TAA_COLS), ty = (int)((u / nux) * TAA_ROWS);
        /* the tile's inner columns and rows, tile-relative [c_lo, c_hi) x [r_lo, r_hi) */
        const int c_lo = min(max((int)ai.left - tx, 0), TAA_COLS), c_hi = min(max((int)(ai.left + ai.iw) - tx, 0), TAA_COLS);
        const int r_lo = min(max((int)ai.top - ty, 0), TAA_ROWS), r_hi = min(max((int)(ai.top + ai.ih) - ty, 0), TAA_ROWS);
        const bool inner = (int)col >= c_lo && (int)col < c_hi && (int)row >= r_lo && (int)row < r_hi;
        float acc[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) acc[c] = 0.0f;
        if (c_lo < c_hi && r_lo < r_hi) {
            if ((int)tid >= c_lo && (int)tid < c_hi)
                ta_taps<REF>(tcol[tid], filter, (uint32_t)(tx + (int)tid - (int)ai.left), ai.iw, n_x, invs_x);
            else if (tid >= TAA_COLS && (int)tid - TAA_COLS >= r_lo && (int)tid - TAA_COLS < r_hi)
                ta_taps<REF>(trow[tid - TAA_COLS], filter, (uint32_t)(ty + (int)tid - TAA_COLS - (int)ai.top), ai.ih, n_y, invs_y);
            __syncthreads();
            const TaTap mc = (int)col >= c_lo && (int)col < c_hi ? tcol[col] : TaTap{ 0, 0, 0.0f, 0.0f };
            const TaTap mr = (int)row >= r_lo && (int)row < r_hi ? trow[row] : TaTap{ 0, 0, 0.0f, 0.0f };
            const int bx0 = x0 + tcol[c_lo].lo, bx1 = x0 + tcol[c_hi - 1].lo + tcol[c_hi - 1].n;      /* the source band, absolute */
            const int by0 = y0 + trow[r_lo].lo, by1 = y0 + trow[r_hi - 1].lo + trow[r_hi - 1].n;
            if (BOX && (bx1 <= wx0 || bx0 >= wx1 || by1 <= wy0 || by0 >= wy1)) {      /* nothing of the picture: the pad itself */
                if constexpr (BOX) {
#pragma unroll
                    for (int c = 0; c < NC; c++) acc[c] = a.spad[c];
                }
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
                            if constexpr (BOX) {
                                if (sy < wy0 || sy >= wy1 || sx + TO_SEG <= wx0 || sx >= wx1) {
#pragma unroll
                                    for (int k = 0; k < TO_SEG; k++)
#pragma unroll
                                        for (int c = 0; c < NC; c++) sbuf[rr][8 * gx + k][c] = a.spad[c];
                                    continue;
                                }
                            }
                            const unsigned long long yv = *reinterpret_cast<const unsigned long long *>(it.src + luma_at(wmb, sx, sy));
                            tc_seg<NC, REF>(it, wmb, win, yv, (uint32_t)sx, (uint32_t)sy, [&](int k, const float *p) {
#pragma unroll
                                for (int c = 0; c < NC; c++) {
                                    float v = p[c];
                                    if constexpr (BOX) v = sx + k >= wx0 && sx + k < wx1 ? v : a.spad[c];
                                    sbuf[rr][8 * gx + k][c] = v;
                                }
                            });
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
        /* the store tail; k_tensor_remap (k_tensor_remap.hip.h) holds its twin, statement for statement: change both or neither */
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

template <int DT, int LAYOUT, int C, bool REF>
__global__ __launch_bounds__(256) void k_tensor_aa(AaArgs a)
{
    ta_tile_body<DT, LAYOUT, C, REF, false>(a);
}

} // namespace h264k
