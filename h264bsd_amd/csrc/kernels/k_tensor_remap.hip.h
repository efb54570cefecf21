/* kernels/k_tensor_remap.hip.h — k_tensor_remap: current pictures sampled through caller-supplied coordinate maps, each map into its
 * own slice of the caller's tensor (h264bsdmiOutputTensorRemap), one launch per call, grid.y = one item per map.  Included by
 * engine.hip AFTER k_tensor_roi.hip.h; it uses the helpers of k_tensor_out.hip.h (TcWin, tc_pixel, tc_blend, the element encoders) and,
 * like the other tensor kernels, is not part of the kernel sources that key the committed counter tables (srchash.py).
 *
 * The coordinates are data: map[oy][ox] = (mx, my), a position in luma samples of the picture's source WINDOW (x0, y0, w, h of the
 * TensorItem), sample (u, v) AT (u, v).  There is no projective arithmetic here: a finite map value is clamped in fp32 ([-1, w]
 * CONSTANT, [0, w - 1] REPLICATE), its floor is the first neighbour and the remainder the weight (exact in fp32 from 0 up; in (-1, 0) rounded to nearest).  A non-finite
 * value writes the pad under the output's scale and forms no address.
 *
 * A workgroup takes an output tile of 32 x 8 at a time, one output pixel per lane: one 8-byte map load per lane (32 lanes read 256
 * contiguous bytes), then the 2 x 2 neighbours gathered straight from the macroblock-tiled frame.  Every neighbour index is clamped
 * into the window before an address is formed, and a neighbour outside the window (CONSTANT) is not loaded at all: it takes the
 * pad under the scale of the converted samples (spad, as in k_tensor_roi).  The four neighbours share their chroma: per plane the
 * quad needs at most the chroma columns cA, cA + 1 (cA that of the first neighbour) and the rows rA - 1, rA, rA + 1, so 2 x 3 samples
 * per plane are loaded once (2 x 2 with nearest chroma) and every neighbour picks its own by comparing indices — 4 + 12 byte loads
 * for a pixel instead of the 36 of four independent conversions.  The chroma arithmetic per neighbour is tcr_convert's, the blend is
 * k_tensor_resize's (tc_blend) and the store tail is the one of k_tensor_aa.hip.h's tile body for the same REF; NEAREST is the same
 * path with one neighbour and weights 0.  No
 * antialiasing: a map that shrinks the picture aliases. */
#pragma once
namespace h264k {

enum { TR_NEAREST = 0, TR_BILINEAR = 1 };
enum { TR_CONSTANT = 0, TR_REPLICATE = 1 };

/* one map: t the TensorItem of the picture (window, colour map) with dst = the map's slice; map: float32 [height][width][2], x then y */
struct RemapItem { TensorItem t; const float *map; };
/* pad: a non-finite coordinate, per output channel, under the output scale; spad: outside the window, under the scale of the
 * converted samples */
struct RemapArgs { const RemapItem *items; uint32_t width, height, chroma, filter, border; float mean[3], std[3], pad[3], spad[3]; };

/* The colours of the neighbours (X[kx], Y[ky]), k = 2 ky + kx < nk, of one output pixel into q[k][0 .. NC); REF: the 8-bit values.
 * X, Y: absolute frame coordinates INSIDE the window with X[1] - X[0], Y[1] - Y[0] in {0, 1}; ok[k]: the neighbour is part of the
 * picture (else it takes spad and nothing is loaded for it). */
template <int NC, bool REF>
__device__ __forceinline__ void trm_quad(float (*q)[NC], const TensorItem &it, int wmb, const TcWin &w, int nk, const uint32_t *X, const uint32_t *Y,
                                         const bool *ok, const float *spad)
{
    const bool bil = w.bil;
    const uint32_t chi = w.chi, rlo = w.rlo, rhi = w.rhi;
    const uint8_t *__restrict__ src = it.src;
    const bool any = ok[0] || ok[1] || ok[2] || ok[3];
    float P[2][3][2];       /* plane, chroma row R[.], chroma column cA / cB */
    const uint32_t cA = X[0] >> 1, cB = min(cA + 1u, chi), rA = Y[0] >> 1;
    const uint32_t R[3] = { max(rA, rlo + 1u) - 1u, rA, min(rA + 1u, rhi) };
    if constexpr (NC == 3) {
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const bool need = any && (r > 0 || (bil && !(Y[0] & 1u)));     /* the row above: bilinear chroma of an even luma row */
                P[p][r][0] = need ? (float)src[chroma_at(wmb, p, (int)cA, (int)R[r])] : 0.0f;
                P[p][r][1] = need ? (float)src[chroma_at(wmb, p, (int)cB, (int)R[r])] : 0.0f;
            }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (k >= nk) continue;
        const uint32_t x = X[k & 1], y = Y[k >> 1];
        const float Yv = ok[k] ? (float)src[luma_at(wmb, (int)x, (int)y)] : 0.0f;
        float t[NC], cc[2] = { 0.0f, 0.0f };
        if constexpr (NC == 3) {
            const uint32_t c0 = x >> 1, r0 = y >> 1;
            const uint32_t c1 = bil ? min(c0 + (x & 1u), chi) : c0;
            const uint32_t r1 = !bil ? r0 : w.nb(y);
#pragma unroll
            for (int p = 0; p < 2; p++) {
                /* rows r0, r1 of the patch: equal indices hold equal samples, so the comparison picks the right one under the clamps */
                const float a0 = r0 == R[1] ? P[p][1][0] : P[p][2][0], a1 = r0 == R[1] ? P[p][1][1] : P[p][2][1];
                const float b0 = r1 == R[1] ? P[p][1][0] : r1 < R[1] ? P[p][0][0] : P[p][2][0];
                const float b1 = r1 == R[1] ? P[p][1][1] : r1 < R[1] ? P[p][0][1] : P[p][2][1];
                const float ra0 = c0 == cA ? a0 : a1, ra1 = c1 == cA ? a0 : a1;
                const float rb0 = c0 == cA ? b0 : b1, rb1 = c1 == cA ? b0 : b1;
                cc[p] = bil ? fmaf(0.25f, 0.5f * (rb0 + rb1), 0.75f * (0.5f * (ra0 + ra1))) : ra0;
            }
        }
        tc_pixel<NC, REF>(t, it, Yv, cc[0] - 128.0f, cc[1] - 128.0f);
#pragma unroll
        for (int c = 0; c < NC; c++) q[k][c] = !ok[k] ? spad[c] : t[c];
    }
}

constexpr int TRM_COLS = 32, TRM_ROWS = 8;      /* output tile of one workgroup and step */

template <int DT, int LAYOUT, int C, bool REF>
__global__ __launch_bounds__(256) void k_tensor_remap(RemapArgs a)
{
    constexpr int NC = tc_nc<C>();
    typedef typename ToElem<DT>::T E;
    const RemapItem ri = a.items[blockIdx.y];
    const TensorItem &it = ri.t;
    const uint32_t W = a.width, H = a.height, tid = threadIdx.x;
    const int wmb = (int)it.wmb, ww = (int)it.w, wh = (int)it.h;
    const bool nearest = a.filter == TR_NEAREST, rep = a.border == TR_REPLICATE;
    const TcWin win = tc_win<REF>(it, a.chroma);
    const float xlo = rep ? 0.0f : -1.0f, xhi = rep ? (float)(ww - 1) : (float)ww;
    const float ylo = rep ? 0.0f : -1.0f, yhi = rep ? (float)(wh - 1) : (float)wh;
    const uint32_t nux = (W + TRM_COLS - 1u) / TRM_COLS, units = nux * ((H + TRM_ROWS - 1u) / TRM_ROWS);
    const uint32_t col = tid % TRM_COLS, row = tid / TRM_COLS;
    const size_t plane = (size_t)W * H;
    const float2 *__restrict__ map = reinterpret_cast<const float2 *>(ri.map);
    const float spad[3] = { a.spad[0], a.spad[1], a.spad[2] };
    E *dst = reinterpret_cast<E *>(it.dst);
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t ox = (u % nux) * TRM_COLS + col, oy = (u / nux) * TRM_ROWS + row;
        if (ox >= W || oy >= H) continue;
        const size_t pix = (size_t)oy * W + ox;
        const float2 m = map[pix];
        const bool finite = fabsf(m.x) < __builtin_inff() && fabsf(m.y) < __builtin_inff();      /* false for NaN as well */
        float acc[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) acc[c] = 0.0f;
        if (finite) {
            const float cx = fminf(fmaxf(m.x, xlo), xhi), cy = fminf(fmaxf(m.y, ylo), yhi);
            const float fx = nearest ? floorf(cx + 0.5f) : floorf(cx), fy = nearest ? floorf(cy + 0.5f) : floorf(cy);
            const float lx = nearest ? 0.0f : cx - fx, ly = nearest ? 0.0f : cy - fy;
            const int xi[2] = { (int)fx, (int)fx + (nearest ? 0 : 1) }, yi[2] = { (int)fy, (int)fy + (nearest ? 0 : 1) };
            /* REPLICATE: only x0 + 1 = w (weight 0) can lie outside; its index is clamped like every address below */
            const bool vx[2] = { rep || (xi[0] >= 0 && xi[0] < ww), rep || (xi[1] >= 0 && xi[1] < ww) };
            const bool vy[2] = { rep || (yi[0] >= 0 && yi[0] < wh), rep || (yi[1] >= 0 && yi[1] < wh) };
            const bool ok[4] = { vx[0] && vy[0], vx[1] && vy[0], vx[0] && vy[1], vx[1] && vy[1] };
            const uint32_t X[2] = { it.x0 + (uint32_t)min(max(xi[0], 0), ww - 1), it.x0 + (uint32_t)min(max(xi[1], 0), ww - 1) };
            const uint32_t Y[2] = { it.y0 + (uint32_t)min(max(yi[0], 0), wh - 1), it.y0 + (uint32_t)min(max(yi[1], 0), wh - 1) };
            float q[4][NC];
            trm_quad<NC, REF>(q, it, wmb, win, nearest ? 1 : 4, X, Y, ok, spad);
            if (nearest) {
#pragma unroll
                for (int c = 0; c < NC; c++) acc[c] = q[0][c];
            } else {
#pragma unroll
                for (int c = 0; c < NC; c++) acc[c] = tc_blend<REF>(q[0][c], q[1][c], q[2][c], q[3][c], lx, ly);
            }
        }
        /* the store tail of ta_tile_body (k_tensor_aa.hip.h), statement for statement: change both or neither */
#pragma unroll
        for (int c = 0; c < C; c++) {
            E e;
            if (c == 3) e = tc_alpha<DT>();
            else if (!finite) {
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
