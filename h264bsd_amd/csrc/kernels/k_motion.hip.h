/* kernels/k_motion.hip.h — the motion side information of decoded pictures: k_motion_keep expands it from the frame jobs of a tick
 * into a buffer that lives beside the picture's frame buffer (h264bsdmiSetMotionExport), k_motion_roi resamples boxes of it onto the
 * grid of a tensor pull (h264bsdmiOutputMotionRegions).  Included by engine.hip after the k_tensor_* headers, whose element encoders
 * and tile shape it uses; like them, not part of the kernel sources that key the committed counter tables (srchash.py).
 *
 * One slot of side information, for a picture of wmb x hmb macroblocks (n = wmb hmb), three planes one behind the other:
 *     mv    uint32 [4 hmb][4 wmb]   one word per 4x4 block, RASTER over the picture: int16 x in the low half, int16 y in the high half,
 *                                   quarter samples; 0 where the block is invalid
 *     quad  uint16 [2 hmb][2 wmb]   one per 8x8 quadrant: bits 0-7 the age of its reference, bit 8 valid
 *     mb    uint16 [hmb][wmb]       one per macroblock: bits 0-7 FjMbRec.kind, bits 8-15 FjMbRec.qp_y
 * 74 bytes per macroblock.  The planes are rasters of the PICTURE, not macroblock tiles as the pixels are: a row of output pixels of
 * k_motion_roi walks along a row of 4x4 blocks, so neighbouring lanes read neighbouring words, and the 16 lanes that k_motion_keep
 * gives to a block row of four macroblocks write 64 contiguous bytes. */
#pragma once
namespace h264k {

constexpr uint32_t MOTION_MV_BYTES = 64, MOTION_QUAD_BYTES = 8, MOTION_MB_BYTES = 2;      /* per macroblock */
__host__ __device__ constexpr size_t motion_slot_bytes(uint32_t n_mbs)
{
    return ((size_t)n_mbs * (MOTION_MV_BYTES + MOTION_QUAD_BYTES + MOTION_MB_BYTES) + 255u) & ~(size_t)255u;
}

/* one job of a tick whose instance exports motion: the records and the sparse vector section of its device copy, the slot buffer
 * it fills, and per DPB slot the age of a reference to it (0: not written since the sequence began, or the picture's own) */
struct MotionKeepItem {
    const FjMbRec *recs; const int16_t *mvx; uint8_t *dst;
    uint32_t n_mbs, wmb, n_slots, n_mvx;
    uint8_t age[FJ_MAX_SLOTS + 3];
};

/* grid (groups of 16 macroblocks, jobs) x 256: a wavefront takes four consecutive macroblocks, lane = 16 (block row) + 4 (macroblock)
 * + block column.  Every macroblock of the picture is written, so that the slot never shows a mixture of two pictures. */
__global__ __launch_bounds__(256) void k_motion_keep(const MotionKeepItem *items)
{
    const MotionKeepItem &it = items[blockIdx.y];
    const uint32_t n_mbs = it.n_mbs, wmb = it.wmb, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t *mvp = reinterpret_cast<uint32_t *>(it.dst);
    uint16_t *quadp = reinterpret_cast<uint16_t *>(it.dst + (size_t)n_mbs * MOTION_MV_BYTES);
    uint16_t *mbp = reinterpret_cast<uint16_t *>(it.dst + (size_t)n_mbs * (MOTION_MV_BYTES + MOTION_QUAD_BYTES));
    const uint32_t by = lane >> 4, bx = lane & 3u, blk = 4u * by + bx, qd = (by >> 1) * 2u + (bx >> 1);
    for (uint32_t g = blockIdx.x; g * 16u < n_mbs; g += gridDim.x) {
        const uint32_t mb = g * 16u + wave * 4u + ((lane >> 2) & 3u);
        if (mb >= n_mbs) continue;
        const uint4 *rp = reinterpret_cast<const uint4 *>(it.recs + mb);
        const uint4 r0 = rp[0], r1 = rp[1];
        const uint32_t kind = r0.x & 255u, qp_y = (r0.x >> 8) & 255u, pred = r0.y & 255u;
        const uint32_t slot = kind == FJ_MB_CONCEAL_P ? (r1.x & 255u) : ((r1.x >> (8u * qd)) & 255u);
        const bool valid = (kind == FJ_MB_INTER || kind == FJ_MB_CONCEAL_P) && slot < it.n_slots;
        uint32_t v = 0;
        if (valid && kind == FJ_MB_INTER) {
            if (pred & FJ_PRED_UNIFORM_MV) v = r1.z;
            else if (r1.w < it.n_mvx) v = reinterpret_cast<const uint32_t *>(it.mvx)[(size_t)r1.w * 16u + blk];
        }
        const uint32_t mbx = mb % wmb, mby = mb / wmb;
        mvp[(size_t)(4u * mby + by) * (4u * wmb) + 4u * mbx + bx] = v;
        if (!((bx | by) & 1u))
            quadp[(size_t)(2u * mby + (by >> 1)) * (2u * wmb) + 2u * mbx + (bx >> 1)] = (uint16_t)(valid ? 256u | it.age[slot] : 0u);
        if (!blk) mbp[mb] = (uint16_t)(kind | (qp_y << 8));
    }
}

enum { MO_NEAREST = 0, MO_AREA = 1 };
enum { MO_MV = 1, MO_VALID = 2, MO_AGE = 4, MO_QP = 8 };
/* one region: the slot of side information, the region's slice of the output, the picture's size, its source window, the box relative
 * to the window, and the inner rectangle of the output the box fills */
struct MotionItem { const uint8_t *src; uint8_t *dst; uint32_t wmb, hmb, x0, y0, w, h; int32_t bx, by; uint32_t bw, bh, left, top, iw, ih; };
struct MotionArgs { const MotionItem *items; uint32_t width, height, planes, sampler, units, per_picture; };

__device__ __forceinline__ float mo_component(int32_t q, uint32_t age, uint32_t per_picture)
{
    const float v = (float)q * 0.25f;
    return per_picture ? v / (float)max(age, 1u) : v;
}

/* grid (tiles, regions) x 256: a workgroup writes tiles of TAA_COLS x TAA_ROWS output pixels, one pixel per lane and all its
 * channels, as k_tensor_roi does; values outside the inner rectangle are 0.  The values (include/h264bsd_mi355x.h):
 * NEAREST in integers; AREA with the footprint's edges, the overlaps and the sums in double, so that what reaches the output is the
 * float64 mean rounded once (the per-block division of per_picture before it, the scaling of UNITS_OUTPUT after it, are fp32). */
template <int DT, int LAYOUT>
__global__ __launch_bounds__(256) void k_motion_roi(MotionArgs a)
{
    typedef typename ToElem<DT>::T E;
    const MotionItem it = a.items[blockIdx.y];
    const uint32_t W = a.width, H = a.height, tid = threadIdx.x;
    const uint32_t C = ((a.planes & MO_MV) ? 2u : 0u) + ((a.planes & MO_VALID) ? 1u : 0u) + ((a.planes & MO_AGE) ? 1u : 0u) + ((a.planes & MO_QP) ? 1u : 0u);
    const uint32_t nux = (W + TAA_COLS - 1u) / TAA_COLS, units = nux * ((H + TAA_ROWS - 1u) / TAA_ROWS);
    const uint32_t col = tid % TAA_COLS, row = tid / TAA_COLS;
    const size_t n_mbs = (size_t)it.wmb * it.hmb, plane = (size_t)W * H;
    const uint32_t *mvp = reinterpret_cast<const uint32_t *>(it.src);
    const uint16_t *quadp = reinterpret_cast<const uint16_t *>(it.src + n_mbs * MOTION_MV_BYTES);
    const uint16_t *mbp = reinterpret_cast<const uint16_t *>(it.src + n_mbs * (MOTION_MV_BYTES + MOTION_QUAD_BYTES));
    const float sx = a.units ? (float)it.iw / (float)it.bw : 1.0f, sy = a.units ? (float)it.ih / (float)it.bh : 1.0f;
    E *dst = reinterpret_cast<E *>(it.dst);
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t ox = (u % nux) * TAA_COLS + col, oy = (u / nux) * TAA_ROWS + row;
        if (ox >= W || oy >= H) continue;
        float val[5] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };          /* dx, dy, valid, age, qp */
        if (ox >= it.left && ox < it.left + it.iw && oy >= it.top && oy < it.top + it.ih) {
            const uint32_t i = ox - it.left, j = oy - it.top;
            if (a.sampler == MO_NEAREST) {
                const int px = it.bx + (int)(((2ull * i + 1ull) * it.bw) / (2ull * it.iw));
                const int py = it.by + (int)(((2ull * j + 1ull) * it.bh) / (2ull * it.ih));
                if (px >= 0 && px < (int)it.w && py >= 0 && py < (int)it.h) {
                    const uint32_t kx = (it.x0 + (uint32_t)px) >> 2, ky = (it.y0 + (uint32_t)py) >> 2;
                    const uint32_t mv = mvp[(size_t)ky * (4u * it.wmb) + kx];
                    const uint32_t q = quadp[(size_t)(ky >> 1) * (2u * it.wmb) + (kx >> 1)];
                    const uint32_t m = mbp[(size_t)(ky >> 2) * it.wmb + (kx >> 2)];
                    const uint32_t age = q & 255u;
                    val[0] = mo_component((int16_t)(mv & 0xFFFFu), age, a.per_picture);
                    val[1] = mo_component((int16_t)(mv >> 16), age, a.per_picture);
                    val[2] = (q & 256u) ? 1.0f : 0.0f;
                    val[3] = (float)age;
                    val[4] = (float)(m >> 8);
                }
            } else {
                /* the footprint in window coordinates, clipped to the window; then in frame coordinates */
                const double fx0 = (double)it.bx + (double)((unsigned long long)i * it.bw) / (double)it.iw;
                const double fx1 = (double)it.bx + (double)((unsigned long long)(i + 1u) * it.bw) / (double)it.iw;
                const double fy0 = (double)it.by + (double)((unsigned long long)j * it.bh) / (double)it.ih;
                const double fy1 = (double)it.by + (double)((unsigned long long)(j + 1u) * it.bh) / (double)it.ih;
                const double cx0 = fmax(fx0, 0.0) + it.x0, cx1 = fmin(fx1, (double)it.w) + it.x0;
                const double cy0 = fmax(fy0, 0.0) + it.y0, cy1 = fmin(fy1, (double)it.h) + it.y0;
                if (cx1 > cx0 && cy1 > cy0) {
                    const uint32_t kx0 = (uint32_t)cx0 >> 2, kx1 = min(((uint32_t)ceil(cx1) + 3u) >> 2, 4u * it.wmb);
                    const uint32_t ky0 = (uint32_t)cy0 >> 2, ky1 = min(((uint32_t)ceil(cy1) + 3u) >> 2, 4u * it.hmb);
                    double s_all = 0.0, s_valid = 0.0, s_dx = 0.0, s_dy = 0.0, s_age = 0.0, s_qp = 0.0;
                    for (uint32_t ky = ky0; ky < ky1; ky++) {
                        const double wy = fmin(cy1, 4.0 * ky + 4.0) - fmax(cy0, 4.0 * ky);
                        if (!(wy > 0.0)) continue;
                        for (uint32_t kx = kx0; kx < kx1; kx++) {
                            const double wx = fmin(cx1, 4.0 * kx + 4.0) - fmax(cx0, 4.0 * kx);
                            if (!(wx > 0.0)) continue;
                            const double wgt = wx * wy;
                            const uint32_t q = quadp[(size_t)(ky >> 1) * (2u * it.wmb) + (kx >> 1)];
                            const uint32_t m = mbp[(size_t)(ky >> 2) * it.wmb + (kx >> 2)];
                            s_all += wgt;
                            s_qp += wgt * (double)(m >> 8);
                            if (q & 256u) {
                                const uint32_t mv = mvp[(size_t)ky * (4u * it.wmb) + kx], age = q & 255u;
                                s_valid += wgt;
                                s_dx += wgt * (double)mo_component((int16_t)(mv & 0xFFFFu), age, a.per_picture);
                                s_dy += wgt * (double)mo_component((int16_t)(mv >> 16), age, a.per_picture);
                                s_age += wgt * (double)age;
                            }
                        }
                    }
                    if (s_valid > 0.0) {
                        val[0] = (float)(s_dx / s_valid);
                        val[1] = (float)(s_dy / s_valid);
                        val[3] = (float)(s_age / s_valid);
                    }
                    val[2] = (float)(s_valid / (((double)it.bw / (double)it.iw) * ((double)it.bh / (double)it.ih)));
                    if (s_all > 0.0) val[4] = (float)(s_qp / s_all);
                }
            }
            val[0] *= sx;
            val[1] *= sy;
        }
        const size_t pix = (size_t)oy * W + ox;
        uint32_t c = 0;
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const uint32_t bit = k < 2 ? MO_MV : k == 2 ? MO_VALID : k == 3 ? MO_AGE : MO_QP;
            if (!(a.planes & bit)) continue;
            const E e = to_enc<DT>(val[k]);
            if constexpr (LAYOUT == TO_NCHW) dst[c * plane + pix] = e;
            else dst[pix * C + c] = e;
            c++;
        }
    }
}

} // namespace h264k
