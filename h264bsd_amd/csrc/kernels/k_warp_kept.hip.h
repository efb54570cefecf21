/* kernels/k_warp_kept.hip.h — the kept pictures of many instances RESAMPLED through an affine map, hi and lo
 * (h264bsdmiWarpKeptPictures): the background model registered on the current picture.  Included by engine.hip behind k_blend.hip.h;
 * like its siblings, not part of the kernel sources that key the committed counter tables (srchash.py).
 *
 * The map goes from OUTPUT to SOURCE: six int32 coefficients a b c d e f in 16.16 fixed point, in luma samples of the window.  For the
 * output luma sample (x, y) of a window w x h, in 64-bit integers,
 *     X = a x + b y + c, Y = d x + e y + f;   outside = X or Y beyond [0, (size - 1) << 16];   both clamped to that range
 *     x0 = X >> 16, x1 = min(x0 + 1, w - 1), fx = (X >> 8) & 255, and y likewise
 *     V = (S00 (256 - fx) + S01 fx)(256 - fy) + (S10 (256 - fx) + S11 fx) fy;   S' = (V + 32768) >> 16
 * with S = 256 hi + lo the state of k_blend (lo reads as 128 where the instance's lo is not valid).  S <= 65535 keeps V + 32768 below
 * 2^32: the blend is done in an unsigned 32-bit lane.  A chroma sample (cx, cy) sits at luma (2 cx + 1/2, 2 cy + 1/2): in units of
 * 2^-18 chroma sample U = 2 (a 2cx + b 2cy + c) + a + b - 65536 (and V' with d e f), clamped to the chroma window, index U >> 18,
 * weight (U >> 10) & 255, outside decided on U, V' themselves.  Under WARP_OUT_CURRENT an output sample whose source was outside takes
 * T = 256 c + 128 of the current picture's sample at the OUTPUT position (what a starting blend writes).  Samples of the coded frame
 * outside the window keep their state.  All of it is integer and exact; no result depends on scheduling.
 *
 * k_warp_kept, grid (blocks, items) x 256: ONE launch for the batch, from the live buffers into the instance's spare ones, of which
 * EVERY byte is written (the host swaps them afterwards).  A workgroup owns a block of 4 macroblocks of a row, 64 x 16 luma: a lane the
 * 4 adjacent samples of a tile row — a wavefront stores the 256 luma bytes of a macroblock as consecutive dwords — and lanes 0 .. 127
 * after that 4 adjacent chroma samples, Cb in the first wavefront, Cr in the second: the 64 bytes of a chroma block as consecutive
 * dwords.  The four neighbours of a sample are GATHERED from the tiles, two byte loads each (hi and lo).  A variant that first staged
 * the exact source box of a block in LDS as 16-bit rows, for the near-identity maps of stabilisation, gave the same bytes and was
 * measurably SLOWER at exactly those maps (docs/EXPERIMENTS.md, "Warped kept pictures"): it is not here.
 * The luma samples of the window whose source was outside are counted per lane, summed per workgroup (wavefront sum, LDS) and added
 * with one integer atomic per workgroup to count[slot], which the host zeroes on the stream ahead of the launch. */
#pragma once
namespace h264k {

constexpr uint32_t WARP_MAX_BLOCKS = 1024;      /* workgroups per item */
enum { WARP_OUT_REPLICATE = 0u, WARP_OUT_CURRENT = 1u };
/* cur: the current picture's frame (WARP_OUT_CURRENT only); hi, lo: the live state (lo NULL: not valid, 128 everywhere); hi_out,
 * lo_out: the spares (lo_out NULL exactly when lo is); the window x0 y0 w h in luma samples of the coded frame, all even; m: a .. f;
 * slot: the instance's word of WarpArgs.count */
struct WarpItem {
    const uint8_t *cur; const uint8_t *hi; const uint8_t *lo; uint8_t *hi_out; uint8_t *lo_out;
    uint32_t wmb, hmb, x0, y0, w, h, slot; int32_t m[6];
};
struct WarpArgs { const WarpItem *items; uint32_t *count; uint32_t outside; };

/* one coordinate in units of 2^-bits sample on an axis of `size` samples: the two indices, the weight, and whether it was outside */
struct WarpAxis { uint32_t i0, i1, f; bool out; };
__device__ __forceinline__ long long warp_clamp(long long X, uint32_t size, int bits)
{
    const long long top = (long long)(size - 1u) << bits;
    return X < 0 ? 0 : X > top ? top : X;
}
__device__ __forceinline__ WarpAxis warp_axis(long long X, uint32_t size, int bits)
{
    WarpAxis r;
    const long long C = warp_clamp(X, size, bits);
    r.out = C != X;
    r.i0 = (uint32_t)(C >> bits);
    r.i1 = min(r.i0 + 1u, size - 1u);
    r.f = (uint32_t)(C >> (bits - 8)) & 255u;
    return r;
}
__device__ __forceinline__ uint32_t warp_mix(uint32_t s00, uint32_t s01, uint32_t s10, uint32_t s11, uint32_t fx, uint32_t fy)
{
    const uint32_t V = (s00 * (256u - fx) + s01 * fx) * (256u - fy) + (s10 * (256u - fx) + s11 * fx) * fy;
    return (V + 32768u) >> 16;
}
/* the state at byte `at` of the frame */
__device__ __forceinline__ uint32_t warp_state(const WarpItem &it, size_t at)
{
    return ((uint32_t)it.hi[at] << 8) | (it.lo ? (uint32_t)it.lo[at] : 128u);
}

__global__ __launch_bounds__(256) void k_warp_kept(const WarpArgs a)
{
    __shared__ uint32_t s_count;
    const WarpItem it = a.items[blockIdx.y];
    const uint32_t tid = threadIdx.x;
    const uint32_t bcols = (it.wmb + 3u) >> 2, nblk = bcols * it.hmb;
    const uint32_t cx0 = it.x0 >> 1, cy0 = it.y0 >> 1, cw = it.w >> 1, ch = it.h >> 1;
    const bool current = a.outside == WARP_OUT_CURRENT;
    const long long A = it.m[0], B = it.m[1], C = it.m[2], D = it.m[3], E = it.m[4], F = it.m[5];
    /* chroma: U = 4 A cx + 4 B cy + CU, V' = 4 D cx + 4 E cy + FU */
    const long long CU = 2 * C + A + B - 65536, FU = 2 * F + D + E - 65536;
    uint32_t count = 0u;
    for (uint32_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const uint32_t mby = blk / bcols, mbx0 = (blk % bcols) * 4u;
        /* ---- luma: macroblock tid >> 6 of the block, row (tid >> 2) & 15, columns 4 (tid & 3) .. + 3 */
        const uint32_t mbx = mbx0 + (tid >> 6);
        if (mbx < it.wmb) {
            const uint32_t py = mby * 16u + ((tid >> 2) & 15u), px = mbx * 16u + (tid & 3u) * 4u;
            const size_t at = luma_at((int)it.wmb, (int)px, (int)py);
            const bool row_in = py >= it.y0 && py < it.y0 + it.h;
            const long long yr = (long long)py - it.y0;
            uint32_t hv = 0u, lv = 0u;
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) {
                const uint32_t x = px + j;
                uint32_t S;
                if (row_in && x >= it.x0 && x < it.x0 + it.w) {
                    const long long xr = (long long)x - it.x0;
                    const WarpAxis ax = warp_axis(A * xr + B * yr + C, it.w, 16), ay = warp_axis(D * xr + E * yr + F, it.h, 16);
                    const bool out = ax.out || ay.out;
                    count += out ? 1u : 0u;
                    if (out && current) S = ((uint32_t)it.cur[at + j] << 8) | 128u;
                    else {
                        const int gx0 = (int)(it.x0 + ax.i0), gx1 = (int)(it.x0 + ax.i1), gy0 = (int)(it.y0 + ay.i0), gy1 = (int)(it.y0 + ay.i1);
                        S = warp_mix(warp_state(it, luma_at((int)it.wmb, gx0, gy0)), warp_state(it, luma_at((int)it.wmb, gx1, gy0)),
                                     warp_state(it, luma_at((int)it.wmb, gx0, gy1)), warp_state(it, luma_at((int)it.wmb, gx1, gy1)), ax.f, ay.f);
                    }
                } else S = warp_state(it, at + j);
                hv |= (S >> 8) << (8u * j);
                lv |= (S & 255u) << (8u * j);
            }
            *reinterpret_cast<uint32_t *>(it.hi_out + at) = hv;
            if (it.lo_out) *reinterpret_cast<uint32_t *>(it.lo_out + at) = lv;
        }
        /* ---- chroma: plane tid >> 6, macroblock (tid >> 4) & 3, row (tid >> 1) & 7, columns 4 (tid & 1) .. + 3 */
        const uint32_t cmbx = mbx0 + ((tid >> 4) & 3u);
        if (tid < 128u && cmbx < it.wmb) {
            const uint32_t plane = tid >> 6;
            const uint32_t py = mby * 8u + ((tid >> 1) & 7u), px = cmbx * 8u + (tid & 1u) * 4u;
            const size_t at = chroma_at((int)it.wmb, (int)plane, (int)px, (int)py);
            const bool row_in = py >= cy0 && py < cy0 + ch;
            const long long yr = (long long)py - cy0;
            uint32_t hv = 0u, lv = 0u;
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) {
                const uint32_t x = px + j;
                uint32_t S;
                if (row_in && x >= cx0 && x < cx0 + cw) {
                    const long long xr = (long long)x - cx0;
                    const WarpAxis ax = warp_axis(4 * A * xr + 4 * B * yr + CU, cw, 18), ay = warp_axis(4 * D * xr + 4 * E * yr + FU, ch, 18);
                    if ((ax.out || ay.out) && current) S = ((uint32_t)it.cur[at + j] << 8) | 128u;
                    else {
                        const int gx0 = (int)(cx0 + ax.i0), gx1 = (int)(cx0 + ax.i1), gy0 = (int)(cy0 + ay.i0), gy1 = (int)(cy0 + ay.i1);
                        S = warp_mix(warp_state(it, chroma_at((int)it.wmb, (int)plane, gx0, gy0)), warp_state(it, chroma_at((int)it.wmb, (int)plane, gx1, gy0)),
                                     warp_state(it, chroma_at((int)it.wmb, (int)plane, gx0, gy1)), warp_state(it, chroma_at((int)it.wmb, (int)plane, gx1, gy1)),
                                     ax.f, ay.f);
                    }
                } else S = warp_state(it, at + j);
                hv |= (S >> 8) << (8u * j);
                lv |= (S & 255u) << (8u * j);
            }
            *reinterpret_cast<uint32_t *>(it.hi_out + at) = hv;
            if (it.lo_out) *reinterpret_cast<uint32_t *>(it.lo_out + at) = lv;
        }
    }
    if (a.count) {                                      /* (the same for every lane of the launch) */
        if (tid == 0u) s_count = 0u;
        __syncthreads();
        count = stats_wave_sum(count);
        if ((tid & 63u) == 0u && count) region_lds_add(&s_count, count);
        __syncthreads();
        if (tid == 0u && s_count) (void)atomicAdd(&a.count[it.slot], s_count);
    }
}

} // namespace h264k
