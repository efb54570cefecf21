/* kernels/k_region_stats.hip.h — integer statistics of boxes of decoded pictures, read from the macroblock tiles where they lie
 * (h264bsdmiOutputRegionStats): per region the number of samples, and per channel their sum, sum of squares, minimum, maximum and
 * a histogram.  Included by engine.hip after region_common.hip.h, whose loader, masks, band geometry and hand-over it uses; like it,
 * not part of the kernel sources that key the committed counter tables (srchash.py).
 *
 * One record, C channels (1 or 3) and B bins (0, 16 .. 256), little endian, 8 + 24 C + 4 C B bytes:
 *     u32 count; u32 zero;  C x { u64 sum; u64 sumsq; u32 min; u32 max; }  C x B x u32 hist
 * grid (S row bands, regions) x 256.  A wavefront takes one macroblock of its band at a time and reads the 384-byte tile once:
 * lane l the luma dword of row l >> 2, columns 4 (l & 3) .. + 3, and for the three-channel sources the two Cb and two Cr bytes
 * under those four samples.  Macroblocks inside box ∩ window take a path without masks; edge macroblocks mask per sample (a byte
 * mask: a masked byte is 0 for the sums and the maximum, 255 for the minimum, and is not counted).  Moments stay in registers per
 * lane (32-bit partial sums folded into 64 bits every STATS_FOLD macroblocks) and are reduced once per workgroup; histograms are
 * wavefront-private in LDS (STATS_HIST_COPIES lane-replicated copies each), filled by LDS adds without return.
 * S == 1: the workgroup writes the record.  S > 1: every band writes a partial record (the same layout) to the engine's scratch;
 * behind region_hand_over the band that drew the last ticket adds the S partials up and writes the record with plain stores, then
 * zeroes the ticket for the next launch.  All integers: the result does not depend on which band arrives last. */
#pragma once
namespace h264k {

/* the two ways of taking pressure off one LDS bin, both on as measured (docs/EXPERIMENTS.md, "Region statistics"): copies of a
 * wavefront's histogram chosen by lane % STATS_HIST_COPIES, one bank apart (4 copies: 48 KB of LDS for three channels; a flat picture,
 * where all 64 lanes add to one bin, costs 3.0-3.8 times less than with one copy); and, in an interior macroblock, ONE add of 4 per
 * chroma sample (by the lane of its even luma row) instead of four adds of 1 */
#ifndef STATS_HIST_COPIES
#define STATS_HIST_COPIES 4
#endif
#ifndef STATS_CHROMA_MULT
#define STATS_CHROMA_MULT 1
#endif
constexpr uint32_t STATS_FOLD = 8192;      /* macroblocks a lane adds up in 32 bits: 8192 x 4 x 255^2 < 2^32 */
constexpr uint32_t STATS_MAX_PARTIALS = 1024, STATS_MAX_RECORD = 8 + 24 * 3 + 4 * 3 * 256;

__host__ __device__ constexpr uint32_t stats_record_bytes(uint32_t channels, uint32_t bins) { return 8u + 24u * channels + 4u * channels * bins; }

/* one region: the picture's frame, the record, and box ∩ window [x0, x1) x [y0, y1) in luma samples of the coded frame (x1 <= x0:
 * empty) */
struct StatsItem { const uint8_t *src; uint8_t *dst; uint32_t wmb, x0, y0, x1, y1; };
/* partials: STATS_MAX_PARTIALS records of `stride` bytes, region r's at (r S + band) stride; tickets: one word per region, zero
 * between launches; shift = 8 - log2 bins */
struct StatsArgs { const StatsItem *items; uint8_t *partials; uint32_t *tickets; uint32_t bins, shift; };

/* the four samples v (one per byte) of channel c of one lane; m: 0xFF in the bytes that count */
template <bool INNER>
__device__ __forceinline__ void stats_moments(uint32_t v, uint32_t m, uint32_t &s32, uint32_t &q32, uint32_t &mn, uint32_t &mx)
{
    const uint32_t vs = INNER ? v : v & m, lo = INNER ? v : v | ~m;
    s32 = __builtin_amdgcn_udot4(vs, 0x01010101u, s32, false);
    q32 = __builtin_amdgcn_udot4(vs, vs, q32, false);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        mn = min(mn, (lo >> (8 * k)) & 255u);
        mx = max(mx, (vs >> (8 * k)) & 255u);
    }
}

/* one macroblock of one wavefront.  h: this lane's histogram copy (HIST) */
template <int SRC, bool HIST, bool INNER>
__device__ __forceinline__ void stats_mb(const uint8_t *tile, uint32_t lane, uint32_t m, uint32_t *h, uint32_t B, uint32_t shift,
                                         uint32_t *s32, uint32_t *q32, uint32_t *mn, uint32_t *mx)
{
    constexpr int C = SRC == ST_Y ? 1 : 3;
    uint32_t v[C];
    region_load<SRC>(tile, lane, v);
#pragma unroll
    for (int c = 0; c < C; c++) {
        stats_moments<INNER>(v[c], m, s32[c], q32[c], mn[c], mx[c]);
        if constexpr (HIST) {
            uint32_t *hc = h + (uint32_t)c * B;
            if (STATS_CHROMA_MULT && INNER && SRC == ST_YCBCR && c > 0) {
                if (!(lane & 4u)) {                                        /* the even luma row of the pair that shares these two samples */
                    region_lds_add(hc + ((v[c] & 255u) >> shift), 4u);
                    region_lds_add(hc + ((v[c] >> 24) >> shift), 4u);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (INNER || ((m >> (8 * k)) & 1u)) region_lds_add(hc + (((v[c] >> (8 * k)) & 255u) >> shift), 1u);
            }
        }
    }
}

template <int SRC, bool HIST>
__global__ __launch_bounds__(256) void k_region_stats(StatsArgs a)
{
    constexpr int C = SRC == ST_Y ? 1 : 3, R = STATS_HIST_COPIES;
    constexpr uint32_t HCAP = C * 256u + 1u;                                /* a copy's stride: one bank on from its neighbour */
    __shared__ uint32_t s_hist[HIST ? 4u * R * HCAP : 1u];
    __shared__ unsigned long long s_sum[4][C][2];
    __shared__ uint32_t s_mm[4][C][2];
    const StatsItem it = a.items[blockIdx.y];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t B = a.bins, S = gridDim.x, band = blockIdx.x, stride = stats_record_bytes(C, B);
    if constexpr (HIST) {
        for (uint32_t i = tid; i < 4u * R * HCAP; i += 256u) s_hist[i] = 0u;
        __syncthreads();
    }
    const RegionBand bd = region_band(it.x0, it.y0, it.x1, it.y1, band, S);
    const bool empty = bd.empty;
    const uint32_t mbx0 = bd.mbx0, cols = bd.cols, r0 = bd.r0, n = (bd.r1 - r0) * cols;
    const uint32_t col4 = (lane & 3u) * 4u, row = lane >> 2;
    uint32_t *h = s_hist + (HIST ? (wave * R + lane % R) * HCAP : 0u);

    unsigned long long sum[C], sq[C];
    uint32_t mn[C], mx[C];
#pragma unroll
    for (int c = 0; c < C; c++) { sum[c] = sq[c] = 0ull; mn[c] = 255u; mx[c] = 0u; }
    for (uint32_t base = wave; base < n; base += 4u * STATS_FOLD) {
        uint32_t s32[C], q32[C];
#pragma unroll
        for (int c = 0; c < C; c++) s32[c] = q32[c] = 0u;
        const uint32_t end = min(n, base + 4u * STATS_FOLD);
        for (uint32_t i = base; i < end; i += 4u) {
            const uint32_t mby = r0 + i / cols, mbx = mbx0 + i % cols;
            const uint8_t *tile = it.src + ((size_t)mby * it.wmb + mbx) * TILE;
            const uint32_t X = mbx * 16u, Y = mby * 16u;
            if (REGION_MB_INNER(X, Y, it)) {
                stats_mb<SRC, HIST, true>(tile, lane, 0xFFFFFFFFu, h, B, a.shift, s32, q32, mn, mx);
            } else {
                const uint32_t m = region_mask(X + col4, Y + row, it.x0, it.y0, it.x1, it.y1);
                stats_mb<SRC, HIST, false>(tile, lane, m, h, B, a.shift, s32, q32, mn, mx);
            }
        }
#pragma unroll
        for (int c = 0; c < C; c++) { sum[c] += s32[c]; sq[c] += q32[c]; }
    }

    /* once per workgroup: the wavefronts' moments through shuffles, then through LDS */
#pragma unroll
    for (int c = 0; c < C; c++) {
        const unsigned long long s = stats_wave_sum(sum[c]), q = stats_wave_sum(sq[c]);
        uint32_t lo = mn[c], hi = mx[c];
#pragma unroll
        for (int d = 32; d; d >>= 1) { lo = min(lo, (uint32_t)__shfl_xor((int)lo, d)); hi = max(hi, (uint32_t)__shfl_xor((int)hi, d)); }
        if (lane == 0u) { s_sum[wave][c][0] = s; s_sum[wave][c][1] = q; s_mm[wave][c][0] = lo; s_mm[wave][c][1] = hi; }
    }
    __syncthreads();
    const uint32_t count = empty ? 0u : (it.x1 - it.x0) * (it.y1 - it.y0);
    uint8_t *out = S == 1u ? it.dst : a.partials + ((size_t)blockIdx.y * S + band) * stride;
    uint32_t *out32 = reinterpret_cast<uint32_t *>(out);
    if (tid == 0u) { out32[0] = count; out32[1] = 0u; }
    if (tid < (uint32_t)C) {
        unsigned long long s = 0ull, q = 0ull;
        uint32_t lo = 255u, hi = 0u;
        for (int w = 0; w < 4; w++) { s += s_sum[w][tid][0]; q += s_sum[w][tid][1]; lo = min(lo, s_mm[w][tid][0]); hi = max(hi, s_mm[w][tid][1]); }
        unsigned long long *m64 = reinterpret_cast<unsigned long long *>(out + 8u + 24u * tid);
        m64[0] = s; m64[1] = q;
        out32[2u + 6u * tid + 4u] = lo; out32[2u + 6u * tid + 5u] = hi;
    }
    if constexpr (HIST) {
        for (uint32_t i = tid; i < (uint32_t)C * B; i += 256u) {
            uint32_t t = 0u;
            for (uint32_t k = 0; k < 4u * R; k++) t += s_hist[k * HCAP + i];
            out32[2u + 6u * C + i] = t;
        }
    }
    if (S == 1u) return;

    if (!region_hand_over(a.tickets, S)) return;
    const uint8_t *pp = a.partials + (size_t)blockIdx.y * S * stride;
    uint32_t *dst32 = reinterpret_cast<uint32_t *>(it.dst);
    if (tid == 0u) { dst32[0] = count; dst32[1] = 0u; }
    if (tid < (uint32_t)C) {
        unsigned long long s = 0ull, q = 0ull;
        uint32_t lo = 255u, hi = 0u;
        for (uint32_t b = 0; b < S; b++) {
            const uint8_t *p = pp + (size_t)b * stride + 8u + 24u * tid;
            s += reinterpret_cast<const unsigned long long *>(p)[0];
            q += reinterpret_cast<const unsigned long long *>(p)[1];
            lo = min(lo, reinterpret_cast<const uint32_t *>(p)[4]);
            hi = max(hi, reinterpret_cast<const uint32_t *>(p)[5]);
        }
        unsigned long long *m64 = reinterpret_cast<unsigned long long *>(it.dst + 8u + 24u * tid);
        m64[0] = s; m64[1] = q;
        dst32[2u + 6u * tid + 4u] = lo; dst32[2u + 6u * tid + 5u] = hi;
    }
    if constexpr (HIST) {
        for (uint32_t i = tid; i < (uint32_t)C * B; i += 256u) {
            uint32_t t = 0u;
            for (uint32_t b = 0; b < S; b++) t += reinterpret_cast<const uint32_t *>(pp + (size_t)b * stride)[2u + 6u * C + i];
            dst32[2u + 6u * C + i] = t;
        }
    }
    region_ticket_rezero(a.tickets);
}

} // namespace h264k
