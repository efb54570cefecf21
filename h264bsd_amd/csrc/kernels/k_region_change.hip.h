/* kernels/k_region_change.hip.h — integer statistics of the DIFFERENCE between two pictures over boxes (h264bsdmiOutputRegionChange):
 * an instance's current picture against the picture it kept (k_keep.hip.h), both read from their macroblock tiles where they lie, at
 * the same tile offset.  Included by engine.hip after k_region_stats.hip.h, whose scheme and constants it uses, with the shared
 * pieces of region_common.hip.h; like them, not part of the kernel sources that key the committed counter tables (srchash.py).
 *
 * One record, C channels (1 or 3) and B bins (0, 16 .. 256), little endian, 8 + 32 C + 4 C B bytes; d = current - kept per sample:
 *     u32 count; u32 zero;  C x { u64 sad; u64 ssd; i64 sum; u32 max; u32 above; }  C x B x u32 hist      (hist of |d|)
 * grid (S row bands, regions) x 256.  A wavefront takes one macroblock of its band at a time and reads the 384-byte tile of BOTH frames
 * once: lane l the luma dword of row l >> 2, columns 4 (l & 3) .. + 3, and for the three-channel sources the two Cb and two Cr bytes
 * under those four samples; RGB is the reference conversion of each picture, then the difference.  Macroblocks inside box ∩ window
 * take a path without masks; in edge macroblocks a byte mask clears the masked bytes of BOTH pictures: their d is 0, which adds
 * nothing to any sum, is no maximum and is above no threshold; only the histogram has to leave them out by hand.
 * Per dword: |d| bytewise; sad = udot4(|d|, 0x01010101), ssd = udot4(|d|, |d|), the signed sum as udot4(current) - udot4(kept), max
 * and `above` per byte.  The 32-bit partial sums are folded into 64 bits every CHANGE_FOLD macroblocks.
 * The histogram is of |d|, and between two pictures of a static camera nearly every sample lands in bin 0: the flat-picture worst
 * case of k_region_stats' LDS histograms, all the time.  So bin 0 is not counted in LDS at all: the band that writes the record sets
 * hist[c][0] = count - (the other bins), which is exact, masked bytes being in neither.  With bin 0 gone ONE histogram per wavefront
 * does as well as k_region_stats' four lane-replicated copies on moving pictures and, at a quarter of the LDS, better on equal ones
 * (both measured, with and without bin 0 in LDS: docs/EXPERIMENTS.md, "Change statistics").
 * S == 1: the workgroup writes the record.  S > 1: partial records (the same layout, bin 0 still open) meet in the engine's scratch
 * behind region_hand_over: the band that draws the last ticket adds the S partials up, writes the record with plain vector stores
 * and zeroes the ticket.  All integers: the result does not depend on which band arrives last. */
#pragma once
namespace h264k {

/* macroblocks a lane adds up in 32 bits, the bound of STATS_FOLD: the largest partial is ssd, 8192 x 4 x 255^2 < 2^32 (sad and the two
 * sums of the signed sum stay below 8192 x 4 x 255; `above` counts samples, at most 2^28 per region, and is never folded) */
constexpr uint32_t CHANGE_FOLD = STATS_FOLD;
constexpr uint32_t CHANGE_MAX_RECORD = 8 + 32 * 3 + 4 * 3 * 256;

__host__ __device__ constexpr uint32_t change_record_bytes(uint32_t channels, uint32_t bins) { return 8u + 32u * channels + 4u * channels * bins; }

/* one region: the two frames, the record, and box ∩ window [x0, x1) x [y0, y1) in luma samples of the coded frame (x1 <= x0: empty) */
struct ChangeItem { const uint8_t *cur; const uint8_t *kept; uint8_t *dst; uint32_t wmb, x0, y0, x1, y1; };
/* partials, tickets: as StatsArgs (region r's partial records at (r S + band) stride); shift = 8 - log2 bins; thr: per channel */
struct ChangeArgs { const ChangeItem *items; uint8_t *partials; uint32_t *tickets; uint32_t bins, shift, thr[3]; };

/* per channel, what a lane carries between folds (32 bits) */
struct ChangeAcc { uint32_t sad, ssd, sc, sk; };

/* one macroblock of one wavefront.  m: 0xFF in the bytes that count; h: this wavefront's histogram (HIST), which has no bin 0 */
template <int SRC, bool HIST, bool INNER>
__device__ __forceinline__ void change_mb(const uint8_t *tc, const uint8_t *tk, uint32_t lane, uint32_t m, uint32_t *h, uint32_t B, uint32_t shift,
                                          const uint32_t *thr, ChangeAcc *acc, uint32_t *mx, uint32_t *above)
{
    constexpr int C = SRC == ST_Y ? 1 : 3;
    uint32_t a[C], b[C];
    region_load<SRC>(tc, lane, a);
    region_load<SRC>(tk, lane, b);
#pragma unroll
    for (int c = 0; c < C; c++) {
        const uint32_t av = INNER ? a[c] : a[c] & m, bv = INNER ? b[c] : b[c] & m;
        uint32_t ad = 0u;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int x = (int)((av >> (8 * k)) & 255u), y = (int)((bv >> (8 * k)) & 255u);
            const uint32_t d = (uint32_t)(x > y ? x - y : y - x);
            ad |= d << (8 * k);
            mx[c] = max(mx[c], d);
            above[c] += d > thr[c] ? 1u : 0u;
        }
        acc[c].sad = __builtin_amdgcn_udot4(ad, 0x01010101u, acc[c].sad, false);
        acc[c].ssd = __builtin_amdgcn_udot4(ad, ad, acc[c].ssd, false);
        acc[c].sc = __builtin_amdgcn_udot4(av, 0x01010101u, acc[c].sc, false);
        acc[c].sk = __builtin_amdgcn_udot4(bv, 0x01010101u, acc[c].sk, false);
        if constexpr (HIST) {
            uint32_t *hc = h + (uint32_t)c * B;
            if (INNER && SRC == ST_YCBCR && c > 0) {
                if (!(lane & 4u)) {                                        /* the even luma row of the pair that shares these two samples */
                    const uint32_t b0 = (ad & 255u) >> shift, b1 = (ad >> 24) >> shift;
                    if (b0) region_lds_add(hc + b0, 4u);
                    if (b1) region_lds_add(hc + b1, 4u);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint32_t bin = ((ad >> (8 * k)) & 255u) >> shift;
                    if ((INNER || ((m >> (8 * k)) & 1u)) && bin) region_lds_add(hc + bin, 1u);
                }
            }
        }
    }
}

template <int SRC, bool HIST>
__global__ __launch_bounds__(256) void k_region_change(ChangeArgs a)
{
    constexpr int C = SRC == ST_Y ? 1 : 3;
    constexpr uint32_t HCAP = C * 256u;                                     /* one histogram per wavefront */
    __shared__ uint32_t s_hist[HIST ? 4u * HCAP : 1u];
    __shared__ unsigned long long s_sum[4][C][3];
    __shared__ uint32_t s_mm[4][C][2];
    __shared__ uint32_t s_rest[3];                                          /* per channel: what the bins other than 0 hold */
    const ChangeItem it = a.items[blockIdx.y];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t B = a.bins, S = gridDim.x, band = blockIdx.x, stride = change_record_bytes(C, B);
    const uint32_t thr[3] = { a.thr[0], a.thr[1], a.thr[2] };
    if (tid < 3u) s_rest[tid] = 0u;
    if constexpr (HIST) {
        for (uint32_t i = tid; i < 4u * HCAP; i += 256u) s_hist[i] = 0u;
    }
    __syncthreads();
    const RegionBand bd = region_band(it.x0, it.y0, it.x1, it.y1, band, S);
    const bool empty = bd.empty;
    const uint32_t mbx0 = bd.mbx0, cols = bd.cols, r0 = bd.r0, n = (bd.r1 - r0) * cols;
    const uint32_t col4 = (lane & 3u) * 4u, row = lane >> 2;
    uint32_t *h = s_hist + (HIST ? wave * HCAP : 0u);

    unsigned long long sad[C], ssd[C];
    long long sum[C];
    uint32_t mx[C], above[C];
#pragma unroll
    for (int c = 0; c < C; c++) { sad[c] = ssd[c] = 0ull; sum[c] = 0ll; mx[c] = above[c] = 0u; }
    for (uint32_t base = wave; base < n; base += 4u * CHANGE_FOLD) {
        ChangeAcc acc[C];
#pragma unroll
        for (int c = 0; c < C; c++) acc[c] = ChangeAcc{ 0u, 0u, 0u, 0u };
        const uint32_t end = min(n, base + 4u * CHANGE_FOLD);
        for (uint32_t i = base; i < end; i += 4u) {
            const uint32_t mby = r0 + i / cols, mbx = mbx0 + i % cols;
            const size_t at = ((size_t)mby * it.wmb + mbx) * TILE;
            const uint32_t X = mbx * 16u, Y = mby * 16u;
            if (REGION_MB_INNER(X, Y, it)) {
                change_mb<SRC, HIST, true>(it.cur + at, it.kept + at, lane, 0xFFFFFFFFu, h, B, a.shift, thr, acc, mx, above);
            } else {
                const uint32_t m = region_mask(X + col4, Y + row, it.x0, it.y0, it.x1, it.y1);
                change_mb<SRC, HIST, false>(it.cur + at, it.kept + at, lane, m, h, B, a.shift, thr, acc, mx, above);
            }
        }
#pragma unroll
        for (int c = 0; c < C; c++) { sad[c] += acc[c].sad; ssd[c] += acc[c].ssd; sum[c] += (long long)acc[c].sc - (long long)acc[c].sk; }
    }

    /* once per workgroup: the wavefronts' sums through shuffles, then through LDS */
#pragma unroll
    for (int c = 0; c < C; c++) {
        const unsigned long long s = stats_wave_sum(sad[c]), q = stats_wave_sum(ssd[c]), g = (unsigned long long)stats_wave_sum(sum[c]);
        const uint32_t ab = stats_wave_sum(above[c]);
        uint32_t hi = mx[c];
#pragma unroll
        for (int d = 32; d; d >>= 1) hi = max(hi, (uint32_t)__shfl_xor((int)hi, d));
        if (lane == 0u) { s_sum[wave][c][0] = s; s_sum[wave][c][1] = q; s_sum[wave][c][2] = g; s_mm[wave][c][0] = hi; s_mm[wave][c][1] = ab; }
    }
    __syncthreads();
    const uint32_t count = empty ? 0u : (it.x1 - it.x0) * (it.y1 - it.y0);
    const uint32_t bmask = B ? B - 1u : 0u, blog = 8u - a.shift;             /* a bin's index and its channel from its place in the histograms */
    uint8_t *out = S == 1u ? it.dst : a.partials + ((size_t)blockIdx.y * S + band) * stride;
    uint32_t *out32 = reinterpret_cast<uint32_t *>(out);
    if (tid == 0u) { out32[0] = count; out32[1] = 0u; }
    if (tid < (uint32_t)C) {
        unsigned long long s = 0ull, q = 0ull, g = 0ull;
        uint32_t hi = 0u, ab = 0u;
        for (int w = 0; w < 4; w++) { s += s_sum[w][tid][0]; q += s_sum[w][tid][1]; g += s_sum[w][tid][2]; hi = max(hi, s_mm[w][tid][0]); ab += s_mm[w][tid][1]; }
        unsigned long long *m64 = reinterpret_cast<unsigned long long *>(out + 8u + 32u * tid);
        m64[0] = s; m64[1] = q; m64[2] = g;
        out32[2u + 8u * tid + 6u] = hi; out32[2u + 8u * tid + 7u] = ab;
    }
    if constexpr (HIST) {
        const bool closes = S == 1u;                                        /* this workgroup writes the record: bin 0 from the count */
        for (uint32_t i = tid; i < (uint32_t)C * B; i += 256u) {
            uint32_t t = 0u;
            for (uint32_t k = 0; k < 4u; k++) t += s_hist[k * HCAP + i];
            if (closes && !(i & bmask)) continue;
            out32[2u + 8u * C + i] = t;
            if (closes && t) region_lds_add(&s_rest[i >> blog], t);
        }
        if (closes) {
            __syncthreads();
            if (tid < (uint32_t)C) out32[2u + 8u * C + tid * B] = count - s_rest[tid];
        }
    }
    if (S == 1u) return;

    if (!region_hand_over(a.tickets, S)) return;
    const uint8_t *pp = a.partials + (size_t)blockIdx.y * S * stride;
    uint32_t *dst32 = reinterpret_cast<uint32_t *>(it.dst);
    if (tid == 0u) { dst32[0] = count; dst32[1] = 0u; }
    if (tid < (uint32_t)C) {
        unsigned long long s = 0ull, q = 0ull, g = 0ull;
        uint32_t hi = 0u, ab = 0u;
        for (uint32_t b = 0; b < S; b++) {
            const uint8_t *p = pp + (size_t)b * stride + 8u + 32u * tid;
            s += reinterpret_cast<const unsigned long long *>(p)[0];
            q += reinterpret_cast<const unsigned long long *>(p)[1];
            g += reinterpret_cast<const unsigned long long *>(p)[2];
            hi = max(hi, reinterpret_cast<const uint32_t *>(p)[6]);
            ab += reinterpret_cast<const uint32_t *>(p)[7];
        }
        unsigned long long *m64 = reinterpret_cast<unsigned long long *>(it.dst + 8u + 32u * tid);
        m64[0] = s; m64[1] = q; m64[2] = g;
        dst32[2u + 8u * tid + 6u] = hi; dst32[2u + 8u * tid + 7u] = ab;
    }
    if constexpr (HIST) {
        for (uint32_t i = tid; i < (uint32_t)C * B; i += 256u) {
            uint32_t t = 0u;
            for (uint32_t b = 0; b < S; b++) t += reinterpret_cast<const uint32_t *>(pp + (size_t)b * stride)[2u + 8u * C + i];
            if (!(i & bmask)) continue;
            dst32[2u + 8u * C + i] = t;
            if (t) region_lds_add(&s_rest[i >> blog], t);
        }
        __syncthreads();
        if (tid < (uint32_t)C) dst32[2u + 8u * C + tid * B] = count - s_rest[tid];
    }
    region_ticket_rezero(a.tickets);
}

} // namespace h264k
