/* kernels/k_corner_points.hip.h — WHICH boxes are worth following: Shi-Tomasi / Harris corner points of boxes of CURRENT pictures
 * (h264bsdmiOutputCornerPoints), luma only, read from the macroblock tiles where they lie.  Included by engine.hip after
 * k_region_shift.hip.h; luma_stage (luma_search.hip.h) stages the luma; the band / ticket scheme and the wave sums are region_common.hip.h's; like
 * them, not part of the kernel sources that key the committed counter tables (srchash.py).
 *
 * The quantity (include/h264bsd_mi355x.h has it in full), all integers, T = box ∩ window:
 *     L~        the luma replicated at the border of the WINDOW (the clamp of luma_stage), the only border rule
 *     gx, gy    the 3 x 3 Sobel gradients of L~, |g| <= 1020
 *     A, B, C   the sums of gx gx, gy gy, gx gy over the b x b samples around a sample, b = 3 or 5: below 2^25
 *     S         MIN_EIGEN: A + B - isqrt((A - B)^2 + 4 C^2), in [0, 2^26)       HARRIS: 16 (A B - C C) - (A + B)^2, |S| < 2^54
 *     candidate a window sample p with S(p) > min_score that no other window sample q within Chebyshev distance nms beats:
 *               S(q) > S(p), or S(q) == S(p) and q earlier in raster order
 *     record    u32 count, found, written, 0; u64 energy (the sum of gx gx + gy gy over T), 0; K x { i32 x, y; i64 score }: the
 *               candidates in T by (score descending, y, x ascending), the first K; 32 + 16 K bytes, written whole
 * grid (S row bands, regions) x 256.  A band walks its rows of T in tiles of at most CORNER_ROWS x COLS samples, by the same
 * workgroup.  Per tile, with h = nms and hb = b / 2, five steps through LDS, a barrier between them:
 *     luma      (th + 2 (h + hb + 1)) rows of dwords, staged once by luma_stage
 *     gradient  gx, gy as the two 16-bit halves of a dword, one sample less on every side; a thread makes four in a row from two
 *               dwords of each of three rows
 *     score     (th + 2 h) x (tw + 2 h); a thread makes four in a row from the sums down 4 + 2 hb columns of the b rows (18 reads for
 *               four samples at b = 3, 40 at b = 5), and adds the energy of those that lie in T.  Samples outside the window, and
 *               negative Harris scores, are stored as 0: a candidate has S > min_score >= 0, so neither ever beats one, which is all
 *               the suppression asks of them.  MIN_EIGEN scores are u32, Harris scores u64: the kernel is a template on the score (and
 *               on b, for the unrolled sums), and the 64-bit one takes tiles half as wide (COLS 32 instead of 64)
 *     row max   the maximum of the score over the 2 h + 1 samples of a row around a sample; it lies where the luma and the gradients
 *               lay, which are dead by then
 *     NMS       p survives iff S(p) > every score EARLIER in raster order within nms (the rows above through the row maxima, the
 *               h samples left of it) and S(p) >= every LATER one: the order of (score, raster position) without a position in the
 *               key.  Survivors are appended to the workgroup's list in LDS (an LDS counter deals the slots: their order in the list
 *               is arbitrary, and the ranking does not see it)
 *     ranking   by counting: every entry's rank is the number of entries that beat it under (score descending, y, x ascending), a
 *               strict total order, so the ranks are a permutation and the first K of it the best K, sorted.  The list holds
 *               CORNER_LIST = 768 entries and is ranked, and cut to K, only when the next tile might not fit behind it — a tile
 *               brings at most CORNER_ROWS COLS / 4 candidates, which are never adjacent (nms >= 1) — and once at the end
 * Bands recompute their own halos; nothing passes between them but the partials.  S == 1: the workgroup closes the record.  S > 1:
 * every band writes its found, its energy and its best K (at most CORNER_PARTIAL bytes) to the engine's scratch under
 * region_hand_over; the band that draws the last ticket ranks the S lists into one, band after band, and closes the record.  The
 * best K of a union under a strict total order is unique, and the sums are integers: the result does not depend on which band
 * arrives last.  No global atomic decides anything but who closes.
 * Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), MIN_EIGEN b = 3 / 5, HARRIS b = 3 / 5: 62 / 74
 * and 54 / 68 VGPRs, no scratch memory, no spills; static LDS 44,376 bytes (MIN_EIGEN) and 38,888 bytes (HARRIS): three and four
 * workgroups of 256 to a compute unit, 3 and 4 wavefronts per SIMD.  Measurements: docs/EXPERIMENTS.md, "Corner points". */
#pragma once
namespace h264k {

constexpr uint32_t CORNER_ROWS = 32;                                /* a tile of candidates: rows */
constexpr uint32_t CORNER_MAX_NMS = 7, CORNER_MAX_HB = 2, CORNER_MAX_K = 256;
constexpr uint32_t CORNER_LIST = 768;                               /* the best K and a tile's candidates behind them: 3 entries a thread */
constexpr uint32_t CORNER_PARTIAL = 32u + 16u * CORNER_MAX_K;       /* a band's partial: a header and its best K, bytes */
enum { CORNER_MIN_EIGEN = 0, CORNER_HARRIS = 1 };

__host__ __device__ constexpr uint32_t corner_record_bytes(uint32_t max_points) { return 32u + 16u * max_points; }

/* one region: the frame, the record, box ∩ window [x0, x1) x [y0, y1) and the window [wx0, wx1) x [wy0, wy1) itself, all in luma
 * samples of the coded frame (x1 <= x0: empty) */
struct CornerItem { const uint8_t *frame; uint8_t *dst; uint32_t wmb, x0, y0, x1, y1, wx0, wy0, wx1, wy1; };
/* partials: region r's band b at (r S + b) CORNER_PARTIAL bytes; tickets: as StatsArgs */
struct CornerArgs { const CornerItem *items; uint8_t *partials; uint32_t *tickets; uint32_t nms, max_points; unsigned long long min_score; };

/* entry a beats entry b: the order of the record */
__device__ __forceinline__ bool corner_beats(unsigned long long sa, uint32_t pa, unsigned long long sb, uint32_t pb)
{
    return sa > sb || (sa == sb && pa < pb);
}

/* the first `total` entries of the list (score, position y << 16 | x) ranked by counting; the best min(total, K) of them are the list
 * afterwards, in order.  Called by the whole workgroup behind a barrier; ends with one */
__device__ __forceinline__ uint32_t corner_rank(unsigned long long *ls, uint32_t *lp, uint32_t total, uint32_t K, uint32_t tid)
{
    unsigned long long sc[CORNER_LIST / 256u];
    uint32_t ps[CORNER_LIST / 256u], rk[CORNER_LIST / 256u];
#pragma unroll
    for (uint32_t e = 0; e < CORNER_LIST / 256u; e++) {
        const uint32_t i = tid + 256u * e;
        rk[e] = 0xFFFFFFFFu;
        if (i < total) {
            sc[e] = ls[i]; ps[e] = lp[i];
            uint32_t r = 0u;
            for (uint32_t j = 0; j < total; j++) r += corner_beats(ls[j], lp[j], sc[e], ps[e]) ? 1u : 0u;
            rk[e] = r;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t e = 0; e < CORNER_LIST / 256u; e++)
        if (rk[e] < K) { ls[rk[e]] = sc[e]; lp[rk[e]] = ps[e]; }
    __syncthreads();
    return min(total, K);
}

/* the exact floor square root of v < 2^52: the double is exact, its root within a unit of the true one, and the integer steps take what
 * is left; r r is carried along, so a step is additions only */
__device__ __forceinline__ uint32_t corner_isqrt(unsigned long long v)
{
    uint32_t r = (uint32_t)__builtin_sqrt((double)v);
    unsigned long long r2 = (unsigned long long)r * r;
    while (r2 > v) { r2 -= 2ull * r - 1ull; r--; }
    while (r2 + 2ull * r + 1ull <= v) { r2 += 2ull * r + 1ull; r++; }
    return r;
}

template <int SCORE, int BLOCK>
__global__ __launch_bounds__(256) void k_corner_points(CornerArgs a)
{
    using score_t = typename std::conditional<SCORE == CORNER_HARRIS, unsigned long long, uint32_t>::type;
    constexpr uint32_t COLS = SCORE == CORNER_HARRIS ? 32u : 64u, HB = BLOCK / 2, NC = 4u + 2u * HB;
    constexpr uint32_t MAX_HALO = CORNER_MAX_NMS + CORNER_MAX_HB + 1u;
    constexpr uint32_t LP = (COLS + 2u * MAX_HALO + 3u) / 4u;                       /* pitches: luma (dwords), gradient, score */
    constexpr uint32_t GP = COLS + 2u * (MAX_HALO - 1u), SP = COLS + 2u * CORNER_MAX_NMS;
    constexpr uint32_t L_WORDS = (CORNER_ROWS + 2u * MAX_HALO) * LP, G_WORDS = (CORNER_ROWS + 2u * (MAX_HALO - 1u)) * GP;
    constexpr uint32_t R_WORDS = (CORNER_ROWS + 2u * CORNER_MAX_NMS) * COLS * (sizeof(score_t) / 4u);
    constexpr uint32_t TILE_MAX = CORNER_ROWS * COLS / 4u;                          /* the candidates of one tile at most */
    static_assert(TILE_MAX + CORNER_MAX_K <= CORNER_LIST, "a tile's candidates and the best K fit the list");
    static_assert(R_WORDS <= L_WORDS + G_WORDS, "the row maxima lie where the luma and the gradients lay");
    /* the luma and the gradients are dead once the scores stand: the row maxima take their place */
    __shared__ unsigned long long s_lgr[(L_WORDS + G_WORDS + 1u) / 2u];
    __shared__ score_t s_s[(CORNER_ROWS + 2u * CORNER_MAX_NMS) * SP];
    __shared__ unsigned long long s_ls[CORNER_LIST];
    __shared__ uint32_t s_lp[CORNER_LIST];
    __shared__ uint32_t s_n;
    __shared__ unsigned long long s_en[4];
    uint32_t *const s_l = reinterpret_cast<uint32_t *>(s_lgr), *const s_g = s_l + L_WORDS;
    score_t *const s_r = reinterpret_cast<score_t *>(s_lgr);
    const CornerItem it = a.items[blockIdx.y];
    const LumaWindow win{ it.wmb, it.wx0, it.wy0, it.wx1, it.wy1 };
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t h = a.nms, halo = h + HB + 1u, K = a.max_points;
    const uint32_t S = gridDim.x, band = blockIdx.x;
    const unsigned long long min_score = a.min_score;
    uint32_t nbest = 0u, found = 0u;                                        /* entries of the list; nbest > K only while unranked */
    bool ranked = true;
    unsigned long long energy = 0ull;
    if (tid == 0u) s_n = 0u;

    const RegionBand bd = region_band(it.x0, it.y0, it.x1, it.y1, band, S);
    const uint32_t ya = max(it.y0, bd.r0 * 16u), yb = bd.empty ? ya : min(it.y1, bd.r1 * 16u);       /* this band's rows of T */
    for (uint32_t ys = ya; ys < yb; ys += CORNER_ROWS) {
        const uint32_t th = min(CORNER_ROWS, yb - ys);
        for (uint32_t xs = it.x0; xs < it.x1; xs += COLS) {
            const uint32_t tw = min(COLS, it.x1 - xs);
            const uint32_t lw = tw + 2u * halo, lh = th + 2u * halo, gw = lw - 2u, gh = lh - 2u, sw = tw + 2u * h, sh = th + 2u * h;
            const uint32_t lq = (lw + 3u) >> 2, gq = (gw + 3u) >> 2, sq = (sw + 3u) >> 2;
            __syncthreads();                                                /* the tile before has been read */
            luma_stage(it.frame, win, (int)xs - (int)halo, (int)ys - (int)halo, lq, lh, s_l, LP, tid);
            __syncthreads();
            /* gradient (i, j) is at luma (i + 1, j + 1); four in a row from two dwords of each of three rows */
            for (uint32_t idx = tid; idx < gh * gq; idx += 256u) {
                const uint32_t i = idx / gq, q = idx - i * gq;
                int cs[6], d[6];                                            /* per column: the 1 2 1 sum down the rows; bottom - top */
                {
                    unsigned long long v[3];
#pragma unroll
                    for (uint32_t r = 0; r < 3u; r++)
                        v[r] = (unsigned long long)s_l[(i + r) * LP + min(q + 1u, lq - 1u)] << 32 | s_l[(i + r) * LP + q];
#pragma unroll
                    for (uint32_t c = 0; c < 6u; c++) {
                        const int p0 = (int)((v[0] >> (8u * c)) & 255u), p1 = (int)((v[1] >> (8u * c)) & 255u), p2 = (int)((v[2] >> (8u * c)) & 255u);
                        cs[c] = p0 + 2 * p1 + p2; d[c] = p2 - p0;
                    }
                }
#pragma unroll
                for (uint32_t k = 0; k < 4u; k++) {
                    const int gx = cs[k + 2u] - cs[k], gy = d[k] + 2 * d[k + 1u] + d[k + 2u];
                    if (4u * q + k < gw) s_g[i * GP + 4u * q + k] = ((uint32_t)gx & 0xFFFFu) | ((uint32_t)gy << 16);
                }
            }
            __syncthreads();
            /* score (i, j) is the sample (xs - h + j, ys - h + i), at gradient (i + HB, j + HB): four in a row from the sums down
             * 4 + 2 HB columns of the b rows.  The samples of T among them: the energy */
            uint32_t e32 = 0u;                                              /* at most 16 samples a thread and tile: below 2^26 */
            for (uint32_t idx = tid; idx < sh * sq; idx += 256u) {
                const uint32_t i = idx / sq, j0 = 4u * (idx - i * sq);
                uint32_t ca[NC] = {}, cb[NC] = {};
                int cc[NC] = {};
#pragma unroll
                for (uint32_t r = 0; r < (uint32_t)BLOCK; r++)
#pragma unroll
                    for (uint32_t c = 0; c < NC; c++) {
                        const uint32_t g = s_g[(i + r) * GP + min(j0 + c, gw - 1u)];
                        const int gx = (int)(short)(g & 0xFFFFu), gy = (int)g >> 16;
                        ca[c] += (uint32_t)(gx * gx); cb[c] += (uint32_t)(gy * gy); cc[c] += gx * gy;
                    }
                const int Y = (int)ys - (int)h + (int)i;
#pragma unroll
                for (uint32_t k = 0; k < 4u; k++) {
                    const uint32_t j = j0 + k;
                    if (j >= sw) continue;
                    const int X = (int)xs - (int)h + (int)j;
                    score_t sc = 0;
                    if (X >= (int)it.wx0 && X < (int)it.wx1 && Y >= (int)it.wy0 && Y < (int)it.wy1) {
                        uint32_t A = 0u, B = 0u;
                        int C = 0;
#pragma unroll
                        for (uint32_t c = k; c < k + (uint32_t)BLOCK; c++) { A += ca[c]; B += cb[c]; C += cc[c]; }
                        if constexpr (SCORE == CORNER_HARRIS) {
                            const long long t = (long long)A + B;
                            const long long v = 16ll * ((long long)A * B - (long long)C * C) - t * t;
                            sc = v > 0 ? (unsigned long long)v : 0ull;
                        } else {
                            const int dd = (int)A - (int)B;                 /* 32 x 32 -> 64 bit products */
                            sc = A + B - corner_isqrt((unsigned long long)((long long)dd * dd) + 4ull * (unsigned long long)((long long)C * C));
                        }
                    }
                    s_s[i * SP + j] = sc;
                    if (i >= h && i < h + th && j >= h && j < h + tw) {
                        const uint32_t g = s_g[(i + HB) * GP + j + HB];
                        const int gx = (int)(short)(g & 0xFFFFu), gy = (int)g >> 16;
                        e32 += (uint32_t)(gx * gx + gy * gy);
                    }
                }
            }
            energy += e32;
            __syncthreads();
            /* row max (i, jc): over the scores (i, jc .. jc + 2 h), the samples within h of column xs + jc */
            for (uint32_t idx = tid; idx < sh * tw; idx += 256u) {
                const uint32_t i = idx / tw, jc = idx - i * tw;
                score_t m = 0;
                for (uint32_t j = jc; j <= jc + 2u * h; j++) m = max(m, s_s[i * SP + j]);
                s_r[i * COLS + jc] = m;
            }
            __syncthreads();
            /* the samples of T in this tile: who survives goes behind the list */
            for (uint32_t idx = tid; idx < th * tw; idx += 256u) {
                const uint32_t ic = idx / tw, jc = idx - ic * tw;
                const score_t p = s_s[(ic + h) * SP + jc + h];
                if ((unsigned long long)p <= min_score) continue;
                score_t before = 0, after = 0;
                for (uint32_t k = 0; k < h; k++) {
                    before = max(before, max(s_s[(ic + h) * SP + jc + k], s_r[(ic + k) * COLS + jc]));
                    after = max(after, max(s_s[(ic + h) * SP + jc + h + 1u + k], s_r[(ic + h + 1u + k) * COLS + jc]));
                }
                if (p > before && p >= after) {
                    const uint32_t at = __hip_atomic_fetch_add(&s_n, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (at < CORNER_LIST) { s_ls[at] = p; s_lp[at] = (ys + ic) << 16 | (xs + jc); }
                }
            }
            __syncthreads();
            /* the same for every thread: the list is ranked, and cut to the best K, when the next tile might not fit behind it */
            const uint32_t total = min(s_n, CORNER_LIST);
            if (total > nbest) { found += total - nbest; nbest = total; ranked = false; }
            if (!ranked && nbest + TILE_MAX > CORNER_LIST) {
                nbest = corner_rank(s_ls, s_lp, nbest, K, tid);
                ranked = true;
                if (tid == 0u) s_n = nbest;
            }
        }
    }
    __syncthreads();
    if (!ranked) nbest = corner_rank(s_ls, s_lp, nbest, K, tid);
    energy = stats_wave_sum(energy);
    if (lane == 0u) s_en[wave] = energy;
    __syncthreads();
    energy = s_en[0] + s_en[1] + s_en[2] + s_en[3];

    if (S > 1u) {
        /* the bands' partials meet in the scratch: u32 entries, found; u64 energy; the entries as u32 position, 0, u64 score at 32 */
        uint8_t *part = a.partials + ((size_t)blockIdx.y * S + band) * CORNER_PARTIAL;
        if (tid == 0u) {
            reinterpret_cast<uint32_t *>(part)[0] = nbest;
            reinterpret_cast<uint32_t *>(part)[1] = found;
            reinterpret_cast<unsigned long long *>(part)[1] = energy;
        }
        if (tid < nbest) {
            reinterpret_cast<unsigned long long *>(part)[4u + 2u * tid] = s_lp[tid];
            reinterpret_cast<unsigned long long *>(part)[5u + 2u * tid] = s_ls[tid];
        }
        if (!region_hand_over(a.tickets, S)) return;
        nbest = 0u; found = 0u; energy = 0ull;
        for (uint32_t b = 0; b < S; b++) {
            const uint8_t *pp = a.partials + ((size_t)blockIdx.y * S + b) * CORNER_PARTIAL;
            const uint32_t nb = min(reinterpret_cast<const uint32_t *>(pp)[0], K);
            found += reinterpret_cast<const uint32_t *>(pp)[1];
            energy += reinterpret_cast<const unsigned long long *>(pp)[1];
            if (!nb) continue;
            if (tid < nb) {
                s_lp[nbest + tid] = (uint32_t)reinterpret_cast<const unsigned long long *>(pp)[4u + 2u * tid];
                s_ls[nbest + tid] = reinterpret_cast<const unsigned long long *>(pp)[5u + 2u * tid];
            }
            __syncthreads();
            nbest = corner_rank(s_ls, s_lp, nbest + nb, K, tid);
        }
    }

    /* the record, whole: the header, the points in the regions' coordinates, zeros behind them */
    uint32_t *dst32 = reinterpret_cast<uint32_t *>(it.dst);
    if (tid == 0u) {
        dst32[0] = bd.empty ? 0u : (it.x1 - it.x0) * (it.y1 - it.y0);
        dst32[1] = found;
        dst32[2] = nbest;
        dst32[3] = 0u;
        reinterpret_cast<unsigned long long *>(it.dst)[2] = energy;
        reinterpret_cast<unsigned long long *>(it.dst)[3] = 0ull;
    }
    if (tid < K) {
        const bool on = tid < nbest;
        const uint32_t pos = on ? s_lp[tid] : 0u;
        dst32[8u + 4u * tid] = on ? (pos & 0xFFFFu) - it.wx0 : 0u;
        dst32[9u + 4u * tid] = on ? (pos >> 16) - it.wy0 : 0u;
        reinterpret_cast<unsigned long long *>(it.dst)[5u + 2u * tid] = on ? s_ls[tid] : 0ull;
    }
    region_ticket_rezero(a.tickets, S > 1u);
}

} // namespace h264k
