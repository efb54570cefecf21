/* kernels/k_point_matches.hip.h — WHERE did the points go, at any distance: a 256-bit binary descriptor of every corner point of a kept and
 * of a current picture, and the Hamming matching of the two sets (h264bsdmiOutputPointMatches), luma only, read from the macroblock tiles
 * where they lie.  Included by engine.hip after k_corner_points.hip.h; luma_stage (luma_search.hip.h) stages the luma, the wave sums
 * are region_common.hip.h's; like them, not part of the kernel sources that key the committed counter tables (srchash.py).
 *
 * The quantity (include/h264bsd_mi355x.h has it in full), all integers, T = box ∩ window:
 *     L~          the luma replicated at the border of the WINDOW (the clamp of luma_stage), the only border rule
 *     B(u, v)     the sum of L~ over the 5 x 5 samples around (u, v), 0 .. 6375
 *     bit t       of the descriptor of (x, y): B(x + px_t, y + py_t) < B(x + qx_t, y + qy_t), the 256 tests of descriptor_pattern.h
 *     valid       slot i of a point record: i < min(written, K) and (x, y) in T; the descriptor of an invalid slot is zero
 *     d(i, j)     popcount(Dk[i] xor Dc[j]) over the candidates j of kept slot i: the valid current slots, within max_move if that is set
 *     best, second, mutual, accepted: as the header says
 *     record      u32 kept_valid, current_valid, accepted, mutual; i32 sum_dx, sum_dy; u32 0, 0; K x { i32 j; u32 best, second, flags };
 *                 K x 32 bytes of kept descriptors; K x 32 bytes of current descriptors: 32 + 80 K bytes, written whole by the two kernels
 * k_point_describe, grid (groups of MATCH_GROUP slots, regions) x 256.  The 2 K slots of a region are the K kept ones and behind them the
 * K current ones, as their descriptors lie in the record.  A wavefront takes one slot at a time, the workgroup four: the 29 x 29 patch
 * around the point is staged by luma_stage as 29 rows of 8 dwords (the clamp at the window happens there), a lane makes four horizontal
 * 5-sums from two dwords (u16, 29 x 28), a lane makes two vertical 5-sums from five dwords of those (u16, 25 x 26: the 25 x 25 values of
 * B the tests can name), and lane l evaluates the tests l, l + 64, l + 128 and l + 192, whose eight LDS offsets it computed once from
 * the pattern; four ballots are the 256 bits, which lanes 0 .. 7 store.  The point records are the caller's memory: `written` is clamped
 * and a point is staged only when it lies in T, so whatever they hold no sample outside the window and no byte outside the record is read.
 * k_point_match, grid (regions) x 256, behind it on the same stream: both descriptor sets (16 KiB at K = 256) and the coordinates in LDS;
 * thread i owns kept slot i and walks the current slots with its descriptor in registers (8 xor + popcount a pair, the other side's
 * descriptor a broadcast read), then thread j owns current slot j and walks the kept slots the same way for the smallest (d, i) of its
 * column: mutuality without an atomic.  The header is a sum over wavefronts, then over the four of them: integers, no order shows.
 * Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): DESIGN.md §4.4 quotes them; no scratch, no spills. */
#pragma once
#include "../descriptor_pattern.h"
namespace h264k {

constexpr uint32_t MATCH_MAX_K = 256;
constexpr uint32_t MATCH_GROUP = 16;                                /* slots a workgroup of k_point_describe takes: four rounds of four */
constexpr uint32_t MATCH_HALO = DESCRIPTOR_REACH + 2u;              /* 14: the samples a descriptor reads around its point */
constexpr uint32_t MATCH_PATCH = 2u * MATCH_HALO + 1u;              /* 29 */
constexpr uint32_t MATCH_B = 2u * DESCRIPTOR_REACH + 1u;            /* 25: the values of B along one axis */
constexpr uint32_t MATCH_PP = 8, MATCH_HP = 28, MATCH_BP = 26;      /* pitches: patch (dwords), horizontal sums and B (u16) */
constexpr uint32_t MATCH_NONE = 257;                                /* no distance */
static_assert(MATCH_PATCH <= 4u * MATCH_PP && MATCH_B + 3u <= MATCH_HP && MATCH_B + 1u <= MATCH_BP, "the pitches hold the rows");
static_assert(MATCH_MAX_K <= 256u, "a thread of k_point_match owns a slot");

__constant__ const signed char DESCRIPTOR_PATTERN_DEV[4 * DESCRIPTOR_TESTS] = { DESCRIPTOR_PATTERN_VALUES };

__host__ __device__ constexpr uint32_t matches_record_bytes(uint32_t max_points) { return 32u + 80u * max_points; }

/* one region: the two frames, the record, the two point records, box ∩ window [x0, x1) x [y0, y1) and the window [wx0, wx1) x [wy0, wy1)
 * itself, all in luma samples of the coded frame (x1 <= x0: empty) */
struct MatchItem { const uint8_t *cur; const uint8_t *kept; uint8_t *dst; const uint8_t *kpts; const uint8_t *cpts;
                   uint32_t wmb, x0, y0, x1, y1, wx0, wy0, wx1, wy1; };
struct MatchArgs { const MatchItem *items; uint32_t max_points, max_distance, ratio, max_move, mutual_only; };

/* slot i of a point record (the caller's memory, whatever it holds): its point in the region's coordinates, and whether it is valid */
__device__ __forceinline__ bool match_point(const uint8_t *pts, const MatchItem &it, uint32_t i, uint32_t K, int *x, int *y)
{
    const uint32_t written = min(reinterpret_cast<const uint32_t *>(pts)[2], K);
    if (i >= written) { *x = 0; *y = 0; return false; }
    *x = reinterpret_cast<const int *>(pts)[8u + 4u * i];
    *y = reinterpret_cast<const int *>(pts)[9u + 4u * i];
    /* T relative to the window's origin: small numbers, whatever x and y are */
    return *x >= (int)it.x0 - (int)it.wx0 && *x < (int)it.x1 - (int)it.wx0 && *y >= (int)it.y0 - (int)it.wy0 && *y < (int)it.y1 - (int)it.wy0;
}

__global__ __launch_bounds__(256) void k_point_describe(MatchArgs a)
{
    __shared__ uint32_t s_p[4][MATCH_PATCH * MATCH_PP];
    __shared__ uint32_t s_h[4][MATCH_PATCH * MATCH_HP / 2u];                /* u16 pairs */
    __shared__ uint32_t s_b[4][MATCH_B * MATCH_BP / 2u];
    const MatchItem it = a.items[blockIdx.y];
    const LumaWindow win{ it.wmb, it.wx0, it.wy0, it.wx1, it.wy1 };
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, K = a.max_points;
    /* this lane's four tests as offsets into B, once */
    uint32_t op[4], oq[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        const signed char *t = DESCRIPTOR_PATTERN_DEV + 4u * (lane + 64u * k);
        op[k] = (uint32_t)(t[1] + (int)DESCRIPTOR_REACH) * MATCH_BP + (uint32_t)(t[0] + (int)DESCRIPTOR_REACH);
        oq[k] = (uint32_t)(t[3] + (int)DESCRIPTOR_REACH) * MATCH_BP + (uint32_t)(t[2] + (int)DESCRIPTOR_REACH);
    }
    uint16_t *hw = reinterpret_cast<uint16_t *>(s_h[wave]);
    const uint16_t *bb = reinterpret_cast<const uint16_t *>(s_b[wave]);
    for (uint32_t s0 = blockIdx.x * MATCH_GROUP; s0 < min((blockIdx.x + 1u) * MATCH_GROUP, 2u * K); s0 += 4u) {
        /* the four slots of this round, the same for every thread; wave w describes slot s0 + w */
        int px[4] = {}, py[4] = {};
        bool ok[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t s = s0 + k;
            ok[k] = s < 2u * K && match_point(s < K ? it.kpts : it.cpts, it, s < K ? s : s - K, K, &px[k], &py[k]);
        }
        __syncthreads();                                                    /* the round before has been read */
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++)
            if (ok[k])
                luma_stage(s0 + k < K ? it.kept : it.cur, win, (int)it.wx0 + px[k] - (int)MATCH_HALO, (int)it.wy0 + py[k] - (int)MATCH_HALO,
                            MATCH_PP, MATCH_PATCH, s_p[k], MATCH_PP, tid);
        __syncthreads();
        const bool mine = wave == 0u ? ok[0] : wave == 1u ? ok[1] : wave == 2u ? ok[2] : ok[3];      /* wave-uniform */
        if (mine) {
            /* horizontal: (r, q) makes the sums of columns 4 q .. 4 q + 3 from the eight bytes of dwords q, q + 1 */
            for (uint32_t i = lane; i < MATCH_PATCH * 7u; i += 64u) {
                const uint32_t r = i / 7u, q = i - r * 7u;
                const unsigned long long v = (unsigned long long)s_p[wave][r * MATCH_PP + q + 1u] << 32 | s_p[wave][r * MATCH_PP + q];
                uint32_t b[8];
#pragma unroll
                for (uint32_t c = 0; c < 8u; c++) b[c] = (uint32_t)(v >> (8u * c)) & 255u;
#pragma unroll
                for (uint32_t c = 0; c < 4u; c++) hw[r * MATCH_HP + 4u * q + c] = (uint16_t)(b[c] + b[c + 1u] + b[c + 2u] + b[c + 3u] + b[c + 4u]);
            }
        }
        __syncthreads();
        if (mine) {
            /* vertical: (r, c2) makes B of columns 2 c2, 2 c2 + 1 of row r from five rows of pairs; the halves never carry (<= 6375) */
            for (uint32_t i = lane; i < MATCH_B * (MATCH_BP / 2u); i += 64u) {
                const uint32_t r = i / (MATCH_BP / 2u), c2 = i - r * (MATCH_BP / 2u);
                uint32_t t = 0u;
#pragma unroll
                for (uint32_t k = 0; k < 5u; k++) t += s_h[wave][(r + k) * (MATCH_HP / 2u) + c2];
                s_b[wave][r * (MATCH_BP / 2u) + c2] = t;
            }
        }
        __syncthreads();
        const uint32_t s = s0 + wave;
        if (s < 2u * K) {
            unsigned long long bits[4];
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) bits[k] = mine ? __ballot(bb[op[k]] < bb[oq[k]]) : 0ull;
            if (lane < 8u) {
                const unsigned long long w = lane < 2u ? bits[0] : lane < 4u ? bits[1] : lane < 6u ? bits[2] : bits[3];
                reinterpret_cast<uint32_t *>(it.dst + 32u + 16u * K)[8u * s + lane] = (uint32_t)(lane & 1u ? w >> 32 : w);
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_point_match(MatchArgs a)
{
    __shared__ uint32_t s_dk[MATCH_MAX_K * 8u], s_dc[MATCH_MAX_K * 8u];
    __shared__ int s_x[2][MATCH_MAX_K], s_y[2][MATCH_MAX_K];
    __shared__ uint32_t s_ok[2][MATCH_MAX_K];
    __shared__ uint32_t s_col[MATCH_MAX_K];                                 /* per current slot: the kept slot of its smallest (d, i), or NONE */
    __shared__ int s_sum[4][6];
    const MatchItem it = a.items[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, K = a.max_points;
    const uint32_t *dsc = reinterpret_cast<const uint32_t *>(it.dst + 32u + 16u * K);
    const uint32_t nk = min(reinterpret_cast<const uint32_t *>(it.kpts)[2], K), nc = min(reinterpret_cast<const uint32_t *>(it.cpts)[2], K);
    for (uint32_t i = tid; i < 8u * K; i += 256u) { s_dk[i] = dsc[i]; s_dc[i] = dsc[8u * K + i]; }
    if (tid < K) {
        int x, y;
        s_ok[0][tid] = match_point(it.kpts, it, tid, K, &x, &y) ? 1u : 0u; s_x[0][tid] = x; s_y[0][tid] = y;
        s_ok[1][tid] = match_point(it.cpts, it, tid, K, &x, &y) ? 1u : 0u; s_x[1][tid] = x; s_y[1][tid] = y;
    }
    __syncthreads();
    const int move = a.max_move ? (int)a.max_move : 0x7FFFFFFF;             /* valid points lie in the window: their differences are small */
    /* thread i, kept slot i: the best and the second of its row.  Thread j, current slot j: the best kept slot of its column */
    const bool row = tid < K && s_ok[0][tid], column = tid < K && s_ok[1][tid];
    uint32_t best = MATCH_NONE, second = MATCH_NONE, bj = 0xFFFFFFFFu;
    if (row) {
        uint32_t d[8];
#pragma unroll
        for (uint32_t k = 0; k < 8u; k++) d[k] = s_dk[8u * tid + k];
        const int x = s_x[0][tid], y = s_y[0][tid];
        for (uint32_t j = 0; j < nc; j++) {
            if (!s_ok[1][j] || abs(s_x[1][j] - x) > move || abs(s_y[1][j] - y) > move) continue;
            uint32_t n = 0u;
#pragma unroll
            for (uint32_t k = 0; k < 8u; k++) n += (uint32_t)__builtin_popcount(d[k] ^ s_dc[8u * j + k]);
            if (n < best) { second = best; best = n; bj = j; }
            else if (n < second) second = n;
        }
    }
    if (tid < K) {
        uint32_t cb = MATCH_NONE, ci = 0xFFFFFFFFu;
        if (column) {
            uint32_t d[8];
#pragma unroll
            for (uint32_t k = 0; k < 8u; k++) d[k] = s_dc[8u * tid + k];
            const int x = s_x[1][tid], y = s_y[1][tid];
            for (uint32_t i = 0; i < nk; i++) {
                if (!s_ok[0][i] || abs(s_x[0][i] - x) > move || abs(s_y[0][i] - y) > move) continue;
                uint32_t n = 0u;
#pragma unroll
                for (uint32_t k = 0; k < 8u; k++) n += (uint32_t)__builtin_popcount(d[k] ^ s_dk[8u * i + k]);
                if (n < cb) { cb = n; ci = i; }
            }
        }
        s_col[tid] = ci;
    }
    __syncthreads();
    const bool has = bj != 0xFFFFFFFFu;
    const bool mutual = has && s_col[bj] == tid;
    const bool accepted = has && best <= a.max_distance && (a.ratio == 256u || best * 256u < a.ratio * second) && (!a.mutual_only || mutual);
    uint32_t *dst32 = reinterpret_cast<uint32_t *>(it.dst);
    if (tid < K) {
        dst32[8u + 4u * tid] = bj;
        dst32[9u + 4u * tid] = best;
        dst32[10u + 4u * tid] = second;
        dst32[11u + 4u * tid] = (row ? 1u : 0u) | (mutual ? 2u : 0u) | (accepted ? 4u : 0u);
    }
    int sums[6] = { row ? 1 : 0, column ? 1 : 0, accepted ? 1 : 0, mutual ? 1 : 0,
                    accepted ? s_x[1][bj] - s_x[0][tid] : 0, accepted ? s_y[1][bj] - s_y[0][tid] : 0 };
#pragma unroll
    for (uint32_t k = 0; k < 6u; k++) {
        sums[k] = stats_wave_sum(sums[k]);
        if (lane == 0u) s_sum[wave][k] = sums[k];
    }
    __syncthreads();
    if (tid < 8u) dst32[tid] = tid < 6u ? (uint32_t)(s_sum[0][tid] + s_sum[1][tid] + s_sum[2][tid] + s_sum[3][tid]) : 0u;
}

} // namespace h264k
