/* kernels/k_region_shift.hip.h — WHERE did a box go: block-matching SAD search of boxes of the KEPT picture (k_keep.hip.h) in the
 * CURRENT picture of the same instance (h264bsdmiOutputRegionShift), luma only, both read from their macroblock tiles where they lie.
 * Included by engine.hip after k_region_change.hip.h; the band / ticket scheme and the wave reduction are region_common.hip.h's, the
 * staging (luma_stage, here on the ShiftItem itself), the masked path (shift_sad4) and the argmin's key (shift_key) luma_search.hip.h's; like them, not part of the kernel sources that key the committed counter tables (srchash.py).
 *
 * One record, R = radius (0 .. 16), D = 2 R + 1, little endian, 32 bytes, with the surface 32 + 4 (D D + 1):
 *     u32 count; u32 D; i32 dx; i32 dy; u32 best; u32 still; u32 ties; u32 zero;   [ D x D x u32 sad[(dy + R) D + (dx + R)]; u32 zero ]
 *     SAD(dx, dy) = sum over (u, v) of T = box ∩ window of | kept(u, v) - current(clamp(u + dx), clamp(v + dy)) |, clamped at the WINDOW
 * grid (S row bands, regions) x 256.  A band is walked in tiles of at most SHIFT_ROWS x 4 SHIFT_COLS4 template samples, column chunk
 * by column chunk, by the same workgroup.  Per tile both pictures are read from memory ONCE and staged in LDS as raster rows of dwords
 * (luma_stage: two aligned tile dwords and v_alignbyte per staged dword; bytewise where the clamp at the window is active): the
 * template with its first sample in byte 0 of dword 0, the current picture from R rows above and R columns left of it, th + 2 R rows of
 * tw4 + Q dwords, Q = ceil(D / 4) rounded up to whole threads.  The halo is what is read more than once: R rows per tile above and
 * below, R columns beside it.
 * LDS (160 KiB per compute unit): 32 x 64 dwords of template (8 KiB), 64 rows at a pitch of 75 dwords of current picture (18.75 KiB;
 * the odd pitch keeps rows that differ by dy on different banks) and 33 x 36 sums (4.6 KiB): 31.5 KiB per workgroup whatever the
 * radius, five workgroups of 256 to a compute unit.  A taller band or a wider box does not grow it: they take more tiles.
 * The sums: a QUAD is four displacements dx = 4 q - R .. + 3 of one row dy of the surface.  v_qsad_pk_u16_u8 takes the template
 * dword u and the eight bytes of the current picture from dword u + q of row v + dy and adds the four SADs of the four byte offsets
 * to four packed 16-bit sums: sixteen differences per instruction.  A thread takes QUADS adjacent quads of one row dy (a PAIR) and
 * walks a segment of a template row: per template dword it reads that dword and ONE new dword of the current picture (the others are
 * the step before's), so with QUADS = 3 two LDS reads feed three instructions.  QUADS is 3 from radius SHIFT_QUADS_FROM on and 1 below
 * it, where whole threads of three quads would mostly compute displacements beyond 2 R: each measured faster on its side.  The pairs
 * are dealt to the threads SHIFT_SPLIT / P ways (P pairs), each share a set of row segments of the tile, so that 256 threads are busy
 * at every radius; a thread unpacks its packed sums after every segment (SHIFT_FOLD instructions would fit; as the tile and SHIFT_SPLIT
 * stand a segment has 32 dwords at the most, from radius 12 on: tests/test_saturated_motion_reach.py), keeps 32-bit sums per tile
 * and adds them to the workgroup's surface in LDS (ds_add_u32, integers: no order shows).  The last template dword of a row, when the
 * width is no multiple of 4, goes through v_sad_u8 with a byte mask on both operands instead.  Displacements beyond 2 R in the last
 * pair of a row are computed and dropped.
 * Two other inner loops were measured and lost (docs/EXPERIMENTS.md, "Region shift"): v_sad_u8 per displacement, and
 * v_mqsad_pk_u16_u8, which SKIPS bytes that are 0 in its reference operand and so needs a guard; tools/experiments/shift_inner_loops.patch
 * puts them back behind -DSHIFT_INNER for whoever wants to measure again.
 * S == 1: the workgroup closes the record.  S > 1: the bands' D D partial sums meet in the engine's scratch under
 * region_hand_over; the band that draws the last ticket adds them up and closes the record: argmin with the tie rule (smallest SAD,
 * then smallest dx^2 + dy^2, then smallest dy, then smallest dx) as ONE 64-bit key per displacement, the number of ties, the header and
 * the surface with plain vector stores.  All integers: the result does not depend on which band arrives last. */
#pragma once
namespace h264k {

constexpr uint32_t SHIFT_QUADS = 3, SHIFT_QUADS_FROM = 4;       /* quads of displacements a thread takes per template dword, from which radius on (below: 1) */
constexpr uint32_t SHIFT_MAX_RADIUS = 16, SHIFT_MAX_D = 2 * SHIFT_MAX_RADIUS + 1;
constexpr uint32_t SHIFT_MAX_Q = ((SHIFT_MAX_D + 3) / 4 + SHIFT_QUADS - 1) / SHIFT_QUADS * SHIFT_QUADS;      /* quads per row of the surface, in whole threads: 9 */
constexpr uint32_t SHIFT_ROWS = 32, SHIFT_COLS4 = 64;                               /* a tile of template: rows, dwords per row */
constexpr uint32_t SHIFT_CUR_ROWS = SHIFT_ROWS + 2 * SHIFT_MAX_RADIUS, SHIFT_PITCH = SHIFT_COLS4 + SHIFT_MAX_Q + 2;     /* 64, 75 */
/* v_qsad_pk_u16_u8 instructions a packed 16-bit sum takes before it is unpacked: each adds at most 4 x 255 = 1020, and
 * 64 x 1020 = 65280 <= 65535.  A segment can never exceed SHIFT_COLS4 = 64 dwords of one row (the rule for L in the kernel keeps it at 32);
 * k_cell_shift's items do reach 64.  The 32-bit sums behind it: a region has at most
 * 4096 x 4096 samples (H264BSDMI_SHIFT_MAX_SIDE), 2^24 x 255 < 2^32 */
constexpr uint32_t SHIFT_FOLD = 64;
static_assert(SHIFT_COLS4 <= SHIFT_FOLD && SHIFT_FOLD * 4 * 255 <= 65535, "a segment's packed sums must fit 16 bits");
constexpr uint32_t SHIFT_SPLIT = 1024;                                              /* (pair, share) work items a workgroup aims at */
constexpr uint32_t SHIFT_MAX_PARTIAL = 4 * SHIFT_MAX_D * SHIFT_MAX_D;               /* a band's partial surface, bytes */

__host__ __device__ constexpr uint32_t shift_record_bytes(uint32_t radius, uint32_t surface)
{
    return 32u + (surface ? 4u * ((2u * radius + 1u) * (2u * radius + 1u) + 1u) : 0u);
}

/* one region: the two frames, the record, box ∩ window [x0, x1) x [y0, y1) and the window [wx0, wx1) x [wy0, wy1) itself, all in luma
 * samples of the coded frame (x1 <= x0: empty) */
struct ShiftItem { const uint8_t *cur; const uint8_t *kept; uint8_t *dst; uint32_t wmb, x0, y0, x1, y1, wx0, wy0, wx1, wy1; };
/* partials: region r's band b at ((r S + b) D D) words; tickets: as StatsArgs */
struct ShiftArgs { const ShiftItem *items; uint8_t *partials; uint32_t *tickets; uint32_t radius, surface; };

template <uint32_t QUADS>
__global__ __launch_bounds__(256) void k_region_shift(ShiftArgs a)
{
    __shared__ uint32_t s_t[SHIFT_ROWS * SHIFT_COLS4];
    __shared__ uint32_t s_c[SHIFT_CUR_ROWS * SHIFT_PITCH];
    __shared__ uint32_t s_sad[SHIFT_MAX_D * 4u * SHIFT_MAX_Q];              /* row dy + R at a pitch of SP */
    __shared__ unsigned long long s_key[4];
    __shared__ uint32_t s_ties[4];
    const ShiftItem it = a.items[blockIdx.y];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t R = a.radius, D = 2u * R + 1u, Q3 = ((D + 3u) / 4u + QUADS - 1u) / QUADS, P = D * Q3, G = (SHIFT_SPLIT + P - 1u) / P;
    const uint32_t SP = 4u * QUADS * Q3;
    const uint32_t S = gridDim.x, band = blockIdx.x, n = D * D;
    for (uint32_t i = tid; i < D * SP; i += 256u) s_sad[i] = 0u;

    const RegionBand bd = region_band(it.x0, it.y0, it.x1, it.y1, band, S);
    const bool empty = bd.empty;
    const uint32_t r0 = bd.r0, r1 = bd.r1;
    const uint32_t ya = max(it.y0, r0 * 16u), yb = empty ? ya : min(it.y1, r1 * 16u);           /* this band's template rows */
    for (uint32_t ys = ya; ys < yb; ys += SHIFT_ROWS) {
        const uint32_t th = min(SHIFT_ROWS, yb - ys);
        for (uint32_t xs = it.x0; xs < it.x1; xs += 4u * SHIFT_COLS4) {
            const uint32_t tw = min(4u * SHIFT_COLS4, it.x1 - xs), tw4 = (tw + 3u) >> 2;
            const uint32_t tail = (tw & 3u) ? (1u << (8u * (tw & 3u))) - 1u : 0xFFFFFFFFu;      /* the bytes of a row's last dword that count */
            __syncthreads();                                                /* the sums are zero / the tile before has been read */
            luma_stage(it.kept, it, (int)xs, (int)ys, tw4, th, s_t, SHIFT_COLS4, tid);
            luma_stage(it.cur, it, (int)xs - (int)R, (int)ys - (int)R, tw4 + QUADS * Q3, th + 2u * R, s_c, SHIFT_PITCH, tid);
            __syncthreads();
            /* segments of L dwords of one row, about four per share */
            uint32_t L = 1u;
            while (L < SHIFT_COLS4 && 2u * L * 4u * G <= th * tw4) L *= 2u;
            const uint32_t spr = (tw4 + L - 1u) / L, ns = th * spr;
            for (uint32_t vp = tid; vp < P * G; vp += 256u) {
                const uint32_t g = vp / P, p = vp - g * P, dyi = p / Q3, q = (p - dyi * Q3) * QUADS;
                uint32_t sum[QUADS][4] = {};
                for (uint32_t s = g; s < ns; s += G) {
                    const uint32_t v = s / spr, u0 = (s - v * spr) * L, u1 = min(u0 + L, tw4);
                    const uint32_t *tp = s_t + v * SHIFT_COLS4, *cp = s_c + (v + dyi) * SHIFT_PITCH + q;
                    unsigned long long acc[QUADS] = {};
                    uint32_t c[QUADS + 1];
#pragma unroll
                    for (uint32_t j = 0; j < QUADS; j++) c[j] = cp[u0 + j];
                    for (uint32_t u = u0; u < u1; u++) {
                        const uint32_t t = tp[u];
                        c[QUADS] = cp[u + QUADS];
                        if (u + 1u == tw4 && tail != 0xFFFFFFFFu) {
#pragma unroll
                            for (uint32_t j = 0; j < QUADS; j++) shift_sad4(c[j], c[j + 1u], t, tail, sum[j]);
                        } else {
#pragma unroll
                            for (uint32_t j = 0; j < QUADS; j++) {
                                const unsigned long long cc = (unsigned long long)c[j + 1u] << 32 | c[j];
                                acc[j] = __builtin_amdgcn_qsad_pk_u16_u8(cc, t, acc[j]);
                            }
                        }
#pragma unroll
                        for (uint32_t j = 0; j < QUADS; j++) c[j] = c[j + 1u];
                    }
#pragma unroll
                    for (uint32_t j = 0; j < QUADS; j++)
#pragma unroll
                        for (uint32_t k = 0; k < 4u; k++) sum[j][k] += shift_field(acc[j], k);
                }
#pragma unroll
                for (uint32_t j = 0; j < QUADS; j++)
#pragma unroll
                    for (uint32_t k = 0; k < 4u; k++) {
                        const uint32_t dxi = 4u * (q + j) + k;
                        if (dxi < D && sum[j][k]) region_lds_add(&s_sad[dyi * SP + dxi], sum[j][k]);
                    }
            }
        }
    }
    __syncthreads();

    if (S > 1u) {
        /* the bands' partial surfaces meet in the scratch */
        uint32_t *part = reinterpret_cast<uint32_t *>(a.partials) + ((size_t)blockIdx.y * S + band) * n;
        for (uint32_t i = tid; i < n; i += 256u) part[i] = s_sad[(i / D) * SP + i % D];
        if (!region_hand_over(a.tickets, S)) return;
        const uint32_t *pp = reinterpret_cast<const uint32_t *>(a.partials) + (size_t)blockIdx.y * S * n;
        for (uint32_t i = tid; i < n; i += 256u) {
            uint32_t t = 0u;
            for (uint32_t b = 0; b < S; b++) t += pp[(size_t)b * n + i];
            s_sad[(i / D) * SP + i % D] = t;
        }
        __syncthreads();
    }

    /* the smallest (SAD, dx^2 + dy^2, dy, dx) as one key; then how many displacements share its SAD */
    unsigned long long key = ~0ull;
    for (uint32_t i = tid; i < n; i += 256u) {
        const uint32_t dyi = i / D, dxi = i - dyi * D;
        key = min(key, shift_key(s_sad[dyi * SP + dxi], dxi, dyi, R));
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) key = min(key, (unsigned long long)__shfl_xor(key, d));
    if (lane == 0u) s_key[wave] = key;
    __syncthreads();
    key = min(min(s_key[0], s_key[1]), min(s_key[2], s_key[3]));
    const uint32_t best = shift_key_best(key);
    uint32_t ties = 0u;
    for (uint32_t i = tid; i < n; i += 256u) ties += s_sad[(i / D) * SP + i % D] == best ? 1u : 0u;
    ties = stats_wave_sum(ties);
    if (lane == 0u) s_ties[wave] = ties;
    __syncthreads();
    uint32_t *dst32 = reinterpret_cast<uint32_t *>(it.dst);
    if (tid == 0u) {
        dst32[0] = empty ? 0u : (it.x1 - it.x0) * (it.y1 - it.y0);
        dst32[1] = D;
        dst32[2] = shift_key_dx(key, R);
        dst32[3] = shift_key_dy(key, R);
        dst32[4] = best;
        dst32[5] = s_sad[R * SP + R];
        dst32[6] = s_ties[0] + s_ties[1] + s_ties[2] + s_ties[3];
        dst32[7] = 0u;
    }
    if (a.surface) {
        for (uint32_t i = tid; i <= n; i += 256u) dst32[8u + i] = i < n ? s_sad[(i / D) * SP + i % D] : 0u;
    }
    region_ticket_rezero(a.tickets, S > 1u);
}

} // namespace h264k
