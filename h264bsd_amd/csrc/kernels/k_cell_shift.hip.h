/* kernels/k_cell_shift.hip.h — WHERE did every cell go: the block-matching SAD search of k_region_shift.hip.h for every cell of a grid
 * of square cells laid over a box (h264bsdmiOutputCellShift): cell (i, j) of a region holds count, dx, dy, best, still and ties of the
 * record k_region_shift writes for the cell's box, template from the KEPT picture, searched in the CURRENT picture clamped at the
 * WINDOW, luma only.  Included by engine.hip after k_region_shift.hip.h, whose constants and inner loop it uses, with the staging (luma_stage), the
 * masked path (shift_sad4) and the argmin's key (shift_key) of luma_search.hip.h and the ownership scheme of k_cell_maps.hip.h; like them, not part of the kernel sources that key the
 * committed counter tables (srchash.py).
 *
 * A slice: P maps of rows x cols u32, row-major, in ascending bit order of H264BSDMI_FLOW_*: count, dx (i32), dy (i32), best, still, ties.
 * grid (rectangles of cells, regions) x 256.  A workgroup OWNS a rectangle of FLOW_RECT_W x FLOW_RECT_H luma samples of the grid,
 * (64 >> s) x (64 >> s) cells of side 1 << s (64, 16, 4 cells or 1).  Every cell belongs to exactly one workgroup: no scratch, no
 * ticket, no hand-over between workgroups, and nothing depends on scheduling.
 * STAGING, once per rectangle: box ∩ window ∩ rectangle of the kept picture as raster rows of dwords from the rectangle's left edge
 * (rounded down to the dword that holds the first sample that counts, so a cell starts on a dword), and the current picture from R rows
 * above and R columns left of it: th + 2 R rows of tw4 + Q dwords, clamped at the window by luma_stage.  The halo is what is read more
 * than once: at R = 16, 96 x 96 samples for 64 x 64 of template.
 * LDS (160 KiB per compute unit): 64 x 16 dwords of template (4 KiB), 96 rows at a pitch of 27 dwords of current picture (10.1 KiB, the
 * odd pitch keeps rows that differ by dy on different banks), FLOW_SURF_WORDS of SAD surfaces (16 KiB) and 5 x 64 results: 31.5 KiB,
 * five workgroups of 256 to a compute unit, as the sibling.
 * THE SUMS: a cell's D x D surface (D = 2 R + 1) is D D words, 1089 at R = 16, so the rectangle's cells are walked in GROUPS of as
 * many cells as FLOW_SURF_WORDS hold.  An ITEM is (cell, share g of G, row dy of the surface, QUADS adjacent quads of displacements):
 * the thread walks the rows va + g, va + g + G, .. of the cell's template, per template dword one new dword of the current picture and
 * QUADS v_qsad_pk_u16_u8, exactly the sibling's loop; the packed 16-bit sums are unpacked before they could have taken more than
 * SHIFT_FOLD instructions (a cell's row is at most 16 dwords, so every fourth row at the worst; a sum takes exactly SHIFT_FOLD for cells
 * of 32 from radius 8 and of 64 from radius 6 on, and no unpacking happens on the way below that: tests/test_saturated_motion_reach.py).
 * A dword of which only some bytes belong to the cell (its first or last, where box or window cut it) goes through v_sad_u8 with a
 * byte mask instead.  G is 1 where the
 * group has FLOW_SPLIT items without it and grows where cells are large and the radius small (radius 0 has one item per cell), up to one
 * row per share.  The final sums are added to the cell's surface with ds_add_u32: integers, no order shows.
 * ARGMIN: after the barrier LPC lanes (a power of two, 64 where the group has four cells or fewer, 256 / cells otherwise) take a cell:
 * the sibling's 64-bit key per displacement (SAD << 32 | d^2 << 12 | dyi << 6 | dxi), its minimum over the lanes by xor shuffles, then
 * the number of displacements whose SAD equals best.  A cell that box or window do not reach has an all-zero surface and so gives
 * dx = dy = best = still = 0 and ties = D D by the same arithmetic; a rectangle they do not reach skips staging and search.
 * STORES: the results wait in LDS until the rectangle is done, then the asked planes are written with plain dword stores, consecutive
 * lanes consecutive cells of a row; count is closed form from the geometry. */
#pragma once
namespace h264k {

constexpr uint32_t FLOW_RECT_W = 64, FLOW_RECT_H = 64;                  /* luma samples of the grid per workgroup */
constexpr uint32_t FLOW_MIN_SHIFT = 3, FLOW_MAX_SHIFT = 6;              /* cells of 8 .. 64 */
constexpr uint32_t FLOW_MAX_CELLS = (FLOW_RECT_W >> FLOW_MIN_SHIFT) * (FLOW_RECT_H >> FLOW_MIN_SHIFT);
constexpr uint32_t FLOW_COLS4 = FLOW_RECT_W / 4;                        /* dwords per template row */
constexpr uint32_t FLOW_CUR_ROWS = FLOW_RECT_H + 2 * SHIFT_MAX_RADIUS, FLOW_PITCH = FLOW_COLS4 + SHIFT_MAX_Q + 2;       /* 96, 27 */
constexpr uint32_t FLOW_SURF_WORDS = 4096;                              /* the surfaces of one group of cells */
constexpr uint32_t FLOW_SPLIT = 512;                                    /* items a group aims at */
constexpr uint32_t FLOW_MAX_GRID = 4096, FLOW_MAX_WORKGROUPS = 1u << 23;
static_assert(FLOW_SURF_WORDS >= SHIFT_MAX_D * SHIFT_MAX_D, "one cell's surface must fit");
static_assert(FLOW_COLS4 <= SHIFT_FOLD && (1u << FLOW_MAX_SHIFT) <= FLOW_RECT_W && (1u << FLOW_MAX_SHIFT) <= FLOW_RECT_H, "a cell's row is one fold at the most");
static_assert((FLOW_PITCH & 1u) == 1u, "rows that differ by dy on different banks");

/* one region: the two frames, the slice, the box's origin (ox, oy) in luma samples of the coded frame, which may be negative or beyond
 * the frame, box ∩ window [x0, x1) x [y0, y1) and the window [wx0, wx1) x [wy0, wy1) in the same (x1 <= x0: empty) */
struct FlowItem { const uint8_t *cur; const uint8_t *kept; uint32_t *dst; uint32_t wmb; int32_t ox, oy; uint32_t x0, y0, x1, y1, wx0, wy0, wx1, wy1; };
/* cols x rows cells of side 1 << shift per slice; rects_x: rectangles per row of rectangles; planes: H264BSDMI_FLOW_* */
struct FlowArgs { const FlowItem *items; uint32_t cols, rows, shift, rects_x, planes, radius; };

template <uint32_t QUADS>
__global__ __launch_bounds__(256) void k_cell_shift(FlowArgs a)
{
    __shared__ uint32_t s_t[FLOW_RECT_H * FLOW_COLS4];
    __shared__ uint32_t s_c[FLOW_CUR_ROWS * FLOW_PITCH];
    __shared__ uint32_t s_sad[FLOW_SURF_WORDS];                             /* cell cl of the group at cl D D, row dy + R at a pitch of D */
    __shared__ uint32_t s_out[5][FLOW_MAX_CELLS];                           /* dx, dy, best, still, ties of the rectangle's cells */
    const FlowItem it = a.items[blockIdx.y];
    const uint32_t tid = threadIdx.x;
    const uint32_t cs = a.shift, planes = a.planes;
    const int cell = 1 << cs;
    const uint32_t R = a.radius, D = 2u * R + 1u, n = D * D, Q3 = ((D + 3u) / 4u + QUADS - 1u) / QUADS, P = D * Q3;
    const uint32_t RW = FLOW_RECT_W >> cs, RH = FLOW_RECT_H >> cs;
    const uint32_t j0 = (blockIdx.x % a.rects_x) * RW, i0 = (blockIdx.x / a.rects_x) * RH;           /* the first cell of the rectangle */
    const uint32_t nj = min(RW, a.cols - j0), ni = min(RH, a.rows - i0), ncell = ni * nj;            /* its cells inside the grid */
    for (uint32_t i = tid; i < 5u * FLOW_MAX_CELLS; i += 256u) s_out[i / FLOW_MAX_CELLS][i % FLOW_MAX_CELLS] = i / FLOW_MAX_CELLS == 4u ? n : 0u;

    /* box ∩ window ∩ rectangle, in luma samples of the coded frame */
    const int rectx = it.ox + (int)j0 * cell, recty = it.oy + (int)i0 * cell;
    const int rx0 = max((int)it.x0, rectx), rx1 = min((int)it.x1, rectx + (int)nj * cell);
    const int ry0 = max((int)it.y0, recty), ry1 = min((int)it.y1, recty + (int)ni * cell);
    if (it.x1 > it.x0 && it.y1 > it.y0 && rx1 > rx0 && ry1 > ry0) {
        const int SX = rectx + (int)(((uint32_t)(rx0 - rectx) >> 2) << 2), SY = ry0;                /* the template's first staged sample */
        const uint32_t tw4 = (uint32_t)(rx1 - SX + 3) >> 2, th = (uint32_t)(ry1 - ry0);
        const LumaWindow win{ it.wmb, it.wx0, it.wy0, it.wx1, it.wy1 };
        luma_stage(it.kept, win, SX, SY, tw4, th, s_t, FLOW_COLS4, tid);
        luma_stage(it.cur, win, SX - (int)R, SY - (int)R, tw4 + QUADS * Q3, th + 2u * R, s_c, FLOW_PITCH, tid);

        const uint32_t gc = min(ncell, FLOW_SURF_WORDS / n);               /* cells per group */
        const uint32_t G = min(max((FLOW_SPLIT + gc * P - 1u) / (gc * P), 1u), (uint32_t)cell);       /* shares of a cell's rows */
        uint32_t LPC = 64u;                                                 /* lanes that take one cell's argmin */
        while (LPC > 1u && LPC * gc > 256u) LPC >>= 1;
        const uint32_t CPP = 256u / LPC, sub = tid & (LPC - 1u), seg = tid / LPC;
        const uint32_t magic = 65536u / D + 1u;                             /* i / D == i * magic >> 16 for i < D D <= 1089 */
        for (uint32_t g0 = 0; g0 < ncell; g0 += gc) {
            const uint32_t gn = min(gc, ncell - g0);
            __syncthreads();                                                /* staged / the group before has been read */
            for (uint32_t i = tid; i < gn * n; i += 256u) s_sad[i] = 0u;
            __syncthreads();
            for (uint32_t vp = tid; vp < gn * G * P; vp += 256u) {
                const uint32_t cl = vp / (G * P), rest = vp - cl * G * P, g = rest / P, p = rest - g * P;
                const uint32_t dyi = p / Q3, q = (p - dyi * Q3) * QUADS;
                const uint32_t c = g0 + cl, ci = c / nj, cj = c - ci * nj;
                const int cellx = rectx + (int)cj * cell, celly = recty + (int)ci * cell;
                const int cx0 = max(rx0, cellx), cx1 = min(rx1, cellx + cell), cy0 = max(ry0, celly), cy1 = min(ry1, celly + cell);
                if (cx1 <= cx0 || cy1 <= cy0) continue;
                /* the cell's bytes [ba, bb) and rows [va, vb) of the staged template; the dwords [u0, u1) that hold them */
                const uint32_t ba = (uint32_t)(cx0 - SX), bb = (uint32_t)(cx1 - SX), va = (uint32_t)(cy0 - SY), vb = (uint32_t)(cy1 - SY);
                const uint32_t u0 = ba >> 2, u1 = (bb + 3u) >> 2;
                const uint32_t mf = 0xFFFFFFFFu << (8u * (ba & 3u)), ml = (bb & 3u) ? (1u << (8u * (bb & 3u))) - 1u : 0xFFFFFFFFu;
                uint32_t sum[QUADS][4] = {};
                unsigned long long acc[QUADS] = {};
                uint32_t pending = 0u;                                      /* v_qsad_pk_u16_u8 per packed sum since it was unpacked */
                for (uint32_t v = va + g; v < vb; v += G) {
                    const uint32_t *tp = s_t + v * FLOW_COLS4, *cp = s_c + (v + dyi) * FLOW_PITCH + q;
                    uint32_t cw[QUADS + 1];
#pragma unroll
                    for (uint32_t j = 0; j < QUADS; j++) cw[j] = cp[u0 + j];
                    for (uint32_t u = u0; u < u1; u++) {
                        const uint32_t t = tp[u];
                        const uint32_t m = (u == u0 ? mf : 0xFFFFFFFFu) & (u + 1u == u1 ? ml : 0xFFFFFFFFu);
                        cw[QUADS] = cp[u + QUADS];
                        if (m != 0xFFFFFFFFu) {
#pragma unroll
                            for (uint32_t j = 0; j < QUADS; j++) shift_sad4(cw[j], cw[j + 1u], t, m, sum[j]);
                        } else {
#pragma unroll
                            for (uint32_t j = 0; j < QUADS; j++) {
                                const unsigned long long cc = (unsigned long long)cw[j + 1u] << 32 | cw[j];
                                acc[j] = __builtin_amdgcn_qsad_pk_u16_u8(cc, t, acc[j]);
                            }
                        }
#pragma unroll
                        for (uint32_t j = 0; j < QUADS; j++) cw[j] = cw[j + 1u];
                    }
                    pending += u1 - u0;
                    if (pending + (u1 - u0) > SHIFT_FOLD) {
#pragma unroll
                        for (uint32_t j = 0; j < QUADS; j++) {
#pragma unroll
                            for (uint32_t k = 0; k < 4u; k++) sum[j][k] += shift_field(acc[j], k);
                            acc[j] = 0ull;
                        }
                        pending = 0u;
                    }
                }
                uint32_t *surf = s_sad + cl * n + dyi * D;
#pragma unroll
                for (uint32_t j = 0; j < QUADS; j++)
#pragma unroll
                    for (uint32_t k = 0; k < 4u; k++) {
                        const uint32_t dxi = 4u * (q + j) + k, s = sum[j][k] + shift_field(acc[j], k);
                        if (dxi < D && s) region_lds_add(&surf[dxi], s);
                    }
            }
            __syncthreads();

            /* per cell the smallest (SAD, dx^2 + dy^2, dy, dx) as one key; then how many displacements share its SAD */
            for (uint32_t c0 = 0; c0 < gn; c0 += CPP) {
                const uint32_t cl = c0 + seg;
                const bool valid = cl < gn;
                const uint32_t *surf = s_sad + (valid ? cl : 0u) * n;
                unsigned long long key = ~0ull;
                for (uint32_t i = sub; valid && i < n; i += LPC) {
                    const uint32_t dyi = (i * magic) >> 16, dxi = i - dyi * D;
                    key = min(key, shift_key(surf[i], dxi, dyi, R));
                }
                for (uint32_t d = LPC >> 1; d; d >>= 1) key = min(key, (unsigned long long)__shfl_xor(key, (int)d));
                const uint32_t best = shift_key_best(key);
                uint32_t ties = 0u;
                for (uint32_t i = sub; valid && i < n; i += LPC) ties += surf[i] == best ? 1u : 0u;
                for (uint32_t d = LPC >> 1; d; d >>= 1) ties += __shfl_xor(ties, (int)d);
                if (valid && sub == 0u) {
                    const uint32_t c = g0 + cl;
                    s_out[0][c] = shift_key_dx(key, R);
                    s_out[1][c] = shift_key_dy(key, R);
                    s_out[2][c] = best;
                    s_out[3][c] = surf[R * D + R];
                    s_out[4][c] = ties;
                }
            }
        }
    }
    __syncthreads();

    /* the rectangle's cells inside the grid, map by map */
    const size_t map_words = (size_t)a.rows * a.cols;
    for (uint32_t t = tid; t < ncell; t += 256u) {
        const uint32_t i = t / nj, j = t - i * nj;
        uint32_t *out = it.dst + (size_t)(i0 + i) * a.cols + (j0 + j);
        if (planes & 1u) {
            const int cx0 = max(rx0, rectx + (int)j * cell), cx1 = min(rx1, rectx + (int)(j + 1u) * cell);
            const int cy0 = max(ry0, recty + (int)i * cell), cy1 = min(ry1, recty + (int)(i + 1u) * cell);
            *out = it.x1 > it.x0 && it.y1 > it.y0 && cx1 > cx0 && cy1 > cy0 ? (uint32_t)(cx1 - cx0) * (uint32_t)(cy1 - cy0) : 0u;
            out += map_words;
        }
#pragma unroll
        for (uint32_t q = 0; q < 5u; q++) {
            if (!(planes & (2u << q))) continue;
            *out = s_out[q][t];
            out += map_words;
        }
    }
}

} // namespace h264k
