/* kernels/k_cell_maps.hip.h — dense per-cell maps of the quantities of k_region_stats (MODE 0, PICTURE), of k_region_change (MODE 1,
 * CHANGE), or of the change against the background spread (MODE 2, SPREAD: per sample and channel t = max(thr[c], V) with V the
 * instance's spread byte, then #(|d| > t), the sum of max(0, |d| - t) and the sum of V; a third frame read the same way) over a grid of square cells laid over a box (h264bsdmiOutputCellMaps): one u32 per cell and map, read from the macroblock
 * tiles where the pictures lie.  Included by engine.hip after k_region_change.hip.h, whose arithmetic per dword it uses, with the
 * loader and the mask of region_common.hip.h (region_load, region_mask); like them, not part of the kernel sources that key the committed counter tables (srchash.py).
 *
 * A slice: P maps of rows x cols u32, row-major: COUNT if asked, then per selected plane, in ascending bit order, C maps.
 * grid (rectangles of cells, regions) x 256.  A workgroup OWNS a rectangle of CELLS_RECT_W x CELLS_RECT_H luma samples of the grid,
 * (128 >> s) x (64 >> s) cells of side 1 << s, whose accumulators (at most 512 cells x 5 planes x 3 channels words, 30 KB) live in
 * its LDS.  Every cell belongs to exactly one workgroup: no scratch, no ticket, no hand-over between workgroups; a macroblock on a
 * rectangle's border is read by the two (or four) workgroups that share it, each masking what is not its own.
 * A wavefront takes one macroblock of its rectangle at a time and reads the tile as k_region_stats does: lane l the luma dword of
 * row l >> 2, columns 4 (l & 3) .. + 3, with the chroma under it, in CHANGE mode the same of the kept frame.  A byte mask (0xFF in the
 * bytes that count) says which of the four samples lie in box ∩ window ∩ rectangle; masked bytes are cleared in both pictures, so that
 * they add nothing, are no maximum and above no threshold, and are set to 255 for the minimum.
 * Because a cell is at least 4 wide a lane's four samples fall into at most two cells along x: the dword is cut at the first cell
 * boundary into part 0 and part 1, and each part is added to its cell with LDS adds, min and max without return.
 * QUAD (cells of 16 and more): the 16 samples of a macroblock row, too, straddle at most one boundary, so the cut is made per row,
 * the four lanes of a row are summed with two quad permutes and only the first commits: 16 lanes instead of 64 meet in one LDS
 * word.  A part that no lane of the wavefront has samples in is skipped altogether.
 * COUNT is closed form from the geometry and never accumulated.  After the barrier the rectangle's part of each selected map is
 * written with plain dword stores, consecutive lanes consecutive cells of a row; rectangles and cells of the grid that the box or the
 * window do not reach are written too (count 0, and PICTURE's minimum 255): the call owes the whole slice.
 * Planes that were not asked for are skipped by wave-uniform branches, not compiled out. */
#pragma once
namespace h264k {

constexpr uint32_t CELLS_RECT_W = 128, CELLS_RECT_H = 64;               /* luma samples of the grid per workgroup */
constexpr uint32_t CELLS_MAX_CELLS = (CELLS_RECT_W / 4) * (CELLS_RECT_H / 4);
constexpr uint32_t CELLS_MAX_GRID = 4096, CELLS_MAX_WORKGROUPS = 1u << 23;

/* one region: the two frames (kept: CHANGE and SPREAD only), the slice, the box's origin (ox, oy) in luma samples of the coded frame,
 * which may be negative or beyond the frame, box ∩ window [x0, x1) x [y0, y1) in the same (x1 <= x0: empty), and the spread frame of
 * the instance (SPREAD only) */
struct CellItem { const uint8_t *cur; const uint8_t *kept; uint32_t *dst; uint32_t wmb; int32_t ox, oy; uint32_t x0, y0, x1, y1; const uint8_t *spread; };
/* cols x rows cells of side 1 << shift per slice; rects_x: rectangles per row of rectangles; planes: H264BSDMI_CELL_* */
struct CellArgs { const CellItem *items; uint32_t cols, rows, shift, rects_x, planes, thr[3]; };

/* the value of lane ^ 1 / lane ^ 2: quad permutes [1, 0, 3, 2] and [2, 3, 0, 1] in the data path, no LDS round trip (every lane is
 * active where these are called) */
__device__ __forceinline__ uint32_t cells_xor1(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true); }
__device__ __forceinline__ uint32_t cells_xor2(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true); }
template <bool QUAD> __device__ __forceinline__ uint32_t cells_row_sum(uint32_t v)
{
    if constexpr (QUAD) { v += cells_xor1(v); v += cells_xor2(v); }
    return v;
}
template <bool QUAD> __device__ __forceinline__ uint32_t cells_row_min(uint32_t v)
{
    if constexpr (QUAD) { v = min(v, cells_xor1(v)); v = min(v, cells_xor2(v)); }
    return v;
}
template <bool QUAD> __device__ __forceinline__ uint32_t cells_row_max(uint32_t v)
{
    if constexpr (QUAD) { v = max(v, cells_xor1(v)); v = max(v, cells_xor2(v)); }
    return v;
}
__device__ __forceinline__ void cells_lds_min(uint32_t *p, uint32_t v) { (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void cells_lds_max(uint32_t *p, uint32_t v) { (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

template <int MODE, int SRC, bool QUAD>
__global__ __launch_bounds__(256) void k_cell_maps(CellArgs a)
{
    constexpr int C = SRC == ST_Y ? 1 : 3, NP = MODE == 2 ? 3 : MODE ? 5 : 4;      /* planes per channel, plane q is bit 2 << q */
    __shared__ uint32_t s_acc[CELLS_MAX_CELLS * NP * C];                    /* [channel][plane][cell row][cell column] */
    const CellItem it = a.items[blockIdx.y];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t cs = a.shift, planes = a.planes;
    const int cell = 1 << cs;
    const uint32_t RW = CELLS_RECT_W >> cs, RH = CELLS_RECT_H >> cs, ncell = RW * RH;
    const uint32_t j0 = (blockIdx.x % a.rects_x) * RW, i0 = (blockIdx.x / a.rects_x) * RH;           /* the first cell of the rectangle */
    const uint32_t nj = min(RW, a.cols - j0), ni = min(RH, a.rows - i0);                             /* its cells inside the grid */
    const uint32_t thr[3] = { a.thr[0], a.thr[1], a.thr[2] };
    for (uint32_t i = tid; i < ncell * NP * C; i += 256u) s_acc[i] = MODE == 0 && (i / ncell) % NP == 2u ? 255u : 0u;
    __syncthreads();

    /* box ∩ window ∩ rectangle, in luma samples of the coded frame */
    const bool empty = it.x1 <= it.x0 || it.y1 <= it.y0;
    const int rx0 = max((int)it.x0, it.ox + (int)j0 * cell), rx1 = min((int)it.x1, it.ox + (int)(j0 + nj) * cell);
    const int ry0 = max((int)it.y0, it.oy + (int)i0 * cell), ry1 = min((int)it.y1, it.oy + (int)(i0 + ni) * cell);
    if (!empty && rx1 > rx0 && ry1 > ry0) {
        const uint32_t mbx0 = (uint32_t)rx0 >> 4, mby0 = (uint32_t)ry0 >> 4;
        const uint32_t mcols = (((uint32_t)rx1 + 15u) >> 4) - mbx0, mrows = (((uint32_t)ry1 + 15u) >> 4) - mby0, n = mcols * mrows;
        const int col4 = (int)(lane & 3u) * 4, row = (int)(lane >> 2);
        for (uint32_t i = wave; i < n; i += 4u) {
            const uint32_t mby = mby0 + i / mcols, mbx = mbx0 + i % mcols;
            const size_t at = ((size_t)mby * it.wmb + mbx) * TILE;
            const int px = (int)mbx * 16 + col4, py = (int)mby * 16 + row;
            const uint32_t m = region_mask(px, py, rx0, ry0, rx1, ry1);
            /* the cut: the first cell boundary behind `from` (the row's first sample, or this lane's); part 0 before it, part 1 from it on */
            const int from = QUAD ? (int)mbx * 16 : px, ub = from - it.ox;
            const int cut = min(max(from + cell - (ub & (cell - 1)) - px, 0), 4);
            const uint32_t first = cut >= 4 ? 0xFFFFFFFFu : (1u << (8 * cut)) - 1u;
            const uint32_t pm[2] = { m & first, m & ~first };
            const uint32_t at0 = (uint32_t)(((py - it.oy) >> cs) - (int)i0) * RW + (uint32_t)((ub >> cs) - (int)j0);      /* part 0's cell */
            bool commit[2], part[2];                                        /* part: some lane of the wavefront has samples in it */
#pragma unroll
            for (int p = 0; p < 2; p++) {
                uint32_t any = pm[p];
                if constexpr (QUAD) { any |= cells_xor1(any); any |= cells_xor2(any); }
                commit[p] = any != 0u && (!QUAD || !(lane & 3u)) && at0 + (uint32_t)p < ncell;
                part[p] = __builtin_amdgcn_ballot_w64(pm[p] != 0u) != 0ull;
            }
            uint32_t va[C], vb[C];
            region_load<SRC>(it.cur + at, lane, va);
            if constexpr (MODE >= 1) region_load<SRC>(it.kept + at, lane, vb);
            [[maybe_unused]] uint32_t vv[C];
            if constexpr (MODE == 2) region_load<SRC>(it.spread + at, lane, vv);
#pragma unroll
            for (int c = 0; c < C; c++) {
                const uint32_t base = (uint32_t)c * NP * ncell + at0;      /* (at0 may be one before its row: only at0 + 1 is used then) */
#pragma unroll
                for (int p = 0; p < 2; p++) {
                    if (!part[p]) continue;                                 /* (wave-uniform: an aligned grid has no part 1 at all) */
                    uint32_t *acc = s_acc + (base + (uint32_t)p);
                    const uint32_t av = va[c] & pm[p];
                    if constexpr (MODE == 0) {
                        if (planes & 2u) {
                            const uint32_t s = cells_row_sum<QUAD>(__builtin_amdgcn_udot4(av, 0x01010101u, 0u, false));
                            if (commit[p]) region_lds_add(acc, s);
                        }
                        if (planes & 4u) {
                            const uint32_t q = cells_row_sum<QUAD>(__builtin_amdgcn_udot4(av, av, 0u, false));
                            if (commit[p]) region_lds_add(acc + ncell, q);
                        }
                        if (planes & 8u) {
                            const uint32_t lo4 = va[c] | ~pm[p];
                            const uint32_t lo = cells_row_min<QUAD>(min(min(lo4 & 255u, (lo4 >> 8) & 255u), min((lo4 >> 16) & 255u, lo4 >> 24)));
                            if (commit[p]) cells_lds_min(acc + 2u * ncell, lo);
                        }
                        if (planes & 16u) {
                            const uint32_t hi = cells_row_max<QUAD>(max(max(av & 255u, (av >> 8) & 255u), max((av >> 16) & 255u, av >> 24)));
                            if (commit[p]) cells_lds_max(acc + 3u * ncell, hi);
                        }
                    } else if constexpr (MODE == 1) {
                        const uint32_t bv = vb[c] & pm[p];
                        uint32_t ad = 0u, hi = 0u, ab = 0u;
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const int x = (int)((av >> (8 * k)) & 255u), y = (int)((bv >> (8 * k)) & 255u);
                            const uint32_t d = (uint32_t)(x > y ? x - y : y - x);
                            ad |= d << (8 * k);
                            hi = max(hi, d);
                            ab += d > thr[c] ? 1u : 0u;
                        }
                        if (planes & 2u) {
                            const uint32_t s = cells_row_sum<QUAD>(__builtin_amdgcn_udot4(ad, 0x01010101u, 0u, false));
                            if (commit[p]) region_lds_add(acc, s);
                        }
                        if (planes & 4u) {
                            const uint32_t q = cells_row_sum<QUAD>(__builtin_amdgcn_udot4(ad, ad, 0u, false));
                            if (commit[p]) region_lds_add(acc + ncell, q);
                        }
                        if (planes & 8u) {                                      /* the signed sum, modulo 2^32 */
                            const uint32_t g = cells_row_sum<QUAD>(__builtin_amdgcn_udot4(av, 0x01010101u, 0u, false) - __builtin_amdgcn_udot4(bv, 0x01010101u, 0u, false));
                            if (commit[p]) region_lds_add(acc + 2u * ncell, g);
                        }
                        if (planes & 16u) {
                            hi = cells_row_max<QUAD>(hi);
                            if (commit[p]) cells_lds_max(acc + 3u * ncell, hi);
                        }
                        if (planes & 32u) {
                            ab = cells_row_sum<QUAD>(ab);
                            if (commit[p]) region_lds_add(acc + 4u * ncell, ab);
                        }
                    } else {                                                /* SPREAD: the threshold of a sample is max(thr[c], V) */
                        const uint32_t bv = vb[c] & pm[p], sv = vv[c] & pm[p];
                        uint32_t fore = 0u, excess = 0u;
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const int x = (int)((av >> (8 * k)) & 255u), y = (int)((bv >> (8 * k)) & 255u);
                            const uint32_t d = (uint32_t)(x > y ? x - y : y - x), t = max(thr[c], (sv >> (8 * k)) & 255u);
                            fore += d > t ? 1u : 0u;
                            excess += d > t ? d - t : 0u;
                        }
                        if (planes & 2u) {
                            fore = cells_row_sum<QUAD>(fore);
                            if (commit[p]) region_lds_add(acc, fore);
                        }
                        if (planes & 4u) {
                            excess = cells_row_sum<QUAD>(excess);
                            if (commit[p]) region_lds_add(acc + ncell, excess);
                        }
                        if (planes & 8u) {
                            const uint32_t g = cells_row_sum<QUAD>(__builtin_amdgcn_udot4(sv, 0x01010101u, 0u, false));
                            if (commit[p]) region_lds_add(acc + 2u * ncell, g);
                        }
                    }
                }
            }
        }
    }
    __syncthreads();

    /* the rectangle's cells inside the grid, map by map */
    const size_t map_words = (size_t)a.rows * a.cols;
    for (uint32_t t = tid; t < ni * nj; t += 256u) {
        const uint32_t i = t / nj, j = t % nj;
        uint32_t *out = it.dst + (size_t)(i0 + i) * a.cols + (j0 + j);
        if (planes & 1u) {
            uint32_t count = 0u;
            if (!empty) {
                const int cx0 = max((int)it.x0, it.ox + (int)(j0 + j) * cell), cx1 = min((int)it.x1, it.ox + (int)(j0 + j + 1u) * cell);
                const int cy0 = max((int)it.y0, it.oy + (int)(i0 + i) * cell), cy1 = min((int)it.y1, it.oy + (int)(i0 + i + 1u) * cell);
                if (cx1 > cx0 && cy1 > cy0) count = (uint32_t)(cx1 - cx0) * (uint32_t)(cy1 - cy0);
            }
            *out = count;
            out += map_words;
        }
#pragma unroll
        for (int q = 0; q < NP; q++) {
            if (!(planes & (2u << q))) continue;
#pragma unroll
            for (int c = 0; c < C; c++) {
                *out = s_acc[((uint32_t)c * NP + (uint32_t)q) * ncell + i * RW + j];
                out += map_words;
            }
        }
    }
}

} // namespace h264k
