/* kernels/k_cell_boxes.hip.h — the connected groups of cells of one map of a cell-map slice (k_cell_maps.hip.h) that pass a level, as
 * boxes (h264bsdmiOutputCellBoxes).  Included by engine.hip after k_cell_maps.hip.h, whose CellItem it reads; like it, not part of the
 * kernel sources that key the committed counter tables (srchash.py).
 *
 * grid (regions) x 256: ONE workgroup labels one slice of at most BOXES_MAX_CELLS cells, and everything it needs lives in its LDS as
 * plain 32-bit words — a label per cell (64 KiB), a counter per cell that is used at the roots (64 KiB) and the records (16 KiB): 144
 * of the compute unit's 160 KiB, which one workgroup may declare on this chip.  No global scratch, no hand-over between workgroups.
 * The steps, between which stand workgroup barriers whose number depends on nothing in the map:
 *   1  the map is read with consecutive lanes on consecutive cells; a cell is foreground when box ∩ window reaches it (the count of
 *      k_cell_maps above 0, from the same geometry) and its value passes the level.  Label: its own raster index, BOXES_NONE otherwise.
 *   2  in the same pass every cell is labelled with the first cell of its horizontal run inside its wavefront's window of 64 consecutive
 *      cells, from two ballots and no LDS traffic: the lockstep worst case of the next step, a chain as long as a row, cannot form.
 *   3  union–find over the labels, the SMALLER raster index as root: the first cell of a window is united with its left neighbour
 *      (a run that crosses the window's border), and a cell whose upper neighbour is foreground is united with it; with
 *      8 neighbours a cell whose upper neighbour is not is united with its upper-left and upper-right neighbours (were the upper one
 *      foreground they would lie in its run).  find shortens the path it walks (every label it stores is an ancestor: labels only
 *      ever point to smaller indices of the same set, so any interleaving terminates and is a valid forest); a root is hung under a
 *      smaller index with an LDS compare-and-swap, repeated from the new root when another lane was faster.  The root of a finished
 *      component is its smallest raster index, whatever the schedule.
 *   4  every cell stores its root (a read-only walk: no root moves any more), then counts itself at its root with an LDS add; a
 *      wavefront whose foreground cells share one root adds once.
 *   5  the roots are numbered in raster order: wavefront w owns quarter w of the raster, counts its surviving roots (cells >=
 *      min_cells) with ballots, the four counts meet in LDS, and a second walk gives every surviving root its number — which replaces
 *      its counter — and initialises the records of the first M.
 *   6  every foreground cell of a numbered component below M reduces into its record with integer LDS atomics: min / max for the
 *      rectangle in cells and the peak, a 64-bit add for the sum; a wavefront whose cells all go to one record reduces them in
 *      registers first and commits once.
 *   7  one lane per record turns the rectangle in cells into region coordinates clipped to box ∩ window; the header and the records go
 *      out with plain dword stores, consecutive lanes consecutive words, the records beyond `written` as zeros.
 * Everything is min, max or an integer sum, and the numbering is by raster order: no result depends on scheduling. */
#pragma once
namespace h264k {

constexpr uint32_t BOXES_MAX_CELLS = 16384, BOXES_MAX_BOXES = 512, BOXES_NONE = 0xFFFFFFFFu;

/* one region beside its CellItem: the boxes slice and the origin of the source window in luma samples of the coded frame (what a
 * region's coordinates are relative to) */
struct BoxItem { uint32_t *dst; int32_t wx, wy; };
/* map_off: the word offset of the chosen map inside a slice of the cell maps; sense 0: value > level, 1: value < level; conn 4 or 8 */
struct BoxArgs { const CellItem *items; const BoxItem *boxes; uint32_t cols, rows, shift, map_off, max_boxes, sense, level, conn, min_cells; };

__device__ __forceinline__ uint32_t boxes_ld(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void boxes_st(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
/* the root of i as far as it is known, shortening the path behind it */
__device__ __forceinline__ uint32_t boxes_find(uint32_t *lab, uint32_t i)
{
    uint32_t cur = boxes_ld(lab + i);
    if (cur != i) {
        uint32_t prev = i, next;
        while (cur > (next = boxes_ld(lab + cur))) { boxes_st(lab + prev, next); prev = cur; cur = next; }
    }
    return cur;
}
/* the root of i, nothing stored */
__device__ __forceinline__ uint32_t boxes_root(const uint32_t *lab, uint32_t i)
{
    uint32_t next;
    while (i > (next = boxes_ld(lab + i))) i = next;
    return i;
}
__device__ __forceinline__ void boxes_union(uint32_t *lab, uint32_t a, uint32_t b)
{
    a = boxes_find(lab, a); b = boxes_find(lab, b);
    while (a != b) {
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        uint32_t seen = a;                                              /* a, a root as far as this lane knows, under the smaller b */
        if (__hip_atomic_compare_exchange_strong(lab + a, &seen, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
        a = boxes_find(lab, seen);                                      /* another lane hung it elsewhere: go on from there */
    }
}

/* v of the first lane of `some` (a ballot, not empty) */
__device__ __forceinline__ uint32_t boxes_first(uint32_t v, unsigned long long some)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)v, __builtin_ctzll(some));
}
/* over the 64 lanes of a wavefront, all of them active; every lane gets the result */
__device__ __forceinline__ uint32_t boxes_wave_min(uint32_t v)
{
#pragma unroll
    for (int m = 32; m; m >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, m, 64));
    return v;
}
__device__ __forceinline__ uint32_t boxes_wave_max(uint32_t v)
{
#pragma unroll
    for (int m = 32; m; m >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, m, 64));
    return v;
}
__device__ __forceinline__ unsigned long long boxes_wave_sum(uint32_t v)
{
    unsigned long long s = v;
#pragma unroll
    for (int m = 32; m; m >>= 1) s += (unsigned long long)__shfl_xor((long long)s, m, 64);
    return s;
}
/* cells [c0, c1] x [r0, r1] with their peak and sum into a record that still holds jmin, imin, jmax, imax */
__device__ __forceinline__ void boxes_commit(uint32_t *rec, uint32_t c0, uint32_t r0, uint32_t c1, uint32_t r1, uint32_t peak, unsigned long long sum, bool below)
{
    cells_lds_min(rec, c0); cells_lds_min(rec + 1, r0); cells_lds_max(rec + 2, c1); cells_lds_max(rec + 3, r1);
    if (below) cells_lds_min(rec + 5, peak); else cells_lds_max(rec + 5, peak);
    (void)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(rec + 6), sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__global__ __launch_bounds__(256) void k_cell_boxes(BoxArgs a)
{
    __shared__ uint32_t s_lab[BOXES_MAX_CELLS];
    __shared__ uint32_t s_cnt[BOXES_MAX_CELLS];
    __shared__ __attribute__((aligned(8))) uint32_t s_rec[BOXES_MAX_BOXES * 8];
    __shared__ uint32_t s_wave[4], s_tot[2];                            /* surviving roots per wavefront; dropped roots, foreground cells */
    const CellItem it = a.items[blockIdx.x];
    const BoxItem bx = a.boxes[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t cols = a.cols, N = a.rows * cols, M = a.max_boxes;
    const int cell = 1 << a.shift;
    const uint32_t *map = it.dst + a.map_off;
    const bool empty = it.x1 <= it.x0 || it.y1 <= it.y0, below = a.sense != 0u;

    /* 1 and 2: foreground, and the run of each cell inside its wavefront's window of 64 consecutive cells, from two ballots: the run
     * starts one past the nearest background cell below the lane, or at the nearest first cell of a row at or below it, or with the window */
    for (uint32_t base = 0u; base < N; base += 256u) {                  /* (base and N are uniform: all 64 lanes are here) */
        const uint32_t i = base + tid;
        uint32_t c = 0u;
        bool fg = false;
        if (i < N) {
            const uint32_t r = i / cols;
            c = i - r * cols;
            const int cx0 = max((int)it.x0, it.ox + (int)c * cell), cx1 = min((int)it.x1, it.ox + (int)(c + 1u) * cell);
            const int cy0 = max((int)it.y0, it.oy + (int)r * cell), cy1 = min((int)it.y1, it.oy + (int)(r + 1u) * cell);
            const uint32_t v = map[i];
            fg = !empty && cx1 > cx0 && cy1 > cy0 && (below ? v < a.level : v > a.level);
            s_cnt[i] = 0u;
        }
        const unsigned long long fgm = __builtin_amdgcn_ballot_w64(fg), rowm = __builtin_amdgcn_ballot_w64(i < N && c == 0u);
        if (i < N) {
            const unsigned long long under = (1ull << lane) - 1ull, stops = ~fgm & under, firsts = rowm & (under | (1ull << lane));
            const uint32_t behind = stops ? 64u - (uint32_t)__builtin_clzll(stops) : 0u, first = firsts ? 63u - (uint32_t)__builtin_clzll(firsts) : 0u;
            s_lab[i] = fg ? i - lane + max(behind, first) : BOXES_NONE;
        }
    }
    for (uint32_t i = tid; i < BOXES_MAX_BOXES * 8u; i += 256u) s_rec[i] = 0u;
    if (tid < 2u) s_tot[tid] = 0u;
    __syncthreads();

    /* 3: the windows of a row are joined, and the rows */
    for (uint32_t i = tid; i < N; i += 256u) {
        if (boxes_ld(s_lab + i) == BOXES_NONE) continue;
        const uint32_t c = i % cols;
        if (lane == 0u && c && boxes_ld(s_lab + i - 1u) != BOXES_NONE) boxes_union(s_lab, i, i - 1u);
        if (i < cols) continue;
        const uint32_t up = i - cols;
        if (boxes_ld(s_lab + up) != BOXES_NONE) boxes_union(s_lab, i, up);
        else if (a.conn == 8u) {
            if (c && boxes_ld(s_lab + up - 1u) != BOXES_NONE) boxes_union(s_lab, i, up - 1u);
            if (c + 1u < cols && boxes_ld(s_lab + up + 1u) != BOXES_NONE) boxes_union(s_lab, i, up + 1u);
        }
    }
    __syncthreads();

    /* 4: roots and their cells (a lane stores to its own cell only: what another lane reads there is the old label or the root) */
    for (uint32_t base = 0u; base < N; base += 256u) {                  /* (base and N are uniform: all 64 lanes are here) */
        const uint32_t i = base + tid;
        uint32_t root = BOXES_NONE;
        if (i < N && boxes_ld(s_lab + i) != BOXES_NONE) {
            root = boxes_root(s_lab, i);
            boxes_st(s_lab + i, root);
        }
        const unsigned long long some = __builtin_amdgcn_ballot_w64(root != BOXES_NONE);
        if (!some) continue;
        const uint32_t first = boxes_first(root, some);
        if (__builtin_amdgcn_ballot_w64(root != BOXES_NONE && root != first) == 0ull) {
            if (lane == 0u) atomicAdd(s_cnt + first, (uint32_t)__builtin_popcountll(some));
        } else if (root != BOXES_NONE) atomicAdd(s_cnt + root, 1u);
    }
    __syncthreads();

    /* 5: numbers in raster order */
    const uint32_t quarter = (((N + 3u) >> 2) + 63u) & ~63u, q0 = min(wave * quarter, N), q1 = min(q0 + quarter, N);
    uint32_t survivors = 0u, dropped = 0u, fgc = 0u;
    for (uint32_t base = q0; base < q1; base += 64u) {
        const uint32_t i = base + lane;
        const bool is_root = i < q1 && s_lab[i] == i;
        const uint32_t n = is_root ? s_cnt[i] : 0u;
        survivors += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(is_root && n >= a.min_cells));
        dropped += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(is_root && n < a.min_cells));
        fgc += n;
    }
    if (lane == 0u) { s_wave[wave] = survivors; if (dropped) atomicAdd(s_tot, dropped); }
    if (fgc) atomicAdd(s_tot + 1, fgc);
    __syncthreads();
    uint32_t number = 0u, found = 0u;
    for (uint32_t w = 0u; w < 4u; w++) { const uint32_t n = s_wave[w]; found += n; if (w < wave) number += n; }
    const uint32_t written = min(found, M);
    for (uint32_t base = q0; base < q1; base += 64u) {
        const uint32_t i = base + lane;
        const bool is_root = i < q1 && s_lab[i] == i;
        const uint32_t n = is_root ? s_cnt[i] : 0u;
        const bool survives = is_root && n >= a.min_cells;
        const unsigned long long votes = __builtin_amdgcn_ballot_w64(survives);
        const uint32_t mine = number + (uint32_t)__builtin_popcountll(votes & ((1ull << lane) - 1ull));
        if (is_root) s_cnt[i] = survives && mine < M ? mine : BOXES_NONE;
        if (survives && mine < M) {
            uint32_t *rec = s_rec + mine * 8u;                          /* jmin, imin, jmax, imax for now */
            rec[0] = BOXES_NONE; rec[1] = BOXES_NONE; rec[2] = 0u; rec[3] = 0u; rec[4] = n; rec[5] = below ? BOXES_NONE : 0u;
        }
        number += (uint32_t)__builtin_popcountll(votes);
    }
    __syncthreads();

    /* 6: the records of the first M.  Atomics of many lanes on one LDS word are served one after the other, and the cells of a large
     * component all meet in one record: a wavefront whose foreground cells belong to ONE record reduces them in registers and lane 0
     * commits once (a run of a large component, the common case); mixed wavefronts, and those with a few cells only, go lane by lane */
    for (uint32_t base = 0u; base < N; base += 256u) {
        const uint32_t i = base + tid;
        uint32_t k = BOXES_NONE, r = 0u, c = 0u, v = 0u;
        if (i < N) {
            const uint32_t root = s_lab[i];
            if (root != BOXES_NONE) k = s_cnt[root];
        }
        const bool mine = k != BOXES_NONE;
        if (mine) { r = i / cols; c = i - r * cols; v = map[i]; }
        const unsigned long long some = __builtin_amdgcn_ballot_w64(mine);
        if (!some) continue;
        const uint32_t first = boxes_first(k, some);
        if (__builtin_popcountll(some) > 4 && __builtin_amdgcn_ballot_w64(mine && k != first) == 0ull) {
            const uint32_t c0 = boxes_wave_min(mine ? c : BOXES_NONE), r0 = boxes_wave_min(mine ? r : BOXES_NONE);
            const uint32_t c1 = boxes_wave_max(mine ? c : 0u), r1 = boxes_wave_max(mine ? r : 0u);
            const uint32_t peak = below ? boxes_wave_min(mine ? v : BOXES_NONE) : boxes_wave_max(mine ? v : 0u);
            const unsigned long long sum = boxes_wave_sum(mine ? v : 0u);
            if (lane == 0u) boxes_commit(s_rec + first * 8u, c0, r0, c1, r1, peak, sum, below);
        } else if (mine) boxes_commit(s_rec + k * 8u, c, r, c, r, v, v, below);
    }
    __syncthreads();

    /* 7: rectangles in region coordinates, then the slice */
    for (uint32_t k = tid; k < written; k += 256u) {
        uint32_t *rec = s_rec + k * 8u;
        const int x0 = max((int)it.x0, it.ox + (int)rec[0] * cell), x1 = min((int)it.x1, it.ox + (int)(rec[2] + 1u) * cell);
        const int y0 = max((int)it.y0, it.oy + (int)rec[1] * cell), y1 = min((int)it.y1, it.oy + (int)(rec[3] + 1u) * cell);
        rec[0] = (uint32_t)(x0 - bx.wx); rec[1] = (uint32_t)(y0 - bx.wy); rec[2] = (uint32_t)(x1 - x0); rec[3] = (uint32_t)(y1 - y0);
    }
    __syncthreads();
    if (tid < 8u) bx.dst[tid] = tid == 0u ? found : tid == 1u ? written : tid == 2u ? s_tot[1] : tid == 3u ? s_tot[0] : 0u;
    for (uint32_t i = tid; i < M * 8u; i += 256u) bx.dst[8u + i] = s_rec[i];
}

} // namespace h264k
