/* kernels/region_common.hip.h — what the picture-analysis kernels share: k_region_stats, k_region_change, k_region_shift and
 * k_cell_maps, which read boxes of current pictures from the macroblock tiles where they lie and write integer records.  Included by
 * engine.hip ahead of k_region_stats.hip.h; like its users, not part of the kernel sources that key the committed counter tables
 * (srchash.py).  Every piece is __forceinline__: the kernels' arithmetic stays in their own headers, and what they get from here is
 * the code they used to carry themselves.
 *     region_lds_add, stats_wave_sum          the LDS add without return; a wavefront's sum
 *     region_load                             a lane's four samples of every channel of a tile
 *     region_mask, REGION_MB_INNER            which of them lie in a rectangle; a macroblock that lies in the box whole
 *     region_band                             the macroblock rows of one of S row bands of a box
 *     region_hand_over, region_ticket_rezero  the one piece of ordering between workgroups of the family */
#pragma once
namespace h264k {

enum { ST_Y = 0, ST_YCBCR = 1, ST_RGB = 2 };

__device__ __forceinline__ void region_lds_add(uint32_t *p, uint32_t v)
{
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);      /* no return value used: ds_add_u32 */
}

template <class T> __device__ __forceinline__ T stats_wave_sum(T v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

/* the four samples of every channel of one lane's place in a tile, one per byte: lane l the luma dword of row l >> 2, columns
 * 4 (l & 3) .. + 3, and for the three-channel sources the two Cb and two Cr bytes under those four samples, expanded (ST_YCBCR) or
 * converted with the reference conversion (ST_RGB) */
template <int SRC>
__device__ __forceinline__ void region_load(const uint8_t *tile, uint32_t lane, uint32_t *v)
{
    v[0] = reinterpret_cast<const uint32_t *>(tile)[lane];
    if constexpr (SRC != ST_Y) {
        const uint32_t at = (lane >> 3) * 8u + (lane & 3u) * 2u;          /* chroma row (l >> 2) >> 1, columns 2 (l & 3), + 1 */
        const uint32_t cb2 = *reinterpret_cast<const uint16_t *>(tile + T_CB + at), cr2 = *reinterpret_cast<const uint16_t *>(tile + T_CR + at);
        if constexpr (SRC == ST_YCBCR) {
            v[1] = (cb2 & 255u) * 0x0101u | (cb2 >> 8) * 0x01010000u;
            v[2] = (cr2 & 255u) * 0x0101u | (cr2 >> 8) * 0x01010000u;
        } else {
            const uint32_t yv = v[0];
            v[0] = v[1] = v[2] = 0u;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                uint32_t px = yuv_pixel(0, (int)((yv >> (8 * k)) & 255u), (int)((cb2 >> (8 * (k >> 1))) & 255u), (int)((cr2 >> (8 * (k >> 1))) & 255u));
                /* the pixel is opaque from here on: seen through, the shift-and-clamp of two neighbours and their packing below were
                 * fused into one v_ashr_pk_u8_i32 in k_cell_maps (and nowhere else), whose results on the device differed from
                 * clip255(x >> 8) in a few samples per picture (docs/EXPERIMENTS.md, "Cell maps") */
                asm volatile("" : "+v"(px));
                v[0] |= (px & 255u) << (8 * k);
                v[1] |= ((px >> 8) & 255u) << (8 * k);
                v[2] |= ((px >> 16) & 255u) << (8 * k);
            }
        }
    }
}

/* 0xFF in the bytes of a lane's four samples (px .. px + 3, py) that lie in [x0, x1) x [y0, y1).  T: uint32_t, or int where the
 * rectangle's arithmetic is signed (k_cell_maps) */
template <class T>
__device__ __forceinline__ uint32_t region_mask(T px, T py, T x0, T y0, T x1, T y1)
{
    uint32_t m = 0u;
    if (py >= y0 && py < y1) {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (px + k >= x0 && px + k < x1) m |= 0xFFu << (8 * k);
    }
    return m;
}
/* the macroblock at (X, Y) lies whole in box ∩ window of item `it`: it needs no mask.  A macro, the one shared piece that is no
 * function: X and Y are wave-uniform, and the kernels' loops branch on the four comparisons one after the other; as an inlined function
 * they reach the loop combined into one condition, which changes the loops of all twelve k_region_stats and k_region_change kernels
 * (docs/EXPERIMENTS.md, "Picture-analysis pulls: one copy") */
#define REGION_MB_INNER(X, Y, it) ((X) >= (it).x0 && (X) + 16u <= (it).x1 && (Y) >= (it).y0 && (Y) + 16u <= (it).y1)

/* band `band` of S row bands over box ∩ window [x0, x1) x [y0, y1): the box's first macroblock, its macroblock columns and rows
 * (none when it is empty), and the macroblock rows r0 .. r1 - 1 that are the band's */
struct RegionBand { bool empty; uint32_t mbx0, mby0, cols, rows, r0, r1; };
__device__ __forceinline__ RegionBand region_band(uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, uint32_t band, uint32_t S)
{
    RegionBand b;
    b.empty = x1 <= x0 || y1 <= y0;
    b.mbx0 = x0 >> 4; b.mby0 = y0 >> 4;
    b.cols = b.empty ? 0u : ((x1 + 15u) >> 4) - b.mbx0;
    b.rows = b.empty ? 0u : ((y1 + 15u) >> 4) - b.mby0;
    b.r0 = b.mby0 + b.rows * band / S;
    b.r1 = b.mby0 + b.rows * (band + 1u) / S;
    return b;
}

/* The hand-over between the S row bands of region blockIdx.y, called by the whole workgroup behind its stores of a partial record to
 * the engine's scratch: every storing wavefront drains, one lane releases at device scope and takes the region's ticket (tickets: one
 * word per region, zero between launches); the band that draws the last ticket acquires, and all its lanes return true: they may read
 * the S partials with plain loads.  All integers behind it: the result does not depend on which band arrives last. */
__device__ __forceinline__ bool region_hand_over(uint32_t *tickets, uint32_t S)
{
    __shared__ uint32_t s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0u) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t t = __hip_atomic_fetch_add(&tickets[blockIdx.y], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = t == S - 1u ? 1u : 0u;
        if (t == S - 1u) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    return s_last != 0u;
}
/* by the band that drew the last ticket (last: false where a workgroup took none, S == 1), behind its stores of the record: the
 * region's ticket is zero again for the next launch */
__device__ __forceinline__ void region_ticket_rezero(uint32_t *tickets, bool last = true)
{
    if (last && threadIdx.x == 0u) __hip_atomic_store(&tickets[blockIdx.y], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

} // namespace h264k
