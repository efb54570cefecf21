/* kernels/k_blend_spread.hip.h — the background model with a per-sample noise level: k_blend's running average and hold mask, and beside
 * hi and lo a third frame in the same tile layout, the SPREAD V — one byte per sample that follows how much the sample usually differs
 * from its background — which the moving test then uses as its threshold (h264bsdmiBlendCurrentPicturesSpread).  Included by
 * engine.hip behind k_blend.hip.h, whose blend4, item flags and lane ownership it uses; like it, not part of the kernel sources that
 * key the committed counter tables (srchash.py).
 *
 * Per sample, with c, hi and V from before the call and d = |c - hi|:
 *     a luma sample is MOVING when d > max(hold, V); a chroma sample when one of the four luma samples it covers is (chroma V never gates)
 *     S is updated as k_blend updates it under that mask (blend4)
 *     A = min(255, gain d);  V' = clamp(V + sign(A - V), lowest, highest)         chroma with its own d
 * update 0: V stays; 1: every sample takes V'; 2: only samples that are not moving.  Where the instance's V is not valid
 * (BLEND_V_UNSET, and always where the model starts) it reads as `lowest` and is written whatever `update` says: the frame is valid
 * behind the launch.  All of it is integer and exact; no result depends on scheduling.
 *
 * k_blend_spread, grid (chunks, items) x 256: ONE launch for the batch, k_blend's ownership — a lane owns 2 luma rows x 8 columns of a
 * tile and the 4 Cb and 4 Cr samples under them, so the chroma gate needs no other lane.  Per lane and tile 6 more dwords are loaded
 * and 6 more stored than k_blend's: 7 frame sizes of traffic against 5.  With update 0 only the 4 luma dwords of V are loaded (chroma
 * V never gates) and none is stored: 5 + 2/3 frame sizes.
 * The bytes are stepped in place in their dwords: every operand is a byte select of a 32-bit register.
 * The moving luma samples are counted as in k_blend: per lane, wavefront sum, LDS, one integer atomic per workgroup. */
#pragma once
namespace h264k {

enum { BLEND_V_UNSET = 4u };                    /* SpreadItem.flags, beside BLEND_LO_UNSET and BLEND_FRESH: V holds nothing yet, read it as `lowest` */
enum { SPREAD_NONE = 0u, SPREAD_ALL = 1u, SPREAD_STILL = 2u };      /* SpreadArgs.update */
/* BlendItem and the spread frame v, `bytes` long and 8-byte aligned like the others */
struct SpreadItem { const uint8_t *cur; uint8_t *hi; uint8_t *lo; uint8_t *v; uint32_t bytes, flags, slot; };
struct SpreadArgs { const SpreadItem *items; uint32_t *moving; uint32_t shift, hold, moving_shift, gain, lowest, highest, update; };

/* 0xFF in the bytes of the four samples with |c - hi| > max(hold, V) */
__device__ __forceinline__ uint32_t spread_moving4(uint32_t c, uint32_t hi, uint32_t v, uint32_t hold)
{
    uint32_t m = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int d = (int)((c >> (8 * j)) & 255u) - (int)((hi >> (8 * j)) & 255u);
        if ((uint32_t)(d < 0 ? -d : d) > max(hold, (v >> (8 * j)) & 255u)) m |= 0xFFu << (8 * j);
    }
    return m;
}
/* four samples of V one step towards min(255, gain |c - hi|), clamped; the bytes of `stay` that are 0xFF keep their value */
__device__ __forceinline__ uint32_t spread_step4(uint32_t c, uint32_t hi, uint32_t v, uint32_t stay, uint32_t gain, uint32_t lowest, uint32_t highest)
{
    uint32_t out = v & stay;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int d = (int)((c >> (8 * j)) & 255u) - (int)((hi >> (8 * j)) & 255u);
        const uint32_t A = min(255u, gain * (uint32_t)(d < 0 ? -d : d)), V = (v >> (8 * j)) & 255u;
        const uint32_t V2 = min(max(V + (A > V ? 1u : 0u) - (A < V ? 1u : 0u), lowest), highest);     /* (V = 0 has A >= V: no borrow) */
        out |= (V2 << (8 * j)) & ~stay;
    }
    return out;
}

__global__ __launch_bounds__(256) void k_blend_spread(const SpreadArgs a)
{
    const SpreadItem it = a.items[blockIdx.y];
    const uint32_t tiles = it.bytes / (uint32_t)TILE;
    const uint32_t sub = threadIdx.x & 15u;
    const uint32_t ya = (sub >> 1) * 32u + (sub & 1u) * 8u, ca = sub * 4u;
    const bool frozen = a.moving_shift == BLEND_FROZEN;
    const uint32_t ks = a.shift, km = frozen ? 0u : a.moving_shift;
    const bool fresh = (it.flags & BLEND_FRESH) != 0u, lo_unset = (it.flags & (BLEND_FRESH | BLEND_LO_UNSET)) != 0u;
    const bool v_unset = (it.flags & (BLEND_FRESH | BLEND_V_UNSET)) != 0u;
    const uint32_t lowest4 = a.lowest * 0x01010101u;
    uint32_t count = 0u;
    for (uint32_t t = blockIdx.x * 16u + (threadIdx.x >> 4); t < tiles; t += gridDim.x * 16u) {
        const size_t at = (size_t)t * TILE;
        /* c, h, l, v: [0..1] the upper luma row's 8 samples, [2..3] the lower row's, [4] Cb, [5] Cr */
        uint32_t c[6], h[6], l[6], v[6];
        const uint2 c0 = *reinterpret_cast<const uint2 *>(it.cur + at + ya), c1 = *reinterpret_cast<const uint2 *>(it.cur + at + ya + 16u);
        c[0] = c0.x; c[1] = c0.y; c[2] = c1.x; c[3] = c1.y;
        c[4] = *reinterpret_cast<const uint32_t *>(it.cur + at + T_CB + ca);
        c[5] = *reinterpret_cast<const uint32_t *>(it.cur + at + T_CR + ca);
        if (fresh) {
#pragma unroll
            for (int q = 0; q < 6; q++) h[q] = c[q];
        } else {
            const uint2 h0 = *reinterpret_cast<const uint2 *>(it.hi + at + ya), h1 = *reinterpret_cast<const uint2 *>(it.hi + at + ya + 16u);
            h[0] = h0.x; h[1] = h0.y; h[2] = h1.x; h[3] = h1.y;
            h[4] = *reinterpret_cast<const uint32_t *>(it.hi + at + T_CB + ca);
            h[5] = *reinterpret_cast<const uint32_t *>(it.hi + at + T_CR + ca);
        }
        if (lo_unset) {
#pragma unroll
            for (int q = 0; q < 6; q++) l[q] = 0x80808080u;
        } else {
            const uint2 l0 = *reinterpret_cast<const uint2 *>(it.lo + at + ya), l1 = *reinterpret_cast<const uint2 *>(it.lo + at + ya + 16u);
            l[0] = l0.x; l[1] = l0.y; l[2] = l1.x; l[3] = l1.y;
            l[4] = *reinterpret_cast<const uint32_t *>(it.lo + at + T_CB + ca);
            l[5] = *reinterpret_cast<const uint32_t *>(it.lo + at + T_CR + ca);
        }
        if (v_unset) {
#pragma unroll
            for (int q = 0; q < 6; q++) v[q] = lowest4;
        } else {
            const uint2 v0 = *reinterpret_cast<const uint2 *>(it.v + at + ya), v1 = *reinterpret_cast<const uint2 *>(it.v + at + ya + 16u);
            v[0] = v0.x; v[1] = v0.y; v[2] = v1.x; v[3] = v1.y;
            if (a.update != SPREAD_NONE) {                  /* (chroma V never gates: without an update it is not read) */
                v[4] = *reinterpret_cast<const uint32_t *>(it.v + at + T_CB + ca);
                v[5] = *reinterpret_cast<const uint32_t *>(it.v + at + T_CR + ca);
            } else v[4] = v[5] = 0u;
        }
        uint32_t mv[6];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            mv[q] = spread_moving4(c[q], h[q], v[q], a.hold);
            count += (uint32_t)__builtin_popcount(mv[q]) >> 3;
        }
        /* chroma sample j lies under luma columns 2 j, 2 j + 1 of both rows */
        const uint32_t left = mv[0] | mv[2], right = mv[1] | mv[3];
        mv[4] = ((left & 0xFFFFu) ? 0xFFu : 0u) | ((left >> 16) ? 0xFF00u : 0u) | ((right & 0xFFFFu) ? 0xFF0000u : 0u) | ((right >> 16) ? 0xFF000000u : 0u);
        mv[5] = mv[4];
        if (a.update != SPREAD_NONE || v_unset) {           /* (the same for every lane of the workgroup) */
            if (a.update != SPREAD_NONE) {
#pragma unroll
                for (int q = 0; q < 6; q++) v[q] = spread_step4(c[q], h[q], v[q], a.update == SPREAD_STILL ? mv[q] : 0u, a.gain, a.lowest, a.highest);
            }
            *reinterpret_cast<uint2 *>(it.v + at + ya) = make_uint2(v[0], v[1]);
            *reinterpret_cast<uint2 *>(it.v + at + ya + 16u) = make_uint2(v[2], v[3]);
            *reinterpret_cast<uint32_t *>(it.v + at + T_CB + ca) = v[4];
            *reinterpret_cast<uint32_t *>(it.v + at + T_CR + ca) = v[5];
        }
#pragma unroll
        for (int q = 0; q < 6; q++) blend4(c[q], mv[q], ks, km, frozen, h[q], l[q]);
        *reinterpret_cast<uint2 *>(it.hi + at + ya) = make_uint2(h[0], h[1]);
        *reinterpret_cast<uint2 *>(it.hi + at + ya + 16u) = make_uint2(h[2], h[3]);
        *reinterpret_cast<uint32_t *>(it.hi + at + T_CB + ca) = h[4];
        *reinterpret_cast<uint32_t *>(it.hi + at + T_CR + ca) = h[5];
        *reinterpret_cast<uint2 *>(it.lo + at + ya) = make_uint2(l[0], l[1]);
        *reinterpret_cast<uint2 *>(it.lo + at + ya + 16u) = make_uint2(l[2], l[3]);
        *reinterpret_cast<uint32_t *>(it.lo + at + T_CB + ca) = l[4];
        *reinterpret_cast<uint32_t *>(it.lo + at + T_CR + ca) = l[5];
    }
    if (a.moving) {                                     /* (the same for every lane of the launch) */
        __shared__ uint32_t s_count;
        if (threadIdx.x == 0u) s_count = 0u;
        __syncthreads();
        count = stats_wave_sum(count);
        if ((threadIdx.x & 63u) == 0u && count) region_lds_add(&s_count, count);
        __syncthreads();
        if (threadIdx.x == 0u && s_count) (void)atomicAdd(&a.moving[it.slot], s_count);
    }
}

} // namespace h264k
