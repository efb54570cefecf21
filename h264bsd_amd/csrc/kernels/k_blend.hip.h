/* kernels/k_blend.hip.h — the kept pictures of many instances as a BACKGROUND MODEL: a running average of the current pictures with a
 * hold mask (h264bsdmiBlendCurrentPictures), and the kept pictures handed out as planar I420 (h264bsdmiOutputKeptPictures).  Included
 * by engine.hip behind k_keep.hip.h; like its siblings, not part of the kernel sources that key the committed counter tables
 * (srchash.py).
 *
 * The state of one sample is 16-bit fixed point, S = hi * 256 + lo: hi is the kept picture every consumer reads (k_region_change,
 * k_region_shift, k_cell_maps: unchanged), lo a second frame in the same tile layout.  With the current sample c, T = c * 256 + 128 and
 * a shift k in 0 .. 7,
 *     S' = S + ((T - S + ((1 << k) >> 1)) >> k)          an arithmetic shift of a 17-bit signed value, done in a 32-bit lane
 * k = 0 is S' = T.  S' lies between S and T, S stays in [128, 65408], and for constant input hi reaches c for every k <= 7.
 * A luma sample is MOVING when |c - hi| > hold (the values from before the update), a chroma sample when one of the four luma samples
 * it covers is.  Still samples take `shift`, moving ones `moving_shift`, or are left as they are (frozen).  All of it is integer and
 * exact; no result depends on scheduling.
 *
 * k_blend, grid (chunks, items) x 256: ONE launch for the batch.  A lane owns 2 luma rows x 8 columns of a tile — two 8-byte pieces,
 * 16 bytes apart — and the 4 Cb and 4 Cr samples under them: the chroma gate needs no other lane.  16 lanes per tile, four tiles per
 * wavefront, 16 per workgroup and step.  Lane l of a tile takes luma rows 2 (l >> 1), + 1 at columns 8 (l & 1), and chroma row l >> 1
 * at columns 4 (l & 1): a lane pair reads a 32-byte sector of luma with its two loads, and the 16 lanes read the 64 bytes of either
 * chroma block as consecutive dwords.  Every byte of the three frames is read once and every byte of the two state frames written
 * once: 5 frame sizes of traffic (3 when the model starts: hi and lo are not read).
 * The moving luma samples of an instance are counted per lane, summed per workgroup (wavefront sum, LDS) and added with one integer
 * atomic per workgroup to moving[slot], which the host zeroes on the stream ahead of the launch.
 *
 * k_kept_out, grid (chunks, items) x 256: k_detile for a batch, tiles -> planar I420, of hi and (where asked for) of lo — 0x80 where the
 * instance's lo is not valid. */
#pragma once
namespace h264k {

constexpr uint32_t BLEND_MAX_CHUNKS = 256;      /* workgroups per item */
constexpr uint32_t BLEND_FROZEN = 8u;           /* BlendArgs.moving_shift: moving samples are left as they are (H264BSDMI_BLEND_FROZEN) */
enum { BLEND_LO_UNSET = 1u,                     /* BlendItem.flags: lo holds nothing yet, read it as 0x80 (a plain keep came last) */
       BLEND_FRESH = 2u };                      /* no kept picture yet: S = T, nothing is moving */
/* bytes: the frame's, a multiple of 384; the three frames are 8-byte aligned; slot: the instance's word of BlendArgs.moving */
struct BlendItem { const uint8_t *cur; uint8_t *hi; uint8_t *lo; uint32_t bytes, flags, slot; };
struct BlendArgs { const BlendItem *items; uint32_t *moving; uint32_t shift, hold, moving_shift; };

/* 0xFF in the bytes of the four samples with |c - hi| > hold */
__device__ __forceinline__ uint32_t blend_moving4(uint32_t c, uint32_t hi, uint32_t hold)
{
    uint32_t m = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int d = (int)((c >> (8 * j)) & 255u) - (int)((hi >> (8 * j)) & 255u);
        if ((uint32_t)(d < 0 ? -d : d) > hold) m |= 0xFFu << (8 * j);
    }
    return m;
}
/* four samples updated: still ones (mv byte 0) with shift ks, moving ones with km, or not at all (frozen) */
__device__ __forceinline__ void blend4(uint32_t c, uint32_t mv, uint32_t ks, uint32_t km, bool frozen, uint32_t &hi, uint32_t &lo)
{
    uint32_t h = 0u, l = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const bool m = ((mv >> (8 * j)) & 1u) != 0u;
        const uint32_t k = m ? km : ks;
        const int S = (int)((((hi >> (8 * j)) & 255u) << 8) | ((lo >> (8 * j)) & 255u));
        const int T = (int)((((c >> (8 * j)) & 255u) << 8) | 128u);
        int d = (T - S + (int)((1u << k) >> 1)) >> k;
        if (frozen && m) d = 0;
        const uint32_t S2 = (uint32_t)(S + d);
        h |= (S2 >> 8) << (8 * j);
        l |= (S2 & 255u) << (8 * j);
    }
    hi = h; lo = l;
}

__global__ __launch_bounds__(256) void k_blend(const BlendArgs a)
{
    const BlendItem it = a.items[blockIdx.y];
    const uint32_t tiles = it.bytes / (uint32_t)TILE;
    const uint32_t sub = threadIdx.x & 15u;
    const uint32_t ya = (sub >> 1) * 32u + (sub & 1u) * 8u, ca = sub * 4u;
    const bool frozen = a.moving_shift == BLEND_FROZEN;
    const uint32_t ks = a.shift, km = frozen ? 0u : a.moving_shift;
    const bool fresh = (it.flags & BLEND_FRESH) != 0u, lo_unset = (it.flags & (BLEND_FRESH | BLEND_LO_UNSET)) != 0u;
    uint32_t count = 0u;
    for (uint32_t t = blockIdx.x * 16u + (threadIdx.x >> 4); t < tiles; t += gridDim.x * 16u) {
        const size_t at = (size_t)t * TILE;
        /* c, h, l: [0..1] the upper luma row's 8 samples, [2..3] the lower row's, [4] Cb, [5] Cr */
        uint32_t c[6], h[6], l[6];
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
        uint32_t mv[6];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            mv[q] = blend_moving4(c[q], h[q], a.hold);
            count += (uint32_t)__builtin_popcount(mv[q]) >> 3;
        }
        /* chroma sample j lies under luma columns 2 j, 2 j + 1 of both rows */
        const uint32_t left = mv[0] | mv[2], right = mv[1] | mv[3];
        mv[4] = ((left & 0xFFFFu) ? 0xFFu : 0u) | ((left >> 16) ? 0xFF00u : 0u) | ((right & 0xFFFFu) ? 0xFF0000u : 0u) | ((right >> 16) ? 0xFF000000u : 0u);
        mv[5] = mv[4];
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

/* one kept picture on its way out: hi and lo as they lie (lo NULL: not valid, 0x80 everywhere), the caller's planar buffers of
 * 384 wmb hmb bytes each (fraction NULL: not asked for), 16-byte aligned */
struct KeptOutItem { const uint8_t *hi; const uint8_t *lo; uint8_t *picture; uint8_t *fraction; uint32_t wmb, hmb; };

/* a 16-byte piece of a tile (a luma row, or two chroma rows) to its place in a planar I420 frame, as k_detile puts it */
__device__ __forceinline__ void kept_out_piece(uint8_t *d, const uint4 v, uint32_t i, uint32_t wmb, uint32_t hmb)
{
    const uint32_t W = wmb * 16u, CW = W >> 1;
    const size_t ysz = (size_t)W * hmb * 16u, csz = ysz >> 2;
    const uint32_t mb = i / (TILE / 16), pc = i % (TILE / 16), mbx = mb % wmb, mby = mb / wmb;
    if (pc < 16u) *reinterpret_cast<uint4 *>(d + (size_t)(mby * 16u + pc) * W + mbx * 16u) = v;
    else {
        const uint32_t plane = (pc - 16u) >> 2, r = ((pc - 16u) & 3u) * 2u;
        uint8_t *q = d + ysz + (plane ? csz : 0) + (size_t)(mby * 8u + r) * CW + mbx * 8u;
        *reinterpret_cast<uint2 *>(q) = make_uint2(v.x, v.y);
        *reinterpret_cast<uint2 *>(q + CW) = make_uint2(v.z, v.w);
    }
}

__global__ __launch_bounds__(256) void k_kept_out(const KeptOutItem *__restrict__ items)
{
    const KeptOutItem it = items[blockIdx.y];
    const uint32_t total = it.wmb * it.hmb * (TILE / 16);
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        kept_out_piece(it.picture, reinterpret_cast<const uint4 *>(it.hi)[i], i, it.wmb, it.hmb);
        if (it.fraction)
            kept_out_piece(it.fraction, it.lo ? reinterpret_cast<const uint4 *>(it.lo)[i] : make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u),
                           i, it.wmb, it.hmb);
    }
}

} // namespace h264k
