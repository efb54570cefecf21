/* kernels/k_dbk.hip.h — k_dbk: boundary strengths and threshold values -> 48-byte deblocking records.  Part of kernels.hip.h (which see); not a stand-alone header. */
#pragma once
namespace h264k {
/* Boundary strengths (8.7.2.1) + threshold values from metadata only; ONE MACROBLOCK PER LANE, 64 entries of the picture's index list
 * per wavefront.  The strengths of a direction are sixteen nibbles in two dwords (nibble 4 * e + k = edge e, segment k: the record's
 * own order), made from the records' bit fields with shifts and masks, not segment by segment.
 * reference: GetBoundaryStrengths / GetLumaEdgeThresholds / GetChromaEdgeThresholds,
 * src/h264bsd_deblocking.c:1187-1541
 * (Until round 6 a macroblock took 16 lanes, one byte of the strength array each: the index walk, the record decode, the threshold
 * indices and the stores were paid per wavefront of four macroblocks — 46 vector + 17 scalar wave-instructions per listed macroblock,
 * and two macroblocks per wavefront had cost 1.7 times that.  Figures of this form: docs/EXPERIMENTS.md, "k_dbk: one macroblock per lane".) */
#ifndef DBK_WG_WAVES
#define DBK_WG_WAVES 8       /* wavefronts per workgroup of k_dbk (64 macroblocks each); the grid is sized by the tick's longest list.
                                1 / 2 / 4 / 8 wavefronts: 84.2 / 83.7 / 83.6 / 83.0 ms per step, 16 no better than 8 (one table fill and one
                                barrier per workgroup) */
#endif

/* ---- the packed pieces (plain C++: no lane exchange, no memory) ---- */
/* the sixteen luma "coded" bits of a record, H.264 block order (bit z_of(x, y)) -> raster order (bit 4 * y + x): bits 1 and 2 of the index change places */
__host__ __device__ __forceinline__ uint32_t dbk_raster16(uint32_t z) { return (z & 0xC3C3u) | ((z & 0x0C0Cu) << 2) | ((z & 0x3030u) >> 2); }
/* raster order -> column order (bit 4 * x + y): the transpose of a 4x4 bit matrix, inside its 2x2 blocks and then of the blocks */
__host__ __device__ __forceinline__ uint32_t dbk_transpose16(uint32_t r)
{
    uint32_t t = (r ^ (r >> 3)) & 0x0A0Au;
    r ^= t ^ (t << 3);
    t = (r ^ (r >> 6)) & 0x00CCu;
    return r ^ t ^ (t << 6);
}
/* eight bits -> the low bits of eight nibbles */
__host__ __device__ __forceinline__ uint32_t dbk_spread8(uint32_t b)
{
    b = (b | (b << 12)) & 0x000F000Fu;
    b = (b | (b << 6)) & 0x03030303u;
    return (b | (b << 3)) & 0x11111111u;
}
/* two vectors (x | y << 16, quarter samples) differ by 4 or more in a component */
__host__ __device__ __forceinline__ bool dbk_mv_differ(uint32_t a, uint32_t b)
{
    const int dx = (int)(int16_t)(a & 0xFFFFu) - (int)(int16_t)(b & 0xFFFFu), dy = ((int32_t)a >> 16) - ((int32_t)b >> 16);
    return (uint32_t)(dx + 3) > 6u || (uint32_t)(dy + 3) > 6u;
}
/* byte i of a ref_slot word differs from byte j of another */
__host__ __device__ __forceinline__ bool dbk_ref_differ(uint32_t a, int i, uint32_t b, int j) { return ((a >> (8 * i)) & 255u) != ((b >> (8 * j)) & 255u); }
/* where the references of the two sides of a segment differ, bit 4 * e + k: across the macroblock edge (e = 0, neighbour's references p)
 * and across the middle edge (e = 2) — edges 1 and 3 lie inside a quadrant.  dir 0: vertical edges, the left neighbour; dir 1: the upper one */
__host__ __device__ __forceinline__ uint32_t dbk_ref_bits(int dir, uint32_t q, uint32_t p)
{
    return dir == 0 ? (dbk_ref_differ(q, 0, p, 1) ? 0x0003u : 0u) | (dbk_ref_differ(q, 2, p, 3) ? 0x000Cu : 0u) |
                      (dbk_ref_differ(q, 1, q, 0) ? 0x0300u : 0u) | (dbk_ref_differ(q, 3, q, 2) ? 0x0C00u : 0u)
                    : (dbk_ref_differ(q, 0, p, 2) ? 0x0003u : 0u) | (dbk_ref_differ(q, 1, p, 3) ? 0x000Cu : 0u) |
                      (dbk_ref_differ(q, 2, q, 0) ? 0x0300u : 0u) | (dbk_ref_differ(q, 3, q, 1) ? 0x0C00u : 0u);
}
/* the segments at which motion is compared at all, bit 4 * e + k: the macroblock edge, and inside a macroblock only the partition
 * boundaries its type has (FJ_PARTS_*, reference deblocking.c:1266-1345) */
__host__ __device__ __forceinline__ uint32_t dbk_compared(int dir, int parts)
{
    return parts == FJ_PARTS_8x8 ? 0xFFFFu : parts == (dir ? FJ_PARTS_16x8 : FJ_PARTS_8x16) ? 0x0F0Fu : 0x000Fu;
}
/* The sixteen strengths of one direction as nibbles (x: edges 0, 1; y: edges 2, 3).  cq: the coded bits of the macroblock in the
 * direction's edge order (bit 4 * e + k); p_edge: those of the four neighbour blocks across the macroblock edge (bit k); motion: where
 * references or vectors differ AND motion is compared.  An intra side gives 3 inside and 4 on the macroblock edge, a coded block on
 * either side 2, differing motion 1. */
__host__ __device__ __forceinline__ uint2 dbk_dir_strengths(uint32_t cq, uint32_t p_edge, bool q_intra, bool p_intra, uint32_t motion, bool edge_on)
{
    uint32_t lo = 0x33334444u, hi = 0x33333333u;
    if (!q_intra) {
        const uint32_t two = (cq | (cq << 4) | p_edge) & 0xFFFFu, one = motion & ~two;
        lo = 2u * dbk_spread8(two & 255u) | dbk_spread8(one & 255u);
        hi = 2u * dbk_spread8(two >> 8) | dbk_spread8((one >> 8) & 255u);
        if (p_intra) lo = (lo & 0xFFFF0000u) | 0x4444u;
    }
    if (!edge_on) lo &= 0xFFFF0000u;
    return make_uint2(lo, hi);
}
/* where the vectors of the two sides of a segment differ, bit 4 * e + k, for both directions (x: dir 0, y: dir 1).  mq: the sixteen
 * vectors of the macroblock (raster), ml: those of the left neighbour's last column, mt: of the upper neighbour's last row */
__host__ __device__ __forceinline__ uint2 dbk_mv_bits(const uint32_t mq[16], const uint32_t ml[4], const uint32_t mt[4])
{
    uint32_t d0 = 0, d1 = 0;
#pragma unroll
    for (int e = 0; e < 4; e++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (dbk_mv_differ(mq[4 * k + e], e ? mq[4 * k + e - 1] : ml[k])) d0 |= 1u << (4 * e + k);
            if (dbk_mv_differ(mq[4 * e + k], e ? mq[4 * (e - 1) + k] : mt[k])) d1 |= 1u << (4 * e + k);
        }
    return make_uint2(d0, d1);
}

__global__ __launch_bounds__(64 * DBK_WG_WAVES) void k_dbk(const FrameDesc *__restrict__ frames)
{
    /* Tables 8-16 / 8-17 in LDS (alpha[64] | beta[64] | tc0[64] as dwords {bS 1, bS 2, bS 3, 0}): a lane-indexed __constant__
     * lookup is a global load */
    __shared__ uint32_t s_tab[32 + 64];
    const FrameDesc &fd = FD_REF(frames, blockIdx.y);
    const int wmb = fd.wmb;
    const uint32_t n_dbk = fd.n_dbk;
    /* the grid is as long as the tick's longest list: the workgroups behind the end of this picture's leave at once */
    if (blockIdx.x * (64u * DBK_WG_WAVES) >= n_dbk) return;
    const uint32_t di = blockIdx.x * (64u * DBK_WG_WAVES) + threadIdx.x;
    const bool live = di < n_dbk;                                  /* a lane behind the end of the list idles on macroblock 0 */
    const uint32_t mb = live ? fd.dbki[di] : 0u;
    const uint32_t mbx = mb - mb_row(fd, mb) * (uint32_t)wmb;
    const uint32_t mbl = mbx ? mb - 1 : mb, mbt = mb >= (uint32_t)wmb ? mb - wmb : mb;    /* in-picture stand-ins */
    /* the lane's record and the records of its left and upper neighbours as whole 16-byte pieces, requested TOGETHER and before
     * anything is looked at, whether the flags in the record (still in flight) will want them or not: two dependent memory round
     * trips per 64 macroblocks, a third for the vectors of partitioned macroblocks.  Neighbouring lanes mostly want neighbouring
     * records.  The tables are filled while the records travel. */
    FjMbRec q, pl, pt;
    {
        const H264K_GLOBAL uint8_t *rq = (const H264K_GLOBAL uint8_t *)(fd.recs + mb), *rl = (const H264K_GLOBAL uint8_t *)(fd.recs + mbl),
                                   *rt = (const H264K_GLOBAL uint8_t *)(fd.recs + mbt);
        uint4 w[6] = { ld16g(rq), ld16g(rq + 16), ld16g(rl), ld16g(rl + 16), ld16g(rt), ld16g(rt + 16) };
        if (threadIdx.x < 64) {
            const uint32_t t = threadIdx.x, ok = t < 52;
            reinterpret_cast<uint8_t *>(s_tab)[t] = ok ? c_alpha[t] : 0;
            reinterpret_cast<uint8_t *>(s_tab)[64 + t] = ok ? c_beta[t] : 0;
            s_tab[32 + t] = ok ? (uint32_t)c_tc0[t][0] | ((uint32_t)c_tc0[t][1] << 8) | ((uint32_t)c_tc0[t][2] << 16) : 0u;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 6; i++) asm volatile("" : "+v"(w[i].x), "+v"(w[i].y), "+v"(w[i].z), "+v"(w[i].w));
        __builtin_memcpy(&q, &w[0], 32); __builtin_memcpy(&pl, &w[2], 32); __builtin_memcpy(&pt, &w[4], 32);
    }
    if (__ballot(live) == 0ull) return;
    uint8_t *out = fd.dbk + (size_t)mb * DBK_REC_BYTES;
    uint8_t *any_out = fd.dbk + (size_t)fd.n_mbs * DBK_REC_BYTES + mb;
    const bool filtered = live && q.dbk && q.kind != FJ_MB_ABSENT;
    if (live && !filtered) { *reinterpret_cast<uint16_t *>(out + 46) = 0; *any_out = 0; }
    /* k_frame_dbk relies on it for its addresses: a left / upper macroblock edge is only ever active where that neighbour exists
     * (the host never says otherwise: GetMbFilteringFlags, deblocking.c:289-320 — enforced here for hand-built jobs) */
    const bool f_left = (q.dbk & FJ_DBK_LEFT) && mbx, f_top = (q.dbk & FJ_DBK_TOP) && mb >= (uint32_t)wmb;
    const bool q_intra = is_intra_kind(q.kind), l_intra = is_intra_kind(pl.kind), t_intra = is_intra_kind(pt.kind);
    /* motion vectors.  A macroblock with ONE vector carries it in its record (FJ_PRED_UNIFORM_MV: five of six — nothing more to
     * fetch, one comparison per macroblock edge and nothing inside); the others have their sixteen in the sparse section, one more
     * dependent round trip for the lanes that see such a macroblock on their own side or on a neighbour's — and for no lane where
     * the ballot finds none.  A side that is not an inter macroblock counts as one zero vector. */
    const bool q_inter = q.kind == FJ_MB_INTER, l_inter = pl.kind == FJ_MB_INTER, t_inter = pt.kind == FJ_MB_INTER;
    const uint32_t q_mv = q_inter ? (uint32_t)(uint16_t)q.mv[0] | ((uint32_t)(uint16_t)q.mv[1] << 16) : 0u;
    const uint32_t l_mv = l_inter ? (uint32_t)(uint16_t)pl.mv[0] | ((uint32_t)(uint16_t)pl.mv[1] << 16) : 0u;
    const uint32_t t_mv = t_inter ? (uint32_t)(uint16_t)pt.mv[0] | ((uint32_t)(uint16_t)pt.mv[1] << 16) : 0u;
    const bool compares = filtered && q_inter;                     /* (an intra side settles every strength before motion is looked at) */
    const bool q_many = compares && !(q.pred & FJ_PRED_UNIFORM_MV);
    const bool l_many = compares && f_left && l_inter && !(pl.pred & FJ_PRED_UNIFORM_MV);
    const bool t_many = compares && f_top && t_inter && !(pt.pred & FJ_PRED_UNIFORM_MV);
    uint2 mvd = make_uint2(dbk_mv_differ(q_mv, l_mv) ? 0x000Fu : 0u, dbk_mv_differ(q_mv, t_mv) ? 0x000Fu : 0u);
    if (__ballot(q_many || l_many || t_many) != 0ull) {
        if (q_many || l_many || t_many) {
            uint32_t mq[16], ml[4], mt[4];
#pragma unroll
            for (int i = 0; i < 16; i++) mq[i] = q_mv;
#pragma unroll
            for (int i = 0; i < 4; i++) { ml[i] = l_mv; mt[i] = t_mv; }
            if (q_many) {
                const H264K_GLOBAL uint8_t *v = (const H264K_GLOBAL uint8_t *)(fd.mvx + 32 * (size_t)q.mvx);
#pragma unroll
                for (int i = 0; i < 4; i++) { const uint4 r = ld16g(v + 16 * i); mq[4 * i] = r.x; mq[4 * i + 1] = r.y; mq[4 * i + 2] = r.z; mq[4 * i + 3] = r.w; }
            }
            if (l_many) {
                const H264K_GLOBAL uint32_t *v = (const H264K_GLOBAL uint32_t *)(fd.mvx + 32 * (size_t)pl.mvx);
#pragma unroll
                for (int i = 0; i < 4; i++) ml[i] = v[4 * i + 3];
            }
            if (t_many) {
                const uint4 r = ld16g((const H264K_GLOBAL uint8_t *)(fd.mvx + 32 * (size_t)pt.mvx) + 48);
                mt[0] = r.x; mt[1] = r.y; mt[2] = r.z; mt[3] = r.w;
            }
            mvd = dbk_mv_bits(mq, ml, mt);
        }
    }
    if (!filtered) return;
    uint32_t qrefs, lrefs, trefs;
    __builtin_memcpy(&qrefs, q.ref_slot, 4);
    __builtin_memcpy(&lrefs, pl.ref_slot, 4);
    __builtin_memcpy(&trefs, pt.ref_slot, 4);
    const int parts = (q.pred >> FJ_PRED_PARTS_SHIFT) & 3;
    const uint32_t cq1 = dbk_raster16(q.coded & 0xFFFFu), cq0 = dbk_transpose16(cq1);
    /* the neighbours' blocks along the edge: the left one's column 3 (z = 5, 7, 13, 15), the upper one's row 3 (z = 10, 11, 14, 15) */
    const uint32_t lc = pl.coded, tc = pt.coded;
    const uint32_t l_edge = ((lc >> 5) & 1u) | ((lc >> 6) & 2u) | ((lc >> 11) & 4u) | ((lc >> 12) & 8u);
    const uint32_t t_edge = ((tc >> 10) & 3u) | ((tc >> 12) & 12u);
    const uint2 s0 = dbk_dir_strengths(cq0, l_edge, q_intra, l_intra, (dbk_ref_bits(0, qrefs, lrefs) | mvd.x) & dbk_compared(0, parts), f_left);
    const uint2 s1 = dbk_dir_strengths(cq1, t_edge, q_intra, t_intra, (dbk_ref_bits(1, qrefs, trefs) | mvd.y) & dbk_compared(1, parts), f_top);
    /* scheduling flags of k_frame_dbk: does this macroblock touch its left / upper neighbour at all? (bytes 0,1 = left edge, 8,9 = upper) */
    const uint32_t left = s0.x & 0xFFFFu, top = s1.x & 0xFFFFu, inner = (s0.x >> 16) | s0.y | (s1.x >> 16) | s1.y;
    const bool any = (left | top | inner) != 0u;
    const uint32_t sched = (any ? DBKF_ANY : 0u) | (left ? DBKF_LEFT : 0u) | (top ? DBKF_TOP : 0u) | (inner ? DBKF_INNER : 0u);
    /* thresholds: indexA and indexB of the six classes (luma left / top / inner, chroma left / top / inner), alpha, beta and the three
     * tc0 looked up: a dword per class and its bS-3 byte */
    uint32_t thr[6], tc3[6];
#pragma unroll
    for (int c = 0; c < 6; c++) {
        const int side = c % 3;                                    /* 0: across the left edge, 1: across the upper edge, 2: inside */
        int a = (int)q.qp_y, b = side == 0 ? (int)pl.qp_y : side == 1 ? (int)pt.qp_y : (int)q.qp_y;
        if (c >= 3) {                                              /* chroma: QPc of both sides with the CURRENT macroblock's offset (deblocking.c:1501,1523) */
            a = qpc_of(clip3(0, 51, a + q.cqp_off));
            b = qpc_of(clip3(0, 51, b + q.cqp_off));
        }
        const int qpav = (a + b + 1) >> 1;
        const int ia = clip3(0, 51, qpav + q.alpha_off), ib = clip3(0, 51, qpav + q.beta_off);
        const uint32_t t = s_tab[32 + ia];
        thr[c] = (uint32_t)reinterpret_cast<const uint8_t *>(s_tab)[ia] | ((uint32_t)reinterpret_cast<const uint8_t *>(s_tab)[64 + ib] << 8) | ((t & 0xFFFFu) << 16);
        tc3[c] = (t >> 16) & 255u;
    }
    const uint32_t tail = (f_left ? FJ_DBK_LEFT : 0u) | (f_top ? FJ_DBK_TOP : 0u) | (q.dbk & FJ_DBK_INNER) | (any ? 0x100u : 0u);
    H264K_GLOBAL uint8_t *o = (H264K_GLOBAL uint8_t *)out;
    st16g(o, make_uint4(s0.x, s0.y, s1.x, s1.y));
    st16g(o + 16, make_uint4(thr[0], thr[1], thr[2], thr[3]));
    st16g(o + 32, make_uint4(thr[4], thr[5], tc3[0] | (tc3[1] << 8) | (tc3[2] << 16) | (tc3[3] << 24), tc3[4] | (tc3[5] << 8) | (tail << 16)));
    *any_out = (uint8_t)sched;
}

} // namespace h264k
