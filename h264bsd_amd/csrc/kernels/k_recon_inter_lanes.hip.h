/* kernels/k_recon_inter_lanes.hip.h — k_recon_inter_lb and k_recon_inter_lq: the inter macroblocks with one motion vector (the first part of the
 * general-inter list) and with one vector per 8x8 quadrant (the second part), a 4x4 block per lane; k_recon_inter (k_recon_inter.hip.h) takes the
 * finer partitions.  Both kernels sort a chunk of the list by interpolation class, stage the reference windows of a group of slots in LDS and then
 * run kernels/inter_lane_block.hip.h; the steps they share — counting sort, coefficient-block load, window staging, luma and chroma from the staged
 * windows, residual — come first in this file, once.  Part of kernels.hip.h (which see); not a stand-alone header. */
#pragma once
namespace h264k {
/* ------------------------------------------------------------------ the steps k_recon_inter_lb and k_recon_inter_lq share */
/* The counting sort of a chunk: bin[r] = the bin 0..9 of this lane's item in round r of 64 items (10: no item) -> rank[r] = its place in the
 * chunk ordered by bin, stably.  The histogram is ten ballots per round, the ranks are prefix counts of them. */
template <int ROUNDS>
__device__ __forceinline__ void lb_sort_ranks(const int bin[ROUNDS], uint32_t rank[ROUNDS])
{
    uint32_t seen = 0;
#pragma unroll
    for (int r = 0; r < ROUNDS; r++) rank[r] = 0;
#pragma unroll
    for (int k = 0; k < 10; k++)
#pragma unroll
        for (int r = 0; r < ROUNDS; r++) {
            const unsigned long long m = __ballot(bin[r] == k);
            const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (bin[r] == k) rank[r] = seen + before;
            seen += (uint32_t)__popcll(m);
        }
}
/* The lane's coefficient blocks: luma block z (H.264 block order), chroma block k8 = 4 * plane + block, the four DC levels of chroma plane
 * dc_plane — 32 + 32 + 8 bytes, zero where `coded` has no such block (the load then reads the first bytes of slot 0 and drops them).
 * cf = the coefficient section, coef_word = the list entry's coef_idx word. */
__device__ __forceinline__ void lb_coef_load(const H264K_GLOBAL uint8_t *cf, const H264K_GLOBAL uint8_t *ref0, uint32_t coef_word, uint32_t coded, int z, int k8,
                                             int dc_plane, uint32_t yl[8], uint32_t cl[8], uint32_t dcl[2])
{
    const uint32_t cidx = FJ_GEN_COEF_IDX(coef_word), nl = (uint32_t)__popc(coded & 0xFFFFu), has_cdc = (coded >> 25) & 1u;
    const bool ybit = (coded >> z) & 1u, cbit = (coded >> (16 + k8)) & 1u;
    const uint32_t yoff = 32u * (cidx + (uint32_t)__popc(coded & ((1u << z) - 1u)));
    const uint32_t coff = 32u * (cidx + nl + has_cdc + (uint32_t)__popc((coded >> 16) & ((1u << k8) - 1u)));
    const uint32_t doff = 32u * (cidx + nl) + 8u * (uint32_t)dc_plane;
    const H264K_GLOBAL uint8_t *py = ybit ? cf + yoff : ref0, *pc = cbit ? cf + coff : ref0, *pd = has_cdc ? cf + doff : ref0;
    const uint4 y0 = ld16g(py), y1 = ld16g(py + 16), c0 = ld16g(pc), c1 = ld16g(pc + 16);
    const uint2 d0 = ld8g(pd);
    const uint32_t ym = ybit ? ~0u : 0u, cm = cbit ? ~0u : 0u, dm = has_cdc ? ~0u : 0u;
    yl[0] = y0.x & ym; yl[1] = y0.y & ym; yl[2] = y0.z & ym; yl[3] = y0.w & ym; yl[4] = y1.x & ym; yl[5] = y1.y & ym; yl[6] = y1.z & ym; yl[7] = y1.w & ym;
    cl[0] = c0.x & cm; cl[1] = c0.y & cm; cl[2] = c0.z & cm; cl[3] = c0.w & cm; cl[4] = c1.x & cm; cl[5] = c1.y & cm; cl[6] = c1.z & cm; cl[7] = c1.w & cm;
    dcl[0] = d0.x & dm; dcl[1] = d0.y & dm;
}
/* Window staging (the pieces, their numbering and the edge rule: LaneWin in kernels/inter_lane_block.hip.h).  Lane j of a slot whose luma
 * window begins at (xi, yi) and whose chroma windows begin at (cxi, cyi) fetches its pieces with lane_window_load — every address clamped
 * into the picture; a lane without a piece, or of a slot that is off, reads the first bytes of slot 0 and drops them — and, once every other
 * global load of the group has been issued behind them, lays them out with lane_window_store at lw, rows of WSTRIDE / CSTRIDE bytes.
 * Windows that leave the picture need no gather: the piece from the clamped tile and row is spread after it arrived (lw_side). */
template <class WIN>
struct LanePieces {
    uint4 vl[WIN::NL];
    uint2 vc[WIN::NC];
    bool l_on[WIN::NL], c_on[WIN::NC];
};
template <class WIN>
__device__ __forceinline__ void lane_window_load(const H264K_GLOBAL uint8_t *ref0, uint32_t refoff, int wmb, int W, int H, bool on, int j, int xi, int yi,
                                                 int cxi, int cyi, LanePieces<WIN> &pcs)
{
    const int xs = (xi >> 4) << 4, cxs = (cxi >> 3) << 3;                            /* first column of the window's first tile */
#pragma unroll
    for (int i = 0; i < WIN::NL; i++) {
        const int p = j + WIN::LANES * i, lr = WIN::luma_row(p), lk = WIN::luma_tile(p);
        pcs.l_on[i] = on && WIN::luma_piece(p) && WIN::tile_needed(lk, xi - xs);
        const uint32_t off = refoff + lw_luma_piece(wmb, W, H, xs + 16 * lk, yi + lr);
        pcs.vl[i] = ld16g(ref0 + (pcs.l_on[i] ? off : 0u));
    }
#pragma unroll
    for (int i = 0; i < WIN::NC; i++) {
        const int p = j + WIN::LANES * i;
        pcs.c_on[i] = on && WIN::chroma_piece(p);
        const uint32_t off = refoff + lw_chroma_piece(wmb, WIN::chroma_plane(p), W >> 1, H >> 1, cxs + 8 * WIN::chroma_tile(p), cyi + WIN::chroma_row(p));
        pcs.vc[i] = ld8g(ref0 + (pcs.c_on[i] ? off : 0u));
    }
}
template <class WIN, int WSTRIDE, int CSTRIDE>
__device__ __forceinline__ void lane_window_store(uint8_t *lw, int W, int H, bool on, int j, int xi, int yi, int cxi, int cyi, LanePieces<WIN> &pcs)
{
    const int xs = (xi >> 4) << 4, cxs = (cxi >> 3) << 3, CW = W >> 1, CH = H >> 1;
    const bool lfast = xi >= 0 && xi + WIN::COLS <= W && yi >= 0 && yi + WIN::ROWS <= H;
    const bool cfast = cxi >= 0 && cxi + WIN::CROWS <= CW && cyi >= 0 && cyi + WIN::CROWS <= CH;
    if (__ballot(on && !(lfast && cfast)) != 0ull) {                                  /* wave-uniform: some window of the group leaves the picture */
#pragma unroll
        for (int i = 0; i < WIN::NL; i++) {
            const int side = lw_side(xs + 16 * WIN::luma_tile(j + WIN::LANES * i), W);
            const uint32_t first = (pcs.vl[i].x & 255u) * 0x01010101u, last = (pcs.vl[i].w >> 24) * 0x01010101u;
            if (side < 0) pcs.vl[i] = make_uint4(first, first, first, first);
            else if (side > 0) pcs.vl[i] = make_uint4(last, last, last, last);
        }
#pragma unroll
        for (int i = 0; i < WIN::NC; i++) {
            const int side = lw_side(cxs + 8 * WIN::chroma_tile(j + WIN::LANES * i), CW);
            const uint32_t first = (pcs.vc[i].x & 255u) * 0x01010101u, last = (pcs.vc[i].y >> 24) * 0x01010101u;
            if (side < 0) pcs.vc[i] = make_uint2(first, first);
            else if (side > 0) pcs.vc[i] = make_uint2(last, last);
        }
    }
#pragma unroll
    for (int i = 0; i < WIN::NL; i++) {
        const int p = j + WIN::LANES * i;
        if (pcs.l_on[i]) {
            uint32_t *d32 = reinterpret_cast<uint32_t *>(lw + WIN::luma_at(WSTRIDE, WIN::luma_row(p), WIN::luma_tile(p)));
            d32[0] = pcs.vl[i].x; d32[1] = pcs.vl[i].y; d32[2] = pcs.vl[i].z; d32[3] = pcs.vl[i].w;
        }
    }
#pragma unroll
    for (int i = 0; i < WIN::NC; i++) {
        const int p = j + WIN::LANES * i;
        if (pcs.c_on[i]) {
            uint32_t *d32 = reinterpret_cast<uint32_t *>(lw + WIN::chroma_at(WSTRIDE, CSTRIDE, WIN::chroma_plane(p), WIN::chroma_row(p), WIN::chroma_tile(p)));
            d32[0] = pcs.vc[i].x; d32[1] = pcs.vc[i].y;
        }
    }
}
/* The lane's 4x4 luma block from its staged window: src = window row 0 of the block (two rows above its first sample row) at the dword that holds window column 0, sh = 8 * (byte of that column in its dword), STRIDE = bytes per staged row.  cls = the
 * lane's interpolation class (-1: none); every class reads the rows and dwords it uses and runs under the mask of its lanes. */
template <int STRIDE>
__device__ __forceinline__ void lb_luma_from_lds(const uint8_t *src, int sh, int cls, int fx, int fy, s2 pl[4][2])
{
    auto row = [&](uint32_t rw[3], int r, int nd) {      /* dwords 0 .. nd - 1 of window row r */
        const uint32_t *q = reinterpret_cast<const uint32_t *>(src + r * STRIDE);
        uint32_t d[4];
#pragma unroll
        for (int k = 0; k < 4; k++) if (k <= nd) d[k] = q[k];
#pragma unroll
        for (int k = 0; k < 3; k++) rw[k] = k < nd ? (uint32_t)(((unsigned long long)d[k + 1] << 32 | d[k]) >> sh) : 0u;
    };
    if (cls == 0) {
        uint32_t rw[9][3] = {};
#pragma unroll
        for (int r = 2; r < 6; r++) row(rw[r], r, 2);
        lb_luma_whole(rw, pl);
    } else if (cls == 1) {
        uint32_t rw[9][3] = {};
#pragma unroll
        for (int r = 2; r < 6; r++) row(rw[r], r, 3);
        lb_luma_hor(rw, fx, pl);
    } else if (cls == 2) {
        uint32_t rw[9][3] = {};
#pragma unroll
        for (int r = 0; r < 9; r++) row(rw[r], r, 2);
        lb_luma_ver(rw, fy, pl);
    } else if (cls == 3) {
        uint32_t rw[9][3] = {};
#pragma unroll
        for (int r = 0; r < 9; r++) row(rw[r], r, (r >= 2 && r <= 6) ? 3 : 2);
        lb_luma_diag(rw, fx, fy, pl);
    } else if (cls == 4) {
        uint32_t rw[9][3] = {};
#pragma unroll
        for (int r = 0; r < 9; r++) row(rw[r], r, 3);
        lb_luma_centre(rw, fx, fy, pl);
    }
}
/* Two chroma rows of four samples from three staged rows of DW dwords: q = the first of them at the dword that holds the first sample,
 * ob & 3 = that sample's byte in it */
template <int DW>
__device__ __forceinline__ void lb_chroma_from_lds(const uint32_t *q, int ob, int cfx, int cfy, s2 pc[2][2])
{
    uint32_t lo[3], hi[3];
#pragma unroll
    for (int t = 0; t < 3; t++) {
        const uint32_t q0 = q[DW * t], q1 = q[DW * t + 1], q2 = q[DW * t + 2];
        lo[t] = __builtin_amdgcn_alignbyte(q1, q0, (uint32_t)(ob & 3)); hi[t] = __builtin_amdgcn_alignbyte(q2, q1, (uint32_t)(ob & 3));
    }
    const s2 w00 = as_s2((uint32_t)((8 - cfx) * (8 - cfy)) * 0x00010001u), w10 = as_s2((uint32_t)(cfx * (8 - cfy)) * 0x00010001u);
    const s2 w01 = as_s2((uint32_t)((8 - cfx) * cfy) * 0x00010001u), w11 = as_s2((uint32_t)(cfx * cfy) * 0x00010001u);
    lb_chroma_row(lo[0], hi[0], lo[1], hi[1], w00, w10, w01, w11, pc[0][0], pc[0][1]);
    lb_chroma_row(lo[1], hi[1], lo[2], hi[2], w00, w10, w01, w11, pc[1][0], pc[1][1]);
}
/* Residual add and clip: the lane's four luma rows (ldw) and the two rows 2 * half, 2 * half + 1 of its chroma block (cdw) as dwords.
 * yl, cl, dcl: the level blocks as loaded (zero where there is none), dci: the chroma block's place in its plane.  any_coded is wave-uniform,
 * and so is the choice of the 32-bit path: all lanes take it when one of them is FJ_CODED_WIDE (equal where 16 bits would do). */
__device__ __forceinline__ void lb_add_residual(const FrameDesc &fd, int lane, bool any_coded, uint32_t coded, int qp_y, int qp_c, const uint32_t yl[8],
                                                const uint32_t cl[8], const uint32_t dcl[2], int dci, int half, const s2 pl[4][2], const s2 pc[2][2],
                                                uint32_t ldw[4], uint32_t cdw[2])
{
    if (!any_coded) {                                                                /* the prediction as it is */
#pragma unroll
        for (int r = 0; r < 4; r++) ldw[r] = perm(as_u32(pl[r][1]), as_u32(pl[r][0]), 0x06040200u);
#pragma unroll
        for (int t = 0; t < 2; t++) cdw[t] = perm(as_u32(pc[t][1]), as_u32(pc[t][0]), 0x06040200u);
        return;
    }
    const int dc = lb_chroma_dc(dcl[0], dcl[1], dci, qp_c);
    if (__ballot((coded & FJ_CODED_WIDE) != 0u) == 0ull) {                            /* 16 bits hold every intermediate of every slot */
        uint32_t rr[4][4];
        lb_residual_pk(yl, cl, qp_y, qp_c, dc, rr);
        const s2 lo = pk(0), hi = pk(255);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const s2 l01 = pk_clip(lo, hi, pl[r][0] + as_s2(perm(rr[r][1], rr[r][0], 0x05040100u)));
            const s2 l23 = pk_clip(lo, hi, pl[r][1] + as_s2(perm(rr[r][3], rr[r][2], 0x05040100u)));
            ldw[r] = perm(as_u32(l23), as_u32(l01), 0x06040200u);
        }
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const uint32_t r0 = half ? rr[2 + t][0] : rr[t][0], r1 = half ? rr[2 + t][1] : rr[t][1];
            const uint32_t r2 = half ? rr[2 + t][2] : rr[t][2], r3 = half ? rr[2 + t][3] : rr[t][3];
            const s2 k01 = pk_clip(lo, hi, pc[t][0] + as_s2(perm(r1, r0, 0x07060302u)));
            const s2 k23 = pk_clip(lo, hi, pc[t][1] + as_s2(perm(r3, r2, 0x07060302u)));
            cdw[t] = perm(as_u32(k23), as_u32(k01), 0x06040200u);
        }
    } else {
        int ry[4][4], rc[4][4];
        const bool over_y = lb_residual_32(yl, qp_y, false, 0, ry), over_c = lb_residual_32(cl, qp_c, true, dc, rc);
        report_residual_range(fd, over_y || over_c, lane);
#pragma unroll
        for (int r = 0; r < 4; r++)
            ldw[r] = pack4(clip255(pl[r][0].x + ry[r][0]), clip255(pl[r][0].y + ry[r][1]), clip255(pl[r][1].x + ry[r][2]), clip255(pl[r][1].y + ry[r][3]));
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const int c0 = half ? rc[2 + t][0] : rc[t][0], c1 = half ? rc[2 + t][1] : rc[t][1], c2 = half ? rc[2 + t][2] : rc[t][2], c3 = half ? rc[2 + t][3] : rc[t][3];
            cdw[t] = pack4(clip255(pc[t][0].x + c0), clip255(pc[t][0].y + c1), clip255(pc[t][1].x + c2), clip255(pc[t][1].y + c3));
        }
    }
}
/* ------------------------------------------------------------------ the one-vector list, a 4x4 block per lane
 * A workgroup is ONE wavefront and takes INTER_LB_CHUNK consecutive entries of the picture's one-vector list.
 *   Binning.  Lane i reads entry i of the chunk and computes its bin, {not coded, coded} x {whole, hor, ver, diag, centre}; the counting
 *     sort lays the entries out in LDS ordered by bin.
 *   Groups.  The wavefront then works through the sorted chunk four entries at a time: lane = (slot 0..3, 4x4 luma block 0..15).
 *     Everything an entry decides — macroblock, vector, reference, window origin, quantisers, coded bits — is a per-lane value, so the
 *     scalar work and the address set-up of a macroblock are paid once for four.  Every interpolation class runs
 *     under the mask of the lanes that are in it (a wavefront-uniform skip when nobody is): a group of one bin pays for one class, a
 *     group that mixes bins (the remainders of a chunk) for each class it holds.  A slot past the end of the chunk idles: it loads
 *     from a fixed valid address, stages nothing and stores nothing.
 *   Staging.  Per slot one 21 x 48 luma and two 9 x 16 chroma windows (LbWin); the 16 lanes of a slot fetch its 63 + 36 aligned
 *     pieces (4 + 3 loads per lane), and with the coefficient blocks (32 bytes of luma block b, 32 bytes of chroma block b & 7, the 8
 *     DC bytes of its plane) all loads of all four slots are issued before the first is used.
 *   Arithmetic.  kernels/inter_lane_block.hip.h: the lane filters its block from a 9 x 12-byte window (9 window rows for 4 output
 *     rows, where a lane per row would fetch 6 each) and transforms its residual block without leaving its registers; lanes b and b + 8
 *     both transform chroma block b & 7 (in the high halves of the packed transform: it costs nothing) and keep two rows each.
 *   Stores.  A 4x4 dword transpose inside each quad of lanes (the four blocks of a block row) gives every lane one whole 16-byte row
 *     of the tile: one global_store_dwordx4 covers the four 256-byte luma tiles; neighbouring lanes swap a dword and store 8-byte
 *     chroma rows, 128 contiguous bytes per slot. */
#ifndef INTER_LB_CHUNK
#define INTER_LB_CHUNK 32    /* list entries per workgroup (= wavefront), a multiple of 4 up to 64 */
#endif
#ifndef INTER_LB_OCC
#define INTER_LB_OCC 4       /* wavefronts per SIMD the register budget is sized for (128 VGPRs): 16 macroblocks in flight per SIMD */
#endif
static_assert(INTER_LB_CHUNK % 4 == 0 && INTER_LB_CHUNK >= 4 && INTER_LB_CHUNK <= 64, "INTER_LB_CHUNK");
constexpr int IW_STRIDE = 52;                        /* bytes per staged luma row: 3 tiles x 16 bytes used, 13-dword stride */
constexpr int IC_STRIDE = 20;                        /* bytes per staged chroma row: 2 tiles x 8 bytes used */
/* A slot's windows: 21 luma rows at IW_STRIDE, then two planes of 9 chroma rows at IC_STRIDE (1452 bytes), padded to 368 dwords =
 * 16 (mod 32): the sixteen lanes of a slot read dword 13 * (4 * by + r) + bx + const — sixteen different banks of 32, {0..3, 8..11,
 * 20..23, 28..31} + const — and the other slot of the same half-wavefront the other sixteen when the two windows start at the same
 * dword of their tiles; otherwise they are up to 2-way.  Measured over the whole kernel (staging writes included):
 * SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 32.1 % (profiles/inter_lane_blocks_sq_counters.txt; the kernel before this one, a
 * macroblock per wavefront on the same strides, measured 48.8 %: profiles/r06_sq_counters.txt, docs/EXPERIMENTS.md). */
constexpr int LB_SLOT_LDS = 1472;
static_assert(LbWin::bytes(IW_STRIDE, IC_STRIDE) <= LB_SLOT_LDS, "a slot's windows");
constexpr int LB_LDS = INTER_LB_CHUNK * 16 + 4 * LB_SLOT_LDS;
__global__ __launch_bounds__(64, INTER_LB_OCC) void k_recon_inter_lb(const FrameDesc *__restrict__ frames)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[LB_LDS];
    const FrameDesc &fd = FD_REF(frames, blockIdx.y);
    const uint32_t bx_ = inter_unit_of_block();
    const uint32_t n_uni = fd.n_gen_uni, first = bx_ * INTER_LB_CHUNK;
    if (first >= n_uni) return;
    const uint32_t n_here = min(n_uni - first, (uint32_t)INTER_LB_CHUNK);            /* wave-uniform */
    const int lane = threadIdx.x & 63;
    const int wmb = fd.wmb, W = wmb * 16, H = fd.hmb * 16;
    const uint32_t frame_bytes = (uint32_t)wmb * fd.hmb * (uint32_t)TILE;            /* a stream's slots are contiguous (slot_ptr): at most 17 x 14 MB */
    const H264K_GLOBAL uint8_t *ref0 = (const H264K_GLOBAL uint8_t *)fd.slot[0];
    const H264K_GLOBAL uint8_t *cf = (const H264K_GLOBAL uint8_t *)fd.coefs;
    H264K_GLOBAL uint8_t *cur = (H264K_GLOBAL uint8_t *)fd.cur;

    /* ---- bin the chunk: lane i < n_here holds entry first + i ---- */
    {
        const bool have = (uint32_t)lane < n_here;
        uint4 e = make_uint4(0u, 0u, 0u, 0u);
        if (have) e = ld16g((const H264K_GLOBAL uint8_t *)fd.gen + 16u * (first + (uint32_t)lane));
        /* class first: a group that mixes classes runs a class pass more (110 .. 700 vector instructions), one that mixes coded and
         * not coded only gives its uncoded slots the residual pass (150) — coded first cost 8 class changes per chunk, this order 4 */
        const int bin[1] = { have ? 2 * lb_class_of((int)(e.y & 3u), (int)((e.y >> 16) & 3u)) + ((e.w & 0x03FFFFFFu) ? 1 : 0) : 10 };
        uint32_t rank[1];
        lb_sort_ranks<1>(bin, rank);
        if (have) *reinterpret_cast<uint4 *>(lds + 16u * rank[0]) = e;                /* rank < n_here */
        wave_sync();
    }

    /* The body below runs in four phases — loads and staging | luma | chroma | residual and store — and each of them derives what it
     * needs from the lane number and the four dwords of the list entry AGAIN (LB_FRESH makes them values of unknown origin): left to
     * itself the compiler computes every address of the body at its top and carries them, with the loop-invariant lane geometry, through
     * the centre-class filter, where the registers are needed (23 spilled VGPRs at 128). */
#define LB_FRESH() asm volatile("" : "+v"(ln), "+v"(ge.x), "+v"(ge.y), "+v"(ge.z), "+v"(ge.w))
#define LB_LANE() const int s = ln >> 4, b = ln & 15, bx = b & 3, by = b >> 2; \
                  uint8_t *lw = lds + INTER_LB_CHUNK * 16 + s * LB_SLOT_LDS; (void)bx; (void)by; (void)lw
#pragma unroll 1
    for (uint32_t g = 0; g < n_here; g += 4) {
        int ln = lane;
        const bool on = g + (uint32_t)(lane >> 4) < n_here;                           /* g + slot <= INTER_LB_CHUNK - 1 */
        uint4 ge = *reinterpret_cast<const uint4 *>(lds + 16u * (g + (uint32_t)(lane >> 4)));
        if (!on) ge = make_uint4(0u, 0u, 0u, 0u);
        uint32_t yl[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u }, cl[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u }, dcl[2] = { 0u, 0u };
        const bool any_coded = __ballot((ge.w & 0x03FFFFFFu) != 0u) != 0ull;          /* wave-uniform */
      {                                              /* ======== loads and staging: every global load of the group back to back, then the LDS stores ======== */
        LB_FRESH();
        LB_LANE();
        const uint32_t mb = ge.x & 0xFFFFu, refoff = (ge.x >> 24) * frame_bytes;
        const int mvx = (int16_t)(ge.y & 0xFFFFu), mvy = (int32_t)ge.y >> 16;
        const int mby = wmb == 1 ? (int)mb : (int)__umulhi(mb, fd.wmb_magic), mbx = (int)mb - mby * wmb;
        const int xi = mbx * 16 + (mvx >> 2) - 2, yi = mby * 16 + (mvy >> 2) - 2;
        const int cxi = mbx * 8 + (mvx >> 3), cyi = mby * 8 + (mvy >> 3);
        LanePieces<LbWin> pcs;
        lane_window_load<LbWin>(ref0, refoff, wmb, W, H, on, b, xi, yi, cxi, cyi, pcs);
        /* coefficient blocks: luma block b, chroma block k = b & 7, the DC levels of its plane */
        if (any_coded) lb_coef_load(cf, ref0, ge.z, ge.w, z_of(bx, by), b & 7, (b & 7) >> 2, yl, cl, dcl);
        lane_window_store<LbWin, IW_STRIDE, IC_STRIDE>(lw, W, H, on, b, xi, yi, cxi, cyi, pcs);
        wave_sync();
      }

        /* ======== luma: window rows 4 * by .. + 8, bytes o .. o + 11 with o = (xi - xs) + 4 * bx; each class reads the rows and dwords it
         * uses.  xi - xs = xi mod 16, and the macroblock's own 16 * mbx drops out of it ======== */
        s2 pl[4][2];
#pragma unroll
        for (int r = 0; r < 4; r++) pl[r][0] = pl[r][1] = pk(0);
        {
            LB_FRESH();
            LB_LANE();
            const int mvx = (int16_t)(ge.y & 0xFFFFu), mvy = (int32_t)ge.y >> 16;
            const int o = (((mvx >> 2) - 2) & 15) + 4 * bx, sh = 8 * (o & 3), fx = mvx & 3, fy = mvy & 3;
            const uint8_t *src = lw + 4 * by * IW_STRIDE + (o & ~3);
            lb_luma_from_lds<IW_STRIDE>(src, sh, on ? lb_class_of(fx, fy) : -1, fx, fy, pl);
        }
        /* ======== chroma: block k8 = 4 * plane + 2 * cby + cbx, rows 2 * half, 2 * half + 1 of it (cxi - cxs = cxi mod 8) ======== */
#define LB_CHROMA_LANE() const int k8 = b & 7, plane = k8 >> 2, cbx = k8 & 1, cby = (k8 >> 1) & 1, half = b >> 3; (void)cbx
        s2 pc[2][2];
        {
            LB_FRESH();
            LB_LANE();
            LB_CHROMA_LANE();
            const int mvx = (int16_t)(ge.y & 0xFFFFu), mvy = (int32_t)ge.y >> 16;
            const int ob = ((mvx >> 3) & 7) + 4 * cbx, cfx = mvx & 7, cfy = mvy & 7;
            const uint32_t *q = reinterpret_cast<const uint32_t *>(lw + LbWin::chroma_at(IW_STRIDE, IC_STRIDE, plane, cby * 4 + 2 * half, 0) + (ob & ~3));
            lb_chroma_from_lds<IC_STRIDE / 4>(q, ob, cfx, cfy, pc);
        }

        /* ======== residual add, clip: the lane's four luma rows and two chroma rows as dwords ======== */
        LB_FRESH();
        LB_LANE();
        LB_CHROMA_LANE();
        const uint32_t mb = ge.x & 0xFFFFu, coded = ge.w;
        const int qp_y = (int)FJ_GEN_QP_Y(ge.z), qp_c = (int)FJ_GEN_QP_C(ge.z);
        uint32_t ldw[4], cdw[2];
        lb_add_residual(fd, lane, any_coded, coded, qp_y, qp_c, yl, cl, dcl, k8 & 3, half, pl, pc, ldw, cdw);
        /* ---- store: after the transpose lane (by, bx) holds row 4 * by + bx of the tile, 16 bytes; lanes b, b ^ 1 hold the left and the right
         * half of two chroma rows, the even one takes the upper row whole, the odd one the lower ---- */
        quad_transpose4(ldw[0], ldw[1], ldw[2], ldw[3], ln);
        const uint32_t got = (uint32_t)quad_xor1((int)((b & 1) ? cdw[0] : cdw[1]));
        H264K_GLOBAL uint8_t *T = cur + (size_t)mb * TILE;
        if (on) {
            st16g(T + (4 * by + bx) * 16, make_uint4(ldw[0], ldw[1], ldw[2], ldw[3]));
            const u32x2 v = (b & 1) ? (u32x2){ got, cdw[1] } : (u32x2){ cdw[0], got };
            *(H264K_GLOBAL u32x2 *)(T + T_CB + plane * 64 + (cby * 4 + 2 * half + (b & 1)) * 8) = v;
        }
        wave_sync();          /* the staged windows are overwritten by the next group's */
    }
#undef LB_FRESH
#undef LB_LANE
#undef LB_CHROMA_LANE
}

/* ------------------------------------------------------------------ the quadrant list, a 4x4 block per lane
 * k_recon_inter_lq follows k_recon_inter_lb; what is sorted and assigned to lanes is the 8x8 QUADRANT, not the macroblock (the quadrants of a macroblock are in two
 * interpolation classes more often than in one: four macroblocks per group in list order would run four class passes per group).
 *   Binning.  A single-wavefront workgroup takes INTER_LQ_CHUNK consecutive entries of the quadrant part of the list.  Lane i fetches entry i,
 *     its four quadrant vectors (vectors 0, 2, 8, 10 of the sixteen in the sparse section) and the ref_slot dword of its record, and leaves
 *     them in LDS; in rounds of 64, lane j then makes the ITEM of quadrant j & 3 of entry 16 * round + (j >> 2) — four dwords laid out like a
 *     one-vector list entry: macroblock | quadrant << 16 | reference slot << 24, the vector, the coef_idx word, the coded word — and the
 *     counting sort (class first, then quadrant coded / not coded) lays the items out ordered by bin.  The sort is stable: the two quadrants of a 16x8 / 8x16 partition stay neighbours.
 *   Groups.  16 items at a time: lane = (slot 0..15, 4x4 luma block j = 0..3 of the quadrant, raster).  A slot past the end idles.
 *   Staging.  Per slot one 13 x 32 luma window and two 5 x 16 chroma windows (LqWin, rows packed); the four lanes of a slot fetch its
 *     26 + 20 aligned pieces (7 + 5 loads per lane) and their coefficient blocks (luma block z = 4 * quadrant + j, chroma block `quadrant`
 *     of plane j >> 1, that plane's DC levels), all before the first use.  Windows that leave the picture: the clamped tile row, spread.
 *   Arithmetic.  kernels/inter_lane_block.hip.h through the steps shared with k_recon_inter_lb; lanes 2 * plane, 2 * plane + 1 both transform
 *     the plane's chroma block and keep two rows each.
 *   Stores.  The two lanes of a block row swap two dwords: the left one stores rows 0, 1 of the pair of blocks, the right one rows 2, 3,
 *     8 bytes each; the chroma rows are 4 bytes wide. */
#ifndef INTER_LQ_CHUNK
#define INTER_LQ_CHUNK 8     /* list entries per workgroup (= wavefront), a multiple of 4 up to 64.  The step with 8 / 12 / 16 / 24 / 32 / 64: 77.4 / 77.5 / 78.0 /
                                78.5 / 79.1 / 80.5 ms (parent 81.2): a picture has at most 707 of these entries, and more and shorter wavefronts beat fewer class
                                passes; 4 (one group, nothing to sort) equals 8 within the spread (docs/EXPERIMENTS.md) */
#endif
#ifndef INTER_LQ_OCC
#define INTER_LQ_OCC 4       /* wavefronts per SIMD the register budget is sized for (128 VGPRs; the kernel takes 126).  With the strides below the LDS allows
                                as many: 16 wavefronts of 9.7 KB in a compute unit's 160 KB */
#endif
/* bytes per staged luma row (32 used) and chroma row (16 used).  Padded rows (36 / 20: 11.2 KB per wavefront, 14 per compute unit, 3 per SIMD
 * by the register budget) cost 0.5-0.6 ms per step against the tight rows, bank conflicts and all */
#ifndef INTER_LQ_WSTRIDE
#define INTER_LQ_WSTRIDE 32
#endif
#ifndef INTER_LQ_CSTRIDE
#define INTER_LQ_CSTRIDE 16
#endif
static_assert(INTER_LQ_CHUNK % 4 == 0 && INTER_LQ_CHUNK >= 4 && INTER_LQ_CHUNK <= 64, "INTER_LQ_CHUNK");
constexpr int LQ_ROUNDS = (INTER_LQ_CHUNK + 15) / 16;       /* sort rounds of 64 items */
constexpr int LQ_W_STRIDE = INTER_LQ_WSTRIDE, LQ_C_STRIDE = INTER_LQ_CSTRIDE;
static_assert(LQ_W_STRIDE >= 32 && LQ_W_STRIDE % 4 == 0 && LQ_C_STRIDE >= 16 && LQ_C_STRIDE % 4 == 0, "staged rows");
constexpr int LQ_SLOT_LDS = LqWin::bytes(LQ_W_STRIDE, LQ_C_STRIDE);
constexpr int LQ_ITEMS_LDS = INTER_LQ_CHUNK * 4 * 16;
constexpr int LQ_LDS = LQ_ITEMS_LDS + 16 * LQ_SLOT_LDS;
static_assert(INTER_LQ_CHUNK * 32 + LQ_ROUNDS * 64 <= 16 * LQ_SLOT_LDS, "the fetched entries lie where the windows will");
__global__ __launch_bounds__(64, INTER_LQ_OCC) void k_recon_inter_lq(const FrameDesc *__restrict__ frames)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[LQ_LDS];
    const FrameDesc &fd = FD_REF(frames, blockIdx.y);
    const uint32_t n_quad = fd.n_gen_quad, first = inter_unit_of_block() * INTER_LQ_CHUNK;
    if (first >= n_quad) return;
    const uint32_t n_here = min(n_quad - first, (uint32_t)INTER_LQ_CHUNK), n_items = 4u * n_here;      /* wave-uniform */
    const int lane = threadIdx.x & 63;
    const int wmb = fd.wmb, W = wmb * 16, H = fd.hmb * 16;
    const uint32_t frame_bytes = (uint32_t)wmb * fd.hmb * (uint32_t)TILE;
    const H264K_GLOBAL uint8_t *ref0 = (const H264K_GLOBAL uint8_t *)fd.slot[0];
    const H264K_GLOBAL uint8_t *cf = (const H264K_GLOBAL uint8_t *)fd.coefs;
    H264K_GLOBAL uint8_t *cur = (H264K_GLOBAL uint8_t *)fd.cur;

    /* ---- fetch: lane i < n_here holds entry n_gen_uni + first + i ---- */
    {
        uint4 *raw_e = reinterpret_cast<uint4 *>(lds + LQ_ITEMS_LDS), *raw_mv = raw_e + INTER_LQ_CHUNK;
        uint32_t *raw_ref = reinterpret_cast<uint32_t *>(raw_mv + INTER_LQ_CHUNK);
        if ((uint32_t)lane < n_here) {
            const uint4 e = ld16g((const H264K_GLOBAL uint8_t *)fd.gen + 16u * (fd.n_gen_uni + first + (uint32_t)lane));
            /* the entry's vector fields hold the index of the macroblock's sixteen vectors (x | y << 16 each, raster) in the sparse section */
            const H264K_GLOBAL uint32_t *mvc = (const H264K_GLOBAL uint32_t *)fd.mvx + 16 * (size_t)e.y;
            const uint32_t refs = *(const H264K_GLOBAL uint32_t *)((const H264K_GLOBAL uint8_t *)fd.recs + sizeof(FjMbRec) * (size_t)(e.x & 0xFFFFu) + offsetof(FjMbRec, ref_slot));
            raw_e[lane] = e;
            raw_mv[lane] = make_uint4(mvc[0], mvc[2], mvc[8], mvc[10]);
            raw_ref[lane] = refs;
        }
        wave_sync();
        /* ---- bin: item (round, lane j) = quadrant j & 3 of entry 16 * round + (j >> 2), so the item order is the list order ---- */
        uint4 it[LQ_ROUNDS];
        int bin[LQ_ROUNDS];
        bool have[LQ_ROUNDS];
#pragma unroll
        for (int r = 0; r < LQ_ROUNDS; r++) {
            const uint32_t ent = 16u * r + ((uint32_t)lane >> 2), q = (uint32_t)lane & 3u;
            have[r] = ent < n_here;
            const uint4 e = raw_e[ent], m4 = raw_mv[ent];
            const uint32_t mv = q == 0u ? m4.x : q == 1u ? m4.y : q == 2u ? m4.z : m4.w;
            it[r] = make_uint4((e.x & 0xFFFFu) | (q << 16) | (((raw_ref[ent] >> (8u * q)) & 255u) << 24), mv, e.z, e.w);
            bin[r] = have[r] ? 2 * lb_class_of((int)(mv & 3u), (int)((mv >> 16) & 3u)) + ((e.w & lq_coded_mask(q)) ? 1 : 0) : 10;
        }
        uint32_t rank[LQ_ROUNDS];
        lb_sort_ranks<LQ_ROUNDS>(bin, rank);
        wave_sync();
#pragma unroll
        for (int r = 0; r < LQ_ROUNDS; r++)
            if (have[r]) *reinterpret_cast<uint4 *>(lds + 16u * rank[r]) = it[r];     /* rank < n_items */
        wave_sync();
    }

    /* the four phases of k_recon_inter_lb's body, each deriving what it needs from the lane number and the item again (which see) */
#define LQ_FRESH() asm volatile("" : "+v"(ln), "+v"(ge.x), "+v"(ge.y), "+v"(ge.z), "+v"(ge.w))
#define LQ_LANE() const int s = ln >> 2, j = ln & 3, jbx = j & 1, jby = j >> 1, qd = (int)((ge.x >> 16) & 3u), plane = j >> 1, half = j & 1; \
                  uint8_t *lw = lds + LQ_ITEMS_LDS + s * LQ_SLOT_LDS; (void)jbx; (void)jby; (void)qd; (void)plane; (void)half; (void)lw
#pragma unroll 1
    for (uint32_t g = 0; g < n_items; g += 16) {
        int ln = lane;
        const bool on = g + (uint32_t)(lane >> 2) < n_items;                          /* g + slot <= 4 * INTER_LQ_CHUNK - 1 */
        uint4 ge = *reinterpret_cast<const uint4 *>(lds + 16u * (g + (uint32_t)(lane >> 2)));
        if (!on) ge = make_uint4(0u, 0u, 0u, 0u);
        uint32_t yl[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u }, cl[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u }, dcl[2] = { 0u, 0u };
        const bool any_coded = __ballot((ge.w & lq_coded_mask((ge.x >> 16) & 3u)) != 0u) != 0ull;       /* wave-uniform */
      {                                              /* ======== loads and staging: every global load of the group back to back, then the LDS stores ======== */
        LQ_FRESH();
        LQ_LANE();
        const uint32_t mb = ge.x & 0xFFFFu, refoff = (ge.x >> 24) * frame_bytes;
        const int mvx = (int16_t)(ge.y & 0xFFFFu), mvy = (int32_t)ge.y >> 16;
        const int mby = wmb == 1 ? (int)mb : (int)__umulhi(mb, fd.wmb_magic), mbx = (int)mb - mby * wmb;
        const int xi = mbx * 16 + 8 * (qd & 1) + (mvx >> 2) - 2, yi = mby * 16 + 8 * (qd >> 1) + (mvy >> 2) - 2;
        const int cxi = mbx * 8 + 4 * (qd & 1) + (mvx >> 3), cyi = mby * 8 + 4 * (qd >> 1) + (mvy >> 3);
        LanePieces<LqWin> pcs;
        lane_window_load<LqWin>(ref0, refoff, wmb, W, H, on, j, xi, yi, cxi, cyi, pcs);
        /* coefficient blocks: luma block z = 4 * quadrant + j (H.264 block order), chroma block `quadrant` of the lane's plane, its DC levels */
        if (any_coded) lb_coef_load(cf, ref0, ge.z, ge.w, 4 * qd + j, 4 * plane + qd, plane, yl, cl, dcl);
        lane_window_store<LqWin, LQ_W_STRIDE, LQ_C_STRIDE>(lw, W, H, on, j, xi, yi, cxi, cyi, pcs);
        wave_sync();
      }

        /* ======== luma: window rows 4 * jby .. + 8, bytes o .. o + 11 with o = xi mod 16 + 4 * jbx (the macroblock's own 16 * mbx drops out) ======== */
        s2 pl[4][2];
#pragma unroll
        for (int r = 0; r < 4; r++) pl[r][0] = pl[r][1] = pk(0);
        {
            LQ_FRESH();
            LQ_LANE();
            const int mvx = (int16_t)(ge.y & 0xFFFFu), mvy = (int32_t)ge.y >> 16;
            const int o = lq_window_byte(qd, mvx) + 4 * jbx, sh = 8 * (o & 3), fx = mvx & 3, fy = mvy & 3;
            const uint8_t *src = lw + 4 * jby * LQ_W_STRIDE + (o & ~3);
            lb_luma_from_lds<LQ_W_STRIDE>(src, sh, on ? lb_class_of(fx, fy) : -1, fx, fy, pl);
        }
        /* ======== chroma: 4x4 block `quadrant` of the lane's plane, rows 2 * half, 2 * half + 1 of it ======== */
        s2 pc[2][2];
        {
            LQ_FRESH();
            LQ_LANE();
            const int mvx = (int16_t)(ge.y & 0xFFFFu), mvy = (int32_t)ge.y >> 16;
            const int ob = lq_chroma_byte(qd, mvx), cfx = mvx & 7, cfy = mvy & 7;
            const uint32_t *q = reinterpret_cast<const uint32_t *>(lw + LqWin::chroma_at(LQ_W_STRIDE, LQ_C_STRIDE, plane, 2 * half, 0) + (ob & ~3));
            lb_chroma_from_lds<LQ_C_STRIDE / 4>(q, ob, cfx, cfy, pc);
        }

        /* ======== residual add, clip, exchange, store ======== */
        LQ_FRESH();
        LQ_LANE();
        const uint32_t mb = ge.x & 0xFFFFu, coded = ge.w;
        const int qp_y = (int)FJ_GEN_QP_Y(ge.z), qp_c = (int)FJ_GEN_QP_C(ge.z);
        uint32_t ldw[4], cdw[2];
        lb_add_residual(fd, lane, any_coded, coded, qp_y, qp_c, yl, cl, dcl, qd, half, pl, pc, ldw, cdw);
        uint32_t r0[2], r1[2];
        lq_pair_rows(ldw, (uint32_t)quad_xor1((int)(jbx ? ldw[0] : ldw[2])), (uint32_t)quad_xor1((int)(jbx ? ldw[1] : ldw[3])), jbx, r0, r1);
        H264K_GLOBAL uint8_t *T = cur + (size_t)mb * TILE;
        if (on) {
            H264K_GLOBAL uint8_t *L = T + lq_luma_store_offset(qd, j);
            *(H264K_GLOBAL u32x2 *)L = (u32x2){ r0[0], r0[1] };
            *(H264K_GLOBAL u32x2 *)(L + 16) = (u32x2){ r1[0], r1[1] };
            H264K_GLOBAL uint8_t *C = T + lq_chroma_store_offset(qd, j);
            *(H264K_GLOBAL uint32_t *)C = cdw[0];
            *(H264K_GLOBAL uint32_t *)(C + 8) = cdw[1];
        }
        wave_sync();          /* the staged windows are overwritten by the next group's */
    }
#undef LQ_FRESH
#undef LQ_LANE
}


} // namespace h264k
