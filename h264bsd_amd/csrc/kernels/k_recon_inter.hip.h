/* kernels/k_recon_inter.hip.h — k_recon_inter: the inter macroblocks with partitions finer than 8x8 (interpolation, residual, write-back), one list
 * entry per wavefront, every lane's window straight from global memory; and what all three inter kernels share, the position of a workgroup in a
 * picture's list.  The one-vector and the quadrant part of the list are k_recon_inter_lb and k_recon_inter_lq (kernels/k_recon_inter_lanes.hip.h).
 * Part of kernels.hip.h (which see); not a stand-alone header. */
#pragma once
namespace h264k {
/* ------------------------------------------------------------------ inter prediction */
__device__ __forceinline__ int tap6(int a, int b, int c, int d, int e, int f) { return a - 5 * (b + e) + 20 * (c + d) + f; }

/* Register window of one lane: rows y-2..y+3, columns x-2..x+9 of the reference plane (9 columns used),
 * rw[r][k] = dword k of window row r, straight from global memory (clamp-to-edge on the slow path =
 * h264bsdFillBlock, src/h264bsd_reconstruct.c:2244). */
__device__ __forceinline__ void luma_window_global(const uint8_t *__restrict__ p, int wmb, int w, int h, int x, int y, uint32_t rw[6][3])
{
    if (x >= 2 && x + 9 < w && y >= 2 && y + 3 < h) {
#pragma unroll
        for (int r = 0; r < 6; r++) {
            rw[r][0] = luma4_at(p, wmb, x - 2, y - 2 + r); rw[r][1] = luma4_at(p, wmb, x + 2, y - 2 + r); rw[r][2] = luma4_at(p, wmb, x + 6, y - 2 + r);
        }
    } else {
#pragma unroll
        for (int r = 0; r < 6; r++) {
            const int yy = clip3(0, h - 1, y - 2 + r);
            uint32_t a = 0, b = 0, c = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                a |= (uint32_t)p[luma_at(wmb, clip3(0, w - 1, x - 2 + i), yy)] << (8 * i);
                b |= (uint32_t)p[luma_at(wmb, clip3(0, w - 1, x + 2 + i), yy)] << (8 * i);
            }
            c = (uint32_t)p[luma_at(wmb, clip3(0, w - 1, x + 6), yy)];
            rw[r][0] = a; rw[r][1] = b; rw[r][2] = c;
        }
    }
}

/* 4 luma samples (x..x+3, y) of the prediction at quarter-sample fraction (fx,fy) from the window (8.4.2.2.1) */
__device__ __forceinline__ void luma_from_window(const uint32_t rw[6][3], int fx, int fy, int out[4])
{
#define GW(r, c) ((int)((rw[(r)][(c) >> 2] >> (8 * ((c) & 3))) & 255u))
    if ((fx | fy) == 0) {                            /* G: whole-sample */
#pragma unroll
        for (int i = 0; i < 4; i++) out[i] = GW(2, i + 2);
        return;
    }
    /* The one-dimensional and diagonal classes run on PAIRS of output samples (packed 16-bit: a six-tap sum of bytes lies
     * in [-2550, 10710]).  CP(r, c) = (sample c, sample c+1) of window row r; the selectors are compile-time constants. */
#define CP(r, c) as_s2(perm(rw[(r)][((c) + 1) >> 2], rw[(r)][(c) >> 2], \
                      0x0C000C00u | (uint32_t)((c) & 3) | ((uint32_t)(((((c) + 1) >> 2) != ((c) >> 2)) ? 4 + (((c) + 1) & 3) : (((c) + 1) & 3)) << 16)))
#define HT2(r, i) (CP(r, i) + CP(r, (i) + 5) - pk(5) * (CP(r, (i) + 1) + CP(r, (i) + 4)) + pk(20) * (CP(r, (i) + 2) + CP(r, (i) + 3)))
#define VT2(c) (CP(0, c) + CP(5, c) - pk(5) * (CP(1, c) + CP(4, c)) + pk(20) * (CP(2, c) + CP(3, c)))
#define RND5(x) pk_clip(pk(0), pk(255), ((x) + pk(16)) >> pk(5))
    if (fy == 0) {                                   /* a, b, c: horizontal only (window row 2) */
        s2 o01 = RND5(HT2(2, 0)), o23 = RND5(HT2(2, 2));
        if (fx == 1) { o01 = (o01 + CP(2, 2) + pk(1)) >> pk(1); o23 = (o23 + CP(2, 4) + pk(1)) >> pk(1); }
        else if (fx == 3) { o01 = (o01 + CP(2, 3) + pk(1)) >> pk(1); o23 = (o23 + CP(2, 5) + pk(1)) >> pk(1); }
        out[0] = o01.x; out[1] = o01.y; out[2] = o23.x; out[3] = o23.y;
        return;
    }
    if (fx == 0) {                                   /* d, h, n: vertical only */
        s2 o01 = RND5(VT2(2)), o23 = RND5(VT2(4));
        if (fy == 1) { o01 = (o01 + CP(2, 2) + pk(1)) >> pk(1); o23 = (o23 + CP(2, 4) + pk(1)) >> pk(1); }
        else if (fy == 3) { o01 = (o01 + CP(3, 2) + pk(1)) >> pk(1); o23 = (o23 + CP(3, 4) + pk(1)) >> pk(1); }
        out[0] = o01.x; out[1] = o01.y; out[2] = o23.x; out[3] = o23.y;
        return;
    }
    if (fx != 2 && fy != 2) {                        /* e, g, p, r: average of the nearest horizontal and vertical half samples */
        s2 b01, b23, h01, h23;
        if (fy == 1) { b01 = HT2(2, 0); b23 = HT2(2, 2); } else { b01 = HT2(3, 0); b23 = HT2(3, 2); }
        if (fx == 1) { h01 = VT2(2); h23 = VT2(4); } else { h01 = VT2(3); h23 = VT2(5); }
        const s2 o01 = (RND5(b01) + RND5(h01) + pk(1)) >> pk(1), o23 = (RND5(b23) + RND5(h23) + pk(1)) >> pk(1);
        out[0] = o01.x; out[1] = o01.y; out[2] = o23.x; out[3] = o23.y;
        return;
    }
    /* vertical 6-tap sums at window columns 2..6 (sample columns x .. x+4): h and m candidates */
#define VH1(c) tap6(GW(0, c), GW(1, c), GW(2, c), GW(3, c), GW(4, c), GW(5, c))
#define HB1(r, i) tap6(GW(r, i), GW(r, (i) + 1), GW(r, (i) + 2), GW(r, (i) + 3), GW(r, (i) + 4), GW(r, (i) + 5))
    if (fx == 2 || fy == 2) {                        /* j, f, q, i, k */
        /* j is the 6-tap filter over un-rounded intermediate sums, and it may run over the vertical sums of nine columns
         * just as well as over the horizontal sums of six rows (8.4.2.2.1: both orders are equal): 9 + 4 filters
         * instead of 24 + 4, and the vertical sums are exactly what i / k need */
        int v1[9];
#pragma unroll
        for (int c = 0; c < 9; c++) v1[c] = VH1(c);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int j = clip255((tap6(v1[i], v1[i + 1], v1[i + 2], v1[i + 3], v1[i + 4], v1[i + 5]) + 512) >> 10);
            int v = j;
            if (fy != 2) {                           /* f / q: with b (row y) or s (row y+1) */
                const int b = clip255(((fy == 1 ? HB1(2, i) : HB1(3, i)) + 16) >> 5);
                v = (j + b + 1) >> 1;
            } else if (fx != 2) {                    /* i / k: with h (col x) or m (col x+1) */
                const int hh = clip255(((fx == 1 ? v1[i + 2] : v1[i + 3]) + 16) >> 5);
                v = (j + hh + 1) >> 1;
            }
            out[i] = v;
        }
        return;
    }
#undef VH1
#undef HB1
#undef GW
#undef CP
#undef HT2
#undef VT2
#undef RND5
}

/* 2 chroma samples from the two rows a[0..2], b[0..2] at eighth-sample fraction (fx,fy), 8.4.2.2.2 */
__device__ __forceinline__ void chroma_from_rows(const int a[3], const int b[3], int fx, int fy, int out[2])
{
    const int w00 = (8 - fx) * (8 - fy), w10 = fx * (8 - fy), w01 = (8 - fx) * fy, w11 = fx * fy;
    out[0] = (w00 * a[0] + w10 * a[1] + w01 * b[0] + w11 * b[1] + 32) >> 6;
    out[1] = (w00 * a[1] + w10 * a[2] + w01 * b[1] + w11 * b[2] + 32) >> 6;
}
/* 2 chroma samples (x, x+1 ; y) of plane `plane` straight from global memory (w, h: chroma plane size) */
__device__ __forceinline__ void chroma_pred2(const uint8_t *__restrict__ f, int wmb, int plane, int w, int h, int x, int y, int fx, int fy, int out[2])
{
    int a[3], b[3];
    const int y0 = clip3(0, h - 1, y), y1 = clip3(0, h - 1, y + 1);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int xx = clip3(0, w - 1, x + i);
        a[i] = f[chroma_at(wmb, plane, xx, y0)]; b[i] = f[chroma_at(wmb, plane, xx, y1)];
    }
    chroma_from_rows(a, b, fx, fy, out);
}

/* ------------------------------------------------------------------ a workgroup's place in the picture's list
 * The three inter kernels are grids of single-wavefront workgroups, (x, picture); workgroup x takes unit u of the picture's part of the
 * list — one entry in k_recon_inter, a chunk of entries in k_recon_inter_lb / _lq.  Workgroups are dealt to the eight XCDs round robin in
 * dispatch order (x fastest), and every XCD has its own L2: with u = x two neighbouring macroblocks — whose reference windows overlap —
 * never share an L2, and every 128-byte line a window touches is fetched from HBM by up to four XCDs (FETCH 1.31 GB per tick for 0.48 GB of
 * windows and coefficients, measured when one kernel walked the whole list an entry per workgroup).  INTER_XCD = 1 (default): the
 * workgroups x = c (mod 8) of a picture — one XCD's — take the c-th contiguous eighth of the units, i.e. a band of the picture: FETCH 0.88 GB
 * (-33 %), time +0.3-0.4 ms per step then (33.4 vs 33.0; HBM bytes are not what the kernels wait for — the request path is).  INTER_XCD = n > 1:
 * block-cyclic runs of n workgroups per XCD (32: FETCH -18 %, time unchanged); 0: u = x. */
#ifndef INTER_XCD
#define INTER_XCD 1
#endif
__device__ __forceinline__ uint32_t inter_unit_of_block()
{
#if INTER_XCD == 1
    const uint32_t cls8 = blockIdx.x & 7u, per8 = gridDim.x >> 3, rem8 = gridDim.x & 7u;
    return cls8 * per8 + (cls8 < rem8 ? cls8 : rem8) + (blockIdx.x >> 3);
#elif INTER_XCD > 1
    const uint32_t C_ = INTER_XCD, full_ = (gridDim.x / (8u * C_)) * (8u * C_);
    const uint32_t b_ = blockIdx.x, o_ = b_ % (8u * C_);
    return b_ >= full_ ? b_ : (b_ - o_) + (o_ & 7u) * C_ + (o_ >> 3);
#else
    return blockIdx.x;
#endif
}

/* ------------------------------------------------------------------ inter macroblocks with partitions finer than 8x8
 * The third part of the general-inter list (after the one-vector and the quadrant entries): one list entry per single-wavefront workgroup,
 * lane = (4x4 block, row of it).  The sixteen blocks have a motion vector each, so nothing is staged: every lane cuts its 6 x 12-byte window
 * out of global memory (a whole-sample vector inside the picture: the four bytes themselves) and runs the textbook interpolation
 * (luma_from_window / chroma_from_rows).  The bundled streams have no such macroblocks; the synthetic jobs of the tests do. */
#ifndef INTER_FINE_OCC
#define INTER_FINE_OCC 6     /* wavefronts per SIMD the register budget is sized for (the kernel takes 74 VGPRs) */
#endif
__global__ __launch_bounds__(64, INTER_FINE_OCC) void k_recon_inter(const FrameDesc *__restrict__ frames)
{
    const FrameDesc &fd = FD_REF(frames, blockIdx.y);
    const uint32_t gi = fd.n_gen_uni + fd.n_gen_quad + inter_unit_of_block();
    if (gi >= fd.n_gen) return;
    /* list entry as whole dwords from a wave-uniform address in read-only memory: scalar loads (there is no scalar
     * byte load: a struct copy would fetch the byte-sized members with vector loads and wait for them) */
    FjGen ge;
    {
        const uint4 w = ld16c((const H264K_CONST FjGen *)fd.gen + gi);
        __builtin_memcpy(&ge, &w, 16);
    }
    const uint32_t mb = ge.mb;
    /* the QPs travel in the list entry (framejob.h); of the record only the four references are needed: FjMbRec.ref_slot[4], one scalar
     * dword instead of the 32-byte record */
    const int qp_y = (int)FJ_GEN_QP_Y(ge.coef_idx), qp_c = (int)FJ_GEN_QP_C(ge.coef_idx);
    const uint32_t refs = *(const H264K_CONST uint32_t *)((const H264K_CONST uint8_t *)((const H264K_CONST FjMbRec *)fd.recs + mb) + offsetof(FjMbRec, ref_slot));
    const int lane = threadIdx.x & 63;
    const int wmb = fd.wmb, W = wmb * 16, H = fd.hmb * 16, CW = W >> 1, CH = H >> 1;
    const int mby = wmb == 1 ? (int)mb : (int)__umulhi(mb, fd.wmb_magic), mbx = (int)mb - mby * wmb;     /* scalar: FrameDesc.wmb_magic */
    /* (address spaces spelled out once: the loads below become global_load / s_load instead of flat_load) */
    /* the list entry's vector fields hold the index of the macroblock's sixteen vectors in the sparse section */
    const uint32_t mvx_idx = (uint32_t)(uint16_t)ge.mvx | ((uint32_t)(uint16_t)ge.mvy << 16);
    const int16_t *mvs = (const int16_t *)((const H264K_CONST int16_t *)fd.mvx + 32 * (size_t)mvx_idx);
    const int16_t *coef = (const int16_t *)((const H264K_CONST int16_t *)fd.coefs + 16 * (size_t)FJ_GEN_COEF_IDX(ge.coef_idx));
    H264K_GLOBAL uint8_t *cur = (H264K_GLOBAL uint8_t *)fd.cur;
    const int blk = lane >> 2, row = lane & 3, bx = blk & 3, by = blk >> 2;
    const uint32_t mv_mine = *reinterpret_cast<const uint32_t *>(mvs + 2 * blk);

    /* the coefficient rows are requested ahead of the reference windows and consumed after the prediction */
    const ResidRows rrows = mb_residual_fetch(ge.coded, coef, lane);
    s2 pl01 = pk(0), pl23 = pk(0);               /* the lane's four luma prediction samples, two packed pairs */
    s2 pc01 = pk(0), pc23 = pk(0);               /* lanes 0..31: the four chroma prediction samples of the lane's row */
    {
        const int mvx = (int16_t)(mv_mine & 0xFFFFu), mvy = (int32_t)mv_mine >> 16;
        const uint8_t *ref = slot_ptr(fd, (refs >> (8 * ((by >> 1) * 2 + (bx >> 1)))) & 255u);
        const int x = mbx * 16 + bx * 4 + (mvx >> 2), y = mby * 16 + by * 4 + row + (mvy >> 2);
        int pl[4];
        if (((mvx | mvy) & 3) == 0 && x >= 0 && x + 3 < W && y >= 0 && y < H) {
            const uint32_t v = luma4_at(ref, wmb, x, y);
            pl[0] = v & 255; pl[1] = (v >> 8) & 255; pl[2] = (v >> 16) & 255; pl[3] = v >> 24;
        } else {
            uint32_t rw[6][3];
            luma_window_global(ref, wmb, W, H, x, y, rw);
            luma_from_window(rw, mvx & 3, mvy & 3, pl);
        }
        pl01 = as_s2((uint32_t)pl[0] | ((uint32_t)pl[1] << 16)); pl23 = as_s2((uint32_t)pl[2] | ((uint32_t)pl[3] << 16));
    }
    if (lane < 32) {
        int pc[4];
        const int k = lane >> 2, plane = k >> 2, cbx = k & 1, cby = (k >> 1) & 1;
        const int cy = cby * 4 + row, cx0 = cbx * 4;
#pragma unroll
        for (int pair = 0; pair < 2; pair++) {
            const int cx = cx0 + 2 * pair;
            const int lb = (cy >> 1) * 4 + (cx >> 1);             /* owning 4x4 luma block */
            const int mvx = mvs[2 * lb], mvy = mvs[2 * lb + 1];
            const uint8_t *ref = slot_ptr(fd, (refs >> (8 * ((cy >> 2) * 2 + (cx >> 2)))) & 255u);
            chroma_pred2(ref, wmb, plane, CW, CH, mbx * 8 + cx + (mvx >> 3), mby * 8 + cy + (mvy >> 3), mvx & 7, mvy & 7, pc + 2 * pair);
        }
        pc01 = as_s2((uint32_t)pc[0] | ((uint32_t)pc[1] << 16)); pc23 = as_s2((uint32_t)pc[2] | ((uint32_t)pc[3] << 16));
    }

    /* (an unconditional use of the coefficient rows here — they arrived long ago — keeps the compiler from sinking their loads
     * into the residual code, where every coded macroblock would wait for a second memory round trip) */
    asm volatile("" :: "v"(rrows.y.x), "v"(rrows.y.y), "v"(rrows.c.x), "v"(rrows.c.y), "v"(rrows.cdc.x), "v"(rrows.cdc.y));
    /* ---- residual add, clip, store.  Lane (block, row) holds 4 samples of row 4*by+row at column 4*bx: the 64 dwords of the
     * wavefront ARE the 256 luma bytes of the tile (each group of 16 lanes one 64-byte piece), the 32 chroma dwords its third
     * line — two coalesced stores, no detour through LDS.  A macroblock without coefficients stores its prediction as it is:
     * no unpacking, no residual, no clipping ---- */
    H264K_GLOBAL uint8_t *T = cur + (size_t)mb * TILE;
    uint32_t luma_dw, chroma_dw;
    if ((ge.coded & 0x03FFFFFFu) == 0u) {                        /* wave-uniform */
        luma_dw = perm(as_u32(pl23), as_u32(pl01), 0x06040200u);
        chroma_dw = perm(as_u32(pc23), as_u32(pc01), 0x06040200u);
    } else if (!(ge.coded & FJ_CODED_WIDE)) {                    /* wave-uniform: the host proved that 16 bits hold every intermediate */
        s2 y01, y23, c01, c23;
        mb_residual_pk(ge.coded, qp_y, qp_c, lane, rrows, y01, y23, c01, c23);
        const s2 lo = pk(0), hi = pk(255);
        const s2 l01 = pk_clip(lo, hi, pl01 + y01), l23 = pk_clip(lo, hi, pl23 + y23);
        const s2 k01 = pk_clip(lo, hi, pc01 + c01), k23 = pk_clip(lo, hi, pc23 + c23);
        luma_dw = perm(as_u32(l23), as_u32(l01), 0x06040200u);
        chroma_dw = perm(as_u32(k23), as_u32(k01), 0x06040200u);
    } else {
        int ry[4], rc[4];
        report_residual_range(fd, mb_residual_compute<false>(ge.coded, qp_y, qp_c, false, coef, lane, rrows, ry, rc), lane);
        luma_dw = pack4(clip255(pl01.x + ry[0]), clip255(pl01.y + ry[1]), clip255(pl23.x + ry[2]), clip255(pl23.y + ry[3]));
        chroma_dw = pack4(clip255(pc01.x + rc[0]), clip255(pc01.y + rc[1]), clip255(pc23.x + rc[2]), clip255(pc23.y + rc[3]));
    }
    *reinterpret_cast<H264K_GLOBAL uint32_t *>(T + (by * 4 + row) * 16 + bx * 4) = luma_dw;
    if (lane < 32) {
        const int k = lane >> 2, plane = k >> 2, cbx = k & 1, cby = (k >> 1) & 1;
        *reinterpret_cast<H264K_GLOBAL uint32_t *>(T + T_CB + plane * 64 + (cby * 4 + row) * 8 + cbx * 4) = chroma_dw;
    }
}

} // namespace h264k
