/* kernels/k_recon_inter.hip.h — k_recon_inter<PATH>, k_recon_inter_lb and k_recon_inter_lq: every inter macroblock that is no plain copy (interpolation,
 * residual, write-back).  k_recon_inter_lb takes the one-vector part of the list, k_recon_inter_lq (both at the end of the file) the part with one vector
 * per 8x8 quadrant, k_recon_inter<2> the finer partitions; k_recon_inter<0> and <1> are the previous kernels of the first two parts, launched with
 * -DINTER_LANE_BLOCKS=0 / -DINTER_LANE_QUADS=0.  Part of kernels.hip.h (which see); not a stand-alone header. */
#pragma once
namespace h264k {
/* ------------------------------------------------------------------ inter prediction */
__device__ __forceinline__ int tap6(int a, int b, int c, int d, int e, int f) { return a - 5 * (b + e) + 20 * (c + d) + f; }

/* Register window of one lane: rows y-2..y+3, columns x-2..x+9 of the reference plane (9 columns used),
 * rw[r][k] = dword k of window row r.  Filled either straight from global memory (clamp-to-edge on the
 * slow path = h264bsdFillBlock, src/h264bsd_reconstruct.c:2244) or from the wave's LDS-staged window. */
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

/* The same prediction for a lane whose window lies in LDS (k_recon_inter, staged windows): src = window row 0 at the dword that
 * holds window column 0, sh = 8 * (byte of that column in its dword).  The interpolation class is wave-uniform (one motion
 * vector per wavefront or quadrant... per lane in the quadrant path, still few classes per wavefront) and every class reads
 * only the window rows and dwords it uses — whole-sample: one row, two dwords; horizontal: one row; vertical: six rows of two
 * dwords; only the centre classes need all 6 x 3 — instead of 24 LDS dwords and 18 funnel shifts for every macroblock.
 * Result: the four samples as two packed pairs (o01, o23), 0..255 each. */
__device__ __forceinline__ void luma_pred_lds(const uint8_t *src, int stride, int sh, int fx, int fy, s2 &o01, s2 &o23)
{
    uint32_t rw[6][3];
    auto row = [&](int r, int nd) {                  /* dwords 0 .. nd-1 of window row r */
        const uint32_t *q = reinterpret_cast<const uint32_t *>(src + r * stride);   /* 4-byte aligned only */
        uint32_t d[4];
#pragma unroll
        for (int k = 0; k < 4; k++) if (k <= nd) d[k] = q[k];
#pragma unroll
        for (int k = 0; k < 3; k++) if (k < nd) rw[r][k] = (uint32_t)(((unsigned long long)d[k + 1] << 32 | d[k]) >> sh);
    };
#define CP(r, c) as_s2(perm(rw[(r)][((c) + 1) >> 2], rw[(r)][(c) >> 2], \
                      0x0C000C00u | (uint32_t)((c) & 3) | ((uint32_t)(((((c) + 1) >> 2) != ((c) >> 2)) ? 4 + (((c) + 1) & 3) : (((c) + 1) & 3)) << 16)))
#define HT2(r, i) (CP(r, i) + CP(r, (i) + 5) - pk(5) * (CP(r, (i) + 1) + CP(r, (i) + 4)) + pk(20) * (CP(r, (i) + 2) + CP(r, (i) + 3)))
#define VT2(c) (CP(0, c) + CP(5, c) - pk(5) * (CP(1, c) + CP(4, c)) + pk(20) * (CP(2, c) + CP(3, c)))
#define RND5(x) pk_clip(pk(0), pk(255), ((x) + pk(16)) >> pk(5))
#define GW(r, c) ((int)((rw[(r)][(c) >> 2] >> (8 * ((c) & 3))) & 255u))
    if ((fx | fy) == 0) {                            /* G: whole-sample */
        row(2, 2);
        o01 = CP(2, 2); o23 = CP(2, 4);
        return;
    }
    if (fy == 0) {                                   /* a, b, c: horizontal only (window row 2) */
        row(2, 3);
        o01 = RND5(HT2(2, 0)); o23 = RND5(HT2(2, 2));
        if (fx == 1) { o01 = (o01 + CP(2, 2) + pk(1)) >> pk(1); o23 = (o23 + CP(2, 4) + pk(1)) >> pk(1); }
        else if (fx == 3) { o01 = (o01 + CP(2, 3) + pk(1)) >> pk(1); o23 = (o23 + CP(2, 5) + pk(1)) >> pk(1); }
        return;
    }
    if (fx == 0) {                                   /* d, h, n: vertical only (columns 2..5) */
        row(0, 2); row(1, 2); row(2, 2); row(3, 2); row(4, 2); row(5, 2);
        o01 = RND5(VT2(2)); o23 = RND5(VT2(4));
        if (fy == 1) { o01 = (o01 + CP(2, 2) + pk(1)) >> pk(1); o23 = (o23 + CP(2, 4) + pk(1)) >> pk(1); }
        else if (fy == 3) { o01 = (o01 + CP(3, 2) + pk(1)) >> pk(1); o23 = (o23 + CP(3, 4) + pk(1)) >> pk(1); }
        return;
    }
    if (fx != 2 && fy != 2) {                        /* e, g, p, r: average of the nearest horizontal and vertical half samples */
        row(0, 2); row(1, 2); row(4, 2); row(5, 2);
        s2 b01, b23, h01, h23;
        if (fy == 1) { row(2, 3); row(3, 2); b01 = HT2(2, 0); b23 = HT2(2, 2); } else { row(2, 2); row(3, 3); b01 = HT2(3, 0); b23 = HT2(3, 2); }
        if (fx == 1) { h01 = VT2(2); h23 = VT2(4); } else { h01 = VT2(3); h23 = VT2(5); }
        o01 = (RND5(b01) + RND5(h01) + pk(1)) >> pk(1); o23 = (RND5(b23) + RND5(h23) + pk(1)) >> pk(1);
        return;
    }
    /* j, f, q, i, k: the 6-tap filter over un-rounded intermediate sums — over the vertical sums of nine columns (8.4.2.2.1: both
     * orders are equal): 9 + 4 filters instead of 24 + 4, and the vertical sums are exactly what i / k need */
    row(0, 3); row(1, 3); row(2, 3); row(3, 3); row(4, 3); row(5, 3);
#define VH1(c) tap6(GW(0, c), GW(1, c), GW(2, c), GW(3, c), GW(4, c), GW(5, c))
#define HB1(r, i) tap6(GW(r, i), GW(r, (i) + 1), GW(r, (i) + 2), GW(r, (i) + 3), GW(r, (i) + 4), GW(r, (i) + 5))
    int v1[9], out[4];
#pragma unroll
    for (int c = 0; c < 9; c++) v1[c] = VH1(c);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int j = clip255((tap6(v1[i], v1[i + 1], v1[i + 2], v1[i + 3], v1[i + 4], v1[i + 5]) + 512) >> 10);
        int v = j;
        if (fy != 2) {                               /* f / q: with b (row y) or s (row y+1) */
            const int b = clip255(((fy == 1 ? HB1(2, i) : HB1(3, i)) + 16) >> 5);
            v = (j + b + 1) >> 1;
        } else if (fx != 2) {                        /* i / k: with h (col x) or m (col x+1) */
            const int hh = clip255(((fx == 1 ? v1[i + 2] : v1[i + 3]) + 16) >> 5);
            v = (j + hh + 1) >> 1;
        }
        out[i] = v;
    }
    o01 = as_s2((uint32_t)out[0] | ((uint32_t)out[1] << 16)); o23 = as_s2((uint32_t)out[2] | ((uint32_t)out[3] << 16));
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
/* The same two samples from STAGED rows in packed 16-bit: s0 points at the first of three consecutive bytes of the upper row, s1 at
 * those of the row below (any byte alignment; the dword behind them belongs to the row's stride).  Weights are at most 64 and
 * samples at most 255: every partial sum fits a signed 16-bit half.  Round 6: the chroma prediction of a macroblock used to be
 * 32 lanes x 4 samples in 32-bit arithmetic from ten ds_read_u8 each — about 56 of the 257 vector instructions of a one-vector
 * macroblock; it is 64 lanes x 2 samples now (lanes 32..63 hand their pair to lanes 0..31 with v_permlane32_swap). */
__device__ __forceinline__ s2 chroma_pair_lds(const uint8_t *s0, const uint8_t *s1, int fx, int fy)
{
    auto three = [](const uint8_t *p) -> uint32_t {
        const uint32_t sh = (uint32_t)(uintptr_t)p & 3u;
        const uint32_t *q = reinterpret_cast<const uint32_t *>(p - sh);
        return __builtin_amdgcn_alignbyte(q[1], q[0], sh);
    };
    const uint32_t ra = three(s0), rb = three(s1);
    const s2 P0 = as_s2(perm(0u, ra, 0x0C010C00u)), P1 = as_s2(perm(0u, ra, 0x0C020C01u));
    const s2 Q0 = as_s2(perm(0u, rb, 0x0C010C00u)), Q1 = as_s2(perm(0u, rb, 0x0C020C01u));
    const int w00 = (8 - fx) * (8 - fy), w10 = fx * (8 - fy), w01 = (8 - fx) * fy, w11 = fx * fy;
    return (P0 * pk(w00) + P1 * pk(w10) + Q0 * pk(w01) + Q1 * pk(w11) + pk(32)) >> pk(6);
}
/* lanes 0..31 receive the pair of lane + 32 (theirs is samples 0, 1 of the row, that one samples 2, 3) */
__device__ __forceinline__ s2 pair_from_upper_half(s2 mine)
{
    const uint32_t x = as_u32(mine);
    const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    return as_s2(r[1]);
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

/* ------------------------------------------------------------------ inter macroblocks */
/* General inter macroblocks, one wavefront each.  When the 16 motion vectors and the four references of
 * the macroblock agree (82 % of the general MBs, everything but sub-partitioned ones) the 21x21 luma and two
 * 9x9 chroma reference windows are staged ONCE in LDS with row-wide coalesced dword loads and every lane
 * cuts its 6x12-byte register window out of LDS; otherwise every lane fetches its own window from global
 * memory.  Both feed the same textbook interpolation (luma_from_window / chroma_from_rows). */
/* 16 / 8 bytes at a 4-byte aligned address (global_load_dwordx4 / dwordx2 need dword alignment only) */
struct __attribute__((packed, aligned(4))) U4a4 { uint32_t x, y, z, w; };
struct __attribute__((packed, aligned(4))) U2a4 { uint32_t x, y; };

/* Reference windows are staged tile row by tile row: a window row is the 16-byte rows of the 2-3 tiles it crosses,
 * loaded whole (aligned 16-byte / 8-byte requests) and laid side by side in LDS, so byte 0 of a staged row is the first
 * column of the window's first tile. */
constexpr int IW_STRIDE = 52;                        /* luma window: 21 rows x 3 tiles x 16 bytes; 13-dword stride.  Not free of bank conflicts, as this line used to say:
                                                        measured, SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE was 48.8 % for k_recon_inter<0> (profiles/r06_sq_counters.txt);
                                                        for k_recon_inter_lb see LB_SLOT_LDS below and docs/EXPERIMENTS.md */
constexpr int IC_STRIDE = 20;                        /* chroma windows: 9 rows x 2 tiles x 8 bytes, two planes */
constexpr int QW_STRIDE = 36;                        /* quadrant luma windows: 13 rows x 2 tiles x 16 bytes, 9-dword stride */
constexpr int QC_STRIDE = 20;                        /* quadrant chroma windows: 5 rows x 2 tiles x 8 bytes, two planes */
constexpr int INTER_WAVE_LDS = 2688;                 /* max(21 * IW_STRIDE + 2 * 9 * IC_STRIDE = 1452, 4 * 13 * QW_STRIDE + 4 * 2 * 5 * QC_STRIDE = 2672), rounded */

#ifndef INTER_OCC
#define INTER_OCC 8      /* macroblock-tile layout: 8 waves per SIMD (64 VGPRs, more spills) beat 7 / 6 / 5: 50.4 vs 54.4 / 58.9 / 59.2 ms per step — the kernel hides latency with wavefronts */
#endif
/* Three instantiations share the list: PATH 0 reconstructs the entries with one motion vector per macroblock (82 % of
 * them in the bundled 1080p stream), PATH 1 those with one per 8x8 quadrant (16x8, 8x16, 8x8 partitions: all the others
 * of that stream), PATH 2 the finer partitions.  Compiled separately, each gets the registers its own path needs — the
 * common cases do not pay (in spills at 8 waves per SIMD) for the per-lane window code of the rare one. */
#ifndef INTER_OCC_PART
#define INTER_OCC_PART 6     /* the partitioned paths: a hint of 6 lets the quadrant path take the 100 scalar registers it wants (60 VGPRs: it still runs
                                8 waves per SIMD); at a hint of 8 it spills 32 scalar registers into vector lanes */
#endif
#ifndef INTER_WG_WAVES
#define INTER_WG_WAVES 1     /* wavefronts (= macroblocks) per workgroup.  The wavefronts of this kernel share nothing, and a workgroup of four
                                needs a free slot on each of the four SIMDs of one CU at the same moment: 1 / 2 / 4 / 8 / 16 wavefronts per
                                workgroup take 34.0 / 35.8 / 38.8 / 42.9 / 48.9 ms per step (the average occupancy, not the instruction
                                count, was what held the kernel back: -10 % instructions had changed nothing) */
#endif
#ifndef INTER_PER_WAVE
#define INTER_PER_WAVE 2     /* list entries per wavefront, the one-vector path: 1 / 2 / 3 / 4 / 6 / 8 -> 34.4 / 32.7 / 33.1 / 33.1 / 33.6 / 34.2 ms per step (both paths' time) */
#endif
#ifndef INTER_PER_WAVE_QUAD
#define INTER_PER_WAVE_QUAD 2   /* ... the quadrant path (69 VGPRs: 7 wavefronts per SIMD instead of 8, and still 0.3 ms better); the finer partitions: always 1 */
#endif
#ifndef INTER_XCD
#define INTER_XCD 1         /* blockIdx -> list position: one XCD takes a contiguous eighth of a picture's list (k_recon_inter, below) */
#endif
template <int PATH> constexpr uint32_t inter_per_wave() { return PATH == 0 ? INTER_PER_WAVE : PATH == 1 ? INTER_PER_WAVE_QUAD : 1; }
#ifdef H264K_INTER_PROFILE
#define IPROF(k) do { if (PATH == 0) ipt[k] = __builtin_readcyclecounter(); } while (0)
#else
#define IPROF(k) do { } while (0)
#endif
template <int PATH>
__global__ __launch_bounds__(64 * INTER_WG_WAVES, PATH == 0 ? INTER_OCC : INTER_OCC_PART) void k_recon_inter(const FrameDesc *__restrict__ frames)
{
#ifdef H264K_INTER_PROFILE
    unsigned long long ipt[6] = { 0, 0, 0, 0, 0, 0 };      /* cycle accounting of one list entry (tools/inter_prof.py): begin | entry here | windows staged | predicted | before the store | end */
#endif
    __shared__ __attribute__((aligned(16))) uint8_t lds[INTER_WG_WAVES * INTER_WAVE_LDS];
    const FrameDesc &fd = FD_REF(frames, blockIdx.y);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   /* wave-uniform: the list entry, the record and
                                                                                 everything derived live in scalar registers */
    /* A wavefront reconstructs INTER_PER_WAVE consecutive list entries, one after the other (nothing of entry i + 1 is requested
     * before entry i is stored: no register is carried from one to the next).  What that amortises is the START of a wavefront:
     * with one macroblock per single-wavefront workgroup the kernel spends a third of its time launching workgroups that do
     * nothing yet (measured with the body cut out behind the first scalar loads: 8 of 22 ms per step), and neighbours in the list
     * are neighbours in the picture — their reference windows overlap, and the second one finds the first one's lines in the L1. */
    const uint32_t g_first = (PATH == 0 ? 0u : PATH == 1 ? fd.n_gen_uni : fd.n_gen_uni + fd.n_gen_quad);
    const uint32_t g_end = (PATH == 0 ? fd.n_gen_uni : PATH == 1 ? fd.n_gen_uni + fd.n_gen_quad : fd.n_gen);
#pragma unroll 1
  for (uint32_t it = 0; it < inter_per_wave<PATH>(); it++) {
    /* Workgroups are dealt to the eight XCDs round robin in dispatch order (x fastest), and every XCD has its own L2: with the plain
     * mapping two neighbouring macroblocks — whose reference windows overlap — never share an L2, and every 128-byte line a window
     * touches is fetched from HBM by up to four XCDs (FETCH 1.31 GB per tick for 0.48 GB of windows and coefficients).  INTER_XCD = 1
     * (default): the workgroups x = c (mod 8) of a picture — one XCD's — take the c-th contiguous eighth of its list, i.e. a band of the
     * picture: FETCH 0.88 GB (-33 %), time +0.3-0.4 ms per step (33.4 vs 33.0; HBM bytes are not what the kernel waits for — the request path
     * is).  INTER_XCD = n > 1: block-cyclic chunks of n workgroups per XCD (32: FETCH -18 %, time unchanged); 0: the plain mapping. */
#if INTER_XCD == 1
    const uint32_t cls8 = blockIdx.x & 7u, per8 = gridDim.x >> 3, rem8 = gridDim.x & 7u;
    const uint32_t bx_ = cls8 * per8 + (cls8 < rem8 ? cls8 : rem8) + (blockIdx.x >> 3);
#elif INTER_XCD > 1
    const uint32_t C_ = INTER_XCD, full_ = (gridDim.x / (8u * C_)) * (8u * C_);
    const uint32_t b_ = blockIdx.x, o_ = b_ % (8u * C_);
    const uint32_t bx_ = b_ >= full_ ? b_ : (b_ - o_) + (o_ & 7u) * C_ + (o_ >> 3);
#else
    const uint32_t bx_ = blockIdx.x;
#endif
    const uint32_t gi = g_first + (bx_ * INTER_WG_WAVES + wave) * inter_per_wave<PATH>() + it;
    if (gi >= g_end) return;
    IPROF(0);                                        /* (the first entry's count begins a few scalar loads into the wavefront's life) */
    /* list entry and record as whole dwords from a wave-uniform address in read-only memory: scalar loads (there is no scalar
     * byte load: a struct copy would fetch the byte-sized members with vector loads and wait for them) */
    FjGen ge;
    {
        const uint4 w = ld16c((const H264K_CONST FjGen *)fd.gen + gi);
        __builtin_memcpy(&ge, &w, 16);
    }
    const uint32_t mb = ge.mb;
#ifdef H264K_INTER_PROFILE
    if (PATH == 0) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
#endif
    IPROF(1);
    /* the QPs travel in the list entry (framejob.h); only the partitioned paths need the record, for their four references */
    const int qp_y = (int)FJ_GEN_QP_Y(ge.coef_idx), qp_c = (int)FJ_GEN_QP_C(ge.coef_idx);
    uint32_t rec_refs = 0u;                          /* FjMbRec.ref_slot[4]: one scalar dword instead of the 32-byte record */
    if (PATH != 0) rec_refs = *(const H264K_CONST uint32_t *)((const H264K_CONST uint8_t *)((const H264K_CONST FjMbRec *)fd.recs + mb) + offsetof(FjMbRec, ref_slot));
    int lane = threadIdx.x & 63;
    if (inter_per_wave<PATH>() > 1) asm volatile("" : "+v"(lane));                   /* (everything a lane derives from its number is worked out again for every entry: hoisted out of
                                                        the loop it would live in registers the kernel does not have at 8 wavefronts per SIMD) */
    uint8_t *lw = lds + wave * INTER_WAVE_LDS, *lc = lw + 21 * IW_STRIDE;
    const int wmb = fd.wmb, W = wmb * 16, H = fd.hmb * 16, CW = W >> 1, CH = H >> 1;
    const int mby = wmb == 1 ? (int)mb : (int)__umulhi(mb, fd.wmb_magic), mbx = (int)mb - mby * wmb;     /* scalar: FrameDesc.wmb_magic */
    /* (address spaces spelled out once: the loads below become global_load / s_load instead of flat_load) */
    /* partitioned macroblocks: the list entry's vector fields hold the index of their sixteen vectors in the sparse section */
    const uint32_t mvx_idx = PATH == 0 ? 0u : (uint32_t)(uint16_t)ge.mvx | ((uint32_t)(uint16_t)ge.mvy << 16);
    const int16_t *mvs = (const int16_t *)((const H264K_CONST int16_t *)fd.mvx + 32 * (size_t)mvx_idx);
    const int16_t *coef = (const int16_t *)((const H264K_CONST int16_t *)fd.coefs + 16 * (size_t)FJ_GEN_COEF_IDX(ge.coef_idx));
    H264K_GLOBAL uint8_t *cur = (H264K_GLOBAL uint8_t *)fd.cur;
    const int blk = lane >> 2, row = lane & 3, bx = blk & 3, by = blk >> 2;
    const bool uniform = PATH == 0, quadwise = PATH == 1;
    uint32_t refs = ge.slot * 0x01010101u, mv_mine = 0;
    const uint32_t mv0 = (uint32_t)(uint16_t)ge.mvx | ((uint32_t)(uint16_t)ge.mvy << 16);
    if (!uniform) {
        refs = rec_refs;
        if (!quadwise) mv_mine = *reinterpret_cast<const uint32_t *>(mvs + 2 * blk);
    }

    /* the coefficient rows are requested right behind the reference windows (whose loads come first: they are needed
     * first) and consumed after the prediction */
    ResidRows rrows;
    if (!uniform) rrows = mb_residual_fetch(ge.coded, coef, lane);
    s2 pl01 = pk(0), pl23 = pk(0);               /* the lane's four luma prediction samples, two packed pairs */
    s2 pc01 = pk(0), pc23 = pk(0);               /* lanes 0..31: the four chroma prediction samples of the lane's row */
    if (uniform) {
        const int mvx = (int16_t)(mv0 & 0xFFFFu), mvy = (int32_t)mv0 >> 16;
        const H264K_GLOBAL uint8_t *ref = (const H264K_GLOBAL uint8_t *)slot_ptr(fd, refs & 255u);
        const int xi = mbx * 16 + (mvx >> 2) - 2, yi = mby * 16 + (mvy >> 2) - 2;
        const int xs = (xi >> 4) << 4;                           /* first column of the window's first tile */
        const int cxi = mbx * 8 + (mvx >> 3), cyi = mby * 8 + (mvy >> 3);
        const int cxs = (cxi >> 3) << 3;
        /* ---- stage: luma rows yi..yi+20 x the tiles at xs, xs+16, xs+32 (the window needs columns xi..xi+20); chroma
         * rows cyi..cyi+8 x the tiles at cxs, cxs+8 (columns cxi..cxi+8).  One aligned 16-byte load per lane for luma
         * (lane = 3 * row + tile: 63 lanes), one 8-byte load for chroma (lane = 18 * plane + 2 * row + tile: 36 lanes). */
        const bool lfast = xi >= 0 && xi + 21 <= W && yi >= 0 && yi + 21 <= H;
        const bool cfast = cxi >= 0 && cxi + 9 <= CW && cyi >= 0 && cyi + 9 <= CH;
        /* All global loads of the macroblock are issued back to back — the window pieces here, the coefficient rows above —
         * and only then consumed: one memory round trip per macroblock.  (A load and the LDS store of its result inside one
         * `if` make the wavefront wait for that load before it issues the next one.)  Lanes without a piece load the first
         * bytes of the reference frame and drop them. */
        const int lr = (lane * 43) >> 7, lk = lane - 3 * lr, lx = xs + 16 * lk;          /* lane / 3, lane % 3 */
        /* (the window's 21 columns reach into the third tile only when they start in the last four columns of the first:
         * in three cases out of four that tile is not requested at all — nothing reads the bytes it would have filled) */
        const bool l_on = lfast && lane < 63 && lx < W && (lk < 2 || xi - xs >= 12);
        const uint4 vl = ld16g(ref + (l_on ? luma_at(wmb, lx, yi + lr) : (size_t)0));
        const int cp = lane >= 18, rem = cp ? lane - 18 : lane, cr = rem >> 1, ck = rem & 1, cx = cxs + 8 * ck;
        const bool c_on = cfast && lane < 36 && cx < CW;
        const uint2 vc = ld8g(ref + (c_on ? chroma_at(wmb, cp, cx, cyi + cr) : (size_t)0));
        rrows = mb_residual_fetch(ge.coded, coef, lane);
        if (l_on) {
            uint32_t *d32 = reinterpret_cast<uint32_t *>(lw + lr * IW_STRIDE + 16 * lk);
            d32[0] = vl.x; d32[1] = vl.y; d32[2] = vl.z; d32[3] = vl.w;
        }
        if (c_on) {
            uint32_t *d32 = reinterpret_cast<uint32_t *>(lc + cp * 9 * IC_STRIDE + cr * IC_STRIDE + 8 * ck);
            d32[0] = vc.x; d32[1] = vc.y;
        }
        if (!lfast) {
            for (int d = lane; d < 21 * 48; d += 64) {
                const int r = d / 48, c = d % 48;
                lw[r * IW_STRIDE + c] = ref[luma_at(wmb, clip3(0, W - 1, xs + c), clip3(0, H - 1, yi + r))];
            }
        }
        if (!cfast) {
            for (int d = lane; d < 2 * 9 * 16; d += 64) {
                const int pp = d / 144, r = (d % 144) / 16, c = d % 16;
                lc[pp * 9 * IC_STRIDE + r * IC_STRIDE + c] = ref[chroma_at(wmb, pp, clip3(0, CW - 1, cxs + c), clip3(0, CH - 1, cyi + r))];
            }
        }
        wave_sync();
#ifdef H264K_INTER_PROFILE
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#endif
        IPROF(2);
        /* ---- luma: window rows (4*by+row)..+5, bytes o..o+11 with o = (xi-xs) + 4*bx ---- */
        {
            const int o = (xi - xs) + 4 * bx, sh = 8 * (o & 3);
            luma_pred_lds(lw + (4 * by + row) * IW_STRIDE + (o & ~3), IW_STRIDE, sh, mvx & 3, mvy & 3, pl01, pl23);
        }
        /* ---- chroma: lanes 0..31, 4 samples of one row = two pairs ---- */
        {
            const int k = (lane & 31) >> 2, plane = k >> 2, cbx = k & 1, cby = (k >> 1) & 1;
            const int cy = cby * 4 + row, cx0 = cbx * 4 + 2 * (lane >> 5);
            const uint8_t *s0 = lc + plane * 9 * IC_STRIDE + cy * IC_STRIDE + (cxi - cxs) + cx0;
            pc01 = chroma_pair_lds(s0, s0 + IC_STRIDE, mvx & 7, mvy & 7);
            pc23 = pair_from_upper_half(pc01);
        }
    } else if (quadwise) {
        /* ---- one motion vector per 8x8 quadrant (16x8, 8x16, 8x8 partitions): four 13x13 luma and four 5x5 (x2 planes)
         * chroma windows staged in LDS, then the same window arithmetic per lane.  Staging: per quadrant 13 luma rows x 2
         * tiles (26 aligned 16-byte pieces: lanes 0..25) and 2 planes x 5 chroma rows x 2 tiles (20 aligned 8-byte pieces:
         * lanes 26..45) — which piece a lane fetches is the same in every quadrant, what differs between the quadrants (motion
         * vector, reference, window origin, whether the window lies inside the picture) is wave-uniform: scalar registers.
         * All four quadrants are requested before the first is consumed (one memory round trip).  (Round 3 let every lane
         * derive quadrant, row and tile of TWO pieces from its lane number with divisions, and load its quadrant's motion
         * vector from memory: 627 vector instructions per macroblock against 290 on the one-vector path.) ---- */
        uint8_t *lq = lw, *cq = lw + 4 * 13 * QW_STRIDE;
        const H264K_CONST uint32_t *mvc = (const H264K_CONST uint32_t *)fd.mvx + 16 * (size_t)mvx_idx;   /* (x | y << 16) per 4x4 block, raster */
        const bool is_l = lane < 26, is_c = lane >= 26 && lane < 46;
        const int e = lane - 26, pp = e >= 10, e2 = pp ? e - 10 : e;
        const int pr = is_l ? lane >> 1 : e2 >> 1, pk2 = (is_l ? lane : e2) & 1;          /* the piece's row in the window, its tile (0 / 1) */
        uint32_t mvq[4];
        uint4 pv[4];
        bool pon[4], lfast[4], cfast[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            mvq[q] = mvc[(q >> 1) * 8 + (q & 1) * 2];
            const int mvx = (int16_t)(mvq[q] & 0xFFFFu), mvy = (int32_t)mvq[q] >> 16;
            const H264K_GLOBAL uint8_t *ref = (const H264K_GLOBAL uint8_t *)slot_ptr(fd, (refs >> (8 * q)) & 255u);
            const int xi = mbx * 16 + 8 * (q & 1) + (mvx >> 2) - 2, yi = mby * 16 + 8 * (q >> 1) + (mvy >> 2) - 2;
            const int cxi = mbx * 8 + 4 * (q & 1) + (mvx >> 3), cyi = mby * 8 + 4 * (q >> 1) + (mvy >> 3);
            lfast[q] = xi >= 0 && xi + 13 <= W && yi >= 0 && yi + 13 <= H;
            cfast[q] = cxi >= 0 && cxi + 5 <= CW && cyi >= 0 && cyi + 5 <= CH;
            const int xs = ((xi >> 4) << 4) + 16 * pk2, cxs = ((cxi >> 3) << 3) + 8 * pk2;
            pon[q] = is_l ? (lfast[q] && xs < W) : (is_c && cfast[q] && cxs < CW);
            const size_t off = !pon[q] ? (size_t)0 : is_l ? luma_at(wmb, xs, yi + pr) : chroma_at(wmb, pp, cxs, cyi + pr);
            pv[q] = ld16g(ref + off);        /* (no branch around a load: its end would wait for it.  Chroma lanes use the first 8 of the 16 bytes;
                                                 the rest is the plane's next row, or the first bytes of what follows the tile) */
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (pon[q]) {
                uint32_t *d32 = reinterpret_cast<uint32_t *>(is_l ? lq + q * 13 * QW_STRIDE + pr * QW_STRIDE + 16 * pk2
                                                                  : cq + (q * 2 + pp) * 5 * QC_STRIDE + pr * QC_STRIDE + 8 * pk2);
                d32[0] = pv[q].x; d32[1] = pv[q].y;
                if (is_l) { d32[2] = pv[q].z; d32[3] = pv[q].w; }
            }
            /* windows that leave the picture (h264bsdFillBlock, reconstruct.c:2244): gathered sample by sample, clamped */
            if (!lfast[q] || !cfast[q]) {                            /* wave-uniform */
                const int mvx = (int16_t)(mvq[q] & 0xFFFFu), mvy = (int32_t)mvq[q] >> 16;
                const uint8_t *ref = slot_ptr(fd, (refs >> (8 * q)) & 255u);
                const int xi = mbx * 16 + 8 * (q & 1) + (mvx >> 2) - 2, yi = mby * 16 + 8 * (q >> 1) + (mvy >> 2) - 2;
                const int cxi = mbx * 8 + 4 * (q & 1) + (mvx >> 3), cyi = mby * 8 + 4 * (q >> 1) + (mvy >> 3);
                if (!lfast[q] && is_l) {
                    const int xs = ((xi >> 4) << 4) + 16 * pk2, yy = clip3(0, H - 1, yi + pr);
                    uint32_t *d32 = reinterpret_cast<uint32_t *>(lq + q * 13 * QW_STRIDE + pr * QW_STRIDE + 16 * pk2);
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        uint32_t v = 0;
#pragma unroll
                        for (int i = 0; i < 4; i++) v |= (uint32_t)ref[luma_at(wmb, clip3(0, W - 1, xs + 4 * c + i), yy)] << (8 * i);
                        d32[c] = v;
                    }
                }
                if (!cfast[q] && is_c) {
                    const int cxs = ((cxi >> 3) << 3) + 8 * pk2, yy = clip3(0, CH - 1, cyi + pr);
                    uint32_t *d32 = reinterpret_cast<uint32_t *>(cq + (q * 2 + pp) * 5 * QC_STRIDE + pr * QC_STRIDE + 8 * pk2);
#pragma unroll
                    for (int c = 0; c < 2; c++) {
                        uint32_t v = 0;
#pragma unroll
                        for (int i = 0; i < 4; i++) v |= (uint32_t)ref[chroma_at(wmb, pp, clip3(0, CW - 1, cxs + 4 * c + i), yy)] << (8 * i);
                        d32[c] = v;
                    }
                }
            }
        }
        wave_sync();
        {
            const int q = (by >> 1) * 2 + (bx >> 1);
            const uint32_t mvm = q == 0 ? mvq[0] : q == 1 ? mvq[1] : q == 2 ? mvq[2] : mvq[3];          /* the lane's quadrant's vector: three selects */
            const int mvx = (int16_t)(mvm & 0xFFFFu), mvy = (int32_t)mvm >> 16;
            const int xi = mbx * 16 + 8 * (q & 1) + (mvx >> 2) - 2;
            const int o = (xi & 15) + 4 * (bx & 1), sh = 8 * (o & 3);
            luma_pred_lds(lq + q * 13 * QW_STRIDE + (4 * (by & 1) + row) * QW_STRIDE + (o & ~3), QW_STRIDE, sh, mvx & 3, mvy & 3, pl01, pl23);
        }
        {
            const int k = (lane & 31) >> 2, plane = k >> 2, cbx = k & 1, cby = (k >> 1) & 1;
            const int q = cby * 2 + cbx;                             /* a 4x4 chroma block = one luma quadrant */
            const uint32_t mvm = q == 0 ? mvq[0] : q == 1 ? mvq[1] : q == 2 ? mvq[2] : mvq[3];
            const int mvx = (int16_t)(mvm & 0xFFFFu), mvy = (int32_t)mvm >> 16;
            const int cxi = mbx * 8 + 4 * (q & 1) + (mvx >> 3);
            const uint8_t *s0 = cq + (q * 2 + plane) * 5 * QC_STRIDE + row * QC_STRIDE + (cxi & 7) + 2 * (lane >> 5);
            pc01 = chroma_pair_lds(s0, s0 + QC_STRIDE, mvx & 7, mvy & 7);
            pc23 = pair_from_upper_half(pc01);
        }
    } else {
        /* ---- per-lane windows straight from global memory ---- */
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
    }

    /* (an unconditional use of the coefficient rows here — they arrived long ago — keeps the compiler from sinking their loads
     * into the residual code, where every coded macroblock would wait for a second memory round trip) */
    asm volatile("" :: "v"(rrows.y.x), "v"(rrows.y.y), "v"(rrows.c.x), "v"(rrows.c.y), "v"(rrows.cdc.x), "v"(rrows.cdc.y));
#ifdef H264K_INTER_PROFILE
    asm volatile("" :: "v"(pl01), "v"(pl23), "v"(pc01), "v"(pc23));
#endif
    IPROF(3);
    /* ---- residual add, clip, store.  Lane (block, row) holds 4 samples of row 4*by+row at column 4*bx: the 64 dwords of the
     * wavefront ARE the 256 luma bytes of the tile (each group of 16 lanes one 64-byte piece), the 32 chroma dwords its third
     * line — two coalesced stores, no detour through LDS.  A macroblock without coefficients (55 % of this list in the bundled
     * stream) stores its prediction as it is: no unpacking, no residual, no clipping ---- */
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
#ifdef H264K_INTER_PROFILE
    asm volatile("" :: "v"(luma_dw), "v"(chroma_dw));
#endif
    IPROF(4);
    *reinterpret_cast<H264K_GLOBAL uint32_t *>(T + (by * 4 + row) * 16 + bx * 4) = luma_dw;
    if (lane < 32) {
        const int k = lane >> 2, plane = k >> 2, cbx = k & 1, cby = (k >> 1) & 1;
        *reinterpret_cast<H264K_GLOBAL uint32_t *>(T + T_CB + plane * 64 + (cby * 4 + row) * 8 + cbx * 4) = chroma_dw;
    }
    IPROF(5);
#ifdef H264K_INTER_PROFILE
    if (PATH == 0 && lane == 0 && (blockIdx.x & 63u) == 0u) {
        unsigned long long *pc64 = reinterpret_cast<unsigned long long *>(fd.err) + 8;
        for (int k = 0; k < 5; k++) atomicAdd(pc64 + k, ipt[k + 1] - ipt[k]);
        atomicAdd(pc64 + 5, 1ull);
        atomicAdd(pc64 + 6, (ge.coded & 0x03FFFFFFu) ? 1ull : 0ull);
    }
#endif
    wave_sync();          /* the staged windows are overwritten by the next entry's */
  }
}

/* ------------------------------------------------------------------ the one-vector list, a 4x4 block per lane
 * k_recon_inter_lb replaces k_recon_inter<0> (INTER_LANE_BLOCKS = 1, the default; 0 keeps the kernel above for A/B runs).
 * A workgroup is ONE wavefront and takes INTER_LB_CHUNK consecutive entries of the picture's one-vector list.
 *   Binning.  Lane i reads entry i of the chunk and computes its bin, {not coded, coded} x {whole, hor, ver, diag, centre}; a counting
 *     sort (the histogram is ten ballots, the ranks are prefix counts of them) lays the entries out in LDS ordered by bin.
 *   Groups.  The wavefront then works through the sorted chunk four entries at a time: lane = (slot 0..3, 4x4 luma block 0..15).
 *     Everything an entry decides — macroblock, vector, reference, window origin, quantisers, coded bits — is a per-lane value, so the
 *     scalar work and the address set-up of the old kernel are paid once for four macroblocks.  Every interpolation class runs
 *     under the mask of the lanes that are in it (a wavefront-uniform skip when nobody is): a group of one bin pays for one class, a
 *     group that mixes bins (the remainders of a chunk) for each class it holds.  A slot past the end of the chunk idles: it loads
 *     from a fixed valid address, stages nothing and stores nothing.
 *   Staging.  Per slot one 21 x 48 luma and two 9 x 16 chroma windows as before; the 16 lanes of a slot fetch its 63 + 36 aligned
 *     pieces (4 + 3 loads per lane), and with the coefficient blocks (32 bytes of luma block b, 32 bytes of chroma block b & 7, the 8
 *     DC bytes of its plane) all loads of all four slots are issued before the first is used.
 *   Arithmetic.  kernels/inter_lane_block.hip.h: the lane filters its block from a 9 x 12-byte window (9 window rows for 4 output
 *     rows where four lanes used to fetch 6 each) and transforms its residual block without leaving its registers; lanes b and b + 8
 *     both transform chroma block b & 7 (in the high halves of the packed transform: it costs nothing) and keep two rows each.
 *   Stores.  A 4x4 dword transpose inside each quad of lanes (the four blocks of a block row) gives every lane one whole 16-byte row
 *     of the tile: one global_store_dwordx4 covers the four 256-byte luma tiles; neighbouring lanes swap a dword and store 8-byte
 *     chroma rows, 128 contiguous bytes per slot. */
#ifndef INTER_LANE_BLOCKS
#define INTER_LANE_BLOCKS 1
#endif
#ifndef INTER_LB_CHUNK
#define INTER_LB_CHUNK 32    /* list entries per workgroup (= wavefront), a multiple of 4 up to 64 */
#endif
#ifndef INTER_LB_OCC
#define INTER_LB_OCC 4       /* wavefronts per SIMD the register budget is sized for (128 VGPRs): 16 macroblocks in flight per SIMD */
#endif
static_assert(INTER_LB_CHUNK % 4 == 0 && INTER_LB_CHUNK >= 4 && INTER_LB_CHUNK <= 64, "INTER_LB_CHUNK");
/* ---- what k_recon_inter_lb and k_recon_inter_lq (below) share: the chunk of a workgroup, and the three steps between the staged windows
 * and the lane's finished dwords.  The arithmetic itself is kernels/inter_lane_block.hip.h. ---- */
/* chunk of this workgroup: the XCD mapping of k_recon_inter (which see), in chunks instead of entries */
__device__ __forceinline__ uint32_t inter_chunk_of_block()
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
/* A slot's windows: 21 luma rows at IW_STRIDE, then two planes of 9 chroma rows at IC_STRIDE (1452 bytes), padded to 368 dwords =
 * 16 (mod 32): the sixteen lanes of a slot read dword 13 * (4 * by + r) + bx + const — sixteen different banks of 32, {0..3, 8..11,
 * 20..23, 28..31} + const — and the other slot of the same half-wavefront the other sixteen when the two windows start at the same
 * dword of their tiles; otherwise they are up to 2-way.  Measured over the whole kernel (staging writes included):
 * SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 32.1 % (profiles/inter_lane_blocks_sq_counters.txt). */
constexpr int LB_SLOT_LDS = 1472;
constexpr int LB_LDS = INTER_LB_CHUNK * 16 + 4 * LB_SLOT_LDS;
__global__ __launch_bounds__(64, INTER_LB_OCC) void k_recon_inter_lb(const FrameDesc *__restrict__ frames)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[LB_LDS];
    const FrameDesc &fd = FD_REF(frames, blockIdx.y);
    const uint32_t bx_ = inter_chunk_of_block();
    const uint32_t n_uni = fd.n_gen_uni, first = bx_ * INTER_LB_CHUNK;
    if (first >= n_uni) return;
    const uint32_t n_here = min(n_uni - first, (uint32_t)INTER_LB_CHUNK);            /* wave-uniform */
    const int lane = threadIdx.x & 63;
    const int wmb = fd.wmb, W = wmb * 16, H = fd.hmb * 16, CW = W >> 1, CH = H >> 1;
    const uint32_t frame_bytes = (uint32_t)wmb * fd.hmb * (uint32_t)TILE;            /* a stream's slots are contiguous (slot_ptr): at most 17 x 14 MB */
    const H264K_GLOBAL uint8_t *ref0 = (const H264K_GLOBAL uint8_t *)fd.slot[0];
    const H264K_GLOBAL uint8_t *cf = (const H264K_GLOBAL uint8_t *)fd.coefs;
    H264K_GLOBAL uint8_t *cur = (H264K_GLOBAL uint8_t *)fd.cur;

    /* ---- bin the chunk: lane i < n_here holds entry first + i ---- */
    {
        const bool have = (uint32_t)lane < n_here;
        uint4 e = make_uint4(0u, 0u, 0u, 0u);
        if (have) e = ld16g((const H264K_GLOBAL uint8_t *)fd.gen + 16u * (first + (uint32_t)lane));
        const int fx = (int)(e.y & 3u), fy = (int)((e.y >> 16) & 3u);
        const int cls = (fx | fy) == 0 ? 0 : fy == 0 ? 1 : fx == 0 ? 2 : (fx != 2 && fy != 2) ? 3 : 4;
        /* class first: a group that mixes classes runs a class pass more (110 .. 700 vector instructions), one that mixes coded and
         * not coded only gives its uncoded slots the residual pass (150) — coded first cost 8 class changes per chunk, this order 4 */
        const int bin = have ? 2 * cls + ((e.w & 0x03FFFFFFu) ? 1 : 0) : 10;
        uint32_t rank = 0, seen = 0;
#pragma unroll
        for (int k = 0; k < 10; k++) {
            const unsigned long long m = __ballot(bin == k);
            const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (bin == k) rank = seen + before;
            seen += (uint32_t)__popcll(m);
        }
        if (have) *reinterpret_cast<uint4 *>(lds + 16u * rank) = e;                   /* rank < n_here */
        wave_sync();
    }

    /* The body below runs in four phases — loads and staging | luma | chroma | residual and store — and each of them derives what it
     * needs from the lane number and the four dwords of the list entry AGAIN (LB_FRESH makes them values of unknown origin): left to
     * itself the compiler computes every address of the body at its top and carries them, with the loop-invariant lane geometry, through
     * the centre-class filter, where the registers are needed (23 spilled VGPRs at 128). */
#define LB_FRESH() asm volatile("" : "+v"(ln), "+v"(ge.x), "+v"(ge.y), "+v"(ge.z), "+v"(ge.w))
#define LB_LANE() const int s = ln >> 4, b = ln & 15, bx = b & 3, by = b >> 2; \
                  uint8_t *lw = lds + INTER_LB_CHUNK * 16 + s * LB_SLOT_LDS, *lc = lw + 21 * IW_STRIDE; (void)bx; (void)by; (void)lc
#pragma unroll 1
    for (uint32_t g = 0; g < n_here; g += 4) {
        int ln = lane;
        const bool on = g + (uint32_t)(lane >> 4) < n_here;                           /* g + slot <= INTER_LB_CHUNK - 1 */
        uint4 ge = *reinterpret_cast<const uint4 *>(lds + 16u * (g + (uint32_t)(lane >> 4)));
        if (!on) ge = make_uint4(0u, 0u, 0u, 0u);
        uint32_t yl[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u }, cl[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u }, dcl[2] = { 0u, 0u };
        const bool any_coded = __ballot((ge.w & 0x03FFFFFFu) != 0u) != 0ull;          /* wave-uniform */
      {                                              /* ======== loads and staging ======== */
        LB_FRESH();
        LB_LANE();
        const uint32_t mb = ge.x & 0xFFFFu, refoff = (ge.x >> 24) * frame_bytes;
        const int mvx = (int16_t)(ge.y & 0xFFFFu), mvy = (int32_t)ge.y >> 16;
        const uint32_t coded = ge.w;
        const int mby = wmb == 1 ? (int)mb : (int)__umulhi(mb, fd.wmb_magic), mbx = (int)mb - mby * wmb;
        const int xi = mbx * 16 + (mvx >> 2) - 2, yi = mby * 16 + (mvy >> 2) - 2, xs = (xi >> 4) << 4;
        const int cxi = mbx * 8 + (mvx >> 3), cyi = mby * 8 + (mvy >> 3), cxs = (cxi >> 3) << 3;
        const bool lfast = on && xi >= 0 && xi + 21 <= W && yi >= 0 && yi + 21 <= H;
        const bool cfast = on && cxi >= 0 && cxi + 9 <= CW && cyi >= 0 && cyi + 9 <= CH;

        /* ---- every global load of the group, back to back (a lane without a piece reads the first bytes of slot 0 and drops them).
         * Windows that leave the picture (h264bsdFillBlock: every sample clamped to the picture) need no gather: pictures are whole tiles,
         * so a piece — one tile row — lies wholly inside the picture, wholly left of it (sixteen times the first sample of the clamped
         * row) or wholly right of it (its last sample); the piece is loaded from the clamped tile and row and spread after it arrived. ---- */
        uint4 vl[4];
        uint2 vc[3];
        bool l_on[4], c_on[3];
        const bool any_edge = __ballot(on && !(lfast && cfast)) != 0ull;              /* wave-uniform */
#pragma unroll
        for (int i = 0; i < 4; i++) {                /* luma piece p = 3 * row + tile of the slot's window, p = b + 16 * i < 63 */
            const int p = b + 16 * i, lr = (p * 43) >> 7, lk = p - 3 * lr;
            const int lx = clip3(0, W - 16, xs + 16 * lk), yy = clip3(0, H - 1, yi + lr);
            /* (the window's 21 columns reach into the third tile only when they start in the last four columns of the first) */
            l_on[i] = on && p < 63 && (lk < 2 || xi - xs >= 12);
            const uint32_t off = refoff + (uint32_t)((yy >> 4) * wmb + (lx >> 4)) * (uint32_t)TILE + (uint32_t)((yy & 15) << 4);
            vl[i] = ld16g(ref0 + (l_on[i] ? off : 0u));
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {                /* chroma piece p = 18 * plane + 2 * row + tile, p = b + 16 * i < 36 */
            const int p = b + 16 * i, cp = p >= 18, rem = cp ? p - 18 : p, cr = rem >> 1, ck = rem & 1;
            const int cx = clip3(0, CW - 8, cxs + 8 * ck), yy = clip3(0, CH - 1, cyi + cr);
            c_on[i] = on && p < 36;
            const uint32_t off = refoff + (uint32_t)((yy >> 3) * wmb + (cx >> 3)) * (uint32_t)TILE + (uint32_t)(T_CB + (cp << 6) + ((yy & 7) << 3));
            vc[i] = ld8g(ref0 + (c_on[i] ? off : 0u));
        }
        /* coefficient blocks: luma block b, chroma block k = b & 7, the DC levels of its plane */
        if (any_coded) {
            const int k8 = b & 7;
            const int z = z_of(bx, by);
            const uint32_t cidx = FJ_GEN_COEF_IDX(ge.z), nl = (uint32_t)__popc(coded & 0xFFFFu), has_cdc = (coded >> 25) & 1u;
            const bool ybit = (coded >> z) & 1u, cbit = (coded >> (16 + k8)) & 1u;
            const uint32_t yoff = 32u * (cidx + (uint32_t)__popc(coded & ((1u << z) - 1u)));
            const uint32_t coff = 32u * (cidx + nl + has_cdc + (uint32_t)__popc((coded >> 16) & ((1u << k8) - 1u)));
            const uint32_t doff = 32u * (cidx + nl) + 8u * (uint32_t)(k8 >> 2);
            const H264K_GLOBAL uint8_t *py = ybit ? cf + yoff : ref0, *pc = cbit ? cf + coff : ref0, *pd = has_cdc ? cf + doff : ref0;
            const uint4 y0 = ld16g(py), y1 = ld16g(py + 16), c0 = ld16g(pc), c1 = ld16g(pc + 16);
            const uint2 d0 = ld8g(pd);
            const uint32_t ym = ybit ? ~0u : 0u, cm = cbit ? ~0u : 0u, dm = has_cdc ? ~0u : 0u;
            yl[0] = y0.x & ym; yl[1] = y0.y & ym; yl[2] = y0.z & ym; yl[3] = y0.w & ym; yl[4] = y1.x & ym; yl[5] = y1.y & ym; yl[6] = y1.z & ym; yl[7] = y1.w & ym;
            cl[0] = c0.x & cm; cl[1] = c0.y & cm; cl[2] = c0.z & cm; cl[3] = c0.w & cm; cl[4] = c1.x & cm; cl[5] = c1.y & cm; cl[6] = c1.z & cm; cl[7] = c1.w & cm;
            dcl[0] = d0.x & dm; dcl[1] = d0.y & dm;
        }
        /* ---- stage ---- */
        if (any_edge) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int p = b + 16 * i, lr = (p * 43) >> 7, lk = p - 3 * lr, lx = xs + 16 * lk;
                const uint32_t first = (vl[i].x & 255u) * 0x01010101u, last = (vl[i].w >> 24) * 0x01010101u;
                if (lx < 0) vl[i] = make_uint4(first, first, first, first);
                else if (lx >= W) vl[i] = make_uint4(last, last, last, last);
            }
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const int p = b + 16 * i, cp = p >= 18, rem = cp ? p - 18 : p, ck = rem & 1, cx = cxs + 8 * ck;
                const uint32_t first = (vc[i].x & 255u) * 0x01010101u, last = (vc[i].y >> 24) * 0x01010101u;
                if (cx < 0) vc[i] = make_uint2(first, first);
                else if (cx >= CW) vc[i] = make_uint2(last, last);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int p = b + 16 * i, lr = (p * 43) >> 7, lk = p - 3 * lr;
            if (l_on[i]) {
                uint32_t *d32 = reinterpret_cast<uint32_t *>(lw + lr * IW_STRIDE + 16 * lk);
                d32[0] = vl[i].x; d32[1] = vl[i].y; d32[2] = vl[i].z; d32[3] = vl[i].w;
            }
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const int p = b + 16 * i, cp = p >= 18, rem = cp ? p - 18 : p, cr = rem >> 1, ck = rem & 1;
            if (c_on[i]) {
                uint32_t *d32 = reinterpret_cast<uint32_t *>(lc + cp * 9 * IC_STRIDE + cr * IC_STRIDE + 8 * ck);
                d32[0] = vc[i].x; d32[1] = vc[i].y;
            }
        }
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
            const int cls = !on ? -1 : (fx | fy) == 0 ? 0 : fy == 0 ? 1 : fx == 0 ? 2 : (fx != 2 && fy != 2) ? 3 : 4;
            lb_luma_from_lds<IW_STRIDE>(src, sh, cls, fx, fy, pl);
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
            const uint32_t *q = reinterpret_cast<const uint32_t *>(lc + plane * 9 * IC_STRIDE + (cby * 4 + 2 * half) * IC_STRIDE + (ob & ~3));
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
 * k_recon_inter_lq replaces k_recon_inter<1> (INTER_LANE_QUADS = 1, the default; 0 keeps the kernel above for A/B runs).  It follows
 * k_recon_inter_lb; what is sorted and assigned to lanes is the 8x8 QUADRANT, not the macroblock (the quadrants of a macroblock are in two
 * interpolation classes more often than in one: four macroblocks per group in list order would run four class passes per group).
 *   Binning.  A single-wavefront workgroup takes INTER_LQ_CHUNK consecutive entries of the quadrant part of the list.  Lane i fetches entry i,
 *     its four quadrant vectors (vectors 0, 2, 8, 10 of the sixteen in the sparse section) and the ref_slot dword of its record, and leaves
 *     them in LDS; in rounds of 64, lane j then makes the ITEM of quadrant j & 3 of entry 16 * round + (j >> 2) — four dwords laid out like a
 *     one-vector list entry: macroblock | quadrant << 16 | reference slot << 24, the vector, the coef_idx word, the coded word — and the
 *     counting sort of k_recon_inter_lb (ten ballots per round, class first, then quadrant coded / not coded) lays the items out ordered by
 *     bin.  The sort is stable: the two quadrants of a 16x8 / 8x16 partition stay neighbours.
 *   Groups.  16 items at a time: lane = (slot 0..15, 4x4 luma block j = 0..3 of the quadrant, raster).  A slot past the end idles.
 *   Staging.  Per slot one 13 x 32 luma window and two 5 x 16 chroma windows (the quadrant windows of k_recon_inter<1>, rows packed); the four lanes of a slot fetch its
 *     26 + 20 aligned pieces (7 + 5 loads per lane) and their coefficient blocks (luma block z = 4 * quadrant + j, chroma block `quadrant`
 *     of plane j >> 1, that plane's DC levels), all before the first use.  Windows that leave the picture: the clamped tile row, spread.
 *   Arithmetic.  kernels/inter_lane_block.hip.h through the steps shared with k_recon_inter_lb; lanes 2 * plane, 2 * plane + 1 both transform
 *     the plane's chroma block and keep two rows each.
 *   Stores.  The two lanes of a block row swap two dwords: the left one stores rows 0, 1 of the pair of blocks, the right one rows 2, 3,
 *     8 bytes each; the chroma rows are 4 bytes wide. */
#ifndef INTER_LANE_QUADS
#define INTER_LANE_QUADS 1
#endif
#ifndef INTER_LQ_CHUNK
#define INTER_LQ_CHUNK 8     /* list entries per workgroup (= wavefront), a multiple of 4 up to 64.  The step with 8 / 12 / 16 / 24 / 32 / 64: 77.4 / 77.5 / 78.0 /
                                78.5 / 79.1 / 80.5 ms (parent 81.2): a picture has at most 707 of these entries, and more and shorter wavefronts beat fewer class
                                passes; 4 (one group, nothing to sort) equals 8 within the spread (docs/EXPERIMENTS.md) */
#endif
#ifndef INTER_LQ_OCC
#define INTER_LQ_OCC 4       /* wavefronts per SIMD the register budget is sized for (128 VGPRs; the kernel takes 126).  With the strides below the LDS allows
                                as many: 16 wavefronts of 9.7 KB in a compute unit's 160 KB */
#endif
/* bytes per staged luma row (32 used) and chroma row (16 used).  QW_STRIDE / QC_STRIDE (36 / 20: 11.2 KB per wavefront, 14 per compute unit, 3 per SIMD
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
constexpr int LQ_SLOT_LDS = 13 * LQ_W_STRIDE + 2 * 5 * LQ_C_STRIDE;
constexpr int LQ_ITEMS_LDS = INTER_LQ_CHUNK * 4 * 16;
constexpr int LQ_LDS = LQ_ITEMS_LDS + 16 * LQ_SLOT_LDS;
static_assert(INTER_LQ_CHUNK * 32 + LQ_ROUNDS * 64 <= 16 * LQ_SLOT_LDS, "the fetched entries lie where the windows will");
__global__ __launch_bounds__(64, INTER_LQ_OCC) void k_recon_inter_lq(const FrameDesc *__restrict__ frames)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[LQ_LDS];
    const FrameDesc &fd = FD_REF(frames, blockIdx.y);
    const uint32_t n_quad = fd.n_gen_quad, first = inter_chunk_of_block() * INTER_LQ_CHUNK;
    if (first >= n_quad) return;
    const uint32_t n_here = min(n_quad - first, (uint32_t)INTER_LQ_CHUNK), n_items = 4u * n_here;      /* wave-uniform */
    const int lane = threadIdx.x & 63;
    const int wmb = fd.wmb, W = wmb * 16, H = fd.hmb * 16, CW = W >> 1, CH = H >> 1;
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
            const int fx = (int)(mv & 3u), fy = (int)((mv >> 16) & 3u);
            const int cls = (fx | fy) == 0 ? 0 : fy == 0 ? 1 : fx == 0 ? 2 : (fx != 2 && fy != 2) ? 3 : 4;
            bin[r] = have[r] ? 2 * cls + ((e.w & lq_coded_mask(q)) ? 1 : 0) : 10;
        }
        uint32_t rank[LQ_ROUNDS] = {}, seen = 0;
#pragma unroll
        for (int k = 0; k < 10; k++)
#pragma unroll
            for (int r = 0; r < LQ_ROUNDS; r++) {
                const unsigned long long m = __ballot(bin[r] == k);
                const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                if (bin[r] == k) rank[r] = seen + before;
                seen += (uint32_t)__popcll(m);
            }
        wave_sync();
#pragma unroll
        for (int r = 0; r < LQ_ROUNDS; r++)
            if (have[r]) *reinterpret_cast<uint4 *>(lds + 16u * rank[r]) = it[r];     /* rank < n_items */
        wave_sync();
    }

    /* the four phases of k_recon_inter_lb's body, each deriving what it needs from the lane number and the item again (which see) */
#define LQ_FRESH() asm volatile("" : "+v"(ln), "+v"(ge.x), "+v"(ge.y), "+v"(ge.z), "+v"(ge.w))
#define LQ_LANE() const int s = ln >> 2, j = ln & 3, jbx = j & 1, jby = j >> 1, qd = (int)((ge.x >> 16) & 3u), plane = j >> 1, half = j & 1; \
                  uint8_t *lw = lds + LQ_ITEMS_LDS + s * LQ_SLOT_LDS, *lc = lw + 13 * LQ_W_STRIDE; (void)jbx; (void)jby; (void)qd; (void)plane; (void)half; (void)lc
#pragma unroll 1
    for (uint32_t g = 0; g < n_items; g += 16) {
        int ln = lane;
        const bool on = g + (uint32_t)(lane >> 2) < n_items;                          /* g + slot <= 4 * INTER_LQ_CHUNK - 1 */
        uint4 ge = *reinterpret_cast<const uint4 *>(lds + 16u * (g + (uint32_t)(lane >> 2)));
        if (!on) ge = make_uint4(0u, 0u, 0u, 0u);
        uint32_t yl[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u }, cl[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u }, dcl[2] = { 0u, 0u };
        const bool any_coded = __ballot((ge.w & lq_coded_mask((ge.x >> 16) & 3u)) != 0u) != 0ull;       /* wave-uniform */
      {                                              /* ======== loads and staging ======== */
        LQ_FRESH();
        LQ_LANE();
        const uint32_t mb = ge.x & 0xFFFFu, refoff = (ge.x >> 24) * frame_bytes;
        const int mvx = (int16_t)(ge.y & 0xFFFFu), mvy = (int32_t)ge.y >> 16;
        const uint32_t coded = ge.w;
        const int mby = wmb == 1 ? (int)mb : (int)__umulhi(mb, fd.wmb_magic), mbx = (int)mb - mby * wmb;
        const int xi = mbx * 16 + 8 * (qd & 1) + (mvx >> 2) - 2, yi = mby * 16 + 8 * (qd >> 1) + (mvy >> 2) - 2, xs = (xi >> 4) << 4;
        const int cxi = mbx * 8 + 4 * (qd & 1) + (mvx >> 3), cyi = mby * 8 + 4 * (qd >> 1) + (mvy >> 3), cxs = (cxi >> 3) << 3;
        const bool lfast = on && xi >= 0 && xi + 13 <= W && yi >= 0 && yi + 13 <= H;
        const bool cfast = on && cxi >= 0 && cxi + 5 <= CW && cyi >= 0 && cyi + 5 <= CH;

        /* ---- every global load of the group, back to back; every address clamped into the picture, also where the lane is off (it then
         * reads the first bytes of slot 0 and drops them).  Edge windows: k_recon_inter_lb, which see ---- */
        uint4 vl[7];
        uint2 vc[5];
        bool l_on[7], c_on[5];
        const bool any_edge = __ballot(on && !(lfast && cfast)) != 0ull;              /* wave-uniform */
#pragma unroll
        for (int i = 0; i < 7; i++) {                /* luma piece p = 2 * row + tile of the slot's window, p = j + 4 * i < 26 */
            const int p = j + 4 * i, lr = p >> 1, lk = p & 1;
            const int lx = clip3(0, W - 16, xs + 16 * lk), yy = clip3(0, H - 1, yi + lr);
            /* (the window's 13 columns reach into the second tile only when they start behind the first four columns of the first) */
            l_on[i] = on && p < 26 && (lk == 0 || xi - xs >= 4);
            const uint32_t off = refoff + (uint32_t)((yy >> 4) * wmb + (lx >> 4)) * (uint32_t)TILE + (uint32_t)((yy & 15) << 4);
            vl[i] = ld16g(ref0 + (l_on[i] ? off : 0u));
        }
#pragma unroll
        for (int i = 0; i < 5; i++) {                /* chroma piece p = 10 * plane + 2 * row + tile, p = j + 4 * i < 20 */
            const int p = j + 4 * i, cp = p >= 10, rem = cp ? p - 10 : p, cr = rem >> 1, ck = rem & 1;
            const int cx = clip3(0, CW - 8, cxs + 8 * ck), yy = clip3(0, CH - 1, cyi + cr);
            c_on[i] = on;
            const uint32_t off = refoff + (uint32_t)((yy >> 3) * wmb + (cx >> 3)) * (uint32_t)TILE + (uint32_t)(T_CB + (cp << 6) + ((yy & 7) << 3));
            vc[i] = ld8g(ref0 + (c_on[i] ? off : 0u));
        }
        /* coefficient blocks: luma block z = 4 * quadrant + j (H.264 block order), chroma block `quadrant` of the lane's plane, its DC levels */
        if (any_coded) {
            const int z = 4 * qd + j, k8 = 4 * plane + qd;
            const uint32_t cidx = FJ_GEN_COEF_IDX(ge.z), nl = (uint32_t)__popc(coded & 0xFFFFu), has_cdc = (coded >> 25) & 1u;
            const bool ybit = (coded >> z) & 1u, cbit = (coded >> (16 + k8)) & 1u;
            const uint32_t yoff = 32u * (cidx + (uint32_t)__popc(coded & ((1u << z) - 1u)));
            const uint32_t coff = 32u * (cidx + nl + has_cdc + (uint32_t)__popc((coded >> 16) & ((1u << k8) - 1u)));
            const uint32_t doff = 32u * (cidx + nl) + 8u * (uint32_t)plane;
            const H264K_GLOBAL uint8_t *py = ybit ? cf + yoff : ref0, *pc = cbit ? cf + coff : ref0, *pd = has_cdc ? cf + doff : ref0;
            const uint4 y0 = ld16g(py), y1 = ld16g(py + 16), c0 = ld16g(pc), c1 = ld16g(pc + 16);
            const uint2 d0 = ld8g(pd);
            const uint32_t ym = ybit ? ~0u : 0u, cm = cbit ? ~0u : 0u, dm = has_cdc ? ~0u : 0u;
            yl[0] = y0.x & ym; yl[1] = y0.y & ym; yl[2] = y0.z & ym; yl[3] = y0.w & ym; yl[4] = y1.x & ym; yl[5] = y1.y & ym; yl[6] = y1.z & ym; yl[7] = y1.w & ym;
            cl[0] = c0.x & cm; cl[1] = c0.y & cm; cl[2] = c0.z & cm; cl[3] = c0.w & cm; cl[4] = c1.x & cm; cl[5] = c1.y & cm; cl[6] = c1.z & cm; cl[7] = c1.w & cm;
            dcl[0] = d0.x & dm; dcl[1] = d0.y & dm;
        }
        /* ---- stage ---- */
        if (any_edge) {
#pragma unroll
            for (int i = 0; i < 7; i++) {
                const int p = j + 4 * i, lk = p & 1, lx = xs + 16 * lk;
                const uint32_t first = (vl[i].x & 255u) * 0x01010101u, last = (vl[i].w >> 24) * 0x01010101u;
                if (lx < 0) vl[i] = make_uint4(first, first, first, first);
                else if (lx >= W) vl[i] = make_uint4(last, last, last, last);
            }
#pragma unroll
            for (int i = 0; i < 5; i++) {
                const int p = j + 4 * i, ck = p & 1, cx = cxs + 8 * ck;                /* (10 is even: the tile of piece p is p & 1 in both planes) */
                const uint32_t first = (vc[i].x & 255u) * 0x01010101u, last = (vc[i].y >> 24) * 0x01010101u;
                if (cx < 0) vc[i] = make_uint2(first, first);
                else if (cx >= CW) vc[i] = make_uint2(last, last);
            }
        }
#pragma unroll
        for (int i = 0; i < 7; i++) {
            const int p = j + 4 * i, lr = p >> 1, lk = p & 1;
            if (l_on[i]) {
                uint32_t *d32 = reinterpret_cast<uint32_t *>(lw + lr * LQ_W_STRIDE + 16 * lk);
                d32[0] = vl[i].x; d32[1] = vl[i].y; d32[2] = vl[i].z; d32[3] = vl[i].w;
            }
        }
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const int p = j + 4 * i, cp = p >= 10, rem = cp ? p - 10 : p, cr = rem >> 1, ck = rem & 1;
            if (c_on[i]) {
                uint32_t *d32 = reinterpret_cast<uint32_t *>(lc + cp * 5 * LQ_C_STRIDE + cr * LQ_C_STRIDE + 8 * ck);
                d32[0] = vc[i].x; d32[1] = vc[i].y;
            }
        }
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
            const int cls = !on ? -1 : (fx | fy) == 0 ? 0 : fy == 0 ? 1 : fx == 0 ? 2 : (fx != 2 && fy != 2) ? 3 : 4;
            lb_luma_from_lds<LQ_W_STRIDE>(src, sh, cls, fx, fy, pl);
        }
        /* ======== chroma: 4x4 block `quadrant` of the lane's plane, rows 2 * half, 2 * half + 1 of it ======== */
        s2 pc[2][2];
        {
            LQ_FRESH();
            LQ_LANE();
            const int mvx = (int16_t)(ge.y & 0xFFFFu), mvy = (int32_t)ge.y >> 16;
            const int ob = lq_chroma_byte(qd, mvx), cfx = mvx & 7, cfy = mvy & 7;
            const uint32_t *q = reinterpret_cast<const uint32_t *>(lc + plane * 5 * LQ_C_STRIDE + 2 * half * LQ_C_STRIDE + (ob & ~3));
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
