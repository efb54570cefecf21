/* kernels/inter_lane_block.hip.h — the register arithmetic and the window geometry of k_recon_inter_lb and k_recon_inter_lq
 * (kernels/k_recon_inter_lanes.hip.h): one lane owns a whole 4x4 luma block and half a 4x4 chroma block.  Nothing here touches memory or other
 * lanes, so tools/probes/lane_quads_host.cpp runs this file on the CPU.  Part of kernels.hip.h (which see); not a stand-alone header. */
#pragma once
namespace h264k {

/* ------------------------------------------------------------------ luma: a 4x4 block from its 9x9 window
 * rw[r][k] = dword k of window row r: rows y-2 .. y+6, columns x-2 .. x+9 (9 used).  Output row r = window row r + 2, output
 * column i = window column i + 2.  Result o[r][0] = samples (0, 1) of row r, o[r][1] = samples (2, 3), packed 16-bit, 0..255 —
 * bit for bit what luma_from_window (k_recon_inter.hip.h) gives a lane per row of the block: the same packed first stage, the same rounding,
 * "vertical sums first" for j.  fx, fy are PER-LANE values here (a wavefront holds four motion vectors): what differs between the
 * letters of one class is a select or a byte selector in a register, the class itself is the caller's branch. */
/* the interpolation class of a quarter-sample fraction: 0 whole (G), 1 horizontal (a, b, c), 2 vertical (d, h, n), 3 diagonal (e, g, p, r),
 * 4 centre (j, f, q, i, k) */
constexpr int lb_class_of(int fx, int fy) { return (fx | fy) == 0 ? 0 : fy == 0 ? 1 : fx == 0 ? 2 : (fx != 2 && fy != 2) ? 3 : 4; }
constexpr uint32_t lb_sel(int c) { return 0x0C000C00u | (uint32_t)c | ((uint32_t)(c + 1) << 16); }      /* bytes (c, c + 1) of 8 -> two 16-bit halves */
/* (column c, column c + 1) of a window row, c = 0 .. 9 */
#define LB_CP(row, c) as_s2((c) <= 6 ? perm((row)[1], (row)[0], lb_sel((c) <= 6 ? (c) : 0)) : perm((row)[2], (row)[1], lb_sel((c) <= 6 ? 0 : (c) - 4)))
#define LB_RND5(x) pk_clip(pk(0), pk(255), ((x) + pk(16)) >> pk(5))
__device__ __forceinline__ s2 lb_tap6(s2 a, s2 b, s2 c, s2 d, s2 e, s2 f) { return a + f - pk(5) * (b + e) + pk(20) * (c + d); }
/* a.x * b.x + a.y * b.y + c in 32 bit */
__device__ __forceinline__ int lb_dot2(s2 a, s2 b, int c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sdot2(a, b, c, false);
#else
    return (int)a.x * b.x + (int)a.y * b.y + c;
#endif
}
__device__ __forceinline__ s2 lb_avg(s2 a, s2 b) { return (a + b + pk(1)) >> pk(1); }
__device__ __forceinline__ s2 lb_pick(bool c, s2 a, s2 b) { return as_s2(c ? as_u32(a) : as_u32(b)); }
/* the horizontal half-sample sums of one row: output pairs (0, 1) and (2, 3) */
__device__ __forceinline__ void lb_hsum(const uint32_t row[3], s2 &h01, s2 &h23)
{
    const s2 c0 = LB_CP(row, 0), c1 = LB_CP(row, 1), c2 = LB_CP(row, 2), c3 = LB_CP(row, 3), c4 = LB_CP(row, 4), c5 = LB_CP(row, 5), c6 = LB_CP(row, 6), c7 = LB_CP(row, 7);
    h01 = lb_tap6(c0, c1, c2, c3, c4, c5); h23 = lb_tap6(c2, c3, c4, c5, c6, c7);
}

/* G: whole-sample (rows 2..5, dwords 0..1) */
__device__ __forceinline__ void lb_luma_whole(const uint32_t rw[9][3], s2 o[4][2])
{
#pragma unroll
    for (int r = 0; r < 4; r++) { o[r][0] = LB_CP(rw[r + 2], 2); o[r][1] = LB_CP(rw[r + 2], 4); }
}
/* a, b, c: horizontal only (rows 2..5, dwords 0..2) */
__device__ __forceinline__ void lb_luma_hor(const uint32_t rw[9][3], int fx, s2 o[4][2])
{
    const uint32_t q01 = lb_sel(2) + (fx == 3 ? 0x00010001u : 0u), q23 = q01 + 0x00020002u;      /* the whole sample next to a (column 2) or c (column 3) */
    const bool quarter = fx & 1;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint32_t *row = rw[r + 2];
        s2 h01, h23;
        lb_hsum(row, h01, h23);
        h01 = LB_RND5(h01); h23 = LB_RND5(h23);
        o[r][0] = lb_pick(quarter, lb_avg(h01, as_s2(perm(row[1], row[0], q01))), h01);
        o[r][1] = lb_pick(quarter, lb_avg(h23, as_s2(perm(row[1], row[0], q23))), h23);
    }
}
/* d, h, n: vertical only (rows 0..8, dwords 0..1) */
__device__ __forceinline__ void lb_luma_ver(const uint32_t rw[9][3], int fy, s2 o[4][2])
{
    s2 a[9][2];
#pragma unroll
    for (int r = 0; r < 9; r++) { a[r][0] = LB_CP(rw[r], 2); a[r][1] = LB_CP(rw[r], 4); }
    const bool quarter = fy & 1, lower = fy == 3;
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int p = 0; p < 2; p++) {
            const s2 v = LB_RND5(lb_tap6(a[r][p], a[r + 1][p], a[r + 2][p], a[r + 3][p], a[r + 4][p], a[r + 5][p]));
            o[r][p] = lb_pick(quarter, lb_avg(v, lb_pick(lower, a[r + 3][p], a[r + 2][p])), v);
        }
}
/* e, g, p, r: average of the nearest horizontal and vertical half samples (rows 0..8; dwords 0..1, rows 2..6 dwords 0..2) */
__device__ __forceinline__ void lb_luma_diag(const uint32_t rw[9][3], int fx, int fy, s2 o[4][2])
{
    const uint32_t v01 = lb_sel(2) + (fx == 3 ? 0x00010001u : 0u), v23 = v01 + 0x00020002u;      /* h (column 2) or m (column 3) */
    const bool lower = fy == 3;                                                                  /* b (row 2) or s (row 3) */
    s2 a[9][2];
#pragma unroll
    for (int r = 0; r < 9; r++) { a[r][0] = as_s2(perm(rw[r][1], rw[r][0], v01)); a[r][1] = as_s2(perm(rw[r][1], rw[r][0], v23)); }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        uint32_t row[3];
#pragma unroll
        for (int k = 0; k < 3; k++) row[k] = lower ? rw[r + 3][k] : rw[r + 2][k];
        s2 h01, h23;
        lb_hsum(row, h01, h23);
        o[r][0] = lb_avg(LB_RND5(h01), LB_RND5(lb_tap6(a[r][0], a[r + 1][0], a[r + 2][0], a[r + 3][0], a[r + 4][0], a[r + 5][0])));
        o[r][1] = lb_avg(LB_RND5(h23), LB_RND5(lb_tap6(a[r][1], a[r + 1][1], a[r + 2][1], a[r + 3][1], a[r + 4][1], a[r + 5][1])));
    }
}
/* j, f, q, i, k (all of the window): the vertical sums of nine columns in packed 16 bit (they lie in [-2550, 10710]), the six-tap
 * filter over them in 32 bit; f / q average j with b / s, i / k with h / m — which are the vertical sums again */
__device__ __forceinline__ void lb_luma_centre(const uint32_t rw[9][3], int fx, int fy, s2 o[4][2])
{
    s2 vs[4][5];                                     /* column pair by column pair: nine pairs in flight, not forty-five */
#pragma unroll
    for (int p = 0; p < 5; p++) {
        s2 a[9];
#pragma unroll
        for (int r = 0; r < 9; r++) a[r] = LB_CP(rw[r], 2 * p);                   /* (pair 4 = columns 8, 9: only 8 is used) */
#pragma unroll
        for (int r = 0; r < 4; r++) vs[r][p] = lb_tap6(a[r], a[r + 1], a[r + 2], a[r + 3], a[r + 4], a[r + 5]);
    }
    const bool lower = fy == 3, right = fx == 3;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const s2 *vp = vs[r];
        /* the second stage as dot products of sum PAIRS with (1, -5), (20, 20), (-5, 1), accumulated in 32 bit (v_dot2_i32_i16): the even
         * outputs take the pairs as they are, the odd ones the pairs shifted by one sum — no unpacking to 32 bit */
        s2 op[4];
#pragma unroll
        for (int k = 0; k < 4; k++) op[k] = as_s2(perm(as_u32(vp[k + 1]), as_u32(vp[k]), 0x05040302u));
        const s2 wa = (s2){ 1, -5 }, wb = (s2){ 20, 20 }, wc = (s2){ -5, 1 };
        int j[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const s2 *pp = (i & 1) ? op + (i >> 1) : vp + (i >> 1);
            j[i] = clip255(lb_dot2(pp[0], wa, lb_dot2(pp[1], wb, lb_dot2(pp[2], wc, 512))) >> 10);
        }
        s2 j01 = as_s2((uint32_t)j[0] | ((uint32_t)j[1] << 16)), j23 = as_s2((uint32_t)j[2] | ((uint32_t)j[3] << 16));
        if (fy != 2) {                               /* f / q */
            uint32_t row[3];
#pragma unroll
            for (int k = 0; k < 3; k++) row[k] = lower ? rw[r + 3][k] : rw[r + 2][k];
            s2 h01, h23;
            lb_hsum(row, h01, h23);
            j01 = lb_avg(j01, LB_RND5(h01)); j23 = lb_avg(j23, LB_RND5(h23));
        } else if (fx != 2) {                        /* i / k: columns (2, 3), (4, 5) or (3, 4), (5, 6) of the vertical sums */
            const s2 m01 = lb_pick(right, as_s2(perm(as_u32(vp[2]), as_u32(vp[1]), 0x05040302u)), vp[1]);
            const s2 m23 = lb_pick(right, as_s2(perm(as_u32(vp[3]), as_u32(vp[2]), 0x05040302u)), vp[2]);
            j01 = lb_avg(j01, LB_RND5(m01)); j23 = lb_avg(j23, LB_RND5(m23));
        }
        o[r][0] = j01; o[r][1] = j23;
    }
}

/* ------------------------------------------------------------------ chroma: one row of four samples
 * (a_lo, a_hi) = bytes 0..7 of the upper source row from the first sample on (five used), (b_lo, b_hi) those of the row below;
 * w = the four bilinear weights, each in both halves.  8.4.2.2.2 in packed 16 bit (weights at most 64, samples at most 255: every partial sum fits a signed half), both pairs of the row. */
__device__ __forceinline__ void lb_chroma_row(uint32_t a_lo, uint32_t a_hi, uint32_t b_lo, uint32_t b_hi, s2 w00, s2 w10, s2 w01, s2 w11, s2 &o01, s2 &o23)
{
    const s2 p0 = as_s2(perm(a_hi, a_lo, lb_sel(0))), p1 = as_s2(perm(a_hi, a_lo, lb_sel(1))), p2 = as_s2(perm(a_hi, a_lo, lb_sel(2))), p3 = as_s2(perm(a_hi, a_lo, lb_sel(3)));
    const s2 q0 = as_s2(perm(b_hi, b_lo, lb_sel(0))), q1 = as_s2(perm(b_hi, b_lo, lb_sel(1))), q2 = as_s2(perm(b_hi, b_lo, lb_sel(2))), q3 = as_s2(perm(b_hi, b_lo, lb_sel(3)));
    o01 = (p0 * w00 + p1 * w10 + q0 * w01 + q1 * w11 + pk(32)) >> pk(6);
    o23 = (p2 * w00 + p3 * w10 + q2 * w01 + q3 * w11 + pk(32)) >> pk(6);
}

/* ------------------------------------------------------------------ residual: a 4x4 inverse transform inside one lane
 * Level blocks are raster 4x4 int16: dword 2 * i + (j >> 1) holds columns j, j + 1 of row i.  The quantiser parameters are per-lane
 * values (qp / 6 by a multiply: qp < 52). */
__device__ __forceinline__ void lb_qp_split(int qp, int &m, int &s) { s = (qp * 43) >> 8; m = qp - 6 * s; }
/* the scaled DC of chroma block i (0..3, raster 2x2) of a plane from the plane's four DC levels (8.5.11), as in mb_residual_pk */
__device__ __forceinline__ int lb_chroma_dc(uint32_t lo, uint32_t hi, int i, int qp_c)
{
    const int c0 = (int16_t)(lo & 0xFFFFu), c1 = (int32_t)lo >> 16, c2 = (int16_t)(hi & 0xFFFFu), c3 = (int32_t)hi >> 16;
    const int f = c0 + ((i & 1) ? -c1 : c1) + ((i & 2) ? -c2 : c2) + ((i == 1 || i == 2) ? -c3 : c3);
    int mc, sc;
    lb_qp_split(qp_c, mc, sc);
    const int ls = level_scale(mc, 0);
    return sc >= 1 ? (f * ls) << (sc - 1) : (f * ls) >> 1;
}
/* Packed 16 bit, luma in the low halves and the lane's chroma block in the high halves (FJ_CODED_WIDE clear: nothing wraps, see
 * mb_residual_pk): r[i][j] = residual sample (row i, column j), luma | chroma << 16.  dc = lb_chroma_dc, 0 without a DC block. */
__device__ __forceinline__ void lb_residual_pk(const uint32_t y[8], const uint32_t c[8], int qp_y, int qp_c, int dc, uint32_t r[4][4])
{
    int my, sy, mc, sc;
    lb_qp_split(qp_y, my, sy); lb_qp_split(qp_c, mc, sc);
    const s2 L0 = as_s2((uint32_t)(level_scale(my, 0) << sy) | ((uint32_t)(level_scale(mc, 0) << sc) << 16));
    const s2 L1 = as_s2((uint32_t)(level_scale(my, 1) << sy) | ((uint32_t)(level_scale(mc, 1) << sc) << 16));
    const s2 L2 = as_s2((uint32_t)(level_scale(my, 2) << sy) | ((uint32_t)(level_scale(mc, 2) << sc) << 16));
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    auto mul = [](uint32_t a, s2 b) { us2 x, z; __builtin_memcpy(&x, &a, 4); __builtin_memcpy(&z, &b, 4); x = x * z; s2 o; __builtin_memcpy(&o, &x, 4); return o; };
    s2 f[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const s2 A = (i & 1) ? L1 : L0, B = (i & 1) ? L2 : L1;
        s2 d0 = mul(perm(c[2 * i], y[2 * i], 0x05040100u), A), d1 = mul(perm(c[2 * i], y[2 * i], 0x07060302u), B);
        const s2 d2 = mul(perm(c[2 * i + 1], y[2 * i + 1], 0x05040100u), A), d3 = mul(perm(c[2 * i + 1], y[2 * i + 1], 0x07060302u), B);
        if (i == 0) d0 = as_s2(perm((uint32_t)dc, as_u32(d0), 0x05040100u));
        const s2 e0 = d0 + d2, e1 = d0 - d2, e2 = (d1 >> pk(1)) - d3, e3 = d1 + (d3 >> pk(1));
        f[i][0] = e0 + e3; f[i][1] = e1 + e2; f[i][2] = e1 - e2; f[i][3] = e0 - e3;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const s2 g0 = f[0][j] + f[2][j] + pk(32), g1 = f[0][j] - f[2][j] + pk(32);
        const s2 g2 = (f[1][j] >> pk(1)) - f[3][j], g3 = f[1][j] + (f[3][j] >> pk(1));
        r[0][j] = as_u32((g0 + g3) >> pk(6)); r[1][j] = as_u32((g1 + g2) >> pk(6)); r[2][j] = as_u32((g1 - g2) >> pk(6)); r[3][j] = as_u32((g0 - g3) >> pk(6));
    }
}
/* One block in 32 bit (FJ_CODED_WIDE), idct_quad's arithmetic: r[i][j]; returns true if a sample leaves [-512, 511] */
__device__ __forceinline__ bool lb_residual_32(const uint32_t lv[8], int qp, bool use_dc, int dc, int r[4][4])
{
    int m, sh;
    lb_qp_split(qp, m, sh);
    const int ls0 = level_scale(m, 0), ls1 = level_scale(m, 1), ls2 = level_scale(m, 2);
    int f[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int lsa = (i & 1) ? ls1 : ls0, lsb = (i & 1) ? ls2 : ls1;
        int d0 = ((int)(int16_t)(lv[2 * i] & 0xFFFFu) * lsa) << sh, d1 = (((int32_t)lv[2 * i] >> 16) * lsb) << sh;
        const int d2 = ((int)(int16_t)(lv[2 * i + 1] & 0xFFFFu) * lsa) << sh, d3 = (((int32_t)lv[2 * i + 1] >> 16) * lsb) << sh;
        if (i == 0 && use_dc) d0 = dc;
        const int e0 = d0 + d2, e1 = d0 - d2, e2 = (d1 >> 1) - d3, e3 = d1 + (d3 >> 1);
        f[i][0] = e0 + e3; f[i][1] = e1 + e2; f[i][2] = e1 - e2; f[i][3] = e0 - e3;
    }
    uint32_t over = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int e0 = f[0][j] + f[2][j], e1 = f[0][j] - f[2][j], e2 = (f[1][j] >> 1) - f[3][j], e3 = f[1][j] + (f[3][j] >> 1);
        r[0][j] = (e0 + e3 + 32) >> 6; r[1][j] = (e1 + e2 + 32) >> 6; r[2][j] = (e1 - e2 + 32) >> 6; r[3][j] = (e0 - e3 + 32) >> 6;
#pragma unroll
        for (int i = 0; i < 4; i++) over |= (uint32_t)(r[i][j] + 512);
    }
    return over > 1023u;
}

/* ------------------------------------------------------------------ a quadrant per four lanes (k_recon_inter_lq)
 * Lane j = 0..3 of a slot owns 4x4 luma block (j & 1, j >> 1) of 8x8 quadrant q (raster in the macroblock) — block z = 4 * q + j in H.264
 * block order — and rows 2 * (j & 1), 2 * (j & 1) + 1 of 4x4 chroma block q of plane j >> 1. */
/* the bits of FjMbRec.coded that reach quadrant q: its four luma blocks, its chroma block in both planes, the chroma DC block */
__device__ __forceinline__ uint32_t lq_coded_mask(uint32_t q) { return (0xFu << (4u * q)) | (0x00110000u << q) | FJ_CODED_CHROMA_DC; }
/* byte of the quadrant's window column 0 (sample column x - 2) in the staged row, which begins at the window's first tile:
 * (16 * mbx + 8 * (q & 1) + (mvx >> 2) - 2) mod 16; and of its first chroma column, (8 * mbx + 4 * (q & 1) + (mvx >> 3)) mod 8 */
__device__ __forceinline__ int lq_window_byte(int q, int mvx) { return (8 * (q & 1) + (mvx >> 2) - 2) & 15; }
__device__ __forceinline__ int lq_chroma_byte(int q, int mvx) { return (4 * (q & 1) + (mvx >> 3)) & 7; }
/* Store exchange: the lanes jbx = 0, 1 of a block row hold the left and the right 4x4 block as four row dwords each.  The left lane sends
 * rows 2, 3 and the right lane rows 0, 1 (got0, got1 = what the other lane sent); r0, r1 = two whole 8-byte rows: rows 0, 1 in the left lane,
 * rows 2, 3 in the right one. */
__device__ __forceinline__ void lq_pair_rows(const uint32_t ldw[4], uint32_t got0, uint32_t got1, int jbx, uint32_t r0[2], uint32_t r1[2])
{
    r0[0] = jbx ? got0 : ldw[0]; r0[1] = jbx ? ldw[2] : got0;
    r1[0] = jbx ? got1 : ldw[1]; r1[1] = jbx ? ldw[3] : got1;
}
/* where r0 goes in the macroblock's tile (r1: the row below, + 16), and the lane's first chroma row (the second: + 8) */
__device__ __forceinline__ int lq_luma_store_offset(int q, int j) { return (8 * (q >> 1) + 4 * (j >> 1) + 2 * (j & 1)) * 16 + 8 * (q & 1); }
__device__ __forceinline__ int lq_chroma_store_offset(int q, int j) { return T_CB + (j >> 1) * 64 + (4 * (q >> 1) + 2 * (j & 1)) * 8 + 4 * (q & 1); }

/* ------------------------------------------------------------------ a slot's staged windows: which lane fetches what, and where it goes
 * A slot (a macroblock in k_recon_inter_lb, a quadrant in k_recon_inter_lq) stages one luma window of ROWS x ROWS samples and two chroma
 * windows of CROWS x CROWS.  A window is staged tile row by tile row: a window row is the 16-byte (chroma: 8-byte) rows of the TILES (chroma:
 * 2) tiles it may cross, loaded whole and laid side by side, so byte 0 of a staged row is the first column of the window's first tile.  These
 * aligned PIECES are numbered luma p = TILES * row + tile and chroma p = 2 * CROWS * plane + 2 * row + tile; the LANES lanes of a slot take
 * them in turn, lane j the pieces j, j + LANES, ...  Pure index arithmetic: the loads and LDS stores are k_recon_inter_lanes.hip.h's. */
template <int ROWS_, int TILES_, int CROWS_, int LANES_>
struct LaneWin {
    static constexpr int ROWS = ROWS_, COLS = ROWS_, TILES = TILES_, CROWS = CROWS_, LANES = LANES_;
    static constexpr int NL = (ROWS * TILES + LANES - 1) / LANES, NC = (4 * CROWS + LANES - 1) / LANES;      /* pieces per lane */
    static_assert((TILES == 2 || TILES == 3) && 15 + COLS <= 16 * TILES && 7 + CROWS <= 16 && NL * LANES <= 128, "window shape");
    static constexpr bool luma_piece(int p) { return p < ROWS * TILES; }
    static constexpr int luma_row(int p) { return TILES == 2 ? p >> 1 : (p * 43) >> 7; }                      /* p / TILES for p < 128 */
    static constexpr int luma_tile(int p) { return p - TILES * luma_row(p); }
    /* tile k of a window row is fetched only if the window's COLS columns, which begin rel = xi - xs columns into tile 0, reach it:
     * nothing reads the bytes it would have filled */
    static constexpr bool tile_needed(int k, int rel) { return rel + COLS > 16 * k; }
    static constexpr bool chroma_piece(int p) { return p < 4 * CROWS; }
    static constexpr int chroma_plane(int p) { return p >= 2 * CROWS; }
    static constexpr int chroma_row(int p) { return (p - 2 * CROWS * chroma_plane(p)) >> 1; }
    static constexpr int chroma_tile(int p) { return (p - 2 * CROWS * chroma_plane(p)) & 1; }
    /* bytes of the slot's windows at staged rows of WSTRIDE / CSTRIDE bytes (luma, then the two chroma planes), and where a piece lies in them */
    static constexpr int bytes(int wstride, int cstride) { return ROWS * wstride + 2 * CROWS * cstride; }
    static constexpr int luma_at(int wstride, int row, int tile) { return row * wstride + 16 * tile; }
    static constexpr int chroma_at(int wstride, int cstride, int plane, int row, int tile) { return ROWS * wstride + (plane * CROWS + row) * cstride + 8 * tile; }
};
typedef LaneWin<21, 3, 9, 16> LbWin;                 /* a macroblock: 16 + 5 luma rows and columns, 8 + 1 chroma; a lane per 4x4 block */
typedef LaneWin<13, 2, 5, 4> LqWin;                  /* a quadrant: 8 + 5 and 4 + 1 */
/* A piece is a tile row of the reference picture, pictures are whole tiles: a piece lies wholly inside the picture, wholly left of it or wholly
 * right of it.  It is loaded from the tile and row clamped into the picture (byte offset in the picture's tiles; x a multiple of 16 / 8, w x h
 * the plane), and where lw_side says it lay outside, its first (-1) or last (+1) sample is spread over it: h264bsdFillBlock's clamping of every
 * sample, src/h264bsd_reconstruct.c:2244. */
__device__ __forceinline__ uint32_t lw_luma_piece(int wmb, int w, int h, int x, int y)
{
    const int xx = clip3(0, w - 16, x), yy = clip3(0, h - 1, y);
    return (uint32_t)((yy >> 4) * wmb + (xx >> 4)) * (uint32_t)TILE + (uint32_t)((yy & 15) << 4);
}
__device__ __forceinline__ uint32_t lw_chroma_piece(int wmb, int plane, int w, int h, int x, int y)
{
    const int xx = clip3(0, w - 8, x), yy = clip3(0, h - 1, y);
    return (uint32_t)((yy >> 3) * wmb + (xx >> 3)) * (uint32_t)TILE + (uint32_t)(T_CB + (plane << 6) + ((yy & 7) << 3));
}
constexpr int lw_side(int x, int w) { return x < 0 ? -1 : x >= w ? 1 : 0; }
/* the shared rules above are the ones the two kernels used to spell out by hand, for every piece and every rel */
constexpr bool lb_win_as_written()
{
    for (int rel = 0; rel < 16; rel++)
        for (int p = 0; p < 64; p++) {
            const int lr = p / 3, lk = p % 3, cp = p >= 18, rem = cp ? p - 18 : p;
            if (LbWin::luma_row(p) != lr || LbWin::luma_tile(p) != lk || LbWin::luma_piece(p) != (p < 63)) return false;
            if (LbWin::tile_needed(lk, rel) != (lk < 2 || rel >= 12)) return false;
            if (p < 48 && LbWin::chroma_piece(p) != (p < 36)) return false;
            if (p < 36 && (LbWin::chroma_plane(p) != cp || LbWin::chroma_row(p) != (rem >> 1) || LbWin::chroma_tile(p) != (rem & 1))) return false;
        }
    return LbWin::NL == 4 && LbWin::NC == 3;
}
constexpr bool lq_win_as_written()
{
    for (int rel = 0; rel < 16; rel++)
        for (int p = 0; p < 28; p++) {
            const int lr = p >> 1, lk = p & 1, cp = p >= 10, rem = cp ? p - 10 : p;
            if (LqWin::luma_row(p) != lr || LqWin::luma_tile(p) != lk || LqWin::luma_piece(p) != (p < 26)) return false;
            if (LqWin::tile_needed(lk, rel) != (lk == 0 || rel >= 4)) return false;
            if (p < 20 && (!LqWin::chroma_piece(p) || LqWin::chroma_plane(p) != cp || LqWin::chroma_row(p) != (rem >> 1) || LqWin::chroma_tile(p) != (rem & 1))) return false;
        }
    return LqWin::NL == 7 && LqWin::NC == 5;
}
static_assert(lb_win_as_written(), "21 x 48 window: p / 3, p < 63, lk < 2 || rel >= 12, p < 36");
static_assert(lq_win_as_written(), "13 x 32 window: p >> 1, p < 26, lk == 0 || rel >= 4, every chroma piece");

} // namespace h264k
