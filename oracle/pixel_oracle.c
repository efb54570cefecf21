/*
 * pixel_oracle.c — TEST INFRASTRUCTURE ONLY: a plain-C, CPU restatement of the reference's pixel
 * path, consuming the same packed frame jobs (h264bsd_amd/csrc/framejob.h) the HIP kernels consume.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this library.  The
 * product (libh264bsd_mi355x.so) never links, imports or falls back to it.
 *
 * PARITY PIN: pinned.  There are no golden vectors in the reference repository; the
 * pin is the compiled reference itself (oracle/_ref, built from /root/reference/src by
 * oracle/Makefile): host parser + this oracle reproduce the reference's decoded frames bit-exactly
 * on all 219 frames of the three bundled streams (sha256 values of SURVEY.md §8c, per-frame
 * fixtures in tests/golden/), and tests/test_oracle_vs_ref.py compares the individual stages
 * below with the reference's own functions on random inputs when oracle/_ref is present.
 *
 * Each stage is written from the H.264 specification (clause cited) and names the reference code
 * whose behaviour it restates:
 *   dequant + 4x4 inverse transform  8.5.12   src/h264bsd_transform.c:97-234  (h264bsdProcessBlock)
 *   Intra16x16 luma DC               8.5.10   src/h264bsd_transform.c:255-338 (h264bsdProcessLumaDc)
 *   chroma DC                        8.5.11   src/h264bsd_transform.c:359-401 (h264bsdProcessChromaDc)
 *   residual orchestration                    src/h264bsd_macroblock_layer.c:1340-1421 (ProcessResidual)
 *   intra prediction                 8.3      src/h264bsd_intra_prediction.c:478-1830
 *   inter prediction                 8.4.2.2  src/h264bsd_reconstruct.c:1818 (h264bsdPredictSamples),
 *                                             :2244 (h264bsdFillBlock = clamp-to-edge), :415 (PredictChroma)
 *   write-back / residual add                 src/h264bsd_image.c:81,172
 *   deblocking                       8.7      src/h264bsd_deblocking.c:575-1745 (h264bsdFilterPicture)
 *   colour conversion                         src/h264bsd_decoder.c:1163-1370 (h264bsdConvertTo*)
 *   concealment of lost macroblocks           src/h264bsd_conceal.c:266-637 (ConcealMb, Transform); the walking
 *                                             order of h264bsdConceal (:124-260) arrives in the frame job
 * (the concealment is pinned twice: tests/test_damaged_streams.py against the compiled reference on damaged streams, which
 *  reach what they happen to lose; tests/test_concealed_jobs.py on chosen neighbour masks and border samples — against a plain
 *  integer model on hand-built jobs, and against the compiled reference on all-I_PCM streams that leave a slice group out;
 *  intra prediction and the intra residual likewise: tests/test_oracle_stage_pins.py against the reference's three prediction
 *  functions, under every availability mask on random modes and on every enumerated (block, mode) cell of Intra4x4, with no
 *  residual; tests/test_intra_jobs.py against a plain integer model, tests/intra_model.py, on hand-built jobs that hold every
 *  cell, the above-right rule of block 5, both luma DC and the chroma DC scalings, FJ_CODED_LUMA_DC_RAW, residuals at both ends
 *  of [-512, 511] and both clips; the transforms themselves against h264bsdProcessBlock / LumaDc / ChromaDc in
 *  tests/test_oracle_vs_ref.py)
 * oracle_deblock_census() is oracle_deblock() that also counts which decisions the filter takes (strength rules, gates, clips,
 * saturation): tests/test_structured_jobs.py holds the hand-built test pictures to taking every one of them.
 * Known, deliberate gap: the reference turns a residual outside [-512,511] into a decode error
 * (transform.c:184-188); the oracle (like the kernels) just clips after prediction.
 */
#include <stdint.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include "framejob.h"

typedef uint8_t u8;

static inline int clip255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
static inline int clip3(int lo, int hi, int v) { return v < lo ? lo : v > hi ? hi : v; }
static inline int iabs(int v) { return v < 0 ? -v : v; }

/* z-order (H.264 4x4 block order) of the block at (x,y) */
static inline int z_of(int x, int y) { return ((y >> 1) << 3) | ((x >> 1) << 2) | ((y & 1) << 1) | (x & 1); }
static const u8 Z_X[16] = { 0, 1, 0, 1, 2, 3, 2, 3, 0, 1, 0, 1, 2, 3, 2, 3 };
static const u8 Z_Y[16] = { 0, 0, 1, 1, 0, 0, 1, 1, 2, 2, 3, 3, 2, 2, 3, 3 };

/* ------------------------------------------------------------------ transforms */
static const int level_scale[6][3] = { /* (even,even) (mixed) (odd,odd) */
    { 10, 13, 16 }, { 11, 14, 18 }, { 13, 16, 20 }, { 14, 18, 23 }, { 16, 20, 25 }, { 18, 23, 29 } };

/* 8.5.12: c[] raster levels -> r[] raster residual.  dc_given: element 0 is already dequantised */
void oracle_idct4x4(const int16_t *c, int qp, int dc_given, int dc, int *r)
{
    int d[16], f[16];
    const int *ls = level_scale[qp % 6];
    const int sh = qp / 6;
    for (int i = 0; i < 16; i++) {
        const int x = i & 3, y = i >> 2;
        const int k = ((x & 1) && (y & 1)) ? 2 : ((x & 1) || (y & 1)) ? 1 : 0;
        d[i] = (c[i] * ls[k]) << sh;
    }
    if (dc_given) d[0] = dc;
    for (int y = 0; y < 4; y++) {
        const int *s = d + 4 * y;
        int e0 = s[0] + s[2], e1 = s[0] - s[2], e2 = (s[1] >> 1) - s[3], e3 = s[1] + (s[3] >> 1);
        f[4 * y + 0] = e0 + e3; f[4 * y + 1] = e1 + e2; f[4 * y + 2] = e1 - e2; f[4 * y + 3] = e0 - e3;
    }
    for (int x = 0; x < 4; x++) {
        int s0 = f[x], s1 = f[4 + x], s2 = f[8 + x], s3 = f[12 + x];
        int e0 = s0 + s2, e1 = s0 - s2, e2 = (s1 >> 1) - s3, e3 = s1 + (s3 >> 1);
        r[x] = (e0 + e3 + 32) >> 6; r[4 + x] = (e1 + e2 + 32) >> 6;
        r[8 + x] = (e1 - e2 + 32) >> 6; r[12 + x] = (e0 - e3 + 32) >> 6;
    }
}

/* 8.5.10: c raster 4x4 of DC levels -> dc[16] (raster: dc[4*i+j] belongs to the block at row i, col j) */
void oracle_luma_dc(const int16_t *c, int qp, int *dc)
{
    int t[16], f[16];
    for (int i = 0; i < 4; i++) {
        int a = c[4 * i], b = c[4 * i + 1], cc = c[4 * i + 2], d = c[4 * i + 3];
        t[4 * i] = a + b + cc + d; t[4 * i + 1] = a + b - cc - d; t[4 * i + 2] = a - b - cc + d; t[4 * i + 3] = a - b + cc - d;
    }
    for (int j = 0; j < 4; j++) {
        int a = t[j], b = t[4 + j], cc = t[8 + j], d = t[12 + j];
        f[j] = a + b + cc + d; f[4 + j] = a + b - cc - d; f[8 + j] = a - b - cc + d; f[12 + j] = a - b + cc - d;
    }
    const int ls = level_scale[qp % 6][0], q = qp / 6;
    for (int i = 0; i < 16; i++) {
        if (q >= 2) dc[i] = (f[i] * ls) << (q - 2);
        else dc[i] = (f[i] * ls + (1 << (1 - q))) >> (2 - q);
    }
}

/* 8.5.11: c[0..3] 2x2 raster -> dc[0..3] */
void oracle_chroma_dc(const int16_t *c, int qpc, int *dc)
{
    int f0 = c[0] + c[1] + c[2] + c[3], f1 = c[0] - c[1] + c[2] - c[3];
    int f2 = c[0] + c[1] - c[2] - c[3], f3 = c[0] - c[1] - c[2] + c[3];
    const int ls = level_scale[qpc % 6][0], q = qpc / 6;
    int f[4] = { f0, f1, f2, f3 };
    for (int i = 0; i < 4; i++) dc[i] = q >= 1 ? (f[i] * ls) << (q - 1) : (f[i] * ls) >> 1;
}

/* residual of one macroblock: res_y[256] raster 16x16, res_c[2][64] raster 8x8 */
static void mb_residual(const FjMbRec *r, const int16_t *coef_base, int *res_y, int *res_c)
{
    const int16_t *p = coef_base + 16 * (size_t)r->coef_idx;
    int dcy[16];
    int have_dcy = 0;
    memset(res_y, 0, 256 * sizeof(int));
    memset(res_c, 0, 128 * sizeof(int));
    if (r->coded & FJ_CODED_LUMA_DC) {
        /* FJ_CODED_LUMA_DC_RAW (damaged streams only): the block already holds the DC values, reference
         * macroblock_layer.c:1366-1374 with totalCoeff[24] == 0 */
        if (r->coded & FJ_CODED_LUMA_DC_RAW) for (int i = 0; i < 16; i++) dcy[i] = p[i];
        else oracle_luma_dc(p, r->qp_y, dcy);
        p += 16; have_dcy = 1;
    }
    for (int z = 0; z < 16; z++) {
        static const int16_t zero[16] = { 0 };
        const int bx = Z_X[z], by = Z_Y[z];
        const int has_ac = (r->coded >> z) & 1;
        const int dc = have_dcy ? dcy[4 * by + bx] : 0;
        if (!has_ac && !dc) continue;
        int out[16];
        oracle_idct4x4(has_ac ? p : zero, r->qp_y, r->kind == FJ_MB_I16x16, dc, out);
        if (has_ac) p += 16;
        for (int i = 0; i < 16; i++) res_y[(4 * by + (i >> 2)) * 16 + 4 * bx + (i & 3)] = out[i];
    }
    int dcc[8] = { 0 };
    if (r->coded & FJ_CODED_CHROMA_DC) { oracle_chroma_dc(p, r->qp_c, dcc); oracle_chroma_dc(p + 4, r->qp_c, dcc + 4); p += 16; }
    for (int k = 0; k < 8; k++) {
        static const int16_t zero[16] = { 0 };
        const int has_ac = (r->coded >> (16 + k)) & 1;
        if (!has_ac && !dcc[k]) continue;
        int out[16];
        oracle_idct4x4(has_ac ? p : zero, r->qp_c, 1, dcc[k], out);
        if (has_ac) p += 16;
        const int bx = k & 1, by = (k >> 1) & 1;
        int *dst = res_c + 64 * (k >> 2);
        for (int i = 0; i < 16; i++) dst[(4 * by + (i >> 2)) * 8 + 4 * bx + (i & 3)] = out[i];
    }
}

/* ------------------------------------------------------------------ frame view */
typedef struct Frame { u8 *y, *cb, *cr; int w, h; } Frame;   /* w,h in luma samples */
static Frame frame_view(u8 *base, int wmb, int hmb)
{
    Frame f;
    f.w = wmb * 16; f.h = hmb * 16;
    f.y = base; f.cb = base + (size_t)f.w * f.h; f.cr = f.cb + (size_t)(f.w / 2) * (f.h / 2);
    return f;
}

/* ------------------------------------------------------------------ intra prediction, 8.3 */
static void intra4x4_pred(int mode, const int *top /* [-1..7] via top[1+k] */, const int *left /* [-1..3] via left[1+k] */,
                          int has_top, int has_left, int *pred)
{
#define T(k) top[1 + (k)]
#define L(k) left[1 + (k)]
    for (int y = 0; y < 4; y++)
        for (int x = 0; x < 4; x++) {
            int v;
            switch (mode) {
            case 0: v = T(x); break;
            case 1: v = L(y); break;
            case 2:
                if (has_top && has_left) v = (T(0) + T(1) + T(2) + T(3) + L(0) + L(1) + L(2) + L(3) + 4) >> 3;
                else if (has_left) v = (L(0) + L(1) + L(2) + L(3) + 2) >> 2;
                else if (has_top) v = (T(0) + T(1) + T(2) + T(3) + 2) >> 2;
                else v = 128;
                break;
            case 3:
                v = (x == 3 && y == 3) ? (T(6) + 3 * T(7) + 2) >> 2 : (T(x + y) + 2 * T(x + y + 1) + T(x + y + 2) + 2) >> 2;
                break;
            case 4:
                if (x > y) v = (T(x - y - 2) + 2 * T(x - y - 1) + T(x - y) + 2) >> 2;
                else if (x < y) v = (L(y - x - 2) + 2 * L(y - x - 1) + L(y - x) + 2) >> 2;
                else v = (T(0) + 2 * T(-1) + L(0) + 2) >> 2;
                break;
            case 5: {
                const int zz = 2 * x - y;
                if (zz >= 0 && !(zz & 1)) v = (T(x - (y >> 1) - 1) + T(x - (y >> 1)) + 1) >> 1;
                else if (zz >= 0) v = (T(x - (y >> 1) - 2) + 2 * T(x - (y >> 1) - 1) + T(x - (y >> 1)) + 2) >> 2;
                else if (zz == -1) v = (L(0) + 2 * T(-1) + T(0) + 2) >> 2;
                else v = (L(y - 1) + 2 * L(y - 2) + L(y - 3) + 2) >> 2;
                break;
            }
            case 6: {
                const int zz = 2 * y - x;
                if (zz >= 0 && !(zz & 1)) v = (L(y - (x >> 1) - 1) + L(y - (x >> 1)) + 1) >> 1;
                else if (zz >= 0) v = (L(y - (x >> 1) - 2) + 2 * L(y - (x >> 1) - 1) + L(y - (x >> 1)) + 2) >> 2;
                else if (zz == -1) v = (L(0) + 2 * T(-1) + T(0) + 2) >> 2;
                else v = (T(x - 1) + 2 * T(x - 2) + T(x - 3) + 2) >> 2;
                break;
            }
            case 7:
                v = !(y & 1) ? (T(x + (y >> 1)) + T(x + (y >> 1) + 1) + 1) >> 1
                             : (T(x + (y >> 1)) + 2 * T(x + (y >> 1) + 1) + T(x + (y >> 1) + 2) + 2) >> 2;
                break;
            default: {
                const int zz = x + 2 * y;
                if (zz > 5) v = L(3);
                else if (zz == 5) v = (L(2) + 3 * L(3) + 2) >> 2;
                else if (!(zz & 1)) v = (L(y + (x >> 1)) + L(y + (x >> 1) + 1) + 1) >> 1;
                else v = (L(y + (x >> 1)) + 2 * L(y + (x >> 1) + 1) + L(y + (x >> 1) + 2) + 2) >> 2;
                break;
            }
            }
            pred[4 * y + x] = v;
        }
#undef T
#undef L
}

static void recon_intra4x4(const FjMbRec *r, Frame *f, int mbx, int mby, const int *res_y)
{
    for (int z = 0; z < 16; z++) {
        const int bx = Z_X[z], by = Z_Y[z];
        const int x0 = mbx * 16 + bx * 4, y0 = mby * 16 + by * 4;
        const int mode = (r->i4mode[z >> 1] >> ((z & 1) * 4)) & 15;
        const int has_left = bx > 0 || (r->avail & FJ_AVAIL_A);
        const int has_top = by > 0 || (r->avail & FJ_AVAIL_B);
        int has_tl, has_tr;
        if (bx > 0 && by > 0) has_tl = 1;
        else if (by > 0) has_tl = (r->avail & FJ_AVAIL_A) != 0;
        else if (bx > 0) has_tl = (r->avail & FJ_AVAIL_B) != 0;
        else has_tl = (r->avail & FJ_AVAIL_D) != 0;
        if (by == 0) has_tr = bx < 3 ? (r->avail & FJ_AVAIL_B) != 0 : (r->avail & FJ_AVAIL_C) != 0;
        else has_tr = bx < 3 && z_of(bx + 1, by - 1) < z;
        int top[9], left[5], pred[16];
        for (int k = 0; k < 9; k++) top[k] = 128;
        for (int k = 0; k < 5; k++) left[k] = 128;
        if (has_top) for (int k = 0; k < 4; k++) top[1 + k] = f->y[(size_t)(y0 - 1) * f->w + x0 + k];
        if (has_top && has_tr) for (int k = 4; k < 8; k++) top[1 + k] = f->y[(size_t)(y0 - 1) * f->w + x0 + k];
        else if (has_top) for (int k = 4; k < 8; k++) top[1 + k] = top[4];
        if (has_left) for (int k = 0; k < 4; k++) left[1 + k] = f->y[(size_t)(y0 + k) * f->w + x0 - 1];
        if (has_tl) top[0] = left[0] = f->y[(size_t)(y0 - 1) * f->w + x0 - 1];
        intra4x4_pred(mode, top, left, has_top, has_left, pred);
        for (int i = 0; i < 16; i++) {
            const int yy = i >> 2, xx = i & 3;
            f->y[(size_t)(y0 + yy) * f->w + x0 + xx] =
                (u8)clip255(pred[i] + res_y[(4 * by + yy) * 16 + 4 * bx + xx]);
        }
    }
}

static void recon_intra16x16(const FjMbRec *r, Frame *f, int mbx, int mby, const int *res_y)
{
    const int x0 = mbx * 16, y0 = mby * 16, W = f->w;
    const int hl = (r->avail & FJ_AVAIL_A) != 0, ht = (r->avail & FJ_AVAIL_B) != 0;
    int top[17], left[17];   /* [0] = corner */
    for (int k = 0; k < 17; k++) top[k] = left[k] = 128;
    if (ht) for (int k = 0; k < 16; k++) top[1 + k] = f->y[(size_t)(y0 - 1) * W + x0 + k];
    if (hl) for (int k = 0; k < 16; k++) left[1 + k] = f->y[(size_t)(y0 + k) * W + x0 - 1];
    if (r->avail & FJ_AVAIL_D) top[0] = left[0] = f->y[(size_t)(y0 - 1) * W + x0 - 1];
    const int mode = r->pred & 3;
    int dc = 128, a = 0, b = 0, c = 0;
    if (mode == 2) {
        int st = 0, sl = 0;
        for (int k = 1; k <= 16; k++) { st += top[k]; sl += left[k]; }
        if (ht && hl) dc = (st + sl + 16) >> 5;
        else if (hl) dc = (sl + 8) >> 4;
        else if (ht) dc = (st + 8) >> 4;
    } else if (mode == 3) {
        int H = 0, V = 0;
        for (int k = 0; k < 8; k++) {
            H += (k + 1) * (top[1 + 8 + k] - top[1 + 6 - k]);
            V += (k + 1) * (left[1 + 8 + k] - left[1 + 6 - k]);
        }
        a = 16 * (left[16] + top[16]); b = (5 * H + 32) >> 6; c = (5 * V + 32) >> 6;
    }
    for (int y = 0; y < 16; y++)
        for (int x = 0; x < 16; x++) {
            int p;
            if (mode == 0) p = top[1 + x];
            else if (mode == 1) p = left[1 + y];
            else if (mode == 2) p = dc;
            else p = clip255((a + b * (x - 7) + c * (y - 7) + 16) >> 5);
            f->y[(size_t)(y0 + y) * W + x0 + x] = (u8)clip255(p + res_y[16 * y + x]);
        }
}

static void recon_intra_chroma(const FjMbRec *r, Frame *f, int mbx, int mby, const int *res_c)
{
    const int x0 = mbx * 8, y0 = mby * 8, W = f->w / 2;
    const int hl = (r->avail & FJ_AVAIL_A) != 0, ht = (r->avail & FJ_AVAIL_B) != 0;
    const int mode = (r->pred >> 2) & 3;
    for (int pl = 0; pl < 2; pl++) {
        u8 *P = pl ? f->cr : f->cb;
        const int *res = res_c + 64 * pl;
        int top[9], left[9];
        for (int k = 0; k < 9; k++) top[k] = left[k] = 128;
        if (ht) for (int k = 0; k < 8; k++) top[1 + k] = P[(size_t)(y0 - 1) * W + x0 + k];
        if (hl) for (int k = 0; k < 8; k++) left[1 + k] = P[(size_t)(y0 + k) * W + x0 - 1];
        if (r->avail & FJ_AVAIL_D) top[0] = left[0] = P[(size_t)(y0 - 1) * W + x0 - 1];
        int dc[4] = { 128, 128, 128, 128 }, a = 0, b = 0, c = 0;
        if (mode == 0) {
            for (int k = 0; k < 4; k++) {
                const int xo = (k & 1) * 4, yo = (k >> 1) * 4;
                int st = 0, sl = 0;
                for (int i = 0; i < 4; i++) { st += top[1 + xo + i]; sl += left[1 + yo + i]; }
                if (k == 0 || k == 3) {
                    if (ht && hl) dc[k] = (st + sl + 4) >> 3;
                    else if (ht) dc[k] = (st + 2) >> 2;
                    else if (hl) dc[k] = (sl + 2) >> 2;
                } else if (k == 1) {
                    if (ht) dc[k] = (st + 2) >> 2; else if (hl) dc[k] = (sl + 2) >> 2;
                } else {
                    if (hl) dc[k] = (sl + 2) >> 2; else if (ht) dc[k] = (st + 2) >> 2;
                }
            }
        } else if (mode == 3) {
            int H = 0, V = 0;
            for (int k = 0; k < 4; k++) {
                H += (k + 1) * (top[1 + 4 + k] - top[1 + 2 - k]);
                V += (k + 1) * (left[1 + 4 + k] - left[1 + 2 - k]);
            }
            a = 16 * (left[8] + top[8]); b = (34 * H + 32) >> 6; c = (34 * V + 32) >> 6;
        }
        for (int y = 0; y < 8; y++)
            for (int x = 0; x < 8; x++) {
                int p;
                if (mode == 0) p = dc[(y >> 2) * 2 + (x >> 2)];
                else if (mode == 1) p = left[1 + y];
                else if (mode == 2) p = top[1 + x];
                else p = clip255((a + b * (x - 3) + c * (y - 3) + 16) >> 5);
                P[(size_t)(y0 + y) * W + x0 + x] = (u8)clip255(p + res[8 * y + x]);
            }
    }
}

/* ------------------------------------------------------------------ inter prediction, 8.4.2.2 */
static inline int ref_px(const u8 *p, int w, int h, int x, int y)
{
    x = x < 0 ? 0 : x >= w ? w - 1 : x;
    y = y < 0 ? 0 : y >= h ? h - 1 : y;
    return p[(size_t)y * w + x];
}
static inline int tap6(int a, int b, int c, int d, int e, int f) { return a - 5 * b + 20 * c + 20 * d - 5 * e + f; }

/* one luma sample at integer (x,y) + quarter-sample fraction (fx,fy), 8.4.2.2.1 */
int oracle_luma_sample(const u8 *p, int w, int h, int x, int y, int fx, int fy)
{
#define G(dx, dy) ref_px(p, w, h, x + (dx), y + (dy))
#define B1(dx, dy) tap6(G((dx) - 2, dy), G((dx) - 1, dy), G(dx, dy), G((dx) + 1, dy), G((dx) + 2, dy), G((dx) + 3, dy))
#define H1(dx, dy) tap6(G(dx, (dy) - 2), G(dx, (dy) - 1), G(dx, dy), G(dx, (dy) + 1), G(dx, (dy) + 2), G(dx, (dy) + 3))
#define HB(dx, dy) clip255((B1(dx, dy) + 16) >> 5)   /* b at (x+dx+1/2, y+dy) */
#define HH(dx, dy) clip255((H1(dx, dy) + 16) >> 5)   /* h at (x+dx, y+dy+1/2) */
    if (!fx && !fy) return G(0, 0);
    if (!fy) { int b = HB(0, 0); return fx == 2 ? b : (b + (fx == 1 ? G(0, 0) : G(1, 0)) + 1) >> 1; }
    if (!fx) { int hh = HH(0, 0); return fy == 2 ? hh : (hh + (fy == 1 ? G(0, 0) : G(0, 1)) + 1) >> 1; }
    if (fx == 2 || fy == 2) {
        int j1 = tap6(B1(0, -2), B1(0, -1), B1(0, 0), B1(0, 1), B1(0, 2), B1(0, 3));
        int j = clip255((j1 + 512) >> 10);
        if (fx == 2 && fy == 2) return j;
        if (fx == 2) return (j + (fy == 1 ? HB(0, 0) : HB(0, 1)) + 1) >> 1;      /* f, q */
        return (j + (fx == 1 ? HH(0, 0) : HH(1, 0)) + 1) >> 1;                   /* i, k */
    }
    /* e, g, p, r: diagonal pairs of the nearest b/s and h/m */
    {
        int b = fy == 1 ? HB(0, 0) : HB(0, 1);
        int hh = fx == 1 ? HH(0, 0) : HH(1, 0);
        return (b + hh + 1) >> 1;
    }
#undef G
#undef B1
#undef H1
#undef HB
#undef HH
}

int oracle_chroma_sample(const u8 *p, int w, int h, int x, int y, int fx, int fy)
{
    int A = ref_px(p, w, h, x, y), B = ref_px(p, w, h, x + 1, y);
    int C = ref_px(p, w, h, x, y + 1), D = ref_px(p, w, h, x + 1, y + 1);
    return ((8 - fx) * (8 - fy) * A + fx * (8 - fy) * B + (8 - fx) * fy * C + fx * fy * D + 32) >> 6;
}

static void recon_inter(const FjMbRec *r, const int16_t (*mv)[2], Frame *f, u8 *const *slots, int wmb, int hmb,
                        int mbx, int mby, const int *res_y, const int *res_c)
{
    for (int blk = 0; blk < 16; blk++) {
        const int bx = blk & 3, by = blk >> 2;
        Frame ref = frame_view(slots[r->ref_slot[(by >> 1) * 2 + (bx >> 1)]], wmb, hmb);
        const int mvx = mv[blk][0], mvy = mv[blk][1];
        const int x0 = mbx * 16 + bx * 4, y0 = mby * 16 + by * 4;
        for (int y = 0; y < 4; y++)
            for (int x = 0; x < 4; x++) {
                int p = oracle_luma_sample(ref.y, ref.w, ref.h, x0 + x + (mvx >> 2), y0 + y + (mvy >> 2), mvx & 3, mvy & 3);
                f->y[(size_t)(y0 + y) * f->w + x0 + x] = (u8)clip255(p + res_y[(4 * by + y) * 16 + 4 * bx + x]);
            }
        const int cx0 = mbx * 8 + bx * 2, cy0 = mby * 8 + by * 2, cw = f->w / 2, ch = f->h / 2;
        for (int y = 0; y < 2; y++)
            for (int x = 0; x < 2; x++) {
                int pb = oracle_chroma_sample(ref.cb, cw, ch, cx0 + x + (mvx >> 3), cy0 + y + (mvy >> 3), mvx & 7, mvy & 7);
                int pr = oracle_chroma_sample(ref.cr, cw, ch, cx0 + x + (mvx >> 3), cy0 + y + (mvy >> 3), mvx & 7, mvy & 7);
                const int ri = (2 * by + y) * 8 + 2 * bx + x;
                f->cb[(size_t)(cy0 + y) * cw + cx0 + x] = (u8)clip255(pb + res_c[ri]);
                f->cr[(size_t)(cy0 + y) * cw + cx0 + x] = (u8)clip255(pr + res_c[64 + ri]);
            }
    }
}

/* ------------------------------------------------------------------ reconstruction of a picture */
static int check_blob(const uint8_t *blob)
{
    const FjHeader *h = (const FjHeader *)blob;
    return h->magic == FJ_MAGIC ? 0 : -1;
}

/* The motion vectors of a finished frame job as a dense array [n_mbs][16][2] (raster 4x4 order), malloc'ed: a macroblock with
 * FJ_PRED_UNIFORM_MV carries its one vector in the record, the others have sixteen in the sparse section at mvx_off
 * (framejob.h); macroblocks that are not inter coded have none (zeros). */
static int16_t (*dense_mvs(const uint8_t *blob))[16][2]
{
    const FjHeader *h = (const FjHeader *)blob;
    const FjMbRec *recs = (const FjMbRec *)(blob + h->rec_off);
    const int16_t (*mvx)[16][2] = (const int16_t (*)[16][2])(blob + h->mvx_off);
    int16_t (*mvs)[16][2] = (int16_t (*)[16][2])calloc((size_t)h->n_mbs + 1, 64);
    if (!mvs) return NULL;
    for (uint32_t a = 0; a < h->n_mbs; a++) {
        const FjMbRec *r = &recs[a];
        if (r->kind != FJ_MB_INTER) continue;
        if (r->pred & FJ_PRED_UNIFORM_MV) for (int b = 0; b < 16; b++) { mvs[a][b][0] = r->mv[0]; mvs[a][b][1] = r->mv[1]; }
        else if (r->mvx < h->n_mvx) memcpy(mvs[a], mvx[r->mvx], 64);
    }
    return mvs;
}

/* un-deblocked picture into slots[cur_slot]; macroblocks are processed in raster order, which
 * satisfies every dependency (the reference decodes in slice order; pixels do not depend on it) */
/* ------------------------------------------------------------------ concealment of lost macroblocks */
/* reference Transform(), src/h264bsd_conceal.c:589-637: inverse transform when only the DC, the lowest horizontal
 * (d[1]) and the lowest vertical (d[4]) coefficient can be non-zero */
static void conceal_transform(int *d)
{
    if (!d[1] && !d[4]) {
        for (int i = 1; i < 16; i++) d[i] = d[0];
        return;
    }
    int t0 = d[0], t1 = d[1];
    d[0] = t0 + t1; d[1] = t0 + (t1 >> 1); d[2] = t0 - (t1 >> 1); d[3] = t0 - t1;
    t0 = d[4];
    d[5] = d[6] = d[7] = t0;
    for (int c = 0; c < 4; c++) {
        t0 = d[c]; t1 = d[4 + c];
        d[c] = t0 + t1; d[4 + c] = t0 + (t1 >> 1); d[8 + c] = t0 - (t1 >> 1); d[12 + c] = t0 - t1;
    }
}

/* One plane of reference ConcealMb (src/h264bsd_conceal.c:346-560): `size` = 16 (luma) or 8 (chroma); the block is
 * rebuilt from the sums of four groups of size/4 border samples on each usable side. */
static void conceal_plane(u8 *pl, int stride, int x0, int y0, int size, unsigned used)
{
    const int g = size / 4, sh = size == 16 ? 0 : 1;      /* luma shifts are one larger than chroma */
    int fp[16] = { 0 }, a[4] = { 0 }, b[4] = { 0 }, l[4] = { 0 }, r[4] = { 0 };
    int j = 0, hor = 0, ver = 0;
    const int A = (used & FJ_CONC_ABOVE) != 0, B = (used & FJ_CONC_BELOW) != 0, L = (used & FJ_CONC_LEFT) != 0,
              R = (used & FJ_CONC_RIGHT) != 0;
    for (int k = 0; k < 4; k++)
        for (int i = 0; i < g; i++) {
            if (A) a[k] += pl[(size_t)(y0 - 1) * stride + x0 + k * g + i];
            if (B) b[k] += pl[(size_t)(y0 + size) * stride + x0 + k * g + i];
            if (L) l[k] += pl[(size_t)(y0 + k * g + i) * stride + x0 - 1];
            if (R) r[k] += pl[(size_t)(y0 + k * g + i) * stride + x0 + size];
        }
    if (A) { j++; hor++; fp[0] += a[0] + a[1] + a[2] + a[3]; fp[1] += a[0] + a[1] - a[2] - a[3]; }
    if (B) { j++; hor++; fp[0] += b[0] + b[1] + b[2] + b[3]; fp[1] += b[0] + b[1] - b[2] - b[3]; }
    if (L) { j++; ver++; fp[0] += l[0] + l[1] + l[2] + l[3]; fp[4] += l[0] + l[1] - l[2] - l[3]; }
    if (R) { j++; ver++; fp[0] += r[0] + r[1] + r[2] + r[3]; fp[4] += r[0] + r[1] - r[2] - r[3]; }
    if (!hor && L && R) fp[1] = (l[0] + l[1] + l[2] + l[3] - r[0] - r[1] - r[2] - r[3]) >> (5 - sh);
    else if (hor) fp[1] >>= (3 - sh + hor);
    if (!ver && A && B) fp[4] = (a[0] + a[1] + a[2] + a[3] - b[0] - b[1] - b[2] - b[3]) >> (5 - sh);
    else if (ver) fp[4] >>= (3 - sh + ver);
    switch (j) {
    case 1: fp[0] >>= (4 - sh); break;
    case 2: fp[0] >>= (5 - sh); break;
    case 3: fp[0] = (21 * fp[0]) >> (10 - sh); break;      /* ~ *4/3 >> 6 */
    default: fp[0] >>= (6 - sh); break;
    }
    conceal_transform(fp);
    for (int y = 0; y < size; y++)
        for (int x = 0; x < size; x++)
            pl[(size_t)(y0 + y) * stride + x0 + x] = (u8)clip255(fp[4 * (y / g) + x / g]);
}

static void conceal_mb(const FjMbRec *r, Frame *f, u8 *const *slots, int wmb, int hmb, int mbx, int mby)
{
    if (r->kind == FJ_MB_CONCEAL_P) {
        Frame ref = frame_view(slots[r->ref_slot[0]], wmb, hmb);
        for (int y = 0; y < 16; y++)
            memcpy(f->y + (size_t)(mby * 16 + y) * f->w + mbx * 16, ref.y + (size_t)(mby * 16 + y) * f->w + mbx * 16, 16);
        for (int y = 0; y < 8; y++) {
            memcpy(f->cb + (size_t)(mby * 8 + y) * (f->w / 2) + mbx * 8, ref.cb + (size_t)(mby * 8 + y) * (f->w / 2) + mbx * 8, 8);
            memcpy(f->cr + (size_t)(mby * 8 + y) * (f->w / 2) + mbx * 8, ref.cr + (size_t)(mby * 8 + y) * (f->w / 2) + mbx * 8, 8);
        }
        return;
    }
    conceal_plane(f->y, f->w, mbx * 16, mby * 16, 16, r->avail);
    conceal_plane(f->cb, f->w / 2, mbx * 8, mby * 8, 8, r->avail);
    conceal_plane(f->cr, f->w / 2, mbx * 8, mby * 8, 8, r->avail);
}

int oracle_recon(const uint8_t *blob, uint8_t *const *slots)
{
    if (check_blob(blob)) return -1;
    const FjHeader *h = (const FjHeader *)blob;
    const FjMbRec *recs = (const FjMbRec *)(blob + h->rec_off);
    int16_t (*mvs)[16][2] = dense_mvs(blob);
    if (!mvs) return -1;
    const int16_t *coefs = (const int16_t *)(blob + h->coef_off);
    Frame f = frame_view(slots[h->cur_slot], h->width_mbs, h->height_mbs);
    int res_y[256], res_c[128];
    uint32_t n_conceal = 0;
    for (uint32_t a = 0; a < h->n_mbs; a++) {
        const FjMbRec *r = &recs[a];
        const int mbx = (int)(a % h->width_mbs), mby = (int)(a / h->width_mbs);
        if (r->kind == FJ_MB_ABSENT || r->kind == FJ_MB_STALE) continue;
        if (h->dbk_only && !(r->pred & FJ_PRED_PHASE2)) continue;     /* its pixels were made by the job before this one (FjHeader.dbk_only) */
        if (r->kind == FJ_MB_CONCEAL_I || r->kind == FJ_MB_CONCEAL_P) { n_conceal++; continue; }
        if (r->kind == FJ_MB_IPCM) {
            const u8 *s = (const u8 *)(coefs + 16 * (size_t)r->coef_idx);
            for (int y = 0; y < 16; y++) memcpy(f.y + (size_t)(mby * 16 + y) * f.w + mbx * 16, s + 16 * y, 16);
            for (int y = 0; y < 8; y++) {
                memcpy(f.cb + (size_t)(mby * 8 + y) * (f.w / 2) + mbx * 8, s + 256 + 8 * y, 8);
                memcpy(f.cr + (size_t)(mby * 8 + y) * (f.w / 2) + mbx * 8, s + 320 + 8 * y, 8);
            }
            continue;
        }
        mb_residual(r, coefs, res_y, res_c);
        if (r->kind == FJ_MB_INTER) {
            recon_inter(r, mvs[a], &f, slots, h->width_mbs, h->height_mbs, mbx, mby, res_y, res_c);
        } else {
            if (r->kind == FJ_MB_I4x4) recon_intra4x4(r, &f, mbx, mby, res_y);
            else recon_intra16x16(r, &f, mbx, mby, res_y);
            recon_intra_chroma(r, &f, mbx, mby, res_c);
        }
    }
    /* lost macroblocks, in the order the reference's concealment loop visits them (FjMbRec.coef_idx) */
    if (n_conceal) {
        uint32_t *ord = (uint32_t *)malloc(sizeof(uint32_t) * h->n_mbs);
        if (!ord) { free(mvs); return -1; }
        for (uint32_t i = 0; i < h->n_mbs; i++) ord[i] = 0xFFFFFFFFu;
        for (uint32_t a = 0; a < h->n_mbs; a++) {
            const FjMbRec *r = &recs[a];
            if (r->kind != FJ_MB_CONCEAL_I && r->kind != FJ_MB_CONCEAL_P) continue;
            if (h->dbk_only && !(r->pred & FJ_PRED_PHASE2)) continue;
            if (r->coef_idx >= h->n_mbs || ord[r->coef_idx] != 0xFFFFFFFFu) { free(ord); free(mvs); return -1; }
            ord[r->coef_idx] = a;
        }
        for (uint32_t i = 0; i < h->n_mbs; i++) {
            const uint32_t a = ord[i];
            if (a == 0xFFFFFFFFu) continue;
            conceal_mb(&recs[a], &f, slots, h->width_mbs, h->height_mbs, (int)(a % h->width_mbs), (int)(a / h->width_mbs));
        }
        free(ord);
    }
    free(mvs);
    return 0;
}

/* ------------------------------------------------------------------ deblocking, 8.7 */
static const u8 alpha_tab[52] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 4, 5, 6, 7, 8, 9, 10, 12, 13,
    15, 17, 20, 22, 25, 28, 32, 36, 40, 45, 50, 56, 63, 71, 80, 90, 101, 113, 127, 144, 162, 182, 203, 226, 255, 255 };
static const u8 beta_tab[52] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 6, 6,
    7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15, 16, 16, 17, 17, 18, 18 };
static const u8 tc0_tab[52][3] = {
    { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 },
    { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 1 },
    { 0, 0, 1 }, { 0, 0, 1 }, { 0, 0, 1 }, { 0, 1, 1 }, { 0, 1, 1 }, { 1, 1, 1 }, { 1, 1, 1 }, { 1, 1, 1 }, { 1, 1, 1 },
    { 1, 1, 2 }, { 1, 1, 2 }, { 1, 1, 2 }, { 1, 1, 2 }, { 1, 2, 3 }, { 1, 2, 3 }, { 2, 2, 3 }, { 2, 2, 4 }, { 2, 3, 4 },
    { 2, 3, 4 }, { 3, 3, 5 }, { 3, 4, 6 }, { 3, 4, 6 }, { 4, 5, 7 }, { 4, 5, 8 }, { 4, 6, 9 }, { 5, 7, 10 }, { 6, 8, 11 },
    { 6, 8, 13 }, { 7, 10, 14 }, { 8, 11, 16 }, { 9, 12, 18 }, { 10, 13, 20 }, { 11, 15, 23 }, { 13, 17, 25 } };
static const u8 qpc_tab[52] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23,
    24, 25, 26, 27, 28, 29, 29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39 };

static inline int is_intra_kind(int k)
{
    /* concealed macroblocks are filtered as Intra4x4 (reference conceal.c:309) */
    return k == FJ_MB_I4x4 || k == FJ_MB_I16x16 || k == FJ_MB_IPCM || k == FJ_MB_CONCEAL_I || k == FJ_MB_CONCEAL_P || k == FJ_MB_STALE;
}

/* ------------------------------------------------------------------ decision census (oracle_deblock_census)
 * Which of the filter's decisions a picture takes: bs_of() and filter_line() count into cn[] when it is given (NULL: nothing is
 * counted, the arithmetic is the same).  Filter classes are counted per line of samples, threshold classes per edge of a
 * macroblock, strength classes per 4-sample segment: S_* below, once for each of vertical macroblock edge, vertical inner
 * edge, horizontal macroblock edge, horizontal inner edge (CN_S + CN_S_N * (2 * dir + inner) + S_*).
 * Classes that cannot occur keep their slot and stay zero: strength 4 on an inner edge and strength 3 on a macroblock edge
 * (an intra side gives 4 exactly on macroblock edges), and "strength 0 by partition type" on a macroblock edge (the type
 * rules only inner edges); tests/test_structured_jobs.py leaves them off its list. */
#define CENSUS_FILTER(X) \
    X(L_CLOSED_ALPHA_ONLY) X(L_CLOSED_P1_ONLY) X(L_CLOSED_Q1_ONLY) \
    X(L_OPEN_AP0_AQ0) X(L_OPEN_AP1_AQ0) X(L_OPEN_AP0_AQ1) X(L_OPEN_AP1_AQ1) \
    X(L_D_CLIP_POS) X(L_D_CLIP_NEG) X(L_D_UNCLIPPED_NONZERO) X(L_D_ZERO) \
    X(L_P1Q1_CLIPPED) X(L_P1Q1_UNCLIPPED) X(L_OPEN_TC0_ZERO) X(L_SAT_0) X(L_SAT_255) \
    X(L4_WEAK) X(L4_STRONG_AP0_AQ0) X(L4_STRONG_AP1_AQ0) X(L4_STRONG_AP0_AQ1) X(L4_STRONG_AP1_AQ1) \
    X(C_D_CLIP_POS) X(C_D_CLIP_NEG) X(C_D_UNCLIPPED) X(C_SAT_0) X(C_SAT_255) X(C_BS4) \
    X(T_INDEXA_CLIP_0) X(T_INDEXA_CLIP_51) X(T_QP_SUM_ODD) X(T_MBEDGE_QP_AND_CQP_OFF_DIFFER) X(T_ALPHA_ZERO)
#define CENSUS_STRENGTH(X) \
    X(BS4) X(BS3) X(BS2) X(BS1_REF) X(BS1_DX_PLUS4_ONLY) X(BS1_DX_MINUS4_ONLY) X(BS1_DY_PLUS4_ONLY) X(BS1_DY_MINUS4_ONLY) \
    X(BS0_MAX_3) X(BS0_BY_TYPE_MV_4_OR_MORE)
#define X(n) CN_##n,
enum { CENSUS_FILTER(X) CN_S };
#undef X
#define X(n) S_##n,
enum { CENSUS_STRENGTH(X) CN_S_N };
#undef X
#define CN_TOTAL (CN_S + 4 * CN_S_N)
#define CNT(i) do { if (cn) cn[i]++; } while (0)

int oracle_census_classes(void) { return CN_TOTAL; }

/* name of class i ("" past the end); the returned string lives until the next call */
const char *oracle_census_name(int i)
{
#define X(n) #n,
    static const char *const filt[] = { CENSUS_FILTER(X) };
    static const char *const str[] = { CENSUS_STRENGTH(X) };
#undef X
    static const char *const where[4] = { "V_MB_", "V_INNER_", "H_MB_", "H_INNER_" };
    static char buf[64];
    if (i < 0 || i >= CN_TOTAL) return "";
    if (i < CN_S) return filt[i];
    strcpy(buf, where[(i - CN_S) / CN_S_N]);
    strcat(buf, str[(i - CN_S) % CN_S_N]);
    return buf;
}

/* boundary strength between the 4x4 block (qx,qy) of MB q and its left (dir 0) / upper (dir 1)
 * neighbour block, which lies in MB p (== q for inner edges) */
static int bs_of(const FjMbRec *q, const int16_t (*qmv)[2], const FjMbRec *p, const int16_t (*pmv)[2],
                 int qx, int qy, int px, int py, int mb_edge, uint64_t *cn)
{
    if (cn) cn += CN_S + CN_S_N * (2 * (qx == px) + !mb_edge);      /* the segment's group of strength classes */
    if (is_intra_kind(q->kind) || is_intra_kind(p->kind)) { CNT(mb_edge ? S_BS4 : S_BS3); return mb_edge ? 4 : 3; }
    if (((q->coded >> z_of(qx, qy)) & 1) || ((p->coded >> z_of(px, py)) & 1)) { CNT(S_BS2); return 2; }
    const int16_t *a = qmv[4 * qy + qx], *b = pmv[4 * py + px];
    const int dx = a[0] - b[0], dy = a[1] - b[1];
    if (!mb_edge) {
        /* inside a macroblock the reference compares motion only across the partition boundaries its TYPE has
         * (deblocking.c:1266-1345): none for 16x16 / P_Skip, the middle horizontal edge for 16x8, the middle vertical one
         * for 8x16.  The same thing as comparing everywhere unless the type and the vectors disagree, which happens
         * when a redundant decode changed the type and then failed before it wrote its vectors (FJ_PRED_PARTS) */
        const int parts = (q->pred >> FJ_PRED_PARTS_SHIFT) & 3, hor = qx == px, mid = hor ? qy == 2 : qx == 2;
        if (parts == FJ_PARTS_16x16 || (parts == FJ_PARTS_16x8 && !(hor && mid)) || (parts == FJ_PARTS_8x16 && !(!hor && mid))) {
            if (iabs(dx) >= 4 || iabs(dy) >= 4) CNT(S_BS0_BY_TYPE_MV_4_OR_MORE);
            return 0;
        }
    }
    if (q->ref_slot[(qy >> 1) * 2 + (qx >> 1)] != p->ref_slot[(py >> 1) * 2 + (px >> 1)]) { CNT(S_BS1_REF); return 1; }
    if (iabs(dx) >= 4 || iabs(dy) >= 4) {
        if (iabs(dx) == 4 && iabs(dy) < 4) CNT(dx > 0 ? S_BS1_DX_PLUS4_ONLY : S_BS1_DX_MINUS4_ONLY);
        if (iabs(dy) == 4 && iabs(dx) < 4) CNT(dy > 0 ? S_BS1_DY_PLUS4_ONLY : S_BS1_DY_MINUS4_ONLY);
        return 1;
    }
    if (iabs(dx) == 3 || iabs(dy) == 3) CNT(S_BS0_MAX_3);
    return 0;
}

/* filter one line of samples across an edge; pix points at q0, step = distance between samples */
static void filter_line(u8 *pix, ptrdiff_t step, int bs, int alpha, int beta, int tc0, int chroma, uint64_t *cn)
{
    int p0 = pix[-step], p1 = pix[-2 * step], q0 = pix[0], q1 = pix[step];
    const int ga = iabs(p0 - q0) < alpha, gp = iabs(p1 - p0) < beta, gq = iabs(q1 - q0) < beta;
    if (!(ga && gp && gq)) {
        if (cn && !chroma && bs < 4 && ga + gp + gq == 2) cn[!ga ? CN_L_CLOSED_ALPHA_ONLY : !gp ? CN_L_CLOSED_P1_ONLY : CN_L_CLOSED_Q1_ONLY]++;
        return;
    }
    if (chroma) {
        if (bs < 4) {
            int tc = tc0 + 1;
            const int raw = (((q0 - p0) * 4) + (p1 - q1) + 4) >> 3;
            int d = clip3(-tc, tc, raw);
            CNT(raw > tc ? CN_C_D_CLIP_POS : raw < -tc ? CN_C_D_CLIP_NEG : CN_C_D_UNCLIPPED);
            if (p0 + d < 0 || q0 - d < 0) CNT(CN_C_SAT_0);
            if (p0 + d > 255 || q0 - d > 255) CNT(CN_C_SAT_255);
            pix[-step] = (u8)clip255(p0 + d);
            pix[0] = (u8)clip255(q0 - d);
        } else {
            CNT(CN_C_BS4);
            pix[-step] = (u8)((2 * p1 + p0 + q1 + 2) >> 2);
            pix[0] = (u8)((2 * q1 + q0 + p1 + 2) >> 2);
        }
        return;
    }
    int p2 = pix[-3 * step], q2 = pix[2 * step];
    int ap = iabs(p2 - p0), aq = iabs(q2 - q0);
    if (bs < 4) {
        int tc = tc0 + (ap < beta) + (aq < beta);
        const int raw = (((q0 - p0) * 4) + (p1 - q1) + 4) >> 3;
        int d = clip3(-tc, tc, raw);
        const int rp = (p2 + ((p0 + q0 + 1) >> 1) - 2 * p1) >> 1, rq = (q2 + ((p0 + q0 + 1) >> 1) - 2 * q1) >> 1;
        if (cn) {
            cn[CN_L_OPEN_AP0_AQ0 + (ap < beta) + 2 * (aq < beta)]++;
            cn[raw > tc ? CN_L_D_CLIP_POS : raw < -tc ? CN_L_D_CLIP_NEG : raw ? CN_L_D_UNCLIPPED_NONZERO : CN_L_D_ZERO]++;
            if (ap < beta) cn[rp > tc0 || rp < -tc0 ? CN_L_P1Q1_CLIPPED : CN_L_P1Q1_UNCLIPPED]++;
            if (aq < beta) cn[rq > tc0 || rq < -tc0 ? CN_L_P1Q1_CLIPPED : CN_L_P1Q1_UNCLIPPED]++;
            if (tc0 == 0) cn[CN_L_OPEN_TC0_ZERO]++;
            if (p0 + d < 0 || q0 - d < 0) cn[CN_L_SAT_0]++;
            if (p0 + d > 255 || q0 - d > 255) cn[CN_L_SAT_255]++;
        }
        if (ap < beta) pix[-2 * step] = (u8)(p1 + clip3(-tc0, tc0, rp));
        if (aq < beta) pix[step] = (u8)(q1 + clip3(-tc0, tc0, rq));
        pix[-step] = (u8)clip255(p0 + d);
        pix[0] = (u8)clip255(q0 - d);
    } else {
        int p3 = pix[-4 * step], q3 = pix[3 * step];
        const int strong = iabs(p0 - q0) < ((alpha >> 2) + 2);
        CNT(strong ? CN_L4_STRONG_AP0_AQ0 + (ap < beta) + 2 * (aq < beta) : CN_L4_WEAK);
        if (strong && ap < beta) {
            pix[-step] = (u8)((p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3);
            pix[-2 * step] = (u8)((p2 + p1 + p0 + q0 + 2) >> 2);
            pix[-3 * step] = (u8)((2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3);
        } else pix[-step] = (u8)((2 * p1 + p0 + q1 + 2) >> 2);
        if (strong && aq < beta) {
            pix[0] = (u8)((p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3);
            pix[step] = (u8)((p0 + q0 + q1 + q2 + 2) >> 2);
            pix[2 * step] = (u8)((2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3);
        } else pix[0] = (u8)((2 * q1 + q0 + p1 + 2) >> 2);
    }
}

static int deblock_walk(const uint8_t *blob, uint8_t *frame, uint64_t *cn)
{
    if (check_blob(blob)) return -1;
    const FjHeader *h = (const FjHeader *)blob;
    const FjMbRec *recs = (const FjMbRec *)(blob + h->rec_off);
    int16_t (*mvs)[16][2] = dense_mvs(blob);
    if (!mvs) return -1;
    Frame f = frame_view(frame, h->width_mbs, h->height_mbs);
    const int W = f.w, CW = f.w / 2;
    for (uint32_t a = 0; a < h->n_mbs; a++) {
        const FjMbRec *q = &recs[a];
        if (q->kind == FJ_MB_ABSENT || !q->dbk) continue;
        const int mbx = (int)(a % h->width_mbs), mby = (int)(a / h->width_mbs);
        for (int dir = 0; dir < 2; dir++) {                 /* vertical edges first, then horizontal */
            for (int e = 0; e < 4; e++) {
                const int mb_edge = e == 0;
                if (mb_edge && !(q->dbk & (dir ? FJ_DBK_TOP : FJ_DBK_LEFT))) continue;
                if (!mb_edge && !(q->dbk & FJ_DBK_INNER)) continue;
                const uint32_t pa = mb_edge ? (dir ? a - h->width_mbs : a - 1) : a;
                const FjMbRec *p = &recs[pa];
                /* thresholds: average QP of the two macroblocks, offsets of the current one */
                const int qpl = (q->qp_y + p->qp_y + 1) >> 1;
                const int qcq = qpc_tab[clip3(0, 51, q->qp_y + q->cqp_off)];
                const int qcp = qpc_tab[clip3(0, 51, p->qp_y + q->cqp_off)];   /* current MB's offset: deblocking.c:1501,1523 */
                const int qpc = (qcq + qcp + 1) >> 1;
                const int ia_l = clip3(0, 51, qpl + q->alpha_off), ib_l = clip3(0, 51, qpl + q->beta_off);
                const int ia_c = clip3(0, 51, qpc + q->alpha_off), ib_c = clip3(0, 51, qpc + q->beta_off);
                if (cn) {
                    if (qpl + q->alpha_off < 0) cn[CN_T_INDEXA_CLIP_0]++;
                    if (qpl + q->alpha_off > 51) cn[CN_T_INDEXA_CLIP_51]++;
                    if ((q->qp_y + p->qp_y) & 1) cn[CN_T_QP_SUM_ODD]++;
                    if (mb_edge && q->qp_y != p->qp_y && q->cqp_off != p->cqp_off) cn[CN_T_MBEDGE_QP_AND_CQP_OFF_DIFFER]++;
                    if (alpha_tab[ia_l] == 0) cn[CN_T_ALPHA_ZERO]++;
                }
                for (int k = 0; k < 4; k++) {               /* four 4-sample segments along the edge */
                    const int qx = dir ? k : e, qy = dir ? e : k;
                    const int px = dir ? k : (mb_edge ? 3 : e - 1), py = dir ? (mb_edge ? 3 : e - 1) : k;
                    const int bs = bs_of(q, mvs[a], p, mvs[pa], qx, qy, px, py, mb_edge, cn);
                    if (!bs) continue;
                    const int tl = bs < 4 ? tc0_tab[ia_l][bs - 1] : 0;
                    for (int i = 0; i < 4; i++) {
                        u8 *pix = dir ? f.y + (size_t)(mby * 16 + 4 * e) * W + mbx * 16 + 4 * k + i
                                      : f.y + (size_t)(mby * 16 + 4 * k + i) * W + mbx * 16 + 4 * e;
                        filter_line(pix, dir ? W : 1, bs, alpha_tab[ia_l], beta_tab[ib_l], tl, 0, cn);
                    }
                    if (e & 1) continue;                    /* chroma has edges only at luma 0 and 8 */
                    const int tcc = bs < 4 ? tc0_tab[ia_c][bs - 1] : 0;
                    for (int pl = 0; pl < 2; pl++) {
                        u8 *P = pl ? f.cr : f.cb;
                        for (int i = 0; i < 2; i++) {
                            u8 *pix = dir ? P + (size_t)(mby * 8 + 2 * e) * CW + mbx * 8 + 2 * k + i
                                          : P + (size_t)(mby * 8 + 2 * k + i) * CW + mbx * 8 + 2 * e;
                            filter_line(pix, dir ? CW : 1, bs, alpha_tab[ia_c], beta_tab[ib_c], tcc, 1, cn);
                        }
                    }
                }
            }
        }
    }
    free(mvs);
    return 0;
}

int oracle_deblock(const uint8_t *blob, uint8_t *frame) { return deblock_walk(blob, frame, NULL); }

/* oracle_deblock() that also counts the decisions it takes: counts[oracle_census_classes()], added to (the caller zeroes them) */
int oracle_deblock_census(const uint8_t *blob, uint8_t *frame, uint64_t *counts) { return deblock_walk(blob, frame, counts); }

int oracle_decode_picture(const uint8_t *blob, uint8_t *const *slots)
{
    if (oracle_recon(blob, slots)) return -1;
    const FjHeader *h = (const FjHeader *)blob;
    return h->any_deblock ? oracle_deblock(blob, slots[h->cur_slot]) : 0;
}

/* ------------------------------------------------------------------ colour conversion */
/* fmt 0: RGBA bytes, 1: BGRA bytes ("ARGB" word), 2: YCbCrA bytes; width/height in samples */
void oracle_convert(int fmt, uint32_t width, uint32_t height, const uint8_t *data, uint32_t *out)
{
    const u8 *Y = data, *Cb = data + (size_t)width * height, *Cr = Cb + (size_t)(width / 2) * (height / 2);
    for (uint32_t y = 0; y < height; y++)
        for (uint32_t x = 0; x < width; x++) {
            const int yy = Y[(size_t)y * width + x];
            const int cb = Cb[(size_t)(y / 2) * (width / 2) + x / 2], cr = Cr[(size_t)(y / 2) * (width / 2) + x / 2];
            uint32_t v;
            if (fmt == 2) v = 0xFF000000u | ((uint32_t)cr << 16) | ((uint32_t)cb << 8) | (uint32_t)yy;
            else {
                const int c = yy - 16, d = cb - 128, e = cr - 128;
                const uint32_t r = (uint32_t)clip255((298 * c + 409 * e + 128) >> 8);
                const uint32_t g = (uint32_t)clip255((298 * c - 100 * d - 208 * e + 128) >> 8);
                const uint32_t b = (uint32_t)clip255((298 * c + 516 * d + 128) >> 8);
                v = fmt == 0 ? 0xFF000000u | (b << 16) | (g << 8) | r : 0xFF000000u | (r << 16) | (g << 8) | b;
            }
            out[(size_t)y * width + x] = v;
        }
}

/* Boundary strengths of a picture, for analysis tools: out[32 * mb + 16 * dir + 4 * e + k] (dir 0 = vertical edges),
 * 0 where the edge is not filtered at all (GetMbFilteringFlags). */
int oracle_strengths(const uint8_t *blob, uint8_t *out)
{
    if (check_blob(blob)) return -1;
    const FjHeader *h = (const FjHeader *)blob;
    const FjMbRec *recs = (const FjMbRec *)(blob + h->rec_off);
    int16_t (*mvs)[16][2] = dense_mvs(blob);
    if (!mvs) return -1;
    memset(out, 0, (size_t)h->n_mbs * 32u);
    for (uint32_t a = 0; a < h->n_mbs; a++) {
        const FjMbRec *q = &recs[a];
        if (q->kind == FJ_MB_ABSENT || !q->dbk) continue;
        for (int dir = 0; dir < 2; dir++)
            for (int e = 0; e < 4; e++) {
                const int mb_edge = e == 0;
                if (mb_edge && !(q->dbk & (dir ? FJ_DBK_TOP : FJ_DBK_LEFT))) continue;
                if (!mb_edge && !(q->dbk & FJ_DBK_INNER)) continue;
                const uint32_t pa = mb_edge ? (dir ? a - h->width_mbs : a - 1) : a;
                for (int k = 0; k < 4; k++) {
                    const int qx = dir ? k : e, qy = dir ? e : k;
                    const int px = dir ? k : (mb_edge ? 3 : e - 1), py = dir ? (mb_edge ? 3 : e - 1) : k;
                    out[32 * a + 16 * dir + 4 * e + k] = (uint8_t)bs_of(q, mvs[a], &recs[pa], mvs[pa], qx, qy, px, py, mb_edge, NULL);
                }
            }
    }
    free(mvs);
    return 0;
}
