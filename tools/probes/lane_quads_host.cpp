// tools/probes/lane_quads_host.cpp — the lane geometry of k_recon_inter_lq against plain H.264 arithmetic, on the CPU.
//   clang++ -O1 -g -std=c++20 -fsanitize=address,undefined tools/probes/lane_quads_host.cpp -o /tmp/lane_quads_host && /tmp/lane_quads_host
// It includes kernels/inter_lane_block.hip.h as it is (tests/lane_arith/lane_shims.h: the few device builtins it uses) and checks, for random pictures,
// macroblocks, quadrants and vectors (windows inside, across and outside the picture):
//   1. the quadrant window cut: the 13 x 32 window staged by the kernels' own rules (LqWin: which lane takes which piece, whether its tile is
//      needed, the clamped tile row lw_luma_piece / lw_chroma_piece, the spread lw_side, the place in the slot), lq_window_byte and the five
//      class filters give every lane the 4x4 block that 8.4.2.2.1 gives at that place;
//   2. the 2-lane chroma split: lq_chroma_byte and two lb_chroma_row per lane give the plane's 4x4 block of 8.4.2.2.2;
//   3. the store exchange: lq_pair_rows, lq_luma_store_offset, lq_chroma_store_offset fill the quadrant's part of the tile exactly once.
#include "../../tests/lane_arith/lane_shims.h"
#include "../../h264bsd_amd/csrc/kernels/inter_lane_block.hip.h"
using namespace h264k;

constexpr int QW_STRIDE = 32, QC_STRIDE = 16;                  // INTER_LQ_WSTRIDE, INTER_LQ_CSTRIDE
static int wmb, hmb, W, H;
static std::vector<uint8_t> frame;                           // macroblock tiles
static size_t luma_at(int x, int y) { return (size_t)((y >> 4) * wmb + (x >> 4)) * TILE + ((y & 15) << 4) + (x & 15); }
static size_t chroma_at(int plane, int x, int y) { return (size_t)((y >> 3) * wmb + (x >> 3)) * TILE + T_CB + (plane << 6) + ((y & 7) << 3) + (x & 7); }
static int Y(int x, int y) { return frame[luma_at(clip3(0, W - 1, x), clip3(0, H - 1, y))]; }
static int C(int p, int x, int y) { return frame[chroma_at(p, clip3(0, W / 2 - 1, x), clip3(0, H / 2 - 1, y))]; }
static int tap(int a, int b, int c, int d, int e, int f) { return a - 5 * b + 20 * c + 20 * d - 5 * e + f; }
// 8.4.2.2.1 at whole position (x, y), fraction (fx, fy)
static int luma_ref(int x, int y, int fx, int fy)
{
    auto b1 = [&](int xx, int yy) { return tap(Y(xx - 2, yy), Y(xx - 1, yy), Y(xx, yy), Y(xx + 1, yy), Y(xx + 2, yy), Y(xx + 3, yy)); };
    auto h1 = [&](int xx, int yy) { return tap(Y(xx, yy - 2), Y(xx, yy - 1), Y(xx, yy), Y(xx, yy + 1), Y(xx, yy + 2), Y(xx, yy + 3)); };
    auto r5 = [](int v) { return clip255((v + 16) >> 5); };
    const int G = Y(x, y), b = r5(b1(x, y)), h = r5(h1(x, y)), s = r5(b1(x, y + 1)), m = r5(h1(x + 1, y));
    const int j = clip255((tap(b1(x, y - 2), b1(x, y - 1), b1(x, y), b1(x, y + 1), b1(x, y + 2), b1(x, y + 3)) + 512) >> 10);
    auto av = [](int p, int q) { return (p + q + 1) >> 1; };
    switch (4 * fy + fx) {
    case 0: return G;               case 1: return av(G, b);        case 2: return b;           case 3: return av(b, Y(x + 1, y));
    case 4: return av(G, h);        case 5: return av(b, h);        case 6: return av(b, j);    case 7: return av(b, m);
    case 8: return h;               case 9: return av(h, j);        case 10: return j;          case 11: return av(j, m);
    case 12: return av(h, Y(x, y + 1)); case 13: return av(h, s);   case 14: return av(j, s);   default: return av(s, m);
    }
}
static int chroma_ref(int p, int x, int y, int fx, int fy)
{
    return ((8 - fx) * (8 - fy) * C(p, x, y) + fx * (8 - fy) * C(p, x + 1, y) + (8 - fx) * fy * C(p, x, y + 1) + fx * fy * C(p, x + 1, y + 1) + 32) >> 6;
}
static long n_luma, n_chroma, n_store, bad;
#define CHECK(c, ...) do { if (!(c)) { if (bad++ < 10) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void one_quadrant(int mbx, int mby, int q, int mvx, int mvy, uint8_t *tile_out, int *written)
{
    alignas(16) uint8_t lds[LqWin::bytes(QW_STRIDE, QC_STRIDE) + 16];
    memset(lds, 0xA5, sizeof lds);
    uint8_t *lw = lds, *lc = lds + LqWin::chroma_at(QW_STRIDE, QC_STRIDE, 0, 0, 0);
    const int CW = W >> 1, CH = H >> 1;
    const int xi = mbx * 16 + 8 * (q & 1) + (mvx >> 2) - 2, yi = mby * 16 + 8 * (q >> 1) + (mvy >> 2) - 2, xs = (xi >> 4) << 4;
    const int cxi = mbx * 8 + 4 * (q & 1) + (mvx >> 3), cyi = mby * 8 + 4 * (q >> 1) + (mvy >> 3), cxs = (cxi >> 3) << 3;
    // staging as the kernel's four lanes do it (lane_window_load / lane_window_store of k_recon_inter_lanes.hip.h, memcpy for the loads and stores):
    // lane j takes the pieces j, j + 4, ...; clamped tile row, spread where the tile is left or right of the picture
    int staged = 0;
    for (int j = 0; j < LqWin::LANES; j++) {
        for (int i = 0; i < LqWin::NL; i++) {
            const int p = j + LqWin::LANES * i, lr = LqWin::luma_row(p), lk = LqWin::luma_tile(p);
            if (!(LqWin::luma_piece(p) && LqWin::tile_needed(lk, xi - xs))) continue;
            uint8_t v[16];
            memcpy(v, &frame[lw_luma_piece(wmb, W, H, xs + 16 * lk, yi + lr)], 16);
            const int side = lw_side(xs + 16 * lk, W);
            if (side < 0) memset(v, v[0], 16); else if (side > 0) memset(v, v[15], 16);
            memcpy(lw + LqWin::luma_at(QW_STRIDE, lr, lk), v, 16);
            staged++;
        }
        for (int i = 0; i < LqWin::NC; i++) {
            const int p = j + LqWin::LANES * i, cp = LqWin::chroma_plane(p), cr = LqWin::chroma_row(p), ck = LqWin::chroma_tile(p);
            if (!LqWin::chroma_piece(p)) continue;
            uint8_t v[8];
            memcpy(v, &frame[lw_chroma_piece(wmb, cp, CW, CH, cxs + 8 * ck, cyi + cr)], 8);
            const int side = lw_side(cxs + 8 * ck, CW);
            if (side < 0) memset(v, v[0], 8); else if (side > 0) memset(v, v[7], 8);
            memcpy(lds + LqWin::chroma_at(QW_STRIDE, QC_STRIDE, cp, cr, ck), v, 8);
            staged++;
        }
    }
    CHECK(staged == (xi - xs >= 4 ? 26 : 13) + 20, "pieces staged: %d", staged);
    uint32_t ldw[4][4], cdw[4][2];
    for (int j = 0; j < 4; j++) {
        const int jbx = j & 1, jby = j >> 1, plane = j >> 1, half = j & 1;
        // ---- luma: the kernel's read (lb_luma_from_lds) ----
        const int o = lq_window_byte(q, mvx) + 4 * jbx, sh = 8 * (o & 3), fx = mvx & 3, fy = mvy & 3;
        CHECK(o == (xi - xs) + 4 * jbx, "window byte %d vs %d", o, (xi - xs) + 4 * jbx);
        const uint8_t *src = lw + 4 * jby * QW_STRIDE + (o & ~3);
        const int cls = lb_class_of(fx, fy);
        uint32_t rw[9][3] = {};
        auto row = [&](int r, int nd) {
            uint32_t d[4] = {};
            CHECK(src + r * QW_STRIDE + 4 * nd + 4 <= lds + 13 * QW_STRIDE, "luma read past the window");
            for (int k = 0; k <= nd; k++) memcpy(&d[k], src + r * QW_STRIDE + 4 * k, 4);
            for (int k = 0; k < 3; k++) rw[r][k] = k < nd ? (uint32_t)(((unsigned long long)d[k + 1] << 32 | d[k]) >> sh) : 0u;
        };
        s2 pl[4][2];
        if (cls == 0) { for (int r = 2; r < 6; r++) row(r, 2); lb_luma_whole(rw, pl); }
        else if (cls == 1) { for (int r = 2; r < 6; r++) row(r, 3); lb_luma_hor(rw, fx, pl); }
        else if (cls == 2) { for (int r = 0; r < 9; r++) row(r, 2); lb_luma_ver(rw, fy, pl); }
        else if (cls == 3) { for (int r = 0; r < 9; r++) row(r, (r >= 2 && r <= 6) ? 3 : 2); lb_luma_diag(rw, fx, fy, pl); }
        else { for (int r = 0; r < 9; r++) row(r, 3); lb_luma_centre(rw, fx, fy, pl); }
        for (int r = 0; r < 4; r++) {
            const int got[4] = { pl[r][0].x, pl[r][0].y, pl[r][1].x, pl[r][1].y };
            for (int c = 0; c < 4; c++) {
                const int x = mbx * 16 + 8 * (q & 1) + 4 * jbx + c + (mvx >> 2), y = mby * 16 + 8 * (q >> 1) + 4 * jby + r + (mvy >> 2);
                const int want = luma_ref(x, y, fx, fy);
                n_luma++;
                CHECK(got[c] == want, "luma mb (%d,%d) q %d mv (%d,%d) lane %d row %d col %d: %d want %d", mbx, mby, q, mvx, mvy, j, r, c, got[c], want);
            }
            ldw[j][r] = perm(as_u32(pl[r][1]), as_u32(pl[r][0]), 0x06040200u);
        }
        // ---- chroma: rows 2 * half, 2 * half + 1 of block q of the plane (lb_chroma_from_lds) ----
        const int ob = lq_chroma_byte(q, mvx), cfx = mvx & 7, cfy = mvy & 7;
        CHECK(ob == cxi - cxs, "chroma byte");
        const uint8_t *qb = lc + plane * 5 * QC_STRIDE + 2 * half * QC_STRIDE + (ob & ~3);
        uint32_t lo[3], hi[3];
        for (int t = 0; t < 3; t++) {
            uint32_t d[3];
            CHECK(qb + QC_STRIDE * t + 12 <= lc + (plane + 1) * 5 * QC_STRIDE, "chroma read past the plane's window");
            memcpy(d, qb + QC_STRIDE * t, 12);
            const uint64_t a = ((uint64_t)d[1] << 32) | d[0], b = ((uint64_t)d[2] << 32) | d[1];
            lo[t] = (uint32_t)(a >> (8 * (ob & 3))); hi[t] = (uint32_t)(b >> (8 * (ob & 3)));
        }
        const s2 w00 = as_s2((uint32_t)((8 - cfx) * (8 - cfy)) * 0x00010001u), w10 = as_s2((uint32_t)(cfx * (8 - cfy)) * 0x00010001u);
        const s2 w01 = as_s2((uint32_t)((8 - cfx) * cfy) * 0x00010001u), w11 = as_s2((uint32_t)(cfx * cfy) * 0x00010001u);
        s2 pc[2][2];
        lb_chroma_row(lo[0], hi[0], lo[1], hi[1], w00, w10, w01, w11, pc[0][0], pc[0][1]);
        lb_chroma_row(lo[1], hi[1], lo[2], hi[2], w00, w10, w01, w11, pc[1][0], pc[1][1]);
        for (int t = 0; t < 2; t++) {
            const int got[4] = { pc[t][0].x, pc[t][0].y, pc[t][1].x, pc[t][1].y };
            for (int c = 0; c < 4; c++) {
                const int want = chroma_ref(plane, mbx * 8 + 4 * (q & 1) + c + (mvx >> 3), mby * 8 + 4 * (q >> 1) + 2 * half + t + (mvy >> 3), cfx, cfy);
                n_chroma++;
                CHECK(got[c] == want, "chroma mb (%d,%d) q %d mv (%d,%d) lane %d row %d col %d: %d want %d", mbx, mby, q, mvx, mvy, j, t, c, got[c], want);
            }
            cdw[j][t] = perm(as_u32(pc[t][1]), as_u32(pc[t][0]), 0x06040200u);
        }
    }
    // ---- store exchange between lanes j, j ^ 1, then the stores ----
    for (int j = 0; j < 4; j++) {
        const int jbx = j & 1, o = j ^ 1;
        const uint32_t got0 = (o & 1) ? ldw[o][0] : ldw[o][2], got1 = (o & 1) ? ldw[o][1] : ldw[o][3];     // what lane o sends
        uint32_t r0[2], r1[2];
        lq_pair_rows(ldw[j], got0, got1, jbx, r0, r1);
        const int lo = lq_luma_store_offset(q, j), co = lq_chroma_store_offset(q, j);
        memcpy(tile_out + lo, r0, 8); memcpy(tile_out + lo + 16, r1, 8);
        memcpy(tile_out + co, &cdw[j][0], 4); memcpy(tile_out + co + 8, &cdw[j][1], 4);
        for (int k = 0; k < 8; k++) { written[lo + k]++; written[lo + 16 + k]++; }
        for (int k = 0; k < 4; k++) { written[co + k]++; written[co + 8 + k]++; }
    }
}

int main()
{
    srand(12345);
    static const int sizes[][2] = { { 1, 1 }, { 3, 2 }, { 5, 4 }, { 11, 6 } };
    for (int content = 0; content < 3; content++)
        for (auto &sz : sizes) {
            wmb = sz[0]; hmb = sz[1]; W = 16 * wmb; H = 16 * hmb;
            frame.assign((size_t)wmb * hmb * TILE, 0);
            for (auto &b : frame) b = content == 0 ? (uint8_t)rand() : content == 1 ? ((rand() & 1) ? 255 : 0) : (uint8_t)(128 + rand() % 5);
            for (int it = 0; it < 4000; it++) {
                const int mbx = rand() % wmb, mby = rand() % hmb;
                uint8_t tile[TILE];
                int written[TILE] = {};
                int mv[4][2];
                for (int q = 0; q < 4; q++) {
                    const int reach = (it % 3 == 0) ? 8 : (it % 3 == 1) ? 4 * W + 64 : 64;
                    mv[q][0] = rand() % (2 * reach + 1) - reach; mv[q][1] = rand() % (2 * reach + 1) - reach;
                    if (it % 5 == 0) { mv[q][0] = (mv[q][0] & ~3) | (it / 5 & 3); mv[q][1] = (mv[q][1] & ~3) | (it / 20 & 3); }
                    one_quadrant(mbx, mby, q, mv[q][0], mv[q][1], tile, written);
                }
                for (int k = 0; k < TILE; k++) { n_store++; CHECK(written[k] == 1, "tile byte %d written %d times", k, written[k]); }
                for (int y = 0; y < 16; y++)
                    for (int x = 0; x < 16; x++) {
                        const int q = (y >> 3) * 2 + (x >> 3);
                        const int want = luma_ref(mbx * 16 + x + (mv[q][0] >> 2), mby * 16 + y + (mv[q][1] >> 2), mv[q][0] & 3, mv[q][1] & 3);
                        CHECK(tile[y * 16 + x] == want, "stored luma (%d,%d): %d want %d", x, y, tile[y * 16 + x], want);
                    }
                for (int p = 0; p < 2; p++)
                    for (int y = 0; y < 8; y++)
                        for (int x = 0; x < 8; x++) {
                            const int q = (y >> 2) * 2 + (x >> 2);
                            const int want = chroma_ref(p, mbx * 8 + x + (mv[q][0] >> 3), mby * 8 + y + (mv[q][1] >> 3), mv[q][0] & 7, mv[q][1] & 7);
                            CHECK(tile[T_CB + 64 * p + y * 8 + x] == want, "stored chroma plane %d (%d,%d): %d want %d", p, x, y, tile[T_CB + 64 * p + y * 8 + x], want);
                        }
            }
        }
    // the coded mask of a quadrant: the bits of its four luma blocks (H.264 block order), its chroma block per plane, the chroma DC
    for (uint32_t q = 0; q < 4; q++) {
        uint32_t want = 1u << 25;
        for (int j = 0; j < 4; j++) want |= 1u << (4 * q + j);
        want |= (1u << (16 + q)) | (1u << (20 + q));
        CHECK(lq_coded_mask(q) == want, "coded mask of quadrant %u", q);
    }
    printf("luma samples %ld, chroma samples %ld, tile bytes %ld: %ld mismatches\n", n_luma, n_chroma, n_store, bad);
    return bad != 0;
}
