// tests/lane_arith/lane_arith_host.cpp — the register arithmetic of the lane inter kernels (kernels/inter_lane_block.hip.h, included as it is), run
// on the CPU on cases that tests/test_inter_jobs.py writes and compares with tests/inter_model.py.  No HIP, nothing loaded into Python:
//   clang++ -O1 -g -std=c++20 [-fsanitize=address,undefined] tests/lane_arith/lane_arith_host.cpp -o lane_arith_host && lane_arith_host cases.txt results.txt
// One case per record of whitespace-separated integers, one result line per case, in order:
//   L fx fy  s[81]                      a 9x9 luma window, rows y - 2 .. y + 6 of columns x - 2 .. x + 6, and the quarter-sample fraction
//       -> L  p[16]                     the 4x4 block of lb_luma_whole / _hor / _ver / _diag / _centre (the class branch is the kernels')
//   C w00 w10 w01 w11  a[5] b[5]        a chroma row and the row below it, five samples each, and the four bilinear weights
//       -> C  p[4]                      lb_chroma_row
//   R qp_y qp_c has_dc i pk  c[4]  y[16] c[16]
//                                       a luma and a chroma level block (raster), the four chroma DC levels of the plane, the chroma block's place i
//                                       in it; has_dc: there is a DC block; pk: the packed transform is run too (the caller says so where the
//                                       parser's bound holds: elsewhere its 16-bit sums overflow, which is undefined for signed vector elements
//                                       and which no sanitizer reports — the caller's exact comparison is the check)
//       -> R dc over_y over_c  y32[16] c32[16] [ypk[16] cpk[16]]
//                                       lb_chroma_dc (0 without a DC block), lb_residual_32 of both blocks and its range verdicts, lb_residual_pk
#include "lane_shims.h"
#include "../../h264bsd_amd/csrc/kernels/inter_lane_block.hip.h"
using namespace h264k;

static FILE *in, *out;
static bool get(int &v) { return fscanf(in, "%d", &v) == 1; }
static int need() { int v; if (!get(v)) { fprintf(stderr, "short case file\n"); exit(2); } return v; }

static void luma_case()
{
    const int fx = need(), fy = need();
    uint8_t row[9][12];
    for (int r = 0; r < 9; r++) {
        for (int c = 0; c < 9; c++) row[r][c] = (uint8_t)need();
        for (int c = 9; c < 12; c++) row[r][c] = 0xA5;          // columns x + 7 .. x + 9 of the dwords: loaded, never part of a result
    }
    uint32_t rw[9][3];
    memcpy(rw, row, sizeof rw);
    s2 o[4][2];
    switch (lb_class_of(fx, fy)) {
    case 0: lb_luma_whole(rw, o); break;
    case 1: lb_luma_hor(rw, fx, o); break;
    case 2: lb_luma_ver(rw, fy, o); break;
    case 3: lb_luma_diag(rw, fx, fy, o); break;
    default: lb_luma_centre(rw, fx, fy, o); break;
    }
    fprintf(out, "L");
    for (int r = 0; r < 4; r++) fprintf(out, " %d %d %d %d", o[r][0].x, o[r][0].y, o[r][1].x, o[r][1].y);
    fprintf(out, "\n");
}

static void chroma_case()
{
    int w[4];
    for (int &v : w) v = need();
    uint8_t a[8] = { 0, 0, 0, 0, 0, 0xA5, 0xA5, 0xA5 }, b[8] = { 0, 0, 0, 0, 0, 0xA5, 0xA5, 0xA5 };
    for (int c = 0; c < 5; c++) a[c] = (uint8_t)need();
    for (int c = 0; c < 5; c++) b[c] = (uint8_t)need();
    uint32_t ad[2], bd[2];
    memcpy(ad, a, 8); memcpy(bd, b, 8);
    s2 o01, o23;
    lb_chroma_row(ad[0], ad[1], bd[0], bd[1], pk(w[0]), pk(w[1]), pk(w[2]), pk(w[3]), o01, o23);
    fprintf(out, "C %d %d %d %d\n", o01.x, o01.y, o23.x, o23.y);
}

static void residual_case()
{
    const int qp_y = need(), qp_c = need(), has_dc = need(), i = need(), run_pk = need();
    int16_t cdc[4], y[16], c[16];
    for (auto &v : cdc) v = (int16_t)need();
    for (auto &v : y) v = (int16_t)need();
    for (auto &v : c) v = (int16_t)need();
    uint32_t dcw[2], yl[8], cl[8];
    memcpy(dcw, cdc, 8); memcpy(yl, y, 32); memcpy(cl, c, 32);
    const int dc = has_dc ? lb_chroma_dc(dcw[0], dcw[1], i, qp_c) : 0;
    int ry[4][4], rc[4][4];
    const bool over_y = lb_residual_32(yl, qp_y, false, 0, ry), over_c = lb_residual_32(cl, qp_c, true, dc, rc);
    fprintf(out, "R %d %d %d", dc, (int)over_y, (int)over_c);
    for (int r = 0; r < 4; r++) for (int k = 0; k < 4; k++) fprintf(out, " %d", ry[r][k]);
    for (int r = 0; r < 4; r++) for (int k = 0; k < 4; k++) fprintf(out, " %d", rc[r][k]);
    if (run_pk) {
        uint32_t rr[4][4];
        lb_residual_pk(yl, cl, qp_y, qp_c, dc, rr);
        for (int r = 0; r < 4; r++) for (int k = 0; k < 4; k++) fprintf(out, " %d", (int)(int16_t)(rr[r][k] & 0xFFFFu));
        for (int r = 0; r < 4; r++) for (int k = 0; k < 4; k++) fprintf(out, " %d", (int)(int32_t)rr[r][k] >> 16);
    }
    fprintf(out, "\n");
}

int main(int argc, char **argv)
{
    if (argc != 3 || !(in = fopen(argv[1], "r")) || !(out = fopen(argv[2], "w"))) { fprintf(stderr, "usage: lane_arith_host cases results\n"); return 2; }
    char kind[8];
    long n = 0;
    while (fscanf(in, "%7s", kind) == 1) {
        if (kind[0] == 'L') luma_case();
        else if (kind[0] == 'C') chroma_case();
        else if (kind[0] == 'R') residual_case();
        else { fprintf(stderr, "case %ld: unknown kind %s\n", n, kind); return 2; }
        n++;
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("%ld cases\n", n);
    return 0;
}
