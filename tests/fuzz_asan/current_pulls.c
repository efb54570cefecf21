/* What the four pulls of CURRENT pictures (api.c: h264bsdmiOutputTensorRegions, ...Remap, ...MotionRegions, ...RegionStats) hand to the
 * engine and write back, without a GPU: bound to tests/fuzz_asan/mock_engine.c, whose entries record all they are given.  Reads one call
 * per line from stdin (the grid: tests/golden/make_current_pull_pins.py, which documents the line), prints per call "#i", rc, the
 * sink's record or "sink: not called", and the output arrays, which start as a sentinel; at the end what every instance's output queue
 * still gives.       usage: current_pulls <test_640x360.h264> <test_1920x1080_fullRange.h264> < cases
 * Instances: A, B popped once (motion export on); C fed to its first picture, nothing popped; D never fed; E popped, then decoded on;
 * F popped, then flushed; G capture mode; H as A without motion export; T as A, never named in a call (the untouched twin). */
#include "host_harness.h"

static const char LETTERS[] = "ABCDEFGHT";
static Inst g_inst[sizeof(LETTERS) - 1];

/* h264bsdDecode until it answers `want` (or the stream ends); every picture of an instance carries the one picId */
static void feed_until(Inst *t, u32 want)
{
    while (t->off < t->len) {
        u32 rb = 0;
        const u32 r = h264bsdDecode(t->s, t->buf + t->off, t->len - t->off, t->id, &rb);
        t->off += rb;
        if (r == want) return;
    }
    fprintf(stderr, "stream ended before status %u\n", want); exit(2);
}
static void make_lettered(Inst *t, char letter, const u8 *stream, u32 len)
{
    t->s = h264bsdAlloc();
    t->buf = malloc(len); memcpy(t->buf, stream, len); t->len = len; t->off = 0; t->id = 100u + (u32)(letter == 'T' ? 'A' : letter);
    if (letter == 'G') {
        if (h264bsdmiInitCapture(t->s, 0, no_job, NULL) != HANTRO_OK) exit(2);
        t->user = NULL;
    } else {
        if (h264bsdInit(t->s, 0) != HANTRO_OK) exit(2);
        t->user = mock_last_attached();
        if (letter != 'H' && h264bsdmiSetMotionExport(t->s, 1)) exit(2);
    }
    if (letter == 'D') return;
    feed_until(t, H264BSD_PIC_RDY);
    if (letter == 'C' || letter == 'G') return;
    if (h264bsdmiNextOutputInfo(t->s, NULL, NULL, NULL) < 0) exit(2);
    if (letter == 'E') { u32 rb = 0; h264bsdDecode(t->s, t->buf + t->off, t->len - t->off, t->id + 1, &rb); }
    if (letter == 'F') h264bsdFlushBuffer(t->s);
}

/* "a,b,c" -> out[]; returns how many */
static int nums(char *tok, double *out, int max)
{
    int k = 0;
    char *save = NULL;
    for (char *p = strtok_r(tok, ",", &save); p && k < max; p = strtok_r(NULL, ",", &save)) out[k++] = strtod(p, NULL);
    return k;
}
static u32 *sentinels(size_t n)
{
    u32 *p = malloc((n ? n : 1) * sizeof(u32));
    for (size_t i = 0; i < (n ? n : 1); i++) p[i] = SENT;
    return p;
}
/* as show(), over all of sentinels(n), and what was written shows though NULL was passed */
static void show_all(const char *name, const u32 *a, size_t n, int passed)
{
    int touched = 0;
    n = n ? n : 1;
    for (size_t i = 0; i < n; i++) touched |= a[i] != SENT;
    printf("%s=", name);
    if (!touched) printf(passed ? "untouched" : "null");
    else for (size_t i = 0; i < n; i++) { if (a[i] == SENT) printf("%sS", i ? "," : ""); else printf("%s%u", i ? "," : "", a[i]); }
    printf("\n");
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    u32 len_a = 0, len_b = 0;
    u8 *sa = load(argv[1], &len_a), *sb = load(argv[2], &len_b);
    for (size_t i = 0; LETTERS[i]; i++) make_lettered(&g_inst[i], LETTERS[i], LETTERS[i] == 'B' ? sb : sa, LETTERS[i] == 'B' ? len_b : len_a);
    static char line[1 << 16];
    for (int idx = 0; fgets(line, sizeof(line), stdin); idx++) {
        char *tok[9], *save = NULL;
        int nt = 0;
        for (char *p = strtok_r(line, " \n", &save); p && nt < 9; p = strtok_r(NULL, " \n", &save)) tok[nt++] = p;
        if (nt != 9) { fprintf(stderr, "case %d: %d fields\n", idx, nt); return 2; }
        const char entry = tok[0][0];
        const u32 n = (u32)strtoul(tok[1], NULL, 0), nr = (u32)strtoul(tok[3], NULL, 0), flags = (u32)strtoul(tok[8], NULL, 0);
        /* the instances: "0" NULL, "-" an empty array, else one letter each ('_': a NULL element) */
        storage_t *dec[16] = { 0 };
        void *users[16] = { 0 };
        const size_t nd = strcmp(tok[2], "0") && strcmp(tok[2], "-") ? strlen(tok[2]) : 0;
        for (size_t i = 0; i < nd && i < 16; i++) {
            const char *at = strchr(LETTERS, tok[2][i]);
            if (tok[2][i] != '_' && !at) { fprintf(stderr, "case %d: instance %c\n", idx, tok[2][i]); return 2; }
            if (at) { dec[i] = g_inst[at - LETTERS].s; users[i] = g_inst[at - LETTERS].user; }
        }
        /* the regions "i,x,y,w,h;..." or maps "i,address;...": "0" NULL, "-" an empty array */
        h264bsdmi_region regs[64];
        h264bsdmi_remap maps[64];
        u32 ni = 0;
        const int null_items = !strcmp(tok[4], "0");        /* (before the list is cut up in place) */
        if (strcmp(tok[4], "0") && strcmp(tok[4], "-")) {
            char *s2 = NULL;
            for (char *p = strtok_r(tok[4], ";", &s2); p && ni < 64; p = strtok_r(NULL, ";", &s2), ni++) {
                double v[5] = { 0 };
                nums(p, v, 5);
                regs[ni] = (h264bsdmi_region){ (u32)v[0], (int)v[1], (int)v[2], (u32)v[3], (u32)v[4] };
                maps[ni] = (h264bsdmi_remap){ (u32)v[0], (const void *)(uintptr_t)v[1] };
            }
        }
        double v[16] = { 0 };
        const int null_spec = !strcmp(tok[5], "0"), null_colour = !strcmp(tok[6], "0") || tok[6][0] == 'x', null_aux = !strcmp(tok[7], "0") || tok[7][0] == 'x';
        const int nv = null_spec ? 0 : nums(tok[5], v, 16);
        (void)nv;
        const h264bsdmi_tensor_spec ts = { (void *)(uintptr_t)v[0], (u32)v[1], (u32)v[2], (u32)v[3], (u32)v[4], (u32)v[5], (u32)v[6], (u32)v[7],
                                           { (float)v[8], (float)v[9], (float)v[10] }, { (float)v[11], (float)v[12], (float)v[13] } };
        const h264bsdmi_motion_spec ms = { (void *)(uintptr_t)v[0], (u32)v[1], (u32)v[2], (u32)v[3], (u32)v[4], (u32)v[5], (u32)v[6], (u32)v[7],
                                           (u32)v[8], (u32)v[9], (u32)v[10] };
        const h264bsdmi_stats_spec ss = { (void *)(uintptr_t)v[0], (u32)v[1], (u32)v[2], (u32)v[3] };
        double c[4] = { 0 }, x[5] = { 0 };
        if (!null_colour) nums(tok[6], c, 4);
        if (!null_aux) nums(tok[7], x, 5);
        const h264bsdmi_colour_spec cs = { (u32)c[0], (u32)c[1], (u32)c[2], (u32)c[3] };
        const h264bsdmi_resize_spec rs = { (u32)x[0], (u32)x[1], { (float)x[2], (float)x[3], (float)x[4] } };
        const h264bsdmi_remap_spec ps = { (u32)x[0], (u32)x[1], { (float)x[2], (float)x[3], (float)x[4] } };
        /* flags: 1 got, 2 box, 4 current, 8 picId are NULL; 16 the sink fails; 32 a stream is named */
        u32 *got = sentinels(nr), *box = sentinels(4 * (size_t)nr), *cur = sentinels(n), *ids = sentinels(n);
        u32 *pgot = flags & 1 ? NULL : got, *pbox = flags & 2 ? NULL : box, *pcur = flags & 4 ? NULL : cur, *pids = flags & 8 ? NULL : ids;
        void *stream = flags & 32 ? (void *)(uintptr_t)0x5000 : NULL;
        storage_t *const *pdec = !strcmp(tok[2], "0") ? NULL : dec;
        mock_fail = flags & 16 ? ~0u : 0;                /* every entry */
        mock_call(n < 16 ? n : 16, users);
        int rc = 99;
        if (entry == 'r') rc = h264bsdmiOutputTensorRegions(n, pdec, nr, null_items ? NULL : regs, null_spec ? NULL : &ts, null_colour ? NULL : &cs, null_aux ? NULL : &rs, stream, pgot, pbox, pcur, pids);
        else if (entry == 'm') rc = h264bsdmiOutputTensorRemap(n, pdec, nr, null_items ? NULL : maps, null_spec ? NULL : &ts, null_colour ? NULL : &cs, null_aux ? NULL : &ps, stream, pgot, pcur, pids);
        else if (entry == 'v') rc = h264bsdmiOutputMotionRegions(n, pdec, nr, null_items ? NULL : regs, null_spec ? NULL : &ms, stream, pgot, pbox, pcur, pids);
        else if (entry == 's') rc = h264bsdmiOutputRegionStats(n, pdec, nr, null_items ? NULL : regs, null_spec ? NULL : &ss, stream, pgot, pcur, pids);
        else { fprintf(stderr, "case %d: entry %c\n", idx, entry); return 2; }
        char name[16];
        snprintf(name, sizeof(name), "%d", idx);
        head(name, rc);
        show_all("got", got, nr, pgot != NULL);
        if (entry == 'r' || entry == 'v') show_all("box", box, 4 * (size_t)nr, pbox != NULL);
        show_all("current", cur, n, pcur != NULL);
        show_all("picId", ids, n, pids != NULL);
        free(got); free(box); free(cur); free(ids);
    }
    /* nothing was popped: what every instance's queue gives now, and A against its untouched twin */
    printf("#final\n");
    u32 first[4] = { 0 };
    for (size_t i = 0; LETTERS[i]; i++) {
        u32 id = SENT, idr = SENT, nerr = SENT;
        const int slot = h264bsdmiNextOutputInfo(g_inst[i].s, &id, &idr, &nerr);
        const u32 now[4] = { (u32)slot, id, idr, nerr };
        if (LETTERS[i] == 'A') memcpy(first, now, sizeof(now));
        if (LETTERS[i] == 'T') printf("twin=%d\n", memcmp(first, now, sizeof(now)) == 0);
        printf("%c next=%d,%u,%u,%u\n", LETTERS[i], slot, id, idr, nerr);
    }
    for (size_t i = 0; LETTERS[i]; i++) unmake(&g_inst[i]);
    free(sa); free(sb);
    return 0;
}
