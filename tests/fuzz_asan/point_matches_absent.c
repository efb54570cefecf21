/* The point matches on an engine that has no eng_sink_entries: tests/fuzz_asan/mock_engine.c as it stands.  api.c refers to the table of
 * entries weakly (engine.h), so this program links, the address is NULL, and h264bsdmiOutputPointMatches is refused with -1 before
 * anything is written, whatever the instances hold; the siblings on the same instances go on working.
 * tests/test_point_matches_host.py builds it, plain and under sanitizers.
 *       usage: point_matches_absent <test_640x360.h264> <test_1920x1080.h264> */
#include "host_harness.h"

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    u32 len_a = 0;
    u8 *sa = load(argv[1], &len_a);
    Inst A;
    make(&A, 0, sa, len_a, 100);
    Inst *const a[] = { &A };
    storage_t *dec[1]; void *users[1];
    const h264bsdmi_matches_spec spec = { (void *)(uintptr_t)0x1000, (void *)(uintptr_t)0x2000, (void *)(uintptr_t)0x3000, 64, 64, 205, 0, 1, 1, 1, 0 };
    const h264bsdmi_shift_spec sibling = { (void *)(uintptr_t)0x1000, 4, 0, 1, 0 };
    pop("A", &A);
    keep("keep_a", 1, a, 0, 0);
    for (int pass = 0; pass < 2; pass++) {
        u32 got[1] = { SENT }, arr[4][1] = { { SENT }, { SENT }, { SENT }, { SENT } };
        aim(1, a, dec, users, 0);
        const int rc = pass ? h264bsdmiOutputRegionShift(1, dec, 1, NULL, &sibling, NULL, got, arr[0], arr[1], arr[2], arr[3])
                            : h264bsdmiOutputPointMatches(1, dec, 1, NULL, &spec, NULL, got, arr[0], arr[1], arr[2], arr[3]);
        head(pass ? "sibling_goes_on" : "refused_engine_without_entry", rc);
        show("got", got, 1, 1);
        show("current", arr[0], 1, 1);
        show("kept", arr[1], 1, 1);
        show("picId", arr[2], 1, 1);
        show("keptPicId", arr[3], 1, 1);
    }
    unmake(&A);
    free(sa);
    return 0;
}
