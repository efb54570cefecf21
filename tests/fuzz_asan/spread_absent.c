/* The background spread on an engine that has no eng_sink_entries: tests/fuzz_asan/mock_engine.c as it stands, which knows every entry
 * of the sink and was written before the table.  api.c refers to the table weakly (engine.h), so this program links, the address is
 * NULL, and h264bsdmiBlendCurrentPicturesSpread, h264bsdmiOutputKeptSpread and the SPREAD mode of the cell maps and cell boxes are
 * refused with -1 before anything is written, whatever the instances hold; the siblings on the same instance go on working.
 * tests/test_spread_host.py builds it, plain and under sanitizers.
 *       usage: spread_absent <test_640x360.h264> <test_1920x1080.h264> */
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
    const h264bsdmi_blend_spec blend = { 3, 12, 3, NULL };
    const h264bsdmi_spread_spec spread = { 2, 2, 255, H264BSDMI_SPREAD_ALL };
    h264bsdmi_cells_spec cells = { (void *)(uintptr_t)0x1000, 40, 23, 16, H264BSDMI_STATS_Y, 1, H264BSDMI_CELLS_SPREAD, H264BSDMI_CELL_FORE, { 4, 0, 0 }, 0 };
    const h264bsdmi_boxes_spec boxes = { (void *)(uintptr_t)0x2000, 16, H264BSDMI_CELL_FORE, 0, H264BSDMI_BOXES_ABOVE, 0, 8, 1 };
    void *const buf[1] = { (void *)(uintptr_t)0x10000 };
    pop("A", &A);
    keep("keep_a", 1, a, 0, 0);
    {
        u32 kept[1] = { SENT }, blended[1] = { SENT }, ids[1] = { SENT };
        aim(1, a, dec, users, 0);
        head("blend_refused_engine_without_entry", h264bsdmiBlendCurrentPicturesSpread(1, dec, &blend, &spread, NULL, kept, blended, ids));
        show("kept", kept, 1, 1); show("blended", blended, 1, 1); show("picId", ids, 1, 1);
        aim(1, a, dec, users, 0);
        head("out_refused_engine_without_entry", h264bsdmiOutputKeptSpread(1, dec, buf, NULL, kept, ids));
        show("got", kept, 1, 1); show("keptPicId", ids, 1, 1);
    }
    for (int pass = 0; pass < 3; pass++) {
        static const char *const names[] = { "cells_refused_engine_without_entry", "boxes_refused_engine_without_entry", "sibling_goes_on" };
        u32 got[1] = { SENT }, arr[4][1] = { { SENT }, { SENT }, { SENT }, { SENT } };
        if (pass == 2) { cells.mode = H264BSDMI_CELLS_CHANGE; cells.planes = H264BSDMI_CELL_ABOVE; }
        aim(1, a, dec, users, 0);
        const int rc = pass == 1 ? h264bsdmiOutputCellBoxes(1, dec, 1, NULL, &cells, &boxes, NULL, got, arr[0], arr[1], arr[2], arr[3])
                                 : h264bsdmiOutputCellMaps(1, dec, 1, NULL, &cells, NULL, got, arr[0], arr[1], arr[2], arr[3]);
        head(names[pass], rc);
        show("got", got, 1, 1); show("current", arr[0], 1, 1); show("kept", arr[1], 1, 1); show("picId", arr[2], 1, 1); show("keptPicId", arr[3], 1, 1);
    }
    {
        u32 kept[1] = { SENT }, blended[1] = { SENT }, ids[1] = { SENT };
        aim(1, a, dec, users, 0);
        head("plain_blend_goes_on", h264bsdmiBlendCurrentPictures(1, dec, &blend, NULL, kept, blended, ids));
        show("kept", kept, 1, 1); show("blended", blended, 1, 1); show("picId", ids, 1, 1);
    }
    unmake(&A);
    free(sa);
    return 0;
}
