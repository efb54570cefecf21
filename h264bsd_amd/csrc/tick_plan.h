/* tick_plan.h — how the two per-picture kernels of a tick (k_frame_dbk, k_frame_intra) split its pictures into row bands: the shape of a tick, the
 * configuration, the plan of one launch (engine.hip, launch_tick).  No HIP in here: a host compiler builds it, tests/test_tick_plan.py pins the plan. */
#ifndef H264BSD_AMD_TICK_PLAN_H
#define H264BSD_AMD_TICK_PLAN_H
#include <algorithm>
#include <cstddef>
#include <cstdint>

/* ---- how the two per-picture kernels split a picture (row bands, kernels.hip.h) ----
 * rows per band for light / heavy pictures (heavy = more than a quarter of the macroblocks intra coded), wavefronts per
 * workgroup, and a cap on the bands of one launch.  H264BSDMI_TAIL="dbk_rows_light,dbk_rows_heavy,dbk_waves,intra_rows_light,
 * intra_rows_heavy,intra_waves" overrides the defaults (0 rows = one band); h264bsdmiDebugSetTail() does the same for tests. */
struct TailConfig {
    uint32_t dbk_rows_light = 17, dbk_rows_heavy = 9, dbk_waves = 12;
    uint32_t dbk_chroma_waves = 0;        /* wavefronts of a k_frame_dbk workgroup that start on the chroma graph; 0 = five twelfths */
    uint32_t intra_rows_light = 0, intra_rows_heavy = 9, intra_waves = 12;
    /* A picture is only split where that puts idle compute units to work: a launch gets at most band_budget workgroups
     * (bands per picture <= band_budget / pictures of the tick, at least 1).  256 pictures in lock-step: one workgroup per
     * picture and compute unit (measured: 4 bands x 4 wavefronts 92 instead of 57 ms per step in k_frame_dbk — a picture's
     * filtering needs about one compute unit's worth of instruction issue whichever way it is cut); the small ticks of
     * stream groups and heavy lanes: several workgroups per picture.  H264BSDMI_BAND_BUDGET overrides. */
    uint32_t band_budget = 320;
    /* ... and the heavy pictures of a tick that has the device to itself share heavy_budget further workgroups: the compute
     * units the tick's light pictures leave idle long before its heavy ones are done (H264BSDMI_HEAVY_BUDGET) */
    uint32_t heavy_budget = 64;
    bool from_env = false;
};

struct TickShape {
    uint32_t n_frames = 0, max_mbs = 0;
    uint32_t max_copy = 0, max_gen = 0, max_gen_uni = 0, max_gen_quad = 0, max_gen_rest = 0, max_dbk = 0, max_levels = 0, max_w = 0, max_h = 0;
    bool any_tail = false, any_deblock = false;
    uint32_t dbk_waves = 0;          /* wavefronts per workgroup of k_frame_dbk; 0 = the configured default (launch_tick) */
    /* row bands of the two per-picture kernels: most bands a light / a heavy picture of the tick wants, for k_frame_dbk [0]
     * and k_frame_intra [1]; number of heavy pictures (more than a quarter of the macroblocks intra coded) */
    uint32_t want_light[2] = { 1, 1 }, want_heavy[2] = { 1, 1 }, n_heavy = 0;
    /* a picture of the tick whose intra schedule may wait for macroblocks BELOW (concealment, FjHeader.intra_down_deps) must
     * stay in ONE band of k_frame_intra: the launch's rows-per-band cap (which the kernel applies to every picture) must
     * then cover a whole picture, whatever the other pictures of the tick want */
    bool intra_whole = false;
    uint32_t load = 0;               /* pictures the device works on at the same time as this tick (other lanes' ticks included): the
                                        band budget is shared between them; 0 = this tick only */
    /* hosted colour conversion (FrameDesc.conv_*): descriptors of this tick name a finished picture to convert */
    bool conv = false;
    uint32_t conv_waves = 0;         /* wavefronts of a k_frame_dbk workgroup that convert before they filter; 0 = CONV_WAVES_N */
};

/* The two per-picture kernels keep per-macroblock scheduling state in LDS next to their wavefronts' tiles: for
 * pictures that leave less than 16 wavefronts' worth of tile space in the 160 KB of a CU, fewer wavefronts run. */
constexpr size_t TAIL_LDS_BUDGET = 160 * 1024 - 512;
/* one launch: workgroups per picture, the rows-per-band cap the kernel applies to every picture, wavefronts, dynamic LDS; light_cap as the kernel takes it */
struct BandPlan { uint32_t bands, rows, waves; size_t lds; uint32_t light_cap; };

/* Row bands of the per-picture kernels (kernels.hip.h).  A picture is split only where that puts IDLE compute units to
 * work — measured: with 256 pictures on 256 compute units every split loses (a picture's work is about one compute unit's
 * worth of instruction issue however it is cut: 4 bands x 4 wavefronts 92 instead of 57 ms per step in k_frame_dbk, bands on
 * the heavy lanes of a saturated desynchronised schedule 775 instead of 827 M MB/s); with few pictures on the device it wins
 * (4-32 streams: +18-20 %), and so it does for the few heavy pictures of a tick that is otherwise done long before them.
 *   light_cap: bands a light picture may use = band_budget / pictures on the device (this tick, or all lanes' ticks: load)
 *   heavy_cap: when the tick is (nearly) alone on the device, its heavy pictures share what the budget leaves
 * which: 0 k_frame_dbk, 1 k_frame_intra; waves: the wavefronts asked for; lds_bytes(waves, width in macroblocks, rows): the kernel's LDS need;
 * may_shorten: bands may get shorter than asked for to fit the LDS (never for k_frame_intra).  -1: the picture does not fit with one wavefront. */
inline int plan_bands(const TickShape &s, const TailConfig &tc, int which, uint32_t waves, size_t (*lds_bytes)(uint32_t, uint32_t, uint32_t),
                      bool may_shorten, BandPlan &bp)
{
    const uint32_t on_device = std::max<uint32_t>(1u, std::max(s.n_frames, s.load));
    const uint32_t light_cap = std::max<uint32_t>(1u, tc.band_budget / on_device);
    uint32_t heavy_cap = light_cap;
    if (s.n_heavy && 2u * s.n_frames >= s.load) heavy_cap = std::max(light_cap, 1u + tc.heavy_budget / s.n_heavy);
    const uint32_t eff_l = std::min(s.want_light[which], light_cap), eff_h = std::min(s.want_heavy[which], heavy_cap);
    /* rows a band can have: the picture with the fewest bands decides (all pictures of a tick have the tick's size in
     * practice; max_h / fewest bands is the bound) */
    uint32_t fewest = s.n_heavy >= s.n_frames ? eff_h : s.n_heavy ? std::min(eff_l, eff_h) : eff_l;
    /* (band_split() clamps a picture's rows per band to this cap: a picture that wants ONE band gets it only if the cap is
     * the picture's height — for k_frame_intra that is a matter of correctness, see TickShape::intra_whole) */
    if (which == 1 && s.intra_whole) fewest = 1;
    uint32_t rows = (s.max_h + fewest - 1) / std::max<uint32_t>(1u, fewest);
    rows = std::max<uint32_t>(1u, std::min<uint32_t>(rows, s.max_h));
    while (may_shorten && lds_bytes(waves, s.max_w, rows) > TAIL_LDS_BUDGET && rows > 1) rows = (rows + 1) / 2;      /* (rows is a cap the kernel applies to every picture) */
    while (lds_bytes(waves, s.max_w, rows) > TAIL_LDS_BUDGET && waves > 1) waves--;
    if (lds_bytes(waves, s.max_w, rows) > TAIL_LDS_BUDGET) return -1;
    bp.rows = rows; bp.waves = waves; bp.lds = lds_bytes(waves, s.max_w, rows);
    bp.bands = std::max<uint32_t>(std::max(s.n_heavy < s.n_frames ? eff_l : 1u, s.n_heavy ? eff_h : 1u), (s.max_h + rows - 1) / rows);
    bp.light_cap = light_cap;
    return 0;
}
#endif
