#!/usr/bin/env python3
"""The pins of the band plan of the two per-picture kernels (h264bsd_amd/csrc/tick_plan.h, plan_bands): bands, rows per band,
wavefronts and LDS bytes of a launch, or the refusal, over a grid of tick shapes.  tests/test_tick_plan.py holds tick_plan.h to
tick_plan_pins.json; this file is the generator and holds the one grid and the one driver program both use.

The pins do NOT come from plan_bands.  They come from the plan as launch_tick carried it before it became a function of its own: a
lambda that captured the tick's shape, the configuration and the two caps.  OLD_PLAN below is that code, statement for statement
(structs, the caps, the lambda), and the generator compiles the driver against it:

    python3 tests/golden/make_tick_plan_pins.py            # writes tests/golden/tick_plan_pins.json

The LDS need is synthetic — waves * 7680 + 5 * (rows + 1) * wmb + 4096 bytes — so that the plan is pinned without the kernels: at
120 x 68 macroblocks twelve wavefronts fit, at 256 x 135 k_frame_dbk shortens its bands, k_frame_intra sheds wavefronts, and a
picture that must stay whole does not fit at all."""
import itertools
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
PINS = os.path.join(HERE, "tick_plan_pins.json")
WAVES = 12                      # asked of both kernels (TailConfig's default)


def cases():
    """(which, n_frames, load, n_heavy, want_light, want_heavy, max_w, max_h, intra_whole, band_budget), each combination once;
    which: 0 k_frame_dbk (bands may get shorter to fit the LDS), 1 k_frame_intra (never)"""
    seen, out = set(), []
    for n in (1, 4, 32, 256):
        for load, heavy, wl, wh, (w, h), whole, budget, which in itertools.product(
                (0, n, 256), (0, 1, n), (1, 4, 8), (1, 4, 8), ((11, 9), (120, 68), (256, 135)), (0, 1), (320, 64), (0, 1)):
            c = (which, n, load, heavy, wl, wh, w, h, whole, budget)
            if c not in seen:
                seen.add(c)
                out.append(c)
    return out


# reads the cases from stdin, one per line; prints "rc bands rows waves lds" for each.  PLAN_IMPL: a file that defines TickShape,
# TailConfig, BandPlan and run_plan(shape, config, which, waves, lds_bytes, may_shorten, plan).
DRIVER = r"""
#include <cstdio>
#include PLAN_IMPL
static size_t lds_need(uint32_t waves, uint32_t wmb, uint32_t rows) { return (size_t)waves * 7680 + 5 * (size_t)(rows + 1) * wmb + 4096; }
int main()
{
    unsigned which, n, load, heavy, wl, wh, w, h, whole, budget;
    while (scanf("%u %u %u %u %u %u %u %u %u %u", &which, &n, &load, &heavy, &wl, &wh, &w, &h, &whole, &budget) == 10) {
        TickShape s;
        s.n_frames = n; s.load = load; s.n_heavy = heavy;
        s.want_light[0] = s.want_light[1] = wl; s.want_heavy[0] = s.want_heavy[1] = wh;
        s.max_w = w; s.max_h = h; s.intra_whole = whole != 0;
        TailConfig tc;
        tc.band_budget = budget;
        BandPlan bp = {};
        const int rc = run_plan(s, tc, (int)which, WAVES, lds_need, which == 0, bp);
        if (rc) printf("%d 0 0 0 0\n", rc);
        else printf("0 %u %u %u %zu\n", bp.bands, bp.rows, bp.waves, bp.lds);
    }
    return 0;
}
"""

OLD_PLAN = r"""
#include <algorithm>
#include <cstddef>
#include <cstdint>
struct TailConfig {
    uint32_t dbk_rows_light = 17, dbk_rows_heavy = 9, dbk_waves = 12;
    uint32_t dbk_chroma_waves = 0;
    uint32_t intra_rows_light = 0, intra_rows_heavy = 9, intra_waves = 12;
    uint32_t band_budget = 320;
    uint32_t heavy_budget = 64;
    bool from_env = false;
};
struct TickShape {
    uint32_t n_frames = 0, max_mbs = 0;
    uint32_t max_copy = 0, max_gen = 0, max_gen_uni = 0, max_gen_quad = 0, max_gen_rest = 0, max_dbk = 0, max_levels = 0, max_w = 0, max_h = 0;
    bool any_tail = false, any_deblock = false;
    uint32_t dbk_waves = 0;
    uint32_t want_light[2] = { 1, 1 }, want_heavy[2] = { 1, 1 }, n_heavy = 0;
    bool intra_whole = false;
    uint32_t load = 0;
    bool conv = false;
    uint32_t conv_waves = 0;
};
struct BandPlan { uint32_t bands, rows, waves; size_t lds; };
static int run_plan(const TickShape &s, const TailConfig &tc, int which_, uint32_t waves_, size_t (*lds_bytes_)(uint32_t, uint32_t, uint32_t),
                    bool may_shorten_, BandPlan &bp_)
{
    constexpr size_t LDS_BUDGET = 160 * 1024 - 512;
    const uint32_t on_device = std::max<uint32_t>(1u, std::max(s.n_frames, s.load));
    const uint32_t light_cap = std::max<uint32_t>(1u, tc.band_budget / on_device);
    uint32_t heavy_cap = light_cap;
    if (s.n_heavy && 2u * s.n_frames >= s.load) heavy_cap = std::max(light_cap, 1u + tc.heavy_budget / s.n_heavy);
    auto plan = [&](int which, uint32_t waves, size_t (*lds_bytes)(uint32_t, uint32_t, uint32_t), bool may_shorten, BandPlan &bp) -> int {
        const uint32_t eff_l = std::min(s.want_light[which], light_cap), eff_h = std::min(s.want_heavy[which], heavy_cap);
        /* rows a band can have: the picture with the fewest bands decides (all pictures of a tick have the tick's size in
         * practice; max_h / fewest bands is the bound) */
        uint32_t fewest = s.n_heavy >= s.n_frames ? eff_h : s.n_heavy ? std::min(eff_l, eff_h) : eff_l;
        /* (band_split() clamps a picture's rows per band to this cap: a picture that wants ONE band gets it only if the cap is
         * the picture's height — for k_frame_intra that is a matter of correctness, see TickShape::intra_whole) */
        if (which == 1 && s.intra_whole) fewest = 1;
        uint32_t rows = (s.max_h + fewest - 1) / std::max<uint32_t>(1u, fewest);
        rows = std::max<uint32_t>(1u, std::min<uint32_t>(rows, s.max_h));
        while (may_shorten && lds_bytes(waves, s.max_w, rows) > LDS_BUDGET && rows > 1) rows = (rows + 1) / 2;      /* (rows is a cap the kernel applies to every picture) */
        while (lds_bytes(waves, s.max_w, rows) > LDS_BUDGET && waves > 1) waves--;
        if (lds_bytes(waves, s.max_w, rows) > LDS_BUDGET) return -1;
        bp.rows = rows; bp.waves = waves; bp.lds = lds_bytes(waves, s.max_w, rows);
        bp.bands = std::max<uint32_t>(std::max(s.n_heavy < s.n_frames ? eff_l : 1u, s.n_heavy ? eff_h : 1u), (s.max_h + rows - 1) / rows);
        return 0;
    };
    return plan(which_, waves_, lds_bytes_, may_shorten_, bp_);
}
"""


def run_driver(impl_text, workdir, include_dirs=()):
    """compiles DRIVER against impl_text with g++ and runs it over cases(): one [bands, rows, waves, lds] or None (refused) per case"""
    impl, src, exe = (os.path.join(workdir, n) for n in ("plan_impl.h", "driver.cpp", "driver"))
    open(impl, "w").write(impl_text)
    open(src, "w").write(DRIVER)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f'-DPLAN_IMPL="{impl}"', f"-DWAVES={WAVES}"]
    subprocess.run(cmd + [f"-I{d}" for d in include_dirs] + [src, "-o", exe], check=True)
    text = "".join(" ".join(map(str, c)) + "\n" for c in cases())
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    rows = [[int(v) for v in line.split()] for line in out if line]
    assert len(rows) == len(cases())
    return [None if r[0] else r[1:] for r in rows]


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        pins = run_driver(OLD_PLAN, tmp)
    with open(PINS, "w") as f:
        json.dump({"columns": ["bands", "rows", "waves", "lds"], "waves_asked": WAVES, "cases": len(pins), "plans": pins}, f,
                  separators=(",", ":"))
        f.write("\n")
    print(f"{PINS}: {len(pins)} cases, {sum(p is None for p in pins)} refused", file=sys.stderr)
