"""CPU: gsr_forward's per-frame choices (gsrast_amd/csrc/frame_policy.hpp) at their switch points. A small C++ driver is
compiled against the header with g++ (no HIP, no GPU) and evaluates the table below; every threshold is tried one step on
each side, so that moving any switch point by one unit fails a case. The GPU tests show that every choice gives the same
pixels; these show which choice each frame gets."""
import os
import subprocess

import pytest

from helpers import ROOT

from gsrast_amd import _capi

DRIVER = r"""
#include <cstdio>
#include "frame_policy.hpp"
using namespace gsr;
int main() {
    char rule[16];
    while (std::scanf("%15s", rule) == 1) {
        unsigned w, dc, ov, bf, mean, longest, calls, cus; unsigned long long tiles;
        std::scanf("%u %u %u %u %u %u %u %llu %u", &w, &dc, &ov, &bf, &mean, &longest, &calls, &tiles, &cus);
        HistoryView h;
        h.wanted = w; h.decorrelated = dc; h.overlapped = ov; h.block_fed = bf; h.mean = mean; h.longest = longest; h.calls = calls;
        const DeviceShape shape = device_shape_of((int)cus);
        if (rule[0] == 'h') {                     // history: fresh s1 s2 s4
            unsigned fresh, s[5] = {1, 0, 0, 0, 0};
            std::scanf("%u %u %u %u", &fresh, &s[1], &s[2], &s[4]);
            const HistoryStep r = step_history(h, fresh ? s : nullptr, tiles, shape);
            std::printf("%d %d %u %u %d\n", r.view.wanted, r.view.decorrelated, r.view.mean, r.view.longest, r.order_now);
        } else if (rule[0] == 'e') {              // early: n flags precomp xy_plan + EnvKnobs
            int n, precomp, xy, cb, fd, pct, dr; unsigned flags;
            std::scanf("%d %u %d %d %d %d %d %d", &n, &flags, &precomp, &xy, &cb, &fd, &pct, &dr);
            const EnvKnobs env{true, cb, fd, pct, dr, false};
            const EarlyChoice r = choose_early(n, flags, precomp, xy, h, tiles, env, shape);
            std::printf("%d %zu %d %d\n", r.colors_mode, r.colors_early, r.fused_depth, r.depth_records);
        } else if (rule[0] == 'b' && rule[1] == 'i') {   // binning: R V big xy_plan blockbin_ok flags
            unsigned R, V, flags; unsigned long long big; int xy, ok;
            std::scanf("%u %u %llu %d %d %u", &R, &V, &big, &xy, &ok, &flags);
            const BinningChoice r = choose_binning(R, V, big, xy, ok, flags, h, tiles, shape);
            std::printf("%d %d %d %d %u\n", r.use_blocks, r.overlap, r.blend_from_lists, r.block_fed, r.plan_used);
        } else {                                  // blend: R V block_fed order_now colors_mode flags deep_by_history
            unsigned R, V, flags; int fed, order, mode, by_history;
            std::scanf("%u %u %d %d %d %u %d", &R, &V, &fed, &order, &mode, &flags, &by_history);
            const BlendChoice r = choose_blend(R, V, fed, order, mode, flags, h, tiles, by_history, shape);
            std::printf("%d %d %d\n", r.deep_wanted, r.deep_all, r.deep_waves);
        }
    }
    return 0;
}
"""

F = {k[len("GSR_FLAG_"):]: getattr(_capi, k) for k in dir(_capi) if k.startswith("GSR_FLAG_")}
SORT, BLOCKS, GENERIC = 1, 2, 3
LISTS_SKIPPED, FROM_LISTS, OVERLAPPED = 0x100, 0x200, 0x800
TILES = 120 * 68            # 1920 x 1080
M = 1 << 24

INPUTS = {
    "history": ["fresh", "s1", "s2", "s4"],
    "early": ["n", "flags", "precomp", "xy_plan", "colors_beside", "fused_depth", "colors_early_pct", "depth_records"],
    "binning": ["R", "V", "big", "xy_plan", "blockbin_ok", "flags"],
    "blend": ["R", "V", "block_fed_now", "order_now", "colors_mode", "flags", "deep_by_history"],
}
OUTPUTS = {
    "history": ["wanted", "decorrelated", "mean", "longest", "order_now"],
    "early": ["colors_mode", "colors_early", "fused_depth", "depth_records"],
    "binning": ["use_blocks", "overlap", "blend_from_lists", "block_fed", "plan_used"],
    "blend": ["deep_wanted", "deep_all", "deep_waves"],
}
DEFAULTS = dict(wanted=0, decorrelated=0, overlapped=0, block_fed=0, mean=0, longest=0, calls=0, tiles=TILES, cus=256,
                fresh=1, s1=0, s2=0, s4=0, flags=0, precomp=0, xy_plan=1, colors_beside=-1, fused_depth=-1,
                colors_early_pct=-1, depth_records=-1, big=0, blockbin_ok=1, block_fed_now=0, order_now=0, colors_mode=1,
                deep_by_history=0)
HIST = ["wanted", "decorrelated", "overlapped", "block_fed", "mean", "longest", "calls", "tiles", "cus"]

# (rule, inputs — history fields and the rule's own, the rest as DEFAULTS —, the outputs expected)
# On a whole MI355X (256 CUs): 5 120 blend wave slots, 3 072 beside the emission, a light frame below 128 000 000 ticks.
CASES = [
    # the history's refresh: 2 x 5 120 x longest > 5 x tiles x mean, or a light frame (tiles x mean < 128 M)
    ("history", dict(s1=62503, s2=15687), dict(wanted=1, mean=15687, longest=62503, order_now=1)),
    ("history", dict(s1=62502, s2=15687), dict(wanted=0, order_now=0)),
    ("history", dict(s1=1, s2=15686), dict(wanted=1)),                       # 127 997 760: light
    ("history", dict(s1=1, s2=15687), dict(wanted=0)),                       # 128 005 920
    ("history", dict(s1=5, s2=0), dict(wanted=1, mean=0)),                   # (no mean: no light frame, any longest tile wins)
    ("history", dict(s1=0, s2=0), dict(wanted=0)),
    ("history", dict(s1=1, s2=15687, s4=1), dict(wanted=0, decorrelated=1, order_now=1)),
    # ... not fresh: the figures stay, and every fourth call sorts
    ("history", dict(fresh=0, wanted=1, mean=7, longest=9, s1=62503, s2=15687), dict(wanted=1, mean=7, longest=9, order_now=1)),
    ("history", dict(fresh=0, decorrelated=1), dict(decorrelated=1, order_now=1)),
    ("history", dict(fresh=0, calls=0), dict(order_now=0)),
    ("history", dict(fresh=0, calls=1), dict(order_now=1)),
    ("history", dict(fresh=0, calls=2), dict(order_now=0)),
    ("history", dict(fresh=0, calls=3), dict(order_now=0)),
    ("history", dict(fresh=0, calls=5), dict(order_now=1)),

    # where geomState.rgb is written: beside the depth sort up to 2^24 Gaussians, beside the blend beyond
    ("early", dict(n=M), dict(colors_mode=1, colors_early=0, fused_depth=0, depth_records=0)),
    ("early", dict(n=M + 1), dict(colors_mode=2, colors_early=0, fused_depth=1, depth_records=1)),
    ("early", dict(n=M + 1, mean=1, overlapped=1), dict(colors_mode=1)),     # (the last blend ran beside the emission)
    ("early", dict(n=M + 1, mean=0, overlapped=1), dict(colors_mode=2)),
    ("early", dict(n=M + 1, flags=F["SEMANTICS_INRIA"]), dict(colors_mode=0, fused_depth=1)),
    ("early", dict(n=M + 1, precomp=1), dict(colors_mode=0)),
    ("early", dict(n=M + 1, flags=F["SERIAL_EMIT"]), dict(colors_mode=0)),
    ("early", dict(n=100, colors_beside=0), dict(colors_mode=0)),
    ("early", dict(n=100, colors_beside=2), dict(colors_mode=2, colors_early=0)),
    ("early", dict(n=M + 1, colors_beside=1), dict(colors_mode=1)),
    ("early", dict(n=M + 1, colors_beside=2, precomp=1), dict(colors_mode=0)),
    # ... of those beside the blend, the share that starts behind the preprocess: what the last blend leaves uncovered of
    # 2 040 ticks per million Gaussians (50 M: 102 000), at most half; a fixed share from the environment
    ("early", dict(n=50_000_000, mean=1, longest=61200), dict(colors_mode=2, colors_early=20_000_000)),   # 40 %
    ("early", dict(n=50_000_000, mean=1, longest=61201), dict(colors_early=19_500_000)),                  # 39.99 %
    ("early", dict(n=50_000_000, mean=1, longest=1), dict(colors_early=25_000_000)),                      # (99 %: half)
    ("early", dict(n=50_000_000, mean=40000, longest=1), dict(colors_early=18_500_000)),                  # 63 750: 37.5 %
    ("early", dict(n=50_000_000, mean=1, longest=102000), dict(colors_early=0)),
    ("early", dict(n=50_000_000), dict(colors_mode=2, colors_early=0)),                                   # (no history)
    ("early", dict(n=50_000_000, mean=1, longest=1, decorrelated=1), dict(colors_early=0)),
    ("early", dict(n=50_000_000, colors_early_pct=30), dict(colors_early=15_000_000)),
    ("early", dict(n=50_000_000, colors_early_pct=0, mean=1, longest=1), dict(colors_early=0)),
    ("early", dict(n=1000, colors_early_pct=30), dict(colors_mode=1, colors_early=0)),
    # ... and the depth order: without the compaction beyond 2^24, in 12-byte records where it has none
    ("early", dict(n=M + 1, xy_plan=0), dict(fused_depth=0, depth_records=0)),
    ("early", dict(n=M, fused_depth=1), dict(fused_depth=1, depth_records=1)),
    ("early", dict(n=M + 1, fused_depth=0), dict(fused_depth=0, depth_records=0)),
    ("early", dict(n=M + 1, depth_records=0), dict(fused_depth=1, depth_records=0)),
    ("early", dict(n=M, depth_records=1), dict(fused_depth=0, depth_records=1)),

    # the binning plan: blocks from 6 instances per visible Gaussian, or with an eighth of them in big splats
    ("binning", dict(R=6000, V=1000), dict(use_blocks=1, plan_used=BLOCKS | FROM_LISTS)),
    ("binning", dict(R=5999, V=1000), dict(use_blocks=0, overlap=0, blend_from_lists=0, block_fed=0, plan_used=SORT)),
    ("binning", dict(R=5000, V=1000, big=625), dict(use_blocks=1)),
    ("binning", dict(R=5000, V=1000, big=624), dict(use_blocks=0)),
    ("binning", dict(R=100000, V=1000, flags=F["PLAN_SORT"]), dict(use_blocks=0, plan_used=SORT)),
    ("binning", dict(R=1000, V=1000, flags=F["PLAN_BLOCKS"]), dict(use_blocks=1)),
    ("binning", dict(R=100000, V=1000, blockbin_ok=0), dict(use_blocks=0, plan_used=SORT)),
    ("binning", dict(R=100000, V=1000, xy_plan=0, flags=F["PLAN_BLOCKS"]), dict(use_blocks=0, plan_used=GENERIC)),
    # ... a serial blend reads the block lists from 48 instances per visible Gaussian
    ("binning", dict(R=48000, V=1000), dict(blend_from_lists=0, block_fed=1, plan_used=BLOCKS)),
    ("binning", dict(R=47999, V=1000), dict(blend_from_lists=1, block_fed=0, plan_used=BLOCKS | FROM_LISTS)),
    ("binning", dict(R=10000, V=1000, flags=F["NO_SORTED_LISTS"]),
     dict(overlap=0, blend_from_lists=0, block_fed=1, plan_used=BLOCKS | LISTS_SKIPPED)),
    ("binning", dict(R=10000, V=1000, flags=F["OVERLAP_EMIT"]),
     dict(overlap=1, blend_from_lists=0, block_fed=1, plan_used=BLOCKS | OVERLAPPED)),
    ("binning", dict(R=10000, V=1000, flags=F["OVERLAP_EMIT"] | F["NO_SORTED_LISTS"]),
     dict(overlap=0, block_fed=1, plan_used=BLOCKS | LISTS_SKIPPED)),
    # ... beside the emission from 16 instances per visible Gaussian, when the last blend's times say it is the shorter:
    # R = 16 000 emits in 4 ticks, under the floor of 7 000: the limit is 14 000
    ("binning", dict(R=16000, V=1000, mean=1, longest=13999, block_fed=1), dict(overlap=1, plan_used=BLOCKS | OVERLAPPED)),
    ("binning", dict(R=16000, V=1000, mean=1, longest=14000, block_fed=1), dict(overlap=0)),
    ("binning", dict(R=15999, V=1000, mean=1, longest=1, block_fed=1), dict(overlap=0, blend_from_lists=1)),
    ("binning", dict(R=16000, V=1000, mean=1, longest=1, block_fed=1, decorrelated=1), dict(overlap=0)),
    ("binning", dict(R=16000, V=1000, mean=0, longest=1, block_fed=1), dict(overlap=0)),
    ("binning", dict(R=16000, V=1000, mean=1, longest=1, block_fed=1, flags=F["SERIAL_EMIT"]), dict(overlap=0)),
    ("binning", dict(R=16000, V=1000, mean=1, longest=1, block_fed=1, flags=F["NO_SORTED_LISTS"]),
     dict(overlap=0, plan_used=BLOCKS | LISTS_SKIPPED)),
    # ... times of a blend that read the sorted lists: x (R + 10 V) / R = 1.625
    ("binning", dict(R=16000, V=1000, mean=1, longest=8615), dict(overlap=1)),                    # 13 999
    ("binning", dict(R=16000, V=1000, mean=1, longest=8616), dict(overlap=0)),                    # 14 001
    # ... the mean over the 5 120 wave slots: 1 x 8 160 / 5 120 = 1; 8 784 x 8 160 / 5 120 = 13 999.5
    ("binning", dict(R=16000, V=1000, mean=8784, longest=1, block_fed=1), dict(overlap=1)),
    ("binning", dict(R=16000, V=1000, mean=8785, longest=1, block_fed=1), dict(overlap=0)),
    # ... twice the limit where the frame is block-fed either way (48 V), the emission's 12 R bytes at 4 TB/s from 7 000 ticks
    ("binning", dict(R=48000, V=1000, mean=1, longest=27999, block_fed=1), dict(overlap=1)),
    ("binning", dict(R=48000, V=1000, mean=1, longest=28000, block_fed=1), dict(overlap=0)),
    ("binning", dict(R=47999, V=1000, mean=1, longest=14000, block_fed=1), dict(overlap=0)),
    ("binning", dict(R=47999, V=1000, mean=1, longest=13999, block_fed=1), dict(overlap=1)),
    ("binning", dict(R=23_333_334, V=1_000_000, mean=1, longest=6999, block_fed=1), dict(overlap=1)),     # 7 000 ticks
    ("binning", dict(R=23_333_334, V=1_000_000, mean=1, longest=7000, block_fed=1), dict(overlap=0)),
    ("binning", dict(R=23_333_333, V=1_000_000, mean=1, longest=13999, block_fed=1), dict(overlap=1)),    # 6 999: 14 000
    # ... once overlapped: the time alone (b - 0.54 e above e = 7 000, 0.46 b below) within 1.1 x the limit
    ("binning", dict(R=16000, V=1000, mean=1, longest=19179, block_fed=1, overlapped=1), dict(overlap=1)),
    ("binning", dict(R=16000, V=1000, mean=1, longest=19180, block_fed=1, overlapped=1), dict(overlap=0)),
    ("binning", dict(R=16000, V=1000, mean=1, longest=30000, block_fed=1, overlapped=0), dict(overlap=0)),
    ("binning", dict(R=16000, V=1000, mean=1, longest=7000, block_fed=1, overlapped=1), dict(overlap=1)),
    # ... over the 3 072 slots beside the emission: 7 230 x 8 160 / 3 072 = 19 204 (11 522 over 5 120)
    ("binning", dict(R=16000, V=1000, mean=7230, longest=1, block_fed=1, overlapped=1), dict(overlap=0)),
    ("binning", dict(R=16000, V=1000, mean=7220, longest=1, block_fed=1, overlapped=1), dict(overlap=1)),   # 19 178

    # deep tiles: every tile of a list-fed blend below 16 instances per visible Gaussian
    ("blend", dict(R=15999, V=1000), dict(deep_wanted=0, deep_all=1, deep_waves=4)),
    ("blend", dict(R=16000, V=1000), dict(deep_all=0, deep_waves=4)),
    ("blend", dict(R=15999, V=1000, colors_mode=2), dict(deep_all=0)),
    ("blend", dict(R=15999, V=1000, block_fed_now=1), dict(deep_all=0)),
    ("blend", dict(R=15999, V=1000, flags=F["NO_DEEP_TILES"]), dict(deep_all=0)),
    ("blend", dict(R=16000, V=1000, flags=F["DEEP_TILES_ALL"]), dict(deep_all=1, deep_waves=4)),
    ("blend", dict(R=16000, V=1000, flags=F["DEEP_TILES_ALL"] | F["NO_DEEP_TILES"], colors_mode=2), dict(deep_all=1)),
    ("blend", dict(R=16000, V=1000, flags=F["DEEP_TILES_ALL"], block_fed_now=1), dict(deep_all=0)),
    ("blend", dict(R=16000, V=1000, flags=F["DEEP_WAVES_8"]), dict(deep_all=1, deep_waves=8)),
    ("blend", dict(R=16000, V=1000, flags=F["DEEP_WAVES_16"]), dict(deep_all=1, deep_waves=16)),
    ("blend", dict(R=16000, V=1000, flags=F["DEEP_WAVES_8"] | F["DEEP_WAVES_16"]), dict(deep_waves=16)),
    # ... waves per deep tile from the tiles as long as the longest (tiles x mean / longest) against the 1 024 SIMDs
    ("blend", dict(R=1000, V=1000, mean=256, longest=TILES), dict(deep_waves=16)),
    ("blend", dict(R=1000, V=1000, mean=257, longest=TILES), dict(deep_waves=8)),
    ("blend", dict(R=1000, V=1000, mean=1024, longest=TILES), dict(deep_waves=8)),
    ("blend", dict(R=1000, V=1000, mean=1025, longest=TILES), dict(deep_waves=4)),
    ("blend", dict(R=1000, V=1000, mean=256, longest=TILES, cus=32), dict(deep_waves=4)),          # (128 SIMDs)
    ("blend", dict(R=1000, V=1000, mean=32, longest=TILES, cus=32), dict(deep_waves=16)),
    ("blend", dict(R=1000, V=1000, mean=256, longest=TILES, decorrelated=1), dict(deep_waves=4)),
    ("blend", dict(R=1000, V=1000, mean=256, longest=0), dict(deep_waves=4)),
    ("blend", dict(R=1000, V=1000, mean=256, longest=TILES, flags=F["DEEP_TILES_ALL"]), dict(deep_waves=4)),
    ("blend", dict(R=1000, V=1000, mean=256, longest=TILES, flags=F["DEEP_WAVES_8"]), dict(deep_waves=8)),
    ("blend", dict(R=16000, V=1000, mean=256, longest=TILES), dict(deep_all=0, deep_waves=4)),
    # ... GSR_DEEP_BY_HISTORY: the history's slowest tiles of an order sorted for this call
    ("blend", dict(R=16000, V=1000, deep_by_history=1, order_now=1), dict(deep_wanted=1, deep_all=0)),
    ("blend", dict(R=16000, V=1000, deep_by_history=1, order_now=0), dict(deep_wanted=0)),
    ("blend", dict(R=16000, V=1000, deep_by_history=1, order_now=1, decorrelated=1), dict(deep_wanted=0)),
    ("blend", dict(R=16000, V=1000, deep_by_history=1, order_now=1, block_fed_now=1), dict(deep_wanted=0)),
    ("blend", dict(R=16000, V=1000, deep_by_history=1, order_now=1, flags=F["NO_DEEP_TILES"]), dict(deep_wanted=0)),
    ("blend", dict(R=16000, V=1000, deep_by_history=0, order_now=1), dict(deep_wanted=0)),
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("frame_policy")
    (d / "driver.cpp").write_text(DRIVER)
    exe = d / "driver"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "gsrast_amd", "csrc"),
                           str(d / "driver.cpp"), "-o", str(exe)])
    return str(exe)


def _evaluate(driver, cases):
    lines = []
    for rule, given, _ in cases:
        v = {**DEFAULTS, **given}
        lines.append(" ".join([rule] + [str(v[k]) for k in HIST + INPUTS[rule]]))
    out = subprocess.check_output([driver], input="\n".join(lines) + "\n", text=True).splitlines()
    assert len(out) == len(cases)
    return [dict(zip(OUTPUTS[rule], map(int, line.split()))) for (rule, _, _), line in zip(cases, out)]


def test_header_needs_no_hip():
    text = open(os.path.join(ROOT, "gsrast_amd", "csrc", "frame_policy.hpp")).read()
    assert "hip_runtime" not in text and "gsr_common.hpp" not in text


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: f"{CASES[i][0]}-{i}")
def test_rule_at_its_switch_point(driver, i):
    rule, given, expected = CASES[i]
    got = _evaluate(driver, [CASES[i]])[0]
    assert {k: got[k] for k in expected} == expected, (rule, given, got)


def test_big_splat_size_is_the_measured_one(driver):
    """kBigSplatTiles is handed to the preprocess and the scan, which count the instances of such splats; the plan's rule
    sees only their count (the `big` cases above), so the size itself is pinned here: 16 x 16 tiles."""
    src = '#include <cstdio>\n#include "frame_policy.hpp"\nint main() { std::printf("%u", gsr::kBigSplatTiles); }\n'
    d = os.path.dirname(driver)
    with open(os.path.join(d, "big.cpp"), "w") as f:
        f.write(src)
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "gsrast_amd", "csrc"), os.path.join(d, "big.cpp"),
                           "-o", os.path.join(d, "big")])
    assert subprocess.check_output([os.path.join(d, "big")], text=True) == "256"
