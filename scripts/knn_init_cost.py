"""What the initialisation from a point cloud costs: gsr_knn_mean_dist2 (csrc/knn.hip) on positions of the bench scene
(bench.py's own scene builder) — a seeded subset of 10^5 and of 10^6 of them and all of them — each as it is and with 0.1 %
of the points moved 100 x further out from the centroid (the outliers of an SfM cloud); and what a user has without it, a
chunked torch.cdist + topk(4, largest=False) (the point itself is the first of the four), with 60 s to finish in.

  python scripts/knn_init_cost.py [--reps N] [--out FILE]     medians of device-event times per call, after a warm-up, the
                                                              variants interleaved round by round; then the baseline
  rocprofv3 --kernel-trace -d DIR -o knn --output-format csv -- python scripts/knn_init_cost.py --trace-run
                                                              the same clouds, one warm-up and TRACED calls each, nothing else
  python scripts/knn_init_cost.py --split DIR [--out FILE]    the per-kernel split of that trace: code + sort, boxes, search
                                                              (--out appends; the sort's clears are memsets, not kernels of
                                                              the library, and are not counted)
profiles/knn_init_cost.txt is the output of the first and the third."""
import csv
import glob
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = (100_000, 1_000_000, None)             # None: every position of the bench scene
TRACED = 3
BASELINE_SECONDS = 60.0
GROUPS = (("code + sort", ("knn_bounds", "knn_code", "histogram_bits", "onesweep")), ("boxes", ("knn_gather", "knn_node")),
          ("search", ("knn_search",)))


def _arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def clouds(dev):
    """[(label, xyz on the device)] in the order every mode of this script walks them."""
    import torch
    import bench
    sc, _, _, _, label = bench.make_scene("garden_like", bench.DEFAULT_SPLATS, dev)
    pos = np.ascontiguousarray(sc["means3D"][:, :3], np.float32)
    rng = np.random.default_rng(1)
    out = []
    for size in SIZES:
        p = pos if size is None else pos[np.sort(rng.choice(pos.shape[0], size, replace=False))]
        far = p.copy()
        rows = rng.choice(p.shape[0], p.shape[0] // 1000, replace=False)
        centre = p.mean(axis=0, dtype=np.float64).astype(np.float32)
        far[rows] = centre + np.float32(100.0) * (p[rows] - centre)
        out.append((f"{p.shape[0]:>8d} points", torch.from_numpy(p).to(dev)))
        out.append((f"{p.shape[0]:>8d} points, 0.1 % outliers", torch.from_numpy(far).to(dev)))
    return out, label


def caller(xyz):
    import torch
    from gsrast_amd import _capi
    L = _capi.lib()
    n = int(xyz.shape[0])
    out = torch.empty(n, dtype=torch.float32, device=xyz.device)
    temp = torch.empty(int(L.gsr_knn_temp_bytes(n)), dtype=torch.uint8, device=xyz.device)
    stream = torch.cuda.current_stream(xyz.device).cuda_stream
    return (lambda: _capi.check(L.gsr_knn_mean_dist2(n, xyz.data_ptr(), out.data_ptr(), temp.data_ptr(), stream), "gsr_knn_mean_dist2")), out


def timed(fn):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def cdist_baseline(xyz, budget):
    """(mean_dist2, seconds, the share of the queries done): chunks of at most 2^29 distances, until `budget` seconds are over."""
    import torch
    n = int(xyz.shape[0])
    chunk = max(1, min(n, (1 << 29) // n))
    out = torch.empty(n, dtype=torch.float32, device=xyz.device)
    torch.cuda.synchronize()
    t0, done = time.perf_counter(), 0
    while done < n and time.perf_counter() - t0 < budget:
        d = torch.cdist(xyz[done:done + chunk], xyz)
        near = torch.topk(d, 4, dim=1, largest=False).values[:, 1:]
        out[done:done + chunk] = (near * near).mean(dim=1)
        done += chunk
        torch.cuda.synchronize()
    return out, time.perf_counter() - t0, min(done, n) / n


def measure(reps):
    import torch
    dev = torch.device("cuda:0")
    sets, label = clouds(dev)
    out = [f"kNN initialisation cost, {torch.cuda.get_device_name(0)}, medians of {reps} rounds of device-event times per call",
           f"positions: bench scene ({label}); subsets are seeded draws of its rows"]
    calls = [(name, xyz) + caller(xyz) for name, xyz in sets]
    for _ in range(2):
        for _, _, fn, _ in calls:
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _, _ in calls}
    for _ in range(reps):
        for name, _, fn, _ in calls:
            ms[name].append(timed(fn))
    out.append("gsr_knn_mean_dist2 (bounds, code, eight sort passes, gather, boxes, search), exact:")
    med = {k: float(np.median(v)) for k, v in ms.items()}
    for i, (name, xyz, _, _) in enumerate(calls):
        v, n = ms[name], int(xyz.shape[0])
        line = f"  {name:<34s}{med[name]:9.3f} ms (rounds {min(v):.3f} .. {max(v):.3f}) = {med[name] * 1e6 / n:7.2f} ns per point"
        if i % 2 == 1:
            line += f"; {med[name] / med[calls[i - 1][0]]:.2f} x the plain cloud"
        out.append(line)
    out.append(f"the baseline a user has without it: torch.cdist + topk(4, largest=False) in chunks, given {BASELINE_SECONDS:.0f} s")
    for i in (0, 2):
        name, xyz, _, ours = calls[i]
        got, seconds, share = cdist_baseline(xyz, BASELINE_SECONDS)
        if share < 1.0:
            out.append(f"  {name:<34s}did not finish: {100 * share:.1f} % of the queries in {seconds:.1f} s "
                       f"(at that rate {seconds / share:.0f} s for all; ours {med[name]:.3f} ms)")
        else:
            rel = float(((got - ours).abs() / ours.clamp(min=1e-30)).max())
            out.append(f"  {name:<34s}{seconds * 1e3:9.1f} ms = {seconds * 1e3 / med[name]:.0f} x ours; its result differs from the exact "
                       f"one by at most {rel:.1e} relative (cdist goes through a matrix product)")
        del got
        torch.cuda.empty_cache()
    return out


def trace_run():
    import torch
    sets, _ = clouds(torch.device("cuda:0"))
    for name, xyz in sets:
        fn, _ = caller(xyz)
        for _ in range(1 + TRACED):
            fn()
        torch.cuda.synchronize()
        print("traced", name, flush=True)


def split(trace_dir):
    f = glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = [r for r in csv.DictReader(open(f)) if "gsr::" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], []
    for r in rows:
        cur.append(r)
        if "knn_search_kernel" in r["Kernel_Name"]:
            calls.append(cur)
            cur = []
    per = 1 + TRACED
    assert len(calls) == 2 * len(SIZES) * per, f"{len(calls)} calls in the trace, expected {2 * len(SIZES) * per}"
    out = [f"per-kernel split (rocprofv3 --kernel-trace, a run of its own; kernel time summed per group, medians of {TRACED} calls"
           " after a warm-up; the clouds in the order above):"]
    for v in range(2 * len(SIZES)):
        sums = {g: [] for g, _ in GROUPS}
        for c in calls[v * per + 1:(v + 1) * per]:
            tot = {g: 0 for g, _ in GROUPS}
            for r in c:
                group = [g for g, keys in GROUPS if any(k in r["Kernel_Name"] for k in keys)]
                assert len(group) == 1, r["Kernel_Name"]
                tot[group[0]] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
            for g in tot:
                sums[g].append(tot[g] / 1e6)
        launches = len(calls[v * per + 1])
        out.append(f"  cloud {v + 1} ({'plain' if v % 2 == 0 else 'outliers'}, {launches} kernels): "
                   + ", ".join(f"{g} {float(np.median(sums[g])):.3f} ms" for g, _ in GROUPS))
    return out


def main():
    if "--trace-run" in sys.argv:
        trace_run()
        return
    out = split(sys.argv[sys.argv.index("--split") + 1]) if "--split" in sys.argv else measure(_arg("--reps", 10))
    print("\n".join(out), flush=True)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a" if "--split" in sys.argv else "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
