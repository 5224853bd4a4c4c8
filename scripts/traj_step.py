#!/usr/bin/env python3
"""Device time of one trajectory-query step: geohip_traj_group + geohip_tstats over one window.

    python scripts/traj_step.py                       # 10 M points at 100 k and at 1 k trajectories
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/<T> -o traj -- \\
        python scripts/traj_step.py --traj <T> --out DIR/<T>/step.json     # per-kernel run, one per T
    python scripts/traj_step.py --merge DIR --out profiles/traj_step.json  # fold the stats in

The window comes from synth.trajectories (interleaved arrival, objIDs veh-<k>, a share of late
timestamps), is uploaded once, and each step is timed with events on the ctx's stream after
warm-up steps.  traj_group reads the trajectory count back in the middle of its step (one host
round trip) and tstats its error word at the end, so a step's event time holds those gaps; the
per-kernel times come from the profiler run.  Bytes are the algorithm's: objID bytes + offsets
+ 24 B per point read, plus the outputs; the share of peak is those bytes over the step time over
the HBM3E peak of the MI355X.  Needs the GPU: there is no other path.
"""
from __future__ import annotations

import argparse
import csv
import json
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_PEAK_BYTES_PER_S = 8.0e12  # MI355X HBM3E spec peak


def algorithmic_bytes(n, oid_bytes, n_traj, n_sel):
    read = oid_bytes + 8 * (n + 1) + 24 * n
    written = 4 * n + 4 * n_sel + 4 * n_traj + 4 * (n_traj + 1) + 24 * n_traj
    return read, written


def run_case(ctx, n, n_traj, seed, warmup, iters):
    import numpy as np
    import torch
    from spatialflink_amd import synth

    w = synth.trajectories(n, n_traj, seed)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to("cuda:0")  # noqa: E731
    x, y, ts = dev(w["x"], np.float64), dev(w["y"], np.float64), dev(w["ts"], np.int64)
    ot, oo = dev(w["oid_text"], np.uint8), dev(w["oid_off"].view(np.int64), np.int64)
    torch.cuda.synchronize()
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    group_ms, stats_ms = [], []
    g = None
    for it in range(warmup + iters):
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        g = ctx.traj_group(ot, oo)
        e1.record()
        out = ctx.tstats(x, y, ts, g["perm"], g["traj_off"])
        e2.record()
        torch.cuda.synchronize()
        if it >= warmup:
            group_ms.append(e0.elapsed_time(e1))
            stats_ms.append(e1.elapsed_time(e2))
    # the grouping at this size against numpy: dense ids in order of first appearance
    u, first = np.unique(w["traj"], return_index=True)
    dense = np.empty(int(u.max()) + 1, dtype=np.int64)
    dense[u[np.argsort(first)]] = np.arange(len(u))
    if not np.array_equal(g["traj_of"].cpu().numpy(), dense[w["traj"]]):
        raise SystemExit("traj_group: grouping differs from the host's")
    lens = (g["traj_off"][1:] - g["traj_off"][:-1]).cpu().numpy()
    read, written = algorithmic_bytes(n, int(ot.numel()), g["n_traj"], g["n_sel"])
    med = lambda v: float(np.median(v))  # noqa: E731
    step = med(np.array(group_ms) + np.array(stats_ms))
    finite = int(torch.isfinite(out[0]).sum())
    return {
        "n": n, "n_traj": g["n_traj"], "n_sel": g["n_sel"], "oid_bytes": int(ot.numel()),
        "points_per_traj": {"min": int(lens.min()), "median": float(np.median(lens)), "max": int(lens.max())},
        "warmup": warmup, "iters": iters,
        "traj_group_ms": {"median": med(group_ms), "min": float(min(group_ms)), "max": float(max(group_ms))},
        "tstats_ms": {"median": med(stats_ms), "min": float(min(stats_ms)), "max": float(max(stats_ms))},
        "step_ms_median": step,
        "algorithmic_bytes": {"read": read, "written": written, "total": read + written},
        "bytes_per_s": (read + written) / (step * 1e-3),
        "fraction_of_hbm_peak": (read + written) / (step * 1e-3) / HBM_PEAK_BYTES_PER_S,
        "finite_spatial_lengths": finite,
    }


def short_name(name: str) -> str:
    """geohip::traj_insert, or rocprim::<kernel>[<algorithm>] for the library's sort and scan kernels."""
    name = re.sub(r"ROCPRIM_\d+_NS::", "", name.replace("(anonymous namespace)::", ""))
    name = name[5:] if name.startswith("void ") else name
    head = re.match(r"[\w:]+", name).group(0)
    algo = re.search(r"wrapped_(\w+?)_config", name)
    return f"{head}[{algo.group(1)}]" if algo else head


def merge(stats_dir: Path, out: Path):
    """Fold rocprofv3's kernel statistics (one run per trajectory count, under stats_dir/<T>/) into
    the result file: per kernel its calls, total and average time, and its time per step."""
    doc = json.loads(out.read_text())
    for case in doc["cases"]:
        d = stats_dir / str(case["n_traj_asked"])
        files = sorted(d.rglob("*kernel_stats.csv"))
        side = d / "step.json"
        if not files or not side.exists():
            continue
        steps = json.loads(side.read_text())["cases"][0]
        steps = steps["warmup"] + steps["iters"]
        by_name = {}
        with files[0].open() as f:
            for row in csv.DictReader(f):
                name = row["Name"]
                # the step's kernels, and the runtime's fill kernel (the table reset is a hipMemsetAsync);
                # torch's own kernels and the window's upload are not part of the step
                if "geohip::" not in name and "rocprim" not in name and "fillBuffer" not in name:
                    continue
                k = by_name.setdefault(short_name(name), {"calls": 0, "total_ms": 0.0})
                k["calls"] += int(row["Calls"])
                k["total_ms"] += int(row["TotalDurationNs"]) / 1e6
        kernels = [{"name": nm, "calls": k["calls"], "total_ms": k["total_ms"], "per_step_ms": k["total_ms"] / steps}
                   for nm, k in by_name.items()]
        kernels.sort(key=lambda k: -k["total_ms"])
        case["kernels_profiled_run"] = {"steps": steps, "kernel_ms_per_step": sum(k["per_step_ms"] for k in kernels),
                                        "kernels": kernels}
    out.write_text(json.dumps(doc, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--traj", type=int, nargs="+", default=[100_000, 1_000])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "traj_step.json")
    ap.add_argument("--merge", type=Path, default=None, help="directory of per-T rocprofv3 runs to fold into --out")
    a = ap.parse_args()
    if a.merge is not None:
        merge(a.merge, a.out)
        return
    from spatialflink_amd import Context, _abi
    ctx = Context(0)  # raises without an MI355X
    cases = []
    for t in a.traj:
        c = run_case(ctx, a.n, t, a.seed, a.warmup, a.iters)
        c["n_traj_asked"] = t
        cases.append(c)
        print(json.dumps({k: c[k] for k in ("n", "n_traj", "traj_group_ms", "tstats_ms", "fraction_of_hbm_peak")}))
    doc = {"what": "geohip_traj_group + geohip_tstats, one window, device events on the ctx stream",
           "library": _abi.version(), "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "cases": cases}
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
