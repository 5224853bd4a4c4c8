#!/usr/bin/env python3
"""Device time of the per-cell trajectory aggregate: geohip_traj_group_flags + geohip_tagg_cells
over one window, next to geohip_traj_group + geohip_tstats over the same window in the same process
(the yardstick: the other trajectory step, scripts/traj_step.py).

    python scripts/tagg_time.py                       # 10 M points at 100 k and at 1 k trajectories
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/<T> -o tagg -- \\
        python scripts/tagg_time.py --traj <T> --profiled --out DIR/<T>/step.json   # per-kernel run, one per T
    python scripts/tagg_time.py --merge DIR --out profiles/tagg_time.json           # fold the stats in

The window comes from synth.trajectories on the 500 x 500 Beijing grid, is uploaded once, and each
call is timed with events on the ctx's stream (3 warm-ups, median of 10).  geohip_tagg_cells reads
the cell rectangle back after its first kernel and the counts at its end (two host round trips), so
its event time holds those gaps; the per-kernel times come from the profiler run, which groups once
and then calls geohip_tagg_cells alone, so the library's sort and scan kernels in its statistics
are the aggregate's but for the one grouping's (1 call in 14).  Bytes are the algorithm's: 32 B per
selected point read (x, y, ts, traj_of, perm), 52 B per cell, 12 B per visit and the visit offsets
written.  The result is checked against numpy at this size (cells, visits, every cell's count and
sum).  Needs the GPU: there is no other path.
"""
from __future__ import annotations

import argparse
import csv
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

from traj_step import HBM_PEAK_BYTES_PER_S, short_name  # noqa: E402

GRID_ROWS = 500


def algorithmic_bytes(n_sel, n_cells, n_visits):
    read = 32 * n_sel
    written = 52 * n_cells + 12 * n_visits + 4 * (n_cells + 1)
    return read, written


def host_check(w, grid, r):
    """Cells, visits, per-cell count and sum with numpy (timestamps here never wrap)."""
    import numpy as np
    cx = np.floor((w["x"] - grid.min_x) / grid.cell_len).astype(np.int64)
    cy = np.floor((w["y"] - grid.min_y) / grid.cell_len).astype(np.int64)
    order = np.lexsort((w["traj"], cy, cx))
    cxs, cys, trs, tss = cx[order], cy[order], w["traj"][order], w["ts"][order]
    run_head = np.r_[True, (cxs[1:] != cxs[:-1]) | (cys[1:] != cys[:-1]) | (trs[1:] != trs[:-1])]
    starts = np.flatnonzero(run_head)
    lens = np.maximum.reduceat(tss, starts) - np.minimum.reduceat(tss, starts)
    rcx, rcy = cxs[starts], cys[starts]
    cell_head = np.r_[True, (rcx[1:] != rcx[:-1]) | (rcy[1:] != rcy[:-1])]
    cstarts = np.flatnonzero(cell_head)
    if r["n_visits"] != len(starts) or r["n_cells"] != len(cstarts):
        raise SystemExit(f"tagg_cells: {r['n_cells']} cells / {r['n_visits']} visits, numpy has {len(cstarts)} / {len(starts)}")
    xy = r["cell_xy"].cpu().numpy()
    if not (np.array_equal(xy[:, 0], rcx[cstarts]) and np.array_equal(xy[:, 1], rcy[cstarts])):
        raise SystemExit("tagg_cells: cells differ from numpy's")
    if not np.array_equal(r["count"].cpu().numpy(), np.diff(np.r_[cstarts, len(starts)])):
        raise SystemExit("tagg_cells: counts differ from numpy's")
    if not np.array_equal(r["sum"].cpu().numpy(), np.add.reduceat(lens, cstarts)):
        raise SystemExit("tagg_cells: sums differ from numpy's")


def run_case(ctx, n, n_traj, seed, warmup, iters, profiled):
    import numpy as np
    import torch
    from spatialflink_amd import _abi, synth

    w = synth.trajectories(n, n_traj, seed)
    bj = synth.BEIJING
    grid = _abi.make_grid(bj[0], bj[2], (bj[1] - bj[0]) / GRID_ROWS, GRID_ROWS)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to("cuda:0")  # noqa: E731
    x, y, ts = dev(w["x"], np.float64), dev(w["y"], np.float64), dev(w["ts"], np.int64)
    ot, oo = dev(w["oid_text"], np.uint8), dev(w["oid_off"].view(np.int64), np.int64)
    torch.cuda.synchronize()
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    times = {"traj_group_flags_ms": [], "tagg_cells_ms": [], "traj_group_ms": [], "tstats_ms": []}
    g = ctx.traj_group(ot, oo, null_key=True) if profiled else None
    r = None
    for it in range(warmup + iters):
        e = [ev() for _ in range(5)]
        e[0].record()
        if not profiled:
            g = ctx.traj_group(ot, oo, null_key=True)
        e[1].record()
        r = ctx.tagg_cells(grid, x, y, ts, g)
        e[2].record()
        if not profiled:
            g0 = ctx.traj_group(ot, oo)
            e[3].record()
            ctx.tstats(x, y, ts, g0["perm"], g0["traj_off"])
            e[4].record()
        torch.cuda.synchronize()
        if it >= warmup:
            times["traj_group_flags_ms"].append(e[0].elapsed_time(e[1]))
            times["tagg_cells_ms"].append(e[1].elapsed_time(e[2]))
            if not profiled:
                times["traj_group_ms"].append(e[2].elapsed_time(e[3]))
                times["tstats_ms"].append(e[3].elapsed_time(e[4]))
    host_check(w, grid, r)
    read, written = algorithmic_bytes(g["n_sel"], r["n_cells"], r["n_visits"])
    stat = lambda v: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}  # noqa: E731
    out = {"n": n, "n_traj": g["n_traj"], "n_sel": g["n_sel"], "n_cells": r["n_cells"], "n_visits": r["n_visits"],
           "grid_rows": GRID_ROWS, "warmup": warmup, "iters": iters, "profiled_run": bool(profiled)}
    out.update({k: stat(v) for k, v in times.items() if v and not (profiled and k == "traj_group_flags_ms")})
    t = out["tagg_cells_ms"]["median"]
    out["algorithmic_bytes"] = {"read": read, "written": written, "total": read + written}
    out["tagg_cells_bytes_per_s"] = (read + written) / (t * 1e-3)
    out["tagg_cells_fraction_of_hbm_peak"] = out["tagg_cells_bytes_per_s"] / HBM_PEAK_BYTES_PER_S
    if not profiled:
        out["aggregate_step_ms_median"] = float(np.median(np.array(times["traj_group_flags_ms"]) + np.array(times["tagg_cells_ms"])))
        out["tstats_step_ms_median"] = float(np.median(np.array(times["traj_group_ms"]) + np.array(times["tstats_ms"])))
    return out


def merge(stats_dir: Path, out: Path):
    """Fold rocprofv3's kernel statistics (one run per trajectory count, under stats_dir/<T>/) into the
    result file: per kernel its calls, total time and time per geohip_tagg_cells call."""
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
                if "geohip::" not in name and "rocprim" not in name and "fillBuffer" not in name:
                    continue
                k = by_name.setdefault(short_name(name), {"calls": 0, "total_ms": 0.0})
                k["calls"] += int(row["Calls"])
                k["total_ms"] += int(row["TotalDurationNs"]) / 1e6
        kernels = [{"name": nm, "calls": k["calls"], "total_ms": k["total_ms"], "per_call_ms": k["total_ms"] / steps}
                   for nm, k in by_name.items()]
        kernels.sort(key=lambda k: -k["total_ms"])
        case["kernels_profiled_run"] = {"tagg_cells_calls": steps, "groupings": 1,
                                        "kernel_ms_per_call": sum(k["per_call_ms"] for k in kernels), "kernels": kernels}
    out.write_text(json.dumps(doc, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--traj", type=int, nargs="+", default=[100_000, 1_000])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--profiled", action="store_true", help="group once, then geohip_tagg_cells alone (the rocprofv3 run)")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "tagg_time.json")
    ap.add_argument("--merge", type=Path, default=None, help="directory of per-T rocprofv3 runs to fold into --out")
    a = ap.parse_args()
    if a.merge is not None:
        merge(a.merge, a.out)
        return
    from spatialflink_amd import Context, _abi
    ctx = Context(0)  # raises without an MI355X
    cases = []
    for t in a.traj:
        c = run_case(ctx, a.n, t, a.seed, a.warmup, a.iters, a.profiled)
        c["n_traj_asked"] = t
        cases.append(c)
        print(json.dumps({k: c[k] for k in c if k.endswith("_ms") or k.endswith("_median") or k in ("n", "n_traj", "n_cells", "n_visits")}))
    doc = {"what": "geohip_traj_group_flags + geohip_tagg_cells against geohip_traj_group + geohip_tstats, one window, "
                   "device events on the ctx stream",
           "library": _abi.version(), "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "cases": cases}
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
