#!/usr/bin/env python3
"""Device time of the trajectory join geohip_tjoin_pp at the C3 shape of bench.py, next to
geohip_join_pp_count_only on the same coordinates in the same process (the yardstick: it decides
the same candidate pairs under the point join's predicate and writes nothing).

    python scripts/tjoin_time.py                                    # 10 M x 10 k points, 100 k x 100 trajectories
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o tjoin -- \\
        python scripts/tjoin_time.py --profiled --out DIR/step.json   # per-kernel run: geohip_tjoin_pp alone
    python scripts/tjoin_time.py --merge DIR --out profiles/tjoin_time.json   # fold the statistics in

The ordinary window is synth.gaussian_clusters(n, 3) and the query window synth.gaussian_clusters(nq, 4)
on the 500 x 500 Beijing grid, r = 0.05, as bench.py's JoinWorkload builds them; objIDs are assigned
at random.  Both windows are uploaded and grouped once (geohip_traj_group); each call is timed with
events on the ctx's stream, the two calls alternating (3 warm-ups, median of 10).  geohip_tjoin_pp
reads back once after its first two kernels and once per probe pass, so its event time holds those
gaps; the per-kernel times come from the profiler run.  The result is checked at this size against
a numpy evaluation over the binned cells (the ordinary window sorted by cell, each query point
against the contiguous span of every column of its square; separate multiply and add, np.sqrt).
Needs the GPU: there is no other path.
"""
from __future__ import annotations

import argparse
import csv
import json
import math
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

from traj_step import short_name  # noqa: E402

GRID_ROWS, RADIUS, SIGMA = 500, 0.05, 0.1


def digit_ids(labels, width=7):
    """(text uint8, off uint64) of the objIDs "%0<width>d" % label, without a Python string per point."""
    import numpy as np
    v = labels.astype(np.int64)
    text = np.empty((len(v), width), np.uint8)
    for k in range(width - 1, -1, -1):
        text[:, k] = 48 + v % 10
        v = v // 10
    return text.reshape(-1), (np.arange(len(labels) + 1, dtype=np.uint64) * width)


def host_pairs(grid, ax, ay, ta, nta, bx, by, tb, ntb, r, min_points=2):
    """The distinct (ta, tb), ascending, by numpy over the binned cells."""
    import numpy as np
    n, l = grid.n, grid.cell_len
    lc = int(math.ceil(r / l))
    cxa = np.floor((ax - grid.min_x) / l).astype(np.int64)
    cya = np.floor((ay - grid.min_y) / l).astype(np.int64)
    ok = (cxa >= 0) & (cxa < n) & (cya >= 0) & (cya < n) & (np.bincount(ta, minlength=nta)[ta] >= min_points)
    idx = np.flatnonzero(ok)
    key = cxa[idx] * n + cya[idx]
    order = np.argsort(key, kind="stable")
    idx, key = idx[order], key[order]
    sx, sy, st = ax[idx], ay[idx], ta[idx]
    start = np.searchsorted(key, np.arange(n * n + 1))
    cxb = np.floor((bx - grid.min_x) / l).astype(np.int64)
    cyb = np.floor((by - grid.min_y) / l).astype(np.int64)
    ok_b = np.bincount(tb, minlength=ntb)[tb] >= min_points
    hit = np.zeros((ntb, nta), bool)
    point_pairs = 0
    for q in range(len(bx)):
        if not ok_b[q]:
            continue
        y0, y1 = max(cyb[q] - lc, 0), min(cyb[q] + lc, n - 1)
        if y0 > y1:
            continue
        for cx in range(max(cxb[q] - lc, 0), min(cxb[q] + lc, n - 1) + 1):
            a, b = start[cx * n + y0], start[cx * n + y1 + 1]
            if a == b:
                continue
            dy, dx = by[q] - sy[a:b], bx[q] - sx[a:b]
            m = np.sqrt(dy * dy + dx * dx) <= r
            point_pairs += int(m.sum())
            hit[tb[q], st[a:b][m]] = True
    return np.argwhere(hit.T).astype(np.int64), point_pairs


def run(a):
    import numpy as np
    import torch
    from spatialflink_amd import Context, _abi, synth

    ctx = Context(0)  # raises without an MI355X
    bj = synth.BEIJING
    grid = _abi.make_grid(bj[0], bj[2], (bj[1] - bj[0]) / GRID_ROWS, GRID_ROWS)
    ax, ay = synth.gaussian_clusters(a.n, 3, sigma=SIGMA)
    bx, by = synth.gaussian_clusters(a.nq, 4, sigma=SIGMA)
    rng = np.random.default_rng(a.seed)
    la, lb = rng.integers(0, a.traj, a.n), rng.integers(0, a.qtraj, a.nq)
    dev = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).to("cuda:0")  # noqa: E731
    dax, day, dbx, dby = dev(ax, np.float64), dev(ay, np.float64), dev(bx, np.float64), dev(by, np.float64)
    groups = []
    for labels in (la, lb):
        text, off = digit_ids(labels)
        groups.append(ctx.traj_group(dev(text, np.uint8), dev(off.view(np.int64), np.int64)))
    ga, gb = groups
    torch.cuda.synchronize()
    p0 = ctx.debug_tjoin_passes()
    first = ctx.tjoin_pp(grid, dax, day, ga, dbx, dby, gb, RADIUS)
    m = int(first.shape[0])
    passes_first = ctx.debug_tjoin_passes() - p0
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    t_join, t_count = [], []
    pairs = None
    p0 = ctx.debug_tjoin_passes()
    for it in range(a.warmup + a.iters):
        e = [ev() for _ in range(3)]
        e[0].record()
        out = ctx.tjoin_pp(grid, dax, day, ga, dbx, dby, gb, RADIUS, cap=m)
        e[1].record()
        if not a.profiled:
            pairs = ctx.join_pp_count(grid, grid, dax, day, dbx, dby, RADIUS)
        e[2].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            t_join.append(e[0].elapsed_time(e[1]))
            t_count.append(e[1].elapsed_time(e[2]))
    passes = (ctx.debug_tjoin_passes() - p0) / (a.warmup + a.iters)
    assert torch.equal(out, first)
    stat = lambda v: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}  # noqa: E731
    case = {"n": a.n, "nq": a.nq, "n_traj": int(ga["n_traj"]), "nq_traj": int(gb["n_traj"]), "grid_rows": GRID_ROWS,
            "r": RADIUS, "sigma": SIGMA, "warmup": a.warmup, "iters": a.iters, "profiled_run": bool(a.profiled),
            "distinct_pairs": m, "probe_passes_per_call": passes, "probe_passes_first_call": passes_first,
            "tjoin_pp_ms": stat(t_join)}
    if not a.profiled:
        case["join_pp_count_only_ms"] = stat(t_count)
        case["join_pp_point_pairs_hypot"] = int(pairs)
        case["tjoin_over_count_only"] = case["tjoin_pp_ms"]["median"] / case["join_pp_count_only_ms"]["median"]
    if not a.profiled and not a.no_check:
        t0 = time.time()
        want, point_pairs = host_pairs(grid, ax, ay, ga["traj_of"].cpu().numpy().astype(np.int64), int(ga["n_traj"]), bx, by,
                                       gb["traj_of"].cpu().numpy().astype(np.int64), int(gb["n_traj"]), RADIUS)
        got = out.cpu().numpy().astype(np.int64)
        if got.shape != want.shape or not np.array_equal(got, want):
            raise SystemExit(f"tjoin_pp: {len(got)} pairs, numpy has {len(want)}, or they differ")
        case["host_check"] = {"distinct_pairs": int(len(want)), "point_pairs_sqrt": point_pairs, "seconds": time.time() - t0}
    print(json.dumps({k: v for k, v in case.items() if not isinstance(v, dict) or k.endswith("_ms")}))
    doc = {"what": "geohip_tjoin_pp against geohip_join_pp_count_only on the same coordinates, alternating, device events "
                   "on the ctx stream", "library": _abi.version(), "cases": [case]}
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(doc, indent=1) + "\n")


def merge(stats_dir: Path, out: Path):
    """Fold rocprofv3's kernel statistics of the --profiled run into the result file: per kernel its
    calls, total time and time per geohip_tjoin_pp call (the one grouping per window and the first,
    untimed call are in the statistics too: calls counts every geohip_tjoin_pp call)."""
    doc = json.loads(out.read_text())
    files = sorted(stats_dir.rglob("*kernel_stats.csv"))
    side = stats_dir / "step.json"
    if not files or not side.exists():
        raise SystemExit(f"no kernel statistics or step.json under {stats_dir}")
    step = json.loads(side.read_text())["cases"][0]
    calls = step["warmup"] + step["iters"] + 1
    by_name = {}
    with files[0].open() as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            if "geohip::" not in name and "rocprim" not in name and "fillBuffer" not in name:
                continue
            k = by_name.setdefault(short_name(name), {"calls": 0, "total_ms": 0.0})
            k["calls"] += int(row["Calls"])
            k["total_ms"] += int(row["TotalDurationNs"]) / 1e6
    kernels = [{"name": nm, "calls": k["calls"], "total_ms": k["total_ms"], "per_call_ms": k["total_ms"] / calls}
               for nm, k in by_name.items()]
    kernels.sort(key=lambda k: -k["total_ms"])
    doc["cases"][0]["kernels_profiled_run"] = {"tjoin_pp_calls": calls, "groupings": 2,
                                               "tjoin_pp_ms": step["tjoin_pp_ms"],
                                               "kernel_ms_per_call": sum(k["per_call_ms"] for k in kernels),
                                               "kernels": kernels}
    out.write_text(json.dumps(doc, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--traj", type=int, default=100_000)
    ap.add_argument("--qtraj", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--profiled", action="store_true", help="geohip_tjoin_pp alone, no check (the rocprofv3 run)")
    ap.add_argument("--no-check", action="store_true", help="skip the numpy evaluation")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "tjoin_time.json")
    ap.add_argument("--merge", type=Path, default=None, help="directory of the rocprofv3 run to fold into --out")
    a = ap.parse_args()
    if a.merge is not None:
        merge(a.merge, a.out)
        return
    run(a)


if __name__ == "__main__":
    main()
