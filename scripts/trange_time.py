#!/usr/bin/env python3
"""Device time of geohip_trange_classify beside geohip_range_ppoly on the same inputs.

    python scripts/trange_time.py                 # the C4 shape: 50 M uniform points, 1 k star polygons, 500 x 500
    python scripts/trange_time.py --points 200000 --iters 2 --out /tmp/t.json   # a rehearsal size

Both calls see the same window (synth_uniform, seed 5) and the same polygons (synth.star_polygons
(1000, 6)); range_ppoly runs at r = 0.005.  After warm-up calls (the polygon plans are cached by
then) the two are timed alternately, each between device events on torch's current stream -- the
calls end in a count readback, so a call's event time is its whole device step -- and the medians
are reported.  The two answer different questions (strict containment in the polygon set per
point; (polygon, point) pairs within r), so no ratio is a pass condition; the figures go side by
side.  Bytes are the algorithm's: 16 B per point read, 1 B class and 4 B per contained index
written.  Needs the GPU: there is no other path.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_PEAK_BYTES_PER_S = 8.0e12  # MI355X HBM3E spec peak


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--polygons", type=int, default=1000)
    ap.add_argument("--grid", type=int, default=500)
    ap.add_argument("--radius", type=float, default=0.005)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "trange_time.json")
    a = ap.parse_args()

    import numpy as np
    import torch
    from spatialflink_amd import Context, _abi, synth

    ctx = Context(0)  # raises without an MI355X
    bj = synth.BEIJING
    grid = _abi.make_grid(bj[0], bj[2], (bj[1] - bj[0]) / a.grid, a.grid)
    n = a.points
    x = torch.empty(n, dtype=torch.float64, device="cuda:0")
    y = torch.empty(n, dtype=torch.float64, device="cuda:0")
    ctx.synth_uniform_async(x, y, 0, 5, bj)
    off, vx, vy = synth.star_polygons(a.polygons, 6)
    torch.cuda.synchronize()
    pairs = len(ctx.range_ppoly(grid, x, y, off, vx, vy, a.radius))
    out = torch.empty((pairs + 1, 2), dtype=torch.int32, device="cuda:0")
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    t_cls, t_old = [], []
    cls = idx = None
    for it in range(a.warmup + a.iters):
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        cls, idx = ctx.trange_classify(grid, x, y, off, vx, vy)
        e1.record()
        got = ctx.range_ppoly(grid, x, y, off, vx, vy, a.radius, out=out)
        e2.record()
        torch.cuda.synchronize()
        if len(got) != pairs:
            raise SystemExit("range_ppoly: the pair count changed between calls")
        if it >= a.warmup:
            t_cls.append(e0.elapsed_time(e1))
            t_old.append(e1.elapsed_time(e2))
    counts = torch.bincount(cls.to(torch.int64), minlength=3).cpu().tolist()
    if counts[2] != len(idx) or not bool((cls[idx.to(torch.int64)] == 2).all()):
        raise SystemExit("trange_classify: the index list does not match the classes")
    stat = lambda v: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}  # noqa: E731
    nbytes = 16 * n + n + 4 * counts[2]
    med = float(np.median(t_cls))
    doc = {
        "what": "geohip_trange_classify and geohip_range_ppoly on the same window and polygons, timed alternately "
                "between device events (whole calls, their count readbacks included)",
        "library": _abi.version(), "points": n, "polygons": a.polygons, "vertices": int(len(vx)), "grid": a.grid,
        "radius": a.radius, "warmup": a.warmup, "iters": a.iters,
        "trange_classify_ms": stat(t_cls), "range_ppoly_ms": stat(t_old),
        "classes": {"0": counts[0], "1": counts[1], "2": counts[2]}, "range_ppoly_pairs": pairs,
        "trange_algorithmic_bytes": nbytes,
        "trange_bytes_per_s": nbytes / (med * 1e-3),
        "trange_fraction_of_hbm_peak": nbytes / (med * 1e-3) / HBM_PEAK_BYTES_PER_S,
        "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
    }
    print(json.dumps({k: doc[k] for k in ("points", "trange_classify_ms", "range_ppoly_ms", "classes", "range_ppoly_pairs",
                                          "trange_fraction_of_hbm_peak")}))
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
