"""Phase timeline of one kNN pass launch (100 MHz timestamps): per-block start, stream end,
slot bound built (tb: before the block barrier, by the first wave out of the stream loop), flush
(block barrier), stores drained, arrived; the last block's acquire, gather and write, its own
chain from its flush on (last_chain, each phase's length) and which final ran.
Percentiles (0, 10, 50, 90, 100) in microseconds relative to the earliest block start (GPU box
measurement)."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from spatialflink_amd import Context, _abi, synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
K = int(sys.argv[2]) if len(sys.argv) > 2 else 50
R = float(sys.argv[3]) if len(sys.argv) > 3 else 0.5
GN = int(sys.argv[4]) if len(sys.argv) > 4 else 100
ABL = int(sys.argv[5]) if len(sys.argv) > 5 else 0
W = 4
ctx = Context(0)
bj, q = synth.BEIJING, synth.README_QUERY
grid = _abi.make_grid(bj[0], bj[2], (bj[1] - bj[0]) / GN, GN)
xs, ys = [], []
for w in range(W):
    x = torch.empty(n, dtype=torch.float64, device="cuda")
    y = torch.empty(n, dtype=torch.float64, device="cuda")
    ctx.synth_uniform_async(x, y, 0, 2 + 7919 * w, bj)
    xs.append(x)
    ys.append(y)
torch.cuda.synchronize()
names = ["start", "stream_end", "flush", "drained", "arrived"] + (["lookback", "emitted"] if ABL < 0 else [])
blk = {"tb": 14, "hist": 8, "listed": 9, "heads": 10}
fin = {"acquired": 5, "loaded": 11, "T": 12, "taken": 13, "gathered": 6, "written": 7}
out = {}
for rep in range(4):
    for w in range(W):  # warm the path, cycle windows
        ctx.knn_pp(grid, xs[w], ys[w], q[0], q[1], R, K)
    tr = ctx.debug_knn_pass_trace(grid, xs[rep % W], ys[rep % W], q[0], q[1], R, K, ABL).astype(np.int64)
    t0 = tr[:, 0].min()
    rel = (tr - t0) / 100.0
    row = {nm: [round(float(np.percentile(rel[:, j], p)), 2) for p in (0, 10, 50, 90, 100)] for j, nm in enumerate(names)}
    # blocks that reached the stamp (0 = not reached: the slot-complete end stamps 8 and 10 but
    # not 9, the list path all three) -- their median and their number
    row["block_median"] = {nm: (round(float(np.median(rel[tr[:, j] != 0, j])), 2) if (tr[:, j] != 0).any() else None)
                           for nm, j in blk.items()}
    row["blocks_reached"] = {nm: int((tr[:, j] != 0).sum()) for nm, j in blk.items()}
    last = int(np.argmax(tr[:, 7]))
    # (None: not reached -- the direct final stamps no "taken")
    row["final"] = {nm: (round(float(rel[last, j]), 2) if tr[last, j] else None) for nm, j in fin.items()}
    row["last_block"] = last
    # the last block's own dependent chain after its last byte: flush -> record stored (heads) ->
    # drained -> arrived -> acquired -> loaded -> gathered -> written; tb_before_flush: how long
    # before its barrier its slot bound stood
    chain = [("flush", 2), ("heads", 10), ("drained", 3), ("arrived", 4), ("acquired", 5), ("loaded", 11),
             ("gathered", 6), ("written", 7)]
    row["last_chain"] = {f"{a}->{b}": round(float(rel[last, j] - rel[last, i]), 2)
                         for (a, i), (b, j) in zip(chain[:-1], chain[1:])}
    row["last_chain"]["flush->written"] = round(float(rel[last, 7] - rel[last, 2]), 2)
    row["last_chain"]["tb_before_flush"] = round(float(rel[last, 2] - rel[last, 14]), 2) if tr[last, 14] else None
    end = ctx.debug_knn_pass_end()
    row["final_ran"] = {1: "direct", 2: "T"}.get(end, end)
    row["stats"] = ctx.debug_knn_pass_stats()
    out[f"rep{rep}"] = row
print(json.dumps({"shape": dict(n=n, k=K, r=R, grid=GN, ablation=ABL), **out}))
