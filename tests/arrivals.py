"""Arrival orders for the parity tests (tests/test_arrivals.py, tests/test_gpu_arrival.py).

Every other GPU test builds its window in shuffled arrival order.  The streaming kernels keep
running bounds (knn_pass), per-wave stages (range_set, ppoly_stream, join_bin) and reservation
cursors, so which of their code runs depends on WHERE in the window the interesting points sit,
not only on which points they are: a trajectory stream delivers runs of nearby points, a
keyBy(gridID) upstream a window sorted by cell.  The orders below are permutations p of a given
window: the caller takes x[p], y[p] (and any side columns) and hands the oracle the permuted
arrays, so expected results need no mapping.

The second half restates the launch geometry on the host (blocks, chunks, waves of an index), so a
test can assert that its window reaches the shape it names before it trusts a comparison.  Each
mirror cites the function it restates; csrc/ paths are below spatialflink_amd/.

Plain helpers, no fixtures.
"""
import numpy as np

import cref

# ------------------------------------------------------------------------------------------
# oracle-side keys
# ------------------------------------------------------------------------------------------


def cells(cg, x, y):
    """(cx, cy) of every point: the arithmetic of the oracle's cell (geohip_oracle_cell: floor((v -
    min) / l), JLS 5.1.3 conversion), vectorised; NaN -> 0 as (int) NaN.  tests/test_arrivals.py
    holds it against cref.cell."""
    out = []
    with np.errstate(invalid="ignore"):
        for v, mn in ((x, cg.min_x), (y, cg.min_y)):
            q = np.floor((np.asarray(v, np.float64) - mn) / cg.cell_len)
            q = np.where(np.isnan(q), 0.0, np.clip(q, -2147483648.0, 2147483647.0))
            out.append(q.astype(np.int64))
    return out[0], out[1]


def oracle_order(cg, x, y, q, r):
    """(order, dist): the oracle's kNN candidates of q in ascending (distance bits, index) order
    (cref.knn_pp at k = n, on one thread: its per-thread heaps hold k entries each) and their
    distances.  Points outside the candidate cells (NaN points among them) are not listed."""
    t = cref.threads()
    cref.set_threads(1)
    try:
        oi, od = cref.knn_pp(cg, x, y, q[0], q[1], r, max(len(x), 1))
    finally:
        cref.set_threads(t)
    return oi.astype(np.int64), od


def _rest(n, listed):
    m = np.ones(n, bool)
    m[listed] = False
    return np.flatnonzero(m)


# ------------------------------------------------------------------------------------------
# orders: each returns an int64 permutation of range(n)
# ------------------------------------------------------------------------------------------


def shuffled(n, seed):
    """The control: what every other test does."""
    return np.random.default_rng(seed).permutation(n).astype(np.int64)


def near_first(n, order):
    """Ascending oracle distance (order: oracle_order's), the unlisted points after them."""
    return np.concatenate([order, _rest(n, order)])


def far_first(n, order):
    """Descending oracle distance; the unlisted points come first, so the nearest point is the
    window's last and the k nearest end in the partial last iteration."""
    return np.concatenate([_rest(n, order), order[::-1]])


def cell_sorted(cx, cy, reverse=False):
    """Row-major by cell (cx major), arrival order kept inside a cell: a keyBy(gridID) upstream."""
    p = np.lexsort((cy, cx)).astype(np.int64)
    return p[::-1].copy() if reverse else p


def cell_sorted_rev(cx, cy):
    return cell_sorted(cx, cy, reverse=True)


def hits_first(n, hits):
    """The oracle's range hits as one run at the head."""
    hits = np.asarray(hits, np.int64)
    return np.concatenate([hits, _rest(n, hits)])


def hits_last(n, hits):
    """The oracle's range hits as one run at the tail (it ends in the partial last iteration)."""
    hits = np.asarray(hits, np.int64)
    return np.concatenate([_rest(n, hits), hits])


def sawtooth(n, order, it=256):
    """Ascending distance across the 256-point iterations, descending within each (every point of
    an iteration beats the bound the iteration started with); unlisted points last."""
    p = near_first(n, order)
    m = len(order)
    out = p.copy()
    for s in range(0, m, it):
        out[s:min(s + it, m)] = p[s:min(s + it, m)][::-1]
    return out


def runs(x, y, cx, cy, seed, max_len=2000):
    """Trajectory-like: the window cut into runs of 1..max_len spatially adjacent points (slices
    of the cell-sorted order), each run a short walk (its points ordered along a random direction
    from a start point), the runs in random order."""
    rng = np.random.default_rng(seed)
    base = cell_sorted(cx, cy)
    n = len(base)
    cuts = [0]
    while cuts[-1] < n:
        cuts.append(min(n, cuts[-1] + int(rng.integers(1, max_len + 1))))
    pieces = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        s = base[a:b]
        th = rng.uniform(0, 2 * np.pi)
        with np.errstate(invalid="ignore"):
            key = np.nan_to_num(np.cos(th) * x[s] + np.sin(th) * y[s])
        pieces.append(s[np.argsort(key, kind="stable")])
    return np.concatenate([pieces[j] for j in rng.permutation(len(pieces))]) if pieces else base


def place(n, groups, seed):
    """A permutation that puts index set groups[j][0] on the window positions groups[j][1] (equal
    lengths, positions disjoint) and every other index on the remaining positions in shuffled
    order."""
    rng = np.random.default_rng(seed)
    p = np.full(n, -1, np.int64)
    used = np.zeros(n, bool)
    for idx, pos in groups:
        idx, pos = np.asarray(idx, np.int64), np.asarray(pos, np.int64)
        assert len(idx) == len(pos) and not used[idx].any() and (p[pos] < 0).all()
        p[pos] = idx
        used[idx] = True
    free = np.flatnonzero(p < 0)
    p[free] = rng.permutation(np.flatnonzero(~used))
    return p


def spread(slots, m):
    """m of the positions ``slots``, evenly spaced over them (several iterations and waves)."""
    assert m <= len(slots)
    return slots[(np.arange(m) * len(slots)) // max(m, 1)]


def in_block(n, chosen, blk, b, seed):
    """``chosen`` placed on the slots of one knn_pass block (positions i with blk[i] == b, blk from
    knn_block_of), as many of them as the block has slots (nearest first); the rest shuffled."""
    slots = np.flatnonzero(blk == b)
    m = min(len(chosen), len(slots))
    return place(n, [(chosen[:m], spread(slots, m))], seed)


def is_permutation(p, n):
    p = np.asarray(p)
    return len(p) == n and np.array_equal(np.sort(p), np.arange(n))


# ------------------------------------------------------------------------------------------
# host mirrors of the launch geometry
# ------------------------------------------------------------------------------------------
PTS_ITER = 256          # device_common.h kPtsIter: points per wave iteration
PASS_MAX_BLOCKS = 256   # csrc/pp_kernels.hip kPassMaxBlocks
PASS_HEADS = 8          # kPassHeads
PASS_CAP = 192 * 16     # PassBlock<kPassNW>::kCap: survivors a block keeps in LDS
STAGE_PTS = 1 << 20     # csrc/abi.cpp kStagePts: a host window's staging chunk


def knn_pass_geometry(n):
    """(nblocks, chunk) of knn_pass_geometry (csrc/pp_kernels.hip)."""
    c = (n + PASS_MAX_BLOCKS - 1) // PASS_MAX_BLOCKS
    c = (c + PTS_ITER - 1) // PTS_ITER * PTS_ITER
    c = max(c, 1024)
    return (n + c - 1) // c, c


def knn_block_of(n, fused_ordered=False, host=False):
    """Block of every window index in knn_pass.  The kNN alone and the unordered fused range sweep
    the window in interleaved fronts: iteration i // 256 belongs to block (i // 256) % nblocks
    (knn_pass: ``kInterleave``).  The ordered fused range keeps a contiguous chunk per block (block
    i // chunk).  host: a pageable window above one staging chunk runs one pass per 2^20-point
    chunk (knn_host_pipelined, csrc/abi.cpp); its blocks are numbered 256 * pass + block."""
    i = np.arange(n, dtype=np.int64)
    if host and n > STAGE_PTS:
        out = np.empty(n, np.int64)
        for p, s in enumerate(range(0, n, STAGE_PTS)):
            m = min(STAGE_PTS, n - s)
            out[s:s + m] = PASS_MAX_BLOCKS * p + knn_block_of(m, fused_ordered)
        return out
    nb, c = knn_pass_geometry(n)
    return i // c if fused_ordered else (i // PTS_ITER) % nb


RANGE_UNIT = 1024       # kUnitPts: one wave's unit of range_fused
RANGE_MAX_BLOCKS = 256  # kRangeMaxBlocks


def range_fused_geometry(n):
    """(nblocks, points per block) of launch_range's one-kernel form (csrc/pp_kernels.hip): blocks
    of upb = ceil(units / 256) contiguous 1024-point units."""
    units = (n + RANGE_UNIT - 1) // RANGE_UNIT
    upb = (units + RANGE_MAX_BLOCKS - 1) // RANGE_MAX_BLOCKS
    return (units + upb - 1) // upb, upb * RANGE_UNIT


SET_NW = 16     # kSetNW: waves per range_set block
SET_RUN = 1024  # kSetRun: hits of one early reservation
SET_BUF = 1408  # kSetBuf: a wave's hit buffer
SET_CAND = 64   # staged band candidates are flushed, 64 at a time, when they reach 64


def range_set_geometry(n, cus):
    """(nblocks, waves W, iterations) of launch_range_set (csrc/pp_kernels.hip): one 16-wave block
    per CU, fewer for small windows; wave gw takes iterations gw, gw + W, ..."""
    iters = (n + PTS_ITER - 1) // PTS_ITER
    nb = min((iters + SET_NW - 1) // SET_NW, cus)
    return nb, nb * SET_NW, iters


def range_set_wave_of(n, cus):
    """Wave (block * 16 + wave in block) of every window index in range_set."""
    _, W, _ = range_set_geometry(n, cus)
    return (np.arange(n, dtype=np.int64) // PTS_ITER) % W


def range_set_wave_trace(kind_of_iteration):
    """range_set's per-wave bookkeeping replayed on the host for one wave.  kind_of_iteration: per
    iteration of the wave, in order, an array of its points' kinds in slot order (four 64-point
    slots): 0 miss, 1 direct hit (guaranteed box, or below the lower squared screen), 2 a point of
    the exact-distance band that the oracle finds inside the circle.  Returns (largest buffer
    fill at a check, early reservations, staged candidates before each iteration, buffered hits
    before each iteration)."""
    hc = cc = peak = early = 0
    staged, held = [], []
    for kinds in kind_of_iteration:
        staged.append(cc)
        held.append(hc)
        for s in range(0, len(kinds), 64):
            k = np.asarray(kinds[s:s + 64])
            hc += int((k == 1).sum())
            cc += int((k == 2).sum())
            if cc >= SET_CAND:       # cand_flush: the newest 64
                cc -= 64
                hc += 64
        peak = max(peak, hc)
        assert hc <= SET_BUF
        if hc >= SET_RUN:
            early += 1
            hc -= SET_RUN
    return peak, early, staged, held


STREAM_CHUNK = 4096          # csrc/cell_kernels.hip kStreamChunk: points per ppoly_stream chunk
STREAM_FIRST_CCAP = 65536    # ppoly_impl: a fresh context's candidate buffer, max(65536, n / 16, ...)


def ppoly_chunk_of(n):
    """ppoly_stream chunk of every window index."""
    return np.arange(n, dtype=np.int64) // STREAM_CHUNK


def ppoly_first_ccap(n):
    return max(STREAM_FIRST_CCAP, n // 16)


def ppoly_candidates_lower_bound(cg, x, y, pairs, npoly, upto=None):
    """A lower bound on the (point, polygon) candidates ppoly_stream stages for points [0, upto):
    the stream decides a C entry by the class of the point's subcell (a quarter of a cell per axis,
    csrc/cell_kernels.hip "4 x 4 split") and stages it as a candidate when that class is mixed.  A
    subcell that holds, among the window's points, both a point the oracle pairs with polygon p
    and one it does not can have no uniform class for p, so every window point in it is a candidate
    for p.  pairs: the oracle's (polygon, point) pairs.  Points within 2^-20 of a subcell edge are
    left out (the host quotient may round across it)."""
    n = len(x)
    upto = n if upto is None else upto
    with np.errstate(invalid="ignore"):
        fx = (np.asarray(x) - cg.min_x) / (cg.cell_len / 4)
        fy = (np.asarray(y) - cg.min_y) / (cg.cell_len / 4)
    ok = np.isfinite(fx) & np.isfinite(fy)
    sx, sy = np.floor(np.where(ok, fx, 0.0)), np.floor(np.where(ok, fy, 0.0))
    ok &= (sx >= 0) & (sx < 4 * cg.n) & (sy >= 0) & (sy < 4 * cg.n)
    for f, s in ((fx, sx), (fy, sy)):
        with np.errstate(invalid="ignore"):
            ok &= (f - s > 2.0 ** -20) & (s + 1 - f > 2.0 ** -20)
    sub = (sx * (4 * cg.n) + sy).astype(np.int64)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    total = 0
    for p in range(npoly):
        hit = np.zeros(n, bool)
        hit[pairs[pairs[:, 0] == p, 1]] = True
        if not hit.any():
            continue
        hs = np.unique(sub[ok & hit])
        ms = np.unique(sub[ok & ~hit])
        mixed = np.intersect1d(hs, ms)
        total += int(np.isin(sub[:upto][ok[:upto]], mixed).sum())
    return total


# ------------------------------------------------------------------------------------------
# the windows of tests/test_gpu_arrival.py (built here so that tests/test_arrivals.py can hold
# their shape conditions on the CPU, with the oracle alone)
# ------------------------------------------------------------------------------------------
from functools import lru_cache  # noqa: E402

from spatialflink_amd import synth  # noqa: E402

BJ = synth.BEIJING
Q = synth.README_QUERY
KNN_GRID, KNN_R = 100, 0.5
KNN_SIZES = (1_200_003, 70_001, 4_097)
KNN_KS = (1, 50, 256, 257, 1000, 1025)   # 1025: the first k of the large-k form
KNN_SHAPES = ("far_first", "near_first", "block_first", "block_last", "halves", "nines", "sawtooth", "cell_sorted")
N_NAN = 10


def cgrid(nb):
    return cref.grid(BJ[0], BJ[2], (BJ[1] - BJ[0]) / nb, nb)


@lru_cache(maxsize=None)
def knn_base(n):
    """n points, all but N_NAN NaN ones inside the candidate cells of (Q, r = 0.5) on the 100-cell
    grid: (x, y, oracle order, oracle distances).  No point coincides with Q."""
    rng = np.random.default_rng(7000 + n)
    x = rng.uniform(Q[0] - 0.4, Q[0] + 0.4, n)
    y = rng.uniform(BJ[2] + 0.02, Q[1] + 0.43, n)
    at = (np.arange(N_NAN) * (n // N_NAN)) + 3
    x[at[::2]] = np.nan
    y[at[1::2]] = np.nan
    order, dist = oracle_order(cgrid(KNN_GRID), x, y, Q, KNN_R)
    # a NaN y reads as cell row 0, a candidate row here: those five are candidates, at the distance
    # the oracle gives a NaN coordinate (Double.MAX_VALUE); a NaN x reads as column 0, no candidate
    assert len(order) == n - N_NAN // 2 and int((dist < 1e300).sum()) == n - N_NAN
    assert dist[0] > 0 and len(np.unique(dist[:2048])) == 2048
    for a in (x, y, order, dist):
        a.setflags(write=False)
    return x, y, order, dist


def knn_perm(n, shape, k, seed=5):
    """The arrival order of one kNN case; the shapes that place the k nearest depend on k."""
    x, y, order, _ = knn_base(n)
    blk = knn_block_of(n)
    nb = int(blk.max()) + 1
    near = order[:k]
    if shape == "shuffled":
        return shuffled(n, seed)
    if shape == "far_first":
        return far_first(n, order)
    if shape == "near_first":
        return near_first(n, order)
    if shape == "sawtooth":
        return sawtooth(n, order)
    if shape == "cell_sorted":
        return cell_sorted(*cells(cgrid(KNN_GRID), x, y))
    if shape == "block_first":
        return in_block(n, near, blk, 0, seed)
    if shape == "block_last":
        return in_block(n, near, blk, nb - 1, seed)
    if shape == "halves":   # half and half over two blocks
        h = (len(near) + 1) // 2
        b1, b2 = nb // 3, (2 * nb) // 3
        s1, s2 = np.flatnonzero(blk == b1), np.flatnonzero(blk == b2)
        return place(n, [(near[:h], spread(s1, h)), (near[h:], spread(s2, len(near) - h))], seed)
    if shape == "nines":    # 9 of the k nearest per block, over ceil(k / 9) blocks (all of them when fewer)
        groups = []
        tgt = (np.arange(len(near)) // 9) % nb
        for b in np.unique(tgt):
            idx = near[tgt == b]
            groups.append((idx, spread(np.flatnonzero(blk == b), len(idx))))
        return place(n, groups, seed)
    raise ValueError(shape)


def per_block(blk, idx):
    """Counts of the window positions idx per block of the map blk."""
    return np.bincount(blk[np.asarray(idx, np.int64)], minlength=int(blk.max()) + 1)


def knn_shape_ok(n, shape, k, wi, wd, x, y):
    """The host-side condition of a kNN case, from the oracle's result (wi, wd) on the arrival-
    ordered window: (holds, figures)."""
    blk = knn_block_of(n)
    nb = int(blk.max()) + 1
    c = per_block(blk, wi)
    kk = len(wi)
    distinct = len(np.unique(wd)) == kk and wd[0] > 0
    slots = np.bincount(blk, minlength=nb)
    if shape in ("near_first", "block_first", "block_last"):
        b = {"near_first": int(blk[wi[0]]), "block_first": 0, "block_last": nb - 1}[shape]
        want = min(kk, int(slots[b])) if shape != "near_first" else None
        if shape == "near_first":   # the first k arrivals: one block while k <= 256, else consecutive blocks
            ok = distinct and (c.max() == kk if kk <= PTS_ITER else c.max() >= PTS_ITER)
        else:
            ok = distinct and c[b] == want and (want == kk or want == slots[b])
        ok = ok and (kk > PASS_HEADS) == (c.max() > PASS_HEADS)
        return ok, {"in_block": int(c.max()), "blocks": int((c > 0).sum())}
    if shape == "halves":
        top = np.sort(c)[::-1]
        ok = distinct and (kk < 2 or (top[0] + top[1] == kk and top[0] - top[1] <= 1))
        ok = ok and (kk < 18 or top[1] > PASS_HEADS)
        return ok, {"halves": top[:2].tolist()}
    if shape == "nines":
        used = c[c > 0]
        ok = distinct and len(used) == min(nb, (kk + 8) // 9) and (kk < 9 or used.max() >= 9)
        ok = ok and (kk <= 9 * nb) == (used.max() <= 9)
        return ok, {"blocks": len(used), "most": int(used.max())}
    if shape == "far_first":
        # descending distance: every candidate is at or below anything seen before it, so it
        # passes the block's running bound whatever that bound is; the block's survivors are its
        # candidates
        cand = np.flatnonzero(np.isfinite(x) & np.isfinite(y))
        with np.errstate(invalid="ignore"):
            d = np.hypot(x[cand] - Q[0], y[cand] - Q[1])
        surv = per_block(blk, cand)
        ok = bool((np.diff(d) <= 0).all()) and wi[0] == n - 1
        return ok, {"survivors_most": int(surv.max()), "spills": bool(surv.max() > PASS_CAP)}
    if shape == "sawtooth":
        with np.errstate(invalid="ignore"):
            d = np.hypot(x - Q[0], y - Q[1])[:n - N_NAN]
        full = (len(d) // PTS_ITER) * PTS_ITER
        it = d[:full].reshape(-1, PTS_ITER)
        ok = bool((np.diff(it, axis=1) <= 0).all() and (it[1:, -1] >= it[:-1, 0]).all())
        return ok, {"iterations": len(it)}
    if shape == "cell_sorted":
        cx, cy = cells(cgrid(KNN_GRID), x, y)
        key = cx * 100000 + cy
        return bool((np.diff(key) >= 0).all()), {"cells": int(len(np.unique(key)))}
    if shape == "shuffled":
        return False, {"in_block": int(c.max())}
    raise ValueError(shape)


@lru_cache(maxsize=None)
def shell_window(dense):
    """test_knn_equal_distance_shell's window (200000 points over the grid plus 50000 on (almost)
    one circle of radius 0.03 about Q), or, dense, knn_base(1200003) with 50000 of its points moved
    to a circle of radius 0.001: there the circle lies among the 64 nearest and the window is large
    enough for a block to spill.  Returned in far_first order."""
    rng = np.random.default_rng(13)
    th = rng.uniform(0, 2 * np.pi, 50000)
    if dense:
        x, y, _, _ = knn_base(KNN_SIZES[0])
        x, y = x.copy(), y.copy()
        at = np.flatnonzero(np.isfinite(x) & np.isfinite(y))[1000:51000]
        rad = 0.001 + rng.integers(-3, 4, 50000) * 1e-17
        x[at] = Q[0] + rad * np.cos(th)
        y[at] = Q[1] + rad * np.sin(th)
    else:
        rad = 0.03 + rng.integers(-3, 4, 50000) * 1e-17
        bx = rng.uniform(BJ[0] - 0.1, BJ[1] + 0.1, 200000)
        by = rng.uniform(BJ[2] - 0.1, BJ[3] + 0.1, 200000)
        x = np.concatenate([bx, Q[0] + rad * np.cos(th)])
        y = np.concatenate([by, Q[1] + rad * np.sin(th)])
    order, _ = oracle_order(cgrid(KNN_GRID), x, y, Q, KNN_R)
    p = far_first(len(x), order)
    return x[p], y[p]


# ---- range ----------------------------------------------------------------------------------
RANGE_SIZES = (300_000, 70_001)
RANGE_SHAPES = ("hits_first", "hits_last", "alternating", "straddle")


@lru_cache(maxsize=None)
def range_base(n, approximate):
    """test_gpu_parity's window (uniform over the grid widened by 0.1, NaN points) and the oracle's
    hits for (Q, r = 0.5) on the 100-cell grid."""
    rng = np.random.default_rng(8000 + n)
    x = rng.uniform(BJ[0] - 0.1, BJ[1] + 0.1, n)
    y = rng.uniform(BJ[2] - 0.1, BJ[3] + 0.1, n)
    x[::997] = np.nan
    y[3::997] = np.nan
    hits = cref.range_pp(cgrid(100), x, y, Q[0], Q[1], 0.5, approximate).astype(np.int64)
    for a in (x, y, hits):
        a.setflags(write=False)
    return x, y, hits


def range_perm(n, shape, approximate, seed=9):
    x, y, hits = range_base(n, approximate)
    _, bp = range_fused_geometry(n)
    if shape == "shuffled":
        return shuffled(n, seed)
    if shape == "hits_first":
        return hits_first(n, hits)
    if shape == "hits_last":
        return hits_last(n, hits)
    if shape == "alternating":  # all-hit and no-hit block chunks in turn, while the hits last
        full = len(hits) // bp
        pos = np.concatenate([np.arange(2 * c * bp, (2 * c + 1) * bp) for c in range(full)])
        miss = _rest(n, hits)
        odd = np.concatenate([np.arange((2 * c + 1) * bp, (2 * c + 2) * bp) for c in range(full)])
        return place(n, [(hits[:len(pos)], pos), (miss[:len(odd)], odd)], seed)
    if shape == "straddle":     # one all-hit 1024-point unit across a block boundary
        b = 3 * bp
        return place(n, [(hits[:RANGE_UNIT], np.arange(b - RANGE_UNIT // 2, b + RANGE_UNIT // 2))], seed)
    raise ValueError(shape)


def range_shape_ok(n, shape, want):
    """want: the oracle's ascending hits on the arrival-ordered window."""
    nb, bp = range_fused_geometry(n)
    hit = np.zeros(n, bool)
    hit[want] = True
    per = np.add.reduceat(hit.astype(np.int64), np.arange(0, n, bp))
    size = np.diff(np.r_[np.arange(0, n, bp), n])
    m = len(want)
    if shape == "hits_first":
        return bool(hit[:m].all()), {"all_hit_blocks": int((per == size).sum())}
    if shape == "hits_last":
        return bool(hit[n - m:].all()) and n % PTS_ITER != 0, {"all_hit_blocks": int((per == size).sum())}
    if shape == "alternating":
        full = m // bp
        ok = full >= 3 and all(per[2 * c] == bp and per[2 * c + 1] == 0 for c in range(full))
        return ok, {"alternations": full}
    if shape == "straddle":
        b = 3 * bp
        ok = bool(hit[b - 512:b + 512].all()) and 0 < per[2] < bp and 0 < per[3] < bp
        return ok, {"boundary": b}
    if shape == "shuffled":
        return False, {"all_hit_blocks": int((per == size).sum())}
    raise ValueError(shape)


SET_N = 5 * (1 << 20) + 77
SET_BAND_GRID, SET_BAND_R = 100, 0.5


def set_band_points(m, seed=3):
    """m points of the exact-distance band of (Q, r = 0.5) that the oracle finds inside the circle:
    on the circle's upper arc (inside the grid), x or y moved by -2..+2 ulp as frames.window moves
    them, kept where the oracle's distance is <= r and within 2^-45 r of it (the kernels' squared
    screens decide only outside 2^-41 r)."""
    import frames
    rng = np.random.default_rng(seed)
    r = SET_BAND_R
    th = rng.uniform(0.4, 2.7, 64 * m)
    du = rng.integers(-2, 3, len(th))
    on_x = rng.integers(0, 2, len(th)) == 0
    bx = frames.ulp_shift(Q[0] + r * np.cos(th), np.where(on_x, du, 0))
    by = frames.ulp_shift(Q[1] + r * np.sin(th), np.where(on_x, 0, du))
    keep = []
    for j in np.flatnonzero(np.abs(np.hypot(bx - Q[0], by - Q[1]) - r) <= r * 2.0 ** -46):
        d = cref.hypot(Q[0] - bx[j], Q[1] - by[j])
        if d <= r and r - d <= r * 2.0 ** -45:
            keep.append(j)
            if len(keep) == m:
                break
    assert len(keep) == m
    return bx[keep], by[keep]


def set_crafted_window(cus):
    """The buffer-bound window of range_set (SET_N points, 100-cell grid, r = 0.5): every point a
    direct hit (inside the guaranteed box) except in two waves.
      wave A (five iterations): 961 direct hits and 63 band points in its first four iterations,
        one band point and 255 direct hits in the fifth -- the fill at that check is
        961 + 64 + 255 = 1280, the most a wave of this window can hold (four iterations bring 1024
        points, so 1023 buffered hits and 63 staged band points cannot both precede a fifth);
      wave 0 (six iterations, the last one the window's 77-point tail): 1023 direct hits, 63 band
        points and 194 misses in five iterations, never 1024 hits at a check, then one band point
        and 76 direct hits in the tail: 1023 + 64 + 76 = 1163.
    Returns (x, y, wave A, kinds) with kinds[i] = 0 miss, 1 direct hit, 2 band point."""
    n = SET_N
    rng = np.random.default_rng(21)
    nb, W, iters = range_set_geometry(n, cus)
    assert iters == 5 * W + 1, "the layout is written for 5 W + 1 iterations (256 CUs)"
    x = rng.uniform(Q[0] - 0.3, Q[0] + 0.3, n)
    y = rng.uniform(Q[1] - 0.29, Q[1] + 0.3, n)
    kinds = np.ones(n, np.int8)
    bx, by = set_band_points(128)
    wa = W // 2 + 5
    its = lambda w: [w + j * W for j in range((iters - w + W - 1) // W)]  # noqa: E731
    used = 0

    def put_band(pos):
        nonlocal used
        x[pos], y[pos] = bx[used:used + len(pos)], by[used:used + len(pos)]
        kinds[pos] = 2
        used += len(pos)
    ia = its(wa)
    assert len(ia) == 5
    for j, it in enumerate(ia[:4]):     # 16 + 16 + 16 + 15 band points, spread over the four slots
        put_band(it * PTS_ITER + np.arange(16 if j < 3 else 15) * 16 + j)
    put_band(np.array([ia[4] * PTS_ITER + 100]))
    i0 = its(0)
    assert len(i0) == 6 and n - i0[5] * PTS_ITER == 77
    for j, it in enumerate(i0[:5]):     # 13 + 13 + 13 + 12 + 12 band points, 39 + 39 + 39 + 39 + 38 misses
        put_band(it * PTS_ITER + np.arange(13 if j < 3 else 12) * 18 + 1)   # odd offsets
        miss = it * PTS_ITER + np.arange(39 if j < 4 else 38) * 6 + 2        # even offsets
        x[miss], y[miss] = BJ[1] - 0.05, BJ[3] - 0.05   # far outside the candidate box
        kinds[miss] = 0
    put_band(np.array([i0[5] * PTS_ITER + 40]))
    return x, y, wa, kinds


def set_wave_kinds(kinds, n, cus, w):
    """Per iteration of wave w, its points' kinds in slot order: slot s of lane l holds point
    base + (s >> 1) * 128 + 2 l + (s & 1) (slot_index, csrc/pp_kernels.hip); points past the
    window's end count as misses."""
    _, W, iters = range_set_geometry(n, cus)
    lane = np.arange(64)
    off = np.concatenate([(s >> 1) * 128 + 2 * lane + (s & 1) for s in range(4)])
    out = []
    for it in range(w, iters, W):
        k = np.zeros(PTS_ITER, np.int8)
        m = min(n, (it + 1) * PTS_ITER) - it * PTS_ITER
        k[:m] = kinds[it * PTS_ITER:it * PTS_ITER + m]
        out.append(k[off])
    return out


# ---- join -----------------------------------------------------------------------------------
JOIN_GRID, JOIN_R = 500, 0.005
JOIN_DATA_ORDERS = ("cell_sorted", "cell_sorted_rev", "runs")
JOIN_QUERY_ORDERS = ("shuffled", "cell_sorted")


@lru_cache(maxsize=None)
def join_base():
    """300000 data points in tight Gaussian clusters (sigma 0.005: tiles of thousands of points on
    the 500-cell grid) and 2000 queries around the same centres."""
    dx, dy = synth.gaussian_clusters(300_000, 11, sigma=0.005)
    qx, qy = synth.gaussian_clusters(2000, 21, sigma=0.02)
    for a in (dx, dy, qx, qy):
        a.setflags(write=False)
    return dx, dy, qx, qy


def order_perm(name, x, y, cg, seed=4):
    cx, cy = cells(cg, x, y)
    if name == "shuffled":
        return shuffled(len(x), seed)
    if name == "cell_sorted":
        return cell_sorted(cx, cy)
    if name == "cell_sorted_rev":
        return cell_sorted_rev(cx, cy)
    if name == "runs":
        return runs(x, y, cx, cy, seed)
    raise ValueError(name)


# ---- point-polygon ----------------------------------------------------------------------------
PPOLY_GRID, PPOLY_R, PPOLY_N = 500, 0.005, 200_000
PPOLY_SETS = ("stars3", "stars40", "holed")
PPOLY_ORDERS = ("cell_sorted", "runs", "inside_first")


@lru_cache(maxsize=None)
def ppoly_polygons(name):
    """(poly_rings or None, ring_off, vx, vy)."""
    if name == "stars3":
        return (None,) + synth.star_polygons(3, 31)
    if name == "stars40":
        return (None,) + synth.star_polygons(40, 32)
    if name == "holed":
        return synth.holed_polygons(12, 33)[:4]
    raise ValueError(name)


@lru_cache(maxsize=None)
def ppoly_base(name):
    """PPOLY_N points: uniform over the grid, 30000 of them drawn around the polygons' boxes (so
    that every polygon has hundreds of points inside, within r and just outside), two NaN points."""
    pr, off, vx, vy = ppoly_polygons(name)
    rng = np.random.default_rng(34)
    npoly = (len(pr) if pr is not None else len(off)) - 1
    x, y = synth.uniform(PPOLY_N, 35)
    x, y = x.copy(), y.copy()
    per = 30000 // npoly
    for p in range(npoly):
        a, b = (int(off[p]), int(off[p + 1])) if pr is None else (int(off[pr[p]]), int(off[pr[p + 1]]))
        lo_x, hi_x, lo_y, hi_y = vx[a:b].min(), vx[a:b].max(), vy[a:b].min(), vy[a:b].max()
        s = 1000 + p * per
        x[s:s + per] = rng.uniform(lo_x - 3 * PPOLY_R, hi_x + 3 * PPOLY_R, per)
        y[s:s + per] = rng.uniform(lo_y - 3 * PPOLY_R, hi_y + 3 * PPOLY_R, per)
    x[7], y[11] = np.nan, np.nan
    p = shuffled(PPOLY_N, 36)
    x, y = x[p], y[p]
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def ppoly_perm(name, order):
    x, y = ppoly_base(name)
    cg = cgrid(PPOLY_GRID)
    if order == "inside_first":     # the oracle's hits as one run
        pr, off, vx, vy = ppoly_polygons(name)
        pairs = cref.range_ppoly(cg, x, y, off, vx, vy, PPOLY_R, False, pr)
        return hits_first(len(x), np.unique(pairs[:, 1].astype(np.int64)))
    return order_perm(order, x, y, cg)


def chunk_share(n, pts, chunk=STREAM_CHUNK):
    """Per ppoly_stream chunk, the share of its points that are in pts."""
    hit = np.zeros(n, bool)
    hit[np.asarray(pts, np.int64)] = True
    starts = np.arange(0, n, chunk)
    return np.add.reduceat(hit.astype(np.int64), starts) / np.diff(np.r_[starts, n])


def chunk_cells(cx, cy, chunk=STREAM_CHUNK):
    """Fewest distinct cells among the 4096 points of one full ppoly_stream chunk: the per-wave
    stages fill early only where a chunk's points share cells."""
    key = cx * 100000 + cy
    return min(len(np.unique(key[s:s + chunk])) for s in range(0, len(key) - chunk + 1, chunk))


EDGE_HEAD = 70_000


@lru_cache(maxsize=None)
def ppoly_edge_window():
    """PPOLY_N points whose first EDGE_HEAD, contiguous, lie within r of a ring edge of 40 star
    polygons and are candidates of the exact test: each lies just inside the distance-r curve of a
    polygon and has a twin 0.004 r farther out, in the same subcell, that the oracle does not pair
    with that polygon -- so the subcell has no uniform class (ppoly_candidates_lower_bound).  The
    twins arrive later, shuffled among the points of helpers.edge_window (uniform points, vertices,
    edge midpoints, points around the grid's west edge, NaN points).
    Returns (ring_off, vx, vy, x, y)."""
    from helpers import edge_window
    cg = cgrid(PPOLY_GRID)
    r = PPOLY_R
    _, off, vx, vy = ppoly_polygons("stars40")
    npoly = len(off) - 1
    rng = np.random.default_rng(37)
    e = np.concatenate([np.arange(int(off[p]), int(off[p + 1]) - 1) for p in range(npoly)])
    m = 6 * EDGE_HEAD   # the stars are spiky: about a quarter of the drawn points qualify
    k = e[rng.integers(0, len(e), m)]
    t = rng.uniform(0.02, 0.98, m)
    ax, ay, ex, ey = vx[k], vy[k], vx[k + 1] - vx[k], vy[k + 1] - vy[k]
    L = np.hypot(ex, ey)
    nx, ny = ey / L, -ex / L    # the rings run counter-clockwise: outward
    d = rng.uniform(0.997, 0.9995, m) * r
    hx, hy = ax + t * ex + d * nx, ay + t * ey + d * ny
    tx, ty = hx + 0.004 * r * nx, hy + 0.004 * r * ny
    pairs = cref.range_ppoly(cg, np.concatenate([hx, tx]), np.concatenate([hy, ty]), off, vx, vy, r)
    key = pairs[:, 1].astype(np.int64) * npoly + pairs[:, 0]
    head, twin = key[pairs[:, 1] < m], key[pairs[:, 1] >= m] - m * npoly
    lost = np.setdiff1d(head, twin) // npoly    # points with a polygon their twin has lost
    sub = lambda a, mn: (a - mn) / (cg.cell_len / 4)  # noqa: E731
    good = np.zeros(m, bool)
    good[lost] = True
    for a, b, mn in ((hx, tx, cg.min_x), (hy, ty, cg.min_y)):
        fa, fb = sub(a, mn), sub(b, mn)
        good &= (np.floor(fa) == np.floor(fb)) & (fa - np.floor(fa) > 1e-3) & (fb - np.floor(fb) > 1e-3)
        good &= (np.ceil(fa) - fa > 1e-3) & (np.ceil(fb) - fb > 1e-3)
    sel = np.flatnonzero(good)[:EDGE_HEAD]
    assert len(sel) == EDGE_HEAD
    bx, by = edge_window(PPOLY_N - 2 * EDGE_HEAD - (2 * len(vx) - 1 + 4002), 38, off, vx, vy)
    tail_x, tail_y = np.concatenate([bx, tx[sel]]), np.concatenate([by, ty[sel]])
    p = rng.permutation(len(tail_x))
    x, y = np.concatenate([hx[sel], tail_x[p]]), np.concatenate([hy[sel], tail_y[p]])
    assert len(x) == PPOLY_N
    return off, vx, vy, x, y


def release():
    """Drop the cached windows (some hundred MB): the test modules call it when they are done, so
    the rest of a suite run does not carry them."""
    for f in (knn_base, shell_window, range_base, join_base, ppoly_polygons, ppoly_base, ppoly_edge_window):
        f.cache_clear()


KNN_PPOLY_KS = (1, 50, 256)


def knn_ppoly_perm(x, y, vx, vy, k, chunk, seed=6):
    """The k nearest of the query polygon (oracle) on positions of one 4096-point chunk, the rest
    shuffled.  Points inside the polygon tie at distance 0 and the lowest indices win, so all of
    them go to the chunk with the k nearest."""
    wi, wd = cref.knn_ppoly(cgrid(PPOLY_GRID), x, y, vx, vy, 0.02, STREAM_CHUNK // 2)
    m = max(k, int((wd == 0).sum()))
    n = len(x)
    slots = np.arange(chunk * STREAM_CHUNK, min(n, (chunk + 1) * STREAM_CHUNK))
    assert m < len(wi) and m <= len(slots)
    return place(n, [(wi[:m].astype(np.int64), spread(slots, m))], seed)
