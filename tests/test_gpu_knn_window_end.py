"""GPU: how knn_pass ends a window -- the blocks' 128-byte records, the direct final and the T path.

After its stream a block publishes one record (its slots, or its list's heads); the last block
ranks the records' entries directly when every block is slot-complete and nothing spilled, and
goes through the heads' histogram and T otherwise (csrc/pp_kernels.hip: knn_pass, pass_final).
Every case compares indices and distance bits with cref.knn_pp (range sets with cref.range_pp) on
the same arrays, never with another GPU path.

Which final a window reaches is asserted from the host where the launch geometry decides it, with
the mirrors of tests/arrivals.py and the oracle's result (``expected_final``):
  * k > 256 turns the slots off, a block that holds more than 8 of the window's k nearest cannot
    be slot-complete, and a block with more candidates in descending order than its 3072-entry
    buffer spills: the T path;
  * k = 1 in a window whose every 256-point iteration holds a candidate: a block's bound T_b is
    at most the upper edge of its own lowest survivor bin as the building wave saw it, that wave
    has run one of the block's iterations, so T_b is at most the edge of the highest of the
    iterations' lowest bins; when every block has at most 8 candidates at or below that, every
    block is slot-complete whatever the order in which blocks and waves finish: the direct final.
Elsewhere (k >= 2 over few iterations per block: a block's T_b then needs k other blocks to have
published before it) the path depends on the order in which blocks finish; the final that ran is
recorded in FIGURES, and what is asserted is what holds either way (``consistent``) and, at the
benchmark's shape, the direct final for k = 50.  Context.debug_knn_pass_end reports the final.

Geometry: up to 262,144 points a block's chunk is 1024 points, nblocks = ceil(n / 1024).
"""
from functools import lru_cache

import numpy as np
import pytest

import arrivals as A
import cref
from spatialflink_amd import Context, _abi, synth
from spatialflink_amd.incremental import IncrementalKNN

pytestmark = pytest.mark.gpu

BJ, Q, R = A.BJ, A.Q, A.KNN_R
DIRECT, TPATH = Context.FINAL_DIRECT, Context.FINAL_T
SIZES = (1, 255, 1_025, 5_000, 262_144, 300_000, 1_200_003)
KS = (1, 50, 256, 257)
FIGURES = {}


def note(key, **fig):
    FIGURES[key] = fig
    print(f"[window end] {key}: {fig}")


def agrid(nb):
    return _abi.make_grid(BJ[0], BJ[2], (BJ[1] - BJ[0]) / nb, nb)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def u32(t):
    return t.cpu().numpy().view(np.uint32) if hasattr(t, "cpu") else np.asarray(t).view(np.uint32)


@pytest.fixture(scope="module", autouse=True)
def _release_windows():
    yield
    A.release()
    base.cache_clear()


@pytest.fixture(scope="module")
def sctx():
    c = Context(0)
    c.set_range_order(True)
    return c


@lru_cache(maxsize=None)
def base(n):
    """n points inside the candidate cells of (Q, r = 0.5) on the 100-cell grid, distinct
    distances among the nearest: (x, y, oracle order, oracle distances)."""
    rng = np.random.default_rng(9100 + n)
    x = rng.uniform(Q[0] - 0.4, Q[0] + 0.4, n)
    y = rng.uniform(BJ[2] + 0.02, Q[1] + 0.43, n)
    order, dist = A.oracle_order(A.cgrid(A.KNN_GRID), x, y, Q, R)
    assert len(order) == n and dist[0] > 1e-6 and len(np.unique(dist[:min(n, 600)])) == min(n, 600)
    for a in (x, y, order, dist):
        a.setflags(write=False)
    return x, y, order, dist


def launch(ctx, ag, tx, ty, k, r=R):
    import torch
    oi = torch.empty(k, dtype=torch.int32, device="cuda")
    od = torch.empty(k, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    ctx.knn_pp_async(ag, tx, ty, Q[0], Q[1], r, k, oi, od, cnt)
    return oi, od, cnt


def check(out, wi, wd, what):
    oi, od, cnt = out
    m = int(cnt.item())
    assert m == len(wi), what
    assert u32(oi[:m]).tolist() == wi.tolist(), what
    assert np.array_equal(od[:m].cpu().numpy().view(np.uint64), wd.view(np.uint64)), what
    assert (oi[m:] == -1).all(), what


def knn_dev(ctx, x, y, k, what, r=R, grid=A.KNN_GRID):
    """One device window against the oracle: (oracle idx, oracle dist, pass stats, final)."""
    import torch
    wi, wd = cref.knn_pp(A.cgrid(grid), x, y, Q[0], Q[1], r, k)
    out = launch(ctx, agrid(grid), dev(x), dev(y), k, r)
    torch.cuda.synchronize()
    check(out, wi, wd, what)
    end = ctx.debug_knn_pass_end()
    stats = ctx.debug_knn_pass_stats()
    consistent(len(x), k, wi, x, y, stats, end, what)
    return wi, wd, stats, end


def consistent(n, k, wi, x, y, stats, end, what):
    """What the host can say about any window, whatever the order in which its blocks finished.
    The direct final needs every block slot-complete: k <= 256, no block holding more than 8 of
    the oracle's k nearest (they all lie at or below any valid T_b), and nothing spilled.  A block
    spills only with more candidates than its buffer holds."""
    blk = A.knn_block_of(n)
    nb = int(blk.max()) + 1
    assert end in (DIRECT, TPATH), (what, end)
    most = int(A.per_block(blk, wi.astype(np.int64)).max()) if len(wi) else 0
    if end == DIRECT:
        assert k <= 256 and most <= A.PASS_HEADS and stats[1] == 0, (what, k, most, stats)
    with np.errstate(invalid="ignore"):
        cand = np.isfinite(x) & np.isfinite(y)
    if A.per_block(blk, np.flatnonzero(cand)).max() <= A.PASS_CAP:
        assert stats[1] == 0, (what, stats)


def dist_bins(d):
    """The survivor histogram's bin of a distance up to the origin: 16 bins per octave of the
    distance bits (hist_bin, csrc/pp_kernels.hip)."""
    return (np.asarray(d, np.float64).view(np.uint64) >> np.uint64(48)).astype(np.int64)


def expected_final(n, k, wi, x, y, order=None):
    """DIRECT / TPATH where the geometry decides the final (module docstring), else None."""
    blk = A.knn_block_of(n)
    nb = int(blk.max()) + 1
    if k > 256:
        return TPATH
    if len(wi) and A.per_block(blk, wi.astype(np.int64)).max() > A.PASS_HEADS:
        return TPATH
    if k != 1 or order is None or len(order) == 0:
        return None
    cand = np.zeros(n, bool)
    cand[order] = True
    with np.errstate(invalid="ignore"):
        b = dist_bins(np.hypot(x - Q[0], y - Q[1]))     # bins need no exact distance: a margin below
    it = np.arange(n) // A.PTS_ITER
    nit = int(it.max()) + 1
    low = np.full(nit, np.iinfo(np.int64).max)
    np.minimum.at(low, it[cand], b[cand])
    if (low == np.iinfo(np.int64).max).any():
        return None     # an iteration without a candidate: its wave may build before any survivor
    worst = np.full(nb, -1)
    np.maximum.at(worst, np.arange(nit) % nb, low)
    at_or_below = np.bincount(blk[cand & (b <= worst[blk] + 1)], minlength=nb)  # + 1: the rounding of hypot
    return DIRECT if at_or_below.max() <= A.PASS_HEADS else None


def assert_final(key, want, end, **fig):
    note(key, expected={DIRECT: "direct", TPATH: "T", None: "either"}[want], ran={DIRECT: "direct", TPATH: "T"}[end],
         **fig)
    if want is not None:
        assert end == want, (key, want, end)


# ------------------------------------------------------------------------------ sizes --------
@pytest.mark.parametrize("n", SIZES)
def test_window_end_sizes(ctx, n):
    """Shuffled uniform windows: 1, 255 (one block, a partial iteration), 1,025 (2 blocks), 5,000
    (5 blocks, partial last iteration), 262,144 (256 blocks of 4 iterations: 12 of a block's 16
    waves never run one), 300,000 (235 blocks) and 1,200,003 points (247 blocks)."""
    x0, y0, order, _ = base(n)
    nb, _ = A.knn_pass_geometry(n)
    assert nb == {1: 1, 255: 1, 1_025: 2, 5_000: 5, 262_144: 256, 300_000: 235, 1_200_003: 247}[n]
    p = A.shuffled(n, 3)
    x, y = x0[p], y0[p]
    inv = np.empty(n, np.int64)
    inv[p] = np.arange(n)
    for k in KS:
        wi, wd, stats, end = knn_dev(ctx, x, y, k, f"n={n} k={k}")
        want = expected_final(n, k, wi, x, y, inv[order])
        if n <= 255 and k == 1:
            assert want == DIRECT   # one block, one iteration: its lowest bin holds at most 8 points
        assert_final(f"shuffled n={n} k={k}", want, end, kept=stats[2], spilled=stats[1])


def test_window_end_many_iterations(ctx):
    """6,500,003 uniform points over the grid: 254 blocks of 99 or 100 iterations, about the smallest
    shape at which blocks publish their lowest bin in mid-stream (the waves claiming iterations niters / 3
    and 2 niters / 3; claims start at iteration 32), so that a block's T_b can exist for k = 50
    and 256 as it does at the benchmark's 10M points -- there the direct final is the common
    case, but not a certain one."""
    n = 6_500_003
    x, y = synth.uniform(n, 93)
    nb = A.knn_pass_geometry(n)[0]
    assert nb == 254 and (-(-n // A.PTS_ITER) // nb) // 3 >= 32
    for k in (50, 256):
        wi, wd, stats, end = knn_dev(ctx, x, y, k, f"n={n} k={k}")
        assert_final(f"uniform n={n} k={k}", expected_final(n, k, wi, x, y), end, kept=stats[2], spilled=stats[1])


@pytest.mark.parametrize("n", [5_000, 262_144])
def test_window_end_direct_by_geometry(ctx, n):
    """One candidate per 256-point iteration (at most 4 per block), every other point outside the
    candidate cells: at k = 1 every block is slot-complete whatever the timing, the direct final;
    the second window puts all candidates on one circle (equal distances up to a few ulp: ties in
    the ranking, 1024 record entries at n = 262,144: above the 64- and 256-entry rank forms)."""
    rng = np.random.default_rng(40 + n)
    nit = -(-n // A.PTS_ITER)
    for shell in (False, True):
        x = rng.uniform(BJ[1] - 0.3, BJ[1] - 0.1, n)      # far east of Q's candidate cells
        y = rng.uniform(BJ[3] - 0.3, BJ[3] - 0.1, n)
        at = np.minimum(np.arange(nit) * A.PTS_ITER + rng.integers(0, A.PTS_ITER, nit), n - 1)
        th = rng.uniform(0, 2 * np.pi, nit)
        rad = 0.03 + rng.integers(-3, 4, nit) * 1e-17 if shell else rng.uniform(0.01, 0.3, nit)
        x[at], y[at] = Q[0] + rad * np.cos(th), Q[1] + rad * np.sin(th)
        order, _ = A.oracle_order(A.cgrid(A.KNN_GRID), x, y, Q, R)
        assert sorted(order.tolist()) == sorted(set(at.tolist()))
        for k in (1, 50, 256):
            wi, wd, stats, end = knn_dev(ctx, x, y, k, f"sparse n={n} shell={shell} k={k}")
            want = expected_final(n, k, wi, x, y, order)
            if k == 1:
                assert want == DIRECT
            assert_final(f"sparse n={n} shell={shell} k={k}", want, end, kept=stats[2])
            if end == DIRECT and shell and n == 262_144:
                assert stats[2] > 256, stats    # every block's candidates share the lowest bin


# ------------------------------------------------------------------------------ arrival ------
@pytest.mark.parametrize("shape", ["near_first", "sawtooth", "far_first"])
def test_window_end_arrival(ctx, shape):
    """300,000 points in ascending distance (the k nearest in one block: not slot-complete for
    k > 8), in the sawtooth order, and in descending distance; far_first also at 1,200,003 points,
    where every block holds more candidates than its buffer and spills: the T path and its
    fallbacks."""
    for n in ((300_000, 1_200_003) if shape == "far_first" else (300_000,)):
        x0, y0, order, _ = base(n)
        p = {"near_first": A.near_first, "sawtooth": A.sawtooth, "far_first": A.far_first}[shape](n, order)
        x, y = x0[p], y0[p]
        spills = shape == "far_first" and A.per_block(A.knn_block_of(n), np.arange(n)).min() > A.PASS_CAP
        assert spills == (n == 1_200_003 and shape == "far_first")
        for k in KS:
            wi, wd, stats, end = knn_dev(ctx, x, y, k, f"{shape} n={n} k={k}")
            want = TPATH if spills else expected_final(n, k, wi, x, y)
            if shape != "far_first" and k in (50, 256):
                assert want == TPATH    # the k nearest arrive together: one block holds more than 8
            if spills:
                assert stats[1] > 0, stats
            assert_final(f"{shape} n={n} k={k}", want, end, kept=stats[2], spilled=stats[1], whole=stats[0])


@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
def test_window_end_equal_distance_shell(ctx, dense):
    """50,000 points on (almost) one circle.  Shuffled at 250,000 points: ties among the records'
    entries.  Dense (1,200,003 points, descending distance): every block spills and more entries
    lie at or below T than the final's LDS gather holds, the selection by rounds, which reads a
    slot-complete block's entries from its record."""
    x, y = A.shell_window(dense)
    if not dense:
        p = A.shuffled(len(x), 17)
        x, y = x[p], y[p]
    for k in (64, 256):
        wi, wd, stats, end = knn_dev(ctx, x, y, k, f"shell dense={dense} k={k}")
        if dense:
            assert stats[1] > 0 and stats[2] > 8 * 1024, stats
        assert_final(f"shell dense={dense} k={k}", TPATH if dense else expected_final(len(x), k, wi, x, y), end,
                     kept=stats[2], spilled=stats[1])


def test_window_end_few_and_no_candidates(ctx):
    """Fewer candidates than k (the count says so, the tail is padded) and none at all."""
    n = 5_000
    rng = np.random.default_rng(77)
    x = rng.uniform(BJ[1] - 0.3, BJ[1] - 0.1, n)
    y = rng.uniform(BJ[3] - 0.3, BJ[3] - 0.1, n)
    for k in (1, 50, 256, 257):
        wi, _, stats, end = knn_dev(ctx, x, y, k, f"no candidate k={k}")
        assert len(wi) == 0
        assert_final(f"no candidate k={k}", TPATH, end, kept=stats[2])   # empty blocks list, never slot
    at = rng.choice(n, 20, replace=False)
    x[at] = Q[0] + rng.uniform(-0.002, 0.002, 20)
    y[at] = Q[1] + rng.uniform(-0.002, 0.002, 20)
    for k in (1, 50, 256, 257):
        wi, _, stats, end = knn_dev(ctx, x, y, k, f"20 candidates k={k}", r=0.005, grid=1000)
        assert len(wi) == min(k, 20)
        # most iterations hold no candidate: at k >= 2 no block finds k published bins
        assert_final(f"20 candidates k={k}", TPATH if k > 1 else None, end, kept=stats[2])


@pytest.mark.parametrize("late", [True, False], ids=["late", "early"])
def test_window_end_late_and_early_entries(ctx, late):
    """The 50 nearest of 300,000 points placed in the window's last two fronts (the iterations a
    block's waves run last: entries that arrive after anything a block could have published
    early), or in its first front; at most 8 of them per block."""
    n, k = 300_000, 50
    x0, y0, order, _ = base(n)
    nb, _ = A.knn_pass_geometry(n)
    nit = -(-n // A.PTS_ITER)
    its = np.arange(nit - 2 * nb, nit - 1) if late else np.arange(nb)
    pos = A.spread(its, k) * A.PTS_ITER + 11
    p = A.place(n, [(order[:k], pos)], 5)
    x, y = x0[p], y0[p]
    wi, wd, stats, end = knn_dev(ctx, x, y, k, f"late={late}")
    assert sorted(wi.tolist()) == sorted(pos.tolist())
    assert A.per_block(A.knn_block_of(n), pos).max() <= A.PASS_HEADS
    assert_final(f"nearest {'late' if late else 'early'}", expected_final(n, k, wi, x, y), end, kept=stats[2])


def test_window_end_c2_shape_direct(ctx):
    """The benchmark's shape: 10M uniform points over the grid, k = 50, 256 blocks of 152 or 153
    iterations.  Every block has published its lowest bin twice in mid-stream long before any
    block ends, so every block finds its T_b, and a block of 39,000 uniform points holds at most
    8 points at or below it (asserted from the oracle for the k nearest; the records held 348-410
    entries in all over the traced windows): the direct final, asserted.  Then the same window
    with its 50 nearest moved into the last two fronts, one per block."""
    n, k = 10_000_000, 50
    x, y = synth.uniform(n, 2)
    nb = A.knn_pass_geometry(n)[0]
    nit = -(-n // A.PTS_ITER)
    assert nb == 256 and nit // nb >= 150
    wi, wd, stats, end = knn_dev(ctx, x, y, k, "C2 shape")
    assert A.per_block(A.knn_block_of(n), wi.astype(np.int64)).max() <= A.PASS_HEADS
    assert_final("C2 shape k=50", DIRECT, end, kept=stats[2])
    pos = A.spread(np.arange(nit - 2 * nb, nit - 1), k) * A.PTS_ITER + 11
    p = np.arange(n)
    src = wi.astype(np.int64)
    p[pos], p[src] = src, pos      # swap the nearest with the points of the late positions
    assert A.is_permutation(p, n)
    x, y = x[p], y[p]
    wi, wd, stats, end = knn_dev(ctx, x, y, k, "C2 shape, nearest late")
    assert sorted(wi.tolist()) == sorted(pos.tolist())
    assert_final("C2 shape k=50, nearest late", DIRECT, end, kept=stats[2])


# ------------------------------------------------------------------------------ sequences ----
def test_window_end_back_to_back(ctx):
    """Four launches on one context with no synchronisation between them, the grid shrinking and
    growing (256 -> 5 -> 235 -> 256 blocks) and k changing: records of blocks outside the smaller
    grid stay behind, and every launch relies on the words the one before re-armed."""
    import torch
    ag, cg = agrid(A.KNN_GRID), A.cgrid(A.KNN_GRID)
    seq = [(262_144, 50), (5_000, 256), (300_000, 1), (262_144, 50), (5_000, 257), (262_144, 256)]
    wins = {}
    for n, _ in seq:
        if n not in wins:
            x0, y0, _, _ = base(n)
            p = A.shuffled(n, 23)
            wins[n] = (x0[p], y0[p], dev(x0[p]), dev(y0[p]))
    torch.cuda.synchronize()
    outs = [launch(ctx, ag, wins[n][2], wins[n][3], k) for n, k in seq]
    torch.cuda.synchronize()
    for (n, k), out in zip(seq, outs):
        wi, wd = cref.knn_pp(cg, wins[n][0], wins[n][1], Q[0], Q[1], R, k)
        check(out, wi, wd, f"sequence n={n} k={k}")
    assert ctx.debug_knn_pass_stats()[1] == 0   # the spill count re-armed all along


# ------------------------------------------------------------------------------ paths --------
def test_window_end_fused_range(ctx, sctx):
    """The fused kNN + range pass in both hit orders at a small C5-like shape: 1000 x 1000 grid,
    k = 100, r = 0.05, 300,000 points."""
    n, k, r = 300_000, 100, 0.05
    x, y = synth.uniform(n, 91)
    ag, cg = agrid(1000), A.cgrid(1000)
    wi, wd = cref.knn_pp(cg, x, y, Q[0], Q[1], r, k)
    want = cref.range_pp(cg, x, y, Q[0], Q[1], r)
    tx, ty = dev(x), dev(y)
    for c, name in ((ctx, "ascending"), (sctx, "set")):
        for rep in range(2):
            (ki, kd), ro = c.knn_range_pp(ag, tx, ty, Q[0], Q[1], r, k)
            assert u32(ki).tolist() == wi.tolist(), name
            assert np.array_equal(kd.cpu().numpy().view(np.uint64), wd.view(np.uint64)), name
            got = u32(ro).astype(np.int64)
            assert np.array_equal(got if name == "ascending" else np.sort(got), want.astype(np.int64)), name
        end = c.debug_knn_pass_end()
        blk = A.knn_block_of(n, fused_ordered=name == "ascending")
        if end == DIRECT:    # needs every block slot-complete: none holds more than 8 of the k nearest
            assert A.per_block(blk, wi.astype(np.int64)).max() <= A.PASS_HEADS
        assert end in (DIRECT, TPATH), end
        note(f"fused range {name}", hits=len(want), ran=end)


def test_window_end_staged_host_window(ctx):
    """A pageable host window of a few staging chunks: one pass per 2^20-point chunk on one
    context, then the merge."""
    n = 3 * A.STAGE_PTS + 5
    rng = np.random.default_rng(55)
    x = rng.uniform(Q[0] - 0.4, Q[0] + 0.4, n)
    y = rng.uniform(BJ[2] + 0.02, Q[1] + 0.43, n)
    cg = A.cgrid(A.KNN_GRID)
    for k in (1, 50, 256):
        wi, wd = cref.knn_pp(cg, x, y, Q[0], Q[1], R, k)
        gi, gd = ctx.knn_pp(agrid(A.KNN_GRID), x, y, Q[0], Q[1], R, k)
        assert u32(gi).tolist() == wi.tolist(), k
        assert np.array_equal(np.asarray(gd).view(np.uint64), wd.view(np.uint64)), k


def test_window_end_pane_merge(ctx):
    """knn_merge_panes_lds over the lists of two passes (a two-pane sliding window)."""
    ag, cg = agrid(100), A.cgrid(100)
    panes, b = [], 0
    for j, s in enumerate((60_000, 5_000, 262_144)):
        panes.append(synth.uniform(s, 60 + j, base=b))
        b += s
    inc = IncrementalKNN(ctx, ag, Q[0], Q[1], 0.5, 50, 2)
    for j, (x, y) in enumerate(panes):
        gi, gd = inc.push(dev(x), dev(y))
        win = panes[max(0, j - 1):j + 1]
        wi, wd = cref.knn_pp(cg, np.concatenate([w[0] for w in win]), np.concatenate([w[1] for w in win]),
                             Q[0], Q[1], 0.5, 50)
        assert gi.cpu().numpy().tolist() == wi.tolist(), j
        assert np.array_equal(gd.cpu().numpy().view(np.uint64), wd.view(np.uint64)), j
