"""GPU: the streaming kernels under ordered and clustered arrival (tests/arrivals.py).

Every other parity test builds its window in shuffled arrival order, and the kernels' running
bounds, per-wave stages and reservation cursors see no pressure there: a shuffled window of 2^20
points holds at most 4 of its 256 nearest in one knn_pass block, under one join record per tile and
segment, and no range_set wave ever collects a 1024-hit run.  Real windows are not shuffled: a
trajectory stream delivers runs of nearby points, a keyBy(gridID) upstream a window sorted by cell.

Same comparisons as the parity tests -- kNN indices and distance bits, ascending range indices, the
set mode through sorted-unique, pair sets through pairs_sorted, trajectory arrays exactly -- against
the C oracle and the Python restatements, which always receive the arrival-ordered arrays.

Each test first asserts on the host that its window reaches the shape it is named for, with the
mirrors of arrivals.py, the oracle's result or Context.debug_knn_pass_stats (never the kernel's
answer), and records the figures in FIGURES (printed with -s).  tests/test_arrivals.py holds the
same conditions on the CPU and shows that the shuffled control meets none of them.

What they found: pass_final's fallback selection (more entries at or below T than its LDS gather
holds: k rounds over every list and the spill) masked only kLenWhole out of a block's length word,
so a slot-complete block (length | kLenSlots) was read to the end of its 3072-entry list region --
whatever an earlier launch, or nobody, had left there.  far_first at 1,200,003 points returned
(index 0, distance 0.0) as the nearest point for every k <= 256 on a device window (all heads empty:
each block's nearest had spilled, so T is none and the whole spill, 250,000 to 330,000 entries, is at or
below it), and near_first / sawtooth did so through the staged host window, whose second pass holds
only far points (24,680 entries in the k-th head's coarse bin).  test_knn_arrival[1200003-far_first],
[1200003-near_first], [1200003-sawtooth], test_knn_far_first_spill_and_repeat and
test_knn_equal_distance_shell_far_first[dense] fail without that mask.

Two figures of the issue that the launch geometry does not bear out are stated where they matter:
1,200,003 points run in 247 blocks of 4864 points, not 256 (knn_pass_geometry rounds a block's chunk
up to whole 256-point iterations); and four range_set iterations bring 1024 points, so a wave
cannot hold 1023 buffered hits and 63 staged band points before a fifth (arrivals.set_crafted_window
reaches the largest fill this window size allows, 1280 of kSetBuf = 1408, and the 1023 + 63 state
in the one wave that has six iterations).
"""
import numpy as np
import pytest

import arrivals as A
import cref
from helpers import binning_shape, pairs_sorted
from spatialflink_amd import Context, _abi, synth
from spatialflink_amd import distributed as D

pytestmark = pytest.mark.gpu

BJ, Q = A.BJ, A.Q
FIGURES = {}


def note(key, **fig):
    FIGURES[key] = fig
    print(f"[arrival] {key}: {fig}")


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


@pytest.fixture(scope="module")
def sctx():
    c = Context(0)
    c.set_range_order(True)
    return c


def same_knn(gi, gd, wi, wd, what=""):
    gi, gd = u32(gi), (gd.cpu().numpy() if hasattr(gd, "cpu") else np.asarray(gd))
    assert gi.tolist() == wi.tolist(), what
    assert np.array_equal(gd.view(np.uint64), wd.view(np.uint64)), what


def same_set(got, want, what=""):
    g = np.sort(u32(got).astype(np.int64))
    assert len(g) == len(want), what
    assert len(np.unique(g)) == len(g), "an index emitted twice " + what
    assert np.array_equal(g, np.sort(np.asarray(want).astype(np.int64))), what


def same_pairs(got, want, what=""):
    g = pairs_sorted(u32(got).reshape(-1, 2))
    assert np.array_equal(g, pairs_sorted(want)), what


def knn_entry_points(ctx, sctx, x, y, k, r=A.KNN_R, grid=A.KNN_GRID, what="", oracle=None):
    """knn_pp on the host window, knn_pp_async on a device window, knn_range_pp ordered and
    unordered (kNN and range results), all against the oracle.  Returns (wi, wd, pass stats of the
    async call or None for the large-k form)."""
    import torch
    ag, cg = agrid(grid), A.cgrid(grid)
    wi, wd = oracle if oracle is not None else cref.knn_pp(cg, x, y, Q[0], Q[1], r, k)
    want_r = cref.range_pp(cg, x, y, Q[0], Q[1], r)
    same_knn(*ctx.knn_pp(ag, x, y, Q[0], Q[1], r, k), wi, wd, what + " knn_pp host")
    tx, ty = dev(x), dev(y)
    oi = torch.empty(k, dtype=torch.int32, device="cuda")
    od = torch.empty(k, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    ctx.knn_pp_async(ag, tx, ty, Q[0], Q[1], r, k, oi, od, cnt)
    torch.cuda.synchronize()
    m = int(cnt.item())
    assert m == len(wi), what
    same_knn(oi[:m], od[:m], wi, wd, what + " knn_pp_async")
    assert (oi[m:] == -1).all()
    stats = ctx.debug_knn_pass_stats() if k <= _abi.KNN_MAX_K else None
    (ki, kd), ro = ctx.knn_range_pp(ag, tx, ty, Q[0], Q[1], r, k)
    same_knn(ki, kd, wi, wd, what + " knn_range_pp")
    assert np.array_equal(u32(ro), want_r), what + " knn_range_pp range"
    (ki, kd), ro = sctx.knn_range_pp(ag, tx, ty, Q[0], Q[1], r, k)
    same_knn(ki, kd, wi, wd, what + " knn_range_pp set")
    same_set(ro, want_r, what + " knn_range_pp set range")
    return wi, wd, stats


# ------------------------------------------------------------------------------ kNN ----------
@pytest.mark.parametrize("shape", A.KNN_SHAPES)
@pytest.mark.parametrize("n", A.KNN_SIZES)
def test_knn_arrival(ctx, sctx, n, shape):
    """n = 1,200,003 (247 blocks of 4864 points, 4688 iterations, a 3-point tail; as a host window two
    staged passes), 70,001 (69 blocks) and 4,097 (5 blocks); ten points are NaN (five of them still
    candidates, at the oracle's distance for a NaN coordinate); k = 1025 takes the large-k form.
    A placement the block cannot hold (k above its slot count at 4,097 and 70,001 points) fills
    the block's slots with the nearest."""
    x0, y0, _, _ = A.knn_base(n)
    nb, chunk = A.knn_pass_geometry(n)
    assert (nb, -(-n // A.PTS_ITER), n % A.PTS_ITER != 0) == {1_200_003: (247, 4688, True), 70_001: (69, 274, True),
                                                               4_097: (5, 17, True)}[n]
    for k in A.KNN_KS:
        p = A.knn_perm(n, shape, k)
        x, y = x0[p], y0[p]
        wi, wd = cref.knn_pp(A.cgrid(A.KNN_GRID), x, y, Q[0], Q[1], A.KNN_R, k)
        ok, fig = A.knn_shape_ok(n, shape, k, wi.astype(np.int64), wd, x, y)
        assert ok, (shape, k, fig)
        _, _, stats = knn_entry_points(ctx, sctx, x, y, k, what=f"{shape} n={n} k={k}", oracle=(wi, wd))
        if stats:
            fig.update(whole_lists=stats[0], spilled=stats[1], kept=stats[2])
        if shape == "far_first" and n == A.KNN_SIZES[0]:
            assert fig["spills"]
            if stats:   # survivors past a block's kCap are in the spill list
                assert stats[1] > 0, stats
        note(f"knn {shape} n={n} k={k}", **fig)


def test_knn_far_first_spill_and_repeat(ctx):
    """The spill path for real: in far_first order a candidate is nearer than everything before it,
    so it passes the running bound (but for iterations a block's waves finish out of order) and each
    of the 247 blocks receives ~4860 survivors against kCap = 3072: spilled > 0 by the stats hook,
    beside the count the geometry gives if every candidate survives.  Twice on one context (the
    spill count and the arrival tickets re-armed), then a shuffled window."""
    import torch
    n = A.KNN_SIZES[0]
    x0, y0, _, _ = A.knn_base(n)
    p = A.knn_perm(n, "far_first", 50)
    x, y = x0[p], y0[p]
    ag, cg = agrid(A.KNN_GRID), A.cgrid(A.KNN_GRID)
    cand = np.flatnonzero(np.isfinite(x) & np.isfinite(y))
    surv = A.per_block(A.knn_block_of(n), cand)
    floor = int(np.maximum(surv - A.PASS_CAP, 0).sum())
    assert surv.min() > A.PASS_CAP and floor > 400_000
    tx, ty = dev(x), dev(y)
    for k in (1, 50, 256, 1000):
        wi, wd = cref.knn_pp(cg, x, y, Q[0], Q[1], A.KNN_R, k)
        oi = torch.empty(k, dtype=torch.int32, device="cuda")
        od = torch.empty(k, dtype=torch.float64, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        for rep in range(2):
            ctx.knn_pp_async(ag, tx, ty, Q[0], Q[1], A.KNN_R, k, oi, od, cnt)
            torch.cuda.synchronize()
            same_knn(oi, od, wi, wd, f"k={k} rep={rep}")
            stats = ctx.debug_knn_pass_stats()
            assert stats[1] > 0, stats
        note(f"knn far_first spill k={k}", spilled=stats[1], if_every_candidate_survives=floor, whole_lists=stats[0],
             kept=stats[2])
    ps = A.shuffled(n, 77)
    xs, ys = x0[ps], y0[ps]
    wi, wd = cref.knn_pp(cg, xs, ys, Q[0], Q[1], A.KNN_R, 50)
    same_knn(*ctx.knn_pp(ag, dev(xs), dev(ys), Q[0], Q[1], A.KNN_R, 50), wi, wd, "shuffled after the spills")
    note("knn shuffled after the spills", spilled=ctx.debug_knn_pass_stats()[1])


@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
def test_knn_equal_distance_shell_far_first(ctx, sctx, dense):
    """test_knn_equal_distance_shell's window in far_first order at k = 64, and at k = 256, the k
    whose k-th distance lies in the shell (at 64 the nearest are inside it: tests/test_arrivals.py).
    That window has 245 blocks of at most 1024 points, so nothing spills; the dense variant puts the
    shell among the 64 nearest of the 1,200,003-point window, where every block spills and more
    entries lie at or below T than the final's gather holds (kept > 8192: the selection by rounds)."""
    x, y = A.shell_window(dense)
    for k in (64, 256):
        _, wd, stats = knn_entry_points(ctx, sctx, x, y, k, what=f"shell k={k}")
        in_shell = abs(wd[-1] - (0.001 if dense else 0.03)) < 1e-9
        assert in_shell == (dense or k == 256)
        if dense:
            assert stats[1] > 0 and stats[2] > 8 * 1024, stats
        note(f"knn shell {'dense' if dense else 'sparse'} k={k}", kth_in_shell=in_shell, whole_lists=stats[0],
             spilled=stats[1], kept=stats[2])


# ------------------------------------------------------------------------------ range --------
@pytest.mark.parametrize("shape", A.RANGE_SHAPES)
@pytest.mark.parametrize("n", A.RANGE_SIZES)
def test_range_arrival(ctx, sctx, n, shape):
    """Ascending mode (range_fused: blocks of contiguous 1024-point units behind a look-back) and set
    mode (range_set), exact and approximate, host and device windows, and the two-phase capacity
    error followed by a retry."""
    ag, cg = agrid(100), A.cgrid(100)
    for approx in (False, True):
        x0, y0, _ = A.range_base(n, approx)
        p = A.range_perm(n, shape, approx)
        x, y = x0[p], y0[p]
        want = cref.range_pp(cg, x, y, Q[0], Q[1], 0.5, approx)
        ok, fig = A.range_shape_ok(n, shape, want.astype(np.int64))
        assert ok, (shape, approx, fig)
        note(f"range {shape} n={n} approx={approx}", hits=len(want), **fig)
        tx, ty = dev(x), dev(y)
        assert np.array_equal(u32(ctx.range_pp(ag, x, y, Q[0], Q[1], 0.5, approx)), want)
        assert np.array_equal(u32(ctx.range_pp(ag, tx, ty, Q[0], Q[1], 0.5, approx)), want)
        same_set(sctx.range_pp(ag, x, y, Q[0], Q[1], 0.5, approx), want)
        same_set(sctx.range_pp(ag, tx, ty, Q[0], Q[1], 0.5, approx), want)
        for c in (ctx, sctx):
            with pytest.raises(_abi.GeohipCapacityError):
                c.range_pp(ag, x, y, Q[0], Q[1], 0.5, approx, cap=len(want) - 1)
            same_set(c.range_pp(ag, x, y, Q[0], Q[1], 0.5, approx, cap=len(want)), want)


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _set_run(sctx, ag, tx, ty, r, approx, n):
    """One async set-mode call into a buffer filled with -1: (count, hits, the rest of the buffer)."""
    import torch
    out = torch.full((n + 4096,), -1, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    sctx.range_pp_async(ag, tx, ty, Q[0], Q[1], r, approx, out, len(out), cnt)
    sctx.sync()
    m = int(cnt.item())
    return m, out[:m], out[m:]


def test_range_set_early_reservation(sctx):
    """5 * 2^20 + 77 points that are all hits (10-cell grid, r = 2: the guaranteed boxes cover the
    grid, as RANGE_CASES' (10, 2.0, ...)).  A wave gets five iterations, 1280 hits, so it takes the
    early 1024-hit reservation and moves the rest to the front.  Every index once, nothing written
    past the count; twice per mode on one context."""
    import torch
    n, cus = A.SET_N, _cus()
    nb, W, iters = A.range_set_geometry(n, cus)
    per_wave = (iters // W) * A.PTS_ITER   # hits of the wave with the fewest iterations
    assert per_wave >= A.SET_RUN, (cus, per_wave)
    ag, cg = agrid(10), A.cgrid(10)
    q = (116.5, 40.3)
    tx = torch.empty(n, dtype=torch.float64, device="cuda")
    ty = torch.empty(n, dtype=torch.float64, device="cuda")
    sctx.synth_uniform_async(tx, ty, 0, 5, BJ)
    hx, hy = synth.uniform(n, 5)
    for approx in (False, True):
        assert cref.range_pp_hash(cg, hx, hy, q[0], q[1], 2.0, approx)[0] == n
        for rep in range(2):
            out = torch.full((n + 4096,), -1, dtype=torch.int32, device="cuda")
            cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
            sctx.range_pp_async(ag, tx, ty, q[0], q[1], 2.0, approx, out, len(out), cnt)
            sctx.sync()
            assert int(cnt.item()) == n
            assert torch.equal(torch.sort(out[:n]).values, torch.arange(n, dtype=torch.int32, device="cuda"))
            assert (out[n:] == -1).all()
    note("range_set early reservation", cus=cus, waves=W, hits_per_wave_at_least=per_wave,
         early_reservations_at_least=W * (per_wave // A.SET_RUN))


def test_range_set_buffer_bound(sctx):
    """arrivals.set_crafted_window: one wave reaches a fill of 1280 at its fifth check (961 buffered
    hits, 63 staged band points flushed by a 64th, 255 direct hits), wave 0 holds 1023 buffered hits
    and 63 staged band points before the window's 77-point tail.  The band points lie a few ulp
    inside the circle (the oracle's dist <= r holds for each), so no tolerance is involved."""
    n, cus = A.SET_N, _cus()
    x, y, wa, kinds = A.set_crafted_window(cus)
    ag, cg = agrid(A.SET_BAND_GRID), A.cgrid(A.SET_BAND_GRID)
    want = cref.range_pp(cg, x, y, Q[0], Q[1], A.SET_BAND_R)
    assert np.array_equal(np.flatnonzero(kinds > 0), want)
    ta = A.range_set_wave_trace(A.set_wave_kinds(kinds, n, cus, wa))
    t0 = A.range_set_wave_trace(A.set_wave_kinds(kinds, n, cus, 0))
    assert ta[:2] == (1280, 1) and (ta[2][4], ta[3][4]) == (63, 961)
    assert t0[:2] == (1163, 1) and (t0[2][5], t0[3][5]) == (63, 1023)
    note("range_set buffer bound", wave=wa, peak_fill=ta[0], wave0_peak_fill=t0[0], buffer=A.SET_BUF)
    tx, ty = dev(x), dev(y)
    for rep in range(2):
        m, hits, rest = _set_run(sctx, ag, tx, ty, A.SET_BAND_R, False, n)
        assert m == len(want)
        same_set(hits, want)
        assert (rest == -1).all()
    want_a = cref.range_pp(cg, x, y, Q[0], Q[1], A.SET_BAND_R, True)
    m, hits, rest = _set_run(sctx, ag, tx, ty, A.SET_BAND_R, True, n)
    same_set(hits, want_a)
    assert (rest == -1).all()


# ------------------------------------------------------------------------------ join ---------
@pytest.mark.parametrize("qorder", A.JOIN_QUERY_ORDERS)
@pytest.mark.parametrize("dorder", A.JOIN_DATA_ORDERS)
def test_join_arrival(ctx, dorder, qorder):
    """300,000 clustered data points sorted by cell (either way) or in runs: one 4096-point
    segment holds thousands of records of one tile (several kJbRound = 1024 rounds in jb_tiles)
    where the shuffled window holds ~130.  join_pp exact and approximate, join_pp_count and
    band_pack_async on the same windows."""
    import torch
    ag, cg = agrid(A.JOIN_GRID), A.cgrid(A.JOIN_GRID)
    dx0, dy0, qx0, qy0 = A.join_base()
    pd_, pq = A.order_perm(dorder, dx0, dy0, cg), A.order_perm(qorder, qx0, qy0, cg)
    dx, dy, qx, qy = dx0[pd_], dy0[pd_], qx0[pq], qy0[pq]
    shape = binning_shape(dx, dy)
    ctl = A.shuffled(len(dx0), 4)
    control = binning_shape(dx0[ctl], dy0[ctl])
    assert shape[3] > 1024 and control[3] <= 1024, (shape, control)
    note(f"join data={dorder} queries={qorder}", records_of_one_tile_in_one_segment=shape[3], shuffled=control[3],
         largest_tile=shape[0])
    for approx in (False, True):
        want = cref.join_pp(cg, cg, dx, dy, qx, qy, A.JOIN_R, approx)
        assert len(want) > 100_000
        same_pairs(ctx.join_pp(ag, ag, dx, dy, qx, qy, A.JOIN_R, approx), want, f"approx={approx}")
        assert ctx.join_pp_count(ag, ag, dx, dy, qx, qy, A.JOIN_R, approx) == len(want)
    same_pairs(ctx.join_pp(ag, ag, dev(dx), dev(dy), dev(qx), dev(qy), A.JOIN_R), cref.join_pp(cg, cg, dx, dy, qx, qy, A.JOIN_R))
    # the owner pack of the same data window: same points, same owners, same order as the torch restatement
    xd, yd = dev(dx), dev(dy)
    base, world = 12345, 4
    ox, oy, oi, cnt = ctx.band_pack_async(ag, A.JOIN_GRID, world, xd, yd, base)
    torch.cuda.synchronize()
    tx, ty, ti, tc = D.torch_band_pack(ag)(torch.from_numpy(dx), torch.from_numpy(dy), base, A.JOIN_GRID, world)
    m = int(tc.sum())
    assert m == len(dx) and cnt.cpu().tolist() == tc.tolist()
    assert np.array_equal(oi[:m].cpu().numpy(), ti.numpy())
    assert np.array_equal(ox[:m].cpu().numpy().view(np.uint64), tx.numpy().view(np.uint64))
    assert np.array_equal(oy[:m].cpu().numpy().view(np.uint64), ty.numpy().view(np.uint64))


# ------------------------------------------------------------------------------ point-polygon -
def _ppoly_calls(c, x, y, pr, off, vx, vy, what):
    ag, cg = agrid(A.PPOLY_GRID), A.cgrid(A.PPOLY_GRID)
    for approx in (False, True):
        want = cref.range_ppoly(cg, x, y, off, vx, vy, A.PPOLY_R, approx, pr)
        same_pairs(c.range_ppoly(ag, x, y, off, vx, vy, A.PPOLY_R, approx, poly_rings=pr), want, f"{what} range {approx}")
    want = cref.join_ppoly(cg, cg, x, y, off, vx, vy, A.PPOLY_R, False, pr)
    same_pairs(c.join_ppoly(ag, ag, x, y, off, vx, vy, A.PPOLY_R, poly_rings=pr), want, what + " join")
    return len(want)


@pytest.mark.parametrize("order", A.PPOLY_ORDERS)
@pytest.mark.parametrize("name", A.PPOLY_SETS)
def test_ppoly_arrival(name, order):
    """200,000 points, 3 and 40 star polygons and synth.holed_polygons, sorted by cell, in runs and
    with the oracle's hits as one run.  A context of its own: the candidate buffer's history is
    the test's."""
    c = Context(0)
    pr, off, vx, vy = A.ppoly_polygons(name)
    x0, y0 = A.ppoly_base(name)
    p = A.ppoly_perm(name, order)
    x, y = x0[p], y0[p]
    cg = A.cgrid(A.PPOLY_GRID)
    pairs = cref.range_ppoly(cg, x, y, off, vx, vy, A.PPOLY_R, False, pr)
    share = A.chunk_share(len(x), np.unique(pairs[:, 1]))
    cells_min = A.chunk_cells(*A.cells(cg, x, y))
    if order == "inside_first":
        assert share[0] == 1.0 and share[1] == 1.0 and share[-1] == 0.0
    else:
        assert cells_min < 2200, cells_min
    note(f"ppoly {name} {order}", pairs=len(pairs), all_hit_chunks=int((share == 1).sum()),
         fewest_cells_in_a_chunk=cells_min)
    for rep in range(2):
        _ppoly_calls(c, x, y, pr, off, vx, vy, f"{name} {order} call {rep}")


def test_ppoly_edge_head_overflows_first_buffer():
    """The first 70,000 points, contiguous, lie within r of ring edges and are candidates of the
    exact test (arrivals.ppoly_edge_window): more than the 65,536 entries of a fresh context's
    candidate buffer, in chunks made of candidates only, so the chunks past the buffer go to the redo
    pass.  Twice (the second call's buffer is sized by the first's count), then a sparse shuffled
    window, then the edge window again; range and join pairs equal the oracle's on every call."""
    c = Context(0)
    off, vx, vy, x, y = A.ppoly_edge_window()
    cg = A.cgrid(A.PPOLY_GRID)
    pairs = cref.range_ppoly(cg, x, y, off, vx, vy, A.PPOLY_R)
    head = A.ppoly_candidates_lower_bound(cg, x, y, pairs, len(off) - 1, upto=A.EDGE_HEAD)
    ccap = A.ppoly_first_ccap(len(x))
    assert head >= A.EDGE_HEAD > ccap == 65536
    note("ppoly edge head", candidates_at_least=head, first_buffer=ccap, chunks_of_candidates_only=A.EDGE_HEAD // A.STREAM_CHUNK)
    sx, sy = synth.uniform(A.PPOLY_N, 39)
    ps = A.shuffled(A.PPOLY_N, 40)
    sx, sy = sx[ps], sy[ps]
    for step, (wx, wy) in enumerate(((x, y), (x, y), (sx, sy), (x, y))):
        _ppoly_calls(c, wx, wy, None, off, vx, vy, f"edge window step {step}")


@pytest.mark.parametrize("k", A.KNN_PPOLY_KS)
def test_knn_ppoly_arrival(k):
    """All k nearest of the query polygon in one 4096-point chunk: the first, one in the middle and
    the partial last one."""
    c = Context(0)
    _, off, vx, vy = A.ppoly_polygons("stars40")
    x0, y0 = A.ppoly_base("stars40")
    v1x, v1y = vx[:int(off[1])].copy(), vy[:int(off[1])].copy()
    ag, cg = agrid(A.PPOLY_GRID), A.cgrid(A.PPOLY_GRID)
    last = (len(x0) - 1) // A.STREAM_CHUNK
    for chunk in (0, 7, last):
        p = A.knn_ppoly_perm(x0, y0, v1x, v1y, k, chunk)
        x, y = x0[p], y0[p]
        wi, wd = cref.knn_ppoly(cg, x, y, v1x, v1y, 0.02, k)
        assert len(wi) == k and (wi // A.STREAM_CHUNK == chunk).all()
        gi, gd = c.knn_ppoly(ag, x, y, v1x, v1y, 0.02, k)
        same_knn(gi, gd, wi, wd, f"knn_ppoly k={k} chunk={chunk}")
        gi, gd = c.knn_ppoly(ag, dev(x), dev(y), v1x, v1y, 0.02, k)
        same_knn(gi, gd, wi, wd, f"knn_ppoly device k={k} chunk={chunk}")


# ------------------------------------------------------------------------------ trajectories --
RUN_LENS = [1, 31, 32, 33, 63, 64, 65, 1024, 2049, 5000]


def _traj_ids(T):
    return [f"t{k:03d}" + "_" * (k % 13) for k in range(T)]


def _traj_windows():
    """name -> objIDs in arrival order."""
    ids = _traj_ids(len(RUN_LENS))
    up = [ids[k] for k, m in enumerate(RUN_LENS) for _ in range(m)]
    down = [ids[k] for k, m in reversed(list(enumerate(RUN_LENS))) for _ in range(m)]
    order = np.random.default_rng(3).permutation(len(RUN_LENS))
    mixed = [ids[k] for k in order for _ in range(RUN_LENS[k])]
    out = {"runs_ascending": up, "runs_descending": down, "runs_mixed": mixed, "one_trajectory": ["solo-object"] * 5000}
    for T in (64, 65, 300):
        rr = _traj_ids(T)
        out[f"round_robin_{T}"] = [rr[i % T] for i in range(64 * 70 + 5)]
    return out


def _waves_of_one_key(oids):
    """64-point waves of traj_insert (wave w inserts points [64 w, 64 w + 64)) whose keys are all equal."""
    return sum(1 for s in range(0, len(oids) - 63, 64) if len(set(oids[s:s + 64])) == 1)


@pytest.mark.parametrize("name", list(_traj_windows()))
def test_traj_arrival(ctx, name):
    """Each trajectory as one contiguous run (lengths 1 to 5000, in ascending, descending and mixed
    id order): whole waves of traj_insert insert 64 equal keys.  Round robin over 64, 65 and 300
    trajectories: a wave's 64 keys are all distinct and a key returns every T points.  One
    trajectory of 5000 points.  traj_group, tstats, traj_gather, traj_selected against traj_ref;
    traj_filter_hit on a trange_classify result against trange_ref.  Timestamps equal, decreasing
    and mixed within a run (fuzz_columns' small ranges)."""
    import test_gpu_traj as T
    import test_gpu_trange as TG
    import traj_ref
    import trange_ref as TR
    oids = _traj_windows()[name]
    n = len(oids)
    eq = _waves_of_one_key(oids)
    if name.startswith("runs") or name == "one_trajectory":
        assert eq >= 70
    else:
        assert eq == 0 and all(len(set(oids[s:s + 64])) == 64 for s in range(0, n - 63, 64))
    note(f"traj {name}", points=n, waves_of_one_key=eq)
    got, want = T.group_both(ctx, oids)
    assert got["n_sel"] == n
    for seed, (lo, hi) in enumerate([(-3, 4), (0, 1), (-2, 3)]):   # (0, 1): every timestamp equal
        x, y, ts = T.fuzz_columns(n, seed=seed + 11, ts_lo=lo, ts_hi=hi)
        T.check_tstats(ctx, x, y, ts, got, want)
    dec = np.arange(n, 0, -1, dtype=np.int64)   # strictly decreasing inside every run
    T.check_tstats(ctx, x, y, dec, got, want)
    gx, gy, gt = ctx.traj_gather(T.dev(x, np.float64), T.dev(y, np.float64), got["perm"], T.dev(ts, np.int64))
    pm = np.array(want["perm"], dtype=np.int64)
    assert np.array_equal(gx.cpu().numpy().view(np.uint64), x[pm].view(np.uint64))
    assert np.array_equal(gy.cpu().numpy().view(np.uint64), y[pm].view(np.uint64))
    assert np.array_equal(gt.cpu().numpy(), ts[pm])
    assert T.u32(ctx.traj_selected(got["traj_of"])) == list(range(n))
    # the hit filter on the device's own classes of these arrivals
    rng = np.random.default_rng(17)
    xs, ys = rng.uniform(-1.0, 17.0, n), rng.uniform(-1.0, 17.0, n)
    polys_in = [[TG.SQUARE], [TG.CONCAVE], [TG.TRIANGLE]]
    cls, _ = TG.classify_gpu(ctx, TG.DY, xs, ys, polys_in)
    wcls = np.array(TR.classify(TG.frames.restate_grid(TG.DY), xs, ys, TR.polygons(polys_in)), np.uint8)
    assert np.array_equal(cls, wcls) and min((wcls == c).sum() for c in (0, 1, 2)) > 20
    TG.check_filter(ctx, oids, cls)
    far = np.where(np.arange(n) < n // 2, wcls, np.minimum(wcls, 1)).astype(np.uint8)   # hits in the first half only
    TG.check_filter(ctx, oids, far)
    assert traj_ref.group(oids)["traj_off"][-1] == n


def test_traj_arrival_nulls_and_selection(ctx):
    """Runs with null objIDs inside them and a selection set that keeps every other trajectory (and
    names absent ones)."""
    import test_gpu_traj as T
    ids = _traj_ids(len(RUN_LENS))
    oids = [ids[k] for k, m in enumerate(RUN_LENS) for _ in range(m)]
    rng = np.random.default_rng(5)
    for i in rng.choice(len(oids), 400, replace=False):
        oids[int(i)] = None
    oids[289:289 + 64] = [None] * 64     # a stretch of the 1024-run: whole waves see null keys
    id_set = set(ids[::2]) | {"nobody", "t00"}
    got, want = T.group_both(ctx, oids, id_set)
    assert 0 < got["n_sel"] < len(oids) and got["n_traj"] == len(ids[::2])
    x, y, ts = T.fuzz_columns(len(oids), seed=23)
    T.check_tstats(ctx, x, y, ts, got, want)
    assert T.u32(ctx.traj_selected(got["traj_of"])) == [i for i, t in enumerate(want["traj_of"]) if t != T.R.UNSELECTED]


# ------------------------------------------------------------------------------ streams -------
def _panes(x, y, cuts):
    return [(x[a:b], y[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]


@pytest.mark.parametrize("order", ["near_first", "far_first"])
@pytest.mark.parametrize("k", [7, 50])
def test_incremental_knn_arrival(ctx, k, order):
    """IncrementalKNN with 3 panes over a near_first stream: the first pane holds all k nearest of
    every window it is part of; once it expires the result must come from the remaining panes.
    far_first: the newest pane always holds the window's k nearest."""
    from spatialflink_amd.incremental import IncrementalKNN
    n = 70_001
    x0, y0, _, _ = A.knn_base(n)
    p = A.knn_perm(n, order, k)
    x, y = x0[p], y0[p]
    cuts = [0, 9_000, 20_001, 20_001, 41_000, 55_555, n]   # ragged panes, an empty one
    panes = _panes(x, y, cuts)
    ag, cg = agrid(A.KNN_GRID), A.cgrid(A.KNN_GRID)
    inc = IncrementalKNN(ctx, ag, Q[0], Q[1], A.KNN_R, k, 3)
    for j, (px, py) in enumerate(panes):
        gi, gd = inc.push(dev(px), dev(py))
        lo = max(0, j - 2)
        wx, wy = x[cuts[lo]:cuts[j + 1]], y[cuts[lo]:cuts[j + 1]]
        wi, wd = cref.knn_pp(cg, wx, wy, Q[0], Q[1], A.KNN_R, k)
        if order == "near_first":
            assert wi.max() < k                         # the window's first k arrivals: its oldest pane that holds any
        elif len(px) >= k:
            assert wi.min() >= len(wx) - len(px)         # all in the newest pane
        same_knn(gi, gd, wi, wd, f"window {j}")


def test_incremental_range_and_ppoly_hits_in_oldest_pane(ctx):
    """IncrementalRange and IncrementalPPolyRange over hits_first streams: every hit of the stream
    sits in its first pane, so later windows carry it as their oldest pane and then lose it."""
    from spatialflink_amd.incremental import IncrementalPPolyRange, IncrementalRange
    n = 70_001
    ag, cg = agrid(100), A.cgrid(100)
    x0, y0, hits = A.range_base(n, False)
    p = A.range_perm(n, "hits_first", False)
    x, y = x0[p], y0[p]
    cuts = [0, 15_000, 33_333, 50_000, n]
    assert len(hits) < cuts[1]
    inc = IncrementalRange(ctx, ag, Q[0], Q[1], 0.5, False, 3)
    for j in range(len(cuts) - 1):
        inc.push(dev(x[cuts[j]:cuts[j + 1]]), dev(y[cuts[j]:cuts[j + 1]]))
        lo = max(0, j - 2)
        want = cref.range_pp(cg, x[cuts[lo]:cuts[j + 1]], y[cuts[lo]:cuts[j + 1]], Q[0], Q[1], 0.5)
        assert len(want) == (len(hits) if lo == 0 else 0)
        local = inc.window_local()
        assert (local.cpu().numpy() if hasattr(local, "cpu") else local).tolist() == want.tolist()
    # point-polygon: the oracle's hits as one run at the head of the stream
    _, off, vx, vy = A.ppoly_polygons("stars40")
    bx, by = A.ppoly_base("stars40")
    pp = A.ppoly_perm("stars40", "inside_first")
    bx, by = bx[pp], by[pp]
    g5, c5 = agrid(A.PPOLY_GRID), A.cgrid(A.PPOLY_GRID)
    cuts = [0, 40_000, 100_000, 150_000, len(bx)]
    c = Context(0)
    incp = IncrementalPPolyRange(c, g5, off, vx, vy, A.PPOLY_R, False, 2)
    for j in range(len(cuts) - 1):
        got = incp.push(dev(bx[cuts[j]:cuts[j + 1]]), dev(by[cuts[j]:cuts[j + 1]]))
        got = np.concatenate([g.cpu().numpy().astype(np.int64).reshape(-1, 2) & 0xFFFFFFFF for g in got])
        got[:, 1] = (got[:, 1] - incp.window_start) & 0xFFFFFFFF
        lo = max(0, j - 1)
        want = cref.range_ppoly(c5, bx[cuts[lo]:cuts[j + 1]], by[cuts[lo]:cuts[j + 1]], off, vx, vy, A.PPOLY_R)
        assert (len(want) > 5000) == (lo == 0)
        assert np.array_equal(pairs_sorted(got), pairs_sorted(want))


@pytest.mark.parametrize("k", [100, 1024])
@pytest.mark.parametrize("order", ["near_first", "far_first"])
def test_knn_merge_arrival(ctx, order, k):
    """knn_merge_async over 8 shards of a near_first window (list 0 holds the whole result, the other
    lists lose every comparison) and of a far_first one (the last list holds it), against the
    unsharded oracle."""
    import torch
    n = 70_001
    x0, y0, _, _ = A.knn_base(n)
    p = A.knn_perm(n, order, k)
    x, y = x0[p], y0[p]
    ag, cg = agrid(A.KNN_GRID), A.cgrid(A.KNN_GRID)
    S = 8
    bounds = [(n * s) // S for s in range(S + 1)]
    wi, wd = cref.knn_pp(cg, x, y, Q[0], Q[1], A.KNN_R, k)
    holder = 0 if order == "near_first" else S - 1
    assert bounds[holder] <= wi.min() and wi.max() < bounds[holder + 1]
    d_all = torch.empty((S, k), dtype=torch.float64, device="cuda")
    i_all = torch.empty((S, k), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(S + 1, dtype=torch.int32, device="cuda")
    for s in range(S):
        a, b = bounds[s], bounds[s + 1]
        ctx.knn_pp_async(ag, dev(x[a:b]), dev(y[a:b]), Q[0], Q[1], A.KNN_R, k, i_all[s], d_all[s], cnt[s:s + 1])
        torch.cuda.synchronize()
        i_all[s] = torch.where(i_all[s] != -1, i_all[s] + a, i_all[s])
    oi = torch.empty(k, dtype=torch.int32, device="cuda")
    od = torch.empty(k, dtype=torch.float64, device="cuda")
    ctx.knn_merge_async(d_all, i_all, S, k, k, oi, od, cnt[S:])
    torch.cuda.synchronize()
    assert int(cnt[S].item()) == k
    same_knn(oi, od, wi, wd)
