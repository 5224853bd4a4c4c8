"""CPU: the arrival orders and launch-geometry mirrors of tests/arrivals.py.

Every order is a permutation; the windows tests/test_gpu_arrival.py feeds the kernels reach the
shapes they are named for, by the oracle and the mirrors alone; and the shuffled control, what every
other parity test uses, reaches none of them -- which is the gap those tests close.
"""
import numpy as np
import pytest

import arrivals as A
import cref
from helpers import binning_shape


@pytest.fixture(scope="module", autouse=True)
def _release_windows():
    yield
    A.release()


def test_mirrors_on_known_sizes():
    # knn_pass_geometry: chunks of whole 256-point iterations, at least 1024 points
    assert A.knn_pass_geometry(1_200_003) == (247, 4864)
    assert A.knn_pass_geometry(70_001) == (69, 1024)
    assert A.knn_pass_geometry(4_097) == (5, 1024)
    assert A.knn_pass_geometry(1 << 20) == (256, 4096)
    blk = A.knn_block_of(4_097)
    assert blk[:256].tolist() == [0] * 256 and blk[256] == 1 and blk[5 * 256] == 0 and blk[4096] == 1
    assert A.knn_block_of(4_097, fused_ordered=True)[[0, 1023, 1024, 4096]].tolist() == [0, 0, 1, 4]
    host = A.knn_block_of(1_200_003, host=True)
    assert host[(1 << 20) - 1] == 255 and host[1 << 20] == 256 and host.max() == 256 + 147
    assert A.range_fused_geometry(300_000) == (147, 2048) and A.range_fused_geometry(70_001) == (69, 1024)
    assert A.range_set_geometry(A.SET_N, 256) == (256, 4096, 20481)
    assert A.range_set_geometry(300_000, 256) == (74, 1184, 1172)   # one iteration per wave
    assert A.ppoly_first_ccap(200_000) == 65536 and A.ppoly_first_ccap(2_000_000) == 125000
    assert A.ppoly_chunk_of(8193)[[0, 4095, 4096, 8192]].tolist() == [0, 0, 1, 2]


def test_cells_equal_the_oracle():
    cg = A.cgrid(500)
    rng = np.random.default_rng(1)
    x = rng.uniform(A.BJ[0] - 0.2, A.BJ[1] + 0.2, 2000)
    y = rng.uniform(A.BJ[2] - 0.2, A.BJ[3] + 0.2, 2000)
    k = rng.integers(0, 501, 200)
    x[:200] = A.BJ[0] + k * cg.cell_len   # on cell edges
    x[200], y[201], x[202], y[203] = np.nan, np.nan, np.inf, -np.inf
    cx, cy = A.cells(cg, x, y)
    want = [cref.cell(cg, float(a), float(b)) for a, b in zip(x, y)]
    assert list(zip(cx.tolist(), cy.tolist())) == want


def test_every_order_is_a_permutation():
    n = 10_007
    rng = np.random.default_rng(2)
    x = rng.uniform(A.Q[0] - 0.4, A.Q[0] + 0.4, n)
    y = rng.uniform(A.BJ[2] + 0.02, A.Q[1] + 0.43, n)
    x[5] = np.nan
    cg = A.cgrid(100)
    order, dist = A.oracle_order(cg, x, y, A.Q, 0.5)
    assert len(order) == n - 1 and (np.diff(dist) >= 0).all()
    hits = cref.range_pp(cg, x, y, A.Q[0], A.Q[1], 0.2)
    cx, cy = A.cells(cg, x, y)
    blk = A.knn_block_of(n)
    perms = {
        "shuffled": A.shuffled(n, 1), "near_first": A.near_first(n, order), "far_first": A.far_first(n, order),
        "cell_sorted": A.cell_sorted(cx, cy), "cell_sorted_rev": A.cell_sorted_rev(cx, cy),
        "hits_first": A.hits_first(n, hits), "hits_last": A.hits_last(n, hits), "sawtooth": A.sawtooth(n, order),
        "runs": A.runs(x, y, cx, cy, 3), "in_block": A.in_block(n, order[:300], blk, 2, 4),
    }
    for name, p in perms.items():
        assert A.is_permutation(p, n), name
    assert not A.is_permutation(np.zeros(n, np.int64), n)
    assert perms["near_first"][:3].tolist() == order[:3].tolist() and perms["far_first"][-1] == order[0]
    assert (blk[np.flatnonzero(np.isin(perms["in_block"], order[:300]))] == 2).all()
    assert set(perms["hits_first"][:len(hits)].tolist()) == set(hits.tolist())
    assert set(perms["hits_last"][n - len(hits):].tolist()) == set(hits.tolist())
    key = (cx * 100000 + cy)[perms["cell_sorted"]]
    assert (np.diff(key) >= 0).all() and (np.diff(key[::-1]) <= 0).all()
    # runs: pieces of 1..2000 spatially adjacent points -- consecutive arrivals are, in the median,
    # far closer than in a shuffled window
    step = lambda p: np.nanmedian(np.hypot(np.diff(x[p]), np.diff(y[p])))  # noqa: E731
    assert step(perms["runs"]) < 0.2 * step(perms["shuffled"])


@pytest.mark.parametrize("n", A.KNN_SIZES)
def test_knn_windows_reach_their_shapes(n):
    cg = A.cgrid(A.KNN_GRID)
    x, y, order, dist = A.knn_base(n)
    for shape in A.KNN_SHAPES + ("shuffled",):
        # (the GPU test asserts every k at every size; here the large window takes three of them)
        for k in A.KNN_KS if n < 1_000_000 else (50, 256, 1025):
            p = A.knn_perm(n, shape, k)
            assert A.is_permutation(p, n)
            xx, yy = x[p], y[p]
            wi, wd = cref.knn_pp(cg, xx, yy, A.Q[0], A.Q[1], A.KNN_R, k)
            ok, fig = A.knn_shape_ok(n, shape, k, wi.astype(np.int64), wd, xx, yy)
            assert ok == (shape != "shuffled"), (shape, k, fig)
            if shape == "far_first":  # only the large window has a block past its survivor buffer
                assert fig["spills"] == (n == A.KNN_SIZES[0]), fig
            if shape == "shuffled" and n == A.KNN_SIZES[0] and k <= 256:
                # the gap: a shuffled window never holds more than kPassHeads of the k nearest in one block
                assert fig["in_block"] <= A.PASS_HEADS, fig


def test_shell_windows():
    """The equal-distance shell in far_first order: in the sparse window the 64 nearest lie inside
    the shell (it is the 256 nearest that reach it) and no block holds more than 1024 points; in
    the dense one the shell is among the 64 nearest and a block gets more survivors than its
    buffer holds."""
    cg = A.cgrid(A.KNN_GRID)
    x, y = A.shell_window(False)
    assert cref.knn_pp(cg, x, y, A.Q[0], A.Q[1], A.KNN_R, 64)[1][-1] < 0.029
    assert cref.knn_pp(cg, x, y, A.Q[0], A.Q[1], A.KNN_R, 256)[1][-1] > 0.0299
    assert np.bincount(A.knn_block_of(len(x))).max() < A.PASS_CAP
    x, y = A.shell_window(True)
    wd = cref.knn_pp(cg, x, y, A.Q[0], A.Q[1], A.KNN_R, 64)[1]
    assert abs(wd[-1] - 0.001) < 1e-12
    near = np.hypot(x - A.Q[0], y - A.Q[1]) < 0.0010001   # at or below any bound T >= the 64th distance
    assert near.sum() > 8 * 1024 and np.bincount(A.knn_block_of(len(x))).min() > A.PASS_CAP


@pytest.mark.parametrize("n", A.RANGE_SIZES)
@pytest.mark.parametrize("approximate", [False, True])
def test_range_windows_reach_their_shapes(n, approximate):
    x, y, hits = A.range_base(n, approximate)
    for shape in A.RANGE_SHAPES + ("shuffled",):
        p = A.range_perm(n, shape, approximate)
        assert A.is_permutation(p, n)
        want = cref.range_pp(A.cgrid(100), x[p], y[p], A.Q[0], A.Q[1], 0.5, approximate).astype(np.int64)
        assert len(want) == len(hits)
        ok, fig = A.range_shape_ok(n, shape, want)
        assert ok == (shape != "shuffled"), (shape, fig)


def test_set_mode_windows():
    """Early reservation: in the all-hit window of 5 * 2^20 + 77 points every wave of a 256-CU
    launch collects 1280 hits or more; below 2^20 points a wave has one iteration and can collect
    256 at most (the gap).  The crafted window: the layout of arrivals.set_crafted_window, replayed
    by the mirror of range_set's bookkeeping."""
    n, cus = A.SET_N, 256
    nb, W, iters = A.range_set_geometry(n, cus)
    assert (iters // W) * A.PTS_ITER >= A.SET_RUN
    assert all(-(-A.range_set_geometry(m, cus)[2] // A.range_set_geometry(m, cus)[1]) == 1 for m in (70_001, 300_000, 1 << 20))
    x, y, wa, kinds = A.set_crafted_window(cus)
    cg = A.cgrid(A.SET_BAND_GRID)
    want = cref.range_pp(cg, x, y, A.Q[0], A.Q[1], A.SET_BAND_R)
    assert np.array_equal(np.flatnonzero(kinds > 0), want)   # band points: the oracle's dist <= r holds
    band = np.flatnonzero(kinds == 2)
    d = np.array([cref.hypot(A.Q[0] - x[i], A.Q[1] - y[i]) for i in band])
    assert len(band) == 128 and (d <= A.SET_BAND_R).all() and (A.SET_BAND_R - d <= A.SET_BAND_R * 2.0 ** -45).all()
    peak, early, staged, held = A.range_set_wave_trace(A.set_wave_kinds(kinds, n, cus, wa))
    assert (peak, early) == (1280, 1) and staged[4] == 63 and held[4] == 961
    peak, early, staged, held = A.range_set_wave_trace(A.set_wave_kinds(kinds, n, cus, 0))
    assert (peak, early) == (1163, 1) and staged[5] == 63 and held[5] == 1023
    peak, early, _, _ = A.range_set_wave_trace(A.set_wave_kinds(kinds, n, cus, 7))   # an ordinary wave
    assert (peak, early) == (1024, 1)


def test_set_mode_direct_hits_lie_in_the_guaranteed_box():
    """The crafted window's kinds by the planner's boxes (geohip_debug_classify, host code): direct
    hits inside G, band points inside C and not G, misses in neither."""
    from spatialflink_amd import _abi
    x, y, _, kinds = A.set_crafted_window(256)
    ag = _abi.make_grid(A.BJ[0], A.BJ[2], (A.BJ[1] - A.BJ[0]) / A.SET_BAND_GRID, A.SET_BAND_GRID)
    sel = np.concatenate([np.flatnonzero(kinds != 1), np.arange(0, len(x), 97)])
    cls = _abi.debug_classify(ag, A.Q[0], A.Q[1], A.SET_BAND_R, x[sel], y[sel])
    k = kinds[sel]
    assert ((cls[k == 1] & 1) == 1).all() and ((cls[k == 2] & 3) == 2).all() and (cls[k == 0] == 0).all()
    xmin, xmax, ymin, ymax = x[kinds == 1].min(), x[kinds == 1].max(), y[kinds == 1].min(), y[kinds == 1].max()
    corners = _abi.debug_classify(ag, A.Q[0], A.Q[1], A.SET_BAND_R, np.array([xmin, xmin, xmax, xmax]),
                                  np.array([ymin, ymax, ymin, ymax]))
    assert ((corners & 1) == 1).all()   # G is a box: every direct hit lies between these corners


def test_join_windows():
    dx, dy, qx, qy = A.join_base()
    cg = A.cgrid(A.JOIN_GRID)
    for o in A.JOIN_DATA_ORDERS:
        p = A.order_perm(o, dx, dy, cg)
        assert A.is_permutation(p, len(dx))
        assert binning_shape(dx[p], dy[p])[3] > 1024, o   # several kJbRound rounds of one tile in one segment
    p = A.order_perm("shuffled", dx, dy, cg)
    assert binning_shape(dx[p], dy[p])[3] <= 1024        # the gap
    for o in A.JOIN_QUERY_ORDERS:
        assert A.is_permutation(A.order_perm(o, qx, qy, cg), len(qx))


@pytest.mark.parametrize("name", A.PPOLY_SETS)
def test_ppoly_windows(name):
    pr, off, vx, vy = A.ppoly_polygons(name)
    x, y = A.ppoly_base(name)
    cg = A.cgrid(A.PPOLY_GRID)
    n = len(x)
    pairs = cref.range_ppoly(cg, x, y, off, vx, vy, A.PPOLY_R, False, pr)
    assert len(pairs) > 5000
    # the control: no chunk is dense in hits, and every chunk's 4096 points lie in over 3500 cells
    assert A.chunk_share(n, np.unique(pairs[:, 1])).max() < 0.2
    assert A.chunk_cells(*A.cells(cg, x, y)) > 3500
    for order in A.PPOLY_ORDERS:
        p = A.ppoly_perm(name, order)
        assert A.is_permutation(p, n)
        got = cref.range_ppoly(cg, x[p], y[p], off, vx, vy, A.PPOLY_R, False, pr)
        assert len(got) == len(pairs)
        share = A.chunk_share(n, np.unique(got[:, 1]))
        if order == "inside_first":
            assert share[0] == 1.0 and share[1] == 1.0 and share[-1] == 0.0
        else:   # some chunk's points share cells: two or more per cell where the control has one
            cx, cy = A.cells(cg, x[p], y[p])
            assert order != "cell_sorted" or (np.diff(cx * 100000 + cy) >= 0).all()
            assert A.chunk_cells(cx, cy) < 2200, (order, A.chunk_cells(cx, cy))


def test_ppoly_edge_window_overflows_the_first_buffer():
    off, vx, vy, x, y = A.ppoly_edge_window()
    cg = A.cgrid(A.PPOLY_GRID)
    pairs = cref.range_ppoly(cg, x, y, off, vx, vy, A.PPOLY_R)
    head = A.ppoly_candidates_lower_bound(cg, x, y, pairs, len(off) - 1, upto=A.EDGE_HEAD)
    assert head >= A.EDGE_HEAD > A.ppoly_first_ccap(len(x)) == 65536
    assert set(range(A.EDGE_HEAD)) <= set(pairs[:, 1].tolist())    # the head: within r of a ring, every point
    # the control: the same points shuffled put about a third of them in any stretch of 70000
    p = A.shuffled(len(x), 1)
    pairs = cref.range_ppoly(cg, x[p], y[p], off, vx, vy, A.PPOLY_R)
    assert A.ppoly_candidates_lower_bound(cg, x[p], y[p], pairs, len(off) - 1, upto=A.EDGE_HEAD) < 65536


def test_knn_ppoly_windows():
    _, off, vx, vy = A.ppoly_polygons("stars40")
    x, y = A.ppoly_base("stars40")
    v1x, v1y = vx[:int(off[1])], vy[:int(off[1])]
    cg = A.cgrid(A.PPOLY_GRID)
    last = (len(x) - 1) // A.STREAM_CHUNK
    for k in A.KNN_PPOLY_KS:
        for chunk in (0, 7, last):
            p = A.knn_ppoly_perm(x, y, v1x, v1y, k, chunk)
            assert A.is_permutation(p, len(x))
            wi, wd = cref.knn_ppoly(cg, x[p], y[p], v1x, v1y, 0.02, k)
            assert len(wi) == k and (wi // A.STREAM_CHUNK == chunk).all()
        wi, _ = cref.knn_ppoly(cg, x, y, v1x, v1y, 0.02, k)
        assert k == 1 or len(np.unique(wi // A.STREAM_CHUNK)) > 1   # the control
