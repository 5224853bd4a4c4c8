"""GPU: keyBy(objID) grouping (geohip_traj_group), windowed TStats (geohip_tstats) and TFilter
(geohip_traj_gather / geohip_traj_selected) against tests/traj_ref.py, the plain-Python restatement
of PointTStatsQuery.java:76-92, TStatsQuery.java:148-189 and PointTFilterQuery.java:62-118.

Integer arrays are compared exactly; spatialLength and avgSpeed by their bits, except that NaN
matches NaN (Java exposes no payload of 0.0 / 0).
"""
from __future__ import annotations

import math
import random

import numpy as np
import pytest

import traj_ref as R
from spatialflink_amd import _abi, synth
from spatialflink_amd.operators import (PointTFilterQuery, PointTStatsQuery, QueryConfiguration, QueryType,
                                        TrajectoryWindow)

pytestmark = pytest.mark.gpu

# objID forms: lengths 1..40 across the 8- and 16-byte boundaries, pairs that differ in the last
# byte only, strict prefixes, multi-byte UTF-8
SPECIAL_IDS = ["a", "ab", "abc", "veh-1", "veh-2", "x" * 8, "x" * 7 + "y", "x" * 9, "x" * 16, "x" * 15 + "y",
               "x" * 17, "é", "éa", "日本語", "日本誤", "long" * 10, "long" * 9 + "lonh", "", "b" * 39 + "c",
               "b" * 39 + "d"]


def make_ids(T):
    ids = list(SPECIAL_IDS[:T])
    k = 0
    while len(ids) < T:
        s = f"id{k}"
        ids.append(s + "_" * ((k % 40 + 1) - len(s)))  # lengths 1..40 where the number leaves room
        k += 1
    assert len(set(ids)) == T
    return ids


def make_window(n, T, seed, null_share=0.0):
    """n objIDs over T distinct strings (each occurs when n >= T), interleaved; some null."""
    rng = random.Random(seed)
    ids = make_ids(T)
    oids = [ids[rng.randrange(T)] for _ in range(n)] if T else []
    if n >= T:
        for slot, k in zip(rng.sample(range(n), T), range(T)):
            oids[slot] = ids[k]
    if null_share:
        oids = [None if rng.random() < null_share else o for o in oids]
    return oids, ids


def dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def dev_strings(strings):
    text, off = _abi.pack_strings(strings)
    return dev(text, np.uint8), dev(off.view(np.int64), np.int64)


def u32(t):
    return t.cpu().numpy().view(np.uint32).tolist()


def check_group(got, want):
    assert got["n_traj"] == len(want["traj_first"])
    assert got["n_sel"] == len(want["perm"])
    assert u32(got["traj_of"]) == want["traj_of"]
    assert u32(got["traj_first"]) == want["traj_first"]
    assert u32(got["traj_off"]) == want["traj_off"]
    assert u32(got["perm"]) == want["perm"]


def group_both(ctx, oids, id_set=(), **kw):
    ot, oo = dev_strings(oids)
    st = so = None
    if id_set:
        st, so = dev_strings(sorted(id_set))
    got = ctx.traj_group(ot, oo, st, so, **kw)
    want = R.group(oids, id_set)
    check_group(got, want)
    return got, want


def same_double(a: float, b: float) -> bool:
    return (math.isnan(a) and math.isnan(b)) or np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


def check_tstats(ctx, x, y, ts, got_group, want_group):
    sp, tl, av = ctx.tstats(dev(x, np.float64), dev(y, np.float64), dev(ts, np.int64), got_group["perm"],
                            got_group["traj_off"])
    want = R.tstats(x, y, ts, want_group["perm"], want_group["traj_off"])
    sp, tl, av = sp.cpu().numpy(), tl.cpu().numpy(), av.cpu().numpy()
    assert len(sp) == len(tl) == len(av) == len(want)
    assert tl.tolist() == [w[1] for w in want]
    bad = [t for t, w in enumerate(want) if not (same_double(sp[t], w[0]) and same_double(av[t], w[2]))]
    assert not bad, (bad[:5], [(sp[t], av[t], want[t]) for t in bad[:5]])


def fuzz_columns(n, seed, ts_lo=-3, ts_hi=4, odd_share=0.02):
    """Coordinates with -0.0, +-Inf and NaN among them; timestamps from a small range so equal,
    zero, negative and out-of-order values are all common."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-10, 10, n), rng.uniform(-10, 10, n)
    odd = np.array([-0.0, 0.0, np.inf, -np.inf, np.nan, 1e308, -1e308, 5e-324])
    for col in (x, y):
        m = rng.random(n) < odd_share
        col[m] = odd[rng.integers(0, len(odd), int(m.sum()))]
    ts = rng.integers(ts_lo, ts_hi, n, dtype=np.int64)
    return x, y, ts


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 5000])
def test_group_and_tstats_shapes(ctx, n):
    """T in {1, 2, 64, 65, n} (one trajectory holding every point, and all distinct), empty set."""
    for T in sorted({t for t in (1, 2, 64, 65, n) if t <= n} or {0}):
        oids, _ = make_window(n, T, seed=1000 + n + T)
        got, want = group_both(ctx, oids)
        assert got["n_traj"] == T and got["n_sel"] == n
        x, y, ts = fuzz_columns(n, seed=n * 7 + T)
        check_tstats(ctx, x, y, ts, got, want)
        gx, gy, gt = ctx.traj_gather(dev(x, np.float64), dev(y, np.float64), got["perm"], dev(ts, np.int64))
        p = np.array(want["perm"], dtype=np.int64)
        assert np.array_equal(gx.cpu().numpy().view(np.uint64), x[p].view(np.uint64))
        assert np.array_equal(gy.cpu().numpy().view(np.uint64), y[p].view(np.uint64))
        assert np.array_equal(gt.cpu().numpy(), ts[p])


def test_selection_sets(ctx):
    oids, ids = make_window(257, 65, seed=7, null_share=0.1)
    rng = random.Random(3)
    subset = set(rng.sample(ids, 20))
    absent = {"nobody", "veh-3", "a" * 41, "日本", "x" * 18}
    for id_set in (subset, subset | absent, set(ids), set(ids) | absent, absent, {"a"}, {"ab"}):
        got, want = group_both(ctx, oids, id_set)
        assert u32(ctx.traj_selected(got["traj_of"])) == [i for i, t in enumerate(want["traj_of"]) if t != R.UNSELECTED]
    got, _ = group_both(ctx, oids, absent)
    assert got["n_traj"] == 0 and got["n_sel"] == 0
    # every objID null under a non-empty set: nothing is selected
    got, _ = group_both(ctx, [None] * 65, {"a"})
    assert got["n_traj"] == 0


def test_null_key_with_empty_set_is_an_argument_error(ctx):
    oids, _ = make_window(257, 65, seed=7)
    group_both(ctx, oids)
    oids[200] = None
    with pytest.raises(R.NullKeyError):
        R.group(oids)
    with pytest.raises(_abi.GeohipArgumentError):
        ctx.traj_group(*dev_strings(oids))


@pytest.mark.parametrize("mask", [0, 3])
def test_masked_hash_gives_the_same_grouping(ctx, mask):
    """Every string in one probe chain (mask 0) or four (mask 3): the byte compare decides."""
    oids, ids = make_window(257, 65, seed=11, null_share=0.05)
    for id_set in (set(ids), set(ids[::2]) | {"nobody"}):
        got, _ = group_both(ctx, oids, id_set, hash_mask=mask)
        plain, _ = group_both(ctx, oids, id_set)
        for key in ("traj_of", "traj_first", "traj_off", "perm"):
            assert u32(got[key]) == u32(plain[key])
    full, _ = make_window(257, 257, seed=12)
    group_both(ctx, full, hash_mask=mask)


def test_capacity(ctx):
    oids, _ = make_window(257, 65, seed=5)
    with pytest.raises(_abi.GeohipCapacityError) as e:
        ctx.traj_group(*dev_strings(oids), cap_traj=64)
    assert e.value.n_traj == 65
    check_group(ctx.traj_group(*dev_strings(oids), cap_traj=65), R.group(oids))


def test_tstats_known_answers(ctx):
    """The hand-computed cases of tests/test_traj_ref.py, one trajectory each, interleaved."""
    # interleave the cases but keep each case's own arrival order
    labels = [f"k{c}" for c, (_, pts, _) in enumerate(R.KNOWN) for _ in pts]
    random.Random(2).shuffle(labels)
    cursor = {f"k{c}": iter(pts) for c, (_, pts, _) in enumerate(R.KNOWN)}
    seq = [(k, next(cursor[k])) for k in labels]
    oids = [k for k, _ in seq]
    x = np.array([p[0] for _, p in seq])
    y = np.array([p[1] for _, p in seq])
    ts = np.array([p[2] for _, p in seq], dtype=np.int64)
    got, want = group_both(ctx, oids)
    sp, tl, av = (t.cpu().numpy() for t in ctx.tstats(dev(x, np.float64), dev(y, np.float64), dev(ts, np.int64),
                                                      got["perm"], got["traj_off"]))
    for t, key in enumerate(want["ids"]):
        name, _, (ws, wt, wa) = R.KNOWN[int(key[1:])]
        assert same_double(sp[t], ws) and tl[t] == wt and same_double(av[t], wa), name


def test_tstats_fuzz(ctx):
    """n = 5000 with small-range timestamps and odd coordinates, at trajectory counts that take the
    one-lane walk (<= 32 points), the wave walk, and many 64-point steps of it."""
    for T in (1, 2, 40, 100, 500, 5000):
        oids, _ = make_window(5000, T, seed=T)
        got, want = group_both(ctx, oids)
        x, y, ts = fuzz_columns(5000, seed=50 + T)
        check_tstats(ctx, x, y, ts, got, want)
    # plain data: finite coordinates, large timestamps with a share out of order, extremes mixed in
    w = synth.trajectories(5000, 7, seed=9)
    oids = [f"veh-{k}" for k in w["traj"]]
    got, want = group_both(ctx, oids)
    ts = w["ts"].copy()
    ts[::997] = R.INT64_MIN
    ts[5::1009] = R.INT64_MAX
    ts[7::499] = 0
    check_tstats(ctx, w["x"], w["y"], ts, got, want)


def test_tstats_path_thresholds(ctx):
    """Trajectory lengths on both sides of the one-lane / wave switch (32) and of the wave walk's
    64-point step, interleaved in one window."""
    lens = [1, 2, 31, 32, 33, 34, 63, 64, 65, 66, 127, 128, 129, 1023, 1024, 1025, 2049]
    oids = [f"t{k}" for k, m in enumerate(lens) for _ in range(m)]
    random.Random(4).shuffle(oids)
    n = len(oids)
    got, want = group_both(ctx, oids)
    assert sorted(b - a for a, b in zip(want["traj_off"], want["traj_off"][1:])) == lens
    for seed, (lo, hi) in enumerate([(-3, 4), (1, 1000), (-2, 3)]):
        x, y, ts = fuzz_columns(n, seed=seed, ts_lo=lo, ts_hi=hi, odd_share=0.0 if seed == 1 else 0.02)
        check_tstats(ctx, x, y, ts, got, want)


def test_tstats_wave_walk_edge_patterns(ctx):
    """Where the re-initialisation quirks decide the result on the wave walk (> 32 points): every
    4-point timestamp prefix over {-2..2} before a 40-point tail, and every 3-point suffix after a
    40-point head, one trajectory each."""
    import itertools
    rng = np.random.default_rng(8)
    vals = (-2, -1, 0, 1, 2)
    seqs = [list(p) + rng.integers(-2, 3, 40).tolist() for p in itertools.product(vals, repeat=4)]
    seqs += [rng.integers(-2, 1, 40).tolist() + list(p) for p in itertools.product(vals, repeat=3)]
    # interleave the trajectories; each keeps its own sequence as its arrival order
    labels = np.array([k for k, q in enumerate(seqs) for _ in q])
    rng.shuffle(labels)
    cursor = [iter(q) for q in seqs]
    w_oids = [f"p{k}" for k in labels]
    w_ts = np.array([next(cursor[k]) for k in labels], dtype=np.int64)
    x, y, _ = fuzz_columns(len(w_oids), seed=3, odd_share=0.0)
    got, want = group_both(ctx, w_oids)
    for t, key in enumerate(want["ids"]):  # each trajectory kept its sequence
        p = want["perm"][want["traj_off"][t]:want["traj_off"][t + 1]]
        assert w_ts[p].tolist() == seqs[int(key[1:])]
    check_tstats(ctx, x, y, w_ts, got, want)


def test_tstats_rejects_a_bad_permutation(ctx):
    import torch
    oids, _ = make_window(65, 2, seed=1)
    got, _ = group_both(ctx, oids)
    x, y, ts = fuzz_columns(65, seed=1)
    perm = got["perm"].clone()
    perm[3] = 65
    with pytest.raises(_abi.GeohipArgumentError):
        ctx.tstats(dev(x, np.float64), dev(y, np.float64), dev(ts, np.int64), perm, got["traj_off"])
    off = got["traj_off"].clone()
    off[-1] = 66
    with pytest.raises(_abi.GeohipArgumentError):
        ctx.tstats(dev(x, np.float64), dev(y, np.float64), dev(ts, np.int64), got["perm"], off)
    assert torch.equal(perm[:3], got["perm"][:3])


def _csv_batch(n, T, seed):
    rng = random.Random(seed)
    ids = [f"veh-{k}" if k % 3 else f"bus {k}" for k in range(T)]
    recs, cols = [], []
    pos = {k: (rng.uniform(115.6, 117.5), rng.uniform(39.7, 41.0)) for k in ids}
    for i in range(n):
        k = ids[rng.randrange(T)]
        px, py = pos[k]
        px, py = px + rng.uniform(-1e-3, 1e-3), py + rng.uniform(-1e-3, 1e-3)
        pos[k] = (px, py)
        ts = 1611022449423 + 100 * i - (700 if rng.random() < 0.1 else 0)
        recs.append(f"{k},{ts},{px!r},{py!r}")
        cols.append((k, px, py, ts))
    return "\n".join(recs).encode(), cols


def test_operators_from_ingest(ctx):
    """ingest_trajectory + ingest_oid_compact -> PointTStatsQuery and PointTFilterQuery (both modes)."""
    import torch
    text, cols = _csv_batch(300, 12, seed=21)
    oids = [c[0] for c in cols]
    x, y = np.array([c[1] for c in cols]), np.array([c[2] for c in cols])
    ts = np.array([c[3] for c in cols], dtype=np.int64)
    dtext = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    got = ctx.ingest_trajectory(_abi.make_ingest_spec(_abi.FMT_CSV, ",", 2, 3, 1, 0), dtext, None, None,
                                with_ts=True, with_cell=False, with_oid=True)
    assert np.array_equal(got["x"].cpu().numpy().view(np.uint64), x.view(np.uint64))
    assert np.array_equal(got["ts"].cpu().numpy(), ts)
    oid_text, oid_off = ctx.ingest_oid_compact(dtext, got["oid"])
    window = TrajectoryWindow(got["x"], got["y"], got["ts"], oid_text, oid_off)
    for id_set in ((), {"veh-1", "bus 3", "veh-99"}):
        want = R.group(oids, id_set)
        stats = PointTStatsQuery(QueryConfiguration(QueryType.WindowBased), ctx=ctx).run(window, id_set)
        ref = R.tstats(x, y, ts, want["perm"], want["traj_off"])
        assert [s[0] for s in stats] == want["ids"]
        for (_, s, t, a), (ws, wt, wa) in zip(stats, ref):
            assert same_double(s, ws) and t == wt and same_double(a, wa)
        lines = PointTFilterQuery(QueryConfiguration(QueryType.WindowBased), ctx=ctx).run(window, id_set)
        assert [l[0] for l in lines] == want["ids"]
        for t, (_, xy) in enumerate(lines):
            p = want["perm"][want["traj_off"][t]:want["traj_off"][t + 1]]
            assert np.array_equal(xy[:, 0].view(np.uint64), x[p].view(np.uint64))
            assert np.array_equal(xy[:, 1].view(np.uint64), y[p].view(np.uint64))
        idx = PointTFilterQuery(QueryConfiguration(QueryType.RealTime), ctx=ctx).run(window, id_set)
        assert u32(idx) == [i for i, t in enumerate(want["traj_of"]) if t != R.UNSELECTED]


def test_repeat_calls_on_one_ctx(ctx):
    """A large window, then a smaller one with other ids, then the first again: nothing of a call's
    table or scratch may reach the next."""
    big, _ = make_window(5000, 65, seed=31)
    small = [f"other{i % 5}" for i in range(63)]
    for oids, id_set in ((big, ()), (small, ()), (big, {"a", "veh-1"}), (small, {"other2"}), (big, ())):
        got, want = group_both(ctx, oids, id_set)
        x, y, ts = fuzz_columns(len(oids), seed=len(oids))
        check_tstats(ctx, x, y, ts, got, want)
