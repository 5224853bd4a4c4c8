"""Plain-Python restatement of PointPointTJoinQuery's window form (test infrastructure; shares no
code with the product).  Paths relative to the reference's src/main/java/GeoFlink:

  trajectories  spatialOperators/tJoin/TJoinQuery.java:158-192: both streams keyBy(objID) (a null objID
                is Flink's null key, traj_ref.NullKeyError); GenerateWindowedTrajectory emits a
                LineString only for MORE than one point (:184).
  replication   TJoinQuery.java:195-211: every query point once per cell of
                uGrid.getNeighboringCells(joinDistance, q) (UniformGrid.java:261-293, restate.
                UniformGrid.neighboring_cells: r == 0 is every cell, candidate layers <= 0 exits, the
                square wraps as Java ints do and never ends at Integer.MAX_VALUE).
  join          tJoin/PointPointTJoinQuery.java:213-240: where(p.gridID).equalTo(q.gridID) on the
                "%05d%05d" strings, kept when DistanceFunctions.getPointPointEuclideanDistance(p.x, p.y,
                q.x, q.y) <= joinDistance (restate.pp_euclid: sqrt(dy*dy + dx*dx), not JTS distance).
  reduction     :246-288: keyBy(e.f0.objID); per key the first tuple's ordinary point and a HashMap
                query objID -> the query point of the largest timestamp; one tuple per map entry.
  back-joins    :293-337: with the ordinary trajectories on e.f0.objID, then with the query
                trajectories on e.f1.objID; a tuple whose objID has no trajectory finds no partner.

``window_literal`` is that pipeline stage by stage, with the join tuples in any order it is given;
``window_set`` is the order-free definition the library implements: the set of (objID a, objID b).
"""
from __future__ import annotations

import restate as R
import traj_ref


def small_windows(f, seed, na=300, nb=100, nta=12, ntb=12, specials=True):
    """(ax, ay, a_ids, bx, by, b_ids): an ordinary and a query window on frame ``f`` (frames.Frame)
    for the parity tests.  Points uniform over the grid, just outside it, on cell edges and corners
    (the grid's own upper edge among them); with ``specials`` NaN coordinates on both sides, +-inf
    and a cell index past 99999 on the ordinary side only (a query point there is an error case)
    and a query point 12 and 1000 cells left of the grid (keys with a '-').  A fifth of the query
    points coincide with ordinary points (the r == 0 hits).  objIDs "a0".."a<nta-1>" / "b0".. at random, plus:
    "soloA" / "soloB", one point each, coincident with a point of the other window (they join and
    are dropped), and "twinA" / "twinB", two identical points each (kept)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    l, n = f.cell_len, f.n
    L = n * l

    def draw(m):
        kind = rng.integers(0, 10, m)
        x = f.min_x + rng.uniform(0, L, m)
        y = f.min_y + rng.uniform(0, L, m)
        out = kind == 6  # within 1.5 cells of the grid, most of them outside it
        x = np.where(out, f.min_x + rng.choice([-1.0, 1.0], m) * rng.uniform(0, 1.5 * l, m) + rng.choice([0.0, L], m), x)
        edge = kind >= 7  # exact lattice values min + k l on one or both axes, k = n included
        kx, ky = rng.integers(0, n + 1, m), rng.integers(0, n + 1, m)
        x = np.where(edge, f.min_x + kx * l, x)
        y = np.where(edge & (kind >= 8), f.min_y + ky * l, y)
        return x, y

    ax, ay = draw(na - 4)
    bx, by = draw(nb - 4)
    k = max(1, (nb - 4) // 5)
    pick = rng.choice(na - 4, k, replace=False)
    bx[:k], by[:k] = ax[pick], ay[pick]
    a_ids = ["a%d" % t for t in rng.integers(0, nta, na - 4)]
    b_ids = ["b%d" % t for t in rng.integers(0, ntb, nb - 4)]
    if specials:
        nan, inf = float("nan"), float("inf")
        sa = [(nan, ay[0]), (ax[1], nan), (inf, ay[2]), (ax[3], -inf), (f.min_x + 123456.5 * l, ay[4])]
        for j, (x, y) in enumerate(sa):
            ax[5 + j], ay[5 + j] = x, y
        sb = [(nan, by[k]), (bx[k + 1], nan), (f.min_x - 11.5 * l, by[k + 2]), (bx[k + 3], f.min_y - 999.5 * l)]
        for j, (x, y) in enumerate(sb):
            bx[k + 4 + j], by[k + 4 + j] = x, y
    inside = [i for i in range(na - 4) if f.min_x <= ax[i] < f.min_x + L and f.min_y <= ay[i] < f.min_y + L]
    p0, p1 = inside[0], inside[1]
    # soloB and twinB sit on ordinary points; soloA and twinA on a query point that sits on one
    bx = np.concatenate([bx, [ax[p0], ax[p1], ax[p1], ax[p0]]])
    by = np.concatenate([by, [ay[p0], ay[p1], ay[p1], ay[p0]]])
    b_ids += ["soloB", "twinB", "twinB", b_ids[0]]
    ax = np.concatenate([ax, [ax[p0], ax[p1], ax[p1], ax[p0]]])
    ay = np.concatenate([ay, [ay[p0], ay[p1], ay[p1], ay[p0]]])
    a_ids += ["soloA", "twinA", "twinA", a_ids[p0]]
    pa, pb = rng.permutation(na), rng.permutation(nb)
    return (ax[pa], ay[pa], [a_ids[i] for i in pa], bx[pb], by[pb], [b_ids[i] for i in pb])


def trajectories(xs, ys, ids):
    """{objID: [(x, y), ...]} of the windowed trajectories: keyBy(objID), more than one point."""
    g = traj_ref.group(list(ids))  # every point is keyed: a null objID raises
    out = {}
    for t, oid in enumerate(g["ids"]):
        pts = g["perm"][g["traj_off"][t]:g["traj_off"][t + 1]]
        if len(pts) > 1:
            out[oid] = [(float(xs[p]), float(ys[p])) for p in pts]
    return out


def join_tuples(grid, ax, ay, bx, by, r):
    """The filtered output of the grid-keyed window join: [(ordinary index, query index)]."""
    repl = {}
    for qi, (qx, qy) in enumerate(zip(bx, by)):
        for key in grid.neighboring_cells(r, grid.key(float(qx), float(qy))):
            repl.setdefault(key, []).append(qi)
    out = []
    for pi, (px, py) in enumerate(zip(ax, ay)):
        px, py = float(px), float(py)
        for qi in repl.get(grid.key(px, py), ()):
            if R.pp_euclid(px, py, float(bx[qi]), float(by[qi])) <= r:
                out.append((pi, qi))
    return out


def window_literal(grid, ax, ay, a_ids, bx, by, b_ids, r, b_ts=None, order=None):
    """[(objID a, objID b)] as the pipeline emits them.  ``order``: a permutation of the join tuples
    (the order in which Flink hands them to the keyed window function is not defined); ``b_ts``: the
    query points' timestamps (default: their index), which pick the point the map keeps."""
    traj_a = trajectories(ax, ay, a_ids)
    traj_b = trajectories(bx, by, b_ids)
    b_ts = list(range(len(bx))) if b_ts is None else b_ts
    tuples = join_tuples(grid, ax, ay, bx, by, r)
    if order is not None:
        assert sorted(order) == list(range(len(tuples)))
        tuples = [tuples[k] for k in order]
    keyed = {}
    for pi, qi in tuples:
        keyed.setdefault(a_ids[pi], []).append((pi, qi))
    reduced = []  # (firstPoint, the kept query point) per (ordinary objID, query objID)
    for key, inp in keyed.items():
        second = {}
        first = None
        for pi, qi in inp:
            if first is None:
                first = pi
            old = second.get(b_ids[qi])
            if old is not None:
                if b_ts[qi] > b_ts[old]:
                    second[b_ids[qi]] = qi
            else:
                second[b_ids[qi]] = qi
        for qi in second.values():
            reduced.append((first, qi))
    with_a = [(a_ids[pi], qi) for pi, qi in reduced if a_ids[pi] in traj_a]
    return [(a, b_ids[qi]) for a, qi in with_a if b_ids[qi] in traj_b]


def window_set(grid, ax, ay, a_ids, bx, by, b_ids, r):
    """{(objID a, objID b)}: both objIDs own more than one point of their window and some ordinary
    point of a lies in a neighbouring cell of some query point of b within r of it."""
    if any(o is None for o in list(a_ids) + list(b_ids)):
        raise traj_ref.NullKeyError("null objID reaches keyBy")
    count_a, count_b = {}, {}
    for o in a_ids:
        count_a[o] = count_a.get(o, 0) + 1
    for o in b_ids:
        count_b[o] = count_b.get(o, 0) + 1
    a_keys = [grid.key(float(x), float(y)) for x, y in zip(ax, ay)]
    out = set()
    for qi, (qx, qy) in enumerate(zip(bx, by)):
        qx, qy = float(qx), float(qy)
        cells = grid.neighboring_cells(r, grid.key(qx, qy))  # raises for every query point, paired or not
        for pi, key in enumerate(a_keys):
            if key in cells and R.pp_euclid(float(ax[pi]), float(ay[pi]), qx, qy) <= r:
                if count_a[a_ids[pi]] > 1 and count_b[b_ids[qi]] > 1:
                    out.add((a_ids[pi], b_ids[qi]))
    return out
