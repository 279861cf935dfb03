"""Neighbour-exact GPU tests of the streamed k-NN form on hard data, through every tile kernel.

At the full budget (p_work = 1.0) the graph must BE the k-NN graph of the float32 rows: streamed_cases.knn_violations (listed
pairs real, no index twice, nothing closer left out beyond the rounding of float32 differences) reports nothing, on every data
family of streamed_cases.FAMILIES, on every route of the dispatch -- and every case asserts which kernel ran, so a dispatch
change cannot move a case off the route it is there for.

Routes (launch_by_dim, ann_stream_launch_knnh, ann_stream_launch_knnbf, ann_stream_launch_knnbk of csrc/):
  two-stage     padded dimension 128, n_neighbors <= 15            k_st_knnh behind k_st_knnbf's warm-up (kind 1, two_stage)
  split         padded dimension <= 128, n_neighbors <= 31         k_st_knnbf (kind 1; K + 2 kept columns fill its 32-entry lists)
  k-blocked     padded dimension 256 .. 1024, n_neighbors <= 63    knnbk.hip (kind 1)
  exact-f32     up to 256 dimensions, n_neighbors 32 .. 128        k_st_knn (kind 0), two workgroups per row tile beyond 65;
                                                                   k_st_guard_expanded + k_st_repair make it exact on hard data

Found with these tests and fixed with them: the exact-f32 route on every ill-conditioned family (no guard at all), and the split
kernels' guard on one row in 1777 of `anisotropic` and of `far_clusters` at d = 20, n_neighbors = 8 (the error measured on K + 2
kept entries alone was too small a sample: it has an a-priori floor now).
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))
import streamed_cases as sc   # noqa: E402

ALL_ROWS_MAX = 4000

# (route, d, n_neighbors, n, expected kind, expected two_stage)
ROUTES = [
    ("two-stage", 128, 15, 1777, 1, True),
    ("two-stage", 100, 15, 1777, 1, True),
    ("split-small", 20, 8, 1777, 1, False),
    ("split-small", 64, 31, 1777, 1, False),
    ("split-128-long", 128, 16, 1777, 1, False),
    ("split-128-long", 128, 31, 1777, 1, False),
    ("k-blocked", 300, 10, 1777, 1, False),
    ("k-blocked", 1024, 63, 1601, 1, False),
    ("exact-f32", 64, 40, 1777, 0, False),
    ("exact-f32", 256, 64, 1777, 0, False),
    ("exact-f32-halves", 128, 100, 1777, 0, False),
]


def _rows_of(n, seed=0):
    return np.arange(n) if n <= ALL_ROWS_MAX else np.sort(np.random.default_rng(seed).choice(n, 600, replace=False))


def _kernels(sa):
    kind, flagged = sa._engine.stream_last_kernel(with_guard=True)
    two_stage, repaired = sa._engine.stream_last_tile_kernels()
    return kind, flagged, two_stage, repaired


def _assert_exact(X, idx, dist, nn, what, rows=None, Q=None, complete=True):
    rows = _rows_of(len(X) if Q is None else len(Q)) if rows is None else rows
    bad = sc.knn_violations(X, rows, idx[rows], dist[rows], nn, sc.gamma_of(sc.padded_dim(X.shape[1])), Q=Q, complete=complete)
    print("%s: %d of %d rows violate" % (what, len(bad), len(rows)))
    assert bad == [], "%s: %d of %d rows, first %s" % (what, len(bad), len(rows), bad[:4])


@pytest.mark.parametrize("name", sorted(sc.FAMILIES))
@pytest.mark.parametrize("route,d,nn,n,kind,two_stage", ROUTES, ids=["%s-d%d-k%d" % r[:3] for r in ROUTES])
def test_routes_by_families_are_neighbour_exact(route, d, nn, n, kind, two_stage, name):
    from annchor_amd.streamed import StreamedAnnchor

    X = sc.family(name, n, d)
    sa = StreamedAnnchor(X, n_anchors=8, n_neighbors=nn, p_work=1.0).fit()
    got = _kernels(sa)
    print("%s d=%d k=%d %s: kernel %d, two-stage %s, flagged %d, repaired %s" % (route, d, nn, name, got[0], got[2], got[1], got[3]))
    assert (got[0], got[2]) == (kind, two_stage), "dispatch moved: %s" % (got,)
    if name == "far_clusters" and not two_stage:
        # the guard + repair must really have been the thing tested (the two-stage kernel filters rigorously and needs neither)
        assert got[1] > 0 and got[3], got
    if kind == 0 and name in sc.ILL_CONDITIONED:
        assert got[1] > 0 and got[3], got   # the expanded form on uncentred rows cannot resolve these: flagged, repaired
    idx, dist = sa.neighbor_graph
    _assert_exact(X, idx, dist, nn, "%s %s" % (route, name))


@pytest.mark.parametrize("name", ["shift_1e3", "shift_1e5", "far_clusters"])
@pytest.mark.parametrize("d,nn,kind", [(128, 15, 1), (20, 31, 1), (300, 10, 1), (64, 40, 0), (128, 100, 0)])
def test_other_entry_points_on_ill_conditioned_data(monkeypatch, d, nn, kind, name):
    """The sharded entry point on one rank (its early stop switched off: at the full budget it runs no join pass that would pick
    up what the stop left), the Annchor front end, and queries with perturbed rows at 5, 40 and 100 neighbours."""
    from annchor_amd import Annchor
    from annchor_amd.streamed import StreamedAnnchor

    monkeypatch.setenv("ANNCHOR_ST_EARLY_WINDOW", "0")
    n = 1777
    X = sc.family(name, n, d)
    sa = StreamedAnnchor(X, n_anchors=8, n_neighbors=nn, p_work=1.0, force_exchange=True).fit()
    assert sa._engine.stream_last_kernel() == kind
    _assert_exact(X, *sa.neighbor_graph, nn, "sharded entry point %s d=%d k=%d" % (name, d, nn))
    ann = Annchor(X, "euclidean", n_anchors=8, n_neighbors=nn, p_work=1.0, streamed=True).fit()
    assert ann._streamed is not None and ann._engine.stream_last_kernel() == kind
    _assert_exact(X, *ann.neighbor_graph, nn, "Annchor(streamed=True) %s d=%d k=%d" % (name, d, nn))
    rng = np.random.default_rng(4)
    qr = rng.choice(n, 300, replace=False)
    step = np.abs(X[qr]).max() * 2.0 ** -12 + np.float32(0.01) * X[qr].std()
    Q = (X[qr] + step * rng.standard_normal((300, d))).astype(np.float32)
    for qn in (5, 40, 100) if d <= 256 else (5, 40):
        qi, qd = sa.query(Q, nn=qn, p_work=1.0)
        _assert_exact(X, qi, qd, qn, "query nn=%d %s d=%d" % (qn, name, d), rows=np.arange(300), Q=Q)


@pytest.mark.parametrize("name", ["plain", "lattice"])
@pytest.mark.parametrize("d", [1, 2, 31, 32, 33, 65, 127, 129, 255, 256, 257, 1023, 1024])
def test_dimension_edges(d, name):
    from annchor_amd.streamed import StreamedAnnchor

    n, nn = 900, 10
    X = sc.family(name, n, d)
    sa = StreamedAnnchor(X, n_anchors=6, n_neighbors=nn, p_work=1.0).fit()
    assert sa._engine.stream_last_kernel() == 1
    _assert_exact(X, *sa.neighbor_graph, nn, "d=%d %s" % (d, name))


@pytest.mark.parametrize("name", ["plain", "lattice"])
@pytest.mark.parametrize("n", [10, 11, 127, 128, 129, 257])
def test_fewer_points_than_a_few_tiles(n, name):
    """n = n_neighbors lists every other point; 11 = k + 1; one tile less one, one tile, one tile and a row, two and a row."""
    from annchor_amd.streamed import StreamedAnnchor

    for d, nn in ((20, 10), (64, 10), (300, 10)) + (((64, 40),) if n > 40 else ()):
        X = sc.family(name, n, d)
        sa = StreamedAnnchor(X, n_anchors=4, n_neighbors=nn, p_work=1.0).fit()
        _assert_exact(X, *sa.neighbor_graph, nn, "n=%d d=%d k=%d %s" % (n, d, nn, name))
    with pytest.raises(Exception):
        StreamedAnnchor(sc.family(name, n, 20), n_anchors=4, n_neighbors=n + 1, p_work=1.0).fit()   # more neighbours than points


@pytest.mark.parametrize("name", ["plain", "lattice"])
@pytest.mark.parametrize("d,nn", [(64, v) for v in (2, 15, 16, 17, 31, 32, 33, 34, 63, 64, 65, 66, 128)] + [(300, 62), (300, 63)])
def test_list_capacity_edges(d, nn, name):
    """Every list-capacity boundary of launch_knn / launch_knnbf / KnnHalf; the kernel each side of a boundary takes."""
    from annchor_amd.streamed import StreamedAnnchor

    n = 1300
    X = sc.family(name, n, d)
    sa = StreamedAnnchor(X, n_anchors=6, n_neighbors=nn, p_work=1.0).fit()
    assert sa._engine.stream_last_kernel() == (1 if nn <= 31 or d > 256 else 0)
    _assert_exact(X, *sa.neighbor_graph, nn, "d=%d k=%d %s" % (d, nn, name))


def test_refused_combinations():
    from annchor_amd.streamed import StreamedAnnchor

    with pytest.raises(Exception):
        StreamedAnnchor(sc.family("plain", 1300, 64), n_anchors=6, n_neighbors=129, p_work=1.0).fit()   # > 128
    with pytest.raises(Exception):
        StreamedAnnchor(sc.family("plain", 1300, 300), n_anchors=6, n_neighbors=64, p_work=1.0).fit()   # > 63 beyond 256 dimensions


@pytest.mark.parametrize("name", ["shift_1e3", "far_clusters"])
@pytest.mark.parametrize("nn", [15, 40])
def test_budgeted_builds_stay_honest_on_hard_data(nn, name):
    """p_work = 0.25 at N = 40 000: every LISTED pair is real (distance, self column, no index twice, ascending), the evaluation
    count stays within the budget, two builds agree bit for bit.  No recall bar: the geometry of these families differs from
    the plain one and nothing has measured it; the recall against the full-budget query is printed for the record."""
    from annchor_amd import compare_neighbor_graphs
    from annchor_amd.streamed import StreamedAnnchor

    n, d = 40000, 64
    X = sc.family(name, n, d)
    nt = (n + 127) // 128
    sa = StreamedAnnchor(X, n_anchors=16, n_neighbors=nn, p_work=0.25).fit()
    assert sa.tile_evals <= int(np.ceil(0.25 * nt)) * nt
    idx, dist = sa.neighbor_graph
    _assert_exact(X, idx, dist, nn, "budgeted %s k=%d" % (name, nn), rows=_rows_of(n), complete=False)
    sb = StreamedAnnchor(X, n_anchors=16, n_neighbors=nn, p_work=0.25).fit()
    assert np.array_equal(idx, sb.neighbor_graph[0]) and np.array_equal(dist, sb.neighbor_graph[1])
    rows = _rows_of(n, seed=2)[:300]
    ti, td = sa.query(X[rows], nn=nn, p_work=1.0)
    err = compare_neighbor_graphs((ti, td), (idx[rows], dist[rows]), nn)
    print("budgeted %s k=%d: recall %.4f against the full-budget query, kernel %s" % (name, nn, 1 - err / (len(rows) * float(nn)), _kernels(sa)))


# (route, d, n_neighbors, expected kind): the join-pass form of every list capacity of k_st_knnbf and k_st_knnbk, and k_st_join
JOIN_ROUTES = [
    ("split-join", 20, 8, 1),
    ("split-join", 64, 25, 1),
    ("split-join", 128, 20, 1),
    ("k-blocked-join", 300, 10, 1),
    ("k-blocked-join", 300, 25, 1),
    ("k-blocked-join", 300, 62, 1),
    ("exact-f32-join", 64, 40, 0),
]


@pytest.mark.parametrize("name", ["plain", "far_clusters"])
@pytest.mark.parametrize("route,d,nn,kind", JOIN_ROUTES, ids=["%s-d%d-k%d" % r[:3] for r in JOIN_ROUTES])
def test_join_passes_on_every_route_list_real_pairs(route, d, nn, kind, name):
    """66 tiles are the fewest at which a budget leaves room for join passes (below 64 tile evaluations per row tile p_work is
    raised to 1): 64 evaluations per row tile, 48 in the tile phase, 8 gathered runs in each of two passes.  The passes must have
    run, on the tile phase's kernel; every LISTED pair is real (distance, self column, no index twice, ascending); the
    evaluations stay within the budget; two builds agree bit for bit."""
    from annchor_amd.streamed import StreamedAnnchor

    n = 8400
    X = sc.family(name, n, d)
    nt = (n + 127) // 128
    sa = StreamedAnnchor(X, n_anchors=12, n_neighbors=nn, p_work=0.9).fit()
    tiles, runs = sa._engine.stream_last_counts()
    got = _kernels(sa)
    print("%s d=%d k=%d %s: kernel %d, tile evaluations %d, join runs %d" % (route, d, nn, name, got[0], tiles, runs))
    assert got[0] == kind, "dispatch moved: %s" % (got,)
    assert runs > 0 and tiles + runs <= 64 * nt
    idx, dist = sa.neighbor_graph
    _assert_exact(X, idx, dist, nn, "joins %s %s" % (route, name), rows=_rows_of(n), complete=False)
    sb = StreamedAnnchor(X, n_anchors=12, n_neighbors=nn, p_work=0.9).fit()
    assert np.array_equal(idx, sb.neighbor_graph[0]) and np.array_equal(dist, sb.neighbor_graph[1])
