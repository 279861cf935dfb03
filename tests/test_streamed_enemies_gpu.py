"""The nearest-enemy graph of the streamed form (StreamedAnnchor.nearest_enemies, Annchor.get_nearest_enemies on streamed data):
class-pure tiles through the unchanged tile kernels in query form, same-label tile pairs masked out of the ranking.

At the full budget (p_work = 1.0) the result must BE the nearest-enemy graph of the float32 rows: enemy_cases.enemy_violations
(every listed row of another label, listed pairs real, no index twice, rows ascending, no closer enemy left out beyond the
rounding of float32 differences) reports nothing, on every data family x label scheme, on every query route of the dispatch
-- and every case asserts which kernel ran.

Query routes (nn entries kept, no self column; launch_by_dim of csrc/streamed.hip):
  split       padded dimension <= 128, nn <= 30     k_st_knnbf (kind 1)
  k-blocked   padded dimension 256 .. 1024, nn <= 62 knnbk.hip (kind 1)
  exact-f32   up to 256 dimensions, nn <= 127       k_st_knn (kind 0) + k_st_guard_expanded + k_st_repair
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))
import enemy_cases as ec   # noqa: E402
import streamed_cases as sc   # noqa: E402

N = 1777
# (d, nn, expected kind)
ROUTES = [(20, 3, 1), (128, 3, 1), (128, 30, 1), (128, 31, 0), (300, 10, 1), (300, 62, 1), (64, 40, 0)]


def _fit(X, **kw):
    from annchor_amd.streamed import StreamedAnnchor

    cfg = dict(n_anchors=8, n_neighbors=6, p_work=1.0)
    cfg.update(kw)
    return StreamedAnnchor(X, **cfg).fit()


def _assert_exact(X, y, idx, dist, nn, what, rows=None, complete=True):
    rows = np.arange(len(X)) if rows is None else rows
    assert idx.shape == (len(X), nn) and dist.shape == (len(X), nn) and idx.dtype == np.int64 and dist.dtype == np.float64
    bad = ec.enemy_violations(X, y, rows, idx[rows], dist[rows], nn, sc.gamma_of(sc.padded_dim(X.shape[1])), complete=complete)
    print("%s: %d of %d rows violate" % (what, len(bad), len(rows)))
    assert bad == [], "%s: %d of %d rows, first %s" % (what, len(bad), len(rows), bad[:4])


@pytest.mark.parametrize("scheme", sorted(ec.SCHEMES))
@pytest.mark.parametrize("name", sorted(sc.FAMILIES))
@pytest.mark.parametrize("d,nn,kind", ROUTES, ids=["d%d-nn%d" % r[:2] for r in ROUTES])
def test_routes_by_families_by_schemes_are_enemy_exact(d, nn, kind, name, scheme):
    X = sc.family(name, N, d)
    y = ec.labels(scheme, X, nn)
    sa = _fit(X)
    idx, dist = sa.nearest_enemies(y, nn, p_work=1.0)
    st = sa.enemy_stats
    k, flagged, two_stage, repaired = st["kernel"], st["guard_rows"], st["two_stage"], st["repaired"]
    print("d=%d nn=%d %s %s: kernel %d, flagged %d, repaired %s, %d tile evaluations on %d tiles"
          % (d, nn, name, scheme, k, flagged, repaired, sa.enemy_tile_evals, sa.enemy_stats["tiles"]))
    assert k == kind and not two_stage, "dispatch moved: %s" % ((k, flagged, two_stage, repaired),)
    if name == "far_clusters":
        # the guard + the repair must really have been the thing tested: the repair scans every tile whose bound lies below the
        # row's nn-th distance, and would readmit same-label columns if the bound were not masked with the key
        assert flagged > 0 and repaired, (flagged, repaired)
    assert sa.enemy_tile_evals <= sa.enemy_stats["tiles"] ** 2
    assert sa.nearest_enemy_graph[0] is idx and sa.nearest_enemy_graph[1] is dist
    _assert_exact(X, y, idx, dist, nn, "d=%d nn=%d %s %s" % (d, nn, name, scheme))


def test_annchor_get_nearest_enemies_on_streamed_data():
    from annchor_amd import Annchor

    X = sc.family("plain", N, 20)
    y = ec.labels("seven_uneven", X, 3)
    ann = Annchor(X, "euclidean", n_anchors=8, n_neighbors=6, p_work=1.0, streamed=True).fit()
    assert ann._streamed is not None
    e0 = ann.evals
    assert ann.get_nearest_enemies(y, nn=3, p_work=1.0) is None
    gi, gd = ann.nearest_enemy_graph
    si, sd = _fit(X).nearest_enemies(y, 3, p_work=1.0)
    assert np.array_equal(gi, si) and np.array_equal(gd, sd)
    assert ann.evals > e0 and ann.enemy_tile_evals > 0
    _assert_exact(X, y, gi, gd, 3, "Annchor euclidean")
    # p_work = None: the fit's budget (1.0 here); loc_min is accepted and means nothing
    ann.get_nearest_enemies(y, nn=3, loc_min=7)
    assert np.array_equal(ann.nearest_enemy_graph[0], si)


def test_cosine_against_a_float64_cosine_brute_force():
    from annchor_amd import Annchor

    X = sc.family("plain", N, 20)
    y = ec.labels("two_random", X, 3)
    ann = Annchor(X, "cosine", n_anchors=8, n_neighbors=6, p_work=1.0, streamed=True).fit()
    assert ann._streamed is not None and ann._cosine_streamed
    ann.get_nearest_enemies(y, nn=3, p_work=1.0)
    gi, gd = ann.nearest_enemy_graph
    bi, bd = ec.brute_cosine_enemies_f64(X, y, np.arange(N), 3)
    assert np.all(y[gi] != y[:, None])
    # the rows are normalised in float32 and d^2 / 2 is formed from float32 distances: a few float32 roundings of O(1) quantities
    assert np.allclose(gd, bd, rtol=1e-4, atol=4e-6)
    agree = np.mean(gi == bi)
    print("cosine: %.4f of the entries name the brute force's row" % agree)   # (printed: near-ties under float32 normalisation may differ)
    U = X.astype(np.float64) / np.linalg.norm(X.astype(np.float64), axis=1)[:, None]
    true = 1.0 - np.einsum("rkd,rd->rk", U[gi], U)
    assert np.allclose(gd, true, rtol=1e-4, atol=4e-6)   # listed pairs are real


def test_fit_graph_and_queries_are_bit_identical_around_an_enemies_call():
    X = sc.family("plain", 3000, 128)
    Q = sc.family("plain", 500, 128, seed=5)
    y = ec.labels("seven_uneven", X, 3)
    sa = _fit(X, n_neighbors=10, p_work=0.3)
    g0 = (sa.neighbor_graph[0].copy(), sa.neighbor_graph[1].copy())
    q0 = sa.query(Q, nn=5, p_work=0.3)
    sa.nearest_enemies(y, 3)
    q1 = sa.query(Q, nn=5, p_work=0.3)
    assert np.array_equal(q0[0], q1[0]) and np.array_equal(q0[1], q1[1])
    assert np.array_equal(sa.neighbor_graph[0], g0[0]) and np.array_equal(sa.neighbor_graph[1], g0[1])
    again = _fit(X, n_neighbors=10, p_work=0.3)
    assert np.array_equal(again.neighbor_graph[0], g0[0]) and np.array_equal(again.neighbor_graph[1], g0[1])
    sa.nearest_enemies(y, 3)   # and a second call on the same object gives the same lines
    e1 = sa.nearest_enemy_graph
    sa.nearest_enemies(y, 3)
    assert np.array_equal(e1[0], sa.nearest_enemy_graph[0]) and np.array_equal(e1[1], sa.nearest_enemy_graph[1])


def test_label_handling():
    from annchor_amd import _native

    X = sc.family("plain", N, 20)
    sa = _fit(X)
    y = ec.labels("seven_uneven", X, 3)
    ref = sa.nearest_enemies(y, 3, p_work=1.0)
    # string labels (np.unique gives them the same codes, so the lines are the same bit for bit)
    names = np.array(["alpha", "beta", "delta", "eta", "gamma", "kappa", "mu"])
    got = sa.nearest_enemies(names[y], 3, p_work=1.0)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    got = sa.nearest_enemies(list(names[y]), 3, p_work=1.0)
    assert np.array_equal(got[0], ref[0])
    # the three assertions of the pair-list form, same texts
    with pytest.raises(AssertionError, match="Label dimension mismatch"):
        sa.nearest_enemies(y[:-1], 3)
    with pytest.raises(AssertionError, match="more than one label"):
        sa.nearest_enemies(np.zeros(N), 3)
    with pytest.raises(AssertionError, match="occurs fewer times than specified nn=4"):
        sa.nearest_enemies(y, 4)   # (one class has exactly 3 rows)
    # the class cap: every class padded to a whole tile may not more than double the rows
    with pytest.raises(ValueError, match=r"%d labels on %d rows.*%d rows" % (N // 2 + 1, N, (N // 2 + 1) * 128)):
        sa.nearest_enemies(np.arange(N) // 2, 1)
    sa.nearest_enemies(np.arange(N) % (N // 128), 3)   # n // 128 classes are always accepted
    # nn beyond the routes' capacities
    with pytest.raises(_native.NativeError, match="nearest enemies support 1 <= nn <= 127"):
        sa.nearest_enemies(np.arange(N) % 2, 128)
    wide = _fit(sc.family("plain", 700, 300))
    with pytest.raises(_native.NativeError, match="beyond 256 dimensions"):
        wide.nearest_enemies(np.arange(700) % 2, 63)
    assert wide.nearest_enemies(np.arange(700) % 2, 62, p_work=1.0)[0].shape == (700, 62)
    # more than one rank: refused (a stand-in communicator of two ranks on the fitted object)
    sa.comm = type("TwoRanks", (), {"world": 2, "rank": 0})()
    with pytest.raises(NotImplementedError, match="2 ranks"):
        sa.nearest_enemies(y, 3)
    # before fit()
    from annchor_amd.streamed import StreamedAnnchor

    with pytest.raises(RuntimeError, match="fit"):
        StreamedAnnchor(X, n_anchors=8, n_neighbors=6).nearest_enemies(y, 3)


def test_pair_list_form_refuses_p_work():
    from annchor_amd import Annchor

    X = sc.family("plain", 400, 20)
    ann = Annchor(X, "euclidean", n_anchors=8, n_neighbors=6, n_samples=500, p_work=0.3, streamed=False).fit()
    with pytest.raises(ValueError, match="streamed form only"):
        ann.get_nearest_enemies(np.arange(400) % 2, nn=3, p_work=0.5)
    ann.get_nearest_enemies(np.arange(400) % 2, nn=3)
    assert ann.nearest_enemy_graph[0].shape == (400, 3)


def _ten_centres(X, seed=3):
    """Ten classes by the nearest of ten fixed random rows."""
    c = X[np.random.default_rng(seed).choice(len(X), 10, replace=False)].astype(np.float64)
    d2 = (X.astype(np.float64) ** 2).sum(1)[:, None] - 2.0 * X.astype(np.float64) @ c.T + (c * c).sum(1)[None, :]
    return np.argmin(d2, axis=1)


def test_budgeted_run_lists_real_enemies_within_the_budget():
    n, d, nn, p = 200_000, 128, 3, 0.1
    X = sc.latent(n, d, seed=11)
    y = _ten_centres(X)
    assert np.unique(y, return_counts=True)[1].min() >= nn
    sa = _fit(X, n_anchors=32, n_neighbors=15, p_work=p)
    idx, dist = sa.nearest_enemies(y, nn)   # p_work = None: the fit's budget
    assert sa.enemy_stats["p_work"] == p
    budget = int(np.ceil(p * sa.enemy_stats["tiles"]))
    print("budgeted: %d tiles (%d unpadded), %d tile evaluations, budget %d per row tile, kernel %s, timings %s"
          % (sa.enemy_stats["tiles"], (n + 127) // 128, sa.enemy_tile_evals, budget, (sa.enemy_stats["kernel"], sa.enemy_stats["guard_rows"]), sa.enemy_stats["timings"]))
    assert 0 < sa.enemy_tile_evals <= budget * sa.enemy_stats["tiles"]
    rows = np.sort(np.random.default_rng(2).choice(n, 1000, replace=False))
    assert np.all(idx >= 0) and np.all(y[idx] != y[:, None])
    _assert_exact(X, y, idx, dist, nn, "budgeted", rows=rows, complete=False)
    bi, _ = ec.brute_enemies_f64(X, y, rows, nn)
    recall = np.mean([len(set(idx[r]) & set(bi[t])) / nn for t, r in enumerate(rows)])
    print("budgeted: recall@%d on %d rows = %.4f" % (nn, len(rows), recall))   # printed, not thresholded


def test_alpha_rss_on_streamed_data():
    from annchor_amd import Annchor

    n = 2000
    X = sc.latent(n, 20, seed=21)
    y = _ten_centres(X)
    for alpha in (0, 0.2):
        ann = Annchor(X, "euclidean", n_anchors=8, n_neighbors=6, p_work=1.0, streamed=True).fit()
        rss = np.asarray(ann.alpha_rss(y, alpha=alpha))
        gi, gd = ann.nearest_enemy_graph
        _assert_exact(X, y, gi, gd, 3, "alpha_rss enemies")
        dne = gd[:, 0]
        adne = dne / (1 + alpha)
        # the defining property, in float64, in the scan order (ascending nearest-enemy distance, stable): a point joins when no
        # earlier member lies within its adne (np.isclose slack as in enemies.alpha_rss), and only then
        Xd = X.astype(np.float64)
        order = np.argsort(dne, kind="stable")
        got_in = np.zeros(n, dtype=bool)
        got_in[rss] = True
        assert len(set(rss.tolist())) == len(rss) and got_in[order[0]]
        members = [int(order[0])]
        for i in order[1:]:
            m = np.sqrt(((Xd[members] - Xd[i][None, :]) ** 2).sum(1)).min()
            edge = np.isclose(m, adne[i])
            if got_in[i]:
                assert m > adne[i] or edge, (int(i), m, adne[i])    # no earlier member within its adne when it was scanned
                members.append(int(i))
            else:
                assert m <= adne[i] or edge, (int(i), m, adne[i])   # an earlier-scanned member lies within its adne
        print("alpha=%g: alpha_rss keeps %d of %d points" % (alpha, len(rss), n))
        assert 1 < len(rss) < n


def test_selective_subset_is_still_refused_on_streamed_data():
    from annchor_amd import Annchor

    X = sc.family("plain", 600, 20)
    ann = Annchor(X, "euclidean", n_anchors=8, n_neighbors=6, p_work=1.0, streamed=True).fit()
    with pytest.raises(NotImplementedError, match="keeps no such.*list.*get_nearest_enemies and alpha_rss are available"):
        ann.annchor_selective_subset(np.arange(600) % 2)
