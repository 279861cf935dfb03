"""The exact k-NN graph from the anchor bounds on the GPU (csrc/knnexact.hip, annchor_amd/radius.py: exact_knn,
Annchor.exact_neighbor_graph) against tests/exact_knn_cases.py.

1. the per-row-radius classifier alone on injected anchor tables and radii: per-row totals (count form) and the emitted list
   (table form) equal the reference, in identical order, also through ranges that split rows and bisect a single row;
2. absorb and finish on injected candidate lists under a line metric, through the host route (edges) and the device route (1-D
   float64 points): per-row entry counts and the graph equal the reference, with rows in LDS and rows read from memory;
3. end to end against BruteForce(X, f).fit(k).neighbor_graph: identical indices, bit-equal distances, under a true, a spoiled, a
   random and an invalid seed, with tiny chunks, k = 1 and k = nx;
4. the default seed on the bundled strings; 5. a Python-callable metric; 6. refusals and call order; 7. non-interference.
No tolerances anywhere."""
import numpy as np
import pytest

import exact_knn_cases as K
import radius_cases as RC

pytestmark = pytest.mark.gpu


def _engine(name, points=False):
    """An engine holding the case's anchor table and, with `points`, its positions as 1-D float64 points under 'euclidean'."""
    from annchor_amd import _native as nat

    c = K.CASES[name]
    D, u, _ = K.build(name)
    eng = nat.Engine()
    if points:
        eng.set_points(K.positions(c["kind"], c["nx"], c["na"], c["seed"])[:, None].astype(np.float64))
    else:
        eng.set_opaque(c["nx"])
    if c["use_bounds"]:
        eng.set_anchor_distances(D, [0])
    return eng, u


# ----------------------------------------------------------------------------------------------- 1. the classifier alone
@pytest.mark.parametrize("name", list(K.CASES))
def test_classifier_totals_and_lists(name):
    from annchor_amd.radius import walk_rows

    c, ref = K.CASES[name], K.case_reference(name)
    nx = c["nx"]
    eng, u = _engine(name)
    try:
        row_eval = eng.knn_exact_begin(c["k"], u, c["rtol"], c["use_bounds"])
        assert row_eval.dtype == np.int64 and np.array_equal(row_eval, ref["row_eval"])
        if c["cap"] is None:
            ne, nn = eng.knn_exact_rows(0, nx, 0, nx, 0, False)
            assert (ne, nn) == (len(ref["eval"]), 0)
            assert np.array_equal(eng.knn_exact_fetch(ne), ref["eval"])
            # a range in the middle, off the chunk edges: its rows and columns only
            if nx >= 65:
                rb, re, cb, ce = nx // 3, nx // 3 + 40, nx // 2 - 3, nx - 2
                E = ref["eval"]
                want = E[(E[:, 0] >= rb) & (E[:, 0] < re) & (E[:, 1] >= cb) & (E[:, 1] < ce)]
                ne, _ = eng.knn_exact_rows(rb, re, cb, ce, 0, False)
                assert ne == len(want) and np.array_equal(eng.knn_exact_fetch(ne), want)
        else:
            got, sizes = [], []

            def consume(ne, nn):
                assert nn == 0 and ne <= c["cap"]
                got.append(eng.knn_exact_fetch(ne))
                sizes.append(ne)

            walk_rows(row_eval, nx, c["cap"], lambda rb, re, cb, ce: eng.knn_exact_rows(rb, re, cb, ce, c["cap"], False), consume, "test")
            assert np.array_equal(np.concatenate(got), ref["eval"]) and len(sizes) > 4
            ne, nn = eng.knn_exact_rows(0, nx, 0, nx, c["cap"], False)
            assert ne == len(ref["eval"]) and nn == -1      # over the cap: counted, nothing emitted
    finally:
        eng.close()


# ------------------------------------------------------------------------------ 2. absorb and finish on injected lists
def _check_graph(got, ref):
    idx, dist, rows = got
    assert idx.dtype == np.int64 and dist.dtype == np.float64 and rows.dtype == np.int64
    assert np.array_equal(rows, ref["row_entries"])
    assert np.array_equal(idx, ref["idx"]) and dist.tobytes() == ref["dist"].tobytes()


@pytest.mark.parametrize("name", list(K.CASES))
def test_absorb_and_finish_through_the_host_route(name):
    """The reference's candidates with the line metric's distances, in three batches, the middle one with its pairs turned round:
    entry counts and graph are the reference's whatever the LDS cap (0: every row in LDS; 3 and 40: longer rows from memory)."""
    c, ref = K.CASES[name], K.case_reference(name)
    eng, u = _engine(name)
    try:
        eng.knn_exact_begin(c["k"], u, c["rtol"], c["use_bounds"])
        E = ref["eval"]
        d = K.metric(name)(E) if len(E) else np.zeros(0)
        cut = [0, len(E) // 3, 2 * len(E) // 3, len(E)]
        for b in range(3):
            part = E[cut[b]:cut[b + 1]]
            eng.knn_exact_edges(part[:, ::-1] if b == 1 else part, d[cut[b]:cut[b + 1]])
        first = eng.knn_exact_finish()
        _check_graph(first, ref)
        for row_cap in (3, 40):
            _check_graph(eng.knn_exact_finish(row_cap), ref)
    finally:
        eng.close()


# integer positions: sqrt((x - y)^2) is |x - y| exactly; a point set has at least two members (the one-point cases ran above)
DEVICE_CASES = [n for n, c in K.CASES.items() if c["kind"] != "line" and c["nx"] >= 2]


@pytest.mark.parametrize("name", DEVICE_CASES)
def test_walk_absorb_and_finish_on_the_device(name):
    from annchor_amd.radius import exact_knn

    c, ref = K.CASES[name], K.case_reference(name)
    eng, u = _engine(name, points=True)
    try:
        (idx, dist), st = exact_knn(eng, c["nx"], c["k"], u, c["rtol"], c["use_bounds"], c["cap"])
        assert np.array_equal(idx, ref["idx"]) and dist.tobytes() == ref["dist"].tobytes()
        assert st["evals"] == ref["evals"] and st["pairs"] == st["pruned"] + st["evals"] == c["nx"] * (c["nx"] - 1) // 2
        assert st["entries"] == int(ref["row_entries"].sum())
        _check_graph(eng.knn_exact_finish(5), ref)
        if c["cap"] is not None:
            assert st["chunks"] > 4
    finally:
        eng.close()


def test_entry_list_keeps_its_content_across_growth():
    """All 7 140 pairs of 120 points with u = +inf (every directed entry passes) through four knn_exact_edges calls: the first
    reserves 4096 entries, the second needs more while 2 x 1785 are held, so the list grows with its content kept.  The distances
    are small integers, so the rows are full of ties: the graph is the rows sorted by (distance, index)."""
    from annchor_amd import _native as nat

    nx, k = 120, 7
    T = np.random.default_rng(11).integers(0, 4, (nx, nx))
    D = np.triu(T, 1)
    D = (D + D.T).astype(np.float64)
    i, j = np.triu_indices(nx, 1)
    E = np.stack([i, j], axis=1).astype(np.int64)
    assert len(E) == 7140
    want_idx = np.stack([np.lexsort((np.arange(nx), D[r]))[:k] for r in range(nx)])   # (the diagonal is (0.0, r))
    want_dist = np.take_along_axis(D, want_idx, axis=1)
    eng = nat.Engine()
    try:
        eng.set_opaque(nx)
        eng.knn_exact_begin(k, np.full(nx, np.inf), 0.0, False)
        for part in np.array_split(E, 4):
            assert len(part) == 1785
            eng.knn_exact_edges(part, D[part[:, 0], part[:, 1]])
        idx, dist, row_entries = eng.knn_exact_finish()
    finally:
        eng.close()
    assert np.array_equal(row_entries, np.full(nx, nx - 1))
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(dist.view(np.int64), want_dist.view(np.int64))


def test_nan_distances_are_not_kept_and_short_rows_are_refused():
    from annchor_amd import _native as nat

    name = "line_k5"
    c, ref = K.CASES[name], K.case_reference(name)
    eng, u = _engine(name)
    try:
        eng.knn_exact_begin(c["k"], u, c["rtol"], True)
        E = ref["eval"]
        d = K.metric(name)(E)
        extra = np.array([[0, c["nx"] - 1], [3, 1]], dtype=np.int64)         # pruned pairs handed in with a NaN distance: dropped
        eng.knn_exact_edges(np.concatenate([E, extra]), np.concatenate([d, [np.nan, np.nan]]))
        _check_graph(eng.knn_exact_finish(), ref)
        # radii that are no upper bounds: rows end short of k - 1 entries and the finish says so
        eng.knn_exact_begin(c["k"], np.zeros(c["nx"]), c["rtol"], True)
        ne, nn = eng.knn_exact_rows(0, c["nx"], 0, c["nx"], 0, False)
        eng.knn_exact_edges(eng.knn_exact_fetch(ne), K.metric(name)(eng.knn_exact_fetch(ne)))
        with pytest.raises(nat.NativeError, match="rows hold fewer than k - 1 = 4 entries"):
            eng.knn_exact_finish()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------ 3. end to end
_BF = {}


def brute(name, k=None, n=None):
    """BruteForce(X, f).fit(k).neighbor_graph of an end-to-end data set (or of its first n members), once per session."""
    from annchor_amd import BruteForce

    key = (name, k, n)
    if key not in _BF:
        X, metric, _ = K.e2e_data(name)
        X = X if n is None else X[:n]
        g = BruteForce(X, metric).fit(K.E2E[name]["k"] if k is None else k).neighbor_graph
        for a in g:
            a.setflags(write=False)
        _BF[key] = (X, metric, g)
    return _BF[key]


def _ann(name, X, metric, k):
    from annchor_amd import Annchor

    return Annchor(X, metric, n_anchors=K.E2E[name]["n_anchors"], n_neighbors=k, n_samples=200, p_work=0.5, random_seed=7)


@pytest.mark.parametrize("name", list(K.E2E))
def test_exact_graph_equals_brute_force_under_every_seed(name):
    X, metric, want = brute(name)
    nx, k = len(X), K.E2E[name]["k"]
    ann = _ann(name, X, metric, k)
    ann.get_anchors()       # (their evaluations are not this feature's: the accounting below starts behind them)
    evals = {}
    for kind in K.SEEDS:
        G = K.seed_graph(kind, want[0], k)
        before = ann.evals
        got = ann.exact_neighbor_graph(seed_graph=G if kind != "spoiled" else (G, np.zeros(G.shape)))
        assert K.same_graph(got, want), kind
        assert ann.exact_pairs == nx * (nx - 1) // 2 == ann.exact_pruned + ann.exact_evals
        assert ann.evals - before == ann.exact_evals + ann.exact_seed_evals and 0 < ann.exact_seed_evals <= nx * k
        assert ann.exact_entries >= nx * (k - 1) and ann.exact_chunks >= 1
        short = sum(len(set(G[i].tolist()) - {i}) < k - 1 for i in range(nx))     # (random entries may repeat or name the row itself)
        assert ann.exact_inf_rows == short and (short >= len(range(0, nx, 3)) if kind == "invalid" else short < nx // 10)
        evals[kind] = ann.exact_evals
        print("%s, %s seed: %d of %d pairs evaluated, %d entries" % (name, kind, ann.exact_evals, ann.exact_pairs, ann.exact_entries))
    assert 0 < evals["true"] < ann.exact_pairs // 4 and evals["true"] < evals["spoiled"] < evals["random"]
    assert ann.__dict__.get("neighbor_graph") is None       # (an explicit seed: no fit ran, and nothing was stored)
    # tiny chunks: many ranges, rows above the cap bisected by column range
    got = ann.exact_neighbor_graph(seed_graph=K.seed_graph("spoiled", want[0], k), max_chunk_pairs=61)
    assert K.same_graph(got, want) and ann.exact_evals == evals["spoiled"] and ann.exact_chunks >= evals["spoiled"] // 61 > 8
    # a wider margin than the default evaluates more and answers the same
    wide = ann.exact_neighbor_graph(seed_graph=want[0], bound_rtol=0.3)
    assert K.same_graph(wide, want) and ann.exact_evals > evals["true"]


@pytest.mark.parametrize("k", [1, 2, 65])
def test_exact_graph_at_k_1_and_k_nx(k):
    for name in ("levenshtein", "euclidean_f32"):
        X, metric, want = brute(name, k, 65)
        ann = _ann(name, X, metric, k)
        for kind in ("true", "random"):
            got = ann.exact_neighbor_graph(seed_graph=K.seed_graph(kind, want[0], k), max_chunk_pairs=None if kind == "true" else 50)
            assert K.same_graph(got, want), (name, kind)
        if k == 65:
            assert ann.exact_evals == 65 * 64 // 2 and ann.exact_entries == 65 * 64


# ------------------------------------------------------------------------------------------------- 4. the default seed
def test_default_seed_certifies_the_fit_on_the_bundled_strings():
    from annchor_amd import Annchor, BruteForce, compare_neighbor_graphs
    from annchor_amd.datasets import load_strings

    X = load_strings()["X"]
    ann = Annchor(X, "levenshtein", n_anchors=15, n_neighbors=25, p_work=0.12, random_seed=42).fit()
    ng = ann.neighbor_graph
    ng0 = tuple(a.copy() for a in ng)
    evals0 = ann.evals
    exact = ann.exact_neighbor_graph()
    want = BruteForce(X, "levenshtein").fit(25).neighbor_graph
    assert K.same_graph(exact, want)
    assert compare_neighbor_graphs(exact, want, 25) == 0
    assert ann.exact_pruned > 0 and ann.exact_pairs == ann.exact_pruned + ann.exact_evals == 1600 * 1599 // 2
    assert ann.evals == evals0 + ann.exact_evals + ann.exact_seed_evals and ann.exact_inf_rows == 0
    assert ann.neighbor_graph is ng and all(np.array_equal(a, b) for a, b in zip(ng, ng0))
    errors = compare_neighbor_graphs(exact, ng, 25)
    print("fit errors %d of %d; exact: %d of %d pairs evaluated (%.1f %%), %d seed evaluations, %d entries"
          % (errors, 1600 * 25, ann.exact_evals, ann.exact_pairs, 100.0 * ann.exact_evals / ann.exact_pairs, ann.exact_seed_evals,
             ann.exact_entries))
    assert errors == compare_neighbor_graphs(want, ng, 25)
    # an unfitted object fits first, and then answers the same
    other = Annchor(X[::5], "levenshtein", n_anchors=8, n_neighbors=10, n_samples=700, p_work=0.3, random_seed=42, niters=2)
    got = other.exact_neighbor_graph()
    assert other.__dict__.get("neighbor_graph") is not None and other.exact_pruned > 0
    assert K.same_graph(got, BruteForce(X[::5], "levenshtein").fit(10).neighbor_graph)


# -------------------------------------------------------------------------------------------- 5. a Python-callable metric
def test_python_callable_metric_goes_through_fetch_and_edges():
    from annchor_amd import Annchor

    X, _, pairs = K.e2e_data("euclidean_f64")
    n, k = 150, 6
    Xs = X[:n]
    M = RC.matrix_of(n, RC.euclidean_pairs(Xs))
    want = K.truth(M, k)
    calls = {"pairs": 0}

    def lookup(f, Xq, IJ):   # the object's evaluator: answers from the host table and counts what it is asked
        IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
        calls["pairs"] += len(IJ)
        return M[IJ[:, 0], IJ[:, 1]]

    def host_metric(a, b):   # (a Python callable, so no device metric is bound; the pairs go through get_exact_ijs)
        raise AssertionError("not called one by one")

    ann = Annchor(list(Xs), host_metric, get_exact_ijs=lookup, n_anchors=8, n_neighbors=k, n_samples=200, p_work=0.5, random_seed=7)
    ann.get_anchors()
    chunks = {}
    for kind, cap in (("true", None), ("spoiled", 97), ("invalid", None)):
        before = calls["pairs"]
        got = ann.exact_neighbor_graph(seed_graph=K.seed_graph(kind, want[0], k), max_chunk_pairs=cap)
        assert K.same_graph(got, want), kind
        assert calls["pairs"] - before == ann.exact_evals + ann.exact_seed_evals      # only the seed entries and the candidates were asked for
        assert 0 < ann.exact_evals < ann.exact_pairs
        chunks[kind] = ann.exact_chunks
    assert chunks["true"] == 1 and chunks["spoiled"] > 8


# ------------------------------------------------------------------------------------------ 6. refusals and call order
def test_refusals():
    from annchor_amd import Annchor

    X = RC.lattice_points(260, 5, 5, np.float32)
    cfg = dict(n_anchors=8, n_neighbors=5, n_samples=200, p_work=0.5, random_seed=7)
    ann = Annchor(X, "euclidean", **cfg)
    G = np.tile(np.arange(5, dtype=np.int64), (260, 1))
    for bad in (0, 261, 2.5, True):
        with pytest.raises(ValueError, match="n_neighbors must be an integer in 1..260"):
            ann.exact_neighbor_graph(bad, seed_graph=G)
    with pytest.raises(ValueError, match="bound_rtol must be in"):
        ann.exact_neighbor_graph(seed_graph=G, bound_rtol=1.0)
    with pytest.raises(ValueError, match="max_chunk_pairs must be >= 1"):
        ann.exact_neighbor_graph(seed_graph=G, max_chunk_pairs=0)
    for bad in (G[:, :4], G[:100], G.astype(np.float64)):
        with pytest.raises(ValueError, match="seed_graph must hold integer indices"):
            ann.exact_neighbor_graph(seed_graph=bad)
    with pytest.raises(ValueError, match=r"is_metric=False.*BruteForce\(X, func\)\.fit\(n_neighbors\)"):
        Annchor(X, "euclidean", is_metric=False, **cfg).exact_neighbor_graph(seed_graph=G)
    with pytest.raises(ValueError, match="cosine.*not a metric"):
        Annchor(X.astype(np.float64) + 1.0, "cosine", **cfg).exact_neighbor_graph(seed_graph=G)
    big = np.random.default_rng(0).standard_normal((2048, 16)).astype(np.float32)
    with pytest.raises(NotImplementedError, match="streamed=False.*p_work=1.0"):
        Annchor(big, "euclidean", streamed=True, n_anchors=8, n_neighbors=5).exact_neighbor_graph()
    # nothing above left a half-made state behind: the object still answers (a seed of arbitrary valid rows)
    from annchor_amd import BruteForce

    assert K.same_graph(ann.exact_neighbor_graph(seed_graph=G), BruteForce(X, "euclidean").fit(5).neighbor_graph)


def test_argument_checks_and_call_order():
    from annchor_amd import _native as nat

    name = "nx129_k5"
    c, ref = K.CASES[name], K.case_reference(name)
    eng, u = _engine(name)
    nx = c["nx"]
    try:
        for call in (lambda: eng.knn_exact_rows(0, nx, 0, nx), lambda: eng.knn_exact_fetch(1), lambda: eng.knn_exact_finish(),
                     lambda: eng.knn_exact_edges(np.array([[0, 1]]), np.array([1.0]))):
            with pytest.raises(nat.NativeError, match="annchor_knn_exact_begin has not run"):
                call()
        for k in (0, nx + 1):
            with pytest.raises(nat.NativeError, match="out of range 1..%d" % nx):
                eng.knn_exact_begin(k, u, 0.0, True)
        for bad in (-1.0, np.nan):
            v = u.copy()
            v[7] = bad
            with pytest.raises(nat.NativeError, match=r"u\[7\] must be a number >= 0: pass \+inf"):
                eng.knn_exact_begin(5, v, 0.0, True)
        with pytest.raises(nat.NativeError, match="rtol must be in"):
            eng.knn_exact_begin(5, u, 1.0, True)
        # a begin takes the radius stages' buffers: a stale radius_rows is refused, not wrong
        eng.radius_count(3.0, 0.0, False, True)
        eng.knn_exact_begin(5, u, 0.0, True)
        with pytest.raises(nat.NativeError, match="annchor_radius_count has not run"):
            eng.radius_rows(0, nx, 0, nx, 0, False)
        with pytest.raises(nat.NativeError, match="no radius range has been processed"):
            eng.radius_fetch(nat.RADIUS_EVAL, 1)
        with pytest.raises(nat.NativeError, match="row range"):
            eng.knn_exact_rows(5, 5, 0, nx)
        with pytest.raises(nat.NativeError, match="column range"):
            eng.knn_exact_rows(0, 5, 0, nx + 1)
        with pytest.raises(nat.NativeError, match="no device metric bound"):
            eng.knn_exact_rows(0, nx, 0, nx, 0, True)
        # an emitted range that nobody absorbed: the finish refuses to answer from an incomplete list
        ne, nn = eng.knn_exact_rows(0, nx, 0, nx, 0, False)
        with pytest.raises(nat.NativeError, match="%d candidates were emitted and never absorbed" % ne):
            eng.knn_exact_finish()
        E = eng.knn_exact_fetch(ne)
        for bad in ([[0, nx]], [[-1, 3]], [[4, 4]]):
            with pytest.raises(nat.NativeError, match="end points must be two different points"):
                eng.knn_exact_edges(np.array(bad, dtype=np.int64), np.array([1.0]))
        eng.knn_exact_edges(E, K.metric(name)(E))
        with pytest.raises(nat.NativeError, match="row_cap must be >= 0"):
            eng.knn_exact_finish(-1)
        _check_graph(eng.knn_exact_finish(), ref)
        # a second begin forgets the first run's entries; the radius stages work again after their own count
        eng.knn_exact_begin(1, np.zeros(nx), 0.0, True)
        idx, dist, rows = eng.knn_exact_finish()
        assert np.array_equal(idx[:, 0], np.arange(nx)) and not dist.any() and not rows.any()
        eng.radius_count(3.0, 0.0, False, True)
        assert eng.radius_rows(0, nx, 0, nx, 0, False)[0] > 0
    finally:
        eng.close()


# --------------------------------------------------------------------------------------------------- 7. non-interference
def test_a_fitted_object_and_the_radius_routes_are_left_as_they_were():
    from annchor_amd import Annchor, _native
    from annchor_amd.datasets import load_strings

    X = load_strings()["X"][::5]
    cfg = dict(n_anchors=8, n_neighbors=10, n_samples=700, p_work=0.3, random_seed=42, niters=2)
    ann = Annchor(X, "levenshtein", **cfg).fit()
    k = cfg["n_neighbors"]
    graph0 = ann._engine.neighbor_graph(k)
    ng0 = tuple(a.copy() for a in ann.neighbor_graph)
    ra0, ijs0, ncm0 = (ann._engine.download(f) for f in (_native.F_RA, _native.F_IJS, _native.F_NCM))
    Q = list(X[3:40:4])
    q0 = ann.query(Q, nn=5)
    eps = float(np.percentile(ann.neighbor_graph[1][:, 1:], 60))
    g0, db0 = ann.radius_graph(eps), ann.dbscan(eps, 4)
    evals0 = ann.evals
    exact = ann.exact_neighbor_graph()
    assert ann.evals == evals0 + ann.exact_evals + ann.exact_seed_evals and ann.exact_pruned > 0    # (no second anchor round)
    graph1 = ann._engine.neighbor_graph(k)
    assert np.array_equal(graph0[0], graph1[0]) and np.array_equal(graph0[1], graph1[1])
    assert np.array_equal(ng0[0], ann.neighbor_graph[0]) and np.array_equal(ng0[1], ann.neighbor_graph[1])
    for f, before in ((_native.F_RA, ra0), (_native.F_IJS, ijs0), (_native.F_NCM, ncm0)):
        assert np.array_equal(ann._engine.download(f), before)
    q1 = ann.query(Q, nn=5)
    assert np.array_equal(q0[0], q1[0]) and np.array_equal(q0[1], q1[1])
    g1, db1 = ann.radius_graph(eps), ann.dbscan(eps, 4)
    assert RC.same_graph((g0.indptr, g0.indices, g0.distances), (g1.indptr, g1.indices, g1.distances))
    assert np.array_equal(db0.labels, db1.labels) and np.array_equal(db0.core_sample_mask, db1.core_sample_mask)
    again = ann.exact_neighbor_graph()
    assert K.same_graph(exact, again)
    # the exact rows are consistent with the fit's: never a larger distance in any column
    assert np.all(exact[1] <= ann.neighbor_graph[1])
