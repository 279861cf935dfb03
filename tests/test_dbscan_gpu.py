"""DBSCAN on the GPU (csrc/dbscan.hip, annchor_amd/radius.py: cluster) against tests/dbscan_cases.py.

1. the clustering kernels on injected edge lists: labels, core mask and n_clusters equal the host reference exactly for every
   case of dbscan_cases.CASES, a second finish returns the same arrays, and the edge orders of one graph give identical arrays;
2. absorb from the radius buffers on injected anchor tables: refused while a range holds unevaluated candidates, and equal to
   the reference on a table that leaves every pair SURE or OUT;
3. end to end: Annchor.dbscan and BruteForce.dbscan equal the reference run on the host double-loop distance matrix, also with
   tiny chunks, consistent with radius_graph(eps) of the same object and with no more evaluations than it;
4. the host-metric route; 5. the refusals; 6. a fitted object is left as it was.
No tolerances anywhere."""
import numpy as np
import pytest

import dbscan_cases as DC
import radius_cases as C

pytestmark = pytest.mark.gpu


def _same(got, want):
    labels, core, ncl = got
    return np.array_equal(labels, want[0]) and np.array_equal(core.astype(bool), want[1]) and ncl == want[2]


# ------------------------------------------------------------------------------------- 1. kernels on injected edge lists
def _run_case(eng, name):
    c = DC.CASES[name]
    eng.set_opaque(c["nx"])
    eng.dbscan_begin(c["min_samples"])
    for part in DC.batches(name):
        eng.dbscan_edges(part)
    return eng.dbscan_finish()


@pytest.mark.parametrize("name", list(DC.CASES))
def test_clustering_kernels_on_injected_edges(name):
    from annchor_amd import _native as nat

    c = DC.CASES[name]
    want = DC.REFERENCE[name]
    eng = nat.Engine()
    try:
        got = _run_case(eng, name)
        assert got[0].dtype == np.int32 and got[1].dtype == np.uint8
        assert _same(got, want), name
        again = eng.dbscan_finish()
        assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1]) and got[2] == again[2]
        # a second begin forgets the first run's edges and degrees
        eng.dbscan_begin(c["min_samples"])
        assert _same(eng.dbscan_finish(), DC.reference(c["nx"], [], c["min_samples"]))
    finally:
        eng.close()


GROUPS = sorted({c["group"] for c in DC.CASES.values() if c["group"]})


@pytest.mark.parametrize("group", GROUPS)
def test_edge_orders_of_one_graph_give_identical_arrays(group):
    """The members of a group are one edge set in different orders, orientations or batches: the device arrays are the same."""
    from annchor_amd import _native as nat

    members = [n for n, c in DC.CASES.items() if c["group"] == group]
    assert len(members) >= 2
    eng = nat.Engine()
    try:
        first = _run_case(eng, members[0])
        for name in members[1:]:
            got = _run_case(eng, name)
            assert np.array_equal(first[0], got[0]) and np.array_equal(first[1], got[1]) and first[2] == got[2], (name, "differs from " + members[0])
    finally:
        eng.close()


def test_finish_after_more_edges_recomputes():
    """Edges added after a finish count: the second finish is the reference of the whole list, the first of its first half."""
    from annchor_amd import _native as nat

    c = DC.CASES["random_ms10"]
    half = len(c["edges"]) // 2
    eng = nat.Engine()
    try:
        eng.set_opaque(c["nx"])
        eng.dbscan_begin(c["min_samples"])
        eng.dbscan_edges(c["edges"][:half])
        assert _same(eng.dbscan_finish(), DC.reference(c["nx"], c["edges"][:half], c["min_samples"]))
        eng.dbscan_edges(c["edges"][half:])
        assert _same(eng.dbscan_finish(), DC.REFERENCE["random_ms10"])
    finally:
        eng.close()


def test_edge_validation_and_call_order():
    from annchor_amd import _native as nat

    eng = nat.Engine()
    try:
        eng.set_opaque(10)
        with pytest.raises(nat.NativeError, match="annchor_dbscan_begin has not run"):
            eng.dbscan_edges(np.array([[0, 1]]))
        with pytest.raises(nat.NativeError, match="annchor_dbscan_begin has not run"):
            eng.dbscan_finish()
        with pytest.raises(nat.NativeError, match="min_samples must be >= 1"):
            eng.dbscan_begin(0)
        eng.dbscan_begin(2)
        for bad in ([[0, 10]], [[-1, 3]], [[4, 4]], [[0, 1], [2, 1 << 40]]):
            with pytest.raises(nat.NativeError, match="end points must be two different points"):
                eng.dbscan_edges(np.array(bad, dtype=np.int64))
        # a refused list left nothing behind (the valid first edge of the last one included)
        assert _same(eng.dbscan_finish(), DC.reference(10, [], 2))
        with pytest.raises(nat.NativeError, match="no radius range has been processed"):
            eng.dbscan_absorb()
    finally:
        eng.close()


@pytest.mark.parametrize("min_samples", [200, 201])
def test_edge_list_keeps_its_content_across_growth(min_samples):
    """The complete graph on 200 points, 19 900 edges in a shuffled order through five dbscan_edges calls: the list grows
    4096 -> 8192 -> 16384 -> 32768 entries with what it holds kept each time.  Every degree is 199: at min_samples = 200 every
    point is core (one lost or repeated edge would change that), at 201 none is and everything is noise."""
    from annchor_amd import _native as nat

    nx = 200
    i, j = np.triu_indices(nx, 1)
    E = np.stack([i, j], axis=1).astype(np.int64)[np.random.default_rng(5).permutation(len(i))]
    assert len(E) == 19900
    want = DC.reference(nx, E, min_samples)
    assert want[2] == (1 if min_samples == 200 else 0) and want[1].all() == (min_samples == 200)
    eng = nat.Engine()
    try:
        eng.set_opaque(nx)
        eng.dbscan_begin(min_samples)
        for part in np.array_split(E, 5):
            eng.dbscan_edges(part)
        grown = eng.dbscan_finish()
        eng.dbscan_begin(min_samples)
        eng.dbscan_edges(E)
        once = eng.dbscan_finish()
    finally:
        eng.close()
    assert _same(grown, want) and _same(once, want)
    assert np.array_equal(grown[0], once[0]) and np.array_equal(grown[1], once[1]) and grown[2] == once[2]


# ------------------------------------------------------------------------------------ 2. absorb from the radius buffers
def test_absorb_refuses_unevaluated_candidates():
    from annchor_amd import _native as nat

    name = "nx129"
    c, D = C.CASES[name], C.build(name)
    want = C.case_reference(name)
    assert len(want["eval"]) > 0
    eng = nat.Engine()
    try:
        eng.set_opaque(c["nx"])
        eng.set_anchor_distances(D, [0])
        eng.radius_count(c["r"], c["rtol"], True, True)
        eng.dbscan_begin(3)
        ne, ns, nk = eng.radius_rows(0, c["nx"], 0, c["nx"], 0, False)
        assert ne == len(want["eval"]) and ns == len(want["sure"]) and nk == 0
        with pytest.raises(nat.NativeError, match="not evaluated and holds %d candidates" % ne):
            eng.dbscan_absorb()
        assert _same(eng.dbscan_finish(), DC.reference(c["nx"], [], 3))     # (nothing was taken)
    finally:
        eng.close()


@pytest.mark.parametrize("cap", [0, 150])
def test_absorb_reproduces_the_reference(cap):
    """Every pair SURE or OUT: the sure lists of all ranges, absorbed on the device, are the graph.  cap 150: many ranges, so
    the edge list grows across absorbs; a range is absorbed once."""
    from annchor_amd import _native as nat
    from annchor_amd.radius import plan_ranges

    D, r = DC.sure_or_out_table()
    nx = len(D)
    L = C.lists(C.classify(D, r, 0.0, True))
    assert len(L["eval"]) == 0
    eng = nat.Engine()
    try:
        eng.set_opaque(nx)
        eng.set_anchor_distances(D, [0])
        row_eval, row_sure = eng.radius_count(r, 0.0, True, True)
        assert row_eval.sum() == 0 and row_sure.sum() == len(L["sure"])
        for ms in (6, 1, 65):
            eng.dbscan_begin(ms)
            taken = calls = 0
            ranges = plan_ranges(row_eval + row_sure, cap) if cap else [(0, nx)]
            for rb, re in ranges:
                ne, ns, nk = eng.radius_rows(rb, re, rb + 1, nx, cap, False)
                assert ne == 0 and nk == 0 and ns > 0
                assert eng.dbscan_absorb() == ns
                taken, calls = taken + ns, calls + 1
            with pytest.raises(nat.NativeError, match="absorbed already"):
                eng.dbscan_absorb()
            assert taken == len(L["sure"]) and (cap == 0 or calls > 10)
            assert _same(eng.dbscan_finish(), DC.reference(nx, L["sure"], ms)), ms
        # the query form's lists are not edges of one data set
        eng.radius_query_count(nx - 3, r, 0.0, True, True)
        eng.radius_query_rows(nx - 3, 0, 3, 0, nx - 3, 0, False)
        with pytest.raises(nat.NativeError, match="query form"):
            eng.dbscan_absorb()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------ 3. end to end
CFG = dict(n_anchors=12, n_neighbors=5, n_samples=200, p_work=0.5, random_seed=7)


def _strings():
    X = C.clustered_strings(C.E2E_STRINGS["n"])
    return X, "levenshtein", C.levenshtein_pairs(X)


def _points():
    X = C.lattice_points(260, 5, 5, np.float64)
    return X, "euclidean", C.euclidean_pairs(X)


DATA = {"levenshtein": _strings, "euclidean_f64": _points}
_CACHE = {}


def data(name):
    """(X, metric, M, edges): the data set, its host distance matrix and the edges {d <= eps} of dbscan_cases.E2E, computed
    once per session and never written."""
    if name not in _CACHE:
        X, metric, pairs = DATA[name]()
        M = C.matrix_of(len(X), pairs)
        M.setflags(write=False)
        g = C.graph_from_matrix(M, DC.E2E[name]["eps"])
        edges = DC.edges_of_csr(g[0], g[1])
        edges.setflags(write=False)
        _CACHE[name] = (X, metric, M, edges)
    return _CACHE[name]


# What the host reference shows at dbscan_cases.E2E (DC.census on the double-loop matrix):
#   levenshtein    300 strings, eps 8, min_samples 10: 1195 edges, 13 clusters, 23 noise points, 154 border points (4 of them
#                  with core neighbours in two clusters)
#   euclidean_f64  260 points, eps 4 (an attained distance), min_samples 10: 688 edges, 8 clusters, 89 noise points, 129 border
#                  points (5 of them with core neighbours in two clusters)
E2E_CENSUS = {"levenshtein": (1195, 13, 23, 154), "euclidean_f64": (688, 8, 89, 129)}


def _check(res, want, eps, ms):
    assert res.labels.dtype == np.int64 and res.core_sample_mask.dtype == bool
    assert np.array_equal(res.labels, want[0]) and np.array_equal(res.core_sample_mask, want[1]) and res.n_clusters == want[2]
    assert np.array_equal(res.core_sample_indices, np.flatnonzero(want[1])) and res.n_noise == int((want[0] < 0).sum())
    assert (res.eps, res.min_samples) == (eps, ms)


@pytest.mark.parametrize("name", list(DATA))
def test_dbscan_equals_the_reference_on_the_double_loop(name):
    from annchor_amd import Annchor, BruteForce

    X, metric, M, edges = data(name)
    nx, eps, ms = len(X), DC.E2E[name]["eps"], DC.E2E[name]["min_samples"]
    s = DC.census(nx, edges, ms)
    assert (len(edges), s["clusters"], s["noise"], s["border"]) == E2E_CENSUS[name]
    assert s["clusters"] >= 2 and s["noise"] >= 1 and s["border"] >= 1
    want = DC.reference(nx, edges, ms)
    ann = Annchor(X, metric, **CFG)
    bf = BruteForce(X, metric)
    res = ann.dbscan(eps, ms)
    _check(res, want, eps, ms)
    assert ann.dbscan_pairs == nx * (nx - 1) // 2 == ann.dbscan_pruned + ann.dbscan_sure + ann.dbscan_evals
    assert ann.dbscan_edges == len(edges) and ann.dbscan_evals < ann.dbscan_pairs
    evals = ann.dbscan_evals
    _check(bf.dbscan(eps, ms), want, eps, ms)
    assert bf.dbscan_evals == bf.dbscan_pairs == nx * (nx - 1) // 2 and bf.dbscan_edges == len(edges)
    # tiny chunks: many ranges, rows above the cap bisected by column range
    _check(ann.dbscan(eps, ms, max_chunk_pairs=61), want, eps, ms)
    assert ann.dbscan_chunks > 8 and ann.dbscan_edges == len(edges)
    _check(bf.dbscan(eps, ms, max_chunk_pairs=200), want, eps, ms)
    assert bf.dbscan_chunks >= -(-(nx * (nx - 1) // 2) // 200)     # (every pair is a candidate and a chunk holds at most 200)
    # other parameters on the same objects: the default min_samples, min_samples 1 (no noise), one above every degree
    for ms2 in (5, 1, nx + 1):
        w2 = DC.reference(nx, edges, ms2)
        _check(ann.dbscan(eps, ms2) if ms2 != 5 else ann.dbscan(eps), w2, eps, ms2)
    # consistent with the radius graph of the same object, and no more evaluations than it
    before = ann.evals
    g = ann.radius_graph(eps, mode="connectivity")
    assert ann.evals - before == ann.radius_evals and evals <= ann.radius_evals
    ge = DC.edges_of_csr(g.indptr, g.indices)
    assert _same((res.labels, res.core_sample_mask, res.n_clusters), DC.reference(nx, ge, ms))
    g2 = ann.radius_graph(eps)
    assert _same((res.labels, res.core_sample_mask, res.n_clusters), DC.reference(nx, DC.edges_of_csr(g2.indptr, g2.indices), ms))


# ------------------------------------------------------------------------------------------------ 4. host-metric route
def test_python_callable_metric_gives_the_same_labels():
    from annchor_amd import Annchor, BruteForce

    X, metric, M, _ = data("levenshtein")
    n = 120
    Xs, Ms = X[:n], M[:n, :n]
    eps, ms = DC.E2E["levenshtein"]["eps"], 6
    calls = {"pairs": 0}

    def lookup(f, Xq, IJ):   # the object's evaluator: answers from the host table and counts what it is asked
        IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
        calls["pairs"] += len(IJ)
        return Ms[IJ[:, 0], IJ[:, 1]]

    def host_metric(a, b):   # (a Python callable, so no device metric is bound; the pairs go through get_exact_ijs)
        raise AssertionError("not called one by one")

    dev = Annchor(Xs, metric, **CFG).dbscan(eps, ms)
    g = C.graph_from_matrix(Ms, eps)
    want = DC.reference(n, DC.edges_of_csr(g[0], g[1]), ms)
    _check(dev, want, eps, ms)
    assert dev.n_clusters >= 2
    ann = Annchor(list(Xs), host_metric, get_exact_ijs=lookup, **CFG)
    host = ann.dbscan(eps, ms)
    assert ann.dbscan_evals < ann.dbscan_pairs
    assert np.array_equal(host.labels, dev.labels) and np.array_equal(host.core_sample_mask, dev.core_sample_mask)
    before = calls["pairs"]
    _check(ann.dbscan(eps, ms, max_chunk_pairs=97), want, eps, ms)
    assert calls["pairs"] - before == ann.dbscan_evals             # only the candidates were asked for
    bf = BruteForce(list(Xs), host_metric, get_exact_ijs=lookup)
    _check(bf.dbscan(eps, ms, max_chunk_pairs=1000), want, eps, ms)
    assert bf.dbscan_evals == n * (n - 1) // 2


# ---------------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals():
    from annchor_amd import Annchor, BruteForce

    X = C.lattice_points(260, 5, 5, np.float32)
    ann = Annchor(X, "euclidean", **CFG)
    bf = BruteForce(X, "euclidean")
    for obj in (ann, bf):
        for bad in (-1.0, float("nan")):
            with pytest.raises(ValueError, match="eps must be a number >= 0"):
                obj.dbscan(bad)
        for bad in (0, 2.5):
            with pytest.raises(ValueError, match="min_samples must be an integer >= 1"):
                obj.dbscan(1.0, bad)
    with pytest.raises(ValueError, match="bound_rtol must be in"):
        ann.dbscan(1.0, bound_rtol=1.0)
    way_out = r"BruteForce\(X, .*\)\.dbscan\(eps, min_samples\)"
    with pytest.raises(ValueError, match="is_metric=False.*" + way_out):
        Annchor(X, "euclidean", is_metric=False, **CFG).dbscan(1.0)
    with pytest.raises(ValueError, match="cosine.*" + way_out):
        Annchor(X.astype(np.float64) + 1.0, "cosine", **CFG).dbscan(0.1)
    big = np.random.default_rng(0).standard_normal((2048, 16)).astype(np.float32)
    with pytest.raises(NotImplementedError, match="streamed=False.*" + way_out):
        Annchor(big, "euclidean", streamed=True, n_anchors=8, n_neighbors=5).dbscan(1.0)
    # nothing above left a half-made state behind: the objects still cluster, and BruteForce takes what Annchor refuses
    M = C.matrix_of(len(X), C.euclidean_pairs(X))
    g = C.graph_from_matrix(M, 4.0)
    want = DC.reference(len(X), DC.edges_of_csr(g[0], g[1]), 10)
    _check(ann.dbscan(4.0, 10), want, 4.0, 10)
    _check(bf.dbscan(4.0, 10), want, 4.0, 10)


# --------------------------------------------------------------------------------------------------- 6. non-interference
def test_a_fitted_object_is_left_as_it_was():
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
    evals0 = ann.evals
    eps = float(np.percentile(ann.neighbor_graph[1][:, 1:], 60))
    res = ann.dbscan(eps, 4)
    assert ann.evals == evals0 + ann.dbscan_evals and ann.dbscan_edges > 0      # (no second anchor round)
    graph1 = ann._engine.neighbor_graph(k)
    assert np.array_equal(graph0[0], graph1[0]) and np.array_equal(graph0[1], graph1[1])
    assert np.array_equal(ng0[0], ann.neighbor_graph[0]) and np.array_equal(ng0[1], ann.neighbor_graph[1])
    for f, before in ((_native.F_RA, ra0), (_native.F_IJS, ijs0), (_native.F_NCM, ncm0)):
        assert np.array_equal(ann._engine.download(f), before)
    q1 = ann.query(Q, nn=5)
    assert np.array_equal(q0[0], q1[0]) and np.array_equal(q0[1], q1[1])
    again = ann.dbscan(eps, 4)
    assert np.array_equal(res.labels, again.labels) and np.array_equal(res.core_sample_mask, again.core_sample_mask)
    g = ann.radius_graph(eps, mode="connectivity")
    assert _same((res.labels, res.core_sample_mask, res.n_clusters), DC.reference(len(X), DC.edges_of_csr(g.indptr, g.indices), 4))
