"""The fixed-radius graph on the GPU (csrc/radius.hip, annchor_amd/radius.py) against tests/radius_cases.py.

1. classification on injected anchor tables with no metric bound: per-row counts and the EVAL / SURE lists, order included,
   equal the NumPy rule bit for bit -- every case of radius_cases.CASES (sizes on the chunk / workgroup / tile edges, ties,
   duplicates, inf, r = 0, all OUT / EVAL / SURE, rtol 0 and > 0, no bounds, forced chunking, empty rows);
2. end to end: Annchor.radius_graph and BruteForce.radius_graph equal the host double-loop graph, indices identical and
   distances bit-equal, at the edge radii, both modes, once with tiny chunks;
3. the accounting; 4. a fitted object is left as it was; 5. the refusals and the host-metric route.
No tolerances anywhere."""
import numpy as np
import pytest

import radius_cases as C

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------- 1. classification
def _collect(eng, nx, row_total, cap):
    """EVAL and SURE lists of all ranges, concatenated in the order the ranges are taken; what happened on the way."""
    from annchor_amd import _native as nat
    from annchor_amd.radius import plan_ranges

    ev, su, info = [], [], dict(calls=0, splits=0, largest=0)

    def take(ne, ns):
        info["calls"] += 1
        info["largest"] = max(info["largest"], ne + ns)
        if ne:
            ev.append(eng.radius_fetch(nat.RADIUS_EVAL, ne))
        if ns:
            su.append(eng.radius_fetch(nat.RADIUS_SURE, ns))

    for rb, re in plan_ranges(row_total, cap):
        ne, ns, nk = eng.radius_rows(rb, re, rb + 1, nx, cap, False)
        if nk >= 0:
            take(ne, ns)
            continue
        assert re - rb == 1
        pieces = [(rb + 1, nx)]
        while pieces:
            cb, ce = pieces.pop()
            ne, ns, nk = eng.radius_rows(rb, re, cb, ce, cap, False)
            if nk < 0:
                info["splits"] += 1
                pieces += [((cb + ce) // 2, ce), (cb, (cb + ce) // 2)]
            else:
                take(ne, ns)
    z = np.zeros((0, 2), dtype=np.int64)
    return (np.concatenate(ev) if ev else z), (np.concatenate(su) if su else z), info


@pytest.mark.parametrize("name", list(C.CASES))
def test_classification_on_injected_tables(name):
    from annchor_amd import _native as nat

    c = C.CASES[name]
    D = C.build(name)
    want = C.case_reference(name)
    eng = nat.Engine()
    try:
        eng.set_opaque(c["nx"])
        eng.set_anchor_distances(D, [0])
        row_eval, row_sure = eng.radius_count(c["r"], c["rtol"], c["conn"], c["use_bounds"])
        assert np.array_equal(row_eval, want["row_eval"]) and np.array_equal(row_sure, want["row_sure"])
        cap = c["cap"] if c["cap"] else 1 << 26
        ev, su, info = _collect(eng, c["nx"], row_eval + row_sure, cap)
        assert ev.dtype == np.int64 and np.array_equal(ev, want["eval"]), "EVAL list (or its order) differs"
        assert np.array_equal(su, want["sure"]), "SURE list (or its order) differs"
        if c["cap"]:
            assert info["largest"] <= cap and info["splits"] > 0 and info["calls"] > 4, info
        # one call over everything gives the same lists (the default chunk never binds at these sizes)
        if c["nx"] > 1:
            ne, ns, nk = eng.radius_rows(0, c["nx"], 0, c["nx"], 0, False)
            assert (ne, ns, nk) == (len(want["eval"]), len(want["sure"]), 0)
            assert np.array_equal(eng.radius_fetch(nat.RADIUS_EVAL, ne), want["eval"])
            assert np.array_equal(eng.radius_fetch(nat.RADIUS_SURE, ns), want["sure"])
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------ 2. end to end
CFG = dict(n_anchors=12, n_neighbors=5, n_samples=200, p_work=0.5, random_seed=7)


def _strings():
    X = C.clustered_strings(C.E2E_STRINGS["n"])
    return X, "levenshtein", C.levenshtein_pairs(X)


def _series():
    from seqdp_cases import clustered_curves, erp_pairs_host

    S = clustered_curves(150, 6, 14, 2, seed=43)
    return S, "erp", (lambda IJ: erp_pairs_host(S, IJ, 0.0))


def _sets():
    import jaccard_cases as jc

    X = jc.fit_sets()
    return X, "jaccard", (lambda IJ: jc.jaccard_pairs_host(X, IJ))


def _points(dtype):
    X = C.lattice_points(260, 5, 5, dtype)
    return X, "euclidean", C.euclidean_pairs(X)


DATA = {"levenshtein": _strings, "erp": _series, "jaccard": _sets, "euclidean_f64": lambda: _points(np.float64),
        "euclidean_f32": lambda: _points(np.float32)}
_CACHE = {}


def data(name):
    """(X, metric, M): the data set and its host distance matrix, computed once per session and never written."""
    if name not in _CACHE:
        X, metric, pairs = DATA[name]()
        M = C.matrix_of(len(X), pairs)
        M.setflags(write=False)
        _CACHE[name] = (X, metric, M)
    return _CACHE[name]


def _triple(g):
    return g.indptr, g.indices, g.distances


@pytest.mark.parametrize("name", list(DATA))
def test_radius_graph_equals_the_double_loop(name):
    from annchor_amd import Annchor, BruteForce

    X, metric, M = data(name)
    nx = len(X)
    na = C.E2E_STRINGS["n_anchors"] if name == "levenshtein" else CFG["n_anchors"]
    ann = Annchor(X, metric, **dict(CFG, n_anchors=na))
    bf = BruteForce(X, metric)
    radii = C.edge_radii(M)
    if name == "levenshtein":
        radii.append(C.E2E_STRINGS["r"])
    for k, r in enumerate(radii):
        want = C.graph_from_matrix(M, r)
        g = ann.radius_graph(r)
        assert g.indptr.dtype == np.int64 and g.indices.dtype == np.int64 and g.distances.dtype == np.float64
        assert C.same_graph(_triple(g), want), (name, r, "distance mode")
        gc = ann.radius_graph(r, mode="connectivity")
        assert gc.distances is None and C.same_graph(_triple(gc), want, distances=False), (name, r, "connectivity mode")
        assert ann.radius_pruned + ann.radius_sure + ann.radius_evals == ann.radius_pairs == nx * (nx - 1) // 2
        if k in (0, 3, len(radii) - 1):
            gb = bf.radius_graph(r)
            assert C.same_graph(_triple(gb), want), (name, r, "brute force")
            assert bf.radius_evals == bf.radius_pairs == nx * (nx - 1) // 2
    # tiny chunks: rows share chunks and single rows are split by column range
    r = radii[4]
    want = C.graph_from_matrix(M, r)
    g = ann.radius_graph(r, max_chunk_pairs=61)
    assert C.same_graph(_triple(g), want) and ann.radius_chunks > 8
    assert C.same_graph(_triple(bf.radius_graph(r, max_chunk_pairs=200)), want) and bf.radius_chunks > 40
    assert C.same_graph(_triple(bf.radius_graph(r, mode="connectivity", max_chunk_pairs=200)), want, distances=False)
    # the sparse form keeps pairs at distance 0
    S = ann.radius_graph(radii[3]).to_sparse_matrix()
    want3 = C.graph_from_matrix(M, radii[3])
    assert S.shape == (nx, nx) and S.nnz == len(want3[1]) and (abs(S - S.T)).nnz == 0


# ------------------------------------------------------------------------------------------------------ 3. accounting
def test_accounting_on_the_clustered_strings():
    from annchor_amd import Annchor

    X, metric, M = data("levenshtein")
    nx, r = len(X), C.E2E_STRINGS["r"]
    ann = Annchor(X, metric, **dict(CFG, n_anchors=C.E2E_STRINGS["n_anchors"]))
    for mode in ("distance", "connectivity"):
        before = ann.evals
        ann.radius_graph(r, mode=mode)
        L = C.lists(C.classify(ann.D, r, 0.0, mode == "connectivity"))
        print("%s: pairs %d, pruned %d, sure %d, evaluated %d, anchor evaluations %d"
              % (mode, ann.radius_pairs, ann.radius_pruned, ann.radius_sure, ann.radius_evals, before))
        assert ann.radius_pairs == nx * (nx - 1) // 2
        assert ann.radius_pruned + ann.radius_sure + ann.radius_evals == ann.radius_pairs
        assert ann.radius_pruned == L["pruned"] and ann.radius_sure == len(L["sure"]) and ann.radius_evals == len(L["eval"])
        assert ann.radius_evals < ann.radius_pairs
        assert 2 * ann.radius_pruned >= ann.radius_pairs
        anchor_evals = ann.evals - ann.radius_evals - before
        # the anchor round runs once, inside the first call; anchors included the route spends fewer evaluations than brute force
        if mode == "distance":
            assert before == 0 and anchor_evals > 0 and ann.evals < ann.radius_pairs
        else:
            assert anchor_evals == 0


# ------------------------------------------------------------------------------------------------- 4. non-interference
def test_a_fitted_object_is_left_as_it_was():
    from annchor_amd import Annchor, _native
    from annchor_amd.datasets import load_strings

    X = load_strings()["X"][::5]
    cfg = dict(n_anchors=8, n_neighbors=10, n_samples=700, p_work=0.3, random_seed=42, niters=2)
    ann = Annchor(X, "levenshtein", **cfg).fit()
    k = cfg["n_neighbors"]
    graph0 = ann._engine.neighbor_graph(k)
    ra0, ijs0, ncm0 = (ann._engine.download(f) for f in (_native.F_RA, _native.F_IJS, _native.F_NCM))
    Q = list(X[3:40:4])
    q0 = ann.query(Q, nn=5)
    evals0 = ann.evals
    r = float(np.percentile(ann.neighbor_graph[1][:, 1:], 60))
    g1 = ann.radius_graph(r)
    assert ann.evals == evals0 + ann.radius_evals and g1.nnz > 0      # (no second anchor round)
    graph1 = ann._engine.neighbor_graph(k)
    assert np.array_equal(graph0[0], graph1[0]) and np.array_equal(graph0[1], graph1[1])
    for f, before in ((_native.F_RA, ra0), (_native.F_IJS, ijs0), (_native.F_NCM, ncm0)):
        assert np.array_equal(ann._engine.download(f), before)
    q1 = ann.query(Q, nn=5)
    assert np.array_equal(q0[0], q1[0]) and np.array_equal(q0[1], q1[1])
    g2 = ann.radius_graph(r)
    assert all(np.array_equal(a, b) for a, b in zip(_triple(g1), _triple(g2)))
    # every listed neighbour of the k-NN graph within r is in the radius graph, at the same distance
    idx, dist = ann.neighbor_graph
    for i in range(0, len(X), 17):
        ni, nd = g1.neighbors(i)
        for j, d in zip(idx[i, 1:], dist[i, 1:]):
            if d <= r:
                assert j in ni and nd[list(ni).index(j)] == d


# ---------------------------------------------------------------------------------- 5. refusals, the host-metric route
def test_refusals():
    from annchor_amd import Annchor

    X, metric, M = data("euclidean_f32")
    ann = Annchor(X, metric, **CFG)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="r must be a number >= 0"):
            ann.radius_graph(bad)
    with pytest.raises(ValueError, match="mode must be"):
        ann.radius_graph(1.0, mode="both")
    with pytest.raises(ValueError, match=r"BruteForce\(X, func\)\.radius_graph"):
        Annchor(X, metric, is_metric=False, **CFG).radius_graph(1.0)
    with pytest.raises(ValueError, match=r"r_euc = sqrt\(2 \* r\)"):
        Annchor(X.astype(np.float64) + 1.0, "cosine", **CFG).radius_graph(0.1)
    big = np.random.default_rng(0).standard_normal((2048, 16)).astype(np.float32)
    with pytest.raises(NotImplementedError, match="streamed=False"):
        Annchor(big, "euclidean", streamed=True, n_anchors=8, n_neighbors=5).radius_graph(1.0)


def test_python_callable_metric_takes_the_download_route():
    from annchor_amd import Annchor, BruteForce

    X, _, M = data("levenshtein")
    nx = len(X)
    calls = {"pairs": 0}

    def lookup(f, Xs, IJ):   # the object's evaluator: answers from the host table and counts what it is asked
        IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
        calls["pairs"] += len(IJ)
        return M[IJ[:, 0], IJ[:, 1]]

    def host_metric(a, b):   # (a Python callable, so no device metric is bound; the pairs go through get_exact_ijs)
        raise AssertionError("not called one by one")

    ann = Annchor(list(X), host_metric, get_exact_ijs=lookup, **dict(CFG, n_anchors=C.E2E_STRINGS["n_anchors"]))
    r = C.E2E_STRINGS["r"]
    want = C.graph_from_matrix(M, r)
    g = ann.radius_graph(r)
    assert C.same_graph(_triple(g), want)
    assert ann.radius_evals < ann.radius_pairs and ann.radius_pruned + ann.radius_evals == ann.radius_pairs
    before = calls["pairs"]
    gc = ann.radius_graph(r, mode="connectivity")
    assert calls["pairs"] - before == ann.radius_evals          # only the candidates were asked for
    assert C.same_graph(_triple(gc), want, distances=False)
    assert ann.radius_pruned + ann.radius_sure + ann.radius_evals == ann.radius_pairs
    bf = BruteForce(list(X), host_metric, get_exact_ijs=lookup)
    assert C.same_graph(_triple(bf.radius_graph(r, max_chunk_pairs=5000)), want) and bf.radius_evals == bf.radius_pairs
