"""Fixed-radius queries for new points on the GPU (csrc/radius.hip: k_rad_classify_q; annchor_amd/radius.py) against
tests/radius_query_cases.py.

1. classification on injected anchor tables with no metric bound: per-query counts and the EVAL / SURE lists, order included,
   equal the NumPy rule bit for bit -- every case of radius_query_cases.CASES -- over planned ranges, in one call over the whole
   rectangle, on sub-ranges, under a forced cap, and against radius_rows where the queries are copies of data rows;
2. end to end: Annchor.radius_query and BruteForce.radius_query equal the host double loop over the rectangle, indices identical
   and distances bit-equal, at the edge radii, both modes, tiny chunks, one query, before and after fit();
3. consistency with radius_graph; 4. the accounting, and a fitted object is left as it was; 5. the refusals and routes.
No tolerances anywhere."""
import numpy as np
import pytest

import radius_cases as C
import radius_query_cases as QC
import test_radius_gpu as G   # its data sets (generators, host matrices cached per session) and object settings

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------- 1. classification
def _collect(eng, nx, row_total, cap):
    """EVAL and SURE lists of all ranges, concatenated in the order the ranges are taken; what happened on the way."""
    from annchor_amd import _native as nat
    from annchor_amd.radius import plan_query_ranges

    ev, su, info = [], [], dict(calls=0, splits=0, largest=0)

    def take(ne, ns):
        info["calls"] += 1
        info["largest"] = max(info["largest"], ne + ns)
        if ne:
            ev.append(eng.radius_fetch(nat.RADIUS_EVAL, ne))
        if ns:
            su.append(eng.radius_fetch(nat.RADIUS_SURE, ns))

    for qb, qe in plan_query_ranges(row_total, nx, cap):
        ne, ns, nk = eng.radius_query_rows(nx, qb, qe, 0, nx, cap, False)
        if nk >= 0:
            take(ne, ns)
            continue
        assert qe - qb == 1
        pieces = [(0, nx)]
        while pieces:
            cb, ce = pieces.pop()
            ne, ns, nk = eng.radius_query_rows(nx, qb, qe, cb, ce, cap, False)
            if nk < 0:
                info["splits"] += 1
                pieces += [((cb + ce) // 2, ce), (cb, (cb + ce) // 2)]
            else:
                take(ne, ns)
    z = np.zeros((0, 2), dtype=np.int64)
    return (np.concatenate(ev) if ev else z), (np.concatenate(su) if su else z), info


@pytest.mark.parametrize("name", list(QC.CASES))
def test_classification_on_injected_tables(name):
    from annchor_amd import _native as nat

    c = QC.CASES[name]
    nx, nq = c["nx"], c["nq"]
    D, QD = QC.build(name)
    cls = QC.case_classes(name)
    want = QC.lists_q(cls)
    eng = nat.Engine()
    try:
        eng.set_opaque(nx + nq)
        eng.set_anchor_distances(np.vstack([D, QD]), [0])
        row_eval, row_sure = eng.radius_query_count(nx, c["r"], c["rtol"], c["conn"], c["use_bounds"])
        assert row_eval.shape == (nq,) and row_eval.dtype == np.int64
        assert np.array_equal(row_eval, want["row_eval"]) and np.array_equal(row_sure, want["row_sure"])
        cap = c["cap"] if c["cap"] else 1 << 26
        ev, su, info = _collect(eng, nx, row_eval + row_sure, cap)
        # (a query split by column range arrives left to right: the concatenation is query-major and ascending as it stands)
        assert ev.dtype == np.int64 and np.array_equal(ev, want["eval"]), "EVAL list (or its order) differs"
        assert np.array_equal(su, want["sure"]), "SURE list (or its order) differs"
        if c["cap"]:
            assert info["largest"] <= cap and info["splits"] > 0 and info["calls"] > 4, info
        # one call over the whole rectangle gives the same lists
        ne, ns, nk = eng.radius_query_rows(nx, 0, nq, 0, nx, 0, False)
        assert (ne, ns, nk) == (len(want["eval"]), len(want["sure"]), 0)
        assert np.array_equal(eng.radius_fetch(nat.RADIUS_EVAL, ne), want["eval"])
        assert np.array_equal(eng.radius_fetch(nat.RADIUS_SURE, ns), want["sure"])
        if c["sub"]:
            sub = QC.restrict(cls, c["sub"])
            ne, ns, nk = eng.radius_query_rows(nx, *c["sub"], 0, False)
            assert (ne, ns) == (len(sub["eval"]), len(sub["sure"]))
            assert np.array_equal(eng.radius_fetch(nat.RADIUS_EVAL, ne), sub["eval"])
            assert np.array_equal(eng.radius_fetch(nat.RADIUS_SURE, ns), sub["sure"])
        if c["kind"] == "copy" and nq <= nx:
            # the queries are the first nq data points: restricted to j > q the lists are the graph form's rows 0 .. nq - 1
            # (columns below nx) on the same engine state
            eng.radius_count(c["r"], c["rtol"], c["conn"], c["use_bounds"])
            ne, ns, nk = eng.radius_rows(0, nq, 0, nx, 0, False)
            for which, n, mine in ((nat.RADIUS_EVAL, ne, want["eval"]), (nat.RADIUS_SURE, ns, want["sure"])):
                above = mine[mine[:, 0] > mine[:, 1] - nx]
                assert np.array_equal(eng.radius_fetch(which, n), np.stack([above[:, 1] - nx, above[:, 0]], axis=1))
    finally:
        eng.close()


def test_a_count_of_one_form_does_not_serve_the_other():
    from annchor_amd import _native as nat

    D, QD = QC.build("copy")
    eng = nat.Engine()
    try:
        eng.set_opaque(len(D) + len(QD))
        eng.set_anchor_distances(np.vstack([D, QD]), [0])
        with pytest.raises(Exception, match="annchor_radius_query_count has not run"):
            eng.radius_query_rows(len(D), 0, 1, 0, len(D))
        eng.radius_query_count(len(D), 3.0, 0.0, False, True)
        with pytest.raises(Exception, match="annchor_radius_count has not run"):
            eng.radius_rows(0, 1, 1, len(D))
        with pytest.raises(Exception, match="column range"):
            eng.radius_query_rows(len(D), 0, 1, 0, len(D) + 1)        # the columns are data points only
        with pytest.raises(Exception, match="row range"):
            eng.radius_query_rows(len(D), 0, len(QD) + 1, 0, len(D))
        for bad in (0, len(D) + len(QD)):
            with pytest.raises(Exception, match="nx_data"):
                eng.radius_query_count(bad, 3.0, 0.0, False, True)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------ 2. end to end
def _queries(name, X):
    """~40 fresh members of X's generator, two verbatim copies of members among them, and the host pairs function over X
    followed by Q."""
    if name == "levenshtein":
        Q = np.array(QC.fresh_strings(X, 36, seed=9))
        assert max(map(len, Q)) > max(map(len, X)) and min(map(len, Q)) < min(map(len, X))
        return Q, C.levenshtein_pairs(list(X) + list(Q))
    if name == "erp":
        from seqdp_cases import clustered_curves, erp_pairs_host

        Q = clustered_curves(38, 6, 14, 2, seed=44) + [X[17], X[len(X) - 1]]
        both = list(X) + list(Q)
        return Q, (lambda IJ: erp_pairs_host(both, IJ, 0.0))
    if name == "jaccard":
        import jaccard_cases as jc

        Q = list(jc.window_sets(38, 600, seed=2)) + [X[17], X[len(X) - 1]]
        both = list(X) + list(Q)
        return Q, (lambda IJ: jc.jaccard_pairs_host(both, IJ))
    Q = QC.fresh_points(X, 38, seed=9)
    return Q, C.euclidean_pairs(np.concatenate([X, Q]))


_CACHE = {}


def qdata(name):
    """(X, metric, M, Q, R): test_radius_gpu's data set and matrix, the queries and the host rectangle [nq, nx] -- computed once
    per session and never written."""
    if name not in _CACHE:
        X, metric, M = G.data(name)
        Q, pairs = _queries(name, X)
        R = QC.rectangle_of(len(X), len(Q), pairs)
        R.setflags(write=False)
        _CACHE[name] = (X, metric, M, Q, R)
    return _CACHE[name]


def _triple(g):
    return g.indptr, g.indices, g.distances


def _anchors(name):
    return C.E2E_STRINGS["n_anchors"] if name == "levenshtein" else G.CFG["n_anchors"]


@pytest.mark.parametrize("name", list(G.DATA))
def test_radius_query_equals_the_double_loop(name):
    from annchor_amd import Annchor, BruteForce

    X, metric, M, Q, R = qdata(name)
    nx, nq = len(X), len(Q)
    assert nq == 40 and np.count_nonzero(R == 0.0) >= 2           # the verbatim copies are at distance 0
    ann = Annchor(X, metric, **dict(G.CFG, n_anchors=_anchors(name)))    # (never fitted: the first call picks the anchors)
    bf = BruteForce(X, metric)
    radii = C.edge_radii(M)
    if name == "levenshtein":
        radii.append(C.E2E_STRINGS["r"])
    for k, r in enumerate(radii):
        want = QC.neighbors_from_matrix(R, r)
        g = ann.radius_query(Q, r)
        assert g.indptr.dtype == np.int64 and g.indices.dtype == np.int64 and g.distances.dtype == np.float64
        assert (g.nq, g.nx) == (nq, nx) and C.same_graph(_triple(g), want), (name, r, "distance mode")
        assert ann.radius_query_pruned + ann.radius_query_sure + ann.radius_query_evals - ann.n_anchors * nq == ann.radius_query_pairs == nq * nx
        gc = ann.radius_query(Q, r, mode="connectivity")
        assert gc.distances is None and C.same_graph(_triple(gc), want, distances=False), (name, r, "connectivity mode")
        assert ann.radius_query_pruned + ann.radius_query_sure + ann.radius_query_evals - ann.n_anchors * nq == nq * nx
        if k in (0, 3, len(radii) - 1):
            gb = bf.radius_query(Q, r)
            assert C.same_graph(_triple(gb), want), (name, r, "brute force")
            assert bf.radius_query_evals == bf.radius_query_pairs == nq * nx
    # tiny chunks: queries share chunks and single queries are split by column range
    r = radii[4]
    want = QC.neighbors_from_matrix(R, r)
    g = ann.radius_query(Q, r, max_chunk_pairs=61)
    assert C.same_graph(_triple(g), want) and ann.radius_query_chunks > 8
    assert C.same_graph(_triple(ann.radius_query(Q, r, mode="connectivity", max_chunk_pairs=61)), want, distances=False)
    assert C.same_graph(_triple(bf.radius_query(Q, r, max_chunk_pairs=100)), want) and bf.radius_query_chunks >= 2 * nq   # (nx > 100: every query is split)
    assert C.same_graph(_triple(bf.radius_query(Q, r, mode="connectivity", max_chunk_pairs=100)), want, distances=False)
    # one query (a verbatim copy of a data member: itself at distance 0)
    one = ann.radius_query(Q[nq - 1:], r)
    lo, hi = want[0][nq - 1], want[0][nq]
    assert C.same_graph(_triple(one), (np.array([0, hi - lo]), want[1][lo:hi], want[2][lo:hi]))
    assert (nx - 1) in one.indices and one.distances[list(one.indices).index(nx - 1)] == 0.0
    assert C.same_graph(_triple(bf.radius_query(Q[nq - 1:], r)), _triple(one))
    # the sparse form keeps the pairs at distance 0
    S = ann.radius_query(Q, radii[3]).to_sparse_matrix()
    want3 = QC.neighbors_from_matrix(R, radii[3])
    assert S.shape == (nq, nx) and S.nnz == len(want3[1]) and S[nq - 1, nx - 1] == np.nextafter(0, 1)
    Sc = ann.radius_query(Q, radii[3], mode="connectivity").to_sparse_matrix()
    assert Sc.shape == (nq, nx) and Sc.nnz == len(want3[1]) and set(Sc.values()) == {1.0}


# --------------------------------------------------------------------------------------- 3. consistency with radius_graph
@pytest.mark.parametrize("name", ["levenshtein", "euclidean_f64"])
def test_rows_of_radius_graph(name):
    """Q = X[:70]: row i of radius_query without i itself is row i of radius_graph, distances bit-equal."""
    from annchor_amd import Annchor

    X, metric, M = G.data(name)
    ann = Annchor(X, metric, **dict(G.CFG, n_anchors=_anchors(name)))
    radii = C.edge_radii(M)
    for r in (radii[0], radii[3], radii[4]):
        g = ann.radius_graph(r)
        q = ann.radius_query(X[:70], r)
        for i in range(70):
            qi, qd = q.neighbors(i)
            gi, gd = g.neighbors(i)
            assert i in qi and qd[list(qi).index(i)] == 0.0
            keep = qi != i
            assert np.array_equal(qi[keep], gi) and qd[keep].tobytes() == gd.tobytes(), (name, r, i)


# ------------------------------------------------------------------------------------- 4. accounting, non-interference
def test_accounting_on_the_clustered_strings():
    from annchor_amd import Annchor, BruteForce

    X, metric, M, Q, R = qdata("levenshtein")
    nx, nq, r = len(X), len(Q), C.E2E_STRINGS["r"]
    ann = Annchor(X, metric, **dict(G.CFG, n_anchors=C.E2E_STRINGS["n_anchors"]))
    for mode in ("distance", "connectivity"):
        evals_before = ann.evals
        ann.radius_query(Q, r, mode=mode)
        na = ann.n_anchors
        A = np.asarray(ann.A, dtype=np.int64)
        assert np.array_equal(ann.D, M[:, A])                         # (integer distances: the anchor table is the host's)
        L = QC.lists_q(QC.classify_q(ann.D, R[:, A], r, 0.0, mode == "connectivity"))
        print("%s: pairs %d, pruned %d (%.1f %%), sure %d, evaluated %d of which %d anchor pairs"
              % (mode, ann.radius_query_pairs, ann.radius_query_pruned, 100.0 * ann.radius_query_pruned / (nq * nx),
                 ann.radius_query_sure, ann.radius_query_evals, na * nq))
        assert ann.radius_query_pairs == nq * nx
        assert ann.radius_query_pairs == ann.radius_query_pruned + ann.radius_query_sure + (ann.radius_query_evals - na * nq)
        assert ann.radius_query_pruned == L["pruned"] and ann.radius_query_sure == len(L["sure"])
        assert ann.radius_query_evals - na * nq == len(L["eval"])
        assert ann.radius_query_evals < nq * nx and 2 * ann.radius_query_pruned >= nq * nx
        if mode == "connectivity":
            assert ann.evals == evals_before                          # (the object's own count moves with its anchor round only)
    bf = BruteForce(X, metric)
    bf.radius_query(Q, r)
    assert bf.radius_query_evals == bf.radius_query_pairs == nq * nx


def test_a_fitted_object_is_left_as_it_was():
    """Before and after fit(); and what a fitted object answers afterwards is what a twin that never called radius_query
    answers, bit for bit."""
    from annchor_amd import Annchor
    from annchor_amd.datasets import load_strings

    X = load_strings()["X"][::5]
    both = list(X)
    Qr = np.array(QC.fresh_strings(X, 20, seed=4))
    R = QC.rectangle_of(len(X), len(Qr), C.levenshtein_pairs(both + list(Qr)))
    cfg = dict(n_anchors=8, n_neighbors=10, n_samples=700, p_work=0.3, random_seed=42, niters=2)
    r = float(np.percentile(R, 2))
    want = QC.neighbors_from_matrix(R, r)
    assert len(want[1]) > len(Qr)
    ann, twin = Annchor(X, "levenshtein", **cfg), Annchor(X, "levenshtein", **cfg)
    assert C.same_graph(_triple(ann.radius_query(Qr, r)), want)       # before any fit()
    ann.fit()
    twin.fit()
    evals = ann.evals
    assert C.same_graph(_triple(ann.radius_query(Qr, r)), want)       # after
    assert C.same_graph(_triple(ann.radius_query(Qr, r, mode="connectivity", max_chunk_pairs=100)), want, distances=False)
    assert ann.evals == evals                                         # (radius_query counts in radius_query_evals only)
    assert ann.evals - twin.evals == cfg["n_anchors"] * len(X)        # the anchor round of the call before fit(), nothing else
    for a, b in zip(ann.neighbor_graph, twin.neighbor_graph):
        assert a.tobytes() == b.tobytes()
    Qk = list(X[3:40:4])
    for a, b in zip(ann.query(Qk, nn=5), twin.query(Qk, nn=5)):
        assert a.tobytes() == b.tobytes()
    ga, gb = ann.radius_graph(r), twin.radius_graph(r)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(_triple(ga), _triple(gb))) and ga.nnz > 0
    assert C.same_graph(_triple(ann.radius_query(Qr, r)), want)       # and after query() and radius_graph()


# ---------------------------------------------------------------------------------- 5. refusals, the host-metric route
def test_refusals():
    from annchor_amd import Annchor, BruteForce

    X, metric, M = G.data("euclidean_f32")
    Q = X[:5]
    ann = Annchor(X, metric, **G.CFG)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="r must be a number >= 0"):
            ann.radius_query(Q, bad)
        with pytest.raises(ValueError, match="r must be a number >= 0"):
            BruteForce(X, metric).radius_query(Q, bad)
    with pytest.raises(ValueError, match="mode must be"):
        ann.radius_query(Q, 1.0, mode="both")
    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError, match=r"bound_rtol must be in \[0, 1\)"):
            ann.radius_query(Q, 1.0, bound_rtol=bad)
    with pytest.raises(ValueError, match="Q is empty"):
        ann.radius_query(X[:0], 1.0)
    with pytest.raises(ValueError, match="Q is empty"):
        BruteForce(X, metric).radius_query(X[:0], 1.0)
    with pytest.raises(ValueError, match=r"BruteForce\(X, func\)\.radius_query"):
        Annchor(X, metric, is_metric=False, **G.CFG).radius_query(Q, 1.0)
    with pytest.raises(ValueError, match=r"r_euc = sqrt\(2 \* r\)"):
        Annchor(X.astype(np.float64) + 1.0, "cosine", **G.CFG).radius_query(Q, 0.1)
    big = np.random.default_rng(0).standard_normal((2048, 16)).astype(np.float32)
    with pytest.raises(NotImplementedError, match=r"streamed=False.*BruteForce\(X, func\)\.radius_query"):
        Annchor(big, "euclidean", streamed=True, n_anchors=8, n_neighbors=5).radius_query(big[:3], 1.0)


def test_python_callable_metric_takes_the_download_route():
    from annchor_amd import Annchor, BruteForce

    X, _, M, Q, R = qdata("levenshtein")
    nx, nq = len(X), len(Q)
    pos = {str(x): i for i, x in enumerate(X)}
    calls = {"pairs": 0}

    def lookup(f, Xs, IJ):   # the object's evaluator for pairs of X: answers from the host table
        IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
        return M[IJ[:, 0], IJ[:, 1]]

    def qlookup(f, Xs, Zs, IJ):   # pairs (Xs[i], Zs[j]); Xs is X or the anchors' members, Zs is Q
        IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
        assert len(Zs) == nq
        calls["pairs"] += len(IJ)
        rows = np.array([pos[str(x)] for x in Xs], dtype=np.int64)
        return R[IJ[:, 1], rows[IJ[:, 0]]]

    def host_metric(a, b):   # (a Python callable, so no device metric is bound)
        raise AssertionError("not called one by one")

    na = C.E2E_STRINGS["n_anchors"]
    ann = Annchor(list(X), host_metric, get_exact_ijs=lookup, **dict(G.CFG, n_anchors=na))
    ann.get_exact_query_ijs = qlookup
    dev = Annchor(X, "levenshtein", **dict(G.CFG, n_anchors=na))
    r = C.E2E_STRINGS["r"]
    want = QC.neighbors_from_matrix(R, r)
    g = ann.radius_query(list(Q), r)
    assert C.same_graph(_triple(g), want) and C.same_graph(_triple(g), _triple(dev.radius_query(Q, r)))
    assert calls["pairs"] == ann.radius_query_evals and na * nq < ann.radius_query_evals < nq * nx
    assert (ann.radius_query_pruned, ann.radius_query_evals) == (dev.radius_query_pruned, dev.radius_query_evals)
    before = calls["pairs"]
    gc = ann.radius_query(list(Q), r, mode="connectivity", max_chunk_pairs=500)
    assert calls["pairs"] - before == ann.radius_query_evals          # the anchor pairs and the candidates, nothing else
    assert C.same_graph(_triple(gc), want, distances=False)
    assert ann.radius_query_pruned + ann.radius_query_sure + ann.radius_query_evals - na * nq == nq * nx
    bf = BruteForce(list(X), host_metric, get_exact_ijs=lookup)
    bf.get_exact_query_ijs = qlookup
    assert C.same_graph(_triple(bf.radius_query(list(Q), r, max_chunk_pairs=5000)), want) and bf.radius_query_evals == nq * nx


def test_sorted_by_distance_orders_ties_by_index():
    from annchor_amd import Annchor

    X, metric, M, Q, R = qdata("levenshtein")
    ann = Annchor(X, metric, **dict(G.CFG, n_anchors=C.E2E_STRINGS["n_anchors"]))
    r = C.edge_radii(M)[4]
    g = ann.radius_query(Q, r)
    s = g.sorted_by_distance()
    assert np.array_equal(s.indptr, g.indptr) and s.nx == g.nx
    ties = 0
    for q in range(len(Q)):
        idx, d = g.neighbors(q)
        order = sorted(range(len(idx)), key=lambda t: (d[t], idx[t]))
        si, sd = s.neighbors(q)
        assert np.array_equal(si, idx[order]) and np.array_equal(sd, d[order])
        ties += len(d) - len(set(d))
    assert ties > 0                                                   # (integer distances tie in every row)
    with pytest.raises(ValueError, match="mode='distance'"):
        ann.radius_query(Q, r, mode="connectivity").sorted_by_distance()
