"""Optimal string alignment on the device (csrc/wed.hip, k_osa) against the host recurrence of osa_cases.py, through every layer:
the three pair-source forms, the scratch engine rebound between the three string metrics, BruteForce, Annchor.fit and .query,
loose objects, refusals.

Tolerance: none.  Every cell is a min of sums of fixed operands, min is exact and the additions are commutative, so every
evaluation order gives the same bits; each comparison of distances below is np.array_equal or ==."""
import numpy as np
import pytest

import affine_cases as ac
import osa_cases as oc
import pool_cases as pc
import wed_cases as wc
from oracle import annchor_oracle as O

pytestmark = pytest.mark.gpu

ref = pc.ref_cache()
NAME = oc.NAME
FIT_CFG = pc.FIT_CFG
FIT_KW = oc.kwargs_of(oc.fit_costs())


def bound(X, costs):
    return pc.bound(NAME, X, **oc.kwargs_of(costs))


def host_matrix(key, X, costs):
    """osa on every pair, [nx, nx], computed once for i <= j and mirrored (test_osa_host.py checks both orders against the loop)."""
    return ref(key, lambda: pc.sym_matrix(lambda X_, IJ: oc.osa_pairs_host(X_, IJ, costs), X))


def three_forms(X, costs, pairs, IJ, anchors, keep=None):
    """The three pair-source forms of one bound data set against the host's values pairs(IJ), bit for bit: explicit pairs
    (metric_pairs on IJ, then on IJ without its last 3 pairs: another last wavefront), one-to-all (pick_anchors_selected writes
    the anchors' columns of D), and positions into the pair list (the list that build_locality makes with every anchor in every
    neighbourhood, evaluated in place as a fit's sampling step does; `keep` picks the listed pairs the host has values for)."""
    from annchor_amd import _native

    nx = len(X)
    want = pairs(IJ)
    eng = bound(X, costs)
    try:
        got = eng.metric_pairs(IJ)
        assert np.array_equal(got, want)
        assert np.array_equal(eng.metric_pairs(IJ[:-3]), want[:-3])
        eng.pick_anchors_selected(anchors)
        D = eng.download(_native.F_D).reshape(nx, len(anchors))
        for col, a in enumerate(anchors):
            assert np.array_equal(D[:, col], pairs(np.stack([np.full(nx, a), np.arange(nx)], axis=1)))
        n, _ = eng.build_locality(len(anchors), 1, nx - 1)
        eng.compute_features()
        listed = eng.download(_native.F_IJS).reshape(-1, 2)
        assert n == len(listed) > 0
        pos = np.arange(n, dtype=np.int64) if keep is None else np.flatnonzero(keep(listed)).astype(np.int64)
        assert len(pos) >= nx - 1
        assert np.array_equal(eng.evaluate_samples(pos), pairs(listed[pos]))
    finally:
        eng.close()
    return got


def from_matrix(T):
    def pairs(IJ):
        IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
        return np.asarray(T[IJ[:, 0], IJ[:, 1]])

    return pairs


# ------------------------------------------------------------------------------------------------------- 1. lengths
@pytest.mark.parametrize("kind", ["dyadic", "ragged"])
@pytest.mark.parametrize("shape", [0, 1, 2])
def test_lengths(shape, kind):
    """The lane model's lengths -- 0, 1, 2, R-1, R, R+1, 2R, GR-1, GR on the two small shapes, 0, 1, 2, R+1, 1023, 1024 on the widest,
    the empty string first and last in the pool -- all crossed in both orders; the data set's longest string picks the shape."""
    R, G = oc.SHAPES[shape]
    Ls = oc.lane_lengths(shape)
    assert max(Ls) == R * G and Ls[0] == 0 and Ls[-1] == 0
    costs = oc.dyadic(5, seed=40 + shape) if kind == "dyadic" else oc.ragged_costs(5, seed=40 + shape)
    X = oc.one_of_each_length(Ls, 5, seed=60 + shape)
    T = host_matrix(("lengths", shape, kind), X, costs)
    wed = wc.wed_pairs_host(X, oc.all_ordered_pairs(len(X)), oc.wed_part(costs))
    assert np.all(np.isfinite(T)) and np.any(T.ravel() < wed)          # the fourth term is in the values
    got = three_forms(X, costs, from_matrix(T), oc.all_ordered_pairs(len(X)), [0, len(X) - 2, 1])
    assert np.all(got.reshape(len(X), -1).diagonal() == 0.0)


# ------------------------------------------------------------------------------------------------ 2. alphabet extents
@pytest.mark.parametrize("A", [1, 2, 127, 128])
def test_alphabet_extents(A):
    """Strings that use every symbol of the alphabet, a swapped copy of the longest and the empty string first and last: code A-1
    against code A-1 and code 0 against code A-1 among them (the last entry of the table, the last entry of a row, the last
    indel cost).  A = 127 and 128: the table's stride is A, and its 127 KiB / 129 KiB take the large-LDS launch."""
    costs = oc.below_every_cost(oc.ragged_costs(A, seed=A))
    X = oc.using_every_symbol(A, seed=A)
    X = [""] + X + [X[-1][:3] + X[-1][4] + X[-1][3] + X[-1][5:], ""]
    T = host_matrix(("alphabet", A), X, costs)
    got = three_forms(X, costs, from_matrix(T), oc.all_ordered_pairs(len(X)), [1, len(X) - 2, 0]).reshape(len(X), -1)
    k = len(X) - 2
    assert X[k] == X[k - 1] or got[k - 1, k] == costs.T == got[k, k - 1]
    assert got[1, 2] == oc.osa_loop(X[1], X[2], costs)


# --------------------------------------------------------------------------------------- 3. single swaps, every position
@pytest.mark.parametrize("shape", [0, 1, 2])
def test_single_swaps_at_every_position(shape):
    """osa(base, base with (p, p+1) swapped) == T for every p, with T below every other cost: the fourth term on every lane's
    row 0 and row 1, on column 1 and on row 1 of lane 0 (test_osa_host.py has the reasoning).  The base is the anchor of the
    one-to-all form, and the positions form evaluates the listed pairs that hold it; the data set's last member has R G
    symbols and picks the shape."""
    X, IJ = oc.swap_case(shape)
    nx = len(X)
    costs = oc.below_every_cost(oc.ragged_costs(5, seed=80 + shape))
    base_to_all = np.stack([np.zeros(nx, dtype=np.int64), np.arange(nx)], axis=1)
    col = ref(("swaps", shape), lambda: oc.osa_pairs_host(X, base_to_all, costs))
    assert col[0] == 0.0 and np.all(col[1:nx - 1] == costs.T) and col[nx - 1] > costs.T

    def pairs(IJ_):
        IJ_ = np.asarray(IJ_, dtype=np.int64).reshape(-1, 2)
        assert np.all(IJ_.min(axis=1) == 0)
        return np.asarray(col[IJ_.max(axis=1)])

    got = three_forms(X, costs, pairs, IJ, [0], keep=lambda listed: (listed == 0).any(axis=1))
    assert np.all(got == costs.T)


# -------------------------------------------------------------- 4. one scratch engine, rebound between the three string metrics
def test_transpose_inf_equals_weighted_levenshtein_on_one_scratch_engine():
    """The scratch engine of the loose-object calls, rebound in turn between osa (transpose = +inf), weighted_levenshtein and
    affine_gap on the same strings and table: osa's values are weighted_levenshtein's bit for bit, each metric answers with its
    own values whatever was bound before, and with a finite transpose osa differs.  Lengths up to 300: the (8, 64) shape."""
    w = wc.ragged_costs(7, seed=12)
    X = oc.one_of_each_length(list(range(0, 60, 3)) + [97, 128, 129, 200, 300], 7, seed=13)
    X[3] = X[2][:1] + X[2][2] + X[2][1] + X[2][3:]             # a swapped neighbour
    IJ = oc.all_ordered_pairs(len(X))
    xs, ys = [X[i] for i in IJ[:, 0]], [X[j] for j in IJ[:, 1]]
    c_inf, c_fin, c_aff = oc.with_transpose(w, np.inf), oc.with_transpose(w, 0.2), ac.with_open(w, 0.7)
    m_inf, m_fin, m_wed, m_aff = oc.metric_of(c_inf), oc.metric_of(c_fin), wc.metric_of(w), ac.metric_of(c_aff)
    want_wed = wc.wed_pairs_host(X, IJ, w)
    want_fin = oc.osa_pairs_host(X, IJ, c_fin)
    want_aff = ac.affine_pairs_host(X, IJ, c_aff)
    assert not np.array_equal(want_fin, want_wed) and not np.array_equal(want_aff, want_wed)
    assert m_inf._scratch_engine() is m_wed._scratch_engine() is m_aff._scratch_engine()
    g_inf = m_inf.many(xs, ys)
    g_wed = m_wed.many(xs, ys)
    assert np.array_equal(g_inf, g_wed) and np.array_equal(g_wed, want_wed)
    assert np.array_equal(m_aff.many(xs, ys), want_aff)
    assert np.array_equal(m_fin.many(xs, ys), want_fin)
    assert np.array_equal(m_wed.many(xs, ys), want_wed)
    assert np.array_equal(m_inf.many(xs, ys), want_wed)
    assert np.array_equal(m_aff.many(xs, ys), want_aff)
    assert np.array_equal(m_fin.many(xs, ys), want_fin)


# ------------------------------------------------------------------------------------ 5. two transpose values in turn
def test_two_transpose_values_rebound_in_turn():
    """Two engines on the same strings and table with different transpose, then ONE engine rebound between the two: the values are
    those of what is bound at that moment."""
    X = oc.one_of_each_length([0, 3, 9, 20, 33, 47, 60, 130], 5, seed=6)
    X[2] = X[3][:9]
    X[2] = X[2][:4] + X[2][5] + X[2][4] + X[2][6:]
    IJ = oc.all_ordered_pairs(len(X))
    c1 = oc.ragged_costs(5, seed=4, T=0.2)
    c2 = oc.with_transpose(c1, 1.1)
    w1, w2 = oc.osa_pairs_host(X, IJ, c1), oc.osa_pairs_host(X, IJ, c2)
    assert not np.array_equal(w1, w2)
    e1, e2 = bound(X, c1), bound(X, c2)
    g1, g2, g1b = e1.metric_pairs(IJ), e2.metric_pairs(IJ), e1.metric_pairs(IJ)
    e2.close()
    assert np.array_equal(g1, w1) and np.array_equal(g2, w2) and np.array_equal(g1b, w1)
    oc.metric_of(c2).bind(e1, X)
    assert np.array_equal(e1.metric_pairs(IJ), w2)
    oc.metric_of(c1).bind(e1, X)
    assert np.array_equal(e1.metric_pairs(IJ), w1)
    e1.close()


# ------------------------------------------------------------------------------------------------------ 6. BruteForce
def test_brute_force():
    from annchor_amd import BruteForce

    X = oc.brute_strings()
    assert len(X) == 200 and min(map(len, X)) >= 20 and max(map(len, X)) <= 60 and len({len(x) for x in X}) > 20
    bf = BruteForce(X, NAME, func_kwargs=FIT_KW).fit()
    nx = len(X)
    T = host_matrix("brute", X, oc.fit_costs())
    off = T[~np.eye(nx, dtype=bool)].reshape(nx, nx - 1)
    assert all(len(np.unique(row)) == nx - 1 for row in off)   # no ties within a row: the index comparison rests on no tie rule
    oi, od, _ = O.brute_force(lambda IJ: T[IJ[:, 0], IJ[:, 1]], nx)
    assert np.array_equal(bf.neighbor_graph[1], od)
    assert np.array_equal(bf.neighbor_graph[0], oi)


# ---------------------------------------------------------------------------------------------------- 7. fit, 8. query
def queries():
    """An empty string, a string of 1024 symbols and 18 strings of 5..90 symbols: the engine that holds X and Q runs the widest
    shape."""
    Q = ["", oc.one_of_each_length([oc.MAX_LENGTH], wc.FIT_A, seed=34)[0]] + oc.mutated_strings(18, 5, 90, wc.FIT_A, seed=35, edits=0.6)
    assert len(Q) == 20 and len({len(q) for q in Q}) > 8 and len(Q[1]) == oc.MAX_LENGTH
    return Q


def fit_matrix():
    """Every pair of the fit data set and the queries, [260, 260]."""
    return host_matrix("fit", oc.fit_strings() + queries(), oc.fit_costs())


def fit_pairs(IJ):
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    return np.asarray(fit_matrix()[IJ[:, 0], IJ[:, 1]])


_FITTED = {}


def fitted(capsys=None):
    """The device fit and the CPU pipeline's fit with the host reference as metric, once."""
    from annchor_amd import Annchor

    if not _FITTED:
        X = oc.fit_strings()
        Annchor(X, NAME, func_kwargs=FIT_KW, **FIT_CFG)
        note = capsys.readouterr().err if capsys else ""
        dev = Annchor(X, NAME, func_kwargs=FIT_KW, is_metric=False, ols="lapack", **FIT_CFG)
        quiet = capsys.readouterr().err if capsys else ""
        dev.fit()
        host = Annchor(X, NAME, func_kwargs=FIT_KW, is_metric=False, ols="lapack", get_exact_ijs=lambda f, Xs, IJ: fit_pairs(IJ),
                       **FIT_CFG).fit()
        _FITTED.update(dev=dev, host=host, note=note, quiet=quiet)
    return _FITTED


def test_fit_parity_with_the_cpu_pipeline(capsys):
    """FIT_CFG's shape: 240 strings of 20 .. 60 symbols over 12 symbols, mutated by adjacent swaps as well as edits, is_metric=False,
    costs a shortest-path closure of random weights (distinct distances).  The graph is the CPU pipeline's with the host
    reference as metric; and the fit is not vacuous: most of the pairs it evaluated have a value that weighted Levenshtein does
    not give."""
    X = oc.fit_strings()
    nx = len(X)
    T = fit_matrix()[:nx, :nx]
    off = T[~np.eye(nx, dtype=bool)].reshape(nx, nx - 1)
    assert all(len(np.unique(row)) == nx - 1 for row in off)   # no ties within a row: the index comparisons rest on no tie rule
    f = fitted(capsys)
    dev, host = f["dev"], f["host"]
    assert "triangle inequality" in f["note"] and "triangle inequality" not in f["quiet"]
    assert dev.evals == host.evals
    assert np.array_equal(dev.neighbor_graph[1], host.neighbor_graph[1])
    assert np.array_equal(dev.neighbor_graph[0], host.neighbor_graph[0])
    idx, dist = dev.neighbor_graph
    NN = np.stack([np.repeat(np.arange(nx), idx.shape[1]), np.asarray(idx).ravel()], axis=1)
    assert np.array_equal(np.asarray(dist).ravel(), fit_pairs(NN))
    # the anchor rows and the refined pairs are the host's values (one-to-all and positions forms inside a fit)
    for col, a in enumerate(np.asarray(dev.A)):
        assert np.array_equal(dev.D[:, col], T[a])
    done = ~dev.not_computed_mask
    evaluated = dev.IJs[done]
    assert done.sum() >= dev.evals - dev.n_anchors * nx > 0
    assert np.array_equal(dev.RefineApprox[done], fit_pairs(evaluated))
    # not vacuous, on the host reference: the share of the evaluated pairs that the fourth term decides
    wed = ref("fit_wed", lambda: wc.wed_pairs_host(X, evaluated, oc.wed_part(oc.fit_costs())))
    share = float((fit_pairs(evaluated) < wed).mean())
    print("evaluated pairs that differ from weighted Levenshtein: %.3f of %d" % (share, len(evaluated)))
    assert share > 0.25


def test_query_with_an_empty_and_a_1024_symbol_string(capsys):
    X, Q = oc.fit_strings(), queries()
    nx = len(X)
    f = fitted(capsys)
    dev, host = f["dev"], f["host"]

    def query_evaluator(fn, Xs, Z, IJ):
        """Pairs (Xs[i], Z[j]); Xs is the data set, or its anchors in the order of host.A."""
        IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
        rows = IJ[:, 0] if len(Xs) == nx else np.asarray(host.A, dtype=np.int64)[IJ[:, 0]]
        return fit_pairs(np.stack([rows, IJ[:, 1] + nx], axis=1))

    gi, gd = dev.query(Q, nn=5, p_work=0.3)
    hi, hd = host.query(Q, nn=5, p_work=0.3, get_exact_query_ijs=query_evaluator)
    assert dev.query_evals == host.query_evals
    assert np.array_equal(gd, hd)
    assert np.array_equal(gi, hi)
    QI = np.stack([np.repeat(np.arange(len(Q)) + nx, gi.shape[1]), np.asarray(gi).ravel()], axis=1)
    assert np.array_equal(np.asarray(gd).ravel(), fit_pairs(QI))


# --------------------------------------------------------------------------------------- 9. loose objects, refusals
def test_loose_objects():
    from annchor_amd.distances import OSA

    costs = oc.below_every_cost(oc.ragged_costs(26, seed=10))
    m = oc.metric_of(costs)
    d = m("kitten", "sitting")
    assert isinstance(d, float) and d == oc.osa_loop("kitten", "sitting", costs) == m("sitting", "kitten")
    assert m("", "") == 0.0 and m("abc", "") == oc.osa_loop("abc", "", costs) == m("", "abc")
    assert m("form", "from") == costs.T == m("from", "form")
    ys = ["", "kitchen", "mitten", "k", "iktten", "sittingsittingsitting"]
    assert np.array_equal(m.one_to_many("kitten", ys), [oc.osa_loop("kitten", y, costs) for y in ys])
    assert np.array_equal(m.many(ys, ys[::-1]), [oc.osa_loop(x, y, costs) for x, y in zip(ys, ys[::-1])])
    # known answers at unit costs; ("ca", "abc") = 3 is what tells this from the unrestricted Damerau-Levenshtein distance
    u = OSA.unit("abcd")
    pairs = [("ab", "ba", 1.0), ("ca", "abc", 3.0), ("abcd", "acbd", 1.0), ("abc", "", 3.0), ("", "", 0.0), ("aa", "aa", 0.0)]
    assert u.many([p[0] for p in pairs], [p[1] for p in pairs]).tolist() == [p[2] for p in pairs]
    assert u.many([p[1] for p in pairs], [p[0] for p in pairs]).tolist() == [p[2] for p in pairs]


def test_refusals():
    from annchor_amd import BruteForce, _native

    kw = oc.kwargs_of(oc.dyadic(3))
    with pytest.raises(ValueError, match="osa: string 1 holds the symbol 'x', which is not in the alphabet"):
        BruteForce(["abc", "abx", "a"], NAME, func_kwargs=kw)
    with pytest.raises(ValueError, match="osa: string 2 has 1025 symbols; at most 1024"):
        BruteForce(["abc", "", "a" * 1025], NAME, func_kwargs=kw)
    with pytest.raises(ValueError, match=r"osa: transpose = -1.0 is not a cost >= 0"):
        BruteForce(["a", "b"], NAME, func_kwargs={"alphabet": "ab", "substitution": [[0, 1], [1, 0]], "transpose": -1.0})
    with pytest.raises(AssertionError, match="requires alphabet and substitution"):
        BruteForce(["a", "b"], NAME)
    # the library's own checks, behind the host's; after each refusal the data set bound before still answers
    S, g, T = 1.0 - np.eye(3), np.ones(3), 0.5
    codes, offs, lens = np.array([0, 1, 2, 0, 2, 1], dtype=np.uint8), np.array([0, 3]), np.array([3, 3])
    IJ = np.array([[0, 1], [1, 0], [1, 1]])
    want = [0.5, 0.5, 0.0]          # "abc" / "acb": one swap
    eng = _native.Engine(0)
    try:
        eng.set_coded_strings_osa(codes, offs, lens, S, g, T)
        assert eng.metric == _native.METRIC_OSA == 29
        assert eng.metric_pairs(IJ).tolist() == want
        for bad_T in (np.nan, -0.5, -np.inf):
            with pytest.raises(_native.NativeError, match=r"error -1: osa: transpose is not a cost >= 0"):
                eng.set_coded_strings_osa(codes, offs, lens, S, g, bad_T)
            assert eng.metric_pairs(IJ).tolist() == want
        long = np.zeros(1025 + 2, dtype=np.uint8)
        with pytest.raises(_native.NativeError, match=r"error -4: string 0 has 1025 symbols: osa supports 0\.\.1024"):
            eng.set_coded_strings_osa(long, np.array([0, 1025]), np.array([1025, 2]), S, g, T)
        assert eng.metric_pairs(IJ).tolist() == want
        bad = codes.copy()
        bad[4] = 3
        with pytest.raises(_native.NativeError, match=r"error -1: string 1 holds code 3: the alphabet has 3 symbols"):
            eng.set_coded_strings_osa(bad, offs, lens, S, g, T)
        with pytest.raises(_native.NativeError, match=r"error -4: alphabet=129: osa supports 1\.\.128"):
            eng.set_coded_strings_osa(codes, offs, lens, 1.0 - np.eye(129), np.ones(129), T)
        with pytest.raises(_native.NativeError, match=r"error -1: osa: substitution\[0\]\[0\] is not 0"):
            eng.set_coded_strings_osa(codes, offs, lens, S + np.eye(3), g, T)
        with pytest.raises(_native.NativeError, match=r"error -1: osa: indel\[1\] is not a finite cost"):
            eng.set_coded_strings_osa(codes, offs, lens, S, np.array([1.0, -1.0, 1.0]), T)
        assert eng.metric_pairs(IJ).tolist() == want
        # +inf is taken and means "no transpositions": two substitutions; and the limit itself is taken
        eng.set_coded_strings_osa(codes, offs, lens, S, g, np.inf)
        assert eng.metric_pairs(IJ).tolist() == [2.0, 2.0, 0.0]
        two = np.concatenate([np.zeros(1024, dtype=np.uint8), np.array([1, 1], dtype=np.uint8)])
        eng.set_coded_strings_osa(two, np.array([0, 1024]), np.array([1024, 2]), S, g, T)
        assert eng.metric_pairs(np.array([[0, 1]])).tolist() == [1022.0 + 2.0]
    finally:
        eng.close()
