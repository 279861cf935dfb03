"""Affine-gap alignment distance on the device (csrc/wed.hip, k_affine) against the host recurrence of affine_cases.py, through
every layer: explicit pairs, the three pair-source forms, BruteForce, Annchor.fit and .query, loose objects, refusals.

Tolerance: none.  Every cell is a min of sums of fixed operands, min is exact and the additions are commutative, so every
evaluation order gives the same bits; each comparison of distances below is np.array_equal."""
import numpy as np
import pytest

import affine_cases as ac
import pool_cases as pc
import wed_cases as wc
from oracle import annchor_oracle as O

pytestmark = pytest.mark.gpu

ref = pc.ref_cache()
NAME = ac.NAME
FIT_CFG = pc.FIT_CFG
FIT_KW = ac.kwargs_of(ac.fit_costs())


def bound(X, costs):
    return pc.bound(NAME, X, **ac.kwargs_of(costs))


def device_pairs(X, IJ, costs):
    return pc.device_pairs(NAME, X, IJ, **ac.kwargs_of(costs))


def fit_host(X, IJ):
    return ac.affine_pairs_host(X, IJ, ac.fit_costs())


def fit_ref():
    """Every pair of the fit data set, [nx * nx]."""
    return ref("fit", lambda: pc.sym_matrix(fit_host, ac.fit_strings()).ravel())


def fit_pairs(IJ):
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    return np.asarray(fit_ref()[IJ[:, 0] * len(ac.fit_strings()) + IJ[:, 1]])


# --------------------------------------------------------------------------------------------------- 1. small lengths
@pytest.mark.parametrize("kind", ["dyadic", "ragged"])
def test_small_lengths(kind):
    """One string of each length 0..96 over 5 symbols, all ordered pairs: n < m, n > m, n = m, the empty string against every
    length, every strip and group boundary of the 4-pairs-per-wavefront shape; then the list without its last 3 pairs (a last
    wavefront with one pair in it)."""
    costs = ac.dyadic(5) if kind == "dyadic" else ac.ragged_costs(5)
    X = ac.one_of_each_length(range(0, 97), 5, seed=41)
    IJ = ac.all_ordered_pairs(len(X))
    want = ref(("small", kind), lambda: ac.affine_pairs_host(X, IJ, costs))
    assert np.all(np.isfinite(want)) and np.all(want[IJ[:, 0] != IJ[:, 1]] > 0)
    eng = bound(X, costs)
    got, got_part = eng.metric_pairs(IJ), eng.metric_pairs(IJ[:-3])
    eng.close()
    assert np.array_equal(got, want)
    assert np.array_equal(got_part, want[:-3])
    assert np.all(got[IJ[:, 0] == IJ[:, 1]] == 0.0)
    assert np.array_equal(got.reshape(len(X), -1), got.reshape(len(X), -1).T)


# ------------------------------------------------------------------------------------------------ 2. boundary lengths
def boundary_case(shape):
    """The data set that runs shape number `shape` -- the kernel is chosen by the data set's longest string -- and its pair list.
    Up to 512 symbols all lengths are crossed; at the widest shape each length meets {0, 1, 16, 1024} in both orders."""
    Ls = ac.boundary_lengths(shape)
    R, G = ac.SHAPES[shape]
    assert max(Ls) == R * G and (shape == 0 or max(ac.boundary_lengths(shape - 1)) == ac.SHAPES[shape - 1][0] * ac.SHAPES[shape - 1][1])
    if shape < 2:
        IJ = ac.all_ordered_pairs(len(Ls))
    else:
        partners = [Ls.index(L) for L in (0, 1, 16, 1024)]
        IJ = np.array([p for k in range(len(Ls)) for q in partners for p in ((k, q), (q, k))], dtype=np.int64)
    return Ls, IJ


@pytest.mark.parametrize("shape", [0, 1, 2])
def test_boundary_lengths(shape):
    """{0, 1, 7, 8, 9, 16, 127, 128} on the (8, 16) shape, with {129, 511, 512} on the (8, 64) shape, with {15, 17, 32, 513, 1023,
    1024} on the (16, 64) shape; non-dyadic costs and open, so that both prefix boundaries and every cell carry values of their
    own."""
    Ls, IJ = boundary_case(shape)
    assert {0, 1, 7, 8, 9, 16, 127, 128} <= set(Ls)
    assert shape < 1 or {129, 511, 512} <= set(Ls)
    assert shape < 2 or {15, 17, 32, 513, 1023, 1024} <= set(Ls)
    costs = ac.ragged_costs(5, seed=50)
    X = ac.one_of_each_length(Ls, 5, seed=50 + shape)
    want = ref(("boundary", shape), lambda: ac.affine_pairs_host(X, IJ, costs))
    assert np.all(np.isfinite(want))
    assert np.array_equal(device_pairs(X, IJ, costs), want)


# ------------------------------------------------------------------------------------------------ 3. alphabet extents
@pytest.mark.parametrize("A", [1, 2, 26, 127, 128])
def test_alphabet_extents(A):
    """40 strings of 1..40 symbols that use every symbol of the alphabet, all ordered pairs: code A-1 against code A-1 and code 0
    against code A-1 among them (the last entry of the table, the last entry of a row, the last extension cost).  A = 127 and
    128: the table's stride is A, and its 127 KiB / 129 KiB take the large-LDS launch."""
    costs = ac.ragged_costs(A, seed=A)
    X = ac.using_every_symbol(A, seed=A)
    IJ = ac.all_ordered_pairs(len(X))
    want = ref(("alphabet", A), lambda: ac.affine_pairs_host(X, IJ, costs))
    got = device_pairs(X, IJ, costs)
    assert np.array_equal(got, want)
    last, first_last = ac.SYMBOLS[A - 1], ac.SYMBOLS[0] + ac.SYMBOLS[A - 1]
    assert X[0] == last and X[1] == first_last and got[0] == 0.0 and got[1] == ac.affine_loop(last, first_last, costs)
    assert A == 1 or got[1] == costs.o + costs.g[0]


# ---------------------------------------------------------------------- 4. open = 0 equals the weighted-Levenshtein kernel
def test_open_zero_equals_the_weighted_levenshtein_kernel():
    """The same strings and table through both kernels: with open = 0.0 the values are k_wed's bit for bit (and the host's); with
    open > 0 they are not.  Lengths up to 300: the (8, 16)-sized members run the (8, 64) shape here."""
    costs0 = ac.ragged_costs(7, seed=12, o=0.0)
    X = ac.one_of_each_length(list(range(0, 60, 3)) + [97, 128, 129, 200, 300], 7, seed=13)
    IJ = ac.all_ordered_pairs(len(X))
    wed = pc.device_pairs("weighted_levenshtein", X, IJ, **wc.kwargs_of(ac.wed_part(costs0)))
    got0 = device_pairs(X, IJ, costs0)
    assert np.array_equal(got0, wed)
    assert np.array_equal(got0, wc.wed_pairs_host(X, IJ, ac.wed_part(costs0)))
    costs = ac.with_open(costs0, ac.RAGGED_OPEN)
    got = device_pairs(X, IJ, costs)
    assert np.array_equal(got, ac.affine_pairs_host(X, IJ, costs))
    off = IJ[:, 0] != IJ[:, 1]
    assert np.all(got[off] >= wed[off]) and np.any(got[off] > wed[off]) and not np.array_equal(got, wed)


# ------------------------------------------------------------------------------------ 5. two opening costs in one process
def test_two_opening_costs_in_one_process():
    """Two engines on the same strings and table with different open: each equals its own reference and the results differ.  Then
    the scratch engine of the loose-object calls, rebound between the two open values and between AffineGap and
    WeightedLevenshtein: the values are those of what is bound at that moment."""
    X = ac.one_of_each_length([0, 3, 9, 20, 33, 47, 60, 130], 5, seed=6)
    IJ = ac.all_ordered_pairs(len(X))
    c1 = ac.ragged_costs(5, seed=4, o=0.7)
    c2 = ac.with_open(c1, 2.5)
    cw = ac.wed_part(c1)
    w1, w2, ww = ac.affine_pairs_host(X, IJ, c1), ac.affine_pairs_host(X, IJ, c2), wc.wed_pairs_host(X, IJ, cw)
    assert not np.array_equal(w1, w2) and not np.array_equal(w1, ww) and not np.array_equal(w2, ww)
    e1, e2 = bound(X, c1), bound(X, c2)
    g1, g2, g1b = e1.metric_pairs(IJ), e2.metric_pairs(IJ), e1.metric_pairs(IJ)
    e1.close()
    e2.close()
    assert np.array_equal(g1, w1) and np.array_equal(g2, w2) and np.array_equal(g1b, w1)
    m1, m2, mw = ac.metric_of(c1), ac.metric_of(c2), wc.metric_of(cw)
    xs, ys = [X[i] for i in IJ[:, 0]], [X[j] for j in IJ[:, 1]]
    assert np.array_equal(m1.many(xs, ys), w1)
    assert np.array_equal(m2.many(xs, ys), w2)
    assert np.array_equal(m1.many(xs, ys), w1)
    assert np.array_equal(mw.many(xs, ys), ww)
    assert np.array_equal(m2.many(xs, ys), w2)
    assert np.array_equal(mw.many(xs, ys), ww)
    assert np.array_equal(m1.many(xs, ys), w1)


# ----------------------------------------------------------------------------------------------- 6. PairSource forms
def test_pair_source_forms():
    """Explicit pairs (metric_pairs), one-to-all (the anchor rows of a fit: pick_anchors_selected and ann.D), and positions into
    the pair list with the result written to RefineApprox / not_computed_mask (the sampling and refinement stages of a fit)."""
    from annchor_amd import Annchor, _native

    X = ac.fit_strings()
    X[7] = X[3]                     # identical members
    nx = len(X)
    IJ = ac.all_ordered_pairs(nx)[::7]
    want = fit_host(X, IJ)
    eng = pc.bound(NAME, X, **FIT_KW)
    got = eng.metric_pairs(IJ)
    assert np.array_equal(got, want)
    assert eng.metric_pairs(np.array([[3, 7], [7, 3], [5, 5]])).tolist() == [0.0, 0.0, 0.0]
    eng.pick_anchors_selected([3, 100])
    D = eng.download(_native.F_D).reshape(nx, 2)
    eng.close()
    for col, a in enumerate((3, 100)):
        assert np.array_equal(D[:, col], fit_host(X, np.stack([np.full(nx, a), np.arange(nx)], 1)))
    assert D[7, 0] == 0.0 and D[3, 0] == 0.0
    ann = Annchor(X, NAME, func_kwargs=FIT_KW, **FIT_CFG).fit()
    A = np.asarray(ann.A)
    for col, a in enumerate(A):
        assert np.array_equal(ann.D[:, col], fit_host(X, np.stack([np.full(nx, a), np.arange(nx)], 1)))
    done = ~ann.not_computed_mask
    assert done.sum() >= ann.evals - ann.n_anchors * nx > 0
    assert np.array_equal(ann.RefineApprox[done], fit_host(X, ann.IJs[done]))


# ------------------------------------------------------------------------------------------------------ 7. BruteForce
def test_brute_force():
    from annchor_amd import BruteForce

    X = ac.brute_strings()
    assert len(X) == 200 and min(map(len, X)) >= 20 and max(map(len, X)) <= 60 and len({len(x) for x in X}) > 20
    bf = BruteForce(X, NAME, func_kwargs=FIT_KW).fit()
    nx = len(X)
    T = pc.sym_matrix(fit_host, X)
    off = T[~np.eye(nx, dtype=bool)].reshape(nx, nx - 1)
    assert all(len(np.unique(row)) == nx - 1 for row in off)   # no ties within a row: the index comparison rests on no tie rule
    oi, od, _ = O.brute_force(lambda IJ: T[IJ[:, 0], IJ[:, 1]], nx)
    assert np.array_equal(bf.neighbor_graph[1], od)
    assert np.array_equal(bf.neighbor_graph[0], oi)


# ---------------------------------------------------------------------------------------------------------- 8. fits
def test_fit_parity_with_the_cpu_pipeline(capsys):
    from annchor_amd import Annchor

    X = ac.fit_strings()
    nx = len(X)
    off = fit_ref().reshape(nx, nx)[~np.eye(nx, dtype=bool)].reshape(nx, nx - 1)
    assert all(len(np.unique(row)) == nx - 1 for row in off)   # no ties within a row: the index comparisons rest on no tie rule
    ann = Annchor(X, NAME, ols="lapack", func_kwargs=FIT_KW, **FIT_CFG)
    assert "triangle inequality" not in capsys.readouterr().err
    ann.fit()
    ora = O.OracleAnnchor(nx, fit_pairs, **FIT_CFG).fit()
    assert np.array_equal(ann.A, ora.A)
    assert np.array_equal(ann.D, ora.D)
    assert ann.evals == ora.evals
    assert np.array_equal(ann.neighbor_graph[1], ora.neighbor_graph[1])
    assert np.array_equal(ann.neighbor_graph[0], ora.neighbor_graph[0])
    # the default solver: whatever the graph lists is an exact distance
    dflt = Annchor(X, NAME, func_kwargs=FIT_KW, **FIT_CFG).fit()
    assert "triangle inequality" not in capsys.readouterr().err
    idx, dist = dflt.neighbor_graph
    IJ = np.stack([np.repeat(np.arange(nx), idx.shape[1]), np.asarray(idx).ravel()], axis=1)
    assert np.array_equal(np.asarray(dist).ravel(), fit_pairs(IJ))


# ----------------------------------------------------------------------------------------------------------- 9. query
def test_query_with_other_lengths():
    """X is the fit data set (20..60 symbols); Q holds an empty string, a string of 1024 symbols and 18 strings of 5..90 symbols:
    the engine that holds X and Q runs the widest shape."""
    from annchor_amd import Annchor

    X = ac.fit_strings()
    Q = ["", ac.one_of_each_length([1024], wc.FIT_A, seed=34)[0]] + ac.clustered_strings(18, 5, 90, wc.FIT_A, seed=35, edits=0.6)
    assert len(Q) == 20 and len({len(q) for q in Q}) > 8 and len(Q[1]) == ac.MAX_LENGTH
    both = list(X) + Q
    nx = len(X)
    ann = Annchor(X, NAME, ols="lapack", func_kwargs=FIT_KW, **FIT_CFG).fit()
    gi, gd = ann.query(Q, nn=5, p_work=0.3)
    ora = O.OracleAnnchor(nx, fit_pairs, **FIT_CFG).fit()
    oi, od, info = O.query(ora, lambda IJ: fit_host(both, np.stack([IJ[:, 0], IJ[:, 1] + nx], 1)), len(Q), nn=5, p_work=0.3)
    assert ann.query_evals == info["evals"]
    assert np.array_equal(gd, od)
    assert np.array_equal(gi, oi)


# --------------------------------------------------------------------------------------- 10. loose objects, refusals
def test_loose_objects():
    costs = ac.ragged_costs(26, seed=10)
    m = ac.metric_of(costs)
    d = m("kitten", "sitting")
    assert isinstance(d, float) and d == ac.affine_loop("kitten", "sitting", costs) == m("sitting", "kitten")
    assert m("", "") == 0.0 and m("abc", "") == ac.affine_loop("abc", "", costs) == m("", "abc")
    ys = ["", "kitchen", "mitten", "k", "sittingsittingsitting"]
    assert np.array_equal(m.one_to_many("kitten", ys), [ac.affine_loop("kitten", y, costs) for y in ys])
    assert np.array_equal(m.many(ys, ys[::-1]), [ac.affine_loop(x, y, costs) for x, y in zip(ys, ys[::-1])])
    # a known answer: unit costs, one gap of three symbols costs open + 3
    from annchor_amd.distances import AffineGap

    assert AffineGap("ab", [[0, 1], [1, 0]], 1.0, 0.5)("abbba", "aa") == 3.5


def test_refusals():
    from annchor_amd import BruteForce, _native

    kw = ac.kwargs_of(ac.dyadic(3))
    with pytest.raises(ValueError, match="affine_gap: string 1 holds the symbol 'x', which is not in the alphabet"):
        BruteForce(["abc", "abx", "a"], NAME, func_kwargs=kw)
    with pytest.raises(ValueError, match="affine_gap: string 2 has 1025 symbols; at most 1024"):
        BruteForce(["abc", "", "a" * 1025], NAME, func_kwargs=kw)
    with pytest.raises(ValueError, match="affine_gap: string 0 is a bytes, not a str"):
        BruteForce([b"abc", "ab"], NAME, func_kwargs=kw)
    with pytest.raises(ValueError, match=r"affine_gap: substitution\[0\]\[1\] = 1.0 but substitution\[1\]\[0\] = 2.0"):
        BruteForce(["a", "b"], NAME, func_kwargs={"alphabet": "ab", "substitution": [[0, 1], [2, 0]]})
    with pytest.raises(ValueError, match=r"affine_gap: open = -1.0 is not a finite cost >= 0"):
        BruteForce(["a", "b"], NAME, func_kwargs={"alphabet": "ab", "substitution": [[0, 1], [1, 0]], "open": -1.0})
    with pytest.raises(AssertionError, match="requires alphabet and substitution"):
        BruteForce(["a", "b"], NAME)
    # the library's own checks, behind the host's; a refusal leaves the engine as it was
    S, g, o = 1.0 - np.eye(3), np.ones(3), 0.5
    codes, offs, lens = np.array([0, 1, 2, 2, 1, 1], dtype=np.uint8), np.array([0, 3]), np.array([3, 3])
    want = [2.0, 0.0]          # "abc" / "cbb": two substitutions (two gaps would cost 3); a member against itself
    eng = _native.Engine(0)
    try:
        eng.set_coded_strings_affine(codes, offs, lens, S, g, o)
        assert eng.metric == _native.METRIC_AFFINE_GAP
        assert eng.metric_pairs(np.array([[0, 1], [1, 1]])).tolist() == want
        bad = codes.copy()
        bad[4] = 3
        with pytest.raises(_native.NativeError, match=r"error -1: string 1 holds code 3: the alphabet has 3 symbols"):
            eng.set_coded_strings_affine(bad, offs, lens, S, g, o)
        long = np.zeros(1025 + 2, dtype=np.uint8)
        with pytest.raises(_native.NativeError, match=r"error -4: string 0 has 1025 symbols: affine_gap supports 0\.\.1024"):
            eng.set_coded_strings_affine(long, np.array([0, 1025]), np.array([1025, 2]), S, g, o)
        with pytest.raises(_native.NativeError, match=r"error -1: string 1 has a negative length"):
            eng.set_coded_strings_affine(codes, offs, np.array([3, -1]), S, g, o)
        with pytest.raises(_native.NativeError, match=r"error -4: alphabet=129: affine_gap supports 1\.\.128"):
            eng.set_coded_strings_affine(codes, offs, lens, 1.0 - np.eye(129), np.ones(129), o)
        for table, match in ((S + np.eye(3), r"substitution\[0\]\[0\] is not 0"),
                             (S - 2 * np.eye(3)[[1, 0, 2]], r"substitution\[0\]\[1\] is not a finite cost"),
                             (np.where(np.eye(3)[[1, 0, 2]] > 0, np.nan, S), r"substitution\[0\]\[1\] is not a finite cost"),
                             (S + np.triu(np.full((3, 3), 2.0 ** -52), 1), r"substitution\[0\]\[1\] != substitution\[1\]\[0\]")):
            with pytest.raises(_native.NativeError, match="error -1: affine_gap: " + match):
                eng.set_coded_strings_affine(codes, offs, lens, table, g, o)
        for extend in (np.array([1.0, -1.0, 1.0]), np.array([1.0, np.inf, 1.0])):
            with pytest.raises(_native.NativeError, match=r"error -1: affine_gap: extend\[1\] is not a finite cost"):
                eng.set_coded_strings_affine(codes, offs, lens, S, extend, o)
        for bad_open in (-0.5, np.nan, np.inf):
            with pytest.raises(_native.NativeError, match=r"error -1: affine_gap: open is not a finite cost >= 0"):
                eng.set_coded_strings_affine(codes, offs, lens, S, g, bad_open)
        assert eng.metric_pairs(np.array([[0, 1], [1, 1]])).tolist() == want
        # the limit itself is taken
        two = np.concatenate([np.zeros(1024, dtype=np.uint8), np.array([1, 1], dtype=np.uint8)])
        eng.set_coded_strings_affine(two, np.array([0, 1024]), np.array([1024, 2]), S, g, o)
        assert eng.metric_pairs(np.array([[0, 1]])).tolist() == [o + 1022.0 + 2.0]
    finally:
        eng.close()
