"""The Jaccard distance on the device (csrc/jaccard.hip), both forms, against the host definition of jaccard_cases.py.

Tolerance: none.  A kernel counts an intersection in integers and makes one float64 division of fixed operands, so lane assignment,
probe side, form and reduction order cannot change a bit; each comparison of distances below is np.array_equal."""
import numpy as np
import pytest

import jaccard_cases as jc
import pool_cases as pc
from oracle import annchor_oracle as O

pytestmark = pytest.mark.gpu

ref = pc.ref_cache()
FORMS = ["tokens", "bits"]


# ----------------------------------------------------------------------------------------------------- 1. small sizes
def small_sets():
    return jc.one_of_each_size(range(0, 97), 150, seed=21)


@pytest.mark.parametrize("form", FORMS)
def test_small_sizes(form):
    """One member of each size 0..96 over 150 tokens, all ordered pairs: n < m, n > m, n = m, the empty set on either side and
    on both, pairs of unequal sizes in one wavefront; then the list without its last 3 pairs.  Both forms give the same array."""
    X = small_sets()
    IJ = jc.all_ordered_pairs(len(X))
    want = ref("small", lambda: jc.jaccard_pairs_host(X, IJ))
    assert want[0] == 0.0 and np.all(want[1:len(X)] == 1.0)   # (empty, empty), (empty, A)
    eng = pc.bound("jaccard", X, form=form)
    got, got_part = eng.metric_pairs(IJ), eng.metric_pairs(IJ[:-3])
    eng.close()
    assert np.array_equal(got, want)
    assert np.array_equal(got_part, want[:-3])
    assert np.all(got[IJ[:, 0] == IJ[:, 1]] == 0.0)


# ------------------------------------------------------------------------------------------ 2. group boundaries, tokens
@pytest.mark.parametrize("G", [4, 16, 64])
def test_group_boundaries(G):
    """The sizes {0, 1, G-1, G, G+1, 2G, 64G-1, 64G, 64G+1} of every G, all ordered pairs.  The kernel is chosen by the data set's
    largest member, so the data set that runs instantiation G holds these sizes up to that G's limit and a member at the limit
    (G = 64: up to 64 G + 1; its limit, 65536, is test_largest_members').  Every size runs on the instantiation that takes it and,
    being below the larger limits too, on every wider one."""
    every = jc.boundary_sizes()
    assert {L for g in (4, 16, 64) for L in (0, 1, g - 1, g, g + 1, 2 * g, 64 * g - 1, 64 * g, 64 * g + 1)} == set(every)
    limit = jc.group_limit(G)
    sizes = sorted({L for L in every if L <= limit} | ({limit} if G < 64 else set()))
    X = jc.one_of_each_size(sizes, 2 * max(sizes), seed=30 + G)
    longest = max(map(len, X))
    assert longest == (limit if G < 64 else 64 * G + 1) and jc.token_group(longest) == G
    IJ = jc.all_ordered_pairs(len(X))
    want = jc.jaccard_pairs_host(X, IJ)
    assert len(np.unique(want)) > len(sizes)
    got = pc.device_pairs("jaccard", X, IJ, form="tokens")
    assert np.array_equal(got, want)


def test_largest_members():
    """A 65536-token member and a 65535-token member against sizes {0, 1, 65536}, in both orders, and against each other."""
    rng = np.random.default_rng(40)
    pick = lambda L: rng.permutation(100000)[:L].astype(np.int64)
    X = [pick(65536), pick(65535), pick(0), pick(1), pick(65536)]
    assert jc.token_group(65536) == 64
    IJ = np.array([p for k in (0, 1) for q in (2, 3, 4) for p in ((k, q), (q, k))] + [(0, 1), (1, 0)], dtype=np.int64)
    want = jc.jaccard_pairs_host(X, IJ)
    assert np.all(want[np.any(IJ == 2, axis=1)] == 1.0) and np.all(want[np.all(IJ != 2, axis=1)] > 0.0)
    assert np.all(want[np.all((IJ != 2) & (IJ != 3), axis=1)] < 1.0)
    got = pc.device_pairs("jaccard", X, IJ, form="tokens")
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ 3. hit position
def hit_cases(G, n, m):
    """Probe side: the n odd tokens 1, 3, ..; searched side: the m even tokens 0, 2, ..; m > n.  One common token is added: the
    probe at position p joins the searched side, or the searched side's first / last token joins the probe side."""
    probe, searched = 2 * np.arange(n) + 1, 2 * np.arange(m)
    X, pairs = [], []
    for p in sorted({0, n - 1, G - 1, G, 2 * G - 1, 2 * G}):
        X += [probe, np.append(searched, probe[p])]
        pairs.append((n, m + 1))
    for v in (searched[0], searched[-1]):
        X += [np.append(probe, v), searched]
        pairs.append((n + 1, m))
    return X, pairs


@pytest.mark.parametrize("G, n, m", [(4, 11, 40), (16, 35, 600), (64, 131, 4200)])
def test_hit_position(G, n, m):
    """Two members disjoint except for one common token, at the first and last position of the probe side, of the searched side,
    and at probe positions G-1, G, 2G-1, 2G: each value is (u - 1) / u.  Then all tokens common except one."""
    assert jc.token_group(m + 1) == G and 2 * G < n < m
    X, sizes = hit_cases(G, n, m)
    IJ = np.array([q for k in range(0, len(X), 2) for q in ((k, k + 1), (k + 1, k))], dtype=np.int64)
    u = np.repeat([a + b - 1 for a, b in sizes], 2).astype(np.float64)
    want = (u - 1.0) / u
    assert np.array_equal(jc.jaccard_pairs_host(X, IJ), want)
    got = pc.device_pairs("jaccard", X, IJ, form="tokens")
    assert np.array_equal(got, want)
    # all common except one: the probes are every third token of the searched side, the probe at position p is replaced by
    # an odd token next to it
    searched = 2 * np.arange(m)
    base = searched[1:3 * n:3]
    assert len(base) == n
    Y = [searched]
    for p in sorted({0, n - 1, G - 1, G, 2 * G - 1, 2 * G}):
        y = base.copy()
        y[p] += 1
        Y.append(y)
    IJ = np.array([q for k in range(1, len(Y)) for q in ((k, 0), (0, k))], dtype=np.int64)
    want = np.full(len(IJ), (m + 1 - (n - 1)) / (m + 1.0))
    assert np.array_equal(jc.jaccard_pairs_host(Y, IJ), want)
    got = pc.device_pairs("jaccard", Y, IJ, form="tokens")
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------- 4. word boundaries, bits
@pytest.mark.parametrize("nbits", [1, 31, 32, 33, 127, 128, 129, 511, 512, 513, 2048, 2049, 8191, 8192])
def test_word_boundaries(nbits):
    """A few random rows, pairs of rows whose only common bit is bit 0, 31, 32, nbits - 1, an all-ones row and an all-zero row:
    the last uint4 of a row, the switch of G at W / 4 = 4 and 16, the empty set."""
    rng = np.random.default_rng(nbits)
    rows = list(jc.fingerprints(4, nbits, 0.3, seed=50 + nbits))
    only = sorted({b for b in (0, 31, 32, nbits - 1) if b < nbits})
    first_only = len(rows)
    for b in only:
        side = rng.random(nbits) < 0.5
        a, c = side.copy(), ~side
        a[b] = c[b] = True
        rows += [a, c]
    rows += [np.ones(nbits, dtype=bool), np.zeros(nbits, dtype=bool)]
    M = np.stack(rows)
    IJ = jc.all_ordered_pairs(len(M))
    want = jc.jaccard_pairs_host(M, IJ).reshape(len(M), len(M))
    for k in range(len(only)):
        assert want[first_only + 2 * k, first_only + 2 * k + 1] == (nbits - 1.0) / nbits
    assert want[-1, -1] == 0.0 and want[-1, -2] == want[-2, -1] == 1.0 and want[-2, -2] == 0.0
    got = pc.device_pairs("jaccard", M, IJ, form="bits")
    assert np.array_equal(got.reshape(want.shape), want)
    assert jc.bits_group(nbits) == (4 if nbits <= 512 else 16 if nbits <= 2048 else 64)


# ------------------------------------------------------------------------------------------------- 5. both forms agree
@pytest.mark.parametrize("seed", [7, 8])
def test_both_forms_agree(seed):
    from annchor_amd.distances import Jaccard

    X = jc.proto_sets(120, 6, 1500, seed)
    M = jc.indicator_matrix(X, 1500)
    IJ = jc.all_ordered_pairs(len(X))[::5]
    want = jc.jaccard_pairs_host(X, IJ)
    assert Jaccard().form_for(M) == "bits"
    tokens = pc.device_pairs("jaccard", X, IJ, form="tokens")
    bits = pc.device_pairs("jaccard", M, IJ, form="bits")
    auto = pc.device_pairs("jaccard", M, IJ, form="auto")
    assert np.array_equal(tokens, want)
    assert np.array_equal(bits, tokens)
    assert np.array_equal(auto, tokens)


# ----------------------------------------------------------------------------------------------- 6. PairSource forms
def fit_data():
    X = jc.fit_sets()
    rng = np.random.default_rng(4)
    X[7] = np.concatenate([X[3], X[3][:9]])[rng.permutation(len(X[3]) + 9)]   # the same set, in another order, with repeats
    return X


def fit_ref():
    """Every pair of the fit data set, [nx * nx]."""
    return ref("fit", lambda: pc.sym_matrix(jc.jaccard_pairs_host, fit_data()).ravel())


def fit_pairs(IJ):
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    return np.asarray(fit_ref()[IJ[:, 0] * 240 + IJ[:, 1]])


@pytest.mark.parametrize("form", FORMS)
def test_pair_source_forms(form):
    """Explicit pairs (metric_pairs), one-to-all (the anchor rows of a fit: ann.D), and positions into the pair list with the
    result written to RefineApprox / not_computed_mask (the sampling and refinement stages of a fit)."""
    from annchor_amd import Annchor, _native

    X = fit_data()
    nx = len(X)
    IJ = jc.all_ordered_pairs(nx)[::7]
    eng = pc.bound("jaccard", X, form=form)
    assert eng.metric == (_native.METRIC_JACCARD_TOKENS if form == "tokens" else _native.METRIC_JACCARD_BITS)
    got = eng.metric_pairs(IJ)
    assert np.array_equal(got, fit_pairs(IJ))
    assert eng.metric_pairs(np.array([[3, 7], [7, 3], [5, 5]])).tolist() == [0.0, 0.0, 0.0]
    eng.pick_anchors_selected([3, 100])
    D = eng.download(_native.F_D).reshape(nx, 2)
    eng.close()
    for col, a in enumerate((3, 100)):
        assert np.array_equal(D[:, col], fit_pairs(np.stack([np.full(nx, a), np.arange(nx)], 1)))
    assert D[7, 0] == 0.0 and D[3, 0] == 0.0
    ann = Annchor(X, "jaccard", func_kwargs={"form": form}, **jc.FIT_CFG).fit()
    A = np.asarray(ann.A)
    for col, a in enumerate(A):
        assert np.array_equal(ann.D[:, col], fit_pairs(np.stack([np.full(nx, a), np.arange(nx)], 1)))
    done = ~ann.not_computed_mask
    assert done.sum() >= ann.evals - ann.n_anchors * nx > 0
    assert np.array_equal(ann.RefineApprox[done], fit_pairs(ann.IJs[done]))


# ------------------------------------------------------------------------------------------------------ 7. BruteForce
def test_brute_force():
    from annchor_amd import BruteForce

    X = jc.brute_sets()
    assert len(X) == 200 and len({len(jc.as_tokens(x)) for x in X}) > 20
    bf = BruteForce(X, "jaccard").fit()
    nx = len(X)
    T = pc.sym_matrix(jc.jaccard_pairs_host, X)
    oi, od, _ = O.brute_force(lambda IJ: T[IJ[:, 0], IJ[:, 1]], nx)
    assert np.array_equal(bf.neighbor_graph[1], od)
    assert np.array_equal(bf.neighbor_graph[0], oi)


# ---------------------------------------------------------------------------------------------------------- 8. fits
def fit_case(name):
    """(X, pairs(IJ)) of a fit test: the window sets as token lists (a third of the pairs tie at 1.0: the tie rules of the
    selection stages decide), the prototype sets as a bool matrix (no pair at 1.0)."""
    if name == "windows":
        X = jc.fit_sets()
        T = ref("fit_windows", lambda: pc.sym_matrix(jc.jaccard_pairs_host, X).ravel())
    else:
        X = jc.fit_protos()
        T = ref("fit_protos", lambda: pc.sym_matrix(jc.jaccard_pairs_host, X).ravel())

    def pairs(IJ):
        IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
        return np.asarray(T[IJ[:, 0] * len(X) + IJ[:, 1]])

    return X, pairs


@pytest.mark.parametrize("name, form", [("windows", "auto"), ("windows", "tokens"), ("protos", "auto")])
def test_fit_parity_with_the_cpu_pipeline(name, form, capsys):
    """Recorded, not asserted (p_work = 0.3, is_metric=True): windows -- see DESIGN.md section 3.14."""
    from annchor_amd import Annchor, compare_neighbor_graphs

    X, pairs = fit_case(name)
    nx = len(X)
    kw = {} if form == "auto" else {"func_kwargs": {"form": form}}
    ann = Annchor(X, "jaccard", ols="lapack", **kw, **jc.FIT_CFG).fit()
    ora = O.OracleAnnchor(nx, pairs, **jc.FIT_CFG).fit()
    assert np.array_equal(ann.A, ora.A)
    assert np.array_equal(ann.D, ora.D)
    assert ann.evals == ora.evals
    assert np.array_equal(ann.neighbor_graph[1], ora.neighbor_graph[1])
    assert np.array_equal(ann.neighbor_graph[0], ora.neighbor_graph[0])
    # the default solver: whatever the graph lists is an exact distance, and no note about the triangle inequality
    dflt = Annchor(X, "jaccard", **kw, **jc.FIT_CFG).fit()
    assert "triangle inequality" not in capsys.readouterr().err
    idx, dist = dflt.neighbor_graph
    IJ = np.stack([np.repeat(np.arange(nx), idx.shape[1]), np.asarray(idx).ravel()], axis=1)
    assert np.array_equal(np.asarray(dist).ravel(), pairs(IJ))
    # (recorded in DESIGN.md, not asserted: wrong neighbours against the exact graph)
    exact = O.brute_force(pairs, nx)
    k = jc.FIT_CFG["n_neighbors"]
    print("%s, form=%s, is_metric=True, p_work=0.3: %d of %d neighbours differ from the exact graph; %d evaluations"
          % (name, form, compare_neighbor_graphs(exact[:2], dflt.neighbor_graph, k), nx * k, dflt.evals))


# ----------------------------------------------------------------------------------------------------------- 9. query
@pytest.mark.parametrize("name", ["query_rows", "query_lists"])
def test_query(name):
    """X a bool matrix [240, 600] and Q 20 bool rows from another seed; X token lists and Q token lists that hold tokens X never
    saw."""
    from annchor_amd import Annchor

    X, Q = getattr(jc, name)()
    if name == "query_rows":
        assert X.shape == (240, 600) and X.dtype == np.bool_ and Q.shape == (20, 600) and Q.dtype == np.bool_
    else:
        seen = np.unique(np.concatenate(X))
        assert any(np.setdiff1d(q, seen).size for q in Q)
    both = list(X) + list(Q)
    nx = len(X)
    T = pc.sym_matrix(jc.jaccard_pairs_host, both)
    pairs = lambda IJ: T[IJ[:, 0], IJ[:, 1]]
    ann = Annchor(X, "jaccard", ols="lapack", **jc.FIT_CFG).fit()
    gi, gd = ann.query(Q, nn=5, p_work=0.3)
    ora = O.OracleAnnchor(nx, pairs, **jc.FIT_CFG).fit()
    oi, od, info = O.query(ora, lambda IJ: pairs(np.stack([IJ[:, 0], IJ[:, 1] + nx], 1)), len(Q), nn=5, p_work=0.3)
    assert ann.query_evals == info["evals"]
    assert np.array_equal(gd, od)
    assert np.array_equal(gi, oi)


# -------------------------------------------------------------------------------------------------- 10. loose objects
def test_loose_objects():
    from annchor_amd.distances import Jaccard, jaccard

    rng = np.random.default_rng(6)
    xs = [rng.integers(0, 60, L) for L in (5, 40, 0, 130)]
    ys = [rng.integers(0, 60, L) for L in (17, 9, 33, 0)]
    assert jaccard(xs[0], ys[0]) == jc.jaccard_loop(xs[0], ys[0])
    assert jaccard(ys[1], xs[1]) == jc.jaccard_loop(ys[1], xs[1])
    assert np.array_equal(jaccard.many(xs, ys), [jc.jaccard_loop(x, y) for x, y in zip(xs, ys)])
    assert np.array_equal(jaccard.one_to_many(xs[1], ys), [jc.jaccard_loop(xs[1], y) for y in ys])
    tok = Jaccard(form="tokens")
    assert np.array_equal(tok.many(xs, ys), [jc.jaccard_loop(x, y) for x, y in zip(xs, ys)])
    # Python sets, an empty member on either side and on both, bool rows
    assert jaccard({1, 2, 3}, {2, 3, 4}) == 0.5
    assert jaccard(set(), frozenset([7])) == 1.0 and jaccard([9], []) == 1.0 and jaccard(set(), []) == 0.0
    assert tok(set(), frozenset([7])) == 1.0 and tok(set(), set()) == 0.0
    a, b = rng.random(77) < 0.4, rng.random(77) < 0.4
    assert jaccard(a, b) == jc.jaccard_loop(a, b) == tok(b, a)


# --------------------------------------------------------------------------------------------------------- 11. limits
def test_limits():
    from annchor_amd import BruteForce, _native

    ok = np.arange(10)
    with pytest.raises(ValueError, match="jaccard: set 1 has dtype float64"):
        BruteForce([ok, np.array([1.0, 2.0])], "jaccard")
    with pytest.raises(ValueError, match="jaccard: set 0 has 2 dimensions"):
        BruteForce([np.zeros((2, 2), dtype=np.int64), ok], "jaccard")
    with pytest.raises(ValueError, match="jaccard: set 1 is bool and set 0 is int64"):
        BruteForce([ok, np.ones(4, dtype=bool)], "jaccard")
    with pytest.raises(ValueError, match="jaccard: set 1 has 5 bits, set 0 has 4"):
        BruteForce([np.ones(4, dtype=bool), np.ones(5, dtype=bool)], "jaccard")
    with pytest.raises(ValueError, match="jaccard: set 0 has 65537 distinct tokens"):
        BruteForce([np.arange(65537), ok], "jaccard")
    with pytest.raises(ValueError, match="jaccard: form='bits' takes at most 8192 distinct tokens, this list has 8193"):
        BruteForce([np.arange(8193), ok], "jaccard", func_kwargs={"form": "bits"})
    # the library's own checks, behind the host's
    eng = _native.Engine(0)
    try:
        big = np.arange(65537 + 10, dtype=np.int32)
        with pytest.raises(_native.NativeError, match=r"error -4: .*set 0 has 65537 tokens.*0\.\.65536"):
            eng.set_token_sets(big, np.array([0, 65537]), np.array([65537, 10]))
        with pytest.raises(_native.NativeError, match="error -1: .*set 1.*not strictly ascending"):
            eng.set_token_sets(np.array([1, 2, 3, 9, 8], dtype=np.int32), np.array([0, 3]), np.array([3, 2]))
        with pytest.raises(_native.NativeError, match="error -1: .*set 0.*not strictly ascending"):
            eng.set_token_sets(np.array([1, 2, 2, 8, 9], dtype=np.int32), np.array([0, 3]), np.array([3, 2]))
        with pytest.raises(_native.NativeError, match="error -1: .*set 1 holds a negative code"):
            eng.set_token_sets(np.array([1, 2, 3, -8, 9], dtype=np.int32), np.array([0, 3]), np.array([3, 2]))
        with pytest.raises(_native.NativeError, match="error -1: .*set 1 has a negative size"):
            eng.set_token_sets(np.array([1, 2, 3], dtype=np.int32), np.array([0, 3]), np.array([3, -1]))
        with pytest.raises(_native.NativeError, match=r"error -4: nbits=0.*1\.\.8192"):
            eng.set_bitsets(np.zeros((2, 4), dtype=np.uint32), 0)
        with pytest.raises(_native.NativeError, match=r"error -4: nbits=8193.*1\.\.8192"):
            eng.set_bitsets(np.zeros((2, 260), dtype=np.uint32), 8193)
        words = np.zeros((3, 4), dtype=np.uint32)
        words[2, 1] = 1 << 8   # bit 40 of a 40-bit row
        with pytest.raises(_native.NativeError, match="error -1: bitset 2 has a padding bit set"):
            eng.set_bitsets(words, 40)
        words[2, 1] = 0
        words[1, 3] = 1        # a bit in a padding word
        with pytest.raises(_native.NativeError, match="error -1: bitset 1 has a padding bit set"):
            eng.set_bitsets(words, 40)
        # 65536 tokens are taken ...
        eng.set_token_sets(big[:65536 + 10], np.array([0, 65536]), np.array([65536, 10]))
        assert eng.metric_pairs(np.array([[0, 1], [1, 0]])).tolist() == [jc.jaccard_loop(big[:65536], big[65536:65546])] * 2
        eng.set_token_sets(big[:65536 + 10], np.array([0, 0]), np.array([65536, 10]))   # (the second a subset of the first)
        assert eng.metric_pairs(np.array([[0, 1], [1, 0]])).tolist() == [jc.jaccard_loop(big[:65536], big[:10])] * 2
        # ... and 8192 bits
        M = jc.fingerprints(3, 8192, 0.3, seed=9)
        M[:, 8191] = True
        words, nbits = np.packbits(M, axis=1, bitorder="little").view(np.uint32), 8192
        eng.set_bitsets(words, nbits)
        IJ = np.array([[0, 1], [1, 2], [2, 0], [1, 1]])
        assert np.array_equal(eng.metric_pairs(IJ), jc.jaccard_pairs_host(M, IJ))
    finally:
        eng.close()
