"""The Jaccard distance on the host: the vectorised helper of jaccard_cases.py against the definition's loop and scipy, the special
values, the triangle inequality, the two packers and their refusals, the form rule, the name lookup, and the usability of the GPU
tests' data (the CPU restatement of the pipeline completes a fit on it; few enough pairs saturate at 1.0).

Tolerance: none.  The value is one division of two exact integers; every comparison is np.array_equal or ==."""
import numpy as np
import pytest

import jaccard_cases as jc
import pool_cases as pc
from oracle import annchor_oracle as O


def test_reference_agreement():
    """jaccard_loop == jaccard_pairs_host == scipy's jaccard on the boolean rows, both orders of every pair, sizes 0 .. 70."""
    X = jc.one_of_each_size(range(0, 71), 110, seed=11)
    IJ = jc.all_ordered_pairs(len(X))
    want = np.array([jc.jaccard_loop(X[i], X[j]) for i, j in IJ])
    got = jc.jaccard_pairs_host(X, IJ)
    assert np.array_equal(got, want)
    n = len(X)
    assert np.array_equal(got.reshape(n, n), got.reshape(n, n).T)
    assert np.all(got[IJ[:, 0] == IJ[:, 1]] == 0.0)
    # bool rows give what the token lists give, and a chunked pass the same
    M = jc.indicator_matrix(X, 110)
    assert np.array_equal(jc.jaccard_pairs_host(M, IJ), want)
    old = jc.CHUNK_CELLS
    try:
        jc.CHUNK_CELLS = 7 * 110
        assert np.array_equal(jc.jaccard_pairs_host(X, IJ), want)
    finally:
        jc.CHUNK_CELLS = old
    sp = pytest.importorskip("scipy.spatial.distance")
    sci = np.array([sp.jaccard(M[i], M[j]) for i, j in IJ])
    assert np.array_equal(sci, want)


def test_the_other_form_of_the_division_differs():
    """(u - i) / u is the definition; 1 - i / u is not the same number everywhere."""
    X = jc.fit_sets()
    IJ = jc.all_ordered_pairs(len(X))[::5]
    S = [jc.as_tokens(x) for x in X]
    common = np.array([np.intersect1d(S[i], S[j], assume_unique=True).size for i, j in IJ], dtype=np.float64)
    u = np.array([len(S[i]) + len(S[j]) for i, j in IJ], dtype=np.float64) - common
    T = jc.jaccard_pairs_host(X, IJ)
    assert np.array_equal((u - common) / u, T)
    assert np.any(1.0 - common / u != T)


def test_special_values():
    both = lambda a, b: (jc.jaccard_loop(a, b), jc.jaccard_pairs_host([a, b], [[0, 1]])[0], jc.jaccard_pairs_host([a, b], [[1, 0]])[0])
    e = np.zeros(0, dtype=np.int64)
    a = np.array([5, 9, -3, 2 ** 40], dtype=np.int64)
    assert both(e, e) == (0.0, 0.0, 0.0)
    assert both(e, a) == (1.0, 1.0, 1.0)
    assert both(a, e) == (1.0, 1.0, 1.0)
    assert both(a, a + 1) == (1.0, 1.0, 1.0)
    assert both(a, a.copy()) == (0.0, 0.0, 0.0)
    assert both(a, a[[2, 0, 3, 1]]) == (0.0, 0.0, 0.0)
    assert both(a, np.concatenate([a, a[[1, 1, 3]]])) == (0.0, 0.0, 0.0)
    assert both([1, 2, 3], [2, 3, 4]) == (0.5, 0.5, 0.5)
    assert both({1, 2, 3}, frozenset([3])) == (2.0 / 3.0,) * 3


def test_triangle_inequality():
    X = jc.fit_sets()
    nx = len(X)
    T = pc.sym_matrix(jc.jaccard_pairs_host, X)
    rng = np.random.default_rng(3)
    i, j, k = rng.integers(0, nx, (3, 5000))
    assert np.all(T[i, k] <= T[i, j] + T[j, k])
    assert T.min() == 0.0 and T.max() == 1.0


# ------------------------------------------------------------------------------------------------------------ packers
def test_pack_token_sets():
    from annchor_amd.distances import pack_token_sets

    X = [np.array([7, 3, 3, 9, 7], dtype=np.int32), [], {2 ** 62, -(2 ** 63), 3}, frozenset([9]), np.array([250, 3], dtype=np.uint8),
         (3, 7)]
    codes, offs, lens, U = pack_token_sets(X)
    universe = [-(2 ** 63), 3, 7, 9, 250, 2 ** 62]
    assert U == 6 and codes.dtype == np.int32 and offs.dtype == np.int64 and lens.dtype == np.int32
    assert lens.tolist() == [3, 0, 3, 1, 2, 2] and offs.tolist() == [0, 3, 3, 6, 7, 9]
    members = [codes[o:o + n].tolist() for o, n in zip(offs, lens)]
    assert members == [[1, 2, 3], [], [0, 1, 5], [3], [1, 4], [1, 2]]
    assert [[universe[c] for c in m] for m in members] == [sorted(set(map(int, x))) for x in X]
    # every member empty
    codes, offs, lens, U = pack_token_sets([[], set()])
    assert (codes.size, offs.tolist(), lens.tolist(), U) == (0, [0, 0], [0, 0], 0)


def test_pack_bitsets():
    from annchor_amd.distances import pack_bitsets, pack_token_sets

    for nbits in (1, 31, 32, 33, 97, 128, 129, 600):
        M = jc.fingerprints(9, nbits, 0.4, seed=nbits)
        M[0] = True
        M[1] = False
        words, nb = pack_bitsets(M)
        W = words.shape[1]
        assert nb == nbits and words.dtype == np.uint32 and W % 4 == 0 and W - 4 < -(-nbits // 32) <= W
        for p in range(W * 32):
            col = (words[:, p // 32] >> np.uint32(p % 32)) & np.uint32(1)
            assert np.array_equal(col.astype(bool), M[:, p] if p < nbits else np.zeros(9, dtype=bool)), (nbits, p)
    # a 2-D int array and the 2-D bool array of the same sets: the same codes, the same bit rows
    rng = np.random.default_rng(5)
    T = np.stack([rng.permutation(90)[:12] for _ in range(30)])
    T[:, 0] = np.arange(30) * 3    # (every token 0 .. 89 occurs, so a code is its token)
    T[:, 1] = np.arange(30) * 3 + 1
    T[:, 2] = np.arange(30) * 3 + 2
    T[4, 5] = T[4, 6]              # a repeat
    M = jc.indicator_matrix(list(T), 90)
    ct, ot, lt, Ut = pack_token_sets(T)
    cm, om, lm, Um = pack_token_sets(M)
    assert Ut == Um == 90
    assert np.array_equal(ct, cm) and np.array_equal(ot, om) and np.array_equal(lt, lm)
    wt, nt = pack_bitsets(T)
    wm, nm = pack_bitsets(M)
    assert nt == nm == 90 and np.array_equal(wt, wm)
    words, nb = pack_bitsets([[], []])
    assert nb == 1 and words.shape == (2, 4) and not words.any()


def test_refusals():
    from annchor_amd.distances import JACCARD_MAX_TOKENS, Jaccard, pack_bitsets, pack_token_sets

    assert JACCARD_MAX_TOKENS == jc.MAX_TOKENS
    ok = np.array([1, 2, 3])
    cases = [
        ([ok, np.array([1.0, 2.0])], "jaccard: set 1 has dtype float64"),
        ([ok, ok, np.array(["a", "b"], dtype=object)], "jaccard: set 2 has dtype object"),
        ([ok, [1.5, 2]], "jaccard: set 1 has dtype float64"),
        (np.zeros((3, 4)), "jaccard: set 0 has dtype float64"),
        ([ok, np.zeros((2, 2), dtype=np.int64)], "jaccard: set 1 has 2 dimensions"),
        ([np.zeros((2, 2), dtype=bool), np.zeros(4, dtype=bool)], "jaccard: set 0 has 2 dimensions"),
        ([ok, np.array([True, False])], "jaccard: set 1 is bool and set 0 is int64"),
        ([np.array([True, False]), ok, ok], "jaccard: set 1 is int64 and set 0 is bool"),
        ([np.zeros(8, dtype=bool), np.zeros(8, dtype=bool), np.zeros(9, dtype=bool)], "jaccard: set 2 has 9 bits, set 0 has 8"),
        ([ok, np.arange(65537)], "jaccard: set 1 has 65537 distinct tokens"),
        ([np.ones(65537, dtype=bool), np.zeros(65537, dtype=bool)], "jaccard: set 0 has 65537 distinct tokens"),
    ]
    for X, msg in cases:
        for pack in (pack_token_sets, pack_bitsets, Jaccard().form_for):
            with pytest.raises(ValueError, match=msg):
                pack(X)
    # 65536 distinct tokens are taken, and repeats do not count
    codes, offs, lens, U = pack_token_sets([np.concatenate([np.arange(65536), np.arange(100)]), ok])
    assert lens.tolist() == [65536, 3] and U == 65536
    with pytest.raises(ValueError, match="form must be"):
        Jaccard(form="dense")
    with pytest.raises(ValueError, match="form must be"):
        Jaccard(form=None)


def test_form_rule():
    """2048-bit fingerprints at 2.5 % and at 0.25 %: a factor of ten around the measured crossover, a mean size of U / 128."""
    from annchor_amd import distances as D

    assert (D.JACCARD_MAX_BITS, D.JACCARD_BITS_DENSITY) == (jc.MAX_BITS, 128)
    dense, sparse = jc.fingerprints(300, 2048, 0.025, seed=1), jc.fingerprints(300, 2048, 0.0025, seed=2)
    assert D.Jaccard().form_for(dense) == "bits"
    assert D.Jaccard().form_for(sparse) == "tokens"
    assert D.Jaccard("auto").form_for(dense) == "bits"
    assert D.Jaccard("tokens").form_for(dense) == "tokens"
    assert D.Jaccard("bits").form_for(sparse) == "bits"
    # the same sets as token lists: the same choice
    assert D.Jaccard().form_for([np.flatnonzero(r) for r in dense]) == "bits"
    # U = 8192 is taken, U = 8193 is not -- whatever the density
    full = np.ones((4, 8192), dtype=bool)
    assert D.Jaccard().form_for(full) == "bits" and D.Jaccard("bits").form_for(full) == "bits"
    over = np.ones((4, 8193), dtype=bool)
    assert D.Jaccard().form_for(over) == "tokens"
    with pytest.raises(ValueError, match="jaccard: form='bits' takes at most 8192 distinct tokens, this list has 8193"):
        D.Jaccard("bits").form_for(over)
    with pytest.raises(ValueError, match="8193"):
        D.Jaccard("bits").form_for([np.arange(8193), np.arange(5)])


def test_name_lookup():
    from annchor_amd import distances as D
    from annchor_amd.utils import get_function_from_input

    f = get_function_from_input("jaccard", None)
    assert f is D.jaccard and f.name == "jaccard" and f.ragged is True and f.form == "auto"
    g = get_function_from_input("jaccard", {"form": "tokens"})
    assert isinstance(g, D.Jaccard) and g.form == "tokens"
    with pytest.raises(ValueError, match="form must be"):
        get_function_from_input("jaccard", {"form": "sparse"})
    with pytest.raises(ValueError, match="form must be"):
        get_function_from_input("jaccard", {"form": None})
    assert get_function_from_input("jaccard", {}) is D.jaccard


# ------------------------------------------------------------------------------------------------ the GPU tests' data
def test_group_tables():
    """The sizes of the GPU tests' boundary data run the instantiation they are meant for."""
    assert jc.TOKEN_GROUPS == [(4, 64), (16, 1024), (64, 65536)]
    for G, limit in jc.TOKEN_GROUPS:
        assert jc.token_group(limit) == G and (limit == jc.MAX_TOKENS or jc.token_group(limit + 1) > G)
        assert set(jc.group_sizes(G)) <= set(jc.boundary_sizes())
    assert [jc.bits_group(b) for b in (1, 512, 513, 2048, 2049, 8192)] == [4, 4, 16, 16, 64, 64]


def test_data_sets():
    X = jc.brute_sets()
    assert len(X) == 200 and len({len(jc.as_tokens(x)) for x in X}) > 20
    P = jc.proto_sets(120, 6, 1500, 7)
    T = pc.sym_matrix(jc.jaccard_pairs_host, P)
    assert T.max() < 1.0


@pytest.mark.parametrize("name", ["fit_sets", "fit_protos", "query_rows", "query_lists"])
def test_fit_data_stays_inside_what_the_pipeline_takes(name):
    """A condition on the data, not a measurement: the CPU restatement of the pipeline completes a fit on each data set the GPU
    tests fit, and at most a third of fit_sets()'s pairs sit at exactly 1.0."""
    X = getattr(jc, name)()
    if name.startswith("query"):
        X = list(X[0]) + list(X[1])
    T = pc.sym_matrix(jc.jaccard_pairs_host, X)
    nx = 240
    ora = O.OracleAnnchor(nx, lambda IJ: T[IJ[:, 0], IJ[:, 1]], **jc.FIT_CFG).fit()
    assert 0 < ora.evals < nx * (nx - 1) // 2
    iu = np.triu_indices(nx, 1)
    ones = float(np.mean(T[:nx, :nx][iu] == 1.0))
    print("%s: %.3f of the pairs at exactly 1.0, %d evaluations" % (name, ones, ora.evals))
    if name == "fit_sets":
        assert ones <= 1.0 / 3.0
    if name == "fit_protos":
        assert ones == 0.0
    if name.startswith("query"):
        nq = len(X) - nx
        O.query(ora, lambda IJ: T[IJ[:, 0], IJ[:, 1] + nx], nq, nn=5, p_work=0.3)
