"""Weighted Levenshtein on the device (csrc/wed.hip) against the host recurrence of wed_cases.py: the tests it alone has.  Its
pair-source, brute-force, fit and query sections are test_seqdp_gpu.py's, which it shares with the sequence measures.

Tolerance: none.  Every cell is the min of three sums of fixed operands, min is exact and the additions are commutative, so
every evaluation order gives the same bits; each comparison of distances below is np.array_equal."""
import numpy as np
import pytest

import pool_cases as pc
import wed_cases as wc

pytestmark = pytest.mark.gpu

ref = pc.ref_cache()
NAME = "weighted_levenshtein"


def bound(X, costs):
    return pc.bound(NAME, X, **wc.kwargs_of(costs))


def device_pairs(X, IJ, costs):
    return pc.device_pairs(NAME, X, IJ, **wc.kwargs_of(costs))


# --------------------------------------------------------------------------------------------------- 1. small lengths
@pytest.mark.parametrize("kind", ["dyadic", "ragged"])
def test_small_lengths(kind):
    """One string of each length 0..96 over 5 symbols, all ordered pairs: n < m, n > m, n = m, the empty string against every
    length, every strip and group boundary of the 4-pairs-per-wavefront shape; then the list without its last 3 pairs (a last
    wavefront with one pair in it)."""
    costs = wc.dyadic(5) if kind == "dyadic" else wc.ragged_costs(5)
    X = wc.one_of_each_length(range(0, 97), 5, seed=41)
    IJ = wc.all_ordered_pairs(len(X))
    want = ref(("small", kind), lambda: wc.wed_pairs_host(X, IJ, costs))
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
    Up to 512 symbols all lengths are crossed; at the widest shape each length meets {0, 1, 32, 2048} in both orders (a
    rectangle: the full crossing's host reference is slow)."""
    Ls = wc.boundary_lengths(shape)
    R, G = wc.SHAPES[shape]
    assert max(Ls) == R * G and (shape == 0 or max(Ls[:-3]) <= wc.SHAPES[shape - 1][0] * wc.SHAPES[shape - 1][1])
    if shape < 2:
        IJ = wc.all_ordered_pairs(len(Ls))
    else:
        partners = [Ls.index(L) for L in (0, 1, 32, 2048)]
        IJ = np.array([p for k in range(len(Ls)) for q in partners for p in ((k, q), (q, k))], dtype=np.int64)
    return Ls, IJ


@pytest.mark.parametrize("shape", [0, 1, 2])
def test_boundary_lengths(shape):
    """{0, 1, 7, 8, 9, 16, 127, 128} on the (8, 16) shape, with {129, 511, 512} on the (8, 64) shape, with {32, 513, 2047, 2048} on
    the (32, 64) shape; non-dyadic costs, so that both prefix boundaries and every cell carry values of their own."""
    Ls, IJ = boundary_case(shape)
    assert {0, 1, 7, 8, 9, 16, 127, 128} <= set(Ls)
    assert shape < 1 or {129, 511, 512} <= set(Ls)
    assert shape < 2 or {32, 513, 2047, 2048} <= set(Ls)
    costs = wc.ragged_costs(5, seed=50)
    X = wc.one_of_each_length(Ls, 5, seed=50 + shape)
    want = ref(("boundary", shape), lambda: wc.wed_pairs_host(X, IJ, costs))
    assert np.all(np.isfinite(want))
    assert np.array_equal(device_pairs(X, IJ, costs), want)


# ------------------------------------------------------------------------------------------------ 3. alphabet extents
@pytest.mark.parametrize("A", [1, 2, 26, 127, 128])
def test_alphabet_extents(A):
    """40 strings of 1..40 symbols that use every symbol of the alphabet, all ordered pairs: code A-1 against code A-1 and code 0
    against code A-1 among them (the last entry of the table, the last entry of a row, the last indel cost).  A = 127 and 128:
    the table's stride is A, and its 127 KiB / 129 KiB take the large-LDS launch."""
    costs = wc.ragged_costs(A, seed=A)
    X = wc.using_every_symbol(A, seed=A)
    IJ = wc.all_ordered_pairs(len(X))
    want = ref(("alphabet", A), lambda: wc.wed_pairs_host(X, IJ, costs))
    got = device_pairs(X, IJ, costs)
    assert np.array_equal(got, want)
    last, first_last = wc.SYMBOLS[A - 1], wc.SYMBOLS[0] + wc.SYMBOLS[A - 1]
    assert X[0] == last and X[1] == first_last and got[0] == 0.0 and got[1] == wc.wed_loop(last, first_last, costs)
    assert A == 1 or got[1] == costs.g[0]


# ------------------------------------------------------------------- 4. unit costs equal the Levenshtein kernel
def test_unit_costs_equal_the_levenshtein_kernel():
    """200 of the bundled strings truncated to 300 symbols, 2000 random pairs: WeightedLevenshtein.unit == "levenshtein" on the
    device == the host.  The host value of all 2000 pairs is wed_pairs_host under unit costs (checked against both loops in
    test_wed_host.py); the plain integer Levenshtein loop, 90 000 cells per pair in Python, runs on 4 of them."""
    from annchor_amd import _native
    from annchor_amd.datasets import load_strings
    from annchor_amd.distances import WeightedLevenshtein

    X = [str(x)[:300] for x in load_strings()["X"][::8]]
    assert len(X) == 200 and max(map(len, X)) == 300
    alphabet = "".join(sorted(set("".join(X))))
    rng = np.random.default_rng(4)
    IJ = rng.integers(0, len(X), size=(2000, 2))
    unit = WeightedLevenshtein.unit(alphabet)
    assert unit.metric_violation() is None
    eng = _native.Engine(0)
    unit.bind(eng, X)
    got = eng.metric_pairs(IJ)
    eng.close()
    lev = pc.device_pairs("levenshtein", X, IJ)
    want = wc.wed_pairs_host(X, IJ, wc.Costs(alphabet, unit.substitution, unit.indel))
    assert got.dtype == np.float64 and np.array_equal(got, lev) and np.array_equal(got, want)
    assert np.array_equal(got[:4], [wc.levenshtein_loop(X[i], X[j]) for i, j in IJ[:4]])


# -------------------------------------------------------------------------------------- 5. two tables in one process
def test_two_tables_in_one_process():
    """Two engines on the same strings with different costs: each equals its own reference and the results differ.  Then the
    scratch engine of the loose-object calls, rebound from one table to another and back, and from 128 symbols to 5: the values
    are the bound table's every time."""
    X = wc.one_of_each_length([0, 3, 9, 20, 33, 47, 60, 130], 5, seed=6)
    IJ = wc.all_ordered_pairs(len(X))
    c1, c2 = wc.dyadic(5, seed=3), wc.ragged_costs(5, seed=4)
    w1, w2 = wc.wed_pairs_host(X, IJ, c1), wc.wed_pairs_host(X, IJ, c2)
    assert not np.array_equal(w1, w2)
    e1, e2 = bound(X, c1), bound(X, c2)
    g1, g2, g1b = e1.metric_pairs(IJ), e2.metric_pairs(IJ), e1.metric_pairs(IJ)
    e1.close()
    e2.close()
    assert np.array_equal(g1, w1) and np.array_equal(g2, w2) and np.array_equal(g1b, w1)
    m1, m2 = wc.metric_of(c1), wc.metric_of(c2)
    xs, ys = [X[i] for i in IJ[:, 0]], [X[j] for j in IJ[:, 1]]
    assert np.array_equal(m1.many(xs, ys), w1)
    assert np.array_equal(m2.many(xs, ys), w2)
    assert np.array_equal(m1.many(xs, ys), w1)
    c3 = wc.ragged_costs(128, seed=9)
    X3 = wc.using_every_symbol(128, seed=9)
    xs3, ys3 = X3[4:], X3[:-4]
    w3 = wc.wed_pairs_host(xs3 + ys3, np.stack([np.arange(36), np.arange(36) + 36], 1), c3)
    assert np.array_equal(wc.metric_of(c3).many(xs3, ys3), w3)
    assert np.array_equal(m2.many(xs, ys), w2)


# ---------------------------------------------------------------------------------------- 6. loose objects, refusals
def test_loose_objects():
    costs = wc.ragged_costs(26, seed=10)
    m = wc.metric_of(costs)
    d = m("kitten", "sitting")
    assert isinstance(d, float) and d == wc.wed_loop("kitten", "sitting", costs) == m("sitting", "kitten")
    assert m("", "") == 0.0 and m("abc", "") == wc.wed_loop("abc", "", costs) == m("", "abc")
    ys = ["", "kitchen", "mitten", "k", "sittingsittingsitting"]
    assert np.array_equal(m.one_to_many("kitten", ys), [wc.wed_loop("kitten", y, costs) for y in ys])
    assert np.array_equal(m.many(ys, ys[::-1]), [wc.wed_loop(x, y, costs) for x, y in zip(ys, ys[::-1])])


def test_refusals():
    from annchor_amd import BruteForce, _native

    kw = wc.kwargs_of(wc.dyadic(3))
    with pytest.raises(ValueError, match="weighted_levenshtein: string 1 holds the symbol 'x', which is not in the alphabet"):
        BruteForce(["abc", "abx", "a"], NAME, func_kwargs=kw)
    with pytest.raises(ValueError, match="weighted_levenshtein: string 2 has 2049 symbols; at most 2048"):
        BruteForce(["abc", "", "a" * 2049], NAME, func_kwargs=kw)
    with pytest.raises(ValueError, match="weighted_levenshtein: string 0 is a bytes, not a str"):
        BruteForce([b"abc", "ab"], NAME, func_kwargs=kw)
    with pytest.raises(ValueError, match=r"weighted_levenshtein: substitution\[0\]\[1\] = 1.0 but substitution\[1\]\[0\] = 2.0"):
        BruteForce(["a", "b"], NAME, func_kwargs={"alphabet": "ab", "substitution": [[0, 1], [2, 0]]})
    with pytest.raises(AssertionError, match="requires alphabet and substitution"):
        BruteForce(["a", "b"], NAME)
    # the library's own checks, behind the host's; a refusal leaves the engine as it was
    S, g = 1.0 - np.eye(3), np.ones(3)
    codes, offs, lens = np.array([0, 1, 2, 2, 1], dtype=np.uint8), np.array([0, 3]), np.array([3, 2])
    want = [2.0, 0.0]
    eng = _native.Engine(0)
    try:
        eng.set_coded_strings(codes, offs, lens, S, g)
        assert eng.metric_pairs(np.array([[0, 1], [1, 1]])).tolist() == want
        bad = codes.copy()
        bad[4] = 3
        with pytest.raises(_native.NativeError, match=r"error -1: string 1 holds code 3: the alphabet has 3 symbols"):
            eng.set_coded_strings(bad, offs, lens, S, g)
        long = np.zeros(2049 + 2, dtype=np.uint8)
        with pytest.raises(_native.NativeError, match=r"error -4: string 0 has 2049 symbols: weighted_levenshtein supports 0\.\.2048"):
            eng.set_coded_strings(long, np.array([0, 2049]), np.array([2049, 2]), S, g)
        with pytest.raises(_native.NativeError, match=r"error -1: string 1 has a negative length"):
            eng.set_coded_strings(codes, offs, np.array([3, -1]), S, g)
        with pytest.raises(_native.NativeError, match=r"error -4: alphabet=129"):
            eng.set_coded_strings(codes, offs, lens, 1.0 - np.eye(129), np.ones(129))
        for table, match in ((S + np.eye(3), r"substitution\[0\]\[0\] is not 0"),
                             (S - 2 * np.eye(3)[[1, 0, 2]], r"substitution\[0\]\[1\] is not a finite cost"),
                             (np.where(np.eye(3)[[1, 0, 2]] > 0, np.nan, S), r"substitution\[0\]\[1\] is not a finite cost"),
                             (S + np.triu(np.full((3, 3), 2.0 ** -52), 1), r"substitution\[0\]\[1\] != substitution\[1\]\[0\]")):
            with pytest.raises(_native.NativeError, match="error -1: weighted_levenshtein: " + match):
                eng.set_coded_strings(codes, offs, lens, table, g)
        for indel in (np.array([1.0, -1.0, 1.0]), np.array([1.0, np.inf, 1.0])):
            with pytest.raises(_native.NativeError, match=r"error -1: weighted_levenshtein: indel\[1\] is not a finite cost"):
                eng.set_coded_strings(codes, offs, lens, S, indel)
        assert eng.metric_pairs(np.array([[0, 1], [1, 1]])).tolist() == want
    finally:
        eng.close()
