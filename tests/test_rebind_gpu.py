"""A metric bound second (or third) on an engine gives the values it gives bound first.  The scalars a binding leaves in the context
(csrc/common.h: BoundState) are shared between metrics and route the launches; csrc/bind.hip gives all of them their defaults back
at every commit.  Each sequence below crosses one of them.  Tolerance: none -- the same kernels on the same uploaded bytes, so
every comparison is np.array_equal against a fresh engine.  Also here: a refused bind leaves the binding before it answering, and
the two Levenshtein loaders refuse a negative offset."""
import numpy as np
import pytest

import pool_cases as pc

pytestmark = pytest.mark.gpu

LATIN = "abcdefghijkl"
WIDE_SYMBOLS = [chr(0x400 + k) for k in range(300)]


def strings(n, lo, hi, symbols, seed):
    rng = np.random.default_rng(seed)
    return ["".join(symbols[k] for k in rng.integers(0, len(symbols), rng.integers(lo, hi + 1))) for _ in range(n)]


def wide_strings(seed):
    """8 strings of <= 40 symbols with more than 256 distinct symbols among them (encode_strings then takes 16-bit codes): seven
    disjoint runs of 40 and one that takes a symbol of each run in turn"""
    rng = np.random.default_rng(seed)
    sym = [WIDE_SYMBOLS[k] for k in rng.permutation(len(WIDE_SYMBOLS))]
    X = ["".join(sym[40 * i:40 * i + 40]) for i in range(7)]
    X.append("".join(sym[(40 * i + i // 7) % 280] for i in range(40)))
    assert len(set("".join(X))) > 256 and max(map(len, X)) == 40
    return X


def slot_class_strings():
    """a dozen strings, the longest of 70 symbols, the others of at most 32: the Levenshtein loader finds a short slot class"""
    return strings(11, 0, 32, LATIN, seed=1) + ["".join(LATIN[(3 * k + k // 5) % 12] for k in range(70))]


def series(n, dim, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=(int(rng.integers(3, 41)), dim)).astype(dtype) for _ in range(n)]


def sets(seed):
    rng = np.random.default_rng(seed)
    return [np.unique(rng.integers(0, 60, rng.integers(0, 30))) for _ in range(8)]


def metrics():
    from annchor_amd import distances as D

    S = np.abs(np.subtract.outer(np.arange(12.0), np.arange(12.0))) * 0.25
    S = np.minimum(S, 1.5)
    g = 1.0 + 0.125 * (np.arange(12) % 3)
    cost = np.abs(np.subtract.outer(np.arange(6.0), np.arange(6.0)))
    return {
        "lev": D.levenshtein, "dlev": D.damerau_levenshtein, "indel": D.indel,
        "wed": D.WeightedLevenshtein(LATIN, S, g), "affine": D.AffineGap(LATIN, S, g, open=0.75), "osa": D.OSA(LATIN, S, g, transpose=0.5),
        "edr_norm": D.EDR(0.5, normalize=True), "edr": D.EDR(0.5), "lcss": D.LCSS(0.5), "lcss_delta": D.LCSS(0.5, delta=2),
        "dtw": D.DTW(), "dtw_window": D.DTW(window=3), "dtw_wide": D.DTW(wide=True), "frechet": D.frechet,
        "hausdorff": D.hausdorff, "hausdorff_wide": D.Hausdorff(wide=True),
        "jaccard_bits": D.Jaccard(form="bits"), "jaccard_tokens": D.Jaccard(form="tokens"),
        "wasserstein": D.Wasserstein(cost), "euclidean": D.euclidean,
    }


def data():
    rng = np.random.default_rng(7)
    return {
        "slots": slot_class_strings(), "latin_a": strings(8, 0, 40, LATIN, seed=2), "latin_b": strings(7, 1, 40, LATIN, seed=3),
        "wide_a": wide_strings(4), "wide_b": wide_strings(5),
        "s1": series(8, 1, 11), "s1b": series(7, 1, 12), "s2": series(8, 2, 13), "s2b": series(6, 2, 14), "s5": series(7, 5, 15),
        "s6": series(7, 6, 16),
        "sets_a": sets(21), "sets_b": sets(22),
        "hist": rng.integers(1, 9, size=(8, 6)).astype(np.float64), "points": rng.normal(size=(7, 5)).astype(np.float32),
    }


# (metric, data set) after (metric, data set): every step from the second on is compared
SEQUENCES = {
    "lev slot classes, indel, lev": [("lev", "slots"), ("indel", "latin_a"), ("lev", "latin_b")],
    "lev u16, weighted": [("lev", "wide_a"), ("wed", "latin_a")],
    "lev u16, dlev, lev": [("lev", "wide_a"), ("dlev", "latin_a"), ("lev", "latin_b")],
    "indel u16, indel bytes": [("indel", "wide_b"), ("indel", "latin_a")],
    "edr normalized, lcss": [("edr_norm", "s2"), ("lcss", "s2b")],
    "lcss delta, edr": [("lcss_delta", "s2"), ("edr", "s2b")],
    "lcss delta, dtw": [("lcss_delta", "s2"), ("dtw", "s2b")],
    "dtw window, frechet": [("dtw_window", "s2"), ("frechet", "s2b")],
    "hausdorff wide, hausdorff": [("hausdorff_wide", "s6"), ("hausdorff", "s2")],
    "dtw wide, dtw": [("dtw_wide", "s5"), ("dtw", "s1")],
    "affine open, weighted": [("affine", "latin_a"), ("wed", "latin_b")],
    "osa transpose, weighted": [("osa", "latin_a"), ("wed", "latin_b")],
    "jaccard bits, tokens": [("jaccard_bits", "sets_a"), ("jaccard_tokens", "sets_b")],
    "wasserstein, euclidean": [("wasserstein", "hist"), ("euclidean", "points")],
}

_ref = pc.ref_cache()


def fresh(step, M, X):
    """all ordered pairs of a step's data set on an engine of its own"""
    def build():
        from annchor_amd import _native

        eng = _native.Engine(0)
        try:
            M[step[0]].bind(eng, X[step[1]])
            return eng.metric_pairs(pc.all_ordered_pairs(len(X[step[1]])))
        finally:
            eng.close()

    return _ref(step, build)


def test_the_slot_classes_exist():
    """(what the first sequence relies on: 64 / (64 / W + 1) >= 1 words for W = 3 words of the longest string)"""
    lens = [len(x) for x in slot_class_strings()]
    assert max(lens) >= 70 and sorted(lens)[-2] <= 32 and 64 // (64 // ((max(lens) + 31) // 32) + 1) >= 1


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_bound_second_equals_bound_first(name):
    from annchor_amd import _native

    M, X = metrics(), data()
    eng = _native.Engine(0)
    try:
        for k, step in enumerate(SEQUENCES[name]):
            M[step[0]].bind(eng, X[step[1]])
            if k == 0:
                continue
            got = eng.metric_pairs(pc.all_ordered_pairs(len(X[step[1]])))
            assert np.array_equal(got, fresh(step, M, X)), "%s: step %d (%s on %s)" % (name, k, *step)
    finally:
        eng.close()


def test_a_refused_bind_leaves_the_binding_before_it():
    from annchor_amd import _native

    M, X = metrics(), data()
    eng = _native.Engine(0)
    try:
        # a float pool with a member over its limit (2048 values for dtw at dim 1)
        step = ("dtw_window", "s1")
        M[step[0]].bind(eng, X[step[1]])
        values, lens = np.zeros(2049 + 5), np.array([2049, 5], dtype=np.int32)
        with pytest.raises(_native.NativeError, match="series 0 has 2049 values"):
            eng.set_series(values, np.array([0, 2049], dtype=np.int64), lens)
        assert np.array_equal(eng.metric_pairs(pc.all_ordered_pairs(len(X[step[1]]))), fresh(step, M, X))
        # a byte string with a code >= alphabet
        step = ("lev", "slots")
        M[step[0]].bind(eng, X[step[1]])
        with pytest.raises(_native.NativeError, match="symbol code out of range in string 1"):
            eng.set_strings(np.array([0, 1, 2, 5, 1], dtype=np.uint8), np.array([0, 3], dtype=np.int64), np.array([3, 2], dtype=np.int32), 3)
        assert np.array_equal(eng.metric_pairs(pc.all_ordered_pairs(len(X[step[1]]))), fresh(step, M, X))
    finally:
        eng.close()


@pytest.mark.parametrize("entry, dtype", [("annchor_set_strings", np.uint8), ("annchor_set_strings_u16", np.uint16)])
def test_the_levenshtein_loaders_refuse_a_negative_offset(entry, dtype):
    from annchor_amd import _native

    M, X = metrics(), data()
    step = ("lev", "latin_a")
    eng = _native.Engine(0)
    try:
        M[step[0]].bind(eng, X[step[1]])
        codes = np.array([0, 1, 2, 1, 0, 2], dtype=dtype)
        offs, lens = np.array([0, -1, 4], dtype=np.int64), np.array([2, 1, 2], dtype=np.int32)
        with pytest.raises(_native.NativeError, match="negative offset at 1"):
            eng._chk(getattr(eng.lib, entry)(eng.h, _native._ptr(codes), _native._ptr(offs), _native._ptr(lens), 3, 3))
        assert np.array_equal(eng.metric_pairs(pc.all_ordered_pairs(len(X[step[1]]))), fresh(step, M, X))
    finally:
        eng.close()
