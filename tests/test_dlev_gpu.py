"""The Damerau-Levenshtein kernel (csrc/dlev.hip, k_dlev) against the full-matrix loop of dlev_cases.py, through every layer.
Tolerance: none.  The distance is an integer; every comparison is np.array_equal or ==."""
import numpy as np
import pytest

import dlev_cases as dc
import exact_knn_cases as KC
import osa_cases as oc
import pool_cases as pc
import radius_cases as RC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape, A", [(s, A) for s in (0, 1, 2) for A in (2, 3)] + [(1, 600)])
def test_lengths_through_the_three_pair_forms(shape, A):
    """One string of each length where the lane layout changes, the empty one first and last, over 2 and 3 symbols (K, L, F and T
    change in nearly every cell); on the widest shape ONE pair is full x full length.  A = 600: 16-bit codes, every one present,
    and a pair that differs in one symbol whose codes, 300 and 556, share their low byte.  All ordered pairs as explicit pairs (and
    without the last 3: another last wavefront), one-to-all (the anchors' columns) and positions into a built pair list."""
    from annchor_amd import _native

    sym = [chr(0x400 + k) for k in range(A)]
    X = dc.random_strings(dc.lane_lengths(shape), sym, seed=10 * shape + A)
    if A > 256:
        X[1:1] = ["".join(sym[:300]), "".join(sym[300:]), X[5] + sym[300], X[5] + sym[556]]
    assert max(map(len, X)) == np.prod(dc.SHAPES[shape]) and X[0] == X[-1] == ""
    M, nx, IJ, anchors = dc.dl_matrix(X), len(X), pc.all_ordered_pairs(len(X)), [0, len(X) - 2, 1]
    assert A <= 256 or M[3, 4] == 1
    eng = pc.bound(dc.NAME, X)
    try:
        assert np.array_equal(eng.metric_pairs(IJ), M[IJ[:, 0], IJ[:, 1]])
        assert np.array_equal(eng.metric_pairs(IJ[:-3]), M[IJ[:-3, 0], IJ[:-3, 1]])
        eng.pick_anchors_selected(anchors)
        assert np.array_equal(eng.download(_native.F_D).reshape(nx, len(anchors)), M[:, anchors])
        n, _ = eng.build_locality(len(anchors), 1, nx - 1)
        eng.compute_features()
        listed = eng.download(_native.F_IJS).reshape(-1, 2)
        assert n == len(listed) >= nx - 1
        assert np.array_equal(eng.evaluate_samples(np.arange(n, dtype=np.int64)), M[listed[:, 0], listed[:, 1]])
    finally:
        eng.close()


@pytest.mark.parametrize("inside", ["", "b"])
@pytest.mark.parametrize("shape", [0, 1, 2])
def test_a_swap_at_every_position(shape, inside):
    """Known answers; no two adjacent symbols of the base are equal, the longer string has G R symbols.  inside = "": (p, p+1)
    swapped, 1 for every p -- case (a) / (b) on every lane's rows 0 and 1, on columns 0 and 1, on lane 0's row 0.  inside = "b", not
    in the base: u c a v against u a b c v, |u| = p, a swap with an insertion (the other order: a deletion) inside it -- 2, where
    optimal string alignment gives 3: a far-back read across every lane boundary."""
    steps = np.random.default_rng(shape).integers(1, 3, size=int(np.prod(dc.SHAPES[shape])) - len(inside))
    base = "".join("acd"[c] for c in np.cumsum(steps) % 3)
    X = [base] + [base[:p] + base[p + 1] + inside + base[p] + base[p + 2:] for p in range(len(base) - 1)]
    want = 1.0 + len(inside)
    assert dc.dl_loop(base[:9], X[4][:9 + len(inside)]) == want
    IJ = np.stack([np.zeros(len(X) - 1, dtype=np.int64), np.arange(1, len(X))], axis=1)
    eng = pc.bound(dc.NAME, X)
    try:
        assert np.all(eng.metric_pairs(IJ) == want) and np.all(eng.metric_pairs(IJ[:, ::-1]) == want)
    finally:
        eng.close()


def test_known_answers_and_loose_objects():
    from annchor_amd.distances import damerau_levenshtein as m

    known = [("ca", "abc", 2), ("ab", "ba", 1), ("abcd", "acbd", 1), ("abcdef", "badcfe", 3), ("abc", "", 3), ("", "", 0), ("aa", "aa", 0)]
    xs, ys, want = [p[0] for p in known], [p[1] for p in known], [p[2] for p in known]
    assert [dc.dl_loop(x, y) for x, y in zip(xs, ys)] == want
    assert m.many(xs, ys).tolist() == want and m.many(ys, xs).tolist() == want
    assert m.one_to_many("ca", ys).tolist() == [dc.dl_loop("ca", y) for y in ys]
    assert isinstance(m("ca", "abc"), int) and m("ca", "abc") == 2


def test_through_the_public_interface(capsys):
    """160 strings of 20 .. 45 symbols over 12 symbols in 6 families mutated by adjacent swaps as well as edits (160 and 45: the
    dense host matrix is the test's time); integer distances with many ties, so the graphs are defined by (distance, index)."""
    from annchor_amd import Annchor, BruteForce

    X, k = oc.mutated_strings(160, 20, 45, 12, seed=5), 10
    M = dc.dl_matrix(X)
    want = KC.truth(M, k)
    assert min(len(np.unique(row)) for row in want[1]) < k   # ties inside the lists
    bf = BruteForce(X, dc.NAME).fit(k)
    assert np.array_equal(bf.neighbor_graph[1], want[1])
    capsys.readouterr()
    ann = Annchor(X, dc.NAME, n_anchors=8, n_neighbors=k, n_samples=700, p_work=0.3, niters=2, is_metric=True)
    assert "triangle inequality" not in capsys.readouterr().err
    assert KC.same_graph(ann.exact_neighbor_graph(), bf.neighbor_graph) and KC.same_graph(bf.neighbor_graph, want)
    r = float(np.percentile(M[np.triu_indices(len(X), k=1)], 5))
    g = ann.radius_graph(r)
    assert RC.same_graph((g.indptr, g.indices, g.distances), RC.graph_from_matrix(M, r)) and len(g.indices) > len(X)


def test_refusals():
    from annchor_amd import BruteForce, _native

    with pytest.raises(ValueError, match="damerau_levenshtein: string 2 has 2049 symbols; at most 2048"):
        BruteForce(["abc", "", "a" * (dc.LIMIT + 1)], dc.NAME)
    with pytest.raises(ValueError, match="damerau_levenshtein: string 1 is a bytes, not a str"):
        BruteForce(["abc", b"abc"], dc.NAME)
    # the library's own checks, behind the host's; after each refusal the data set bound before still answers
    codes, offs, lens = np.array([0, 1, 2, 0, 2, 1], dtype=np.uint16), np.array([0, 3]), np.array([3, 3])
    IJ, want, long = np.array([[0, 1], [1, 0], [1, 1]]), [1.0, 1.0, 0.0], np.zeros(dc.LIMIT + 3, dtype=np.uint16)   # "abc" / "acb": one swap
    eng = _native.Engine(0)
    try:
        eng.set_strings_dlev(codes, offs, lens, 3)
        for message, args in ((r"-4: string 0 has 2049 symbols: damerau_levenshtein supports 0\.\.2048",
                               (long, np.array([0, dc.LIMIT + 1]), np.array([dc.LIMIT + 1, 2]), 3)),
                              (r"-1: string 0 holds code 2: the alphabet has 2 symbols", (codes, offs, lens, 2))):
            with pytest.raises(_native.NativeError, match="error " + message):
                eng.set_strings_dlev(*args)
            assert eng.metric_pairs(IJ).tolist() == want
        long[dc.LIMIT:] = 1   # the limit itself is taken: 2048 x "a" against "bb"
        eng.set_strings_dlev(long[:dc.LIMIT + 2], np.array([0, dc.LIMIT]), np.array([dc.LIMIT, 2]), 2)
        assert eng.metric_pairs(np.array([[0, 1]])).tolist() == [float(dc.LIMIT)] and eng.metric == _native.METRIC_DAMERAU_LEVENSHTEIN == 30
    finally:
        eng.close()
