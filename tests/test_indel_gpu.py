"""The indel (LCS) kernels (csrc/indel.hip: k_indel_f<1>, k_indel_f<2>, k_indel_w) against the two-row loop of indel_cases.py,
through every layer.  Tolerance: none.  The distance is an integer; every comparison is np.array_equal or ==."""
import numpy as np
import pytest

import exact_knn_cases as KC
import indel_cases as ic
import osa_cases as oc
import pool_cases as pc
import radius_cases as RC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("lengths, A", [(s, A) for s in (0, 1) for A in (2, 3, 600)])
def test_lengths_through_the_three_pair_forms(lengths, A):
    """One string of each length where the lane layout changes, the empty one first and last, over 2 and 3 symbols (dense matches:
    a carry in nearly every column); the second list reaches 2048 symbols (two words per lane).  A = 600: 16-bit codes, every one
    present, and a pair that differs in one symbol whose codes, 300 and 556, share their low byte.  All ordered pairs as explicit
    pairs (and without the last 3: another last wavefront), one-to-all (the anchors' columns) and positions into a built pair
    list."""
    from annchor_amd import _native

    sym = [chr(0x400 + k) for k in range(A)]
    X = ic.random_strings(ic.LENGTHS[lengths], sym, seed=10 * lengths + A)
    if A > 256:
        X[1:1] = ["".join(sym[:300]), "".join(sym[300:]), X[5] + sym[300], X[5] + sym[556]]
    assert max(map(len, X)) == (1024, 2048)[lengths] and X[0] == X[-1] == ""
    M, nx, IJ, anchors = ic.indel_matrix(X), len(X), pc.all_ordered_pairs(len(X)), [0, len(X) - 2, 1]
    assert A <= 256 or M[3, 4] == 2
    eng = pc.bound(ic.NAME, X)
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


@pytest.mark.parametrize("limit", [64, 1024, 2048])
def test_the_carry_chain_at_its_longest(limit):
    """Known answers, no loop.  "a" * m against "a" * n = |m - n|: every column carries through every lane boundary of the pattern.
    "b" * m against "a" * n = m + n: no carry anywhere.  One common symbol at row 31, 32, 1023 or 1024 of an otherwise disjoint
    pair = m + n - 2.  limit: the data set's longest string, so the slot width (2, 32 and 32 lanes) and the words per lane
    (1, 1 and 2)."""
    ms, ns = [m for m in (32, 33, 64, 1024, 2048) if m <= limit], [n for n in (1, 31, 32, 33, 2048) if n <= limit]
    rows = [r for r in (31, 32, 1023, 1024) if r < limit]
    X = ["a" * n for n in ns] + ["a" * m for m in ms] + ["b" * m for m in ms] + ["b" * r + "c" + "b" * (limit - r - 1) for r in rows]
    X.append("a" * 5 + "c" + "a" * 7)
    na, nm = len(ns), len(ms)
    IJ = [(na + i, j, abs(m - n)) for i, m in enumerate(ms) for j, n in enumerate(ns)]
    IJ += [(na + nm + i, j, m + n) for i, m in enumerate(ms) for j, n in enumerate(ns)]
    IJ += [(na + 2 * nm + i, len(X) - 1, limit + 13 - 2) for i in range(len(rows))]
    IJ = np.array(IJ, dtype=np.int64)
    eng = pc.bound(ic.NAME, X)
    try:
        assert np.array_equal(eng.metric_pairs(IJ[:, :2]), IJ[:, 2]) and np.array_equal(eng.metric_pairs(IJ[:, 1::-1]), IJ[:, 2])
    finally:
        eng.close()


def test_known_answers_and_loose_objects():
    from annchor_amd.distances import indel as f

    known = [("kitten", "sitting", 5), ("lewenstein", "levenshtein", 3), ("ab", "ba", 2), ("ca", "abc", 3), ("abc", "", 3), ("", "", 0)]
    xs, ys, want = [p[0] for p in known], [p[1] for p in known], [p[2] for p in known]
    assert [ic.indel_loop(x, y) for x, y in zip(xs, ys)] == want
    assert f.many(xs, ys).tolist() == want and f.many(ys, xs).tolist() == want
    assert f.one_to_many("ca", ys).tolist() == [ic.indel_loop("ca", y) for y in ys]
    assert isinstance(f("kitten", "sitting"), int) and f("kitten", "sitting") == 5 and f("sitting", "kitten") == 5


def test_through_the_public_interface(capsys):
    """160 strings of 20 .. 45 symbols over 12 symbols in 6 families; integer distances with many ties, so the graphs are defined by
    (distance, index).  Against "levenshtein" on the device: lev <= indel <= 2 lev, and indel has the parity of |x| + |y|."""
    from annchor_amd import Annchor, BruteForce

    X, k = oc.mutated_strings(160, 20, 45, 12, seed=5), 10
    M = ic.indel_matrix(X)
    want = KC.truth(M, k)
    bf = BruteForce(X, ic.NAME).fit(k)
    assert np.array_equal(bf.neighbor_graph[1], want[1])
    capsys.readouterr()
    ann = Annchor(X, ic.NAME, n_anchors=8, n_neighbors=k, n_samples=700, p_work=0.3, niters=2, is_metric=True)
    assert "triangle inequality" not in capsys.readouterr().err
    assert KC.same_graph(ann.exact_neighbor_graph(), bf.neighbor_graph) and KC.same_graph(bf.neighbor_graph, want)
    r = float(np.percentile(M[np.triu_indices(len(X), k=1)], 5))
    g = ann.radius_graph(r)
    assert RC.same_graph((g.indptr, g.indices, g.distances), RC.graph_from_matrix(M, r)) and len(g.indices) > len(X)
    IJ, lens = pc.all_ordered_pairs(len(X)), np.array([len(x) for x in X])
    L, D = pc.device_pairs("levenshtein", X, IJ), M[IJ[:, 0], IJ[:, 1]]
    assert np.all(L <= D) and np.all(D <= 2 * L) and np.array_equal(D % 2, (lens[IJ[:, 0]] + lens[IJ[:, 1]]) % 2)


def test_refusals():
    from annchor_amd import BruteForce, _native

    with pytest.raises(ValueError, match="indel: string 2 has 2049 symbols; at most 2048"):
        BruteForce(["abc", "", "a" * (ic.LIMIT + 1)], ic.NAME)
    with pytest.raises(ValueError, match="indel: string 1 is a bytes, not a str"):
        BruteForce(["abc", b"abc"], ic.NAME)
    # the library's own checks, behind the host's; after each refusal the data set bound before still answers
    codes, offs, lens = np.array([0, 1, 2, 0, 2, 1], dtype=np.uint16), np.array([0, 3]), np.array([3, 3])
    IJ, want, long = np.array([[0, 1], [1, 0], [1, 1]]), [2.0, 2.0, 0.0], np.zeros(ic.LIMIT + 3, dtype=np.uint16)   # "abc" / "acb"
    eng = _native.Engine(0)
    try:
        eng.set_strings_indel(codes, offs, lens, 3)
        for message, args in ((r"-4: string 0 has 2049 symbols: indel supports 0\.\.2048",
                               (long, np.array([0, ic.LIMIT + 1]), np.array([ic.LIMIT + 1, 2]), 3)),
                              (r"-1: string 0 holds code 2: the alphabet has 2 symbols", (codes, offs, lens, 2)),
                              (r"-4: alphabet=65536: indel supports 1\.\.65535 symbols", (codes, offs, lens, 65536))):
            with pytest.raises(_native.NativeError, match="error " + message):
                eng.set_strings_indel(*args)
            assert eng.metric_pairs(IJ).tolist() == want
        long[ic.LIMIT:] = 1   # the limit itself is taken: 2048 x "a" against "bb"
        eng.set_strings_indel(long[:ic.LIMIT + 2], np.array([0, ic.LIMIT]), np.array([ic.LIMIT, 2]), 2)
        assert eng.metric_pairs(np.array([[0, 1]])).tolist() == [float(ic.LIMIT + 2)] and eng.metric == _native.METRIC_INDEL == 31
    finally:
        eng.close()
