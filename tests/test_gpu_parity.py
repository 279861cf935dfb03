"""
GPU parity tests (run on the MI355X box with `-m gpu`): the HIP path, called through
the C-ABI, against the CPU oracle on the same seeded inputs and against the golden
fixtures.  Integer / index work is compared bit-exactly; float work within the
tolerance written next to each assert.
"""
import os

import numpy as np
import pytest

from oracle import annchor_oracle as O
from oracle import metrics as om

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def strings():
    return om.load_strings()[0]


# ------------------------------------------------------------------ metric: a2/a3
def test_levenshtein_known_answers():
    """reference tests/test_distances.py:9-12."""
    from annchor_amd.distances import levenshtein

    assert levenshtein("cat", "cart") == 1
    assert levenshtein("cat", "cap") == 1
    assert levenshtein("cat", "at") == 1
    assert levenshtein("123456789", "92346781") == 3


def test_levenshtein_edge_cases():
    from annchor_amd.distances import levenshtein

    xs = ["", "", "a", "abc", "a" * 31, "a" * 32, "a" * 33, "ab" * 40, "x" * 64, "kitten", "flaw", "z" * 100]
    ys = ["", "abc", "", "abc", "a" * 32, "b" * 32, "a" * 65, "ba" * 40, "y" * 64, "sitting", "lawn", "z" * 99 + "y"]
    got = levenshtein.many(xs, ys)
    want = [om.levenshtein(x, y, "dp") for x, y in zip(xs, ys)]
    assert list(got) == want


def test_levenshtein_pairs_vs_oracle(strings):
    from annchor_amd import _native
    from annchor_amd.distances import levenshtein

    eng = _native.Engine(0)
    levenshtein.bind(eng, strings)
    rng = np.random.default_rng(0)
    IJ = rng.integers(0, len(strings), (20000, 2))
    IJ[:50, 1] = IJ[:50, 0]  # i == j
    IJ[50:100] = IJ[100:150]  # repeats
    got = eng.metric_pairs(IJ)
    want = om.PackedStrings(strings).pairs(IJ)
    assert np.array_equal(got, want)
    assert got[0] == 0
    # reference tests/test_datasets.py:234-235
    assert eng.metric_pairs(np.array([[10, 165]]))[0] == 299


def test_levenshtein_random_ragged():
    from annchor_amd.distances import levenshtein

    rng = np.random.default_rng(1)
    xs, ys = [], []
    for _ in range(600):
        la, lb = rng.integers(0, 300, 2)
        a = "".join(rng.choice(list("abcd"), la))
        b = list(a)
        for _ in range(rng.integers(0, 20)):  # mutate so that distances are non-trivial
            if b and rng.random() < 0.5:
                b.pop(rng.integers(0, len(b)))
            else:
                b.insert(rng.integers(0, len(b) + 1), rng.choice(list("abcd")))
        xs.append(a)
        ys.append("".join(b) if rng.random() < 0.7 else "".join(rng.choice(list("abcd"), lb)))
    got = levenshtein.many(xs, ys)
    want = [om.levenshtein(x, y, "dp") for x, y in zip(xs, ys)]
    assert list(got) == want


def test_levenshtein_slot_classes():
    """k_lev_f's two slot classes (lists of >= 4096 pairs): longest string 594 symbols = 19 words -> 3 pairs
    per wave, 4 for pairs whose shorter string has <= 16 words.  Lengths straddle the 512-symbol class
    boundary; pairs of two long strings, two short ones, mixed, equal and empty strings."""
    from annchor_amd import _native
    from annchor_amd.distances import levenshtein

    rng = np.random.default_rng(11)
    lens = [0, 1, 31, 32, 33, 480, 509, 510, 511, 512, 513, 514, 543, 544, 545, 560, 593, 594]
    X = ["".join(rng.choice(list("acgt"), n)) for n in lens for _ in range(6)]
    eng = _native.Engine(0)
    levenshtein.bind(eng, X)
    for npairs in (4096, 9001):
        IJ = rng.integers(0, len(X), (npairs, 2))
        IJ[:100, 1] = IJ[:100, 0]
        assert np.array_equal(eng.metric_pairs(IJ), om.PackedStrings(X).pairs(IJ))
    # all pairs long (empty short class) and all pairs short (empty long class)
    long_ids = np.array([i for i, x in enumerate(X) if len(x) > 512])
    short_ids = np.array([i for i, x in enumerate(X) if len(x) <= 512])
    for ids in (long_ids, short_ids):
        IJ = ids[rng.integers(0, len(ids), (5000, 2))]
        assert np.array_equal(eng.metric_pairs(IJ), om.PackedStrings(X).pairs(IJ))


@pytest.mark.parametrize("variant", ["1", "9"])
def test_levenshtein_kernel_variants_ragged(variant, monkeypatch):
    """Both pair-list Levenshtein kernels (k_lev_r<1>, the kernel of strings beyond 1024 symbols, forced here = 1; k_lev_f, the
    default = 9) against the oracle on ragged input: empty strings, lengths
    around the 32-symbol word boundaries, one very long string (sets the slot width), equal
    strings, a 60-symbol alphabet."""
    from annchor_amd import _native
    from annchor_amd.distances import levenshtein

    monkeypatch.setenv("ANNCHOR_LEV_R", variant)
    rng = np.random.default_rng(7)
    alphabet = [chr(c) for c in range(60, 120)]
    lens = list(range(0, 70)) + [95, 96, 97, 127, 128, 129, 255, 256, 257, 300, 511, 512, 513, 640, 1000]
    X = ["".join(rng.choice(alphabet[: rng.integers(2, 60)], n)) for n in lens for _ in range(3)]
    X += [X[5], X[100], "", ""]
    eng = _native.Engine(0)
    levenshtein.bind(eng, X)
    IJ = rng.integers(0, len(X), (12000, 2))
    IJ[:200, 1] = IJ[:200, 0]
    got = eng.metric_pairs(IJ)
    want = om.PackedStrings(X).pairs(IJ)
    assert np.array_equal(got, want)
    few = IJ[:7]  # a launch smaller than one wave's slots
    assert np.array_equal(eng.metric_pairs(few), want[:7])


@pytest.mark.parametrize("n_pairs", [70, 1001, 5000])
def test_levenshtein_short_list_kernel_ragged(monkeypatch, n_pairs):
    """Short pair lists of long strings take k_lev_p2 (two pairs per wave, each split into a forward and a backward half;
    pairs of two strings above 512 symbols a wave of their own).  Forced here for every list (ANNCHOR_LEV_P2_MAX) on strings
    of every interesting length -- empty, one symbol, around the 32-symbol word boundaries and the 512-symbol class boundary,
    the longest the kernel takes -- including (i, i) pairs and repeated pairs, against the oracle and against k_lev_f."""
    from annchor_amd import _native
    from annchor_amd.distances import levenshtein

    rng = np.random.default_rng(33)
    alphabet = [chr(c) for c in range(60, 120)]
    lens = list(range(0, 70)) + [95, 96, 97, 127, 128, 129, 255, 256, 257, 300, 480, 511, 512, 513, 544, 640, 1000, 1023, 1024]
    X = ["".join(rng.choice(alphabet[: rng.integers(2, 60)], n)) for n in lens for _ in range(2)]
    X += [X[9], X[150], "", ""]
    nx = len(X)
    IJ = rng.integers(0, nx, (n_pairs, 2))
    IJ[:40, 1] = IJ[:40, 0]          # (i, i)
    IJ[40:50] = IJ[60:70]            # repeats
    long_ids = np.flatnonzero(np.array([len(s) for s in X]) > 512)
    both_long = long_ids[: 2 * (len(long_ids) // 2)].reshape(-1, 2)[:8]
    IJ[60:60 + len(both_long)] = both_long   # both strings above 512 symbols: the unpacked class
    want = om.PackedStrings(X).pairs(IJ)
    out = {}
    for mode in ("1000000", "0"):
        monkeypatch.setenv("ANNCHOR_LEV_P2_MAX", mode)
        eng = _native.Engine(0)
        levenshtein.bind(eng, X)
        out[mode] = eng.metric_pairs(IJ)
        eng.close()
    assert np.array_equal(out["1000000"], want)
    assert np.array_equal(out["0"], want)


def test_levenshtein_anchor_round_kernel_ragged(monkeypatch):
    """The one-to-all launches of the picker run k_lev_a (one pair per wave, the two half-waves walk the two
    halves of the text towards each other, lev = min_i F[i] + B'[m - i]).  Anchor rows for selected anchors of every
    interesting length -- empty, one symbol, around the 32-symbol word boundaries, the longest string -- against the
    oracle, and equal to what the pair-list kernel gives for the same pairs."""
    from annchor_amd import _native
    from annchor_amd.distances import levenshtein

    rng = np.random.default_rng(21)
    alphabet = [chr(c) for c in range(60, 120)]
    lens = list(range(0, 70)) + [95, 96, 97, 127, 128, 129, 255, 256, 257, 300, 511, 512, 513, 640, 1000, 1023, 1024]
    X = ["".join(rng.choice(alphabet[: rng.integers(2, 60)], n)) for n in lens for _ in range(2)]
    X += [X[9], X[150], "", ""]
    nx = len(X)
    anchors = [0, 2, 3, 62, 64, 66, 130, 140, 150, 160, nx - 6, nx - 5, nx - 1, 9]
    P = om.PackedStrings(X)
    want = np.stack([P.pairs(np.stack([np.full(nx, a), np.arange(nx)], axis=1)) for a in anchors], axis=1)
    eng = _native.Engine(0)
    levenshtein.bind(eng, X)
    eng.pick_anchors_selected(anchors)
    got = eng.download(_native.F_D).reshape(nx, len(anchors))
    assert np.array_equal(got, want)
    for mode in ("0",):   # the pair-list kernel on the same one-to-all launches
        monkeypatch.setenv("ANNCHOR_LEV_ANCHOR", mode)
        eng2 = _native.Engine(0)
        levenshtein.bind(eng2, X)
        eng2.pick_anchors_selected(anchors)
        assert np.array_equal(eng2.download(_native.F_D).reshape(nx, len(anchors)), want)
    # a data set where every string has <= 16 words (all waves packed) and one with none (no wave packed)
    for lo, hi in ((0, 500), (513, 700)):
        Y = ["".join(rng.choice(alphabet[:7], n)) for n in rng.integers(lo, hi, 301)]
        monkeypatch.delenv("ANNCHOR_LEV_ANCHOR", raising=False)
        e3 = _native.Engine(0)
        levenshtein.bind(e3, Y)
        an = [0, 7, 300]
        e3.pick_anchors_selected(an)
        Py = om.PackedStrings(Y)
        w3 = np.stack([Py.pairs(np.stack([np.full(len(Y), a_), np.arange(len(Y))], axis=1)) for a_ in an], axis=1)
        assert np.array_equal(e3.download(_native.F_D).reshape(len(Y), 3), w3)


def test_levenshtein_anchor_rounds_one_launch(monkeypatch):
    """k_lev_ap: every round of the max-min picker in one launch (resident waves, the arrival slots are the arg-max).  A and D
    against the oracle's picker (pickers.py:44-50 incl. the D[1:] quirk and np.argmax's first index) and against the
    round-by-round launches, on ragged strings (duplicates, empties, all slot shapes); the rescue form (forced by a zero
    time limit: the first poll that finds a slot missing gives up) must give the same; a fit through either has the same graph."""
    from annchor_amd import Annchor, _native
    from annchor_amd.distances import levenshtein

    rng = np.random.default_rng(77)
    alphabet = [chr(c) for c in range(60, 120)]
    sets = []
    lens = list(range(0, 70)) + [95, 96, 97, 127, 128, 129, 255, 256, 257, 300, 511, 512, 513, 640, 1000, 1023, 1024]
    X = ["".join(rng.choice(alphabet[: rng.integers(2, 60)], n)) for n in lens for _ in range(2)]
    sets.append(X + [X[9], X[150], "", ""])
    sets.append(["".join(rng.choice(alphabet[:7], n)) for n in rng.integers(0, 500, 301)])      # every wave packed (odd count)
    sets.append(["".join(rng.choice(alphabet[:5], n)) for n in rng.integers(513, 700, 150)])    # no wave packed
    sets.append(["".join(rng.choice(alphabet[:3], n)) for n in rng.integers(1, 12, 900)])       # many ties
    for X in sets:
        nx = len(X)
        P = om.PackedStrings(X)
        for na, first in ((1, 0), (2, nx - 1), (3, 5), (17, nx // 2)):
            # (O.maxmin_anchors with the first index given instead of drawn)
            D = np.full((na, nx), np.inf)
            A = np.zeros(na, dtype=np.int64)
            ix = first
            for i in range(na):
                A[i] = ix
                D[i] = P.pairs(np.stack([np.full(nx, ix), np.arange(nx)], axis=1))
                ix = int(np.argmax(D[:1].min(axis=0))) if i == 0 else int(np.argmax(D[1:i + 1].min(axis=0)))
            for mode in ("default", "loop", "rescue"):
                monkeypatch.delenv("ANNCHOR_LEV_PERSIST", raising=False)
                monkeypatch.delenv("ANNCHOR_LEV_PERSIST_TIMEOUT_US", raising=False)
                if mode == "loop":
                    monkeypatch.setenv("ANNCHOR_LEV_PERSIST", "0")
                if mode == "rescue":
                    monkeypatch.setenv("ANNCHOR_LEV_PERSIST_TIMEOUT_US", "0")
                eng = _native.Engine(0)
                levenshtein.bind(eng, X)
                for _ in range(2):   # (twice: the arrival slots carry the previous launch's tags)
                    eng.pick_anchors_maxmin(na, first)
                    assert np.array_equal(eng.download(_native.F_A), A), (mode, na, first)
                    assert np.array_equal(eng.download(_native.F_D).reshape(nx, na), D.T), (mode, na, first)
                eng.close()
    monkeypatch.delenv("ANNCHOR_LEV_PERSIST", raising=False)
    monkeypatch.delenv("ANNCHOR_LEV_PERSIST_TIMEOUT_US", raising=False)
    X = sets[0]
    graphs = []
    for mode in ("default", "loop", "rescue"):
        if mode == "loop":
            monkeypatch.setenv("ANNCHOR_LEV_PERSIST", "0")
        if mode == "rescue":
            monkeypatch.delenv("ANNCHOR_LEV_PERSIST", raising=False)
            monkeypatch.setenv("ANNCHOR_LEV_PERSIST_TIMEOUT_US", "0")
        ann = Annchor(X, "levenshtein", n_anchors=9, n_neighbors=5, n_samples=400, p_work=0.3, random_seed=3)
        ann.fit()
        graphs.append((ann.neighbor_graph[0].copy(), ann.neighbor_graph[1].copy(), np.asarray(ann.A).copy()))
    for g in graphs[1:]:
        assert np.array_equal(g[2], graphs[0][2])
        assert np.array_equal(g[0], graphs[0][0]) and np.array_equal(g[1], graphs[0][1])


def test_persistent_anchor_launch_switches_itself_off(monkeypatch):
    """A persistent anchor launch that gives up costs its whole time limit before the rescue form runs.  The library looks at the
    abort word after the next host wait and, after two such launches, runs the picker's rounds as separate launches for the rest
    of the process (here: time limit 0 with ANNCHOR_LEV_PERSIST_LEARN so that the forced give-ups count); re-arming restores it.
    Results are the same throughout."""
    from annchor_amd import _native
    from annchor_amd.distances import levenshtein

    rng = np.random.default_rng(5)
    X = ["".join(rng.choice(list("abcdefg"), n)) for n in rng.integers(5, 300, 400)]
    assert _native.lev_persist_state(1) == 1
    eng = _native.Engine(0)
    levenshtein.bind(eng, X)
    eng.pick_anchors_maxmin(6, 3)
    ref = (eng.download(_native.F_A).copy(), eng.download(_native.F_D).copy())
    def launches(e):
        e.prof_enable(True)
        e.prof_reset()
        e.pick_anchors_maxmin(6, 3)
        e.synchronize()
        n = e.prof_get()["levenshtein_pairs"]["launches"]
        e.prof_enable(False)
        return n
    assert launches(eng) == 1                      # one persistent launch (the rescue instantiation is not a profiled launch)
    monkeypatch.setenv("ANNCHOR_LEV_PERSIST_TIMEOUT_US", "0")
    monkeypatch.setenv("ANNCHOR_LEV_PERSIST_LEARN", "1")
    try:
        for _ in range(3):                         # every launch gives up; each download below is a host wait that looks at the word
            eng.pick_anchors_maxmin(6, 3)
            assert np.array_equal(eng.download(_native.F_A), ref[0]) and np.array_equal(eng.download(_native.F_D), ref[1])
        assert _native.lev_persist_state() == 0    # switched off after the second
        monkeypatch.delenv("ANNCHOR_LEV_PERSIST_TIMEOUT_US")
        monkeypatch.delenv("ANNCHOR_LEV_PERSIST_LEARN")
        assert launches(eng) == 6                  # the rounds one by one
        assert np.array_equal(eng.download(_native.F_A), ref[0]) and np.array_equal(eng.download(_native.F_D), ref[1])
    finally:
        assert _native.lev_persist_state(1) == 1   # re-armed for the tests that follow
    assert launches(eng) == 1
    eng.close()


def test_levenshtein_wide_alphabet(monkeypatch):
    """More than 256 distinct symbols (16-bit codes, k_lev_w: match words computed per column).  (i) The wide kernel forced
    on the ragged byte-alphabet set must equal the oracle's C restatement; (ii) strings over ~3000 distinct code points
    (CJK range) against a NumPy DP; (iii) a fit on such strings equals the fit with a Python metric on the host."""
    from annchor_amd import Annchor, _native
    from annchor_amd.distances import levenshtein

    rng = np.random.default_rng(31)
    alphabet = [chr(c) for c in range(60, 120)]
    lens = list(range(0, 70)) + [95, 96, 97, 127, 128, 129, 255, 256, 257, 300, 511, 512, 513, 640, 1000]
    X = ["".join(rng.choice(alphabet[: rng.integers(2, 60)], n)) for n in lens for _ in range(2)] + ["", ""]
    monkeypatch.setenv("ANNCHOR_LEV_WIDE", "1")
    eng = _native.Engine(0)
    levenshtein.bind(eng, X)
    IJ = rng.integers(0, len(X), (6000, 2))
    IJ[:100, 1] = IJ[:100, 0]
    assert np.array_equal(eng.metric_pairs(IJ), om.PackedStrings(X).pairs(IJ))
    eng.pick_anchors_selected([3, 150, len(X) - 1])
    P = om.PackedStrings(X)
    want = np.stack([P.pairs(np.stack([np.full(len(X), a_), np.arange(len(X))], axis=1)) for a_ in (3, 150, len(X) - 1)], axis=1)
    assert np.array_equal(eng.download(_native.F_D).reshape(len(X), 3), want)
    monkeypatch.delenv("ANNCHOR_LEV_WIDE")

    def dp(a, b):   # textbook unit-cost DP, one NumPy row at a time
        a, b = np.array([ord(c) for c in a]), np.array([ord(c) for c in b])
        prev = np.arange(len(b) + 1)
        for i in range(len(a)):
            sub = prev[:-1] + (b != a[i])
            cur = np.minimum(sub, prev[1:] + 1)
            cur = np.concatenate([[i + 1], cur])
            # insertions: cur[j] = min(cur[j], cur[j-1] + 1), a running minimum of (cur[j] - j)
            cur = np.minimum.accumulate(cur - np.arange(len(b) + 1)) + np.arange(len(b) + 1)
            prev = cur
        return int(prev[-1])

    cjk = [chr(c) for c in range(0x4E00, 0x4E00 + 3000)]
    Y = []
    for _ in range(120):
        base = list(rng.choice(cjk, rng.integers(0, 180)))
        Y.append("".join(base))
        for _ in range(2):   # near-duplicates: non-trivial distances
            v = list(base)
            for _ in range(rng.integers(0, 12)):
                if v and rng.random() < 0.5:
                    v.pop(rng.integers(0, len(v)))
                else:
                    v.insert(rng.integers(0, len(v) + 1), rng.choice(cjk))
            Y.append("".join(v))
    e2 = _native.Engine(0)
    levenshtein.bind(e2, Y)
    assert e2.lib is not None
    IJ2 = rng.integers(0, len(Y), (400, 2))
    got = e2.metric_pairs(IJ2)
    assert list(got) == [dp(Y[i], Y[j]) for i, j in IJ2]
    cfg = dict(n_anchors=6, n_neighbors=6, n_samples=300, p_work=0.4)
    a = Annchor(np.array(Y, dtype=object), "levenshtein", **cfg).fit()
    b = Annchor(np.array(Y, dtype=object), dp, **cfg).fit()
    assert np.array_equal(a.A, b.A) and np.array_equal(a.D, b.D)
    assert np.array_equal(a.neighbor_graph[1], b.neighbor_graph[1])


@pytest.mark.parametrize("variant", ["0"])
def test_anchor_round_kernel_vs_pair_list_kernel_fit(variant, strings, monkeypatch):
    """Max-min picking on the anchor kernels against the same fit with the anchor rounds on the pair-list
    kernel (ANNCHOR_LEV_ANCHOR=0): same anchors, distances and graph."""
    from annchor_amd import Annchor
    X = np.array(strings[::4])
    cfg = dict(n_anchors=12, n_neighbors=10, n_samples=700, p_work=0.3, random_seed=42)
    ref = Annchor(X, "levenshtein", **cfg).fit()
    monkeypatch.setenv("ANNCHOR_LEV_ANCHOR", variant)
    alt = Annchor(X, "levenshtein", **cfg).fit()
    assert np.array_equal(ref.A, alt.A) and np.array_equal(ref.D, alt.D)
    assert np.array_equal(ref.neighbor_graph[0], alt.neighbor_graph[0]) and np.array_equal(ref.neighbor_graph[1], alt.neighbor_graph[1])


@pytest.mark.parametrize("variant", ["1"])
def test_anchor_pick_fused_vs_separate(variant, strings, monkeypatch):
    """The default fit (persistent anchor launch, k_lev_f pair lists) against the same fit on k_lev_r<1> with the max-min pick
    (pickers.py:47-50) fused into the next round's launch (ANNCHOR_LEV_R=1): same anchors, same anchor distances, same graph."""
    from annchor_amd import Annchor
    X = np.array(strings[::4])
    cfg = dict(n_anchors=12, n_neighbors=10, n_samples=700, p_work=0.3, random_seed=42)
    ref = Annchor(X, "levenshtein", **cfg)
    ref.fit()
    monkeypatch.setenv("ANNCHOR_LEV_R", variant)
    alt = Annchor(X, "levenshtein", **cfg)
    alt.fit()
    assert np.array_equal(ref.A, alt.A)
    assert np.array_equal(ref.D, alt.D)
    assert np.array_equal(ref.neighbor_graph[0], alt.neighbor_graph[0])
    assert np.array_equal(ref.neighbor_graph[1], alt.neighbor_graph[1])


@pytest.mark.parametrize("dtype,dim", [(np.float32, 128), (np.float64, 64), (np.float64, 5)])
def test_cosine_pairs_vs_scipy(dtype, dim):
    """'cosine' (reference utils.py:14,67 -> scipy.spatial.distance.cosine).  No reference test pins
    it: pinned here against scipy itself.  Tolerance: the three dot products are summed
    in a different order than BLAS does -- 1e-12 absolute for float64 data, 2e-6 for float32 data
    (dot products rounded to float32 as scipy's are)."""
    from scipy.spatial.distance import cosine as sp_cosine

    from annchor_amd import Annchor, BruteForce, _native
    from annchor_amd.distances import cosine

    rng = np.random.default_rng(11)
    X = (rng.standard_normal((400, dim)) + 0.5).astype(dtype)
    eng = _native.Engine(0)
    cosine.bind(eng, X)
    IJ = rng.integers(0, 400, (3000, 2))
    IJ[:20, 1] = IJ[:20, 0]
    got = eng.metric_pairs(IJ)
    want = np.array([sp_cosine(X[i], X[j]) for i, j in IJ])
    tol = 2e-6 if dtype == np.float32 else 1e-12
    np.testing.assert_allclose(got, want, rtol=0, atol=tol)
    assert np.all(got >= 0) and np.all(got <= 2)
    # the whole pipeline runs on the device metric: exact graph by brute force, Annchor reports true distances
    bf = BruteForce(X, "cosine").fit(n_neighbors=6)
    ann = Annchor(X, "cosine", n_anchors=10, n_neighbors=6, n_samples=600, p_work=0.5).fit()
    idx, dist = ann.neighbor_graph
    for r in range(0, 400, 37):
        np.testing.assert_allclose(dist[r, 1:], [sp_cosine(X[r], X[j]) for j in idx[r, 1:]], rtol=0, atol=tol)
    assert np.all(bf.neighbor_graph[1][:, 0] <= tol)


@pytest.mark.parametrize("dtype,dim", [(np.float32, 128), (np.float64, 3), (np.float32, 7), (np.float64, 64)])
def test_euclidean_pairs_vs_oracle(dtype, dim):
    from annchor_amd import _native

    rng = np.random.default_rng(2)
    X = rng.standard_normal((500, dim)).astype(dtype)
    eng = _native.Engine(0)
    eng.set_points(X)
    IJ = rng.integers(0, 500, (5000, 2))
    got = eng.metric_pairs(IJ)
    want = om.euclidean_pairs(X, IJ)
    # float tolerance: one rounding of the input precision (reference: np.linalg.norm in X's dtype)
    np.testing.assert_allclose(got, want, rtol=2e-6 if dtype == np.float32 else 1e-14, atol=0)


# ----------------------------------------------------- full pipeline, stage by stage
def _staged_compare(ann, ora_factory, float_metric=False):
    """Run Annchor.fit()'s stages on the GPU and the oracle side by side and compare
    the state after every stage."""
    trace = {}
    ora = ora_factory(trace)
    ora.fit()
    ann.get_anchors()
    assert np.array_equal(ann.A, ora.A)
    if float_metric:
        np.testing.assert_allclose(ann.D, ora.D, rtol=1e-14)
    else:
        assert np.array_equal(ann.D, ora.D)
    ann.get_locality()
    assert np.array_equal(ann.IJs, ora.IJs)
    assert np.array_equal(ann.I.ptr, ora.I_ptr)
    assert np.array_equal(ann.I.idx, ora.I_idx)
    ann.get_features()
    if not float_metric:
        assert np.array_equal(ann.features, trace["features"]["features"])
    assert np.array_equal(ann.not_computed_mask, trace["features"]["ncm"])
    for it in range(ann.niters):
        ann.get_sample()
        r = trace["regress%d" % it]
        assert np.array_equal(ann.sample_ixs, r["sample_ixs"])
        if float_metric:
            np.testing.assert_allclose(ann.sample_bins[1:-1], r["bins"][1:-1], rtol=1e-13)
        else:
            assert np.array_equal(ann.sample_bins, r["bins"])
        if float_metric:
            np.testing.assert_allclose(ann.sample_y, r["sample_y"], rtol=1e-14)
        else:
            assert np.array_equal(ann.sample_y, r["sample_y"])
        ann.fit_predict_regression()
        ann.fit_predict_errors()
        np.testing.assert_allclose(ann.regression.coef_, r["W"], rtol=1e-9, atol=1e-12)
        if not float_metric:
            # same coefficients to the last bit => same predictions to the last bit
            if np.array_equal(ann.regression.coef_, r["W"]) and np.array_equal(ann.regression.intercept_, r["c"]):
                assert np.array_equal(ann.RefineApprox, r["RA"])
            np.testing.assert_allclose(ann.RefineApprox, r["RA"], rtol=1e-12, atol=1e-9)
        assert np.array_equal(ann.errors, r["labels"])
        ann.select_refine_candidate_pairs(w=1 / ann.niters, it=it)
        s = trace["select%d" % it]
        assert s["n_refine"] == ann.n_refine
        if not float_metric:
            assert np.array_equal(ann.thresh, s["thresh"])
            assert np.array_equal(ann.mapback, s["mapback"])
            assert np.array_equal(ann.nextback, s["nextback"])
        if it < ann.niters - 1:
            ann.update_anchor_points()
            if not float_metric:
                u = trace["update%d" % it]
                assert np.array_equal(ann.features[:, 0], u["lb"])
                assert np.array_equal(ann.features[:, 1], u["ub"])
            elif "update%d" % it in trace:
                # (the anchor distances differ from the oracle's by their rounding: no equality)
                u = trace["update%d" % it]
                np.testing.assert_allclose(ann.features[:, 0], u["lb"], rtol=1e-12)
                np.testing.assert_allclose(ann.features[:, 1], u["ub"], rtol=1e-12)
    ann.get_ann()
    assert ann.evals == ora.evals
    if not float_metric:
        assert np.array_equal(ann.neighbor_graph[1], ora.neighbor_graph[1])
        assert np.array_equal(ann.neighbor_graph[0], ora.neighbor_graph[0])
    return ora


def test_fit_strings_small_matches_oracle_stagewise(strings):
    from annchor_amd import Annchor

    Xs = strings[::5]
    cfg = dict(n_anchors=8, n_neighbors=10, n_samples=700, p_work=0.3, random_seed=42, niters=2)
    ann = Annchor(np.array(Xs), "levenshtein", **cfg)
    P = om.PackedStrings(Xs)
    _staged_compare(ann, lambda tr: O.OracleAnnchor(len(Xs), P.pairs, trace=tr, **cfg))
    # and against the golden vectors captured from the reference itself
    G = np.load(os.path.join(GOLD, "strings_small.npz"))
    assert np.array_equal(ann.A, G["A"]) and np.array_equal(ann.D, G["D"])
    assert np.array_equal(ann.IJs, G["IJs"])
    assert ann.evals == int(G["evals"])


def test_fit_euclid_small_matches_oracle_stagewise():
    """float64 Euclidean, sparse (asymmetric) locality, 3 iterations."""
    from annchor_amd import Annchor

    G = np.load(os.path.join(GOLD, "euclid_small.npz"))
    X = G["X"]
    cfg = dict(n_anchors=12, n_neighbors=8, n_samples=400, p_work=0.25, random_seed=3, niters=3, locality=3)
    ann = Annchor(X, "euclidean", **cfg)
    ora = _staged_compare(ann, lambda tr: O.OracleAnnchor(len(X), lambda IJ: om.euclidean_pairs(X, IJ), trace=tr, **cfg),
                          float_metric=True)
    assert np.array_equal(ann.A, G["A"])
    assert np.array_equal(ann.IJs, G["IJs"])  # reference's own candidate set (adjust_check path)
    np.testing.assert_allclose(ann.neighbor_graph[1], ora.neighbor_graph[1], rtol=1e-12)


@pytest.mark.parametrize("n_anchors,locality", [(70, 9), (130, 5), (200, 40)])
def test_fit_more_than_64_anchors_matches_oracle_stagewise(strings, n_anchors, locality):
    """More anchors than one 64-bit mask word holds (the reference takes any n_anchors, annchor.py:117-148): the nearest-anchor
    sets become 2- or 4-word masks (up to 256 anchors).  Every stage against the oracle, strings and float64 points; the
    query path and the nearest-enemy candidates run on the same masks."""
    from annchor_amd import Annchor

    Xs = strings[::3]
    cfg = dict(n_anchors=n_anchors, n_neighbors=10, n_samples=900, p_work=0.6, random_seed=7, niters=2, locality=locality,
               loc_thresh=max(1, locality // 4))
    ann = Annchor(np.array(Xs), "levenshtein", **cfg)
    P = om.PackedStrings(Xs)
    _staged_compare(ann, lambda tr: O.OracleAnnchor(len(Xs), P.pairs, trace=tr, **cfg))
    sid = ann.sid
    want = O.nearest_anchor_sets(ann.D, locality)
    assert all(set(a) == set(b) for a, b in zip(sid, want))
    rng = np.random.default_rng(n_anchors)
    X = rng.standard_normal((700, 6))
    cfg2 = dict(n_anchors=n_anchors, n_neighbors=8, n_samples=600, p_work=0.5, random_seed=3, niters=2, locality=locality)
    b = Annchor(X, "euclidean", **cfg2)
    _staged_compare(b, lambda tr: O.OracleAnnchor(len(X), lambda IJ: om.euclidean_pairs(X, IJ), trace=tr, **cfg2), float_metric=True)
    # query: the device path equals the oracle's query on the fitted state
    Q = rng.standard_normal((40, 6))
    qi, qd = b.query(Q, nn=5, p_work=0.9)
    d_all = np.sqrt(((Q[:, None, :] - X[None]) ** 2).sum(-1))
    truth = np.sort(d_all, axis=1)[:, :5]
    assert np.mean(np.isclose(qd, truth, rtol=1e-9)) > 0.8     # (an approximate search: few of many anchors are shared)
    # nearest enemies run on the same masks
    y = (X[:, 0] > 0).astype(np.int64)
    b.get_nearest_enemies(y, nn=2)
    ne_truth = np.array([np.sort(np.sqrt(((X[i] - X[y != y[i]]) ** 2).sum(-1)))[0] for i in range(len(X))])
    assert np.mean(np.isclose(np.asarray(b.nearest_enemy_graph[1])[:, 0], ne_truth, rtol=1e-9)) > 0.8


def test_fit_strings_c2_full(strings):
    """BASELINE config 2: N=1600, n_anchors=15, k=25, p_work=0.12."""
    from annchor_amd import Annchor, compare_neighbor_graphs

    G = np.load(os.path.join(GOLD, "strings_full.npz"))          # captured from the reference
    Go = np.load(os.path.join(GOLD, "strings_full_oracle.npz"))  # the oracle at the same config
    ann = Annchor(np.array(strings), "levenshtein", n_anchors=15, n_neighbors=25, p_work=0.12, random_seed=42).fit()
    assert np.array_equal(ann.A, G["c1_A"])
    assert np.array_equal(ann.D, G["c1_D"].astype(np.float64))
    assert ann.evals == int(G["c1_evals"]) == int(Go["c1_evals"])
    # candidate set: equals the oracle's; the reference's differs by 26 pairs whose
    # membership hinges on a tie at the 5th-nearest-anchor cut (unstable argsort there)
    assert ann.n_pairs == int(Go["c1_npairs"])
    assert abs(ann.n_pairs - int(G["c1_npairs"])) < 100
    # the graph is bit-identical to the oracle's
    assert np.array_equal(ann.neighbor_graph[1], Go["c1_ng_dist"].astype(np.float64))
    assert np.array_equal(ann.neighbor_graph[0], Go["c1_ng_idx"].astype(np.int64))
    truth = (G["truth_idx"].astype(np.int64), G["truth_dist"].astype(np.float64))
    err = compare_neighbor_graphs(truth, ann.neighbor_graph, 25)
    assert err == int(Go["c1_errors"]) and err <= int(G["c1_errors"])  # 346 <= the reference's 504 of 40 000
    # every reported distance is the exact metric value of the reported neighbour
    idx, dist = ann.neighbor_graph
    IJ = np.stack([np.repeat(np.arange(1600), 24), idx[:, 1:].ravel()], axis=1)
    assert np.array_equal(om.PackedStrings(strings).pairs(IJ), dist[:, 1:].ravel())


def test_fit_strings_readme_config_zero_errors(strings):
    """reference README.md:102-116: n_anchors=20 (default), k=25, p_work=0.12 -> 0 errors."""
    from annchor_amd import Annchor, compare_neighbor_graphs

    G = np.load(os.path.join(GOLD, "strings_full.npz"))
    ann = Annchor(np.array(strings), "levenshtein", n_neighbors=25, p_work=0.12).fit()
    truth = (G["truth_idx"].astype(np.int64), G["truth_dist"].astype(np.float64))
    Go = np.load(os.path.join(GOLD, "strings_full_oracle.npz"))
    assert np.array_equal(ann.A, G["readme_A"])
    assert np.array_equal(ann.neighbor_graph[1], Go["readme_ng_dist"].astype(np.float64))
    assert compare_neighbor_graphs(truth, ann.neighbor_graph, 25) == int(Go["readme_errors"]) == 0   # reference: 0 (README.md:116)


def test_fit_strings_reference_test_config(strings):
    """The reference's own test_strings configuration (tests/test_annchor.py:83-102): n_anchors=23,
    n_neighbors=15, n_samples=5000, p_work=0.12, niters=4 -- three update_bounds passes on the
    device.  Anchors / anchor distances / evaluation count equal the reference run's; the graph is
    bit-identical to the oracle's (tests/golden/make_oracle_fixtures.py); the reference test's bar
    is < 15 errors (its own run here: 4)."""
    from annchor_amd import Annchor, compare_neighbor_graphs

    G = np.load(os.path.join(GOLD, "strings_full.npz"))
    Go = np.load(os.path.join(GOLD, "strings_full_oracle.npz"))
    cfg = dict(n_anchors=23, n_neighbors=15, n_samples=5000, p_work=0.12, niters=4, random_seed=42)
    ann = Annchor(np.array(strings), "levenshtein", **cfg).fit()
    assert np.array_equal(ann.A, G["test_A"])
    assert np.array_equal(ann.D, G["test_D"].astype(np.float64))
    assert ann.evals == int(G["test_evals"]) == int(Go["test_evals"])
    assert ann.n_pairs == int(G["test_npairs"]) == int(Go["test_npairs"])
    assert np.array_equal(ann.neighbor_graph[1], Go["test_ng_dist"].astype(np.float64))
    assert np.array_equal(ann.neighbor_graph[0], Go["test_ng_idx"].astype(np.int64))
    truth = (G["truth_idx"].astype(np.int64), G["truth_dist"].astype(np.float64))
    err = compare_neighbor_graphs(truth, ann.neighbor_graph, 15)
    assert err == int(Go["test_errors"]) and err < 15
    idx, dist = ann.neighbor_graph
    IJ = np.stack([np.repeat(np.arange(1600), 14), idx[:, 1:].ravel()], axis=1)
    assert np.array_equal(om.PackedStrings(strings).pairs(IJ), dist[:, 1:].ravel())


def test_fit_strings_four_iterations_stagewise(strings):
    """niters=4 stage by stage against the oracle (every update_bounds pass, every selection)."""
    from annchor_amd import Annchor

    Xs = strings[::4]
    cfg = dict(n_anchors=10, n_neighbors=8, n_samples=600, p_work=0.3, random_seed=7, niters=4)
    ann = Annchor(np.array(Xs), "levenshtein", **cfg)
    P = om.PackedStrings(Xs)
    _staged_compare(ann, lambda tr: O.OracleAnnchor(len(Xs), P.pairs, trace=tr, **cfg))


def test_blobs_pinned_anchors_and_errors():
    """reference tests/test_examples.py:88-230: pinned A, 0 errors with max-min anchors."""
    from annchor_amd import Annchor, compare_neighbor_graphs

    G = np.load(os.path.join(GOLD, "blobs.npz"))
    X = G["X"]
    ann = Annchor(X, "euclidean", n_anchors=10, p_work=0.05).fit()
    assert np.array_equal(ann.A, np.array([102, 674, 347, 586, 214, 963, 365, 348, 430, 429]))
    bf = (np.zeros((1000, 16), dtype=np.int64), G["bf_dist"])
    assert compare_neighbor_graphs(bf, ann.neighbor_graph, 15) == 0


def test_host_metric_path(strings):
    """A user-supplied Python metric is evaluated on the host; everything after it
    still runs on the GPU (reference tests/test_annchor.py:105-145 pattern)."""
    from annchor_amd import Annchor

    Xs = list(strings[::5])
    P = om.PackedStrings(Xs)
    calls = []

    def evaluator(f, X, IJ):
        calls.append(len(IJ))
        return P.pairs(np.asarray(IJ, dtype=np.int64))

    cfg = dict(n_anchors=8, n_neighbors=10, n_samples=700, p_work=0.3, random_seed=42, niters=2)
    ann = Annchor(np.array(Xs), lambda a, b: 0.0, get_exact_ijs=evaluator, **cfg).fit()
    ora = O.OracleAnnchor(len(Xs), P.pairs, **cfg).fit()
    assert ann.evals == ora.evals
    assert np.array_equal(ann.neighbor_graph[1], ora.neighbor_graph[1])
    assert np.array_equal(ann.neighbor_graph[0], ora.neighbor_graph[0])
    assert sum(calls) >= ora.evals


# ------------------------------------------------------------------ metric: a4
def test_wasserstein_known_answer_and_stored_graph():
    """reference tests/test_datasets.py:107-108 and the reference's stored exact-EMD graph."""
    from annchor_amd import _native
    from annchor_amd.distances import Wasserstein

    d = om.load_digits()
    X, M, (ngi, ngd) = d["X"], d["cost_matrix"], d["neighbor_graph"]
    eng = _native.Engine(0)
    Wasserstein(M).bind(eng, X)
    assert abs(eng.metric_pairs(np.array([[10, 676]]))[0] - 0.305587260000565) < 1e-12
    rng = np.random.default_rng(0)
    rows = rng.integers(0, 1797, 30000)
    cols = rng.integers(0, 100, 30000)
    IJ = np.stack([rows, ngi[rows, cols]], axis=1)
    got = eng.metric_pairs(IJ)
    # float tolerance: 1e-12 absolute against the reference's stored float64 distances
    np.testing.assert_allclose(got, ngd[rows, cols], rtol=0, atol=1e-12)


def test_wasserstein_pairs_vs_oracle_far_pairs():
    from annchor_amd import _native
    from annchor_amd.distances import Wasserstein

    d = om.load_digits()
    X, M = d["X"], d["cost_matrix"]
    eng = _native.Engine(0)
    Wasserstein(M).bind(eng, X)
    rng = np.random.default_rng(1)
    IJ = rng.integers(0, 1797, (20000, 2))
    IJ[:10, 1] = IJ[:10, 0]
    got = eng.metric_pairs(IJ)
    want = om.Histograms(X, M).pairs(IJ)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    assert np.all(got[:10] == 0)


def test_wasserstein_non_integer_histograms():
    """General float histograms with sparse and full supports, non-grid cost."""
    from annchor_amd import _native
    from annchor_amd.distances import Wasserstein

    rng = np.random.default_rng(2)
    nb = 24
    pts = rng.random((nb, 3))
    M = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))
    X = rng.random((200, nb)) * (rng.random((200, nb)) < 0.6)
    X[:, 0] += 0.1  # no empty histogram
    X[5] = 1.0      # full support
    eng = _native.Engine(0)
    Wasserstein(M).bind(eng, X)
    IJ = rng.integers(0, 200, (3000, 2))
    got = eng.metric_pairs(IJ)
    want = om.Histograms(X, M).pairs(IJ)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("solver", ["simplex", "simplex_bland", "ssp", "ssp_wide_flows"])
def test_wasserstein_solver_variants(monkeypatch, solver):
    """Metric ground costs take the transportation simplex (k_emd_ns: one lane per node, Dantzig pricing); forced here: the same
    kernel under Bland's rule from the first pivot (its anti-cycling fallback), and the successive-shortest-path kernel with int16 /
    int32 flow slabs.  Each against the oracle: digits (integer masses; near, far and identical pairs, the one-to-all form of the
    anchor rounds), float histograms on a 64-bin non-grid metric with full supports (n + m = 64 nodes), two-bin histograms."""
    from annchor_amd import _native
    from annchor_amd.distances import Wasserstein

    if solver == "simplex_bland":
        monkeypatch.setenv("ANNCHOR_EMD_DANTZIG_CAP", "0")
    if solver.startswith("ssp"):
        monkeypatch.setenv("ANNCHOR_EMD_SOLVER", "ssp")
    if solver == "ssp_wide_flows":
        monkeypatch.setenv("ANNCHOR_EMD_WIDE_FLOWS", "1")
    d = om.load_digits()
    X, M, (ngi, _) = d["X"], d["cost_matrix"], d["neighbor_graph"]
    rng = np.random.default_rng(11)
    eng = _native.Engine(0)
    Wasserstein(M).bind(eng, X)
    rows = rng.integers(0, 1797, 3000)
    IJ = np.concatenate([np.stack([rows, ngi[rows, rng.integers(0, 100, 3000)].astype(np.int64)], axis=1), rng.integers(0, 1797, (3000, 2))])
    IJ[:5, 1] = IJ[:5, 0]
    H = om.Histograms(X, M)
    np.testing.assert_allclose(eng.metric_pairs(IJ), H.pairs(IJ), rtol=0, atol=1e-12)
    eng.pick_anchors_selected([7, 1500])
    D = eng.download(_native.F_D).reshape(1797, 2)
    for col, a_ in enumerate((7, 1500)):
        np.testing.assert_allclose(D[:, col], H.pairs(np.stack([np.full(1797, a_), np.arange(1797)], axis=1)), rtol=0, atol=1e-12)
    eng.close()
    nb = 64
    pts = rng.random((nb, 2))
    M2 = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))
    Y = rng.random((120, nb)) * (rng.random((120, nb)) < 0.7)
    Y[:, 0] += 0.05
    Y[3] = rng.random(nb) + 0.1      # full supports: after the common mass cancels every bin is a source or a sink
    Y[4] = rng.random(nb) + 0.1
    Y[5] = 0; Y[5, 9] = 1.0          # one bin against everything
    Y[6] = 0; Y[6, 9] = 0.3; Y[6, 40] = 0.7
    e2 = _native.Engine(0)
    Wasserstein(M2).bind(e2, Y)
    IJ2 = rng.integers(0, 120, (2500, 2))
    IJ2[:4] = [[3, 4], [5, 6], [5, 3], [6, 6]]
    np.testing.assert_allclose(e2.metric_pairs(IJ2), om.Histograms(Y, M2).pairs(IJ2), rtol=0, atol=1e-12)
    e2.close()


@pytest.mark.parametrize("integral", [True, False])
def test_wasserstein_more_than_64_bins_sparse(integral):
    """Histograms of more than 64 bins (the reference takes any: utils.py:75-86) run when each has at most 32 non-zero entries
    and the ground cost is a metric: the simplex kernel takes the (bin, mass) lists -- x's entries on lanes 0..31, y's on 32..63,
    costs from global memory.  200 bins on a 2-d point cloud against the oracle (pairs with overlapping, disjoint, identical and
    one-bin supports; the one-to-all form); a small fit against brute force; the two refusals (support > 32, non-metric cost)."""
    from annchor_amd import Annchor, BruteForce, _native, compare_neighbor_graphs
    from annchor_amd.distances import Wasserstein

    rng = np.random.default_rng(5 + integral)
    nb, nx = 200, 400
    pts = rng.random((nb, 2)) * 10
    M = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))
    X = np.zeros((nx, nb))
    for i in range(nx):
        k = int(rng.integers(1, 33))
        centre = rng.integers(0, nb)
        near = np.argsort(M[centre])[:60]
        sup = rng.choice(near, k, replace=False)
        X[i, sup] = rng.integers(1, 40, k) if integral else rng.random(k) + 0.01
    X[7] = 0; X[7, 13] = 5 if integral else 0.7            # one bin
    X[8] = X[9]                                            # identical pair
    X[10] = 0; X[10, :32] = np.arange(1, 33)               # the fullest support
    X[11] = 0; X[11, 32:64] = np.arange(1, 33)             # ... against a disjoint one: 64 nodes
    eng = _native.Engine(0)
    Wasserstein(M).bind(eng, X)
    IJ = rng.integers(0, nx, (4000, 2))
    IJ[:5] = [[7, 20], [8, 9], [10, 11], [11, 10], [7, 7]]
    H = om.Histograms(X, M)
    got = eng.metric_pairs(IJ)
    np.testing.assert_allclose(got, H.pairs(IJ), rtol=0, atol=1e-11)
    assert got[1] == 0 and got[4] == 0
    eng.pick_anchors_selected([10, 200])
    D = eng.download(_native.F_D).reshape(nx, 2)
    for col, a_ in enumerate((10, 200)):
        np.testing.assert_allclose(D[:, col], H.pairs(np.stack([np.full(nx, a_), np.arange(nx)], axis=1)), rtol=0, atol=1e-11)
    eng.close()
    f = Wasserstein(M)
    ann = Annchor(X, f, n_anchors=8, n_neighbors=6, n_samples=300, p_work=0.6, random_seed=1).fit()
    bf = BruteForce(X, Wasserstein(M)).fit(6)
    assert compare_neighbor_graphs(bf.neighbor_graph, ann.neighbor_graph, 6) <= 0.03 * nx * 6
    Xbad = X.copy(); Xbad[0, :40] = 1.0
    with pytest.raises(Exception, match="32 non-zero"):
        Wasserstein(M).bind(_native.Engine(0), Xbad)
    with pytest.raises(Exception, match="metric ground cost"):
        Wasserstein(M ** 2).bind(_native.Engine(0), X)


@pytest.mark.parametrize("kind", ["squared", "asymmetric", "metric_integer"])
def test_wasserstein_cost_matrix_kinds(kind):
    """The solver cancels the mass two histograms share on a bin only when the ground cost is a metric (zero diagonal,
    triangle inequality: checked when the histograms are bound).  A squared-distance cost and an asymmetric cost with a
    non-zero diagonal keep the full problem; an integer-valued metric cost on integer histograms takes the reduced integer
    route.  All against the CPU restatement (which never reduces)."""
    from annchor_amd import _native
    from annchor_amd.distances import Wasserstein

    rng = np.random.default_rng(11)
    nb = 20
    pts = rng.integers(0, 6, (nb, 2)).astype(np.float64)
    D = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))
    if kind == "squared":
        M = D ** 2
        X = rng.random((120, nb)) * (rng.random((120, nb)) < 0.7)
    elif kind == "asymmetric":
        M = D + rng.random((nb, nb))          # no symmetry, positive diagonal
        X = rng.random((120, nb)) * (rng.random((120, nb)) < 0.7)
    else:
        M = np.abs(pts[:, None, 0] - pts[None, :, 0]) + np.abs(pts[:, None, 1] - pts[None, :, 1])   # L1: a metric (repeated points: zero off-diagonal entries)
        X = rng.integers(0, 9, (120, nb)).astype(np.float64) * (rng.random((120, nb)) < 0.7)
    X[:, 0] += 1.0
    X[7] = X[3]          # identical histograms: nothing left to move
    X[9] = 2.0 * X[3]    # ... also after normalisation
    eng = _native.Engine(0)
    Wasserstein(M).bind(eng, X)
    IJ = np.vstack([rng.integers(0, 120, (2500, 2)), [[3, 7], [7, 3], [3, 9], [5, 5]]])
    got = eng.metric_pairs(IJ)
    want = om.Histograms(X, M).pairs(IJ)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-11 if kind == "squared" else 1e-12)
    if kind == "metric_integer":
        assert got[-4] == 0.0 and got[-3] == 0.0 and got[-2] == 0.0 and got[-1] == 0.0
    eng.close()


def test_fit_digits_c4():
    """BASELINE config 4: digits Wasserstein, N=1797, n_anchors=20, k=25, p_work=0.16."""
    from annchor_amd import Annchor, compare_neighbor_graphs

    d = om.load_digits()
    G = np.load(os.path.join(GOLD, "digits_full.npz"))
    ann = Annchor(d["X"], "wasserstein", func_kwargs={"cost_matrix": d["cost_matrix"]}, n_anchors=20,
                  n_neighbors=25, n_samples=5000, p_work=0.16, random_seed=42).fit()
    assert np.array_equal(ann.A, G["c4_A"])
    np.testing.assert_allclose(ann.D, G["c4_D"], rtol=0, atol=1e-12)
    assert ann.evals == int(G["c4_evals"])
    err = compare_neighbor_graphs(d["neighbor_graph"], ann.neighbor_graph, 25)
    assert err <= 7, err  # no worse than the reference's own run here: 7 of 44 925 (measured: 4); reference test bar: < 10
    # every reported distance within 1e-9 of the exact EMD of the reported neighbour
    idx, dist = ann.neighbor_graph
    IJ = np.stack([np.repeat(np.arange(1797), 24), idx[:, 1:].ravel()], axis=1)
    np.testing.assert_allclose(om.Histograms(d["X"], d["cost_matrix"]).pairs(IJ), dist[:, 1:].ravel(), rtol=0, atol=1e-9)


# ------------------------------------------------------------------ BruteForce (f1)
def test_brute_force_digits_matches_stored_graph():
    """reference tests/test_annchor.py:216-248: BruteForce on X[:500] == stored graph restricted
    to the first 500 points -> 0 errors."""
    from annchor_amd import BruteForce, compare_neighbor_graphs

    d = om.load_digits()
    ngi, ngd = d["neighbor_graph"]
    small = (np.array([ngi[i][ngi[i] < 500][:10] for i in range(500)]), np.array([ngd[i][ngi[i] < 500][:10] for i in range(500)]))
    bf = BruteForce(d["X"][:500], "wasserstein", func_kwargs={"cost_matrix": d["cost_matrix"]}).fit()
    assert bf.neighbor_graph[0].shape == (500, 500)
    assert compare_neighbor_graphs(small, bf.neighbor_graph, 10) == 0
    assert np.array_equal(bf.neighbor_graph[0][:, 0], np.arange(500))


def test_brute_force_strings_equals_oracle(strings):
    from annchor_amd import BruteForce

    Xs = strings[::4]
    bf = BruteForce(np.array(Xs), "levenshtein").fit()
    oi, od, _ = O.brute_force(om.PackedStrings(Xs).pairs, len(Xs))
    assert np.array_equal(bf.neighbor_graph[1], od)
    assert np.array_equal(bf.neighbor_graph[0], oi)   # stable (distance, index) order
    part = BruteForce(np.array(Xs), "levenshtein").fit(n_neighbors=7)
    assert np.array_equal(part.neighbor_graph[0], oi[:, :7])


# ------------------------------------------------------------------ query (f2)
def test_query_matches_oracle_strings(strings):
    """Annchor.query (annchor.py:643-683, query_functions.py:183-212) against the oracle."""
    from annchor_amd import Annchor

    Xs, Q = list(strings[::5]), list(strings[2::40])
    cfg = dict(n_anchors=8, n_neighbors=10, n_samples=700, p_work=0.3, random_seed=42, niters=2)
    ann = Annchor(np.array(Xs), "levenshtein", **cfg).fit()
    gi, gd = ann.query(np.array(Q), nn=5, p_work=0.3)
    P = om.PackedStrings(Xs)
    PQ = om.PackedStrings(Xs + Q)
    ora = O.OracleAnnchor(len(Xs), P.pairs, **cfg).fit()
    oi, od, info = O.query(ora, lambda IJ: PQ.pairs(np.stack([IJ[:, 0], IJ[:, 1] + len(Xs)], 1)), len(Q), nn=5, p_work=0.3)
    assert ann.query_evals == info["evals"]
    assert np.array_equal(gd, od)
    assert np.array_equal(gi, oi)


def test_query_digits_recall():
    """reference tests/test_examples.py:12-58 pattern: fit on a train split, query the rest;
    recall >= 0.99 against brute force at p_work = 0.2."""
    from annchor_amd import Annchor, compare_neighbor_graphs

    d = om.load_digits()
    X, M = d["X"], d["cost_matrix"]
    rs = np.random.RandomState(0)
    perm = rs.permutation(len(X))
    tr, te = perm[:1347], perm[1347:]
    ann = Annchor(X[tr], "wasserstein", func_kwargs={"cost_matrix": M}, n_anchors=25, n_neighbors=25, p_work=0.16).fit()
    gi, gd = ann.query(X[te], nn=15, p_work=0.2)
    H = om.Histograms(X, M)
    IJ = np.stack([np.repeat(te, len(tr)), np.tile(tr, len(te))], axis=1)
    full = H.pairs(IJ).reshape(len(te), len(tr))
    bd = np.sort(full, axis=1)[:, :15]
    err = compare_neighbor_graphs((np.zeros_like(bd, dtype=np.int64), bd), (gi, gd), 15)
    assert 1 - err / bd.size >= 0.99, err
    # reported neighbours are train-set members at their exact distances
    np.testing.assert_allclose(full[np.arange(len(te))[:, None], gi], gd, rtol=0, atol=1e-9)


def test_query_reference_digits_split():
    """The reference test's own query configuration (tests/test_examples.py:12-58) against the
    reference's own run of it (tests/golden/query_digits.npz, make_golden.py::gen_query): digits
    train_test_split(random_state=0), n_anchors=25, k=25, n_samples=5000, p_work=0.16; query
    nn=15, p_work=0.2.  Float tolerance: EMD values 1e-9 absolute."""
    from annchor_amd import Annchor, compare_neighbor_graphs

    G = np.load(os.path.join(GOLD, "query_digits.npz"))
    d = om.load_digits()
    X, M = d["X"], d["cost_matrix"]
    tr, te = G["idx_train"], G["idx_test"]
    ann = Annchor(X[tr], "wasserstein", func_kwargs={"cost_matrix": M}, n_anchors=25, n_neighbors=25, n_samples=5000,
                  p_work=0.16).fit()
    assert np.array_equal(ann.A, G["A"])
    np.testing.assert_allclose(ann.D, G["D"], rtol=0, atol=1e-12)
    gi, gd = ann.query(X[te], nn=15, p_work=0.2)
    assert gi.shape == G["q_e2e_idx"].shape
    # the reference's own answer: at most a handful of rows differ (float ties at the selection cut)
    assert compare_neighbor_graphs((G["q_e2e_idx"], G["q_e2e_dist"]), (gi, gd), 15) <= 5
    errs = sum(len(np.setdiff1d(G["truth_idx"][i], gi[i])) for i in range(len(te)))
    assert 1 - errs / (15.0 * len(te)) >= 0.99          # the reference test's criterion
    H = om.Histograms(np.concatenate([X[tr], X[te]]), M)
    IJ = np.stack([gi.ravel(), len(tr) + np.repeat(np.arange(len(te)), 15)], axis=1)
    np.testing.assert_allclose(H.pairs(IJ), gd.ravel(), rtol=0, atol=1e-9)


def test_query_reference_strings_split(strings):
    """Annchor.query against the reference's run on the strings split of gen_query (integer
    metric: every reported distance exact; error count vs brute force no worse than the reference
    run's, whose argpartition resolves tie groups arbitrarily), and bit-exact against the oracle."""
    from annchor_amd import Annchor, compare_neighbor_graphs

    G = np.load(os.path.join(GOLD, "query_strings.npz"))
    sub = strings[::4]
    trn = [s for t, s in enumerate(sub) if t % 5]
    qs = [s for t, s in enumerate(sub) if t % 5 == 0]
    cfg = dict(n_anchors=8, n_neighbors=10, n_samples=700, p_work=0.3, random_seed=42, niters=2)
    ann = Annchor(np.array(trn), "levenshtein", **cfg).fit()
    assert np.array_equal(ann.A, G["A"]) and np.array_equal(ann.D, G["D"])
    PQ = om.PackedStrings(trn + qs)
    qp = lambda IJ: PQ.pairs(np.stack([IJ[:, 0], IJ[:, 1] + len(trn)], 1))  # noqa: E731
    ora = O.OracleAnnchor(len(trn), om.PackedStrings(trn).pairs, **cfg).fit()
    nx = len(trn)
    dense = qp(np.stack([np.repeat(np.arange(nx), len(qs)), np.tile(np.arange(len(qs)), nx)], 1)).reshape(nx, len(qs)).T
    for tag, Q in (("q", qs), ("qlow", qs[:7])):
        nn, pw = int(G[tag + "_nn"]), float(G[tag + "_p_work"])
        gi, gd = ann.query(np.array(Q), nn=nn, p_work=pw)
        oi, od, info = O.query(ora, qp, len(Q), nn=nn, p_work=pw, apply_floor=True)
        assert np.array_equal(gd, od) and np.array_equal(gi, oi)
        assert ann.query_evals == info["evals"] == ora.n_anchors * len(Q) + len(G[tag + "_mapback"])
        order = np.argsort(dense[:len(Q)], axis=1, kind="stable")[:, :nn]
        truth = (order, np.take_along_axis(dense[:len(Q)], order, axis=1))
        e_gpu = compare_neighbor_graphs(truth, (gi, gd), nn)
        e_ref = compare_neighbor_graphs(truth, (G[tag + "_e2e_idx"], G[tag + "_e2e_dist"]), nn)
        assert e_gpu <= e_ref + 0.02 * len(Q) * nn + 2, (e_gpu, e_ref)   # no worse than the reference's run (tie order differs)


# ------------------------------------------------------------------ reference e2e tests not covered above
def test_fit_digits_reference_test_config():
    """reference tests/test_annchor.py:35-68 (n_anchors=25): anchors, anchor distances and evaluation count
    of the reference's own run; its bar of < 10 errors."""
    from annchor_amd import Annchor, compare_neighbor_graphs

    d = om.load_digits()
    G = np.load(os.path.join(GOLD, "digits_full.npz"))
    ann = Annchor(d["X"], "wasserstein", func_kwargs={"cost_matrix": d["cost_matrix"]}, n_anchors=25,
                  n_neighbors=25, n_samples=5000, p_work=0.16, random_seed=42).fit()
    assert np.array_equal(ann.A, G["test_A"])
    np.testing.assert_allclose(ann.D, G["test_D"], rtol=0, atol=1e-12)
    assert ann.evals == int(G["test_evals"])
    assert compare_neighbor_graphs(d["neighbor_graph"], ann.neighbor_graph, 25) < 10


def test_fit_graph_sp_python_metric():
    """reference tests/test_annchor.py:105-145: an arbitrary Python callable over node ids (shortest-path
    length).  The callable runs on the host, everything else on the GPU; anchors, anchor distances,
    evaluation count equal the reference's own run (tests/golden/graph_sp.npz), the graph the restatement's."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    from annchor_amd import Annchor, compare_neighbor_graphs

    G = np.load(os.path.join(GOLD, "graph_sp.npz"))
    e, w = G["edges"].astype(np.int64), G["weights"]
    n = int(e.max()) + 1
    SP = dijkstra(coo_matrix((w, (e[:, 0], e[:, 1])), shape=(n, n)).tocsr(), directed=False)
    assert np.isclose(SP[2, 5], 0.1487023176704947) and np.isclose(SP[300, 701], 1.2342577780314983)

    def sp_dist(i, j):
        return SP[i, j]

    ann = Annchor(G["X"].astype(np.int64), sp_dist, n_anchors=20, n_neighbors=15, random_seed=42,
                  n_samples=5000, p_work=0.15).fit()
    assert np.array_equal(ann.A, G["A"])
    assert np.array_equal(ann.D, G["D"])
    assert ann.evals == int(G["evals"]) and ann.n_pairs == int(G["npairs"])
    X = G["X"].astype(np.int64)
    ora = O.OracleAnnchor(len(X), lambda IJ: SP[X[IJ[:, 0]], X[IJ[:, 1]]], n_anchors=20, n_neighbors=15,
                          n_samples=5000, p_work=0.15, random_seed=42).fit()
    assert np.array_equal(ann.neighbor_graph[1], ora.neighbor_graph[1])
    assert np.array_equal(ann.neighbor_graph[0], ora.neighbor_graph[0])
    err = compare_neighbor_graphs((G["ng_idx"].astype(np.int64), G["ng_dist"]), ann.neighbor_graph, 15)
    assert err <= int(G["errors"]) < 10


def test_fit_strings_with_duplicates_and_empty_strings_stagewise():
    """Collisions: a third of the strings are exact copies of others (distance 0 between distinct points,
    whole tie groups in every order statistic), three are empty, lengths are ragged (0..90) -- every stage
    equal to the oracle's, which follows the reference's tie rules (np.argmax first index, stable sorts,
    partition order statistics)."""
    from annchor_amd import Annchor

    rng = np.random.default_rng(31)
    base = ["".join(rng.choice(list("abc"), rng.integers(1, 90))) for _ in range(220)]
    Xs = base + [base[i] for i in rng.integers(0, 220, 110)] + ["", "", ""]
    order = rng.permutation(len(Xs))
    Xs = [Xs[i] for i in order]
    cfg = dict(n_anchors=7, n_neighbors=8, n_samples=600, p_work=0.35, random_seed=5, niters=2)
    ann = Annchor(np.array(Xs, dtype=object), "levenshtein", **cfg)
    P = om.PackedStrings(Xs)
    ora = _staged_compare(ann, lambda tr: O.OracleAnnchor(len(Xs), P.pairs, trace=tr, **cfg))
    assert (ora.neighbor_graph[1][:, 1] == 0).sum() >= 100   # the copies found each other


def test_fit_euclid_integer_grid_with_duplicates_stagewise():
    """Euclidean on a small integer grid (float64): many exactly equal distances and duplicated points, so the
    order statistics, the arg-max of the picker and the candidate cuts all sit inside tie groups.  Integer
    coordinates make the device's and NumPy's distances bit-equal (sums of squares are exact), so the stages
    are compared exactly like an integer metric's."""
    from annchor_amd import Annchor

    rng = np.random.default_rng(9)
    X = rng.integers(0, 6, (520, 3)).astype(np.float64)
    X[400:] = X[rng.integers(0, 400, 120)]          # exact copies
    cfg = dict(n_anchors=9, n_neighbors=7, n_samples=500, p_work=0.3, random_seed=11, niters=2)
    ann = Annchor(X, "euclidean", **cfg)
    _staged_compare(ann, lambda tr: O.OracleAnnchor(len(X), lambda IJ: om.euclidean_pairs(X, IJ), trace=tr, **cfg),
                    float_metric=True)
    idx, dist = ann.neighbor_graph
    assert np.all(dist[400:, 1] == 0)               # every copy has its original (or another copy) at distance 0
