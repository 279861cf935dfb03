"""The shared Levenshtein column (`csrc/levcol.h`) inside each kernel that uses it -- k_lev_f, k_lev_p2, k_lev_a2, k_lev_ap and
its rescue form -- at the smallest shapes at which a wrong carry between lanes shows.  Exact integers, compared with the
oracle by `array_equal`.

Data sets are named by their longest string, which fixes k_lev_f's slots: 32 symbols = 64 one-lane slots (every lane a first
lane), 64 = 32 two-lane slots, 96 = 21 three-lane slots with lane 63 idle, 512 = 4 x 16 lanes with no idle lane between
slots, 594 = 3 x 19 lanes.  Consecutive list positions share a wave, and the lists alternate, slot by slot, pairs that
saturate the horizontal deltas ("a" * L against "b" * L, and against ""), identical strings (distance 0) and pairs one symbol
short of a word multiple: a carry leaking from a slot's last lane into the next slot's first lane changes a distance.
One more data set, ODD_SHORT, gives the forward / backward kernels an odd number of short strings (and k_lev_p2 an odd
number of short-pattern pairs): the last packed wave then holds a single pair (`_data`).

The max-min pick of the round-by-round launches (k_lev_a2, k_lev_f, k_lev_r) and of every other route: test_anchor_pick_gpu.py."""
import numpy as np
import pytest

from oracle import metrics as om

pytestmark = pytest.mark.gpu

LONGEST = [32, 64, 96, 512, 594]


def _dataset(L, seed=5):
    rng = np.random.default_rng(seed + L)
    sym = list("abcd")
    r1 = "".join(rng.choice(sym, L))
    r2 = "".join(rng.choice(sym, L - 1))
    t = list(r2)
    for p in sorted(rng.integers(0, L - 1, 3)):
        t[p] = "a" if t[p] != "a" else "b"
    r3 = "".join(rng.choice(sym, int(rng.integers(1, L + 1))))
    base = ["a" * L, r1, "b" * L, r1, "", r2, "a" * (L - 1), "".join(t), "b" * (L - 1), r3]
    return base * 3


ODD_SHORT = "594-odd-short"


def _data(key):
    """`_dataset(L)` for a length; for ODD_SHORT the 594-symbol data plus as many strings of 512 symbols (16 words: the longest of
    the short class) as it takes to make the number of strings of <= 512 symbols odd.  The half-chain kernels pack two short
    strings (k_lev_a2, k_lev_ap) or two short-pattern pairs (k_lev_p2) into a wave: the odd one out has a wave to itself, its
    second pair slot empty."""
    if key != ODD_SHORT:
        return _dataset(key)
    X = _dataset(594)
    rng = np.random.default_rng(11)
    while sum(len(s) <= 512 for s in X) % 2 == 0:
        X.append("".join(rng.choice(list("abcd"), 512)))
    assert sum(len(s) <= 512 for s in X) % 2 == 1 and len(X) == 31
    return X


# by position in `base`: saturated, identical, against the empty string, one symbol short of a word multiple, ...
CYCLE = [(0, 2), (1, 3), (0, 4), (5, 7), (2, 0), (3, 3), (6, 8), (9, 1)]


def _pair_list(n):
    t = np.arange(n)
    return np.array(CYCLE)[t % 8] + 10 * ((t // 8) % 3)[:, None]


def _engine(X):
    from annchor_amd import _native
    from annchor_amd.distances import levenshtein

    eng = _native.Engine(0)
    levenshtein.bind(eng, X)
    return eng


@pytest.mark.parametrize("L", LONGEST)
@pytest.mark.parametrize("p2_max", ["0", "1000000"])
def test_pair_list_kernels(L, p2_max, monkeypatch):
    """k_lev_f (ANNCHOR_LEV_P2_MAX=0) and k_lev_p2 (forced for every list of 64 pairs or more) on lists of 7, 64 and 300."""
    monkeypatch.setenv("ANNCHOR_LEV_P2_MAX", p2_max)
    X = _dataset(L)
    P = om.PackedStrings(X)
    eng = _engine(X)
    for n in (7, 64, 300):
        IJ = _pair_list(n)
        want = P.pairs(IJ)
        assert want[1] == 0 and want[0] == L and want[2] == L   # the kinds are what they claim to be
        assert np.array_equal(eng.metric_pairs(IJ), want), (L, p2_max, n)
    eng.close()


def test_pair_list_both_slot_classes(monkeypatch):
    """4100 pairs of the 512- and 594-symbol data: k_lev_f classifies the list and runs 4 x 16-lane and 3 x 19-lane slots in one
    launch."""
    monkeypatch.setenv("ANNCHOR_LEV_P2_MAX", "0")
    X = _dataset(512) + _dataset(594)
    rng = np.random.default_rng(3)
    IJ = rng.integers(0, len(X), (4100, 2))
    fixed = np.concatenate([_pair_list(300), _pair_list(300) + 30])   # the alternating kinds within each data set
    IJ[:600] = fixed
    eng = _engine(X)
    assert np.array_equal(eng.metric_pairs(IJ), om.PackedStrings(X).pairs(IJ))
    eng.close()


def _rows(P, anchors):
    nx = P.nx
    return np.stack([P.pairs(np.stack([np.full(nx, a), np.arange(nx)], axis=1)) for a in anchors], axis=1)


def test_pair_list_odd_short_class(monkeypatch):
    """k_lev_p2 on a list whose packed class is odd: 65 pairs, the 33 at positions 0, 2, .. 64 with a pattern of <= 16 words
    (two to a wave; the 33rd alone in its wave), the 32 at positions 1, 3, .. 63 with two longer strings (a wave each)."""
    monkeypatch.setenv("ANNCHOR_LEV_P2_MAX", "1000000")
    X = _data(ODD_SHORT)
    # long against empty, the 92-symbol string against a long one, empty against empty, 512 against 593 symbols, identical, ...
    short = [(0, 4), (9, 1), (4, 14), (30, 5), (19, 9), (30, 30), (24, 2), (7, 30)]
    # saturated, identical, one symbol short of a word multiple with three substitutions, 594 against 593 symbols, ...
    long_ = [(0, 2), (1, 3), (5, 7), (2, 0), (3, 3), (6, 8), (10, 22), (21, 15)]
    IJ = np.empty((65, 2), dtype=np.int64)
    IJ[0::2] = [short[r % 8] for r in range(33)]
    IJ[1::2] = [long_[r % 8] for r in range(32)]
    lens = np.array([len(s) for s in X])
    words = (np.minimum(lens[IJ[:, 0]], lens[IJ[:, 1]]) + 31) // 32   # of a pair's shorter string: k_lev_classify's rule
    assert np.count_nonzero(words <= 16) == 33 and np.count_nonzero(words > 16) == 32
    eng = _engine(X)
    assert np.array_equal(eng.metric_pairs(IJ), om.PackedStrings(X).pairs(IJ))
    eng.close()


@pytest.mark.parametrize("L", LONGEST + [ODD_SHORT])
def test_anchor_round_kernel(L):
    """k_lev_a2: one-to-all rounds for chosen anchors -- the saturating strings, the empty one, a random one."""
    from annchor_amd import _native

    X = _data(L)
    anchors = [0, 2, 4, 1, 17, 26]
    eng = _engine(X)
    eng.pick_anchors_selected(anchors)
    got = eng.download(_native.F_D).reshape(len(X), len(anchors))
    assert np.array_equal(got, _rows(om.PackedStrings(X), anchors))
    eng.close()


@pytest.mark.parametrize("L", LONGEST + [ODD_SHORT])
@pytest.mark.parametrize("mode", ["persistent", "rescue"])
def test_anchor_rounds_one_launch(L, mode, monkeypatch):
    """k_lev_ap and its rescue form (forced by a zero time limit): the max-min picker's rounds, A and D against the oracle."""
    from annchor_amd import _native

    monkeypatch.delenv("ANNCHOR_LEV_PERSIST", raising=False)
    if mode == "rescue":
        monkeypatch.setenv("ANNCHOR_LEV_PERSIST_TIMEOUT_US", "0")
    else:
        monkeypatch.delenv("ANNCHOR_LEV_PERSIST_TIMEOUT_US", raising=False)
    X = _data(L)
    P = om.PackedStrings(X)
    nx, na, first = len(X), 6, 5
    D = np.zeros((na, nx))
    A = np.zeros(na, dtype=np.int64)
    ix = first
    for i in range(na):   # pickers.py:44-50 with the first index given
        A[i] = ix
        D[i] = P.pairs(np.stack([np.full(nx, ix), np.arange(nx)], axis=1))
        ix = int(np.argmax(D[:1].min(axis=0))) if i == 0 else int(np.argmax(D[1:i + 1].min(axis=0)))
    eng = _engine(X)
    eng.pick_anchors_maxmin(na, first)
    assert np.array_equal(eng.download(_native.F_A), A), (L, mode)
    assert np.array_equal(eng.download(_native.F_D).reshape(nx, na), D.T), (L, mode)
    eng.close()
