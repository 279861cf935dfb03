"""The Jaccard distance on the host, and the data sets of the Jaccard tests.

Definition (annchor_amd.distances.Jaccard).  For two finite sets A and B of integers

    i = |A n B|      u = |A| + |B| - i
    jaccard(A, B) = 0.0 if u == 0 (both empty),   (double)(u - i) / (double)u otherwise

one IEEE float64 division of two exact integers.  `jaccard_loop` is the definition: a two-pointer merge over the sorted distinct
tokens, then the division.  `jaccard_pairs_host` counts the intersections of a whole pair list on 0/1 incidence rows;
test_jaccard_host.py checks the two against each other and against scipy bit for bit, and the kernels must equal them."""
import numpy as np

from pool_cases import FIT_CFG, all_ordered_pairs   # noqa: F401

MAX_TOKENS = 65536
MAX_BITS = 8192
# csrc/jaccard.hip: lanes per pair by the data set's largest member (tokens form) and by the uint4 per row (bits form)
TOKEN_GROUPS = [(4, 64), (16, 1024), (64, MAX_TOKENS)]


def token_group(longest):
    """G of the k_jaccard_tokens instantiation that a data set whose largest member has `longest` tokens runs."""
    return next(G for G, limit in TOKEN_GROUPS if longest <= limit)


def bits_group(nbits):
    """G of the k_jaccard_bits instantiation at `nbits`: W / 4 <= 4 -> 4, <= 16 -> 16, else 64."""
    W = (-(-nbits // 32) + 3) // 4 * 4
    return 4 if W // 4 <= 4 else 16 if W // 4 <= 16 else 64


def as_tokens(x):
    """The sorted distinct tokens of a member, int64: a bool row gives its True positions."""
    if isinstance(x, (set, frozenset, list, tuple)):
        x = np.array(sorted(x), dtype=np.int64)
    x = np.asarray(x)
    if x.dtype == np.bool_:
        return np.flatnonzero(x).astype(np.int64)
    assert x.dtype.kind in "iu" and x.ndim == 1
    return np.unique(x.astype(np.int64))


def jaccard_loop(a, b):
    """The reference: a plain two-pointer merge, then the definition."""
    a, b = as_tokens(a).tolist(), as_tokens(b).tolist()
    p = q = common = 0
    while p < len(a) and q < len(b):
        if a[p] == b[q]:
            common += 1
            p += 1
            q += 1
        elif a[p] < b[q]:
            p += 1
        else:
            q += 1
    u = len(a) + len(b) - common
    if u == 0:
        return 0.0
    return float(np.float64(u - common) / np.float64(u))


CHUNK_CELLS = 1 << 24   # cells of the incidence rows held at a time


def jaccard_pairs_host(X, IJ):
    """jaccard(X[i], X[j]) for every row (i, j) of IJ -> float64 [len(IJ)]: the vectorised twin of jaccard_loop."""
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    S = [as_tokens(x) for x in X]
    sizes = np.array([len(s) for s in S], dtype=np.int64)
    universe = np.unique(np.concatenate(S)) if sizes.sum() else np.zeros(0, dtype=np.int64)
    used = np.unique(IJ)
    row_of = np.full(len(S), -1, dtype=np.int64)
    row_of[used] = np.arange(len(used))
    B = np.zeros((len(used), max(1, len(universe))), dtype=np.uint8)
    for r, s in enumerate(used):
        B[r, np.searchsorted(universe, S[s])] = 1
    common = np.zeros(len(IJ), dtype=np.int64)
    step = max(1, CHUNK_CELLS // B.shape[1])
    for t in range(0, len(IJ), step):
        bi, bj = B[row_of[IJ[t:t + step, 0]]], B[row_of[IJ[t:t + step, 1]]]
        common[t:t + step] = (bi & bj).sum(axis=1, dtype=np.int64)
    u = sizes[IJ[:, 0]] + sizes[IJ[:, 1]] - common
    out = np.zeros(len(IJ), dtype=np.float64)
    nz = u > 0
    out[nz] = (u[nz] - common[nz]).astype(np.float64) / u[nz].astype(np.float64)
    return out


# ------------------------------------------------------------------------------------------------------------- data
def window_sets(nx, universe, seed, lo=8, hi=120, keep=0.7, noise=6):
    """Member s: a centre c and a half width w in lo .. hi; each token of the window (c + [-w .. w]) mod universe is kept
    with probability `keep`; up to `noise` random tokens are added.  Unsorted int64 arrays."""
    rng = np.random.default_rng(seed)
    X = []
    for _ in range(nx):
        c, w = int(rng.integers(0, universe)), int(rng.integers(lo, hi + 1))
        win = (c + np.arange(-w, w + 1)) % universe
        x = np.concatenate([win[rng.random(len(win)) < keep], rng.integers(0, universe, int(rng.integers(0, noise + 1)))])
        X.append(x[rng.permutation(len(x))].astype(np.int64))
    return X


def proto_sets(nx, nproto, universe, seed):
    """`nproto` prototypes, each a random 20..200-subset of the universe joined with a prefix of a common core of 150 tokens (at
    least 10 of them: the prefixes' lengths spread the distances between members of different prototypes); a member drops
    5..45 % of its prototype's tokens -- never one of the core's first 5 -- and adds as many random ones.  Every member holds the core's first 5 tokens, so no two members are disjoint."""
    rng = np.random.default_rng(seed)
    core = rng.choice(universe, 150, replace=False)
    protos = []
    for _ in range(nproto):
        body = rng.choice(universe, int(rng.integers(20, 201)), replace=False)
        protos.append(np.union1d(body, core[:int(rng.integers(10, 151))]))
    X = []
    for s in range(nx):
        p = protos[s % nproto]
        free = np.setdiff1d(p, core[:5])
        ndrop = int(len(p) * rng.uniform(0.05, 0.45))
        dropped = rng.choice(free, min(ndrop, len(free)), replace=False)
        x = np.concatenate([np.setdiff1d(p, dropped), rng.integers(0, universe, len(dropped))])
        X.append(x[rng.permutation(len(x))].astype(np.int64))
    return X


def indicator_matrix(X, nbits):
    """Token members with tokens in 0 .. nbits-1 -> bool [nx, nbits]."""
    M = np.zeros((len(X), nbits), dtype=bool)
    for s, x in enumerate(X):
        M[s, as_tokens(x)] = True
    return M


def fingerprints(nx, nbits, density, seed):
    """bool [nx, nbits], every bit set with probability `density`."""
    return np.random.default_rng(seed).random((nx, nbits)) < density


def one_of_each_size(sizes, universe, seed):
    """One member per size: a random subset of 0 .. universe-1, unsorted.  Neighbouring members overlap heavily when the sizes
    come near the universe."""
    rng = np.random.default_rng(seed)
    return [rng.permutation(universe)[:L].astype(np.int64) for L in sizes]


def group_sizes(G):
    return sorted({0, 1, G - 1, G, G + 1, 2 * G, 64 * G - 1, 64 * G, 64 * G + 1})


def boundary_sizes():
    """The group sizes of every G, ascending."""
    return sorted({L for G, _ in TOKEN_GROUPS for L in group_sizes(G)})


def group_limit(G):
    """The largest member of a data set that still runs the instantiation G."""
    return dict(TOKEN_GROUPS)[G]


def fit_sets():
    """The fit tests' data: 240 window sets over 600 tokens; 31.8 % of the pairs are disjoint, at exactly 1.0."""
    return window_sets(240, 600, seed=1)


def fit_protos():
    """The second fit data set, as a bool matrix [240, 1500]: no disjoint pair."""
    return indicator_matrix(proto_sets(240, 12, 1500, 1), 1500)


def query_rows():
    """X bool [240, 600] and Q bool [20, 600] from another seed."""
    return indicator_matrix(fit_sets(), 600), indicator_matrix(window_sets(20, 600, seed=2), 600)


def query_lists():
    """X: the fit data as token lists; Q: 20 window sets over 0 .. 699, so they hold tokens (600 .. 699) that X never saw."""
    Q = window_sets(20, 700, seed=5)
    assert max(int(q.max()) for q in Q) >= 600
    return fit_sets(), Q


def brute_sets():
    """200 members of more than 20 different sizes: proto sets over 1200 tokens."""
    return proto_sets(200, 10, 1200, seed=3)
