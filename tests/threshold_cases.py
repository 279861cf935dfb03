"""EDR and LCSS on the host, the dim-aware DTW loop, and the data sets of the threshold measures' tests.

Definitions (annchor_amd.distances.EDR, LCSS).  A series is 1 .. L points of `dim` coordinates, dim in 1 .. 4.  All arithmetic is
float64; float32 input widens exactly.  eps is a finite float64 >= 0.

    match(p, q) iff fabs(p[k] - q[k]) <= eps for every k = 0 .. dim-1      (each subtraction rounded on its own)

    E(-1,-1) = 0,  E(i,-1) = i + 1,  E(-1,j) = j + 1
    E(i,j)   = min( E(i-1,j-1) + (match(x[i], y[j]) ? 0.0 : 1.0),  E(i-1,j) + 1.0,  E(i,j-1) + 1.0 )
    edr(x,y) = E(n-1,m-1)                       normalize=False
             = E(n-1,m-1) / (double)max(n,m)    normalize=True

    L(-1,-1) = L(i,-1) = L(-1,j) = 0
    L(i,j)   = L(i-1,j-1) + 1.0          if match(x[i], y[j]) and (delta is None or |i - j| <= delta)
             = max(L(i-1,j), L(i,j-1))   otherwise
    lcss(x,y) = 1.0 - L(n-1,m-1) / (double)min(n,m)

Every cell is a small integer that float64 holds exactly, so every evaluation order gives the same bits: the loops here (which
never swap the members), seqdp_cases.pairs_host and seqdp_cases.lanes with the measures below, and the kernel must agree bit for
bit.  The measures' finish() sees no lengths, so the final division is applied outside, by `edr_pairs_host` and
`lcss_pairs_host`."""
import numpy as np

import seqdp_cases as sc
from pool_cases import FIT_CFG, all_ordered_pairs   # noqa: F401  (the tests' builders)
from seqdp_cases import as_curve


# --------------------------------------------------------------------------------------------------------- the loops
def _match(p, q, eps):
    for k in range(len(p)):
        if not abs(p[k] - q[k]) <= eps:
            return False
    return True


def edr_count_loop(x, y, eps):
    """E(n-1, m-1), cell by cell."""
    x, y = as_curve(x), as_curve(y)
    n, m = len(x), len(y)
    E = np.zeros((n + 1, m + 1))
    E[:, 0] = np.arange(n + 1)
    E[0, :] = np.arange(m + 1)
    for i in range(n):
        for j in range(m):
            E[i + 1, j + 1] = min(E[i, j] + (0.0 if _match(x[i], y[j], eps) else 1.0), E[i, j + 1] + 1.0, E[i + 1, j] + 1.0)
    return E[n, m]


def edr_loop(x, y, eps, normalize=False):
    v = np.float64(edr_count_loop(x, y, eps))
    return v / np.float64(max(len(x), len(y))) if normalize else v


def lcss_count_loop(x, y, eps, delta=None):
    """L(n-1, m-1), cell by cell."""
    x, y = as_curve(x), as_curve(y)
    n, m = len(x), len(y)
    L = np.zeros((n + 1, m + 1))
    for i in range(n):
        for j in range(m):
            if _match(x[i], y[j], eps) and (delta is None or abs(i - j) <= delta):
                L[i + 1, j + 1] = L[i, j] + 1.0
            else:
                L[i + 1, j + 1] = max(L[i, j + 1], L[i + 1, j])
    return L[n, m]


def lcss_loop(x, y, eps, delta=None):
    return np.float64(1.0) - np.float64(lcss_count_loop(x, y, eps, delta)) / np.float64(min(len(x), len(y)))


def dtw_loop(x, y, window=None):
    """DTW on curves of any dim, cell by cell: dtw_cases.dtw_loop with Frechet's c(i, j)."""
    x, y = as_curve(x), as_curve(y)
    n, m, dim = len(x), len(y), x.shape[1]
    assert y.shape[1] == dim
    w = None if window is None else max(int(window), abs(n - m))
    D = np.full((n + 1, m + 1), np.inf)
    D[0, 0] = 0.0
    for i in range(n):
        for j in range(m):
            if w is not None and abs(i - j) > w:
                continue
            t = x[i, 0] - y[j, 0]
            c = t * t
            for k in range(1, dim):
                t = x[i, k] - y[j, k]
                c = c + t * t
            D[i + 1, j + 1] = c + min(D[i, j + 1], D[i + 1, j], D[i, j])
    return np.sqrt(D[n, m])


# ------------------------------------------------------------------------------------------------------- the measures
def _match_v(x, y, eps):
    hit = np.abs(x[..., 0] - y[..., 0]) <= eps
    for k in range(1, x.shape[-1]):
        hit = hit & (np.abs(x[..., k] - y[..., k]) <= eps)
    return hit


class Edr(sc._Measure):
    def __init__(self, eps):
        self.eps = np.float64(eps)

    def edge(self, members):
        return np.concatenate([np.arange(1, len(s) + 1, dtype=np.float64) for s in members])

    def cell(self, x, xp, y, yp, gx, gy, e, dg, up, left):
        return np.minimum(np.minimum(dg + np.where(_match_v(x, y, self.eps), 0.0, 1.0), up + 1.0), left + 1.0)


class Lcss(sc._Measure):
    def __init__(self, eps, delta=None):
        self.eps, self.delta = np.float64(eps), delta

    def edge(self, members):
        return np.zeros(sum(len(s) for s in members))

    def cell(self, x, xp, y, yp, gx, gy, e, dg, up, left):
        hit = _match_v(x, y, self.eps)
        if self.delta is not None:
            hit = hit & (np.abs(e) <= self.delta)
        return np.where(hit, dg + 1.0, np.maximum(up, left))


def _lens(series, IJ):
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    L = np.array([len(s) for s in series], dtype=np.int64)
    return L[IJ[:, 0]], L[IJ[:, 1]]


def edr_finish(count, series, IJ, normalize):
    n, m = _lens(series, IJ)
    return count / np.maximum(n, m).astype(np.float64) if normalize else count


def lcss_finish(count, series, IJ):
    n, m = _lens(series, IJ)
    return 1.0 - count / np.minimum(n, m).astype(np.float64)


def edr_pairs_host(series, IJ, eps, normalize=False):
    return edr_finish(sc.pairs_host(series, IJ, Edr(eps)), series, IJ, normalize)


def lcss_pairs_host(series, IJ, eps, delta=None):
    return lcss_finish(sc.pairs_host(series, IJ, Lcss(eps, delta)), series, IJ)


def edr_lanes(series, IJ, eps, normalize, R, G):
    return edr_finish(sc.lanes(series, IJ, Edr(eps), R, G), series, IJ, normalize)


def lcss_lanes(series, IJ, eps, delta, R, G):
    return lcss_finish(sc.lanes(series, IJ, Lcss(eps, delta), R, G), series, IJ)


def dtw_pairs_host(series, IJ, window=None):
    return sc.dtw_pairs_host(series, IJ, window)


# ------------------------------------------------------------------------------------------------------------- data
# Bounded data: coordinates from the grid {0, 0.5, ..., 2.0}, so that differences of exactly eps occur, with a threshold per dim
# at which 20 % .. 80 % of all point pairs match.  Of the 25 ordered value pairs, 5 are at difference 0, 8 at 0.5, 6 at 1.0, 4 at
# 1.5 and 2 at 2.0: a coordinate matches with probability 13/25 at eps 0.5, 19/25 at 1.0 and 23/25 at 1.5, and a point with that
# probability to the power dim: 0.52 at (dim 1, eps 0.5), 0.58 at (2, 1.0), 0.44 at (3, 1.0), 0.33 at (4, 1.0).
GRID_EPS = {1: 0.5, 2: 1.0, 3: 1.0, 4: 1.0}


def grid_series(lengths, dim, seed, dtype=np.float64):
    """One series per length, coordinates drawn from {0, 0.5, 1.0, 1.5, 2.0}; dim 1: flat members."""
    rng = np.random.default_rng(seed)
    X = [(rng.integers(0, 5, size=(int(L), dim)) * 0.5).astype(dtype) for L in lengths]
    return [x[:, 0] for x in X] if dim == 1 else X


def match_share(X, eps, pairs=2000, seed=0):
    """The share of matching point pairs between random members of X."""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([as_curve(x) for x in X], axis=0)
    a, b = pool[rng.integers(0, len(pool), pairs)], pool[rng.integers(0, len(pool), pairs)]
    return float(np.mean(_match_v(a, b, np.float64(eps))))


def integer_sequences(count=60, lo=1, hi=40, symbols=4, seed=7):
    """Random sequences over `symbols` integers, lengths lo .. hi."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, symbols, size=int(rng.integers(lo, hi + 1))).astype(np.float64) for _ in range(count)]


FIT_EPS = 0.3


def fit_series():
    """The fit tests' data for EDR and LCSS: seqdp_cases.clustered_curves(240, 20, 60, 2, seed=31) with each curve's cluster offset
    3.0 * (s % 6) subtracted again from coordinate 0 (with the offsets in place nothing matches between clusters and LCSS
    saturates at 1.0)."""
    X = sc.clustered_curves(240, 20, 60, 2, seed=31)
    for s, x in enumerate(X):
        x[:, 0] -= 3.0 * (s % sc.SHAPES)
    return X


def query_series():
    """20 held-out members of 30..70 points, shifted like fit_series."""
    Q = sc.clustered_curves(20, 30, 70, 2, seed=34)
    for s, x in enumerate(Q):
        x[:, 0] -= 3.0 * (s % sc.SHAPES)
    return Q


FIT_PARAMS = {
    "edr": [{"eps": FIT_EPS}, {"eps": FIT_EPS, "normalize": True}],
    "lcss": [{"eps": FIT_EPS}, {"eps": FIT_EPS, "delta": 5}],
}
HOSTS = {"edr": edr_pairs_host, "lcss": lcss_pairs_host, "dtw": dtw_pairs_host}
