"""Move-Split-Merge (MSM) and the time warp edit distance (TWE) on the host, lane-by-lane restatements of the kernel's schedule,
and the data sets of their tests.

Definitions (annchor_amd.distances.MSM and .TWE).  All arithmetic is float64, every subtraction, product and addition rounded on
its own; float32 input widens exactly.  Indices are 0-based; x has n >= 1 points, y has m >= 1.  Both measures share one boundary:
T(-1, -1) = 0, T(i, -1) = T(-1, j) = +inf, and the virtual previous points x[-1] and y[-1] are the origin.

    MSM, univariate, c finite and > 0:
        C(v, a, b) = c                              if a <= v <= b or a >= v >= b
                   = c + min(|v - a|, |v - b|)      otherwise
        M(i, j) = min( M(i-1, j-1) + |x[i] - y[j]|,   M(i-1, j) + C(x[i], x[i-1], y[j]),   M(i, j-1) + C(y[j], x[i], y[j-1]) )
        msm(x, y) = M(n-1, m-1)

    TWE, dim 1 .. 4, nu and lam finite and >= 0, nl = nu + lam and nu2 = 2.0 * nu formed once, dist ERP's dist (seqdp_cases._dist):
        dx(i) = dist(x[i], x[i-1]) + nl        dy(j) = dist(y[j], y[j-1]) + nl
        T(i, j) = min( T(i-1, j-1) + ((dist(x[i], y[j]) + dist(x[i-1], y[j-1])) + nu2 * (double)|i - j|),
                       T(i-1, j) + dx(i),   T(i, j-1) + dy(j) )
        twe(x, y) = T(n-1, m-1)

Every cell is the min of three sums of fixed operands, so every evaluation order gives the same bits: `*_loop` (the plain double
loop, which never swaps the members), `*_pairs_host` (anti-diagonals, many pairs at once, the SHORTER member on the vectorised
axis) and `*_lanes` (the kernel's schedule, the LONGER member on the lanes) must agree bit for bit, and so must the kernel.
The last two are seqdp_cases' shared sweep and lane model with the Msm and Twe measures."""
import numpy as np

from pool_cases import FIT_CFG, all_ordered_pairs   # noqa: F401
from seqdp_cases import (DIMS, _dist, as_curve, clustered_curves, msm_lanes, msm_pairs_host, one_of_each_length,   # noqa: F401
                         twe_lanes, twe_pairs_host, univariate)

INF = float("inf")


# ------------------------------------------------------------------------------------------------------- the double loops
def msm_cost(v, a, b, c):
    """C(v, a, b) of the definition, on Python floats."""
    if a <= v <= b or a >= v >= b:
        return c
    return c + min(abs(v - a), abs(v - b))


def msm_loop(x, y, c=1.0):
    """The definition, cell by cell."""
    x, y = as_curve(x), as_curve(y)
    assert x.shape[1] == 1 and y.shape[1] == 1
    x, y, c = x[:, 0].tolist(), y[:, 0].tolist(), float(c)
    m = len(y)
    prev = [0.0] + [INF] * m                     # row -1: M(-1, -1), M(-1, 0), ...
    for i, xi in enumerate(x):
        xm = x[i - 1] if i > 0 else 0.0
        cur = [INF] * (m + 1)
        for j, yj in enumerate(y):
            ym = y[j - 1] if j > 0 else 0.0
            cur[j + 1] = min(prev[j] + abs(xi - yj), prev[j + 1] + msm_cost(xi, xm, yj, c), cur[j] + msm_cost(yj, xi, ym, c))
        prev = cur
    return np.float64(prev[m])


def msm_textbook(x, y, c=1.0):
    """Stefan, Athitsos & Das' form: M(0, 0) = |x[0] - y[0]|, a first column and row of running sums of C, no virtual points."""
    x, y, c = np.asarray(x, dtype=np.float64).tolist(), np.asarray(y, dtype=np.float64).tolist(), float(c)
    n, m = len(x), len(y)
    D = [[0.0] * m for _ in range(n)]
    D[0][0] = abs(x[0] - y[0])
    for i in range(1, n):
        D[i][0] = D[i - 1][0] + msm_cost(x[i], x[i - 1], y[0], c)
    for j in range(1, m):
        D[0][j] = D[0][j - 1] + msm_cost(y[j], x[0], y[j - 1], c)
    for i in range(1, n):
        for j in range(1, m):
            D[i][j] = min(D[i - 1][j - 1] + abs(x[i] - y[j]), D[i - 1][j] + msm_cost(x[i], x[i - 1], y[j], c),
                          D[i][j - 1] + msm_cost(y[j], x[i], y[j - 1], c))
    return np.float64(D[n - 1][m - 1])


def twe_loop(x, y, nu=0.001, lam=1.0):
    """The definition, cell by cell (the point distances are evaluated elementwise beforehand)."""
    x, y = as_curve(x), as_curve(y)
    n, m = len(x), len(y)
    assert y.shape[1] == x.shape[1]
    nl, nu2 = float(nu) + float(lam), 2.0 * float(nu)
    xp = np.concatenate([np.zeros((1, x.shape[1])), x[:-1]])       # x[i - 1], the origin before x[0]
    yp = np.concatenate([np.zeros((1, y.shape[1])), y[:-1]])
    dx, dy = _dist(x, xp).tolist(), _dist(y, yp).tolist()
    prev = [0.0] + [INF] * m
    for i in range(n):
        here = _dist(x[i][None, :], y).tolist()                    # dist(x[i], y[j])
        before = _dist(xp[i][None, :], yp).tolist()                # dist(x[i-1], y[j-1])
        dxi = dx[i] + nl
        cur = [INF] * (m + 1)
        for j in range(m):
            cur[j + 1] = min(prev[j] + ((here[j] + before[j]) + nu2 * float(abs(i - j))), prev[j + 1] + dxi, cur[j] + (dy[j] + nl))
        prev = cur
    return np.float64(prev[m])


# ------------------------------------------------------------------------------------------------------------- data
def tie_series(kind, lengths, seed):
    """Series on which MSM's `between` test meets its ties in most cells: "ints", values drawn from {-1, 0, 1, 2}; "grid", from three
    float32 levels that are no dyadic fractions (float32); "walk", non-dyadic random walks, where the min is decided in the last
    bits."""
    rng = np.random.default_rng(seed)
    if kind == "ints":
        return [rng.integers(-1, 3, size=int(L)).astype(np.float64) for L in lengths]
    if kind == "grid":
        levels = np.array([0.1, 0.7, 1.3], dtype=np.float32)
        return [levels[rng.integers(0, 3, size=int(L))] for L in lengths]
    assert kind == "walk"
    return [np.cumsum(rng.standard_normal(int(L)) / 3.0) for L in lengths]


def with_repeats(curves, seed):
    """The same series with about a third of the points repeating their predecessor: dist = 0 and dx = nl there."""
    rng = np.random.default_rng(seed)
    out = []
    for x in curves:
        x = x.copy()
        for i in range(1, len(x)):
            if rng.random() < 1 / 3:
                x[i] = x[i - 1]
        out.append(x)
    return out


def msm_fit_series():
    """MSM's fit data: 240 univariate series in 6 shape clusters, 20..60 values."""
    return univariate(clustered_curves(240, 20, 60, 1, seed=41))


def msm_brute_series():
    """200 ragged univariate series, 20..60 values."""
    return univariate(clustered_curves(200, 20, 60, 1, seed=42))


def twe_fit_series():
    """TWE's fit data: 240 series of dim 2 in 6 shape clusters, 20..60 points."""
    return clustered_curves(240, 20, 60, 2, seed=43)


def twe_brute_series():
    """200 ragged series of dim 3, 20..60 points."""
    return clustered_curves(200, 20, 60, 3, seed=44)


def twe_univariate_series():
    """120 ragged univariate series, 20..60 values."""
    return univariate(clustered_curves(120, 20, 60, 1, seed=45))
