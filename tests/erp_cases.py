"""Edit distance with real penalty (ERP) on the host, a lane-by-lane restatement of the kernel's schedule, and the data sets of
the ERP tests.

Definition (annchor_amd.distances.ERP).  A series is 1 .. L points of `dim` coordinates, dim in 1 .. 4.  All arithmetic is
float64; float32 input widens exactly.  g is the gap value, a finite float64 scalar with default 0.0.  The gap point is
(g, ..., g).

    dist(a, b)  dim 1:   |a[0] - b[0]|
                dim > 1: sqrt( sum over k = 0 .. dim-1, in that order, of t_k * t_k ),  t_k = a[k] - b[k],  correctly rounded sqrt
                (every subtraction, product and addition rounded on its own, never an fma; the sum starts from the k = 0 product)
    gx(i) = dist(x[i], gap point)        gy(j) = dist(y[j], gap point)
    E(-1, -1) = 0     E(i, -1) = E(i-1, -1) + gx(i)     E(-1, j) = E(-1, j-1) + gy(j)        (left to right, one addition per step)
    E(i, j) = min( E(i-1, j-1) + dist(x[i], y[j]),   E(i-1, j) + gx(i),   E(i, j-1) + gy(j) )
    erp(x, y) = E(n-1, m-1)                                                                    (no square root at the end)

Every cell is the min of three sums of fixed operands; min is exact and the additions are commutative, so every evaluation order
gives the same bits: `erp_loop` (the plain double loop), `erp_pairs_host` (anti-diagonals, many pairs at once) and `erp_lanes`
(the kernel's schedule; both are seqdp_cases' shared code with the Erp measure) must agree bit for bit, and so must the
kernel.  dist is symmetric bit for bit, so the transposed matrix has the same cells, which lets `erp_pairs_host` keep the
SHORTER member of a pair on the vectorised axis and the kernel the LONGER one on the lanes; test_erp_host.py checks both against
`erp_loop`, which never swaps."""
import numpy as np

from pool_cases import FIT_CFG, all_ordered_pairs   # noqa: F401
from seqdp_cases import (DIMS, _dist, as_curve, clustered_curves, erp_lanes, erp_pairs_host, gap_sums,   # noqa: F401
                         one_of_each_length)


def erp_loop(x, y, gap=0.0):
    """The definition, cell by cell (the point distances of a row are evaluated elementwise beforehand)."""
    x, y = as_curve(x), as_curve(y)
    n, m = len(x), len(y)
    assert y.shape[1] == x.shape[1]
    g = np.float64(gap)
    gx, gy = _dist(x, g).tolist(), _dist(y, g).tolist()
    prev = [0.0] * (m + 1)                       # row -1: E(-1, -1), E(-1, 0), ...
    for j in range(m):
        prev[j + 1] = prev[j] + gy[j]
    left = 0.0                                   # E(i - 1, -1)
    for i in range(n):
        dist = _dist(x[i][None, :], y).tolist()
        gxi = gx[i]
        left = left + gxi                        # E(i, -1)
        cur = [left] * (m + 1)
        e = left
        for j in range(m):
            e = min(prev[j] + dist[j], prev[j + 1] + gxi, e + gy[j])
            cur[j + 1] = e
        prev = cur
    return np.float64(prev[m])


# ------------------------------------------------------------------------------------------------------------- data
def fit_curves():
    """The fit tests' data: 240 series of dim 2 in 6 shape clusters, 20..60 points."""
    return clustered_curves(240, 20, 60, 2, seed=31)


def brute_curves():
    """200 ragged series of dim 3, 20..60 points."""
    return clustered_curves(200, 20, 60, 3, seed=32)


def univariate_series():
    """120 ragged univariate series, 20..60 values."""
    return [x[:, 0] for x in clustered_curves(120, 20, 60, 1, seed=35)]
