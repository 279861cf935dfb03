"""The discrete Frechet distance on the host, and the data sets of the Frechet tests.

Definition (annchor_amd.distances.Frechet).  A curve is a sequence of 1 .. L points of `dim` coordinates, dim in 1 .. 4.  All
arithmetic is float64; float32 input widens exactly.

    c(i, j) = sum over k = 0 .. dim-1, in that order, of t_k * t_k,  t_k = x[i][k] - y[j][k]
              (every subtraction, product and addition rounded on its own, never an fma;
               the sum starts from the k = 0 product, not from 0.0 + ...)
    F(i, j) = max(c(i, j), min(F(i-1, j), F(i, j-1), F(i-1, j-1))),   F(-1, -1) = 0, +inf outside the matrix
    frechet(x, y) = sqrt(F(n-1, m-1)), correctly rounded

max and min are exact and every c(i, j) has fixed operands, so every evaluation order gives the same bits: `frechet_loop` (the
plain double loop) and `frechet_pairs_host` (anti-diagonals, many pairs at once) must agree bit for bit, and so must the kernel.
The transposed matrix has the same cells -- (x - y)^2 == (y - x)^2 exactly, and the order of k is fixed -- which lets
`frechet_pairs_host` keep the SHORTER curve of a pair on the vectorised axis; test_frechet_host.py checks that against
`frechet_loop`, which never swaps."""
import numpy as np

from pool_cases import FIT_CFG, all_ordered_pairs   # noqa: F401  (the tests' builders)
from seqdp_cases import DIMS, as_curve, clustered_curves, frechet_pairs_host, one_of_each_length   # noqa: F401


def frechet_loop(x, y):
    """The definition, cell by cell."""
    x, y = as_curve(x), as_curve(y)
    n, m, dim = len(x), len(y), x.shape[1]
    assert y.shape[1] == dim
    F = np.full((n + 1, m + 1), np.inf)
    F[0, 0] = 0.0
    for i in range(n):
        for j in range(m):
            t = x[i, 0] - y[j, 0]
            c = t * t
            for k in range(1, dim):
                t = x[i, k] - y[j, k]
                c = c + t * t
            F[i + 1, j + 1] = max(c, min(F[i, j + 1], F[i + 1, j], F[i, j]))
    return np.sqrt(F[n, m])


# ------------------------------------------------------------------------------------------------------------- data
def fit_curves():
    """The fit tests' data: 240 curves of dim 2 in 6 shape clusters, 20..60 points."""
    return clustered_curves(240, 20, 60, 2, seed=31)


def brute_curves():
    """200 ragged curves of dim 3, 20..60 points."""
    return clustered_curves(200, 20, 60, 3, seed=32)
