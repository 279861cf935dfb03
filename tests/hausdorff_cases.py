"""The Hausdorff distance on the host, and the data sets of the Hausdorff tests.

Definition (annchor_amd.distances.Hausdorff).  A point set is 1 .. 4096 points of `dim` coordinates, with `dim` in 1 .. 4.  All
arithmetic is float64.  float32 input widens exactly.

    c(i, j)  = sum over k = 0 .. dim-1, in that order, of t_k * t_k,   t_k = x[i][k] - y[j][k]
               (every subtraction, product and addition rounded on its own: -ffp-contract=off, never an fma;
                the sum starts from the k = 0 product, not from 0.0 + ...)
    h(x, y)  = max over i of ( min over j of c(i, j) )          -- directed, x to y
    hausdorff(x, y) = sqrt( max( h(x, y), h(y, x) ) ), correctly rounded

(x - y)^2 == (y - x)^2 exactly and the order of k is fixed, so c(j, i) computed with the roles swapped has the same bits as
c(i, j); min and max are exact and associative.  `hausdorff_loop` is the definition cell by cell: it computes h(y, x) from
y[j] - x[i], with no swap.  `hausdorff_pairs_host` builds the cost matrix of a pair once (x[i] - y[j], a block of rows at a
time) and takes both directed distances from it; test_hausdorff_host.py checks the two against each other bit for bit, and the
kernel must equal them."""
import numpy as np

import seqdp_cases as sc
from seqdp_cases import clustered_curves, one_of_each_length   # noqa: F401  (the tests' builders)
from pool_cases import FIT_CFG, all_ordered_pairs   # noqa: F401

DIMS = sc.DIMS
MAX_POINTS = 4096
SHORT = 512   # csrc/hausdorff.hip HAUS_SHORT: the longest set of a data set that still runs the 4-pairs-per-wavefront shape


def as_set(x):
    """[len, dim] float64; a 1-D member is a set of dim 1."""
    x = np.asarray(x, dtype=np.float64)
    return x[:, None] if x.ndim == 1 else x


def _directed_loop(x, y):
    n, m, dim = len(x), len(y), x.shape[1]
    h = -np.inf
    for i in range(n):
        lo = np.inf
        for j in range(m):
            t = x[i, 0] - y[j, 0]
            c = t * t
            for k in range(1, dim):
                t = x[i, k] - y[j, k]
                c = c + t * t
            lo = min(lo, c)
        h = max(h, lo)
    return h


def hausdorff_loop(x, y):
    """The definition, cell by cell: two directed passes, each with its own subtractions."""
    x, y = as_set(x), as_set(y)
    assert x.shape[1] == y.shape[1]
    return np.sqrt(max(_directed_loop(x, y), _directed_loop(y, x)))


CHUNK_CELLS = 1 << 20   # cells of the cost matrix held at a time: 8 MB, so a 4096 x 4096 pair runs in 16 blocks of 256 rows


def hausdorff_pair_host(x, y):
    x, y = as_set(x), as_set(y)
    n, m, dim = len(x), len(y), x.shape[1]
    assert y.shape[1] == dim
    yk = [np.ascontiguousarray(y[:, k]) for k in range(dim)]
    rows = max(1, CHUNK_CELLS // m)
    colmin = np.full(m, np.inf)
    hxy = -np.inf
    for r0 in range(0, n, rows):
        xb = x[r0:r0 + rows]
        t = xb[:, 0, None] - yk[0][None, :]
        c = t * t
        for k in range(1, dim):
            t = xb[:, k, None] - yk[k][None, :]
            c = c + t * t
        hxy = max(hxy, c.min(axis=1).max())
        np.minimum(colmin, c.min(axis=0), out=colmin)
    return np.sqrt(max(hxy, colmin.max()))


def hausdorff_pairs_host(sets, IJ):
    """hausdorff(sets[i], sets[j]) for every row (i, j) of IJ -> float64 [len(IJ)]."""
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    S = [as_set(s) for s in sets]
    return np.array([hausdorff_pair_host(S[i], S[j]) for i, j in IJ], dtype=np.float64)


def all_pairs_matrix(sets):
    """Every ordered pair, [nx, nx], each computed in its own order."""
    nx = len(sets)
    return hausdorff_pairs_host(sets, all_ordered_pairs(nx)).reshape(nx, nx)


# ------------------------------------------------------------------------------------------------------------- data
def instantiations(dim):
    """The kernel's shapes (R points per lane, G lanes per pair), the same at every `dim`: (8, 16) for data sets whose longest
    set has up to SHORT points, (8, 64) beyond."""
    return [(8, 16), (8, 64)]


def shape_limit(shape):
    """The longest set of a data set that runs shape number `shape`."""
    return (SHORT, MAX_POINTS)[shape]


def boundary_lengths(dim):
    """{1, R-1, R, R+1, 2R, GR-1, GR, GR+1, 2GR+1} of every shape, 4095 and 4096."""
    Ls = {1, MAX_POINTS - 1, MAX_POINTS}
    for R, G in instantiations(dim):
        Ls.update((R - 1, R, R + 1, 2 * R, G * R - 1, G * R, G * R + 1, 2 * G * R + 1))
    return sorted(Ls)


def fit_sets():
    """The fit tests' data: the point lists of 240 curves of dim 2 in 6 shape clusters, 20..60 points."""
    return clustered_curves(240, 20, 60, 2, seed=31)


def brute_sets():
    """200 ragged sets of dim 3, 20..60 points."""
    return clustered_curves(200, 20, 60, 3, seed=32)
