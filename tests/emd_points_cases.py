"""The earth mover's distance between point clouds on the host, and the data sets of its tests.

Definition (annchor_amd.distances.PointEMD).  A cloud is 1 .. 128 points of `dim` coordinates, with `dim` in 1 .. 4.  Masses are
uniform.  All arithmetic is float64.  float32 input widens exactly.

    c(i, j)   dim 1:   |x[i][0] - y[j][0]|
              dim > 1: sqrt( sum over k = 0 .. dim-1, in that order, of t_k * t_k ),  t_k = x[i][k] - y[j][k]
    emd(x, y) = min over F >= 0 of  sum_ij F_ij c(i, j)   with  sum_j F_ij = 1/n,  sum_i F_ij = 1/m

Reference: the oracle's exact solver (oracle/emd.c through oracle.metrics.Histograms), which takes any cost matrix of up to 256
bins.  A pair becomes two histograms over n + m bins -- ones on the first n bins, ones on the last m -- and an (n + m)^2 cost
matrix that holds c in its two off-diagonal blocks; the solver normalises each histogram to unit mass.  It is an LP optimum in
floating point, not a bit-exact restatement: the tests compare with ATOL (the project's bar for solves of more than 64 nodes,
test_wasserstein_wide_gpu.py) on data of that test's scale, coordinates in [0, 10)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import seqdp_cases as sc
from oracle import metrics as om
from pool_cases import FIT_CFG, all_ordered_pairs   # noqa: F401  (the tests' builders)

ATOL = 1e-11
DIMS = (1, 2, 3, 4)
MAX_POINTS = 128
SLOT = 64   # csrc/emd.hip: nodes per slot of the wide simplex


def as_cloud(x):
    """[len, dim] float64; a 1-D member is a cloud of dim 1."""
    x = np.asarray(x, dtype=np.float64)
    return x[:, None] if x.ndim == 1 else x


def ground_cost(x, y):
    """c(i, j) of the definition, [n, m], operation by operation."""
    x, y = as_cloud(x), as_cloud(y)
    assert x.shape[1] == y.shape[1]
    t = x[:, 0, None] - y[None, :, 0]
    if x.shape[1] == 1:
        return np.abs(t)
    s = t * t
    for k in range(1, x.shape[1]):
        t = x[:, k, None] - y[None, :, k]
        s = s + t * t
    return np.sqrt(s)


def emd_pair_host(x, y):
    x, y = as_cloud(x), as_cloud(y)
    n, m = len(x), len(y)
    c = ground_cost(x, y)
    H = np.zeros((2, n + m))
    H[0, :n] = 1.0
    H[1, n:] = 1.0
    C = np.zeros((n + m, n + m))
    C[:n, n:] = c
    C[n:, :n] = c.T
    return float(om.Histograms(H, C).pairs(np.array([[0, 1]]), nthreads=1)[0])


def emd_pairs_host(clouds, IJ):
    """emd(clouds[i], clouds[j]) for every row (i, j) of IJ -> float64 [len(IJ)].  (One solver call per pair -- each has its own
    cost matrix -- so the pairs are spread over a few threads; the calls release the interpreter lock.)"""
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    S = [as_cloud(s) for s in clouds]
    om.lib()
    with ThreadPoolExecutor(max_workers=8) as ex:
        out = list(ex.map(lambda p: emd_pair_host(S[p[0]], S[p[1]]), IJ.tolist(), chunksize=16))
    return np.array(out, dtype=np.float64)


def emd_1d_closed_form(x, y):
    """dim 1: the integral of |F - G| between the two empirical distribution functions (at equal sizes this is
    mean |sort(x) - sort(y)|)."""
    x, y = np.sort(np.asarray(x, dtype=np.float64).ravel()), np.sort(np.asarray(y, dtype=np.float64).ravel())
    z = np.sort(np.concatenate([x, y]))
    F = np.searchsorted(x, z[:-1], side="right") / len(x)
    G = np.searchsorted(y, z[:-1], side="right") / len(y)
    return float(np.sum(np.abs(F - G) * np.diff(z)))


def emd_linprog(x, y):
    """The LP itself, handed to scipy's HiGHS."""
    from scipy.optimize import linprog

    c = ground_cost(x, y)
    n, m = c.shape
    A = np.zeros((n + m, n * m))
    for i in range(n):
        A[i, i * m:(i + 1) * m] = 1.0
    for j in range(m):
        A[n + j, j::m] = 1.0
    b = np.concatenate([np.full(n, 1.0 / n), np.full(m, 1.0 / m)])
    r = linprog(c.ravel(), A_eq=A, b_eq=b, bounds=(0, None), method="highs")
    assert r.status == 0, r.message
    return float(r.fun)


# ------------------------------------------------------------------------------------------------------------- data
def random_clouds(sizes, dim, seed, dtype=np.float64):
    """One cloud per size, coordinates uniform in [0, 10)."""
    rng = np.random.default_rng(seed)
    return [(rng.random((int(L), dim)) * 10).astype(dtype) for L in sizes]


def shape_clouds(nx, lo, hi, dim, seed):
    """nx ragged clouds of lo..hi points in six shape clusters (seqdp_cases.clustered_curves, read as point lists), mapped into
    [0, 10) by one affine map for the whole data set.  The clusters' offsets on coordinate 0 are 1.5 apart, not 3: with the gaps
    that 3 leaves between the clusters' distances, a fit of 160 members under FIT_CFG finds sampler partitions with fewer than two
    pairs and raises, in the CPU pipeline as well."""
    X = sc.clustered_curves(nx, lo, hi, dim, seed=seed)
    X = [x - np.array([1.5 * (s % sc.SHAPES)] + [0.0] * (dim - 1)) for s, x in enumerate(X)]
    a, b = min(x.min() for x in X), max(x.max() for x in X)
    return [(x - a) * (9.99 / (b - a)) for x in X]


def lattice_clouds(sizes, dim, seed):
    """Clouds on the integer lattice {0 .. 7}^dim, drawn with replacement: duplicates inside a cloud, points shared between
    clouds, heavily tied costs."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 8, (int(L), dim)).astype(np.float64) for L in sizes]


def sym_table(pairs, nx):
    """pairs(IJ) on every pair i <= j, mirrored, [nx, nx]."""
    iu = np.triu_indices(nx)
    T = np.zeros((nx, nx))
    T[iu] = pairs(np.stack(iu, axis=1))
    T.T[iu] = T[iu]
    return T
