"""Dynamic time warping on the host, and the data sets of the DTW tests.

Definition (annchor_amd.distances.DTW), all arithmetic in float64 (float32 input widens exactly):

    c(i, j) = t * t with t = x_i - y_j                  -- two roundings, no fused multiply-add
    D(i, j) = c(i, j) + min(D(i-1, j), D(i, j-1), D(i-1, j-1)),   D(-1, -1) = 0, +inf outside the matrix
    window w >= 0: cells with |i - j| > max(w, |n - m|) are +inf
    dtw(x, y) = sqrt(D(n-1, m-1))

min is exact and every cell has fixed operands, so every evaluation order gives the same bits: `dtw_loop` (the plain
double loop) and `dtw_pairs_host` (anti-diagonals, many pairs at once) must agree bit for bit, and so must the kernel.
The transposed matrix has the same cells -- (x_i - y_j)^2 == (y_j - x_i)^2 exactly -- which lets `dtw_pairs_host` keep the
SHORTER series of a pair on the vectorised axis; test_dtw_host.py checks that against `dtw_loop`, which never swaps."""
import numpy as np

from pool_cases import FIT_CFG, all_ordered_pairs   # noqa: F401  (the tests' builders)
from seqdp_cases import dtw_pairs_host   # noqa: F401  (the shared sweep with the Dtw measure)


def dtw_loop(x, y, window=None):
    """The definition, cell by cell."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, m = len(x), len(y)
    w = None if window is None else max(int(window), abs(n - m))
    D = np.full((n + 1, m + 1), np.inf)
    D[0, 0] = 0.0
    for i in range(n):
        for j in range(m):
            if w is not None and abs(i - j) > w:
                continue
            t = x[i] - y[j]
            D[i + 1, j + 1] = t * t + min(D[i, j + 1], D[i + 1, j], D[i, j])
    return np.sqrt(D[n, m])


# ------------------------------------------------------------------------------------------------------------- data
SHAPES = 6


def _shape(kind, u):
    """Six families of curves on u in [0, 1]."""
    return [np.sin(2 * np.pi * u), np.sin(4 * np.pi * u), 2 * u - 1, np.abs(4 * u - 2) - 1, np.sign(np.sin(3 * np.pi * u + 0.3)),
            np.exp(-40 * (u - 0.5) ** 2) * 2 - 0.5][kind]


def clustered_series(nx, lo, hi, seed, dtype=np.float64):
    """nx ragged series of lengths lo..hi in SHAPES shape clusters: a family's curve under a random time warp, amplitude and
    noise."""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(nx):
        L = int(rng.integers(lo, hi + 1))
        u = np.linspace(0, 1, L) ** rng.uniform(0.7, 1.4)
        x = rng.uniform(0.8, 1.2) * _shape(s % SHAPES, u) + 3.0 * (s % SHAPES) + 0.15 * rng.standard_normal(L)
        out.append(x.astype(dtype))
    return out


def one_of_each_length(lengths, seed, dtype=np.float64):
    """One random-walk series per length."""
    rng = np.random.default_rng(seed)
    return [np.cumsum(rng.standard_normal(int(L))).astype(dtype) for L in lengths]


# the kernel's instantiations (R rows per lane, G lanes per pair, longest series of the data set they take)
INSTANTIATIONS = [(8, 16), (8, 64), (32, 64)]
MAX_LENGTH = 2048


def boundary_lengths(R, G):
    return [L for L in (R - 1, R, R + 1, 2 * R, G * R - 1, G * R, G * R + 1) if L <= MAX_LENGTH]


def fit_series():
    """The fit tests' data: 240 series in 6 shape clusters, lengths 20..60."""
    return clustered_series(240, 20, 60, seed=11)


def brute_series():
    """200 ragged series, lengths 20..60."""
    return clustered_series(200, 20, 60, seed=12)
