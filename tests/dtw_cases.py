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


def dtw_pairs_host(series, IJ, window=None):
    """dtw(series[i], series[j]) for every row (i, j) of IJ -> float64 [len(IJ)].

    All pairs advance together, one anti-diagonal k = i + j per step.  A pair's state is one value per element of its
    shorter series (index i): diagonal k holds D(i, k - i).  The pairs are laid end to end in one flat array, ordered by
    their number of diagonals (descending), so the pairs still running are always a prefix of it."""
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    P = IJ.shape[0]
    out = np.zeros(P, dtype=np.float64)
    if P == 0:
        return out
    ser = [np.asarray(s, dtype=np.float64) for s in series]
    lens = np.array([len(s) for s in ser], dtype=np.int64)
    la, lb = lens[IJ[:, 0]], lens[IJ[:, 1]]
    swap = la > lb                                   # the shorter series on the vectorised axis
    A = np.where(swap, IJ[:, 1], IJ[:, 0])
    B = np.where(swap, IJ[:, 0], IJ[:, 1])
    a, b = lens[A], lens[B]
    order = np.argsort(-(a + b), kind="stable")
    A, B, a, b = A[order], B[order], a[order], b[order]
    band = None if window is None else np.maximum(int(window), b - a)
    # the data set, once: values end to end
    pool = np.concatenate(ser)
    start = np.concatenate([[0], np.cumsum(lens)[:-1]])
    seg = np.concatenate([[0], np.cumsum(a)])        # a pair's elements: seg[p] .. seg[p + 1]
    pid = np.repeat(np.arange(P), a)
    I = np.arange(seg[-1]) - seg[pid]                # row i of each element
    X = pool[start[A][pid] + I]
    ybase, ylen = start[B][pid], b[pid]
    first = I == 0
    wel = None if band is None else band[pid]
    last_el = seg[1:] - 1                            # the element of row a - 1
    fin = a + b - 2                                  # the diagonal of the corner cell (descending)
    d1 = np.full(seg[-1], np.inf)                    # diagonal k - 1
    d2 = np.full(seg[-1], np.inf)                    # diagonal k - 2
    live = P
    for k in range(int(fin[0]) + 1):
        E = seg[live]
        J = k - I[:E]
        valid = (J >= 0) & (J < ylen[:E])
        if wel is not None:
            valid &= np.abs(I[:E] - J) <= wel[:E]
        yv = pool[ybase[:E] + np.clip(J, 0, ylen[:E] - 1)]
        t = X[:E] - yv
        c = t * t
        up = np.empty(E)                             # D(i - 1, j): the element before, one diagonal back
        up[1:] = d1[:E - 1]
        up[first[:E]] = np.inf
        dg = np.empty(E)                             # D(i - 1, j - 1): the element before, two diagonals back
        dg[1:] = d2[:E - 1]
        dg[first[:E]] = 0.0 if k == 0 else np.inf
        cur = c + np.minimum(np.minimum(d1[:E], up), dg)
        cur[~valid] = np.inf
        lo = np.searchsorted(-fin[:live], -k, side="left")   # pairs lo .. live - 1 end on this diagonal
        out[order[lo:live]] = np.sqrt(cur[last_el[lo:live]])
        live = lo
        d2, d1 = d1, cur
        if live == 0:
            break
    return out


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
