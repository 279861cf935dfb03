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


def as_curve(x):
    """[len, dim] float64; a 1-D member is a curve of dim 1."""
    x = np.asarray(x, dtype=np.float64)
    return x[:, None] if x.ndim == 1 else x


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


def frechet_pairs_host(curves, IJ):
    """frechet(curves[i], curves[j]) for every row (i, j) of IJ -> float64 [len(IJ)].

    All pairs advance together, one anti-diagonal k = i + j per step.  A pair's state is one value per point of its shorter
    curve (index i): diagonal k holds F(i, k - i).  The pairs are laid end to end in one flat array, ordered by their number
    of diagonals (descending), so the pairs still running are always a prefix of it."""
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    P = IJ.shape[0]
    out = np.zeros(P, dtype=np.float64)
    if P == 0:
        return out
    cur_ = [as_curve(s) for s in curves]
    dim = cur_[0].shape[1]
    lens = np.array([len(s) for s in cur_], dtype=np.int64)
    la, lb = lens[IJ[:, 0]], lens[IJ[:, 1]]
    swap = la > lb                                   # the shorter curve on the vectorised axis
    A = np.where(swap, IJ[:, 1], IJ[:, 0])
    B = np.where(swap, IJ[:, 0], IJ[:, 1])
    a, b = lens[A], lens[B]
    order = np.argsort(-(a + b), kind="stable")
    A, B, a, b = A[order], B[order], a[order], b[order]
    # the data set, once: points end to end, one array per coordinate
    pool = np.concatenate(cur_, axis=0)
    assert pool.shape[1] == dim
    pool = [np.ascontiguousarray(pool[:, k]) for k in range(dim)]
    start = np.concatenate([[0], np.cumsum(lens)[:-1]])
    seg = np.concatenate([[0], np.cumsum(a)])        # a pair's points: seg[p] .. seg[p + 1]
    pid = np.repeat(np.arange(P), a)
    I = np.arange(seg[-1]) - seg[pid]                # row i of each point
    X = [p[start[A][pid] + I] for p in pool]
    ybase, ylen = start[B][pid], b[pid]
    first = I == 0
    last_el = seg[1:] - 1                            # the point of row a - 1
    fin = a + b - 2                                  # the diagonal of the corner cell (descending)
    d1 = np.full(seg[-1], np.inf)                    # diagonal k - 1
    d2 = np.full(seg[-1], np.inf)                    # diagonal k - 2
    live = P
    for k in range(int(fin[0]) + 1):
        E = seg[live]
        J = k - I[:E]
        valid = (J >= 0) & (J < ylen[:E])
        at = ybase[:E] + np.clip(J, 0, ylen[:E] - 1)
        t = X[0][:E] - pool[0][at]
        c = t * t
        for q in range(1, dim):
            t = X[q][:E] - pool[q][at]
            c = c + t * t
        up = np.empty(E)                             # F(i - 1, j): the point before, one diagonal back
        up[1:] = d1[:E - 1]
        up[first[:E]] = np.inf
        dg = np.empty(E)                             # F(i - 1, j - 1): the point before, two diagonals back
        dg[1:] = d2[:E - 1]
        dg[first[:E]] = 0.0 if k == 0 else np.inf
        cur = np.maximum(c, np.minimum(np.minimum(d1[:E], up), dg))
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
    """Six families of coordinate functions on u in [0, 1]."""
    return [np.sin(2 * np.pi * u), np.sin(4 * np.pi * u), 2 * u - 1, np.abs(4 * u - 2) - 1, np.cos(3 * np.pi * u + 0.3),
            np.exp(-40 * (u - 0.5) ** 2) * 2 - 0.5][kind % SHAPES]


def clustered_curves(nx, lo, hi, dim, seed, dtype=np.float64):
    """nx ragged curves of lo..hi points in SHAPES shape clusters: coordinate k of cluster s is family s + k under a random
    reparametrisation and amplitude, the cluster's offset on coordinate 0, and noise on every coordinate of every point (so no
    two point pairs are at the same distance by construction, and no two curve pairs tie)."""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(nx):
        L = int(rng.integers(lo, hi + 1))
        u = np.linspace(0, 1, L) ** rng.uniform(0.7, 1.4)
        amp = rng.uniform(0.8, 1.2)
        x = np.stack([amp * _shape(s % SHAPES + k, u) for k in range(dim)], axis=1)
        x[:, 0] += 3.0 * (s % SHAPES)
        x += 0.15 * rng.standard_normal((L, dim))
        out.append(x.astype(dtype))
    return out


def one_of_each_length(lengths, dim, seed, dtype=np.float64):
    """One random-walk curve per length."""
    rng = np.random.default_rng(seed)
    return [np.cumsum(rng.standard_normal((int(L), dim)), axis=0).astype(dtype) for L in lengths]


DIMS = (1, 2, 3, 4)


def max_length(dim):
    return 2048 if dim <= 2 else 1024


def instantiations(dim):
    """The kernel's shapes at `dim` (R rows per lane, G lanes per pair); a shape takes data sets whose longest curve has up to
    R G points."""
    return [(8, 16), (8, 64), (32, 64) if dim <= 2 else (16, 64)]


def boundary_lengths(dim):
    """{R-1, R, R+1, 2R, GR-1, GR, GR+1} of every shape at `dim` that are within the limit, the limit and the limit minus 1; and
    1, the shortest partner."""
    limit = max_length(dim)
    Ls = {1, limit - 1, limit}
    for R, G in instantiations(dim):
        Ls.update(L for L in (R - 1, R, R + 1, 2 * R, G * R - 1, G * R, G * R + 1) if L <= limit)
    return sorted(Ls)


def fit_curves():
    """The fit tests' data: 240 curves of dim 2 in 6 shape clusters, 20..60 points."""
    return clustered_curves(240, 20, 60, 2, seed=31)


def brute_curves():
    """200 ragged curves of dim 3, 20..60 points."""
    return clustered_curves(200, 20, 60, 3, seed=32)
