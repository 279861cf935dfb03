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
(the kernel's schedule) must agree bit for bit, and so must the kernel.  dist is symmetric bit for bit, so the transposed matrix
has the same cells, which lets `erp_pairs_host` keep the SHORTER member of a pair on the vectorised axis and the kernel the
LONGER one on the lanes; test_erp_host.py checks both against `erp_loop`, which never swaps."""
import numpy as np

from frechet_cases import as_curve, clustered_curves, one_of_each_length   # noqa: F401  (the tests' builders)
from pool_cases import FIT_CFG, all_ordered_pairs   # noqa: F401

DIMS = (1, 2, 3, 4)


def _dist(a, b):
    """dist of the definition between arrays of points [..., dim] (or a point and the gap value), elementwise: NumPy rounds
    every subtraction, product and addition on its own, and its float64 square root is correctly rounded."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if b.ndim == 0:
        b = b[None]
    t = a[..., 0] - b[..., 0]
    if a.shape[-1] == 1:
        return np.abs(t)
    c = t * t
    for k in range(1, a.shape[-1]):
        t = a[..., k] - b[..., k if b.shape[-1] > 1 else 0]
        c = c + t * t
    return np.sqrt(c)


def gap_sums(x, gap):
    """E(i, -1) of a member for i = 0 .. len-1: summed left to right, one addition per point."""
    g = _dist(as_curve(x), np.float64(gap)).tolist()
    out, e = [], 0.0
    for v in g:
        e = e + v
        out.append(e)
    return np.array(out, dtype=np.float64)


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


def erp_pairs_host(series, IJ, gap=0.0):
    """erp(series[i], series[j]) for every row (i, j) of IJ -> float64 [len(IJ)].

    All pairs advance together, one anti-diagonal k = i + j per step.  A pair's state is one value per point of its shorter
    member (index i): diagonal k holds E(i, k - i), and E(i, -1) where k - i < 0.  The pairs are laid end to end in one flat
    array, ordered by their number of diagonals (descending), so the pairs still running are always a prefix of it."""
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    P = IJ.shape[0]
    out = np.zeros(P, dtype=np.float64)
    if P == 0:
        return out
    cur_ = [as_curve(s) for s in series]
    dim = cur_[0].shape[1]
    lens = np.array([len(s) for s in cur_], dtype=np.int64)
    la, lb = lens[IJ[:, 0]], lens[IJ[:, 1]]
    swap = la > lb                                   # the shorter member on the vectorised axis
    A = np.where(swap, IJ[:, 1], IJ[:, 0])
    B = np.where(swap, IJ[:, 0], IJ[:, 1])
    a, b = lens[A], lens[B]
    order = np.argsort(-(a + b), kind="stable")
    A, B, a, b = A[order], B[order], a[order], b[order]
    # the data set, once: points end to end, every point's gap cost, every member's running sums of them
    pool = np.concatenate(cur_, axis=0)
    assert pool.shape[1] == dim
    gcost = _dist(pool, np.float64(gap))
    gsum = np.concatenate([gap_sums(s, gap) for s in cur_])
    start = np.concatenate([[0], np.cumsum(lens)[:-1]])
    seg = np.concatenate([[0], np.cumsum(a)])        # a pair's points: seg[p] .. seg[p + 1]
    pid = np.repeat(np.arange(P), a)
    I = np.arange(seg[-1]) - seg[pid]                # row i of each point
    xat = start[A][pid] + I
    X, GX, E0 = pool[xat], gcost[xat], gsum[xat]     # E0: E(i, -1)
    ybase, ylen = start[B][pid], b[pid]
    first = I == 0
    last_el = seg[1:] - 1                            # the point of row a - 1
    fin = a + b - 2                                  # the diagonal of the corner cell (descending)
    d1 = E0.copy()                                   # diagonal k - 1
    d2 = E0.copy()                                   # diagonal k - 2
    live = P
    for k in range(int(fin[0]) + 1):
        E = seg[live]
        J = k - I[:E]
        valid = (J >= 0) & (J < ylen[:E])
        at = ybase[:E] + np.clip(J, 0, ylen[:E] - 1)
        dist = _dist(X[:E], pool[at])
        f = first[:E]
        up = np.empty(E)                             # E(i - 1, j): the point before, one diagonal back; row -1 for i = 0
        up[1:] = d1[:E - 1]
        up[f] = gsum[at[f]]
        dg = np.empty(E)                             # E(i - 1, j - 1): the point before, two diagonals back
        dg[1:] = d2[:E - 1]
        dg[f] = np.where(J[f] > 0, gsum[np.maximum(at[f] - 1, 0)], 0.0)
        cur = np.minimum(np.minimum(dg + dist, up + GX[:E]), d1[:E] + gcost[at])
        cur[~valid] = E0[:E][~valid]                 # (j < 0: column -1; j >= m: cells nobody reads)
        lo = np.searchsorted(-fin[:live], -k, side="left")   # pairs lo .. live - 1 end on this diagonal
        out[order[lo:live]] = cur[last_el[lo:live]]
        live = lo
        d2, d1 = d1, cur
        if live == 0:
            break
    return out


# ------------------------------------------------------------------------------------------ the kernel's schedule, restated
WAVE = 64


def _lane_down(v):
    """Lane l receives lane l - 1's value; lane 0 of the wavefront keeps its own (axis 1 is the lane)."""
    out = v.copy()
    out[:, 1:] = v[:, :-1]
    return out


def _lane_up(v):
    """Lane l receives lane l + 1's value; lane 63 keeps its own."""
    out = v.copy()
    out[:, :-1] = v[:, 1:]
    return out


def erp_lanes(series, IJ, gap, R, G):
    """k_seqdp<T, DIM, R, G, ErpOp> of csrc/seqdp.hip restated lane by lane: 64 lanes per wavefront (axis 1; axis 0 is the
    wavefronts, which do not interact and are advanced together), one pair per group of G lanes, the longer member on the
    lanes, R rows per lane, the point of y moving down the lanes and the strip (points of y and E(-1, .)) moving up, column -1
    and row -1 from the gap sums, slots past the end of the list on pair (0, 0) storing nothing."""
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    P = len(IJ)
    cur_ = [as_curve(s) for s in series]
    dim = cur_[0].shape[1]
    lens = np.array([len(s) for s in cur_], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    val = np.concatenate(cur_, axis=0)
    gapsum = np.concatenate([gap_sums(s, gap) for s in cur_])
    g = np.float64(gap)
    PPW = WAVE // G
    W = (P + PPW - 1) // PPW
    lane = np.tile(np.arange(WAVE), (W, 1))
    gl, slot = lane & (G - 1), lane // G
    t = np.arange(W)[:, None] * PPW + slot
    active = t < P
    i = np.where(active, IJ[np.minimum(t, P - 1), 0], 0)
    j = np.where(active, IJ[np.minimum(t, P - 1), 1], 0)
    n, m = lens[i], lens[j]
    xo, yo = off[i], off[j]
    sw = n < m                                         # the longer member on the lanes
    n, m, xo, yo = np.where(sw, m, n), np.where(sw, n, m), np.where(sw, yo, xo), np.where(sw, xo, yo)
    xr, d, gxr = [], [], []
    for r in range(R):
        row = np.minimum(gl * R + r, n - 1)
        xr.append(val[xo + row])
        gxr.append(_dist(xr[r], g))
        d.append(gapsum[xo + row])                     # column -1
    steps = (m + (n - 1) // R).max(axis=1)             # (wave-uniform: the largest of the wavefront's pairs)
    INF = np.inf
    bottom = d[R - 1].copy()
    top_prev = np.where(gl == 0, 0.0, INF)
    ycur = np.zeros((W, WAVE, dim))
    ynext = val[yo + np.minimum(gl, m - 1)]
    gnext = gapsum[yo + np.minimum(gl, m - 1)]
    alive = np.ones(W, dtype=bool)
    for s0 in range(0, int(steps.max()), G):
        at = yo + np.minimum(s0 + G + gl, m - 1)
        ybuf, ynext = ynext, val[at]
        gbuf, gnext = gnext, gapsum[at]
        for s in range(s0, min(s0 + G, int(steps.max()))):
            alive = s < steps                          # a wavefront past its own step count has left the loop
            top = _lane_down(bottom)
            yv = _lane_down(ycur)
            ycur_new = np.where((gl == 0)[..., None], ybuf, yv)
            ybuf = _lane_up(ybuf)
            top = np.where(gl == 0, gbuf, top)         # row -1: E(-1, s)
            gbuf = _lane_up(gbuf)
            diag = top_prev
            jc = s - gl
            on = (jc >= 0) & (jc < m) & alive[:, None]
            keep = alive[:, None]
            ycur = np.where(keep[..., None], ycur_new, ycur)
            top_prev = np.where(keep, top, top_prev)
            gy = _dist(ycur, g)
            up, dg = top, diag
            for r in range(R):
                dist = _dist(xr[r], ycur)
                left = d[r]
                v = np.minimum(np.minimum(dg + dist, up + gxr[r]), left + gy)
                dg, up = left, v
                d[r] = np.where(on, v, d[r])
            bottom = np.where(on, up, bottom)
    out = np.full(P, np.nan)
    res = np.take_along_axis(np.stack(d, axis=-1), ((n - 1) % R)[..., None], axis=-1)[..., 0]
    store = active & (gl == (n - 1) // R)
    assert store.sum() == P
    out[t[store]] = res[store]
    return out


# ------------------------------------------------------------------------------------------------------------- data
def max_length(dim):
    return 2048 if dim == 1 else 1024


def instantiations(dim):
    """The kernel's shapes at `dim` (R rows per lane, G lanes per pair); a shape takes data sets whose longest series has up to
    R G points.  A lane holds R DIM coordinates, R cells and R gap costs: R = 32 at dim 1 only."""
    return [(8, 16), (8, 64), (32, 64) if dim == 1 else (16, 64)]


def boundary_lengths(dim):
    """{R-1, R, R+1, 2R, GR-1, GR, GR+1} of every shape at `dim` that are within the limit, the limit and the limit minus 1; and
    1, the shortest partner."""
    limit = max_length(dim)
    Ls = {1, limit - 1, limit}
    for R, G in instantiations(dim):
        Ls.update(L for L in (R - 1, R, R + 1, 2 * R, G * R - 1, G * R, G * R + 1) if L <= limit)
    return sorted(Ls)


def fit_curves():
    """The fit tests' data: 240 series of dim 2 in 6 shape clusters, 20..60 points."""
    return clustered_curves(240, 20, 60, 2, seed=31)


def brute_curves():
    """200 ragged series of dim 3, 20..60 points."""
    return clustered_curves(200, 20, 60, 3, seed=32)


def univariate_series():
    """120 ragged univariate series, 20..60 values."""
    return [x[:, 0] for x in clustered_curves(120, 20, 60, 1, seed=35)]
