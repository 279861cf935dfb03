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

    TWE, dim 1 .. 4, nu and lam finite and >= 0, nl = nu + lam and nu2 = 2.0 * nu formed once, dist ERP's dist (erp_cases._dist):
        dx(i) = dist(x[i], x[i-1]) + nl        dy(j) = dist(y[j], y[j-1]) + nl
        T(i, j) = min( T(i-1, j-1) + ((dist(x[i], y[j]) + dist(x[i-1], y[j-1])) + nu2 * (double)|i - j|),
                       T(i-1, j) + dx(i),   T(i, j-1) + dy(j) )
        twe(x, y) = T(n-1, m-1)

Every cell is the min of three sums of fixed operands, so every evaluation order gives the same bits: `*_loop` (the plain double
loop, which never swaps the members), `*_pairs_host` (anti-diagonals, many pairs at once, the SHORTER member on the vectorised
axis) and `*_lanes` (the kernel's schedule, the LONGER member on the lanes) must agree bit for bit, and so must the kernel."""
import numpy as np

from erp_cases import WAVE, _dist, _lane_down, _lane_up
from frechet_cases import as_curve, clustered_curves, one_of_each_length   # noqa: F401  (the tests' builders)
from pool_cases import FIT_CFG, all_ordered_pairs   # noqa: F401

DIMS = (1, 2, 3, 4)
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


# ----------------------------------------------------------------------------------------- anti-diagonals, many pairs at once
def _msm_cost_v(v, a, b, c):
    between = ((a <= v) & (v <= b)) | ((a >= v) & (v >= b))
    return np.where(between, c, c + np.minimum(np.abs(v - a), np.abs(v - b)))


class _Msm:
    def __init__(self, c=1.0):
        self.c = np.float64(c)

    def sums(self, x, xp, y, yp, e, dg, up, left):
        """The three sums of a cell: x = x[i], xp = x[i-1], y = y[j], yp = y[j-1] as [..., 1] points, e = i - j."""
        x, xp, y, yp = x[..., 0], xp[..., 0], y[..., 0], yp[..., 0]
        return dg + np.abs(x - y), up + _msm_cost_v(x, xp, y, self.c), left + _msm_cost_v(y, x, yp, self.c)


class _Twe:
    def __init__(self, nu=0.001, lam=1.0):
        self.nl, self.nu2 = np.float64(nu) + np.float64(lam), 2.0 * np.float64(nu)

    def sums(self, x, xp, y, yp, e, dg, up, left):
        return (dg + ((_dist(x, y) + _dist(xp, yp)) + self.nu2 * np.abs(e).astype(np.float64)), up + (_dist(x, xp) + self.nl),
                left + (_dist(y, yp) + self.nl))


def _pairs_host(series, IJ, measure):
    """measure(series[i], series[j]) for every row (i, j) of IJ -> float64 [len(IJ)].

    All pairs advance together, one anti-diagonal k = i + j per step.  A pair's state is one value per point of its shorter member
    (index i): diagonal k holds T(i, k - i).  The pairs are laid end to end in one flat array, ordered by their number of diagonals
    (descending), so the pairs still running are always a prefix of it."""
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
    pool = np.concatenate(cur_, axis=0)
    assert pool.shape[1] == dim
    start = np.concatenate([[0], np.cumsum(lens)[:-1]])
    seg = np.concatenate([[0], np.cumsum(a)])        # a pair's points: seg[p] .. seg[p + 1]
    pid = np.repeat(np.arange(P), a)
    I = np.arange(seg[-1]) - seg[pid]                # row i of each point
    xat = start[A][pid] + I
    first = I == 0
    X = pool[xat]
    XP = np.where(first[:, None], 0.0, pool[np.maximum(xat - 1, 0)])   # x[i - 1], the origin before x[0]
    ybase, ylen = start[B][pid], b[pid]
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
        Y = pool[at]
        YP = np.where((J > 0)[:, None], pool[np.maximum(at - 1, 0)], 0.0)   # y[j - 1], the origin before y[0]
        f = first[:E]
        up = np.empty(E)                             # T(i - 1, j): the point before, one diagonal back
        up[1:] = d1[:E - 1]
        up[f] = np.inf
        dg = np.empty(E)                             # T(i - 1, j - 1): the point before, two diagonals back
        dg[1:] = d2[:E - 1]
        dg[f] = 0.0 if k == 0 else np.inf
        s_match, s_up, s_left = measure.sums(X[:E], XP[:E], Y, YP, I[:E] - J, dg, up, d1[:E])
        cur = np.minimum(np.minimum(s_match, s_up), s_left)
        cur[~valid] = np.inf
        lo = np.searchsorted(-fin[:live], -k, side="left")   # pairs lo .. live - 1 end on this diagonal
        out[order[lo:live]] = cur[last_el[lo:live]]
        live = lo
        d2, d1 = d1, cur
        if live == 0:
            break
    return out


def msm_pairs_host(series, IJ, c=1.0):
    return _pairs_host(series, IJ, _Msm(c))


def twe_pairs_host(series, IJ, nu=0.001, lam=1.0):
    return _pairs_host(series, IJ, _Twe(nu, lam))


# ------------------------------------------------------------------------------------------ the kernel's schedule, restated
def _lanes(series, IJ, measure, R, G, carry_dist):
    """k_seqdp<T, DIM, R, G, MsmOp / TweOp> of csrc/seqdp.hip restated lane by lane: 64 lanes per wavefront (axis 1; axis 0 is the
    wavefronts, which do not interact and are advanced together), one pair per group of G lanes, the longer member on the lanes,
    R rows per lane, the point of y moving down the lanes and the strip moving up, +inf in column -1 and row -1, slots past the
    end of the list on pair (0, 0) storing nothing.  What MSM and TWE add: `xab`, the point above a lane's first row (x[l R - 1];
    the origin on lane 0 of a group), loaded once; `yprev`, the value the lane's point of y had before this step's move (y[jc - 1];
    the 0.0 it started from at jc = 0); and, with carry_dist (TWE's shapes that keep them in registers), `pd`, the R distances
    dist(x[row], y[jc - 1]) of the lane's last step, which start as dist(x[row], origin) and of which row r reads row r - 1's."""
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    P = len(IJ)
    cur_ = [as_curve(s) for s in series]
    dim = cur_[0].shape[1]
    lens = np.array([len(s) for s in cur_], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    val = np.concatenate(cur_, axis=0)
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
    origin = np.zeros((W, WAVE, dim))
    xab = np.where((gl == 0)[..., None], 0.0, val[xo + np.minimum(np.maximum(gl * R - 1, 0), n - 1)])
    xr, d, pd = [], [], []
    for r in range(R):
        xr.append(val[xo + np.minimum(gl * R + r, n - 1)])
        d.append(np.full((W, WAVE), np.inf))           # column -1
        pd.append(_dist(xr[r], origin))                # dist(x[row], y[-1])
    steps = (m + (n - 1) // R).max(axis=1)             # (wave-uniform: the largest of the wavefront's pairs)
    bottom = np.full((W, WAVE), np.inf)
    top_prev = np.where(gl == 0, 0.0, np.inf)
    ycur = np.zeros((W, WAVE, dim))
    yprev = np.zeros((W, WAVE, dim))
    ynext = val[yo + np.minimum(gl, m - 1)]
    for s0 in range(0, int(steps.max()), G):
        ybuf, ynext = ynext, val[yo + np.minimum(s0 + G + gl, m - 1)]
        for s in range(s0, min(s0 + G, int(steps.max()))):
            alive = (s < steps)[:, None]               # a wavefront past its own step count has left the loop
            top = _lane_down(bottom)
            ycur_new = np.where((gl == 0)[..., None], ybuf, _lane_down(ycur))
            ybuf = _lane_up(ybuf)
            top = np.where(gl == 0, np.inf, top)       # row -1
            diag = top_prev
            jc = s - gl
            on = (jc >= 0) & (jc < m) & alive
            yprev = np.where(alive[..., None], ycur, yprev)      # what ycur held before this step's move
            ycur = np.where(alive[..., None], ycur_new, ycur)
            top_prev = np.where(alive, top, top_prev)
            carry = _dist(xab, yprev)                  # row 0 of the lane: dist(x[l R - 1], y[jc - 1])
            up, dg = top, diag
            for r in range(R):
                xp = xab if r == 0 else xr[r - 1]
                if carry_dist:                         # (what the sums below recompute from xp and yprev, handed down the rows)
                    assert np.array_equal(carry[on], _dist(xp, yprev)[on])
                    carry = pd[r]
                    pd[r] = np.where(on, _dist(xr[r], ycur), pd[r])
                left = d[r]
                s_match, s_up, s_left = measure.sums(xr[r], xp, ycur, yprev, gl * R + r - jc, dg, up, left)
                v = np.minimum(np.minimum(s_match, s_up), s_left)
                dg, up = left, v
                d[r] = np.where(on, v, d[r])
            bottom = np.where(on, up, bottom)
    out = np.full(P, np.nan)
    res = np.take_along_axis(np.stack(d, axis=-1), ((n - 1) % R)[..., None], axis=-1)[..., 0]
    store = active & (gl == (n - 1) // R)
    assert store.sum() == P
    out[t[store]] = res[store]
    return out


def msm_lanes(series, IJ, c, R, G):
    return _lanes(series, IJ, _Msm(c), R, G, carry_dist=False)


def twe_lanes(series, IJ, nu, lam, R, G):
    dim = as_curve(series[0]).shape[1]
    return _lanes(series, IJ, _Twe(nu, lam), R, G, carry_dist=not (dim == 1 and R > 16))


# ------------------------------------------------------------------------------------------------------------- data
MSM_MAX_LENGTH = 2048


def twe_max_length(dim):
    """The tests read TWE's boundaries from the package."""
    from annchor_amd.distances import twe_max_length as f

    return f(dim)


def instantiations(dim, limit):
    """The kernel's shapes at `dim` (R rows per lane, G lanes per pair); a shape takes data sets whose longest series has up to
    R G points, the widest `limit` of them."""
    assert limit % 64 == 0
    return [(8, 16), (8, 64), (limit // 64, 64)]


def boundary_lengths(dim, limit):
    """{R-1, R, R+1, 2R, GR-1, GR, GR+1} of every shape at `dim` that are within the limit, the limit and the limit minus 1; and
    1, the shortest partner."""
    Ls = {1, limit - 1, limit}
    for R, G in instantiations(dim, limit):
        Ls.update(L for L in (R - 1, R, R + 1, 2 * R, G * R - 1, G * R, G * R + 1) if L <= limit)
    return sorted(Ls)


def boundary_case(dim, limit, shape):
    """The data set that runs shape number `shape` at `dim` -- the kernel is chosen by the data set's longest series, so it holds
    the boundary lengths up to the shape's capacity R G -- and its pair list.  Up to 512 points all lengths are crossed; at the
    widest shape each length meets {1, R, the limit} in both orders (a rectangle: the full crossing's host reference is slow)."""
    Ls = boundary_lengths(dim, limit)
    R, G = instantiations(dim, limit)[shape]
    cap = R * G
    nkeep = sum(L <= cap for L in Ls)   # (Ls ascends: the data set is its first nkeep series)
    assert Ls[nkeep - 1] == cap
    if cap <= 512:
        IJ = all_ordered_pairs(nkeep)
    else:
        assert cap == limit
        partners = [Ls.index(L) for L in (1, R, cap)]
        IJ = np.array([p for k in range(nkeep) for q in partners for p in ((k, q), (q, k))], dtype=np.int64)
    return nkeep, IJ


def univariate(curves):
    return [x[:, 0] for x in curves]


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
