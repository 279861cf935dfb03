"""What the host side of the five k_seqdp measures (DTW, Frechet, ERP, MSM, TWE) shares: one vectorised sweep (`pairs_host`), one
lane-by-lane restatement of the kernel's schedule (`lanes`), and the builders of the tests' data sets.

A measure is a dynamic programme over the pair's cost matrix; the definitions are in dtw_cases, frechet_cases, erp_cases and
elastic_cases, beside their plain double loops, which are the independent statements the code here is checked against.  All
arithmetic is float64, every subtraction, product and addition rounded on its own; float32 input widens exactly.  What a measure
object supplies:

    cell(x, xp, y, yp, gx, gy, e, dg, up, left)   the cell (i, j) from x = x[i], xp = x[i-1], y = y[j], yp = y[j-1] as [..., dim]
                                                  points, e = i - j, and the neighbours dg = (i-1, j-1), up = (i-1, j),
                                                  left = (i, j-1); xp, yp are None unless `prev`; gx, gy are point_cost's
    prev                                          whether the cell reads x[i-1] and y[j-1] (the origin before the first point)
    point_cost(points)                            a cost per point, evaluated once (ERP's gap costs), or None
    edge(members)                                 column -1 / row -1 per point of the members laid end to end: +inf, or ERP's
                                                  running gap sums; the cell (-1, -1) is 0
    band(a, b)                                    DTW's band per pair from the two lengths (a <= b), or None
    finish(v)                                     the distance from the corner cell

Every cell has fixed operands and min and max are exact, so every evaluation order gives the same bits: a measure's loop (which
never swaps the members), `pairs_host` (anti-diagonals, many pairs at once, the SHORTER member on the vectorised axis), `lanes`
(the kernel's schedule, the LONGER member on the lanes) and the kernel must agree bit for bit."""
import numpy as np

from pool_cases import all_ordered_pairs

DIMS = (1, 2, 3, 4)


def as_curve(x):
    """[len, dim] float64; a 1-D member is a curve of dim 1."""
    x = np.asarray(x, dtype=np.float64)
    return x[:, None] if x.ndim == 1 else x


def _sq(a, b):
    """The sum over k = 0 .. dim-1, in that order, of t_k * t_k, t_k = a[k] - b[k]; it starts from the k = 0 product."""
    t = a[..., 0] - b[..., 0]
    c = t * t
    for k in range(1, a.shape[-1]):
        t = a[..., k] - b[..., k]
        c = c + t * t
    return c


def _dist(a, b):
    """ERP's and TWE's dist between arrays of points [..., dim] (or a point and the gap value), elementwise: |a - b| at dim 1, the
    correctly rounded square root of the sum of squares beyond.  NumPy rounds every subtraction, product and addition on its own."""
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
    """ERP's E(i, -1) of a member for i = 0 .. len-1: summed left to right, one addition per point."""
    g = _dist(as_curve(x), np.float64(gap)).tolist()
    out, e = [], 0.0
    for v in g:
        e = e + v
        out.append(e)
    return np.array(out, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------- the measures
class _Measure:
    prev = False

    def point_cost(self, points):
        return None

    def edge(self, members):
        return np.full(sum(len(s) for s in members), np.inf)

    def band(self, a, b):
        return None

    def finish(self, v):
        return v


class Dtw(_Measure):
    def __init__(self, window=None):
        self.window = window

    def cell(self, x, xp, y, yp, gx, gy, e, dg, up, left):
        return _sq(x, y) + np.minimum(np.minimum(left, up), dg)

    def band(self, a, b):
        return None if self.window is None else np.maximum(int(self.window), b - a)

    finish = staticmethod(np.sqrt)


class Frechet(_Measure):
    def cell(self, x, xp, y, yp, gx, gy, e, dg, up, left):
        return np.maximum(_sq(x, y), np.minimum(np.minimum(left, up), dg))

    finish = staticmethod(np.sqrt)


class Erp(_Measure):
    def __init__(self, gap=0.0):
        self.gap = np.float64(gap)

    def point_cost(self, points):
        return _dist(points, self.gap)

    def edge(self, members):
        return np.concatenate([gap_sums(s, self.gap) for s in members])

    def cell(self, x, xp, y, yp, gx, gy, e, dg, up, left):
        return np.minimum(np.minimum(dg + _dist(x, y), up + gx), left + gy)


def _msm_cost_v(v, a, b, c):
    between = ((a <= v) & (v <= b)) | ((a >= v) & (v >= b))
    return np.where(between, c, c + np.minimum(np.abs(v - a), np.abs(v - b)))


class Msm(_Measure):
    prev = True

    def __init__(self, c=1.0):
        self.c = np.float64(c)

    def cell(self, x, xp, y, yp, gx, gy, e, dg, up, left):
        x, xp, y, yp = x[..., 0], xp[..., 0], y[..., 0], yp[..., 0]
        return np.minimum(np.minimum(dg + np.abs(x - y), up + _msm_cost_v(x, xp, y, self.c)), left + _msm_cost_v(y, x, yp, self.c))


class Twe(_Measure):
    prev = True

    def __init__(self, nu=0.001, lam=1.0):
        self.nl, self.nu2 = np.float64(nu) + np.float64(lam), 2.0 * np.float64(nu)

    def cell(self, x, xp, y, yp, gx, gy, e, dg, up, left):
        match = dg + ((_dist(x, y) + _dist(xp, yp)) + self.nu2 * np.abs(e).astype(np.float64))
        return np.minimum(np.minimum(match, up + (_dist(x, xp) + self.nl)), left + (_dist(y, yp) + self.nl))


# ----------------------------------------------------------------------------------------- anti-diagonals, many pairs at once
def pairs_host(series, IJ, measure):
    """measure(series[i], series[j]) for every row (i, j) of IJ -> float64 [len(IJ)].

    All pairs advance together, one anti-diagonal k = i + j per step.  A pair's state is one value per point of its shorter member
    (index i): diagonal k holds the cell (i, k - i), and column -1 where k - i < 0.  The pairs are laid end to end in one flat
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
    band = measure.band(a, b)
    # the data set, once: points end to end, every point's cost, every member's column -1
    pool = np.concatenate(cur_, axis=0)
    assert pool.shape[1] == dim
    cost, edge = measure.point_cost(pool), measure.edge(cur_)
    start = np.concatenate([[0], np.cumsum(lens)[:-1]])
    seg = np.concatenate([[0], np.cumsum(a)])        # a pair's points: seg[p] .. seg[p + 1]
    pid = np.repeat(np.arange(P), a)
    I = np.arange(seg[-1]) - seg[pid]                # row i of each point
    xat = start[A][pid] + I
    first = I == 0
    byk = np.ascontiguousarray(pool.T)               # (one contiguous array per coordinate: x[..., k] of a gather's transpose)
    X, E0 = np.stack([col[xat] for col in byk]).T, edge[xat]   # E0: the cell (i, -1)
    GX = None if cost is None else cost[xat]
    XP = np.where(first[:, None], 0.0, pool[np.maximum(xat - 1, 0)]) if measure.prev else None   # x[i - 1]
    ybase, ylen = start[B][pid], b[pid]
    wel = None if band is None else band[pid]
    last_el = seg[1:] - 1                            # the point of row a - 1
    fin = a + b - 2                                  # the diagonal of the corner cell (descending)
    d1 = E0.copy()                                   # diagonal k - 1
    d2 = E0.copy()                                   # diagonal k - 2
    live = P
    for k in range(int(fin[0]) + 1):
        E = seg[live]
        J = k - I[:E]
        valid = (J >= 0) & (J < ylen[:E])
        if wel is not None:
            valid &= np.abs(I[:E] - J) <= wel[:E]
        at = ybase[:E] + np.clip(J, 0, ylen[:E] - 1)
        YP = np.where((J > 0)[:, None], pool[np.maximum(at - 1, 0)], 0.0) if measure.prev else None   # y[j - 1]
        f = seg[:live]                               # the pairs' first points: i = 0, j = k
        up = np.empty(E)                             # (i - 1, j): the point before, one diagonal back; row -1 for i = 0
        up[1:] = d1[:E - 1]
        up[f] = edge[at[f]]
        dg = np.empty(E)                             # (i - 1, j - 1): the point before, two diagonals back
        dg[1:] = d2[:E - 1]
        dg[f] = edge[np.maximum(at[f] - 1, 0)] if k > 0 else 0.0
        Y = np.stack([col[at] for col in byk])       # y[j], a coordinate at a time
        cur = measure.cell(X[:E], None if XP is None else XP[:E], Y.T, YP, None if GX is None else GX[:E],
                           None if cost is None else cost[at], I[:E] - J, dg, up, d1[:E])
        np.copyto(cur, E0[:E], where=~valid)         # (j < 0: column -1; j >= m or outside the band: +inf or cells nobody reads)
        lo = np.searchsorted(-fin[:live], -k, side="left")   # pairs lo .. live - 1 end on this diagonal
        out[order[lo:live]] = measure.finish(cur[last_el[lo:live]])
        live = lo
        d2, d1 = d1, cur
        if live == 0:
            break
    return out


def dtw_pairs_host(series, IJ, window=None):
    return pairs_host(series, IJ, Dtw(window))


def frechet_pairs_host(curves, IJ):
    return pairs_host(curves, IJ, Frechet())


def erp_pairs_host(series, IJ, gap=0.0):
    return pairs_host(series, IJ, Erp(gap))


def msm_pairs_host(series, IJ, c=1.0):
    return pairs_host(series, IJ, Msm(c))


def twe_pairs_host(series, IJ, nu=0.001, lam=1.0):
    return pairs_host(series, IJ, Twe(nu, lam))


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


def lanes(series, IJ, measure, R, G, carry_dist=False):
    """k_seqdp<T, DIM, R, G, Op> of csrc/seqdp.hip restated lane by lane: 64 lanes per wavefront (axis 1; axis 0 is the wavefronts,
    which do not interact and are advanced together), one pair per group of G lanes, the longer member on the lanes, R rows per
    lane, the point of y moving down the lanes and the strip (points of y and the row -1 under them) moving up, column -1 and
    row -1 from measure.edge, slots past the end of the list on pair (0, 0) storing nothing.  What MSM and TWE read besides: `xab`,
    the point above a lane's first row (x[l R - 1]; the origin on lane 0 of a group), loaded once; `yprev`, the value the lane's
    point of y had before this step's move (y[jc - 1]; the 0.0 it started from at jc = 0); and, with carry_dist (TWE's shapes
    that keep them in registers), `pd`, the R distances dist(x[row], y[jc - 1]) of the lane's last step, which start as
    dist(x[row], origin) and of which row r reads row r - 1's."""
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    P = len(IJ)
    cur_ = [as_curve(s) for s in series]
    dim = cur_[0].shape[1]
    lens = np.array([len(s) for s in cur_], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    val = np.concatenate(cur_, axis=0)
    edge = measure.edge(cur_)
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
    xr, d, gxr, pd = [], [], [], []
    for r in range(R):
        row = np.minimum(gl * R + r, n - 1)
        xr.append(val[xo + row])
        gxr.append(measure.point_cost(xr[r]))
        d.append(edge[xo + row])                       # column -1
        if carry_dist:
            pd.append(_dist(xr[r], origin))            # dist(x[row], y[-1])
    steps = (m + (n - 1) // R).max(axis=1)             # (wave-uniform: the largest of the wavefront's pairs)
    bottom = d[R - 1].copy()
    top_prev = np.where(gl == 0, 0.0, np.inf)
    ycur = np.zeros((W, WAVE, dim))
    yprev = np.zeros((W, WAVE, dim))
    ynext = val[yo + np.minimum(gl, m - 1)]
    gnext = edge[yo + np.minimum(gl, m - 1)]
    for s0 in range(0, int(steps.max()), G):
        at = yo + np.minimum(s0 + G + gl, m - 1)
        ybuf, ynext = ynext, val[at]
        gbuf, gnext = gnext, edge[at]
        for s in range(s0, min(s0 + G, int(steps.max()))):
            alive = (s < steps)[:, None]               # a wavefront past its own step count has left the loop
            top = _lane_down(bottom)
            ycur_new = np.where((gl == 0)[..., None], ybuf, _lane_down(ycur))
            ybuf = _lane_up(ybuf)
            top = np.where(gl == 0, gbuf, top)         # row -1
            gbuf = _lane_up(gbuf)
            diag = top_prev
            jc = s - gl
            on = (jc >= 0) & (jc < m) & alive
            yprev = np.where(alive[..., None], ycur, yprev)      # what ycur held before this step's move
            ycur = np.where(alive[..., None], ycur_new, ycur)
            top_prev = np.where(alive, top, top_prev)
            gy = measure.point_cost(ycur)
            if carry_dist:
                carry = _dist(xab, yprev)              # row 0 of the lane: dist(x[l R - 1], y[jc - 1])
            up, dg = top, diag
            for r in range(R):
                xp = xab if r == 0 else xr[r - 1]
                if carry_dist:                         # (what the cell recomputes from xp and yprev, handed down the rows)
                    assert np.array_equal(carry[on], _dist(xp, yprev)[on])
                    carry = pd[r]
                    pd[r] = np.where(on, _dist(xr[r], ycur), pd[r])
                left = d[r]
                v = measure.cell(xr[r], xp, ycur, yprev, gxr[r], gy, gl * R + r - jc, dg, up, left)
                dg, up = left, v
                d[r] = np.where(on, v, d[r])
            bottom = np.where(on, up, bottom)
    out = np.full(P, np.nan)
    res = np.take_along_axis(np.stack(d, axis=-1), ((n - 1) % R)[..., None], axis=-1)[..., 0]
    store = active & (gl == (n - 1) // R)
    assert store.sum() == P
    out[t[store]] = res[store]
    return out


def erp_lanes(series, IJ, gap, R, G):
    return lanes(series, IJ, Erp(gap), R, G)


def msm_lanes(series, IJ, c, R, G):
    return lanes(series, IJ, Msm(c), R, G)


def twe_lanes(series, IJ, nu, lam, R, G):
    dim = as_curve(series[0]).shape[1]
    return lanes(series, IJ, Twe(nu, lam), R, G, carry_dist=not (dim == 1 and R > 16))


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


def univariate(curves):
    return [x[:, 0] for x in curves]


def max_length(measure, dim):
    """The longest member the measure of that name takes at `dim`, read from the package."""
    from annchor_amd import distances

    f = getattr(distances, measure + "_max_length", None)
    return f(dim) if f else getattr(distances, measure.upper() + "_MAX_LENGTH")


def instantiations(measure, dim):
    """The kernel's shapes at `dim` (R rows per lane, G lanes per pair); a shape takes data sets whose longest member has up to
    R G points, the widest the measure's limit."""
    limit = max_length(measure, dim)
    assert limit % 64 == 0
    return [(8, 16), (8, 64), (limit // 64, 64)]


def boundary_lengths(measure, dim):
    """{R-1, R, R+1, 2R, GR-1, GR, GR+1} of every shape at `dim` that are within the limit, the limit and the limit minus 1; and
    1, the shortest partner."""
    limit = max_length(measure, dim)
    Ls = {1, limit - 1, limit}
    for R, G in instantiations(measure, dim):
        Ls.update(L for L in (R - 1, R, R + 1, 2 * R, G * R - 1, G * R, G * R + 1) if L <= limit)
    return sorted(Ls)


def boundary_case(measure, dim, shape):
    """The data set that runs shape number `shape` at `dim` -- the kernel is chosen by the data set's longest member, so it holds
    the boundary lengths up to the shape's capacity R G -- and its pair list.  Up to 512 points all lengths are crossed; at the
    widest shape each length meets {1, R, the limit} in both orders (a rectangle: the full crossing's host reference is slow)."""
    Ls = boundary_lengths(measure, dim)
    R, G = instantiations(measure, dim)[shape]
    cap = R * G
    nkeep = sum(L <= cap for L in Ls)   # (Ls ascends: the data set is its first nkeep members)
    assert Ls[nkeep - 1] == cap
    if cap <= 512:
        IJ = all_ordered_pairs(nkeep)
    else:
        assert cap == max_length(measure, dim)
        partners = [Ls.index(L) for L in (1, R, cap)]
        IJ = np.array([p for k in range(nkeep) for q in partners for p in ((k, q), (q, k))], dtype=np.int64)
    return nkeep, IJ


def lane_case(measure, dim, shape):
    """(lengths, pair list) of one shape for the lane model's tests: every length crossed with every length, minus the last pair
    at the narrow shape with 4 pairs per wavefront, so that its last wavefront has inactive slots."""
    R, G = instantiations(measure, dim)[shape]
    limit = max_length(measure, dim)
    Ls = [1, 2, R - 1, R, R + 1, 2 * R, G * R - 1, G * R] if shape < 2 else [1, R + 1, limit - 1, limit]
    IJ = all_ordered_pairs(len(Ls))
    if G < WAVE:
        IJ = IJ[:-1]
        assert len(IJ) % (WAVE // G) != 0
    return Ls, IJ
