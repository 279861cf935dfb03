"""Affine-gap alignment distance on the host -- the definition as a loop, as an enumeration of alignments, vectorised over
anti-diagonals, and as a lane-by-lane restatement of the kernel's schedule -- and the cost sets of the affine-gap tests.

Definition (annchor_amd.distances.AffineGap).  An alphabet of A distinct symbols, 1 <= A <= 128; S a float64 [A, A] substitution
table under WeightedLevenshtein's rules, g a float64 [A] extension cost per symbol (finite, >= 0), o the cost of opening a gap
(finite, >= 0); x_i and y_j are the symbols' codes.

    H(-1,-1) = 0      P(-1,j) = +inf      Q(i,-1) = +inf      P(-1,-1) = Q(-1,-1) = +inf
    P(i,j) = min( P(i-1,j), H(i-1,j) + o ) + g[x_i]                     (x_i against a gap)
    Q(i,j) = min( Q(i,j-1), H(i,j-1) + o ) + g[y_j]                     (y_j against a gap)
    H(i,j) = min( H(i-1,j-1) + S[x_i][y_j],   P(i,j),   Q(i,j) )
    affine(x,y) = H(n-1, m-1)      affine(x, "") = P(n-1,-1) = ((o + g[x_0]) + g[x_1]) + ...      affine("", "") = 0.0

Every cell is a min of sums of fixed operands; min is exact and the additions are commutative, so every evaluation order gives
the same bits: `affine_loop` (the definition, which never swaps), `affine_pairs_host` (anti-diagonals, many pairs at once, the
SHORTER string on the vectorised axis) and `affine_lanes` (the kernel's schedule, the LONGER string on the lanes) must agree bit
for bit, and so must the kernel.  The transposed matrix swaps P and Q and holds the same H, which is what lets the two swap."""
from collections import namedtuple

import numpy as np

import wed_cases as wc
from pool_cases import FIT_CFG, all_ordered_pairs   # noqa: F401
from seqdp_cases import WAVE, _lane_down, _lane_up
from wed_cases import SYMBOLS, codes_of, one_of_each_length, using_every_symbol   # noqa: F401

NAME = "affine_gap"
MAX_LENGTH = 1024
SHAPES = [(8, 16), (8, 64), (16, 64)]   # the kernel's (R rows per lane, G lanes per pair); a shape takes strings of up to R G symbols
INF = float("inf")

Costs = namedtuple("Costs", "alphabet S g o")   # wed_cases.Costs and the opening cost


def with_open(costs, o):
    return Costs(costs.alphabet, costs.S, costs.g, float(o))


def wed_part(costs):
    """The same table as weighted-Levenshtein costs: g as the indel costs."""
    return wc.Costs(costs.alphabet, costs.S, costs.g)


def metric_of(costs):
    from annchor_amd.distances import AffineGap

    return AffineGap(costs.alphabet, costs.S, costs.g, costs.o)


def kwargs_of(costs):
    return {"alphabet": costs.alphabet, "substitution": costs.S, "extend": costs.g, "open": costs.o}


# ---------------------------------------------------------------------------------------------------------- cost sets
DYADIC_OPEN, RAGGED_OPEN = 0.75, 0.7   # dyadic: every sum stays exact; 0.7: no sum is


def dyadic(A, seed=1, o=DYADIC_OPEN):
    return with_open(wc.dyadic(A, seed), o)


def ragged_costs(A, seed=2, o=RAGGED_OPEN):
    return with_open(wc.ragged_costs(A, seed), o)


def fit_costs():
    return with_open(wc.fit_costs(), RAGGED_OPEN)


# ---------------------------------------------------------------------------------------------------- host references
def gap_sums(codes, costs):
    """H(i, -1) = P(i, -1) of a string for i = 0 .. len-1: ((o + g[x_0]) + g[x_1]) + ..., one addition per symbol."""
    out, e = [], costs.o
    for v in costs.g[codes].tolist():
        e = e + v
        out.append(e)
    return np.array(out, dtype=np.float64)


def affine_loop(x, y, costs):
    """The definition, cell by cell; x on the rows, y on the columns, never swapped."""
    cx, cy = codes_of(x, costs).tolist(), codes_of(y, costs).tolist()
    S, g, o = costs.S.tolist(), costs.g.tolist(), costs.o
    m = len(cy)
    Hp = [0.0] * (m + 1)                         # row -1: H(-1, -1), H(-1, 0), ...   (index j + 1)
    Pp = [INF] * (m + 1)                         # P(-1, .)
    e = o
    for j in range(m):
        e = e + g[cy[j]]
        Hp[j + 1] = e                            # H(-1, j) = Q(-1, j)
    left = o                                     # the running sum of column -1
    for a in cx:
        ga, Sa = g[a], S[a]
        left = left + ga
        Hc, Pc = [left] * (m + 1), [left] * (m + 1)   # column -1: H(i, -1) = P(i, -1)
        h, q = left, INF                         # H(i, j-1), Q(i, j-1); Q(i, -1) = +inf
        for j in range(m):
            gy = g[cy[j]]
            p = min(Pp[j + 1], Hp[j + 1] + o) + ga
            q = min(q, h + o) + gy
            h = min(Hp[j] + Sa[cy[j]], p, q)
            Hc[j + 1], Pc[j + 1] = h, p
        Hp, Pp = Hc, Pc
    return np.float64(Hp[m])


def affine_by_enumeration(x, y, costs):
    """The cheapest alignment, by walking every path of match (x_i with y_j), delete (x_i against a gap) and insert (y_j against a
    gap) moves from (0, 0) to (n, m): a match costs S, and every maximal run of equal gap moves costs o plus the g of its
    symbols.  Exponential: short strings only.  The sums are taken along the path, in another order than the recurrence's, so
    the costs must be dyadic for the two to agree bit for bit."""
    cx, cy = codes_of(x, costs).tolist(), codes_of(y, costs).tolist()
    S, g, o = costs.S.tolist(), costs.g.tolist(), costs.o
    n, m = len(cx), len(cy)
    best = [INF]

    def walk(i, j, last, cost):
        if i == n and j == m:
            best[0] = min(best[0], cost)
            return
        if i < n and j < m:
            walk(i + 1, j + 1, "M", cost + S[cx[i]][cy[j]])
        if i < n:
            walk(i + 1, j, "D", cost + (0.0 if last == "D" else o) + g[cx[i]])
        if j < m:
            walk(i, j + 1, "I", cost + (0.0 if last == "I" else o) + g[cy[j]])

    walk(0, 0, "M", 0.0)
    return np.float64(best[0])


def all_strings(A, longest):
    """Every string of 0 .. `longest` symbols over the first A symbols, the empty string first."""
    out, level = [""], [""]
    for _ in range(longest):
        level = [s + SYMBOLS[a] for s in level for a in range(A)]
        out += level
    return out


def _pool(X, costs):
    """The data set, once: codes end to end with one slack entry (as the loader keeps it), every symbol's extension cost, every
    member's running sums from o, the members' lengths and starts."""
    cod = [codes_of(x, costs) for x in X]
    lens = np.array([len(c) for c in cod], dtype=np.int64)
    pool = np.concatenate(cod + [np.zeros(1, dtype=np.int64)])
    gsum = np.concatenate([gap_sums(c, costs) for c in cod] + [np.zeros(1)])
    start = np.concatenate([[0], np.cumsum(lens)[:-1]])
    return pool, gsum, lens, start


def affine_pairs_host(X, IJ, costs):
    """affine(X[i], X[j]) for every row (i, j) of IJ -> float64 [len(IJ)].

    wed_pairs_host's sweep with three states: all pairs advance together, one anti-diagonal k = i + j per step; a pair's state
    is, per symbol of its shorter string (index i), H on the diagonals k - 1 and k - 2 and P and Q on the diagonal k - 1.  Where
    k - i < 0 the state is column -1's: H = P = the running sum from o, Q = +inf.  A pair with an empty string has no cell: its
    value is the other string's last sum, 0.0 when both are empty."""
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(IJ.shape[0], dtype=np.float64)
    if IJ.shape[0] == 0:
        return out
    pool, gsum, lens, start = _pool(X, costs)
    o = costs.o
    gcost = costs.g[pool]
    la, lb = lens[IJ[:, 0]], lens[IJ[:, 1]]
    swap = la > lb                                   # the shorter string on the vectorised axis
    A_all = np.where(swap, IJ[:, 1], IJ[:, 0])
    B_all = np.where(swap, IJ[:, 0], IJ[:, 1])
    none = lens[A_all] == 0
    longer = B_all[none]
    out[none] = np.where(lens[longer] > 0, gsum[start[longer] + np.maximum(lens[longer] - 1, 0)], 0.0)
    where = np.flatnonzero(~none)
    P = len(where)
    if P == 0:
        return out
    A, B = A_all[where], B_all[where]
    a, b = lens[A], lens[B]
    order = np.argsort(-(a + b), kind="stable")
    A, B, a, b = A[order], B[order], a[order], b[order]
    seg = np.concatenate([[0], np.cumsum(a)])        # a pair's symbols: seg[p] .. seg[p + 1]
    pid = np.repeat(np.arange(P), a)
    I = np.arange(seg[-1]) - seg[pid]                # row i of each symbol
    xat = start[A][pid] + I
    X_, GX, E0 = pool[xat], gcost[xat], gsum[xat]    # E0: H(i, -1)
    ybase, ylen = start[B][pid], b[pid]
    first = I == 0
    last_el = seg[1:] - 1                            # the symbol of row a - 1
    fin = a + b - 2                                  # the diagonal of the corner cell (descending)
    h1, h2 = E0.copy(), E0.copy()                    # H on the diagonals k - 1 and k - 2
    p1 = E0.copy()                                   # P on the diagonal k - 1 (column -1: P = H)
    q1 = np.full(len(E0), INF)                       # Q on the diagonal k - 1 (column -1: +inf)
    res = np.zeros(P)
    live = P
    for k in range(int(fin[0]) + 1):
        E = seg[live]
        J = k - I[:E]
        valid = (J >= 0) & (J < ylen[:E])
        at = ybase[:E] + np.clip(J, 0, ylen[:E] - 1)
        sub = costs.S[X_[:E], pool[at]]
        f = first[:E]
        up = np.empty(E)                             # H(i - 1, j): the symbol before, one diagonal back; row -1 for i = 0
        up[1:] = h1[:E - 1]
        up[f] = gsum[at[f]]
        up_p = np.empty(E)                           # P(i - 1, j); +inf on row -1
        up_p[1:] = p1[:E - 1]
        up_p[f] = INF
        dg = np.empty(E)                             # H(i - 1, j - 1): the symbol before, two diagonals back
        dg[1:] = h2[:E - 1]
        dg[f] = np.where(J[f] > 0, gsum[np.maximum(at[f] - 1, 0)], 0.0)
        p = np.minimum(up_p, up + o) + GX[:E]
        q = np.minimum(q1[:E], h1[:E] + o) + gcost[at]
        cur = np.minimum(np.minimum(dg + sub, p), q)
        cur[~valid] = E0[:E][~valid]                 # (j < 0: column -1; j >= m: cells nobody reads)
        p[~valid] = E0[:E][~valid]
        q[~valid] = INF
        lo = np.searchsorted(-fin[:live], -k, side="left")   # pairs lo .. live - 1 end on this diagonal
        res[lo:live] = cur[last_el[lo:live]]
        live = lo
        h2, h1, p1, q1 = h1, cur, p, q
        if live == 0:
            break
    out[where[order]] = res
    return out


# ------------------------------------------------------------------------------------------ the kernel's schedule, restated
def affine_lanes(X, IJ, costs, R, G):
    """k_affine<R, G> of csrc/wed.hip restated lane by lane: wed_lanes' schedule -- 64 lanes per wavefront, one pair per group of G
    lanes, the longer string on the lanes, R rows per lane, the code of y moving down the lanes and the strip (codes of y and
    H(-1, .)) moving up, every index clamped from both sides, no step for a pair with an empty string -- with what the affine
    states add: per row the Q of the column worked on last (+inf at first) beside its H, P flowing down the rows inside a step,
    and a boundary of TWO words between lanes (the bottom row's H and P); lane 0's top is the strip's H with P = +inf, and the
    diagonal boundary tracks H only.  Column -1 and row -1 come from sums that start from o."""
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    P = len(IJ)
    val, gapsum, lens, off = _pool(X, costs)
    A = len(costs.alphabet)
    o = costs.o
    lds = np.concatenate([costs.g, costs.S.ravel()])
    assert len(lds) == A + A * A
    PPW = WAVE // G
    W = (P + PPW - 1) // PPW
    lane = np.tile(np.arange(WAVE), (W, 1))
    gl, slot = lane & (G - 1), lane // G
    t = np.arange(W)[:, None] * PPW + slot
    active = t < P
    i = np.where(active, IJ[np.minimum(t, P - 1), 0], 0)
    j = np.where(active, IJ[np.minimum(t, P - 1), 1], 0)
    n, m = lens[i], lens[j]
    xo_, yo = off[i], off[j]
    sw = n < m                                         # the longer string on the lanes
    n, m, xo_, yo = np.where(sw, m, n), np.where(sw, n, m), np.where(sw, yo, xo_), np.where(sw, xo_, yo)

    def at_(k, length):
        return np.maximum(np.minimum(k, length - 1), 0)

    xo, h, q, gxr = [], [], [], []
    for r in range(R):
        row = at_(gl * R + r, n)
        code = val[xo_ + row]
        xo.append(code * A)
        gxr.append(lds[code])
        h.append(gapsum[xo_ + row])                    # column -1: H = P
        q.append(np.full((W, WAVE), INF))              # column -1: Q
    steps = np.where(m > 0, m + np.maximum(n - 1, 0) // R, 0).max(axis=1)   # (wave-uniform: the largest of the wavefront's pairs)
    bottom = h[R - 1].copy()
    bottom_p = np.full((W, WAVE), INF)
    top_prev = np.zeros((W, WAVE))
    ycur = np.zeros((W, WAVE), dtype=np.int64)
    ynext = val[yo + at_(gl, m)]
    gnext = gapsum[yo + at_(gl, m)]
    for s0 in range(0, int(steps.max()), G):
        at = yo + at_(s0 + G + gl, m)
        ybuf, ynext = ynext, val[at]
        gbuf, gnext = gnext, gapsum[at]
        for s in range(s0, min(s0 + G, int(steps.max()))):
            alive = s < steps                          # a wavefront past its own step count has left the loop
            top = _lane_down(bottom)
            top_p = _lane_down(bottom_p)
            yv = _lane_down(ycur)
            ycur_new = np.where(gl == 0, ybuf, yv)
            ybuf = _lane_up(ybuf)
            top = np.where(gl == 0, gbuf, top)         # row -1: H(-1, s)
            top_p = np.where(gl == 0, INF, top_p)      # row -1: P(-1, s)
            gbuf = _lane_up(gbuf)
            diag = top_prev
            jc = s - gl
            keep = alive[:, None]
            on = (jc >= 0) & (jc < m) & keep
            ycur = np.where(keep, ycur_new, ycur)
            top_prev = np.where(keep, top, top_prev)
            gy = lds[ycur]
            up, up_p, dg = top, top_p, diag
            for r in range(R):
                left = h[r]
                p = np.minimum(up_p, up + o) + gxr[r]
                qq = np.minimum(q[r], left + o) + gy
                v = np.minimum(np.minimum(dg + lds[xo[r] + (A + ycur)], p), qq)
                dg, up, up_p = left, v, p
                h[r] = np.where(on, v, h[r])
                q[r] = np.where(on, qq, q[r])
            bottom = np.where(on, up, bottom)
            bottom_p = np.where(on, up_p, bottom_p)
    out = np.full(P, np.nan)
    sel = (n - 1) % R                                  # (Python's -1 % R is R - 1; the kernel's is -1 and picks nothing: n = 0 gives 0.0)
    res = np.take_along_axis(np.stack(h, axis=-1), sel[..., None], axis=-1)[..., 0]
    res = np.where(n == 0, 0.0, res)
    store = active & (gl == np.maximum(n - 1, 0) // R)
    assert store.sum() == P
    out[t[store]] = res[store]
    return out


# ------------------------------------------------------------------------------------------------------------- data
def boundary_lengths(shape):
    """The lengths the data set of shape number `shape` holds: 0, 1, and the strip and group boundaries up to its capacity."""
    Ls = [0, 1, 7, 8, 9, 16, 127, 128]
    if shape >= 1:
        Ls += [129, 511, 512]
    if shape >= 2:
        Ls += [15, 17, 32, 513, 1023, 1024]
    return Ls


fit_strings, brute_strings, clustered_strings = wc.fit_strings, wc.brute_strings, wc.clustered_strings
