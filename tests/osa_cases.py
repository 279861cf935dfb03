"""Optimal string alignment (OSA) on the host -- the definition as a loop, vectorised over anti-diagonals, and as a lane-by-lane
restatement of the kernel's schedule -- and the cost sets and data sets of the OSA tests.

Definition (annchor_amd.distances.OSA).  An alphabet of A distinct symbols, 1 <= A <= 128; S a float64 [A, A] substitution table
and g a float64 [A] insert / delete cost per symbol under WeightedLevenshtein's rules; T the cost of swapping two adjacent
symbols, a float >= 0, +inf for "no transpositions"; x_i and y_j are the symbols' codes.

    E(-1,-1) = 0      E(i,-1) = E(i-1,-1) + g[x_i]      E(-1,j) = E(-1,j-1) + g[y_j]
    E(i,j)   = min( E(i-1,j-1) + S[x_i][y_j],   E(i-1,j) + g[x_i],   E(i,j-1) + g[y_j],
                    E(i-2,j-2) + T   if i >= 1 and j >= 1 and x_i == y_{j-1} and x_{i-1} == y_j )
    osa(x,y) = E(n-1, m-1)      osa(x, "") = E(n-1,-1)      osa("", "") = 0.0

Row -1 and column -1 are legal sources of the fourth term.  Every cell is a min of sums of fixed operands; min is exact and the
additions are commutative, so every evaluation order gives the same bits: `osa_loop` (the definition, which never swaps its
arguments), `osa_pairs_host` (anti-diagonals, many pairs at once, the SHORTER string on the vectorised axis) and `osa_lanes` (the
kernel's schedule, the LONGER string on the lanes) must agree bit for bit, and so must the kernel.  The fourth term's condition
is symmetric in the two strings and S is symmetric, which is what lets the two swap.

This is the restricted form -- no substring is edited twice -- not the unrestricted Damerau-Levenshtein distance, and it is not a
metric: at unit costs osa("ca", "abc") = 3 > osa("ca", "ac") + osa("ac", "abc") = 2."""
from collections import namedtuple

import numpy as np

import wed_cases as wc
from pool_cases import FIT_CFG, all_ordered_pairs   # noqa: F401
from seqdp_cases import WAVE, _lane_down, _lane_up
from wed_cases import SYMBOLS, codes_of, one_of_each_length, using_every_symbol   # noqa: F401

NAME = "osa"
MAX_LENGTH = 1024
SHAPES = [(8, 16), (8, 64), (16, 64)]   # the kernel's (R rows per lane, G lanes per pair); a shape takes strings of up to R G symbols
INF = float("inf")

Costs = namedtuple("Costs", "alphabet S g T")   # wed_cases.Costs and the cost of a transposition


def with_transpose(costs, T):
    return Costs(costs.alphabet, costs.S, costs.g, float(T))


def wed_part(costs):
    """The same table as weighted-Levenshtein costs."""
    return wc.Costs(costs.alphabet, costs.S, costs.g)


def metric_of(costs):
    from annchor_amd.distances import OSA

    return OSA(costs.alphabet, costs.S, costs.g, costs.T)


def kwargs_of(costs):
    return {"alphabet": costs.alphabet, "substitution": costs.S, "indel": costs.g, "transpose": costs.T}


# ---------------------------------------------------------------------------------------------------------- cost sets
# dyadic: off-diagonal S and g are 1 .. 2 in quarters and every sum stays exact; ragged: the closure of weights drawn from 0.3 .. 3,
# no sum is exact.  Either T is cheaper than two substitutions often enough for swaps to win on random strings over 5 symbols.
DYADIC_T, RAGGED_T = 0.75, 0.7


def unit(A):
    return with_transpose(wc.unit(A), 1.0)


def dyadic(A, seed=1, T=DYADIC_T):
    return with_transpose(wc.dyadic(A, seed), T)


def ragged_costs(A, seed=2, T=RAGGED_T):
    return with_transpose(wc.ragged_costs(A, seed), T)


def below_every_cost(costs):
    """The same costs with T a non-dyadic value below every other cost of the set: a single adjacent swap then costs exactly T."""
    S, g = costs.S, costs.g
    off = S[~np.eye(len(g), dtype=bool)]
    low = min(float(g.min()), float(off.min()) if off.size else INF)
    assert low > 0.0
    return with_transpose(costs, low * 0.3)


FIT_T = 0.25   # below every cost of fit_costs (test_osa_host checks): a swap is the cheapest edit, and wins where the data has one


def fit_costs():
    return with_transpose(wc.fit_costs(), FIT_T)


# ---------------------------------------------------------------------------------------------------- host references
gap_sums = wc.gap_sums


def osa_loop(x, y, costs):
    """The definition, cell by cell; x on the rows, y on the columns, never swapped."""
    cx, cy = codes_of(x, costs).tolist(), codes_of(y, costs).tolist()
    S, g, T = costs.S.tolist(), costs.g.tolist(), costs.T
    m = len(cy)
    prev = [0.0] * (m + 1)                       # row i - 1: E(i-1, -1), E(i-1, 0), ...   (index j + 1)
    for j in range(m):
        prev[j + 1] = prev[j] + g[cy[j]]
    prev2 = None                                 # row i - 2; row -2 does not exist
    left = 0.0
    for i, a in enumerate(cx):
        ga, Sa = g[a], S[a]
        left = left + ga                         # E(i, -1)
        cur = [left] * (m + 1)
        e = left
        for j in range(m):
            b = cy[j]
            e = min(prev[j] + Sa[b], prev[j + 1] + ga, e + g[b])
            if i >= 1 and j >= 1 and a == cy[j - 1] and cx[i - 1] == b:
                e = min(e, prev2[j - 1] + T)     # E(i-2, j-2) at index j - 2 + 1
            cur[j + 1] = e
        prev2, prev = prev, cur
    return np.float64(prev[m])


def osa_int_loop(x, y):
    """Unit-cost OSA on integers over the full matrix, written on its own: d[i][j] for prefixes of i and j symbols."""
    n, m = len(x), len(y)
    d = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        d[i][0] = i
    for j in range(m + 1):
        d[0][j] = j
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            best = min(d[i - 1][j - 1] + (x[i - 1] != y[j - 1]), d[i - 1][j] + 1, d[i][j - 1] + 1)
            if i > 1 and j > 1 and x[i - 1] == y[j - 2] and x[i - 2] == y[j - 1]:
                best = min(best, d[i - 2][j - 2] + 1)
            d[i][j] = best
    return d[n][m]


def all_strings(A, longest):
    """Every string of 0 .. `longest` symbols over the first A symbols, the empty string first."""
    out, level = [""], [""]
    for _ in range(longest):
        level = [s + SYMBOLS[a] for s in level for a in range(A)]
        out += level
    return out


_pool = wc._pool   # codes end to end with one slack entry, running sums of g from 0.0 with one slack entry, lengths, starts


def osa_pairs_host(X, IJ, costs):
    """osa(X[i], X[j]) for every row (i, j) of IJ -> float64 [len(IJ)].

    wed_pairs_host's sweep with the fourth term: all pairs advance together, one anti-diagonal k = i + j per step; a pair's state
    is, per symbol of its shorter string (index i), E on the diagonals k - 1 .. k - 4: the cell (i-2, j-2) lies on diagonal k - 4,
    two symbols back.  Where k - i < 0 the state is column -1's running sum.  Row 0 has no fourth term; row 1 takes E(-1, j-2)
    from the other string's sums (0.0 at j = 1).  A pair with an empty string has no cell: its value is the other string's last
    sum, 0.0 when both are empty."""
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(IJ.shape[0], dtype=np.float64)
    if IJ.shape[0] == 0:
        return out
    pool, gsum, lens, start = _pool(X, wed_part(costs))
    T = costs.T
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
    X_, GX, E0 = pool[xat], gcost[xat], gsum[xat]    # E0: E(i, -1)
    XP = np.where(I > 0, pool[np.maximum(xat - 1, 0)], -1)   # x_{i-1}; row 0 has none
    ybase, ylen = start[B][pid], b[pid]
    first, second = I == 0, I == 1
    last_el = seg[1:] - 1                            # the symbol of row a - 1
    fin = a + b - 2                                  # the diagonal of the corner cell (descending)
    d1, d2, d3, d4 = E0.copy(), E0.copy(), E0.copy(), E0.copy()   # diagonals k - 1 .. k - 4
    res = np.zeros(P)
    live = P
    for k in range(int(fin[0]) + 1):
        E = seg[live]
        J = k - I[:E]
        valid = (J >= 0) & (J < ylen[:E])
        at = ybase[:E] + np.clip(J, 0, ylen[:E] - 1)
        ycode = pool[at]
        yprev = np.where(J >= 1, pool[np.maximum(at - 1, 0)], -2)   # y_{j-1}; column 0 has none
        sub = costs.S[X_[:E], ycode]
        f, g2 = first[:E], second[:E]
        up = np.empty(E)                             # E(i - 1, j): the symbol before, one diagonal back; row -1 for i = 0
        up[1:] = d1[:E - 1]
        up[f] = gsum[at[f]]
        dg = np.empty(E)                             # E(i - 1, j - 1): the symbol before, two diagonals back
        dg[1:] = d2[:E - 1]
        dg[f] = np.where(J[f] > 0, gsum[np.maximum(at[f] - 1, 0)], 0.0)
        tr = np.full(E, INF)                         # E(i - 2, j - 2): two symbols before, four diagonals back; row -1 for i = 1
        tr[2:] = d4[:max(E - 2, 0)]
        tr[g2] = np.where(J[g2] > 1, gsum[np.maximum(at[g2] - 2, 0)], 0.0)
        match = (X_[:E] == yprev) & (XP[:E] == ycode)   # (x_{i-1} = -1 on row 0 and y_{j-1} = -2 on column 0 match nothing)
        cur = np.minimum(np.minimum(dg + sub, up + GX[:E]), d1[:E] + gcost[at])
        cur = np.minimum(cur, np.where(match, tr + T, INF))
        cur[~valid] = E0[:E][~valid]                 # (j < 0: column -1; j >= m: cells nobody reads)
        lo = np.searchsorted(-fin[:live], -k, side="left")   # pairs lo .. live - 1 end on this diagonal
        res[lo:live] = cur[last_el[lo:live]]
        live = lo
        d4, d3, d2, d1 = d3, d2, d1, cur
        if live == 0:
            break
    out[where[order]] = res
    return out


# ------------------------------------------------------------------------------------------ the kernel's schedule, restated
X_SENTINEL, Y_SENTINEL = -1, -2   # the kernel's 0xfff8 and 0xfff0, as codes: lane 0's "row above" and column 0's "column before"


def osa_lanes(X, IJ, costs, R, G):
    """k_osa<R, G> of csrc/wed.hip restated lane by lane: wed_lanes' schedule -- 64 lanes per wavefront, one pair per group of G
    lanes, the longer string on the lanes, R rows per lane, the code of y moving down the lanes and the strip (codes of y and
    E(-1, .)) moving up, every index clamped from both sides with the slack entry behind the pool, no step for a pair with an
    empty string, the table as one flat image -- with what the fourth term adds:
      d2[r], the cell of row r two columns back, taking d[r] as a column is finished, and two values carried down the row loop so
        that row r reads the OLD d2[r-2];
      top_prev2 beside top_prev: `top` two steps ago, E(l R - 1, j-2), the source of a lane's row 1;
      a second boundary word, the lane above's d[R-2], moved down beside `bottom`, and its two-step history: E(l R - 2, j-2), the
        source of a lane's row 0; before a lane's first active step both words are the lane above's column -1;
      the last code of the lane above, moved down ONCE before the step loop, as x_{i-1} of a lane's row 0, lane 0 holding a
        sentinel that matches nothing (row -2 does not exist);
      the lane's `ycur` of the step before as y_{j-1}, replaced by a second sentinel on column 0;
      the term as a select: match ? source + T : +inf (the kernel packs the two codes of a row into one word and the two of a
        column into another and compares once; the condition is the same).
    The histories shift on every step a wavefront makes, whether or not the lane is on a column of its pair."""
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    P = len(IJ)
    val, gapsum, lens, off = _pool(X, wed_part(costs))
    A = len(costs.alphabet)
    T = costs.T
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

    xcode, d, d2, gxr = [], [], [], []
    for r in range(R):
        row = at_(gl * R + r, n)
        code = val[xo_ + row]
        xcode.append(code)
        gxr.append(lds[code])
        d.append(gapsum[xo_ + row])                    # column -1
        d2.append(np.full((W, WAVE), INF))             # read from column 1 on, when it holds column -1
    xabove = np.where(gl == 0, X_SENTINEL, _lane_down(xcode[R - 1]))
    steps = np.where(m > 0, m + np.maximum(n - 1, 0) // R, 0).max(axis=1)   # (wave-uniform: the largest of the wavefront's pairs)
    bottom = d[R - 1].copy()
    top_prev = np.zeros((W, WAVE))
    top_prev2 = np.full((W, WAVE), INF)
    top2_prev = np.full((W, WAVE), INF)
    top2_prev2 = np.full((W, WAVE), INF)
    ycur = np.zeros((W, WAVE), dtype=np.int64)
    ynext = val[yo + at_(gl, m)]
    gnext = gapsum[yo + at_(gl, m)]
    for s0 in range(0, int(steps.max()), G):
        at = yo + at_(s0 + G + gl, m)
        ybuf, ynext = ynext, val[at]
        gbuf, gnext = gnext, gapsum[at]
        for s in range(s0, min(s0 + G, int(steps.max()))):
            alive = s < steps                          # a wavefront past its own step count has left the loop
            keep = alive[:, None]
            top = _lane_down(bottom)
            top2 = _lane_down(d[R - 2])                # the second boundary word
            yv = _lane_down(ycur)
            yprev = ycur
            ycur_new = np.where(gl == 0, ybuf, yv)
            ybuf = _lane_up(ybuf)
            top = np.where(gl == 0, gbuf, top)         # row -1: E(-1, s)
            gbuf = _lane_up(gbuf)
            diag, src0, src1 = top_prev, top2_prev2, top_prev2
            top_prev2 = np.where(keep, top_prev, top_prev2)
            top_prev = np.where(keep, top, top_prev)
            top2_prev2 = np.where(keep, top2_prev, top2_prev2)
            top2_prev = np.where(keep, top2, top2_prev)
            ycur = np.where(keep, ycur_new, ycur)
            jc = s - gl
            on = (jc >= 0) & (jc < m) & keep
            gy = lds[ycur]
            yp = np.where(jc >= 1, yprev, Y_SENTINEL)
            up, dg, t0, t1, xprev = top, diag, src0, src1, xabove
            for r in range(R):
                left = d[r]
                v = np.minimum(np.minimum(dg + lds[xcode[r] * A + (A + ycur)], up + gxr[r]), left + gy)
                match = (xcode[r] == yp) & (xprev == ycur)
                v = np.minimum(v, np.where(match, t0 + T, INF))
                t0, t1 = t1, d2[r]
                d2[r] = np.where(on, left, d2[r])
                xprev = xcode[r]
                dg, up = left, v
                d[r] = np.where(on, v, d[r])
            bottom = np.where(on, up, bottom)
    out = np.full(P, np.nan)
    sel = (n - 1) % R                                  # (Python's -1 % R is R - 1; the kernel's is -1 and picks nothing: n = 0 gives 0.0)
    res = np.take_along_axis(np.stack(d, axis=-1), sel[..., None], axis=-1)[..., 0]
    res = np.where(n == 0, 0.0, res)
    store = active & (gl == np.maximum(n - 1, 0) // R)
    assert store.sum() == P
    out[t[store]] = res[store]
    return out


# ------------------------------------------------------------------------------------------------------------- data
def lane_lengths(shape):
    """The lengths of shape number `shape`: 0, 1, 2, R-1, R, R+1, 2R, GR-1, GR at the two small shapes, 0, 1, 2, R+1, 1023, 1024 at
    the widest; the empty string first AND last in the pool."""
    R, G = SHAPES[shape]
    Ls = [0, 1, 2, R - 1, R, R + 1, 2 * R, G * R - 1, G * R] if shape < 2 else [0, 1, 2, R + 1, MAX_LENGTH - 1, MAX_LENGTH]
    return Ls + [0]


def lane_case(shape):
    """(lengths, pair list) of one shape: every length crossed with every length in both orders, minus the last pair at the narrow
    shape with 4 pairs per wavefront, so that its last wavefront has inactive slots."""
    Ls = lane_lengths(shape)
    IJ = all_ordered_pairs(len(Ls))
    if SHAPES[shape][1] < WAVE:
        IJ = IJ[:-1]
        assert len(IJ) % (WAVE // SHAPES[shape][1]) != 0
    return Ls, IJ


SWAP_LENGTH = [128, 200, 200]   # the base strings' lengths: the first shape's capacity; 25 lanes and 4 strips; 13 lanes and 4 strips


def swap_base(shape, A=5, seed=70):
    """A string of SWAP_LENGTH[shape] symbols in which no two adjacent symbols are equal: every adjacent swap changes it."""
    rng = np.random.default_rng(seed + shape)
    codes = [int(rng.integers(0, A))]
    while len(codes) < SWAP_LENGTH[shape]:
        codes.append(int((codes[-1] + rng.integers(1, A)) % A))
    assert all(p != q for p, q in zip(codes, codes[1:]))
    return "".join(SYMBOLS[k] for k in codes)


def swapped(base):
    """base with positions (p, p+1) swapped, for p = 0 .. n-2: the cell (p+1, p+1) takes the fourth term, so the swaps end on every
    row 1 .. n-1 -- a lane's row 0 and its row 1 among them -- and at column 1."""
    return [base[:p] + base[p + 1] + base[p] + base[p + 2:] for p in range(len(base) - 1)]


def swap_case(shape):
    """The data set [base, every swapped string, one string of R G symbols] and the pairs (0, k), (k, 0) over the swapped strings.
    The last member makes the data set's longest string the shape's capacity, so that the device runs this shape on it."""
    R, G = SHAPES[shape]
    base = swap_base(shape)
    X = [base] + swapped(base) + one_of_each_length([R * G], 5, seed=75 + shape)
    k = np.arange(1, len(X) - 1)
    IJ = np.concatenate([np.stack([np.zeros_like(k), k], 1), np.stack([k, np.zeros_like(k)], 1)]).astype(np.int64)
    return X, IJ


def mutated_strings(nx, lo, hi, A, seed, clusters=6, edits=0.25, swaps=0.08):
    """wed_cases.clustered_strings with adjacent swaps as a fourth kind of mutation: after the edits, each position is swapped
    with its right neighbour at the rate `swaps` (a swapped pair is skipped over, so the swaps do not overlap)."""
    rng = np.random.default_rng(seed)
    seeds = [wc.random_string(rng, int(L), A) for L in rng.integers(lo + 5, hi - 5, size=clusters)]
    X = []
    while len(X) < nx:
        out = []
        for ch in seeds[len(X) % clusters]:
            u = rng.random()
            if u < edits / 3:
                continue                                           # deletion
            if u < 2 * edits / 3:
                ch = SYMBOLS[rng.integers(0, A)]                   # substitution
            out.append(ch)
            if rng.random() < edits / 3:
                out.append(SYMBOLS[rng.integers(0, A)])            # insertion
        p = 0
        while p + 1 < len(out):
            if rng.random() < swaps:
                out[p], out[p + 1] = out[p + 1], out[p]
                p += 2
            else:
                p += 1
        if lo <= len(out) <= hi:
            X.append("".join(out))
    return X


def fit_strings():
    """The fit tests' data: 240 strings in 6 clusters, 20..60 symbols over 12 symbols, mutated by edits and adjacent swaps."""
    return mutated_strings(240, 20, 60, wc.FIT_A, seed=31)


def brute_strings():
    """200 ragged strings of 20..60 symbols over 12 symbols, mutated the same way."""
    return mutated_strings(200, 20, 60, wc.FIT_A, seed=32)
