"""Weighted Levenshtein distance on the host, a lane-by-lane restatement of the kernel's schedule, and the cost sets and data
sets of the weighted-Levenshtein tests.

Definition (annchor_amd.distances.WeightedLevenshtein).  An alphabet of A distinct symbols, 1 <= A <= 128; S a float64 [A, A]
substitution table (finite, >= 0, zero diagonal, symmetric bit for bit), g a float64 [A] insert / delete cost per symbol
(finite, >= 0); x_i and y_j are the symbols' codes.

    E(-1,-1) = 0      E(i,-1) = E(i-1,-1) + g[x_i]      E(-1,j) = E(-1,j-1) + g[y_j]      (left to right, one addition per step)
    E(i,j)   = min( E(i-1,j-1) + S[x_i][y_j],   E(i-1,j) + g[x_i],   E(i,j-1) + g[y_j] )
    wed(x,y) = E(n-1, m-1)                       wed(x, "") = E(n-1,-1)       wed("", "") = 0.0

Every cell is the min of three sums of fixed operands; min is exact and the additions are commutative, so every evaluation order
gives the same bits: `wed_loop` (the plain double loop), `wed_pairs_host` (anti-diagonals, many pairs at once) and `wed_lanes`
(the kernel's schedule) must agree bit for bit, and so must the kernel.  S is symmetric bit for bit, so the transposed matrix has
the same cells, which lets `wed_pairs_host` keep the SHORTER string of a pair on the vectorised axis and the kernel the LONGER one
on the lanes; test_wed_host.py checks both against `wed_loop`, which never swaps."""
import string
from collections import namedtuple

import numpy as np

from pool_cases import FIT_CFG, all_ordered_pairs   # noqa: F401
from seqdp_cases import WAVE, _lane_down, _lane_up

MAX_LENGTH = 2048
SHAPES = [(8, 16), (8, 64), (32, 64)]   # the kernel's (R rows per lane, G lanes per pair); a shape takes strings of up to R G symbols

# 128 distinct one-character symbols; an alphabet of A symbols is the first A of them
SYMBOLS = (string.ascii_lowercase + string.ascii_uppercase + string.digits + "".join(chr(k) for k in range(0x3b1, 0x3b1 + 66)))[:128]
assert len(set(SYMBOLS)) == 128

Costs = namedtuple("Costs", "alphabet S g")


def metric_of(costs):
    from annchor_amd.distances import WeightedLevenshtein

    return WeightedLevenshtein(costs.alphabet, costs.S, costs.g)


def kwargs_of(costs):
    return {"alphabet": costs.alphabet, "substitution": costs.S, "indel": costs.g}


# ---------------------------------------------------------------------------------------------------------- cost sets
def unit(A):
    return Costs(SYMBOLS[:A], 1.0 - np.eye(A), np.ones(A))


def dyadic(A, seed=1):
    """Integers / 4, so every sum is exact: off-diagonal S and g in {4 .. 8} / 4 = 1 .. 2, which is a metric (every cost is at most
    2 and every sum of two at least 2)."""
    rng = np.random.default_rng(seed)
    S = np.triu(rng.integers(4, 9, size=(A, A)), 1) / 4.0
    return Costs(SYMBOLS[:A], S + S.T, rng.integers(4, 9, size=A) / 4.0)


def ragged_costs(A, seed=2):
    """Random non-dyadic float64 costs that are a metric: the shortest-path closure of random positive weights over the A symbols
    and the gap as an (A+1)-th point.  The relaxation D = min(D, D[:, c] + D[c, :]) over every c is repeated until nothing
    changes, so at the end D[a][b] <= fl(D[a][c] + D[c][b]) holds for every triple in floating point, which is exactly what
    metric_violation() tests; every step keeps D symmetric bit for bit (a + b == b + a)."""
    rng = np.random.default_rng(seed)
    W = np.triu(rng.uniform(0.3, 3.0, size=(A + 1, A + 1)), 1)
    D = W + W.T
    while True:
        before = D.copy()
        for c in range(A + 1):
            D = np.minimum(D, D[:, c, None] + D[None, c, :])
        if np.array_equal(D, before):
            break
    assert np.array_equal(D, D.T) and np.all(np.diag(D) == 0.0)
    return Costs(SYMBOLS[:A], np.ascontiguousarray(D[:A, :A]), np.ascontiguousarray(D[:A, A]))


def nonmetric(A=4):
    """One triangle broken and nothing else: S[0][1] = 3 > S[0][2] + S[2][1] = 2, with indel costs of 4 so that no condition on g
    fails before it."""
    S = 1.0 - np.eye(A)
    S[0, 1] = S[1, 0] = 3.0
    return Costs(SYMBOLS[:A], S, np.full(A, 4.0))


# ---------------------------------------------------------------------------------------------------- host references
def codes_of(x, costs):
    at = {ch: a for a, ch in enumerate(costs.alphabet)}
    return np.array([at[ch] for ch in x], dtype=np.int64)


def gap_sums(codes, costs):
    """E(i, -1) of a string for i = 0 .. len-1: summed left to right, one addition per symbol."""
    out, e = [], 0.0
    for v in costs.g[codes].tolist():
        e = e + v
        out.append(e)
    return np.array(out, dtype=np.float64)


def wed_loop(x, y, costs):
    """The definition, cell by cell."""
    cx, cy = codes_of(x, costs).tolist(), codes_of(y, costs).tolist()
    S, g = costs.S.tolist(), costs.g.tolist()
    m = len(cy)
    prev = [0.0] * (m + 1)                       # row -1: E(-1, -1), E(-1, 0), ...
    for j in range(m):
        prev[j + 1] = prev[j] + g[cy[j]]
    left = 0.0                                   # E(i - 1, -1)
    for a in cx:
        ga, Sa = g[a], S[a]
        left = left + ga                         # E(i, -1)
        cur = [left] * (m + 1)
        e = left
        for j in range(m):
            e = min(prev[j] + Sa[cy[j]], prev[j + 1] + ga, e + g[cy[j]])
            cur[j + 1] = e
        prev = cur
    return np.float64(prev[m])


def levenshtein_loop(x, y):
    """Plain unit-cost Levenshtein on integers."""
    prev = list(range(len(y) + 1))
    for i, a in enumerate(x):
        cur = [i + 1]
        for j, b in enumerate(y):
            cur.append(min(prev[j] + (a != b), prev[j + 1] + 1, cur[j] + 1))
        prev = cur
    return prev[len(y)]


def _pool(X, costs):
    """The data set, once: codes end to end with one slack entry (as the loader keeps it), every symbol's indel cost, every
    member's running sums of them, the members' lengths and starts."""
    cod = [codes_of(x, costs) for x in X]
    lens = np.array([len(c) for c in cod], dtype=np.int64)
    pool = np.concatenate(cod + [np.zeros(1, dtype=np.int64)])
    gsum = np.concatenate([gap_sums(c, costs) for c in cod] + [np.zeros(1)])
    start = np.concatenate([[0], np.cumsum(lens)[:-1]])
    return pool, gsum, lens, start


def wed_pairs_host(X, IJ, costs):
    """wed(X[i], X[j]) for every row (i, j) of IJ -> float64 [len(IJ)].

    All pairs advance together, one anti-diagonal k = i + j per step.  A pair's state is one value per symbol of its shorter
    string (index i): diagonal k holds E(i, k - i), and E(i, -1) where k - i < 0.  The pairs are laid end to end in one flat
    array, ordered by their number of diagonals (descending), so the pairs still running are always a prefix of it.  A pair with
    an empty string has no cell: its value is the other string's last gap sum, 0.0 when both are empty."""
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(IJ.shape[0], dtype=np.float64)
    if IJ.shape[0] == 0:
        return out
    pool, gsum, lens, start = _pool(X, costs)
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
    ybase, ylen = start[B][pid], b[pid]
    first = I == 0
    last_el = seg[1:] - 1                            # the symbol of row a - 1
    fin = a + b - 2                                  # the diagonal of the corner cell (descending)
    d1 = E0.copy()                                   # diagonal k - 1
    d2 = E0.copy()                                   # diagonal k - 2
    res = np.zeros(P)
    live = P
    for k in range(int(fin[0]) + 1):
        E = seg[live]
        J = k - I[:E]
        valid = (J >= 0) & (J < ylen[:E])
        at = ybase[:E] + np.clip(J, 0, ylen[:E] - 1)
        sub = costs.S[X_[:E], pool[at]]
        f = first[:E]
        up = np.empty(E)                             # E(i - 1, j): the symbol before, one diagonal back; row -1 for i = 0
        up[1:] = d1[:E - 1]
        up[f] = gsum[at[f]]
        dg = np.empty(E)                             # E(i - 1, j - 1): the symbol before, two diagonals back
        dg[1:] = d2[:E - 1]
        dg[f] = np.where(J[f] > 0, gsum[np.maximum(at[f] - 1, 0)], 0.0)
        cur = np.minimum(np.minimum(dg + sub, up + GX[:E]), d1[:E] + gcost[at])
        cur[~valid] = E0[:E][~valid]                 # (j < 0: column -1; j >= m: cells nobody reads)
        lo = np.searchsorted(-fin[:live], -k, side="left")   # pairs lo .. live - 1 end on this diagonal
        res[lo:live] = cur[last_el[lo:live]]
        live = lo
        d2, d1 = d1, cur
        if live == 0:
            break
    out[where[order]] = res
    return out


# ------------------------------------------------------------------------------------------ the kernel's schedule, restated
def wed_lanes(X, IJ, costs, R, G):
    """k_wed<R, G> of csrc/wed.hip restated lane by lane: 64 lanes per wavefront (axis 1; axis 0 is the wavefronts, which do not
    interact and are advanced together), one pair per group of G lanes, the longer string on the lanes, R rows per lane, the code
    of y moving down the lanes and the strip (codes of y and E(-1, .)) moving up, column -1 and row -1 from the gap sums, every
    index clamped to 0 .. len-1 from both sides (an empty string reads entry 0, at worst the slack entry behind the pool), no
    step for a pair with an empty string, slots past the end of the list on pair (0, 0) storing nothing.  The table is indexed
    as the kernel does it: one flat image, the indel costs first, S behind them at A + code(x) A + code(y); the widest shape
    keeps no g[x_i] per row and reads it from the image per cell, which is the same value."""
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    P = len(IJ)
    val, gapsum, lens, off = _pool(X, costs)
    A = len(costs.alphabet)
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

    xo, d, gxr = [], [], []
    for r in range(R):
        row = at_(gl * R + r, n)
        code = val[xo_ + row]
        xo.append(code * A)
        gxr.append(lds[code])
        d.append(gapsum[xo_ + row])                    # column -1
    steps = np.where(m > 0, m + np.maximum(n - 1, 0) // R, 0).max(axis=1)   # (wave-uniform: the largest of the wavefront's pairs)
    bottom = d[R - 1].copy()
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
            yv = _lane_down(ycur)
            ycur_new = np.where(gl == 0, ybuf, yv)
            ybuf = _lane_up(ybuf)
            top = np.where(gl == 0, gbuf, top)         # row -1: E(-1, s)
            gbuf = _lane_up(gbuf)
            diag = top_prev
            jc = s - gl
            keep = alive[:, None]
            on = (jc >= 0) & (jc < m) & keep
            ycur = np.where(keep, ycur_new, ycur)
            top_prev = np.where(keep, top, top_prev)
            gy = lds[ycur]
            up, dg = top, diag
            for r in range(R):
                left = d[r]
                v = np.minimum(np.minimum(dg + lds[xo[r] + (A + ycur)], up + gxr[r]), left + gy)
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
def random_string(rng, L, A):
    return "".join(SYMBOLS[k] for k in rng.integers(0, A, size=L))


def one_of_each_length(lengths, A, seed):
    rng = np.random.default_rng(seed)
    return [random_string(rng, L, A) for L in lengths]


def boundary_lengths(shape):
    """The lengths the data set of shape number `shape` holds: 0, 1, and the strip and group boundaries up to its capacity."""
    Ls = [0, 1, 7, 8, 9, 16, 127, 128]
    if shape >= 1:
        Ls += [129, 511, 512]
    if shape >= 2:
        Ls += [32, 513, 2047, 2048]
    return Ls


def using_every_symbol(A, seed):
    """40 strings of 1 .. 40 symbols over A symbols that together use every symbol; string 0 is the last symbol alone and string 1
    the first and the last, so code A-1 meets code A-1 and code 0 meets code A-1."""
    rng = np.random.default_rng(seed)
    X = [random_string(rng, L, A) for L in range(1, 41)]
    X[0] = SYMBOLS[A - 1]
    X[1] = SYMBOLS[0] + SYMBOLS[A - 1]
    rest = rng.permutation(A)
    body = "".join(SYMBOLS[k] for k in rest)           # every symbol, 36 at a time at the head of the longest strings (37 .. 40 symbols)
    for k, lo in enumerate(range(0, A, 36)):
        part = body[lo:lo + 36]
        s = 39 - k
        X[s] = part + X[s][len(part):]
    assert set("".join(X)) == set(SYMBOLS[:A]) and [len(x) for x in X] == list(range(1, 41))
    return X


def clustered_strings(nx, lo, hi, A, seed, clusters=6, edits=0.25):
    """nx strings of lo .. hi symbols over A symbols in `clusters` clusters: a seed string per cluster, and per member random
    substitutions, insertions and deletions at a rate of `edits` per symbol."""
    rng = np.random.default_rng(seed)
    seeds = [random_string(rng, int(L), A) for L in rng.integers(lo + 5, hi - 5, size=clusters)]
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
        if lo <= len(out) <= hi:
            X.append("".join(out))
    return X


FIT_A = 12


def fit_costs():
    return ragged_costs(FIT_A, seed=21)


def fit_strings():
    """The fit tests' data: 240 strings in 6 clusters, 20..60 symbols over 12 symbols."""
    return clustered_strings(240, 20, 60, FIT_A, seed=31)


def brute_strings():
    """200 ragged strings of 20..60 symbols over 12 symbols."""
    return clustered_strings(200, 20, 60, FIT_A, seed=32)
