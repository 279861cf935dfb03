"""Constructed inputs for the device model kernels of csrc/model.hip (k_ols_bins, k_err_sort) and the prediction pass of
csrc/features.hip (k_predict_merge, k_sample_predict_scatter), an exact least-squares reference and NumPy restatements of the
prediction pass and the residual lists.  Host only: test_model_cases.py checks the cases and the reference on the CPU,
test_model_kernels_gpu.py drives the kernels with them.

A case is one call of fit_regression_device + fit_errors_device: feature rows [lb, ub, dad, anc] for EVERY pair of the fixture's
complete pair list, the sample request (pair positions in request order), the partition edges, and the facts it was built for
(claims: per-partition row counts, solver status, rank, null vectors, flags).  The anchor column is left 0 here: which pairs hold
an anchor is the engine's own state (the anchor override reads the anchor table by it), so the device test puts the engine's
column there.

The targets y are not free: y is the device metric of the sampled pair.  The fixtures' points therefore have coordinates that are
integers or halves (squared distances are exact in float64), every builder takes the distances Y of all pairs as an argument --
the host's by default, the device's own (evaluate_samples) in the device test -- and derives the features from them where the
case needs a relation between the two.  WHICH pairs a case samples never depends on Y, only on the points."""
import functools
from dataclasses import dataclass, field

import numpy as np

import row_paths_cases as C

U = 2.0 ** -53            # unit roundoff of float64
MAXBINS = 64              # common.h
ERR_CAP = 8192            # model.hip: residuals per partition the LDS sorter takes
OLS_RCOND = 1e-13         # model.hip: relative singular value below which the minimum-norm branch drops a direction
QR_LINE = 1e-10           # model.hip: |R_jj| <= QR_LINE * max |R_kk| sends a partition to the minimum-norm branch
EXACT_MAX_ROWS = 400      # partitions up to this many rows go through exact_ols
NO_LABEL = -1             # what download(F_LABELS) gives for the device's 255 ("in no error partition")
# gamma of the coefficient bound: 8 x the largest ratio  ||w_dgelsd - w|| / (u kappa (1 + kappa rho) ||w||)  that
# scipy.linalg.lstsq (dgelsd, the reference's solver) attains over the full-rank partitions of the cases below, and not less than
# 1.  Measured by test_model_cases.py::test_dgelsd_stays_inside_the_bound_and_fixes_gamma (scipy 1.15, OpenBLAS): 27.5 on the
# seven-row filler partition of full_n4 and 13.6 on the 300 rows of full_n300 -- the SVD-based drivers (gelsd, gelss) lose two
# digits there that a QR solve of the same centred data keeps (ratio 0.05) -- and 0.08 .. 1.7 on every other partition.
GAMMA = 220.0

CLASSES = {"short": C.CLASSES["short"], "mid": C.CLASSES["mid"]}
N_LINE = 48               # short class: points 0 .. 47 (before the shuffle) lie on a line at half-integer abscissae


# ------------------------------------------------------------------------------------------------------------ fixtures
@functools.lru_cache(maxsize=None)
def points(cls):
    """float64 [nx][2], coordinates integers or halves.
    short: 48 points on the x axis at distinct half-integer abscissae (their pair distances are exact halves, with massive
           ties), 47 points with integer coordinates in [-40, 40]^2, and two duplicates of earlier points (pairs of distance 0);
    mid:   700 points of a 27 x 26 integer lattice (few distinct distances: tie groups) and one duplicate.
    The order is shuffled, so that the pairs of one kind are spread over the pair list."""
    nx = CLASSES[cls]
    rng = np.random.default_rng(1000 + nx)
    if cls == "short":
        P = np.zeros((nx, 2))
        P[:N_LINE, 0] = rng.permutation(60)[:N_LINE] / 2.0
        cells = rng.permutation(81 * 81)[:nx - N_LINE - 2]
        P[N_LINE:nx - 2, 0], P[N_LINE:nx - 2, 1] = cells // 81 - 40.0, cells % 81 - 40.0
        P[N_LINE:nx - 2, 1] += (P[N_LINE:nx - 2, 1] == 0)          # keep them off the line
        P[nx - 2], P[nx - 1] = P[0], P[N_LINE]
        kind = np.r_[np.zeros(N_LINE, int), np.ones(nx - N_LINE - 2, int), [2, 2]]
    else:
        cells = rng.permutation(27 * 26)[:nx - 1]
        P = np.stack([cells // 26, cells % 26], axis=1).astype(np.float64)
        P = np.concatenate([P, P[:1]])
        kind = np.r_[np.ones(nx - 1, int), [2]]
    order = rng.permutation(nx)
    P, kind = P[order], kind[order]
    P.setflags(write=False)
    points_kind[cls] = kind
    return P


points_kind = {}          # cls -> per point: 0 on the line, 1 general, 2 a duplicate of another point


@functools.lru_cache(maxsize=None)
def pairs(cls):
    """IJs int64 [n][2] of the complete pair list as the library lays it out."""
    return C.complete_index(CLASSES[cls])[2]


@functools.lru_cache(maxsize=None)
def host_distances(cls):
    """float64 [n]: the Euclidean distance of every pair as the device computes it (float64 sum of squared differences, which is
    exact on these points, then one correctly rounded square root)."""
    P, IJ = points(cls), pairs(cls)
    d = P[IJ[:, 0]] - P[IJ[:, 1]]
    Y = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    Y.setflags(write=False)
    return Y


def _pair_sets(cls):
    """positions of (pairs of two points on the line, pairs of distance 0, every other pair)."""
    points(cls)
    k, IJ = points_kind[cls], pairs(cls)
    P = points(cls)
    zero = np.flatnonzero((P[IJ[:, 0]] == P[IJ[:, 1]]).all(axis=1))
    line = np.flatnonzero((k[IJ[:, 0]] == 0) & (k[IJ[:, 1]] == 0))
    rest = np.setdiff1d(np.arange(IJ.shape[0]), np.concatenate([zero, line]))
    return line, zero, rest


# ------------------------------------------------------------------------------------------------------------ the cases
@dataclass
class Case:
    name: str
    cls: str
    features: np.ndarray          # float64 [n][4]: lb, ub, dad, 0
    pos: np.ndarray               # int64 [m]: the sample request, in request order
    edges: np.ndarray             # float64 [nb + 1]
    rows: list                    # samples per regression partition (lo < dad <= hi)
    err_rows: list                # samples per residual partition (lo <= dad <= hi)
    status: list                  # k_ols_bins' status per partition: 0 solved, 2 fewer than three rows
    rank: list                    # rank of the centred partition (None: refused, or too long for the exact reference)
    null: dict = field(default_factory=dict)    # partition -> null vectors of the centred partition (not normalised)
    qr_deficient: dict = field(default_factory=dict)   # partition -> True: takes the minimum-norm branch
    ref_rank: dict = field(default_factory=dict)       # partition -> rank the exact reference uses where it is not `rank`
    flags: tuple = (0, 0, 0)      # the sticky flags after both fits (sample step, regression, residual lists)
    order: str = "sorted"         # "shuffled": request order is not position order

    @property
    def nb(self):
        return len(self.edges) - 1

    @property
    def m(self):
        return len(self.pos)


def _generic(y, rng, dlo, dhi):
    """rows [lb, ub, dad] loosely tied to y the way a pair's bounds are (full rank, condition number 10 .. 100, residual about a
    tenth of y), dad uniform in (dlo, dhi)."""
    m = len(y)
    t = y / 8.0
    return np.stack([0.7 * t - rng.uniform(0, 1, m), 1.3 * t + rng.uniform(0, 1, m) + 1.0,
                     dlo + (dhi - dlo) * rng.uniform(0.02, 0.98, m)], axis=1)


def _background(cls, rng, edges, Y):
    """feature rows of every pair: bounds around the pair's own distance (so the clip binds on both sides for some pairs), dad
    spread over the partitions, beyond the outer edges, and exactly ON every finite edge for a tenth of the pairs."""
    n = len(Y)
    fin = edges[np.isfinite(edges)]
    lo, hi = (fin.min(), fin.max()) if fin.size else (0.0, 20.0)
    w = max(hi - lo, 1.0)
    F = np.zeros((n, 4))
    F[:, :3] = _generic(np.asarray(Y), rng, lo - 0.3 * w - 1.0, hi + 0.3 * w + 1.0)
    if fin.size:
        on = rng.random(n) < 0.1
        F[on, 2] = fin[np.arange(int(on.sum())) % fin.size]
    return F


def _filler(cls, Y, rng, avoid, k, dlo, dhi):
    """k plain full-rank samples with dad in (dlo, dhi): (positions, rows)."""
    _, _, rest = _pair_sets(cls)
    pos = rng.permutation(np.setdiff1d(rest, avoid))[:k]
    return pos, _generic(np.asarray(Y)[pos], rng, dlo, dhi)


def _null_mp(rows):
    """null vectors of the centred rows, from exact arithmetic: the cross product for rank 2, two vectors orthogonal to the one
    direction for rank 1."""
    import mpmath as mp
    with mp.workdps(60):
        R = [[mp.mpf(float(v)) for v in r] for r in rows]
        mean = [sum(r[k] for r in R) / len(R) for k in range(3)]
        Rc = [[r[k] - mean[k] for k in range(3)] for r in R]
        nz = [r for r in Rc if any(v != 0 for v in r)]
        a = nz[0]
        cross = lambda p, q: [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]  # noqa: E731
        for b in nz[1:]:
            v = cross(a, b)
            if any(x != 0 for x in v):
                s = mp.sqrt(sum(x * x for x in v))
                return [np.array([float(x / s) for x in v])]
        e = [mp.mpf(1), mp.mpf(0), mp.mpf(0)] if abs(a[0]) <= min(abs(a[1]), abs(a[2])) else [mp.mpf(0), mp.mpf(1), mp.mpf(0)] \
            if abs(a[1]) <= abs(a[2]) else [mp.mpf(0), mp.mpf(0), mp.mpf(1)]
        v1 = cross(a, e)
        v2 = cross(a, v1)
        out = []
        for v in (v1, v2):
            s = mp.sqrt(sum(x * x for x in v))
            out.append(np.array([float(x / s) for x in v]))
        return out


def _exact_rows(y, rng, ub, dad, w=(4.0, 0.75, -0.25), c=1.5):
    """lb such that y = w0 lb + w1 ub + w2 dad + c up to the rounding of lb: a (nearly) zero-residual partition, the features
    derived from the targets."""
    return np.stack([(y - w[1] * ub - w[2] * dad - c) / w[0], ub, dad], axis=1)


SHORT_CASES = ("full_n4", "full_n257", "full_n300", "shuffled", "offset_1e6", "scaled_1e-6", "half_integer", "near_dep_1e-6",
               "near_dep_1e-9", "n3", "const_dad", "lb_zero", "ub_2dad", "two_deps", "all_const", "dup_rows", "near_dep_1e-11",
               "refusals", "nb1", "nb64", "finite_outer", "inner_edge", "lowest_edge")
MID_CASES = ("sort_8192", "sort_8193", "sort_5000", "sort_ties")
ALL_CASES = SHORT_CASES + MID_CASES
FULL_RANK_CASES = ("full_n4", "full_n257", "full_n300", "shuffled", "offset_1e6", "scaled_1e-6", "half_integer", "near_dep_1e-6",
                   "near_dep_1e-9", "near_dep_1e-11", "nb1", "nb64", "finite_outer", "inner_edge", "lowest_edge")
DEFICIENT_CASES = ("n3", "const_dad", "lb_zero", "ub_2dad", "two_deps", "all_const", "dup_rows")
N_TARGET = {"full_n4": 4, "full_n257": 257, "full_n300": 300, "shuffled": 150, "offset_1e6": 60, "scaled_1e-6": 60,
            "half_integer": 80, "near_dep_1e-6": 50, "near_dep_1e-9": 50, "near_dep_1e-11": 50, "n3": 3, "const_dad": 20,
            "lb_zero": 20, "ub_2dad": 20, "two_deps": 20, "all_const": 10, "dup_rows": 6}
N_FILL = 7


def case_class(name):
    return "mid" if name in MID_CASES else "short"


def build(name, Y=None):
    """The case `name`; Y: the distance of every pair of its class (None: the host's)."""
    cls = case_class(name)
    Y = host_distances(cls) if Y is None else np.asarray(Y, dtype=np.float64)
    rng = np.random.default_rng(ALL_CASES.index(name) + 77)
    line, zero, rest = _pair_sets(cls)
    n = len(Y)

    def finish(pos, srows, edges, bg_map=None, **claims):
        edges = np.asarray(edges, dtype=np.float64)
        F = _background(cls, rng, edges if bg_map is None else bg_map[1](edges), Y)
        if bg_map is not None:
            F[:, :3] = bg_map[0](F[:, :3])
        pos = np.asarray(pos, dtype=np.int64)
        assert len(np.unique(pos)) == len(pos) and len(pos) == len(srows)
        F[pos, :3] = srows
        if claims.get("order", "sorted") == "sorted":
            pos = np.sort(pos)
        return Case(name=name, cls=cls, features=F, pos=pos, edges=edges, **claims)

    # ---- one target partition (-inf, T] and a plain filler partition (T, inf)
    if name in N_TARGET:
        k = N_TARGET[name]
        pool = line if name == "half_integer" else rest
        tpos = rng.permutation(pool)[:k]
        if name != "shuffled":
            tpos = np.sort(tpos)
        y = Y[tpos]
        T, fmap = 10.0, None
        X = _generic(y, rng, 1.0, 9.0)
        rank, null, qrd, refr = 3, {}, {}, {}
        if name == "offset_1e6":       # cancellation in the centring: unit spread at 10^6
            fmap = (lambda A: A + 1e6, lambda e: e - 1e6)
            X, T = X + 1e6, T + 1e6
        elif name == "scaled_1e-6":
            fmap = (lambda A: A * 1e-6, lambda e: e * 1e6)
            X, T = X * 1e-6, T * 1e-6
        elif name == "half_integer":   # y is a half by construction of the line; so are the features: massive ties
            h = lambda: rng.integers(0, 5, k) / 2.0   # noqa: E731
            X = np.stack([np.floor(y) - h(), np.ceil(y) + h() + 0.5, 2.0 + rng.integers(0, 13, k) / 2.0], axis=1)
        elif name.startswith("near_dep"):
            # ub = 2 dad perturbed: condition number ~ 3 / perturbation.  The targets lie on a plane up to the rounding of lb, so
            # that the bound's kappa^2 rho term stays small and the bound says something at these condition numbers.
            eps = float(name.split("_")[-1])
            dad = 1.0 + 8.0 * rng.uniform(0.02, 0.98, k)
            ub = 2.0 * dad * (1.0 + eps * rng.choice([-1.0, 1.0], k))
            X = _exact_rows(y, rng, ub, dad)
            if eps < 1e-10:            # below the QR's line, above OLS_RCOND: the minimum-norm branch keeps all three directions
                qrd, refr = {0: True}, {0: 3}
        elif name == "n3":
            rank, null, qrd = 2, {0: _null_mp(X)}, {0: True}
        elif name == "const_dad":
            X[:, 2] = 4.5
            rank, null, qrd = 2, {0: [np.array([0.0, 0.0, 1.0])]}, {0: True}
        elif name == "lb_zero":
            X[:, 0] = 0.0
            rank, null, qrd = 2, {0: [np.array([1.0, 0.0, 0.0])]}, {0: True}
        elif name == "ub_2dad":
            X[:, 1] = 2.0 * X[:, 2]
            rank, null, qrd = 2, {0: [np.array([0.0, 1.0, -2.0])]}, {0: True}
        elif name == "two_deps":
            X[:, 0], X[:, 1] = 3.0, 2.0 * X[:, 2]
            rank, null, qrd = 1, {0: [np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, -2.0])]}, {0: True}
        elif name == "all_const":
            X[:] = [1.25, 7.5, 4.0]
            rank, null, qrd = 0, {0: [np.eye(3)[0], np.eye(3)[1], np.eye(3)[2]]}, {0: True}
        elif name == "dup_rows":
            X[:] = np.where((np.arange(k) % 2 == 0)[:, None], X[0], X[1])
            rank, null, qrd = 1, {0: _null_mp(X)}, {0: True}
        if fmap is None:
            fpos, frows = _filler(cls, Y, rng, tpos, N_FILL, T + 1.0, T + 9.0)
        else:
            fpos, frows = _filler(cls, Y, rng, tpos, N_FILL, 11.0, 19.0)
            frows = fmap[0](frows)
        pos, rows = np.concatenate([tpos, fpos]), np.concatenate([X, frows])
        if name == "shuffled":
            p = rng.permutation(len(pos))
            pos, rows = pos[p], rows[p]
        return finish(pos, rows, [-np.inf, T, np.inf], bg_map=fmap, rows=[k, N_FILL], err_rows=[k, N_FILL], status=[0, 0],
                      rank=[rank, 3], null=null, qr_deficient=qrd, ref_rank=refr, order="shuffled" if name == "shuffled" else "sorted")

    if name == "refusals":     # partitions of 5, 0, 1, 2 and 8 rows: three refusals, and an empty residual partition
        counts, edges = [5, 0, 1, 2, 8], [-np.inf, 2.0, 4.0, 6.0, 8.0, np.inf]
        pos = np.sort(rng.permutation(rest)[:sum(counts)])
        y, rows, at = Y[pos], [], 0
        for b, kb in enumerate(counts):
            rows.append(_generic(y[at:at + kb], rng, 2.0 * b + 0.1, 2.0 * b + 1.9))
            at += kb
        return finish(pos, np.concatenate(rows), edges, rows=counts, err_rows=counts, status=[0, 2, 2, 2, 0],
                      rank=[3, None, None, None, 3], flags=(0, 2, 1))

    if name == "nb1":
        pos = np.sort(rng.permutation(rest)[:40])
        return finish(pos, _generic(Y[pos], rng, -5.0, 30.0), [-np.inf, np.inf], rows=[40], err_rows=[40], status=[0], rank=[3])

    if name == "nb64":         # MAXBINS partitions of five rows; the request walks round the partitions
        edges = np.r_[-np.inf, np.arange(1.0, 64.0), np.inf]
        pos = np.sort(rng.permutation(rest)[:320])
        part = np.arange(320) % 64
        rows = _generic(Y[pos], rng, 0.0, 1.0)
        rows[:, 2] += part
        return finish(pos, rows, edges, rows=[5] * 64, err_rows=[5] * 64, status=[0] * 64, rank=[3] * 64)

    if name in ("finite_outer", "inner_edge", "lowest_edge"):
        if name == "inner_edge":
            # three samples exactly on the inner edge: partition 0 of the regression, BOTH residual lists (err_ptr[nb] = m + 3)
            edges, counts = [-np.inf, 5.0, np.inf], [10, 8]
            pos = np.sort(rng.permutation(rest)[:18])
            rows = np.concatenate([_generic(Y[pos[:10]], rng, 1.0, 5.0), _generic(Y[pos[10:]], rng, 5.0, 9.0)])
            rows[[2, 5, 9], 2] = 5.0
            return finish(pos, rows, edges, rows=counts, err_rows=[10, 11], status=[0, 0], rank=[3, 3])
        edges = [2.0, 5.0, 9.0]
        if name == "finite_outer":
            # three samples below and three above every partition (no regression partition, prediction 0, no residual list)
            pos = np.sort(rng.permutation(rest)[:27])
            rows = np.concatenate([_generic(Y[pos[:12]], rng, 2.0, 5.0), _generic(Y[pos[12:21]], rng, 5.0, 9.0),
                                   _generic(Y[pos[21:24]], rng, -3.0, 2.0), _generic(Y[pos[24:]], rng, 9.0, 14.0)])
            return finish(pos, rows, edges, rows=[12, 9], err_rows=[12, 9], status=[0, 0], rank=[3, 3])
        # lowest_edge: two samples exactly on the lowest finite edge, one of them a pair of distance 0 -- no regression
        # partition, prediction 0, FIRST residual list, residuals y - 0 (a +0.0 among them); and one on the highest edge
        pos = np.concatenate([np.sort(rng.permutation(rest)[:19]), zero[:1]])
        rows = np.concatenate([_generic(Y[pos[:10]], rng, 2.0, 5.0), _generic(Y[pos[10:18]], rng, 5.0, 9.0),
                               _generic(Y[pos[18:]], rng, 0.0, 1.0)])
        rows[17, 2] = 9.0
        rows[18:, 2] = 2.0
        return finish(pos, rows, edges, rows=[10, 8], err_rows=[12, 8], status=[0, 0], rank=[3, 3])

    # ---- the residual sorter (mid class): one long partition (-inf, T] and a filler
    if name in ("sort_8192", "sort_8193", "sort_5000"):
        k = int(name.split("_")[1])
        pos = np.sort(rng.permutation(rest)[:k + 40])
        p = rng.permutation(k + 40)
        rows = np.concatenate([_generic(Y[pos[p[:k]]], rng, 1.0, 9.0), _generic(Y[pos[p[k:]]], rng, 11.0, 19.0)])
        rows = rows[np.argsort(p)]
        return finish(pos, rows, [-np.inf, 10.0, np.inf], rows=[k, 40], err_rows=[k, 40], status=[0, 0], rank=[None, 3],
                      flags=(0, 0, 2 if k > ERR_CAP else 0))
    if name == "sort_ties":
        # rows that depend on the pair's squared lattice distance alone: pairs of equal distance have identical rows and identical
        # targets, hence identical residuals -- tie groups of hundreds; five samples on the lowest finite edge (prediction 0,
        # residual y) with a +0.0 among them
        P, IJ = points(cls), pairs(cls)
        perm = rng.permutation(rest)
        pos = np.concatenate([np.sort(perm[:3050]), zero[:1], perm[3050:3054]])
        d = P[IJ[pos, 0]] - P[IJ[pos, 1]]
        q = d[:, 0] ** 2 + d[:, 1] ** 2
        yh = np.sqrt(q)
        rows = np.stack([np.floor(yh), np.ceil(yh) + 1.0, 3.0 + q % 7.0], axis=1)
        rows[3000:3050, 2] += 8.0
        rows[3050:, 2] = 2.0
        return finish(pos, rows, [2.0, 10.0, 18.0], rows=[3000, 50], err_rows=[3005, 50], status=[0, 0], rank=[None, None])
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------------------ exact least squares
def exact_ols(X, y, rank=3, dps=60):
    """Ordinary least squares with intercept of float64 rows X [n][3] on y [n] in `dps`-digit arithmetic (the float64 inputs
    convert exactly): (w, c) as lists of mpmath numbers.  rank 3: the 3 x 3 normal equations of the centred data; rank < 3, GIVEN
    (by the case's construction, not by a threshold): the minimum-norm solution pinv(Xc) yc from the singular value
    decomposition, the `rank` largest singular values kept."""
    import mpmath as mp
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = X.shape[0]
    assert X.shape == (n, 3) and y.shape == (n,) and n <= EXACT_MAX_ROWS
    with mp.workdps(dps):
        Xm = [[mp.mpf(float(v)) for v in r] for r in X]
        ym = [mp.mpf(float(v)) for v in y]
        mx = [sum(r[k] for r in Xm) / n for k in range(3)]
        my = sum(ym) / n
        Xc = [[r[k] - mx[k] for k in range(3)] for r in Xm]
        yc = [v - my for v in ym]
        if rank == 3:
            G = mp.matrix(3, 3)
            g = mp.matrix(3, 1)
            for a in range(3):
                g[a] = sum(Xc[i][a] * yc[i] for i in range(n))
                for b in range(a, 3):
                    G[a, b] = G[b, a] = sum(Xc[i][a] * Xc[i][b] for i in range(n))
            w = list(mp.lu_solve(G, g))
        elif rank == 0:
            w = [mp.mpf(0)] * 3
        else:
            Uu, S, V = mp.svd_r(mp.matrix(Xc))          # Xc = Uu diag(S) V, S descending
            w = [mp.mpf(0)] * 3
            for i in range(rank):
                coef = sum(Uu[r, i] * yc[r] for r in range(n)) / S[i]
                w = [w[k] + coef * V[i, k] for k in range(3)]
        c = my - sum(mx[k] * w[k] for k in range(3))
        return w, c


def centred_exact(X, y, dps=60):
    """(Xc, yc, mean_x, mean_y): centred in exact arithmetic, then rounded to float64."""
    import mpmath as mp
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = X.shape[0]
    with mp.workdps(dps):
        mx = [sum(mp.mpf(float(v)) for v in X[:, k]) / n for k in range(3)]
        my = sum(mp.mpf(float(v)) for v in y) / n
        Xc = np.array([[float(mp.mpf(float(X[i, k])) - mx[k]) for k in range(3)] for i in range(n)])
        yc = np.array([float(mp.mpf(float(v)) - my) for v in y])
        return Xc, yc, np.array([float(v) for v in mx]), float(my)


@dataclass
class Reference:
    w: np.ndarray        # exact coefficients, rounded to float64
    c: float
    kappa: float         # sigma_1 / sigma_rank of the centred partition
    rho: float           # ||r|| / (||Xc||_2 ||w||)
    unit: float          # kappa (1 + kappa rho): the bound on ||dw|| / ||w|| is GAMMA u unit
    mean_x: np.ndarray
    mean_y: float
    Xc: np.ndarray
    pred: np.ndarray     # exact predictions of the rows, rounded
    rank: int

    def tol_w(self, gamma=GAMMA):
        """|| w_solver - w ||_2 <= gamma u kappa (1 + kappa rho) ||w||_2: the first-order perturbation bound of the least-squares
        problem for a backward stable solver, whose backward error is gamma u."""
        return gamma * U * self.unit * float(np.linalg.norm(self.w))

    def tol_c(self, gamma=GAMMA):
        return float(np.linalg.norm(self.mean_x)) * self.tol_w(gamma) + 4 * U * (abs(self.mean_y) + float(np.abs(self.mean_x * self.w).sum()))

    def tol_pred(self, X, w_dev, gamma=GAMMA):
        """bound on |prediction_device - prediction_exact| of the rows X: the coefficient bound through the centred row (the
        null-space part of the coefficient error multiplies a zero), plus the roundings of the intercept (4, each relative to
        |mean_y| + sum |mean_k w_k|) and of the association ((w0 l + w1 u) + w2 d) + c (4 more, with |x_k w_k| and |c| in them)."""
        aw = np.abs(np.asarray(w_dev))
        return (np.linalg.norm(np.asarray(X) - self.mean_x, axis=1) * self.tol_w(gamma)
                + 8 * U * (abs(self.mean_y) + ((np.abs(self.mean_x) + np.abs(np.asarray(X))) * aw).sum(axis=1)))


def reference(X, y, rank):
    import mpmath as mp
    w, c = exact_ols(X, y, rank)
    Xc, yc, mx, my = centred_exact(X, y)
    with mp.workdps(60):
        pred = np.array([float(c + sum(mp.mpf(float(X[i, k])) * w[k] for k in range(3))) for i in range(len(y))])
        res = np.array([float(mp.mpf(float(y[i])) - (c + sum(mp.mpf(float(X[i, k])) * w[k] for k in range(3)))) for i in range(len(y))])
    wf = np.array([float(v) for v in w])
    s = np.linalg.svd(Xc, compute_uv=False)
    nw = float(np.linalg.norm(wf))
    if rank == 0 or nw == 0.0:
        kappa, rho = 1.0, 0.0
    else:
        kappa = float(s[0] / s[rank - 1])
        rho = float(np.linalg.norm(res) / (s[0] * nw))
    return Reference(w=wf, c=float(c), kappa=kappa, rho=rho, unit=kappa * (1.0 + kappa * rho), mean_x=mx, mean_y=my, Xc=Xc,
                     pred=pred, rank=rank)


def dgelsd(X, y):
    """The reference's solver on the partition: sklearn's LinearRegression centres in float64 and hands the rest to
    scipy.linalg.lstsq (dgelsd)."""
    from scipy.linalg import lstsq
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    mx, my = X.mean(axis=0), y.mean()
    w = lstsq(X - mx, y - my)[0]
    return w, my - mx @ w


# ------------------------------------------------------------------------------------------------------------ restatements
def reg_bin(dad, edges, closed_lo=False):
    """regressors.py:84-101: partition lo < dad <= hi, the later partition wins, -1 outside all.  (closed_lo: the mutation
    `>=` for `>`, for the tests of the cases' own sensitivity.)"""
    b = np.full(len(dad), -1, dtype=np.int64)
    for k in range(len(edges) - 1):
        b[((dad >= edges[k]) if closed_lo else (dad > edges[k])) & (dad <= edges[k + 1])] = k
    return b


def err_bin(dad, edges, open_=False):
    """error_predictors.py:50-66: lo <= dad <= hi, the later partition wins, NO_LABEL outside all."""
    b = np.full(len(dad), NO_LABEL, dtype=np.int64)
    for k in range(len(edges) - 1):
        b[((dad > edges[k]) & (dad < edges[k + 1])) if open_ else ((dad >= edges[k]) & (dad <= edges[k + 1]))] = k
    return b


def predict(F, edges, W, c, closed_lo=False):
    """The unclipped prediction of every row of F: 0 outside every partition, ((w0 lb + w1 ub) + w2 dad) + c inside."""
    lb, ub, dad = F[:, 0], F[:, 1], F[:, 2]
    b = reg_bin(dad, edges, closed_lo)
    Wb, cb = np.asarray(W)[np.maximum(b, 0)], np.asarray(c)[np.maximum(b, 0)]
    pred = ((Wb[:, 0] * lb + Wb[:, 1] * ub) + Wb[:, 2] * dad) + cb
    return np.where(b >= 0, pred, 0.0)


def prediction_pass(F, edges, W, c, pos, y, first, is_metric, RA0=None, ncm=None, IJs=None, A=None, D=None):
    """annchor.py:356-380: (RefineApprox, error labels, sample predictions) after the pass."""
    pred = predict(F, edges, W, c)
    spred = pred[pos]
    pr = np.clip(pred, F[:, 0], F[:, 1])
    if not is_metric:
        for i, a in enumerate(A):      # a later anchor in A overwrites an earlier one
            sel = (IJs[:, 0] == a) | (IJs[:, 1] == a)
            other = np.where(IJs[:, 0] == a, IJs[:, 1], IJs[:, 0])
            pr[sel] = D[other[sel], i]
    if first:
        RA = pr.copy()
    else:
        RA = np.array(RA0, dtype=np.float64)
        u = np.asarray(ncm).astype(bool)
        RA[u] = pr[u]
    RA[pos] = y
    return RA, err_bin(F[:, 2], edges), spred


def residual_lists(sdad, y, spred, edges, open_=False):
    """error_predictors.py:26-53: (err_ptr, the partitions' sorted residuals one after the other)."""
    res = np.asarray(y) - np.asarray(spred)
    lists = []
    for k in range(len(edges) - 1):
        mask = ((sdad > edges[k]) & (sdad < edges[k + 1])) if open_ else ((sdad >= edges[k]) & (sdad <= edges[k + 1]))
        lists.append(np.sort(res[mask]))
    ptr = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int64)
    return ptr, lists
