"""The exact k-NN graph from per-row radii on the host: seed radii, classification, the directed absorb and the row selection
restated in NumPy, the ground truth they are checked against, the injected anchor tables of the kernel tests and the data of
the end-to-end tests.

The rule (include/annchor_hip.h).  k counts the point itself; the exact row of i is the k smallest of {(d(i, j), j)} over all
j, d(i, i) = 0, by distance, then index.
    radii     u[i] = max d(i, g) over the distinct entries g != i of row i of a guess, when there are >= k - 1 of them, all in
              [0, nx); +inf otherwise
    classify  i < j, R = max(u[i], u[j]); for every anchor a: s = D[i, a], t = D[j, a]
              out(a): (|s - t| - R) > rtol * ((s + t) + R);   OUT if any out(a), else EVAL
    absorb    an evaluated pair with distance d gives (i -> j, d) if d <= u[i] and (j -> i, d) if d <= u[j]
    finish    row i = the k smallest of its entries plus (0.0, i), by (distance, index)
NumPy evaluates every operation on its own (no fused multiply-add), as the library does (-ffp-contract=off): the classes are
the kernel's bit for bit.

`route(..., wrong=...)` is the same code with one deliberate mistake; tests/test_exact_knn_cases.py shows that the case set
notices each of them."""
import numpy as np

import radius_cases as RC

WRONG = ("min_for_max", "ui_only", "lt_for_le", "one_direction", "desc_ties", "no_diagonal", "drop_last_anchor", "drop_last_column",
         "drop_last_row")


# ------------------------------------------------------------------------------------------------------ the reference
def truth(M, k):
    """Rows of the full matrix (zero diagonal) in stable order: (idx int64 [nx, k], dist float64 [nx, k])."""
    order = np.argsort(M, axis=1, kind="stable")[:, :k]
    return order.astype(np.int64), np.take_along_axis(M, order, axis=1).astype(np.float64)


def seed_radii(nx, k, G, pairs_fn):
    """u float64 [nx] from a guess G (int64 [nx, >= k]), one row at a time."""
    u = np.full(nx, np.inf)
    for i in range(nx):
        ent = sorted({int(g) for g in G[i, :k]} - {i})
        if len(ent) < k - 1 or any(g < 0 or g >= nx for g in ent):
            continue
        if not ent:
            u[i] = 0.0
            continue
        d = np.asarray(pairs_fn(np.array([[min(i, g), max(i, g)] for g in ent], dtype=np.int64)), dtype=np.float64)
        u[i] = d.max()
    return u


def classify(D, u, rtol, use_bounds=True, wrong=None):
    """EVAL mask of every pair: bool [nx, nx], False outside i < j."""
    D = np.asarray(D, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    nx = D.shape[0]
    na = D.shape[1] if use_bounds else 0
    if wrong == "drop_last_anchor" and na > 0:
        na -= 1
    rtol = np.float64(rtol)
    if wrong == "min_for_max":
        R = np.minimum(u[:, None], u[None, :])
    elif wrong == "ui_only":
        R = np.broadcast_to(u[:, None], (nx, nx))
    else:
        R = np.maximum(u[:, None], u[None, :])
    out = np.zeros((nx, nx), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(na):
            s, t = D[:, a][:, None], D[:, a][None, :]
            out |= (np.abs(s - t) - R) > rtol * ((s + t) + R)
    valid = np.triu(np.ones((nx, nx), dtype=bool), k=1)
    if wrong == "drop_last_column" and nx > 0:
        valid[:, nx - 1] = False
    if wrong == "drop_last_row" and nx > 1:
        valid[nx - 2, :] = False   # (the last row that holds a pair)
    return valid & ~out


def lists(ev):
    """EVAL pairs in row-major order, ascending j inside a row (int64 [n, 2]), and the per-row counts."""
    return dict(eval=np.argwhere(ev).astype(np.int64), row_eval=ev.sum(axis=1).astype(np.int64))


def absorb(ij, d, u, wrong=None):
    """Directed entries (row, col, d) of evaluated candidates; the i -> j entries first."""
    ij, d = np.asarray(ij, dtype=np.int64).reshape(-1, 2), np.asarray(d, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        a = (d < u[ij[:, 0]]) if wrong == "lt_for_le" else (d <= u[ij[:, 0]])
        b = (d < u[ij[:, 1]]) if wrong == "lt_for_le" else (d <= u[ij[:, 1]])
    if wrong == "one_direction":
        b = np.zeros_like(b)
    row = np.concatenate([ij[a, 0], ij[b, 1]])
    col = np.concatenate([ij[a, 1], ij[b, 0]])
    return row, col, np.concatenate([d[a], d[b]])


def finish(nx, k, entries, wrong=None):
    """(idx, dist, row_entries); a row with fewer than k items is padded with (-1, nan) (the library refuses it)."""
    row, col, d = entries
    idx = np.full((nx, k), -1, dtype=np.int64)
    dist = np.full((nx, k), np.nan)
    counts = np.bincount(row, minlength=nx).astype(np.int64)
    order = np.argsort(row, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(counts)])
    for i in range(nx):
        sel = order[ptr[i]:ptr[i + 1]]
        c, v = col[sel], d[sel]
        if wrong != "no_diagonal":
            c, v = np.append(c, i), np.append(v, 0.0)
        o = np.lexsort((-c if wrong == "desc_ties" else c, v))[:k]   # (last key first: distance, then index)
        idx[i, :len(o)], dist[i, :len(o)] = c[o], v[o]
    return idx, dist, counts


def route(D, pairs_fn, u, k, rtol, use_bounds=True, wrong=None):
    """The whole route: classes from D and u, pairs_fn (IJ -> float64) on the EVAL pairs, absorb, finish."""
    nx = np.asarray(D).shape[0]
    L = lists(classify(D, u, rtol, use_bounds, wrong))
    d = np.asarray(pairs_fn(L["eval"]), dtype=np.float64) if len(L["eval"]) else np.zeros(0)
    idx, dist, counts = finish(nx, k, absorb(L["eval"], d, np.asarray(u, dtype=np.float64), wrong), wrong)
    return dict(idx=idx, dist=dist, row_entries=counts, evals=len(L["eval"]), **L)


def same_graph(a, b):
    return np.array_equal(a[0], b[0]) and a[1].shape == b[1].shape and np.asarray(a[1], dtype=np.float64).tobytes() == np.asarray(b[1], dtype=np.float64).tobytes()


def maxmin_table(nx, pairs_fn, na, first=0):
    """Anchor table of the max-min picker from a fixed first anchor: float64 [nx, na]."""
    D = np.zeros((nx, na), dtype=np.float64)
    a, runmin = first, None
    for c in range(na):
        D[:, c] = pairs_fn(np.stack([np.full(nx, a), np.arange(nx)], axis=1).astype(np.int64))
        runmin = D[:, c].copy() if runmin is None else np.minimum(runmin, D[:, c])
        a = int(np.argmax(runmin))
    return D


# ------------------------------------------------------------------------------------- injected anchor tables (kernel tests)
def positions(kind, nx, na, seed):
    """The points on the line behind radius_cases.table(kind, nx, na, seed) (the same draws in the same order): the table is
    |x - anchor|, so |x_i - x_j| is a true metric under it."""
    rng = np.random.default_rng(seed)
    if kind == "line":
        return np.sort(rng.uniform(0.0, 100.0, nx)) + np.arange(nx) * 1e-3
    if kind == "dups":
        return np.full(nx, 7.0)
    if kind == "islands":
        return np.where(np.arange(nx) % 2 == 0, rng.integers(0, 4, nx), 1000.0 * (1 + np.arange(nx))).astype(np.float64)
    return rng.integers(0, 12, nx).astype(np.float64)


def _case(kind, nx, na, k, umode, rtol=0.0, cap=None, seed=1, use_bounds=True):
    return dict(kind=kind, nx=nx, na=na, k=k, umode=umode, rtol=rtol, cap=cap, seed=seed, use_bounds=use_bounds)


# umode: kth -- the true k-th distance (attained: |s - t| = R ties, the tightest valid radii); loose -- the k-th distance plus an
# attained distance of the row (valid, uneven); some_inf -- kth with +inf scattered; all_inf; zero -- 0 everywhere (valid only
# where every row has k - 1 duplicates)
CASES = {}
for _nx in (1, 2, 63, 64, 65, 129):
    for _k in sorted({1, 2, 5, _nx}):
        if _k <= _nx:
            CASES["nx%d_k%d" % (_nx, _k)] = _case("ints", _nx, 3, _k, "kth", seed=10 * _nx + _k)
    CASES["nx%d_loose" % _nx] = _case("ints", _nx, 2, min(2, _nx), "loose", seed=500 + _nx)
CASES["nx1100"] = _case("ints", 1100, 5, 5, "loose", seed=7)
CASES["nx1100_line"] = _case("line", 1100, 1, 5, "kth", rtol=1e-9, seed=8)   # (float positions: the computed |x - a| obey the triangle inequality up to rounding only)
CASES["nx1100_k1100"] = _case("islands", 1100, 2, 1100, "kth", seed=9)
for _na in (1, 32, 33, 65):
    CASES["na%d" % _na] = _case("ints", 129, _na, 5, "kth", seed=200 + _na)
    CASES["na%d_rtol" % _na] = _case("ints", 67, _na, 2, "loose", rtol=0.05, seed=300 + _na)
CASES["some_inf"] = _case("ints", 131, 4, 5, "some_inf", seed=31)
CASES["all_inf"] = _case("ints", 70, 3, 5, "all_inf", seed=32)
CASES["dups_u0"] = _case("dups", 70, 4, 5, "zero")
CASES["dups_u0_knx"] = _case("dups", 65, 2, 65, "zero")
CASES["line_k5"] = _case("line", 140, 2, 5, "kth", rtol=1e-9, seed=13)
CASES["line_rtol"] = _case("line", 140, 2, 5, "loose", rtol=1e-6, seed=14)
CASES["inf_anchor"] = _case("inf", 131, 5, 5, "kth", seed=16)
CASES["inf_anchor_wide"] = _case("inf", 66, 34, 2, "loose", rtol=0.01, seed=17)
CASES["no_bounds"] = _case("ints", 65, 3, 5, "kth", use_bounds=False, seed=18)
CASES["islands"] = _case("islands", 140, 2, 5, "kth", seed=23)
CASES["chunked"] = _case("ints", 200, 3, 5, "loose", cap=37, seed=20)          # rows share ranges, and rows of > 37 candidates are split
CASES["chunked_inf"] = _case("ints", 129, 2, 5, "all_inf", cap=50, seed=22)    # every row above the cap down to row 78
CASES["chunked_one"] = _case("islands", 140, 2, 5, "loose", cap=1, seed=24)    # every candidate a range of its own


def metric(name):
    c = CASES[name]
    x = positions(c["kind"], c["nx"], c["na"], c["seed"])
    return lambda IJ: np.abs(x[IJ[:, 0]] - x[IJ[:, 1]])


def build(name):
    """(D float64 [nx, na], u float64 [nx], M float64 [nx, nx]) of a case."""
    c = CASES[name]
    nx, k = c["nx"], c["k"]
    D = RC.table(c["kind"], nx, c["na"], c["seed"])
    x = positions(c["kind"], nx, c["na"], c["seed"])
    M = np.abs(x[:, None] - x[None, :])
    kth = np.sort(M, axis=1)[:, k - 1]
    rng = np.random.default_rng(c["seed"] + 99991)
    if c["umode"] == "kth":
        u = kth
    elif c["umode"] == "loose":
        u = kth + M[np.arange(nx), rng.integers(0, nx, nx)]
    elif c["umode"] == "some_inf":
        u = np.where(rng.random(nx) < 0.15, np.inf, kth)
    elif c["umode"] == "all_inf":
        u = np.full(nx, np.inf)
    else:
        u = np.zeros(nx)
    return D, np.ascontiguousarray(u, dtype=np.float64), M


_REF = {}


def case_reference(name):
    """route() of a case, computed once and never written."""
    if name not in _REF:
        c = CASES[name]
        D, u, _ = build(name)
        r = route(D, metric(name), u, c["k"], c["rtol"], c["use_bounds"])
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[name] = r
    return _REF[name]


# ------------------------------------------------------------------------------------------------ end-to-end data sets
E2E = {
    "levenshtein": dict(n=300, n_anchors=12, k=10, rtol=0.0),
    "euclidean_f32": dict(n=400, n_anchors=8, k=10, rtol=1e-4),
    "euclidean_f64": dict(n=400, n_anchors=8, k=10, rtol=1e-9),
}
SEEDS = ("true", "spoiled", "random", "invalid")


def e2e_data(name):
    """(X, metric name, pairs_fn)."""
    if name == "levenshtein":
        X = RC.clustered_strings(E2E[name]["n"])
        return X, "levenshtein", RC.levenshtein_pairs(X)
    X = RC.lattice_points(E2E[name]["n"], 3, 5, np.float32 if name.endswith("f32") else np.float64)
    return X, "euclidean", RC.euclidean_pairs(X)


def seed_graph(kind, T, k, seed=11):
    """A guess of the graph from the true one T (int64 [nx, k]): true -- T itself; spoiled -- a fifth of the rows get three random
    last neighbours; random -- every row k random points; invalid -- every third row repeats one entry (fewer than k - 1 distinct
    ones: u = +inf), the others are true."""
    nx = T.shape[0]
    rng = np.random.default_rng(seed)
    G = T.copy()
    if kind == "spoiled":
        rows = rng.random(nx) < 0.2
        G[rows, max(k - 3, 0):] = rng.integers(0, nx, (int(rows.sum()), min(3, k)))
    elif kind == "random":
        G = rng.integers(0, nx, (nx, k))
    elif kind == "invalid":
        G[::3, :] = G[::3, :1]
    else:
        assert kind == "true"
    return np.ascontiguousarray(G, dtype=np.int64)
