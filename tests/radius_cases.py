"""The fixed-radius graph on the host: the classification rule, the threshold and the CSR assembly restated in NumPy, the
plain double loop they are checked against, the injected anchor tables of the kernel tests and the data of the end-to-end tests.

The rule (include/annchor_hip.h), float64, for a pair i < j and every anchor a:
    s = D[i, a]   t = D[j, a]   m = (s + t) + r
    out(a): (|s - t| - r) > rtol * m          in(a): (r - (s + t)) > rtol * m
    OUT if any out(a);  else SURE if connectivity mode and any in(a);  else EVAL
NumPy evaluates every operation on its own (no fused multiply-add), as the library does (-ffp-contract=off): the classes are the
kernel's bit for bit.  The graph is {d <= r} over the EVAL pairs plus, in connectivity mode, the SURE pairs.

`reference(..., wrong=...)` is the same code with one deliberate mistake; tests/test_radius_cases.py shows that the case set
notices each of them."""
import numpy as np

OUT, EVAL, SURE = 0, 1, 2
WRONG = ("lt_for_le", "max_for_min", "no_rtol", "j_ge_i", "drop_last_anchor", "drop_last_column")


# ------------------------------------------------------------------------------------------------------ the reference
def classify(D, r, rtol, conn, use_bounds=True, wrong=None):
    """Class of every pair: int8 [nx, nx], -1 outside i < j."""
    D = np.asarray(D, dtype=np.float64)
    nx = D.shape[0]
    na = D.shape[1] if use_bounds else 0
    if wrong == "drop_last_anchor" and na > 0:
        na -= 1
    r = np.float64(r)
    rtol = np.float64(0.0 if wrong == "no_rtol" else rtol)
    out = np.zeros((nx, nx), dtype=bool)
    any_in = np.zeros((nx, nx), dtype=bool)
    all_in = np.ones((nx, nx), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(na):
            s, t = D[:, a][:, None], D[:, a][None, :]
            sm = s + t
            tol = rtol * (sm + r)
            out |= (np.abs(s - t) - r) > tol
            inn = (r - sm) > tol
            any_in |= inn
            all_in &= inn
    inside = (all_in & (na > 0)) if wrong == "max_for_min" else any_in   # (the upper bound is the MIN over anchors of s + t)
    cls = np.full((nx, nx), EVAL, dtype=np.int8)
    if conn:
        cls[inside] = SURE
    cls[out] = OUT
    valid = np.triu(np.ones((nx, nx), dtype=bool), k=0 if wrong == "j_ge_i" else 1)
    if wrong == "drop_last_column" and nx > 0:
        valid[:, nx - 1] = False
    cls[~valid] = -1
    return cls


def lists(cls):
    """EVAL and SURE pairs in row-major order, ascending j inside a row (int64 [n, 2]), and the per-row counts of both."""
    ev, su = np.argwhere(cls == EVAL).astype(np.int64), np.argwhere(cls == SURE).astype(np.int64)
    return dict(eval=ev, sure=su, row_eval=(cls == EVAL).sum(axis=1).astype(np.int64), row_sure=(cls == SURE).sum(axis=1).astype(np.int64),
                pruned=int((cls == OUT).sum()))


def csr(nx, ij, d):
    """Symmetric CSR of upper-triangle pairs, every row ascending by column: (indptr, indices, distances or None)."""
    rows = np.concatenate([ij[:, 0], ij[:, 1]])
    cols = np.concatenate([ij[:, 1], ij[:, 0]])
    order = np.argsort(rows * max(nx, 1) + cols, kind="stable")
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=nx))]).astype(np.int64)
    return indptr, cols[order].astype(np.int64), (None if d is None else np.concatenate([d, d])[order])


def reference(D, pairs_fn, r, rtol, conn, use_bounds=True, wrong=None):
    """The whole route: classes from D, pairs_fn (IJ -> float64) on the EVAL pairs, threshold, CSR.  Returns the graph, the
    lists and the number of evaluations."""
    nx = np.asarray(D).shape[0]
    L = lists(classify(D, r, rtol, conn, use_bounds, wrong))
    d = np.asarray(pairs_fn(L["eval"]), dtype=np.float64) if len(L["eval"]) else np.zeros(0)
    keep = (d < r) if wrong == "lt_for_le" else (d <= r)
    ij = np.concatenate([L["eval"][keep], L["sure"]])
    vals = None if conn else d[keep]
    return dict(graph=csr(nx, ij, vals), evals=len(L["eval"]), **L)


def double_loop(nx, dist, r):
    """Ground truth: the metric on every pair, one by one.  Returns (indptr, indices, distances)."""
    rows = [[] for _ in range(nx)]
    for i in range(nx):
        for j in range(i + 1, nx):
            d = dist(i, j)
            if d <= r:
                rows[i].append((j, d))
                rows[j].append((i, d))
    indptr = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
    flat = [e for x in rows for e in sorted(x)]
    return (indptr, np.array([e[0] for e in flat], dtype=np.int64).reshape(-1), np.array([e[1] for e in flat], dtype=np.float64).reshape(-1))


def graph_from_matrix(M, r):
    """double_loop for a precomputed symmetric distance matrix."""
    nx = M.shape[0]
    keep = (M <= r) & ~np.eye(nx, dtype=bool)
    indptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    i, j = np.nonzero(keep)
    return indptr, j.astype(np.int64), M[i, j].astype(np.float64)


def matrix_of(nx, pairs_fn):
    """All pairs through pairs_fn (IJ -> float64) as a symmetric matrix, zero diagonal."""
    iu = np.triu_indices(nx, k=1)
    M = np.zeros((nx, nx), dtype=np.float64)
    if len(iu[0]):
        M[iu] = pairs_fn(np.stack(iu, axis=1).astype(np.int64))
    return M + M.T


def same_graph(a, b, distances=True):
    ok = np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    if distances:
        ok = ok and a[2] is not None and b[2] is not None and a[2].tobytes() == b[2].tobytes()
    return ok


def edge_radii(M):
    """0, one below the smallest non-zero distance, attained distances (a small and a middle one), one above the largest."""
    v = np.unique(M[np.triu_indices(M.shape[0], k=1)])
    pos = v[v > 0]
    return [0.0, float(pos[0]) * 0.5, float(pos[0]), float(pos[len(pos) // 8]), float(pos[len(pos) // 2]), float(v[-1]) * 1.5 + 1.0]


# ------------------------------------------------------------------------------------- injected anchor tables (kernel tests)
# The kernel's own sizes (csrc/radius.hip): 128 rows per workgroup, 64 columns per chunk, 32 anchors per tile.
ROWS, COLS, TILE = 128, 64, 32


def table(kind, nx, na, seed):
    """float64 [nx, na].  ints: points on a line at few integer positions (many duplicates, many ties at |s - t| = r and
    s + t = r for integer r), anchors at drawn positions; line: distinct float positions, anchors left of all of them (so
    |s - t| is the true distance and the class is OUT exactly when the points are further apart than r); dups: one point
    repeated; inf: ints with an all-inf anchor and scattered inf entries (inf - inf = NaN: neither test fires); islands: even
    points in a tight group, odd points far from everything (rows without candidates between rows with some)."""
    rng = np.random.default_rng(seed)
    if kind == "line":
        x = np.sort(rng.uniform(0.0, 100.0, nx)) + np.arange(nx) * 1e-3
        anchors = -1.0 - np.arange(na, dtype=np.float64)
    elif kind == "dups":
        x = np.full(nx, 7.0)
        anchors = rng.integers(0, 12, na).astype(np.float64)
    elif kind == "islands":
        x = np.where(np.arange(nx) % 2 == 0, rng.integers(0, 4, nx), 1000.0 * (1 + np.arange(nx))).astype(np.float64)
        anchors = -1.0 - np.arange(na, dtype=np.float64)
    else:
        x = rng.integers(0, 12, nx).astype(np.float64)
        anchors = rng.integers(0, 12, na).astype(np.float64)
    D = np.abs(x[:, None] - anchors[None, :])
    if kind == "inf":
        D[:, na - 1] = np.inf
        D[rng.random(D.shape) < 0.05] = np.inf
    return np.ascontiguousarray(D, dtype=np.float64)


def _case(kind, nx, na, r, rtol=0.0, conn=False, use_bounds=True, cap=None, seed=1):
    return dict(kind=kind, nx=nx, na=na, r=r, rtol=rtol, conn=conn, use_bounds=use_bounds, cap=cap, seed=seed)


CASES = {}
for _nx in (1, 2, 63, 64, 65, 129):                       # nx on the chunk and workgroup edges (65: one past the column chunk)
    CASES["nx%d" % _nx] = _case("ints", _nx, 2, 3.0, conn=True, seed=_nx)
    CASES["nx%d_dist" % _nx] = _case("ints", _nx, 3, 2.0, seed=100 + _nx)
CASES["nx1100"] = _case("ints", 1100, 5, 3.0, conn=True, seed=7)
CASES["nx1100_line"] = _case("line", 1100, 1, 0.8, seed=8)
for _na in (1, 2, TILE, TILE + 1, 65, 257):               # anchor counts on the tile edges
    CASES["na%d" % _na] = _case("ints", 129, _na, 3.0, conn=True, seed=200 + _na)
    CASES["na%d_rtol" % _na] = _case("ints", 67, _na, 4.0, rtol=0.05, conn=True, seed=300 + _na)
CASES["dups"] = _case("dups", 70, 4, 0.0, conn=True)
CASES["r0"] = _case("ints", 130, 3, 0.0, conn=True, seed=11)
CASES["r0_dist"] = _case("ints", 130, 3, 0.0, seed=12)
CASES["all_out"] = _case("line", 140, 2, 1e-6, conn=True, seed=13)
CASES["all_eval"] = _case("ints", 140, 2, 1e9, seed=14)
CASES["all_sure"] = _case("ints", 140, 2, 1e9, conn=True, seed=14)
CASES["rtol_pos"] = _case("ints", 200, 4, 3.0, rtol=0.05, conn=True, seed=15)
CASES["rtol_pos_dist"] = _case("ints", 200, 4, 3.0, rtol=0.05, seed=15)
CASES["inf"] = _case("inf", 131, 5, 3.0, conn=True, seed=16)
CASES["inf_wide"] = _case("inf", 66, TILE + 2, 3.0, rtol=0.01, conn=True, seed=17)
CASES["no_bounds"] = _case("ints", 131, 3, 3.0, use_bounds=False, seed=18)
CASES["no_bounds_conn"] = _case("ints", 65, 3, 3.0, conn=True, use_bounds=False, seed=19)
CASES["chunked"] = _case("ints", 200, 3, 3.0, conn=True, cap=37, seed=20)      # rows share chunks, and rows of > 37 candidates are split
CASES["chunked_dist"] = _case("ints", 150, 2, 5.0, cap=10, seed=21)
CASES["chunked_all"] = _case("ints", 129, 2, 1e9, cap=50, seed=22)             # every row above the cap down to row 78
CASES["islands"] = _case("islands", 140, 2, 5.0, conn=True, seed=23)
CASES["islands_chunked"] = _case("islands", 140, 2, 5.0, cap=16, seed=24)


def build(name):
    c = CASES[name]
    return table(c["kind"], c["nx"], c["na"], c["seed"])


def case_reference(name):
    c = CASES[name]
    return lists(classify(build(name), c["r"], c["rtol"], c["conn"], c["use_bounds"]))


def line_metric(name):
    """For the tables built from points on a line: the true distance |x_i - x_j| as a pairs function (the mutation test's
    metric).  Recovered from anchor 0 of the line / islands kinds (all points right of it) -- other kinds have no such reading."""
    c = CASES[name]
    assert c["kind"] in ("line", "islands")
    x = build(name)[:, 0]
    return lambda IJ: np.abs(x[IJ[:, 0]] - x[IJ[:, 1]])


# ------------------------------------------------------------------------------------------------ end-to-end data sets
E2E_STRINGS = dict(n=300, n_anchors=12, r=8.0)   # 12 clusters of 25 strings of ~40 symbols; mean degree 8 at r = 8


def clustered_strings(n, length=40, seed=3):
    """n strings in clusters of 25 (annchor_amd.datasets.synthetic_string_clusters): a few edits inside a cluster, unrelated
    strings across clusters -- the anchor bounds prune most cross-cluster pairs at a within-cluster radius."""
    from annchor_amd.datasets import synthetic_string_clusters

    return synthetic_string_clusters(n, cluster=25, length=length, seed=seed)


def levenshtein_pairs(X):
    from oracle import metrics as om

    P = om.PackedStrings(list(X))
    return lambda IJ: P.pairs(np.ascontiguousarray(IJ, dtype=np.int64))


def lattice_points(n, dim, seed, dtype):
    """Rows of small integers in clusters: every difference, square and sum is an exact integer below 2^24 in float32 and
    float64 alike, so the Euclidean distance is one correctly rounded square root of an exact integer whatever the order of
    the sum -- the host loop and the kernel agree bit for bit, and distances tie massively (attained radii, duplicates)."""
    rng = np.random.default_rng(seed)
    centres = rng.integers(0, 60, (6, dim))
    X = centres[rng.integers(0, 6, n)] + rng.integers(-3, 4, (n, dim))
    X[n - 10:] = X[:10]   # exact copies: distance 0
    return np.ascontiguousarray(X, dtype=dtype)


def euclidean_pairs(X):
    """np.linalg.norm(x - y) in X's dtype, stored as float64 (the reference's definition)."""
    def f(IJ):
        diff = X[IJ[:, 0]] - X[IJ[:, 1]]
        return np.sqrt((diff * diff).sum(axis=1, dtype=X.dtype)).astype(np.float64)
    return f
