"""Hard data families and a neighbour-exactness checker for the streamed (tile-granular) k-NN form.

The families attack what a distance-only comparison on centred Gaussian data cannot see: rows far from the origin
(|x|^2 >> d^2), tight clusters, ties, duplicates, and magnitudes at the ends of the float32 range.  The checker decides
whether a graph IS the k-NN graph of the float32 rows, up to the rounding of the reference's own arithmetic, and says why
not where it is not.  Both are plain NumPy (float64) and are themselves tested on the CPU (test_streamed_cases.py).
"""
import numpy as np

U32 = 2.0 ** -24   # unit roundoff of float32


def padded_dim(d):
    """The kernels' padded dimension (csrc/streamed.hip padded_dim)."""
    return 32 if d <= 32 else 64 if d <= 64 else 128 if d <= 128 else (d + 127) & ~127


def gamma_of(dimp):
    """Relative error bound of a float32 sum of `dimp` squared differences: see knn_violations."""
    return (dimp + 4) * U32


# ----------------------------------------------------------------------------------------------------------- families
def latent(n, d, seed=1234, k=8):
    """SURVEY.md section 8d recipe: low intrinsic dimension so that k-NN is meaningful (test_streamed_gpu.latent)."""
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((n, k))
    W = rng.standard_normal((k, d))
    return (Z @ W + 0.05 * rng.standard_normal((n, d))).astype(np.float32)


def _far_clusters(n, d, seed):
    rng = np.random.default_rng(seed)
    nc = max(4, n // 100)   # ~100 points per cluster: lists of up to 64 stay inside one
    cent = 30.0 * rng.standard_normal((nc, d))
    spread = np.exp(rng.uniform(np.log(0.02), np.log(0.3), nc))
    lab = rng.integers(0, nc, n)
    return (cent[lab] + spread[lab][:, None] * rng.standard_normal((n, d))).astype(np.float32)


def _outliers(n, d, seed):
    X = (1e-3 * latent(n, d, seed)).astype(np.float32)
    rows = np.random.default_rng(seed + 1).choice(n, min(5, n), replace=False)
    X[rows] = X[rows] * np.float32(1e7)
    return X


def _anisotropic(n, d, seed):
    X = latent(n, d, seed)
    X[:, 0] = (1e4 * np.random.default_rng(seed + 1).integers(0, 20, n)).astype(np.float32)
    return X


def _duplicates8(n, d, seed):
    base = latent((n + 7) // 8, d, seed)
    X = np.repeat(base, 8, axis=0)[:n]
    return np.ascontiguousarray(X[np.random.default_rng(seed + 1).permutation(n)])


FAMILIES = {
    "plain": lambda n, d, s: latent(n, d, s),
    "shift_1e3": lambda n, d, s: (latent(n, d, s) + np.float32(1e3)).astype(np.float32),
    "shift_1e5": lambda n, d, s: (latent(n, d, s) + np.float32(1e5)).astype(np.float32),
    "far_clusters": _far_clusters,
    "outliers": _outliers,
    "anisotropic": _anisotropic,
    "lattice": lambda n, d, s: np.random.default_rng(s).integers(0, 4, (n, d)).astype(np.float32),
    "duplicates_8": _duplicates8,
    "duplicates_all": lambda n, d, s: np.repeat(latent(1, d, s), n, axis=0),
    "tiny": lambda n, d, s: (latent(n, d, s) * np.float32(1e-12)).astype(np.float32),
    "huge": lambda n, d, s: (latent(n, d, s) * np.float32(1e12)).astype(np.float32),
}
ILL_CONDITIONED = ("shift_1e3", "shift_1e5", "far_clusters", "anisotropic")   # |x|^2 >> d^2 for the uncentred rows


def family(name, n, d, seed=1234):
    X = np.ascontiguousarray(FAMILIES[name](n, d, seed), dtype=np.float32)
    assert X.shape == (n, d) and np.all(np.isfinite(X))
    return X


# ------------------------------------------------------------------------------------------------------------ checker
def _sq_dists(C, c2, q, cols=None):
    """float64 squared distances of the centred point q to centred rows: by differences for a column subset, by the
    expanded form for all rows (then good to ~1e-12 (|q|^2 + |y|^2) absolute: see knn_violations)."""
    if cols is not None:
        return ((C[cols] - q[None, :]) ** 2).sum(axis=1)
    return c2 + float(q @ q) - 2.0 * (C @ q)


def knn_violations(X, rows, idx, dist, k, gamma, Q=None, complete=True):
    """Where (idx, dist) -- one line of k entries per entry of `rows` -- is NOT the k-NN graph of the float32 rows X.

    With D(r, j) = sum((X64[r] - X64[j])**2) in float64, a line passes when
      * listed pairs are real: |dist[e] - sqrt(D(r, idx[e]))| <= 1e-5 sqrt(D) + tiny, the project's tolerance for
        reported distances; tiny = one float32 ulp of the line's largest listed distance (zero distances of duplicates pass);
      * column 0 is the row itself at distance 0 (graphs; not for queries), no index appears twice, every index lies in
        [0, n), the distances ascend;
      * nothing closer was left out (`complete`): every j that is not listed (j != r) has
        D(r, j) >= (1 - 3 gamma) max_e D(r, idx[e]).
    gamma = (dimp + 4) 2^-24 for the padded dimension dimp (gamma_of): a float32 sum of dimp terms (x_i - y_i)^2 is within
    (dimp + 2) u of the exact sum, relative (u = 2^-24: one rounding for the difference -- squared, so twice --, one for the
    product, dimp - 1 for the additions); that holds for the listed and for the unlisted side, and the comparison of the two
    takes the third gamma.  It is a bound on the REFERENCE's arithmetic (np.linalg.norm(x - y) on float32 rows), not on any
    kernel: a graph selected by exact float32 differences passes whatever the data, one selected by anything coarser does not
    where the data is hard.  Under exact ties any choice passes (the kernels break ties by position in the k-d order).

    Q: float32 queries; `rows` then index Q and the lines have no self column.
    Returns a list of (row, kind, listed worst D, unlisted best D, ratio) -- empty when everything passes."""
    X = np.asarray(X)
    assert X.dtype == np.float32
    n = X.shape[0]
    rows = np.asarray(rows, dtype=np.int64)
    idx = np.asarray(idx).reshape(len(rows), k)
    dist = np.asarray(dist, dtype=np.float64).reshape(len(rows), k)
    # distances are translation invariant: centring in float64 (exact to 1e-16 of the coordinates) keeps the expanded form
    # below accurate where |x|^2 >> d^2; it only SCREENS the unlisted columns, everything that decides is done by differences
    centre = X.astype(np.float64).mean(axis=0)
    C = X.astype(np.float64) - centre[None, :]
    c2 = (C * C).sum(axis=1)
    P = C if Q is None else np.asarray(Q, dtype=np.float32).astype(np.float64) - centre[None, :]
    out = []
    for t, r in enumerate(rows):
        li, ld = idx[t], dist[t]
        if np.any(li < 0) or np.any(li >= n):
            out.append((int(r), "index out of range", np.nan, np.nan, np.nan))
            continue
        q = P[r]
        Dl = _sq_dists(C, c2, q, li)
        worst = float(Dl.max())
        if len(np.unique(li)) != k:
            out.append((int(r), "index listed twice", worst, np.nan, np.nan))
            continue
        if Q is None and (li[0] != r or ld[0] != 0.0):
            out.append((int(r), "column 0 is not the row itself at distance 0", worst, np.nan, np.nan))
            continue
        if np.any(np.diff(ld) < 0) or not np.all(np.isfinite(ld)):
            out.append((int(r), "distances not ascending", worst, np.nan, np.nan))
            continue
        tiny = float(np.spacing(np.float32(ld.max())))
        bad = np.abs(ld - np.sqrt(Dl)) > 1e-5 * np.sqrt(Dl) + tiny
        if np.any(bad):
            e = int(np.argmax(bad))
            out.append((int(r), "reported distance %.9g is not that of the listed pair" % ld[e], float(Dl[e]), np.nan,
                        float(ld[e] ** 2 / Dl[e]) if Dl[e] > 0 else np.inf))
            continue
        if not complete:
            continue
        Da = _sq_dists(C, c2, q)
        Da[li] = np.inf
        if Q is None:
            Da[r] = np.inf
        cand = np.nonzero(Da < worst + 1e-12 * (c2 + float(q @ q)))[0]   # the rest is farther than every listed column
        if len(cand) == 0:
            continue
        Du = _sq_dists(C, c2, q, cand)
        best = float(Du.min())
        if best < (1.0 - 3.0 * gamma) * worst:
            out.append((int(r), "a closer column (%d) was left out" % int(cand[int(np.argmin(Du))]), worst, best, best / worst))
    return out


# ------------------------------------------------------------------------------- brute forces (CPU stand-ins of arithmetics)
def _graph_from(D, rows, k, self_col):
    """k smallest of each line of D (stable: ties by index); with self_col the row itself comes first."""
    D = D.copy()
    if self_col:
        D[np.arange(len(rows)), rows] = -np.inf
    return np.argsort(D, axis=1, kind="stable")[:, :k]


def true_dists(X, rows, idx, Q=None):
    """float64 distances of the listed pairs, by differences."""
    Xd = X.astype(np.float64)
    P = Xd if Q is None else np.asarray(Q).astype(np.float64)
    return np.sqrt(((Xd[idx] - P[rows][:, None, :]) ** 2).sum(-1))


def brute_f64(X, rows, k, Q=None):
    """The k-NN lines of `rows` by float64 differences (blocked)."""
    Xd = X.astype(np.float64)
    P = Xd if Q is None else np.asarray(Q).astype(np.float64)
    rows = np.asarray(rows)
    idx = np.empty((len(rows), k), dtype=np.int64)
    for b in range(0, len(rows), 16):
        rb = rows[b:b + 16]
        D = ((Xd[None, :, :] - P[rb][:, None, :]) ** 2).sum(-1)
        idx[b:b + 16] = _graph_from(D, rb, k, Q is None)
    return _ascending(X, rows, idx, Q)


def _ascending(X, rows, idx, Q=None):
    """(idx, true distances) with every line ascending; graphs keep the row itself first among its duplicates."""
    dist = true_dists(X, rows, idx, Q)
    s = 1 if Q is None else 0
    o = s + np.argsort(dist[:, s:], axis=1, kind="stable")
    idx[:, s:] = np.take_along_axis(idx, o, 1)
    dist[:, s:] = np.take_along_axis(dist, o, 1)
    if Q is None:
        dist[:, 0] = 0.0
    return idx, dist


def select_f32_differences(X, rows):
    """float32 squared distances of `rows` to every row, summed coordinate by coordinate in float32: the reference's arithmetic
    (np.linalg.norm(x - y) on float32 rows) in its plainest order."""
    rows = np.asarray(rows)
    acc = np.zeros((len(rows), X.shape[0]), dtype=np.float32)
    for c in range(X.shape[1]):
        t = X[None, :, c] - X[rows, c][:, None]
        acc += t * t
    return acc


def select_f32_expanded(X, rows):
    """|x|^2 + |y|^2 - 2 x.y in float32 on the UNCENTRED rows: what the exact-f32 tile kernel selects by."""
    rows = np.asarray(rows)
    rs = (X * X).sum(axis=1, dtype=np.float32)
    G = (X[rows] @ X.T).astype(np.float32)
    return (rs[rows][:, None] + rs[None, :]) - np.float32(2.0) * G


def graph_selected_by(D, X, rows, k):
    """The graph lines a selection by the approximate squared distances D would report: its k smallest columns (self first),
    with the TRUE distances of those columns, ascending -- a wrong selection that reports real pairs, like the kernels."""
    rows = np.asarray(rows)
    idx = _graph_from(np.asarray(D, dtype=np.float64), rows, k, True)
    dist = true_dists(X, rows, idx)
    o = 1 + np.argsort(dist[:, 1:], axis=1, kind="stable")
    idx[:, 1:] = np.take_along_axis(idx, o, 1)
    dist[:, 1:] = np.take_along_axis(dist, o, 1)
    dist[:, 0] = 0.0
    return idx, dist
