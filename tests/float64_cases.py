"""float64 data families and the float64 exactness checker of the streamed form's float64 mode (streamed='float64').

The families are those of streamed_cases widened to float64 plus two that float32 cannot hold: a shift of 1e8 on unit-scale
structure (float32 spacing there: 8) and near-ties that differ at 1e-10.  The truth everywhere is a float64 brute force by
differences in NumPy, and "exact" is derived, not measured: a float64 sum of dimp squared differences carries a relative
error of at most (dimp + 2) 2^-53 -- on the kernel's side and on NumPy's --, so with gamma64 = (dimp + 4) 2^-52 a line passes when
  * no index appears twice, every index is a row of X;
  * (graphs) column 0 is the row itself at distance 0;
  * the distances ascend;
  * every listed distance is within gamma64, relative, of the truth;
  * (complete) no unlisted point is closer than the K-th listed one by more than gamma64, relative.
"""
import numpy as np

import streamed_cases as sc


def gamma64_of(dimp):
    return (dimp + 4) * 2.0 ** -52


def _near_ties(n, d, seed):
    """A binary lattice (squared distances are small integers: whole shells of neighbours tie) plus float64 noise of 1e-10: the
    float32 copy ties where float64 does not, at every list length -- the K-th and the K'-th entry share a shell on many rows."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2, (n, d)).astype(np.float64) + 1e-10 * rng.standard_normal((n, d))


FAMILIES64 = {name: (lambda n, d, s, _f=f: np.asarray(_f(n, d, s), dtype=np.float32).astype(np.float64)) for name, f in sc.FAMILIES.items()}
FAMILIES64["shift_1e8"] = lambda n, d, s: sc.latent(n, d, s).astype(np.float64) + 1e8
FAMILIES64["near_ties"] = _near_ties
BEYOND_FLOAT32 = ("shift_1e8", "near_ties")


def family64(name, n, d, seed=1234):
    X = np.ascontiguousarray(FAMILIES64[name](n, d, seed), dtype=np.float64)
    assert X.shape == (n, d) and np.all(np.isfinite(X))
    return X


def sq_dists_f64(X, P, rows):
    """float64 squared distances of P[rows] to every row of X, by differences: [len(rows), n]."""
    out = np.empty((len(rows), X.shape[0]))
    for b in range(0, len(rows), 16):
        out[b:b + 16] = ((X[None, :, :] - P[rows[b:b + 16]][:, None, :]) ** 2).sum(-1)
    return out


def violations64(X, rows, idx, dist, k, Q=None, complete=True, D=None):
    """Lines of (idx, dist) -- one of k entries per entry of `rows` -- that are NOT the float64 k-NN lines of X (of the queries Q
    when given: no self column then) by the criteria above.  Returns (row, what) pairs -- empty when everything passes."""
    X = np.asarray(X)
    assert X.dtype == np.float64
    n, g = X.shape[0], gamma64_of(sc.padded_dim(X.shape[1]))
    rows = np.asarray(rows, dtype=np.int64)
    idx = np.asarray(idx).reshape(len(rows), k)
    dist = np.asarray(dist).reshape(len(rows), k)
    assert dist.dtype == np.float64
    P = X if Q is None else np.asarray(Q, dtype=np.float64)
    D = sq_dists_f64(X, P, rows) if D is None else D
    bad = []
    for t, r in enumerate(rows):
        li, ld = idx[t], dist[t]
        if np.any(li < 0) or np.any(li >= n):
            bad.append((int(r), "index out of range"))
            continue
        if len(np.unique(li)) != k:
            bad.append((int(r), "index listed twice"))
            continue
        if Q is None and (li[0] != r or ld[0] != 0.0):
            bad.append((int(r), "column 0 is not the row itself at distance 0"))
            continue
        if np.any(np.diff(ld) < 0) or not np.all(np.isfinite(ld)):
            bad.append((int(r), "distances not ascending"))
            continue
        true = np.sqrt(D[t, li])
        if np.any(np.abs(ld - true) > g * true):
            e = int(np.argmax(np.abs(ld - true) - g * true))
            bad.append((int(r), "listed distance %.17g, truth %.17g" % (ld[e], true[e])))
            continue
        if not complete:
            continue
        rest = D[t].copy()
        rest[li] = np.inf
        if Q is None:
            rest[r] = np.inf
        s = 1 if Q is None else 0
        if k > s and np.sqrt(rest.min()) < true[s:].max() * (1.0 - g):
            bad.append((int(r), "column %d at %.17g is closer than the last listed one at %.17g" % (int(np.argmin(rest)), np.sqrt(rest.min()),
                                                                                                  true[s:].max())))
    return bad


def truth64(X, rows, k, Q=None, D=None):
    """(idx, D): the float64 k-NN lines of `rows` ordered by (d^2, index), self first for graphs; D as sq_dists_f64."""
    P = X if Q is None else np.asarray(Q, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.int64)
    D = sq_dists_f64(X, P, rows) if D is None else D
    Ds = D.copy()
    if Q is None:
        Ds[np.arange(len(rows)), rows] = -np.inf
    return np.argsort(Ds, axis=1, kind="stable")[:, :k], D
