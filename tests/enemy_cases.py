"""Label schemes and an exactness checker for the nearest-enemy graph of the streamed form (the nn nearest rows of a DIFFERENT
label), over the hard data families of streamed_cases.py.

The checker decides whether lines ARE the nearest-enemy lines of the float32 rows, up to the rounding of the reference's own
arithmetic (float32 differences), and says why not where they are not.  Plain NumPy in float64; tested on the CPU
(test_enemy_cases.py) before any kernel is held to it.
"""
import numpy as np

import streamed_cases as sc


# ------------------------------------------------------------------------------------------------------------ label schemes
def _two_random(X, nn, seed):
    """Two balanced labels, interleaved: a row's enemies are among its nearest neighbours."""
    n = X.shape[0]
    return np.random.default_rng(seed).permutation(n) % 2


def _by_half_space(X, nn, seed):
    """The sign of the first coordinate about its median (rows on the median by row number, so that both halves exist
    whatever the data): enemies sit across a boundary and are far for most rows."""
    n = X.shape[0]
    y = np.zeros(n, dtype=np.int64)
    y[np.argsort(X[:, 0], kind="stable")[n // 2:]] = 1
    return y


def _seven_uneven(X, nn, seed):
    """Seven classes: one of exactly nn rows, one of 128 (a full tile, no padding), one of 129 (a tile and one row), and
    four that share the rest 1 : 2 : 3 : 4; assigned at random."""
    n = X.shape[0]
    rest = n - nn - 128 - 129
    assert rest >= 10 * max(nn, 1), "too few rows for the seven classes"
    sizes = [nn, 128, 129] + [rest * w // 10 for w in (1, 2, 3)]
    sizes.append(n - sum(sizes))
    y = np.repeat(np.arange(7), sizes)
    return y[np.random.default_rng(seed).permutation(n)]


def _many(X, nn, seed):
    """n // 128 classes of (almost) equal size: the most the class-padded order always accepts."""
    n = X.shape[0]
    return np.random.default_rng(seed).permutation(n) % (n // 128)


SCHEMES = {"two_random": _two_random, "by_half_space": _by_half_space, "seven_uneven": _seven_uneven, "many": _many}


def labels(scheme, X, nn, seed=77):
    y = np.asarray(SCHEMES[scheme](X, nn, seed), dtype=np.int64)
    assert y.shape == (X.shape[0],)
    cnt = np.unique(y, return_counts=True)[1]
    assert len(cnt) > 1 and cnt.min() >= nn
    return y


# ------------------------------------------------------------------------------------------------------------------ checker
def enemy_violations(X, y, rows, idx, dist, nn, gamma, complete=True):
    """Where (idx, dist) -- one line of nn entries per entry of `rows` -- is NOT the nearest-enemy graph of the float32 rows X
    with labels y.

    With D(r, j) = sum((X64[r] - X64[j])**2) in float64, a line passes when
      * every index lies in [0, n) and every listed j has y[j] != y[r];
      * no index appears twice, the distances are finite and ascend;
      * listed pairs are real: |dist[e] - sqrt(D(r, idx[e]))| <= 1e-5 sqrt(D) + tiny (tiny: one float32 ulp of the line's
        largest listed distance, as streamed_cases.knn_violations has it);
      * nothing closer was left out (`complete`): every j with y[j] != y[r] that is not listed has
        D(r, j) >= (1 - 3 gamma) max_e D(r, idx[e]).
    gamma = (dimp + 4) 2^-24 (streamed_cases.gamma_of): the bound on the REFERENCE's arithmetic derived in knn_violations, not
    an allowance for any kernel.  Exact ties may fall either way.
    Returns a list of (row, kind, listed worst D, unlisted best D, ratio) -- empty when everything passes."""
    X = np.asarray(X)
    assert X.dtype == np.float32
    y = np.asarray(y)
    n = X.shape[0]
    rows = np.asarray(rows, dtype=np.int64)
    idx = np.asarray(idx).reshape(len(rows), nn)
    dist = np.asarray(dist, dtype=np.float64).reshape(len(rows), nn)
    centre = X.astype(np.float64).mean(axis=0)   # (screening only: see knn_violations)
    C = X.astype(np.float64) - centre[None, :]
    c2 = (C * C).sum(axis=1)
    out = []
    for t, r in enumerate(rows):
        li, ld = idx[t], dist[t]
        if np.any(li < 0) or np.any(li >= n):
            out.append((int(r), "index out of range", np.nan, np.nan, np.nan))
            continue
        q = C[r]
        Dl = sc._sq_dists(C, c2, q, li)
        worst = float(Dl.max())
        same = y[li] == y[r]
        if np.any(same):
            out.append((int(r), "listed row %d has the row's own label" % int(li[int(np.argmax(same))]), worst, np.nan, np.nan))
            continue
        if len(np.unique(li)) != nn:
            out.append((int(r), "index listed twice", worst, np.nan, np.nan))
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
        Da = sc._sq_dists(C, c2, q)
        Da[li] = np.inf
        Da[y == y[r]] = np.inf
        cand = np.nonzero(Da < worst + 1e-12 * (c2 + float(q @ q)))[0]
        if len(cand) == 0:
            continue
        Du = sc._sq_dists(C, c2, q, cand)
        best = float(Du.min())
        if best < (1.0 - 3.0 * gamma) * worst:
            out.append((int(r), "a closer enemy (%d) was left out" % int(cand[int(np.argmin(Du))]), worst, best, best / worst))
    return out


# ------------------------------------------------------------------------------------------------------------ brute forces
def _ascending(X, rows, idx):
    dist = sc.true_dists(X, rows, idx)
    o = np.argsort(dist, axis=1, kind="stable")
    return np.take_along_axis(idx, o, 1), np.take_along_axis(dist, o, 1)


def enemies_selected_by(D, X, y, rows, nn):
    """The lines a selection by the (approximate) squared distances D [len(rows), n] would report: the nn smallest columns of
    another label, with the TRUE distances of those columns, ascending."""
    rows = np.asarray(rows)
    D = np.asarray(D, dtype=np.float64).copy()
    D[y[rows][:, None] == y[None, :]] = np.inf
    idx = np.argsort(D, axis=1, kind="stable")[:, :nn]
    return _ascending(X, rows, idx)


def brute_enemies_f64(X, y, rows, nn):
    """The nearest-enemy lines of `rows` by float64 differences (blocked): (idx [len(rows), nn], dist)."""
    Xd = X.astype(np.float64)
    y = np.asarray(y)
    rows = np.asarray(rows)
    idx = np.empty((len(rows), nn), dtype=np.int64)
    for b in range(0, len(rows), 16):
        rb = rows[b:b + 16]
        D = ((Xd[None, :, :] - Xd[rb][:, None, :]) ** 2).sum(-1)
        D[y[rb][:, None] == y[None, :]] = np.inf
        idx[b:b + 16] = np.argsort(D, axis=1, kind="stable")[:, :nn]
    return _ascending(X, rows, idx)


def brute_cosine_enemies_f64(X, y, rows, nn):
    """Nearest enemies under the cosine distance 1 - x.y / (|x||y|) in float64: (idx, dist)."""
    Xd = X.astype(np.float64)
    U = Xd / np.linalg.norm(Xd, axis=1)[:, None]
    rows = np.asarray(rows)
    D = 1.0 - U[rows] @ U.T
    D[np.asarray(y)[rows][:, None] == np.asarray(y)[None, :]] = np.inf
    idx = np.argsort(D, axis=1, kind="stable")[:, :nn]
    return idx, np.take_along_axis(D, idx, 1)
