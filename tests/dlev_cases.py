"""The reference of the Damerau-Levenshtein tests: Lowrance and Wagner's full-matrix loop, as distances.DamerauLevenshtein states it."""
import numpy as np

NAME = "damerau_levenshtein"
SHAPES, LIMIT = [(8, 16), (8, 64), (32, 64)], 2048   # (R, G) of k_dlev by the data set's longest string; the longest of all


def dl_loop(x, y):
    """H over rows / columns -1 .. n-1 / m-1 (stored shifted by one); `last` holds k per symbol, `l` runs along the row."""
    n, m = len(x), len(y)
    H = [[max(i, j) if i == 0 or j == 0 else 0 for j in range(m + 1)] for i in range(n + 1)]
    last = {}
    for i in range(n):
        l, xi, above, row = -1, x[i], H[i], H[i + 1]
        for j in range(m):
            yj = y[j]
            v = min(above[j] + (xi != yj), above[j + 1] + 1, row[j] + 1)
            k = last.get(yj, -1)
            if k >= 0 and l >= 0:
                v = min(v, H[k][l] + (i - k - 1) + 1 + (j - l - 1))
            row[j + 1] = v
            if xi == yj:
                l = j
        last[xi] = i
    return H[n][m]


def dl_matrix(X):
    """dl_loop on every pair i < j, mirrored, zero diagonal (x == x needs no edit): float64 [nx, nx]."""
    M = np.zeros((len(X), len(X)))
    for i in range(len(X)):
        for j in range(i + 1, len(X)):
            M[i, j] = M[j, i] = dl_loop(X[i], X[j])
    return M


def lane_lengths(shape):
    R, G = SHAPES[shape]
    return [0, 1, 2, R + 1, LIMIT - 1, LIMIT, 0] if R * G == LIMIT else [0, 1, 2, R - 1, R, R + 1, 2 * R, G * R - 1, G * R, 0]


def random_strings(lengths, symbols, seed):
    rng = np.random.default_rng(seed)
    return ["".join(symbols[c] for c in rng.integers(0, len(symbols), size=n)) for n in lengths]
