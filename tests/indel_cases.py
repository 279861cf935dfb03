"""The reference of the indel (LCS) distance tests: the two-row LCS loop, as distances.Indel states the distance."""
import numpy as np

NAME = "indel"
LIMIT = 2048
# one string of each length where the lane layout changes (word and half-wave boundaries, the one- and two-word-per-lane kernels),
# the empty one first and last
LENGTHS = ([0, 1, 31, 32, 33, 63, 64, 65, 1023, 1024, 0], [0, 1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 0])


def indel_loop(x, y):
    """L[i][j] = max(L[i-1][j], L[i][j-1], L[i-1][j-1] + (x[i] == y[j])), two rows; a row is computed at once: the running maximum
    along it is the L[i][j-1] term.  indel = |x| + |y| - 2 L[|x|][|y|]."""
    if len(x) > len(y):
        x, y = y, x
    b = np.frombuffer(y.encode("utf-32-le"), dtype=np.uint32)
    prev = np.zeros(len(y) + 1, dtype=np.int64)
    for c in np.frombuffer(x.encode("utf-32-le"), dtype=np.uint32):
        cur = np.zeros_like(prev)
        np.maximum(prev[1:], prev[:-1] + (b == c), out=cur[1:])
        prev = np.maximum.accumulate(cur)
    return len(x) + len(y) - 2 * int(prev[-1])


def indel_matrix(X):
    """indel_loop on every pair i < j, mirrored, zero diagonal: float64 [nx, nx]."""
    M = np.zeros((len(X), len(X)))
    for i in range(len(X)):
        for j in range(i + 1, len(X)):
            M[i, j] = M[j, i] = indel_loop(X[i], X[j])
    return M


def random_strings(lengths, symbols, seed):
    rng = np.random.default_rng(seed)
    return ["".join(symbols[c] for c in rng.integers(0, len(symbols), size=n)) for n in lengths]
