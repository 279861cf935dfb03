"""The rules k_emd_points (csrc/emd.hip) adds to k_emd_wide's simplex, restated on the CPU: the canonical orientation of a pair,
packed nodes (source cloud 0 .. n-1, sink cloud n .. n+m-1), integer masses m/g and n/g with g = gcd(n, m), and the pricing
tolerance 2^-43 x the diagonal of the pair's bounding box.  The pivoting itself is emd_wide_sim.solve, handed the pair as two
histograms over n + m bins (its masses come out scaled by the total, which changes no comparison).  Checks, on clouds with
coordinates in [0, 10): the value against the oracle, both argument orders equal bit for bit, exactly 0.0 on permuted copies
(duplicates included), no NaN, and the pivot counts against the kernel's caps.
    python tools/sim/emd_points_sim.py"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "..", "tests"))
from emd_wide_sim import solve   # noqa: E402
import emd_points_cases as ec    # noqa: E402


def orient(x, y):
    """Fewer points first; at equal sizes the cloud whose first differing stored coordinate is smaller."""
    if len(x) != len(y):
        return (x, y) if len(x) < len(y) else (y, x)
    d = np.flatnonzero(x.ravel() != y.ravel())
    return (y, x) if len(d) and y.ravel()[d[0]] < x.ravel()[d[0]] else (x, y)


def emd_points(x, y, stats=None, dcap=-1):
    x, y = orient(ec.as_cloud(x), ec.as_cloud(y))
    n, m, dim = len(x), len(y), x.shape[1]
    g = math.gcd(n, m)
    P = np.concatenate([x, y])
    w = P.max(0) - P.min(0)
    if dim == 1:
        diag = w[0]
    else:
        s = w[0] * w[0]
        for k in range(1, dim):
            s = s + w[k] * w[k]
        diag = np.sqrt(s)
    c = ec.ground_cost(x, y)
    M = np.zeros((n + m, n + m))
    M[:n, n:] = c
    M[n:, :n] = c.T
    hx, hy = np.zeros(n + m), np.zeros(n + m)
    hx[:n] = m // g
    hy[n:] = n // g
    return solve(hx, hy, M, True, dcap, stats, eps=diag * 2.0 ** -43)


if __name__ == "__main__":
    rng = np.random.default_rng(5)
    st, worst = [], 0.0
    cases = []
    for dim in (1, 2, 3, 4):
        X = ec.random_clouds((1, 2, 20, 30, 64, 65, 128, 128), dim, seed=dim)
        cases += [(X[i], X[j]) for i in range(8) for j in range(i + 1, 8)][::3]
    L = ec.lattice_clouds((128, 100, 64, 128), 2, seed=9) + ec.lattice_clouds((128, 37, 96), 3, seed=10)
    cases += [(L[0], L[1]), (L[0], L[3]), (L[2], L[1]), (L[4], L[6]), (L[5], L[4])]
    for x, y in cases:
        a, b = emd_points(x, y, st), emd_points(y, x)
        assert a == b and not np.isnan(a), (a, b)
        worst = max(worst, abs(a - ec.emd_pair_host(x, y)))
    print("%d pairs: largest difference from the oracle %.3g; pivots / N at most %.2f (Dantzig cap 16 N + 64)"
          % (len(cases), worst, max(p / N for N, p, _ in st)))
    zeros = 0
    for dim in (1, 2, 3, 4):
        for Lp in (1, 2, 37, 64, 128):
            x = rng.random((Lp, dim)) * 10
            dup = x[rng.integers(0, Lp, Lp)]
            for z in (x, dup, ec.lattice_clouds((Lp,), dim, seed=Lp)[0]):
                for dcap in (-1, 0):
                    assert emd_points(z, z[rng.permutation(Lp)], dcap=dcap) == 0.0
                    zeros += 1
    print("%d permuted copies (duplicates and lattice clouds included, Dantzig and Bland): all exactly 0.0" % zeros)
    bl = [emd_points(x, y, dcap=0) for x, y in cases[::9]]
    print("Bland alone on %d pairs: largest difference from Dantzig %.3g" % (len(bl), max(abs(u - emd_points(x, y)) for u, (x, y) in zip(bl, cases[::9]))))
