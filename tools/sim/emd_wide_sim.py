"""Sequential restatement of k_emd_wide's pivoting rules (csrc/emd.hip): the same reduction, row-minimum start, block pricing
(whole sources, at most 1024 arcs, round robin, Dantzig inside a block), Bland fallback, pointer-walk cycle, leaving-arc tie
rule, subtree climb and parent reversal -- one node at a time in NumPy.  Compared with the oracle's shortest-path solver on
256-bin data; prints the largest difference, the pivot counts (the kernel's caps were chosen from them) and the longest cycle.
    python tools/sim/emd_wide_sim.py
DESIGN.md quotes its output: at most 7.1e-15 from the oracle, at most 3.3 N pivots under Dantzig, 23.6 N under Bland alone."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from oracle import metrics as om   # noqa: E402


def solve(hx, hy, M, integral, dcap=-1, stats=None, eps=None):
    nb = len(hx)
    sa = 0.0; sb = 0.0
    for k in range(nb): sa += hx[k]; sb += hy[k]
    if integral:
        xm = np.trunc(hx * sb).astype(np.int64); ym = np.trunc(hy * sa).astype(np.int64)
    else:
        xm = hx / sa; ym = hy / sb
    d = xm - ym
    src = np.flatnonzero(d > 0); snk = np.flatnonzero(d < 0)
    n, m = len(src), len(snk); N = n + m
    if n == 0 or m == 0: return 0.0
    binL = np.concatenate([src, snk])
    pfl = np.concatenate([d[src], -d[snk]]).astype(np.int64 if integral else np.float64)
    par = np.full(N, -2); pot = np.zeros(N); mark = np.zeros(N, int); order = []
    cur, nso, nko = 0, n, m
    for step in range(N - 1):
        i = cur
        opens = np.array([v for v in range(n, N) if par[v] == -2])
        cc = M[binL[i], binL[opens]]
        j = opens[np.argmin(cc)]; cmin = cc.min()
        ai, bj = pfl[i], pfl[j]; f = min(ai, bj)
        last_src, last_snk = nso == 1, nko == 1
        close_src = (last_snk and not last_src) if (ai - f > 0) else (not (last_src and not last_snk))
        cn, on = (i, j) if close_src else (j, i)
        pfl[on] = (bj if close_src else ai) - f
        pfl[cn] = f; par[cn] = on; pot[cn] = cmin; order.append(cn)
        if close_src: cur += 1; nso -= 1
        else: nko -= 1
    root = int(np.flatnonzero(par == -2)[0]); par[root] = -1; pot[root] = 0
    for s in range(N - 2, -1, -1):
        cn = order[s]; pot[cn] = pot[cn] - pot[par[cn]]
    if eps is None: eps = M.max() * 2.0 ** -43   # (k_emd_points passes its own, from the pair)
    dantzig_cap = dcap if dcap >= 0 else 16 * N + 64
    total_cap = dantzig_cap + 16 * N + 4096
    bs = max(1, 1024 // m); nblk = (n + bs - 1) // bs
    piv = blk = clean = 0
    C = M[np.ix_(binL[:n], binL[n:])]
    maxwalk = 0
    while True:
        if piv >= total_cap: return float('nan')
        bland = piv >= dantzig_cap
        i0 = blk * bs; cnt = min(bs, n - i0)
        rc = (C[i0:i0 + cnt] - pot[i0:i0 + cnt, None]) - pot[None, n:]
        found = False
        if not bland:
            k = np.argmin(rc); il, jl = divmod(k, m)
            if rc[il, jl] < -eps: found = True
        else:
            idx = np.flatnonzero(rc.ravel() < -eps)
            if len(idx): found = True; il, jl = divmod(idx[0], m)
        if not found:
            clean += 1
            if clean >= nblk: break
            blk = blk + 1 if blk + 1 < nblk else 0
            continue
        x, y = i0 + il, n + jl; rcin = rc[il, jl]
        stamp = piv + 1
        w = x
        while w >= 0: mark[w] = stamp; w = par[w]
        apex = y
        while mark[apex] != stamp: apex = par[apex]
        theta = None; leave = -1; lkey = 1 << 40; on_x = False
        w = y; wl = 0
        while w != apex:
            p = par[w]
            if w >= n:
                f = pfl[w]; key = (p << 16) | w
                if theta is None or f < theta or (f == theta and key < lkey): theta, leave, lkey, on_x = f, w, key, False
            w = p; wl += 1
        w = x
        while w != apex:
            p = par[w]
            if w < n:
                f = pfl[w]; key = (w << 16) | p
                if theta is None or f < theta or (f == theta and key < lkey): theta, leave, lkey, on_x = f, w, key, True
            w = p; wl += 1
        maxwalk = max(maxwalk, wl)
        in2 = np.zeros(N, bool)
        for v in range(N):
            w = v
            while w >= 0:
                if w == leave: in2[v] = True; break
                w = par[w]
        w = y
        while w != apex: pfl[w] += -theta if w >= n else theta; w = par[w]
        w = x
        while w != apex: pfl[w] += -theta if w < n else theta; w = par[w]
        q, p = (x, y) if on_x else (y, x)
        for v in np.flatnonzero(in2): pot[v] += rcin if ((v < n) == (q < n)) else -rcin
        w, cpar, cflow = q, p, theta
        while True:
            opar, oflow = par[w], pfl[w]
            par[w] = cpar; pfl[w] = cflow
            if w == leave: break
            cpar, cflow, w = w, oflow, opar
        piv += 1; clean = 0
        blk = 0 if bland else (blk + 1 if blk + 1 < nblk else 0)
    tot = 0.0
    for v in range(N):
        p = par[v]
        if p >= 0:
            tot += float(pfl[v]) * (M[binL[v], binL[p]] if v < n else M[binL[p], binL[v]])
    if integral: tot /= sa * sb
    if stats is not None: stats.append((N, piv, maxwalk))
    return tot

if __name__ == '__main__':
    rng = np.random.default_rng(3)
    nb = 256
    pts = rng.random((nb, 2)) * 10
    M = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))
    for integral in (True, False):
        X = np.zeros((12, nb))
        for i in range(12):
            k = [128, 128, 255, 1, 200, 60, 256, 256, 100, 30, 192, 64][i]
            sup = rng.choice(nb, k, replace=False)
            X[i, sup] = rng.integers(1, 40, k) if integral else rng.random(k) + 0.01
        X[0] = 0; X[0, :128] = rng.integers(1, 40, 128) if integral else rng.random(128) + .01
        X[1] = 0; X[1, 128:] = rng.integers(1, 40, 128) if integral else rng.random(128) + .01
        IJ = np.array([(i, j) for i in range(12) for j in range(12) if i != j][:60])
        t = time.time(); want = om.Histograms(X, M).pairs(IJ); t_or = time.time() - t
        for dcap in (-1, 0):
            st = []
            got = np.array([solve(X[i], X[j], M, integral, dcap, st) for i, j in IJ[: (60 if dcap < 0 else 12)]])
            err = np.abs(got - want[:len(got)])
            print(integral, dcap, 'maxerr', err.max(), 'oracle s', t_or, 'max piv/N', max(p / N for N, p, _ in st), 'maxpiv', max(p for _, p, _ in st), 'maxwalk', max(w for *_, w in st))
