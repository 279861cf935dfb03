"""Streamed nearest enemies at N = 10^6, d = 128, nn = 3 beside the closest existing workload: StreamedAnnchor.query of all
rows against the fitted data at the same budget (the same tile kernels in the same form).  For 2, 10 and 1000 classes: wall
times (host clock around calls that end in a device wait), the second context's per-kernel-family times (device events,
taken in a separate profiled call), tile evaluations, padded tile counts and recall@3 on 2500 rows against a float64 brute
force -- beside the k-NN recall of the same fit.  Prints a markdown table.

    python tools/enemies_probe.py [n] [p_work] [repeats]
"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from annchor_amd.streamed import StreamedAnnchor   # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
p_work = float(sys.argv[2]) if len(sys.argv) > 2 else 0.1
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
d, nn, NROWS = 128, 3, 2500
rng = np.random.default_rng(1234)
W = rng.standard_normal((8, d))
X = (rng.standard_normal((n, 8)) @ W + 0.05 * rng.standard_normal((n, d))).astype(np.float32)
Xd = None


def labels_by_centres(k, seed=3):
    """k classes: the nearest of k fixed random rows (k = 2: a half-space; spatially coherent classes, like real labels)."""
    c = X[np.random.default_rng(seed).choice(n, k, replace=False)]
    best, arg = np.full(n, np.inf), np.zeros(n, dtype=np.int64)
    x2 = (X.astype(np.float64) ** 2).sum(1)
    for b in range(0, k, 50):
        cb = c[b:b + 50].astype(np.float64)
        d2 = x2[:, None] - 2.0 * (X @ cb.T.astype(np.float32)).astype(np.float64) + (cb * cb).sum(1)[None, :]
        a = d2.argmin(1)
        v = d2[np.arange(n), a]
        upd = v < best
        best[upd], arg[upd] = v[upd], a[upd] + b
    return arg


def brute(rows, y=None, k=nn, skip_self=False):
    """float64 truth on the GPU through torch (plumbing, not the path under test): the expanded form in float64 on centred rows
    is good to ~1e-13 relative on this data, far below the gaps between neighbours."""
    import torch

    global Xd
    if Xd is None:
        Xd = torch.from_numpy(X).cuda().double()
        Xd -= Xd.mean(0, keepdim=True)
    x2 = (Xd * Xd).sum(1)
    yt = torch.from_numpy(y).cuda() if y is not None else None
    out = np.empty((len(rows), k), dtype=np.int64)
    for b in range(0, len(rows), 500):
        rb = torch.from_numpy(rows[b:b + 500]).cuda()
        D = x2[None, :] + x2[rb][:, None] - 2.0 * (Xd[rb] @ Xd.T)
        if yt is not None:
            D[yt[rb][:, None] == yt[None, :]] = float("inf")
        if skip_self:
            D[torch.arange(len(rb), device="cuda"), rb] = float("inf")
        out[b:b + 500] = torch.topk(D, k, dim=1, largest=False).indices.cpu().numpy()
    return out


def recall(idx, truth, rows):
    return float(np.mean([len(set(idx[r].tolist()) & set(truth[t].tolist())) / truth.shape[1] for t, r in enumerate(rows)]))


def best_of(f):
    f()   # warm-up: code objects, allocations
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return min(ts), max(ts)


sa = StreamedAnnchor(X, n_anchors=32, n_neighbors=15, p_work=p_work).fit()
rows = np.sort(rng.choice(n, NROWS, replace=False))
knn_truth = brute(rows, k=nn, skip_self=True)
knn_recall = recall(sa.neighbor_graph[0][:, 1:nn + 1], knn_truth, rows)
q_lo, q_hi = best_of(lambda: sa.query(X, nn=nn, p_work=p_work))
print("N = %d, d = %d, nn = %d, p_work = %.3g, %d repeats (min .. max); fit %.3f s, k-NN recall@%d of the fit %.4f"
      % (n, d, nn, p_work, reps, sa.timings["total"], nn, knn_recall))
print("query of all rows (the yardstick): %.3f .. %.3f s, %d tiles" % (q_lo, q_hi, sa.n_tiles_total))
print()
print("| classes | tiles (padded) | wall s (min .. max) | x query | bind + anchors | class order | ranking + mask | tile phase | guard | repair | finalize + emit | tile evals | recall@3 |")
print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
for k in (2, 10, 1000):
    y = labels_by_centres(k)
    if np.unique(y, return_counts=True)[1].min() < nn:
        print("| %d | classes smaller than nn: skipped |" % k)
        continue
    lo, hi = best_of(lambda: sa.nearest_enemies(y, nn, p_work=p_work))
    idx, _ = sa.nearest_enemies(y, nn, p_work=p_work, profile=True)   # (profiled in a call of its own)
    pf, tm = sa.enemy_stats["profile"], sa.enemy_stats["timings"]
    ms = lambda *names: sum(pf[x]["ms"] for x in names if x in pf)   # noqa: E731
    order_ms = ms("stream_order_tiles", "stream_order_classes")
    rec = recall(idx, brute(rows, y), rows)
    print("| %d | %d | %.3f .. %.3f | %.2f | %.1f ms | %.1f ms (%.1f on the device) | %.1f ms | %.1f ms | %.1f ms | %.1f ms | %.1f ms | %d | %.4f |"
          % (k, sa.enemy_stats["tiles"], lo, hi, lo / q_lo, 1e3 * tm["bind_anchors"], 1e3 * tm["class_order"], order_ms, ms("stream_rank_tile_pairs"),
             ms("stream_tile_gemm_topk"), ms("stream_tile_expanded_form_guard"), ms("stream_tile_exact_repair"),
             ms("stream_finalize", "stream_enemies_emit"), sa.enemy_tile_evals, rec))
    print("  kernel %s, repaired %s, flagged rows %d" % (sa.enemy_stats["kernel"], sa.enemy_stats["repaired"], sa.enemy_stats["guard_rows"]), file=sys.stderr)
