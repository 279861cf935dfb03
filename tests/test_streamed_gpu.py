"""GPU tests of the streamed (tile-granular) Euclidean form: exactness against brute force
when the budget does not bind, budgeted recall, padding, and the two-rank path."""
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))
import streamed_cases as sc   # noqa: E402


def latent(n, d, seed=1234, k=8):
    """SURVEY.md section 8d recipe: low intrinsic dimension so that k-NN is meaningful."""
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((n, k))
    W = rng.standard_normal((k, d))
    return (Z @ W + 0.05 * rng.standard_normal((n, d))).astype(np.float32)


def brute(X, rows, k):
    Xd = X.astype(np.float64)
    out_i, out_d = [], []
    for r in rows:
        d = np.sqrt(((Xd - Xd[r][None, :]) ** 2).sum(axis=1))
        d[r] = -1
        o = np.argsort(d, kind="stable")[:k]
        out_i.append(o)
        out_d.append(np.maximum(d[o], 0))
    return np.array(out_i), np.array(out_d)


@pytest.mark.parametrize("n,d,na,k", [(5000, 128, 16, 15), (3003, 20, 8, 8), (1000, 64, 4, 33), (260, 200, 5, 5),
                                      (2500, 64, 8, 50), (1500, 128, 6, 65), (900, 256, 4, 40),   # > 33 neighbours: 64-entry lists
                                      (2000, 64, 6, 66), (1500, 128, 5, 100), (1100, 20, 4, 128), (700, 256, 4, 90)])   # > 65: two workgroups per row tile
def test_exact_when_budget_does_not_bind(n, d, na, k):
    from annchor_amd.streamed import StreamedAnnchor

    X = latent(n, d)
    sa = StreamedAnnchor(X, n_anchors=na, n_neighbors=k, p_work=1.0).fit()
    idx, dist = sa.neighbor_graph
    rows = np.arange(n) if n <= 3003 else np.random.default_rng(0).choice(n, 600, replace=False)
    bi, bd = brute(X, rows, k)
    assert np.array_equal(idx[:, 0], np.arange(n)) and np.all(dist[:, 0] == 0)
    # float tolerance: distances are float32 norms (reference: np.linalg.norm in X's dtype), rtol 1e-5
    np.testing.assert_allclose(dist[rows], bd, rtol=1e-5, atol=1e-6)
    # ... and the lists are the neighbours themselves: nothing twice, nothing closer left out (streamed_cases.knn_violations)
    assert sc.knn_violations(X, rows, idx[rows], dist[rows], k, sc.gamma_of(sc.padded_dim(d))) == []
    # every reported neighbour really is at the reported distance
    r0 = rows[:50]
    for r in r0:
        dd = np.sqrt(((X[idx[r]].astype(np.float64) - X[r].astype(np.float64)) ** 2).sum(axis=1))
        np.testing.assert_allclose(dd, dist[r], rtol=1e-5, atol=1e-6)
    assert np.all(np.diff(dist, axis=1) >= 0)  # rows sorted
    # pruning really happened on the clustered data (fewer tiles than all pairs) when there are many tiles
    nt = (n + 127) // 128
    assert sa.tile_evals <= nt * nt


@pytest.mark.parametrize("n,d,na,k", [(3000, 300, 8, 10), (2500, 384, 8, 15), (2000, 512, 6, 25), (1500, 768, 6, 8), (1300, 1024, 5, 15), (1500, 384, 6, 50), (900, 640, 4, 63)])
def test_exact_beyond_256_dimensions(n, d, na, k):
    """Rows of 257 .. 1024 dimensions (padded to a multiple of 128) take the k-blocked split-fp16 kernel (csrc/knnbk.hip: the
    column tile finished block by block, four accumulators per wave): with the budget not binding the graph is the exact k-NN
    graph -- against a float64 brute force at rtol 1e-5, like every other shape (the reference's euclidean takes any dimension:
    distances.py:8-13); the query path runs the same kernel."""
    from annchor_amd.streamed import StreamedAnnchor

    X = latent(n, d)
    sa = StreamedAnnchor(X, n_anchors=na, n_neighbors=k, p_work=1.0).fit()
    assert sa._engine.stream_last_kernel() == 1   # the split-fp16 kernel ran (no silent fall-back)
    idx, dist = sa.neighbor_graph
    rows = np.random.default_rng(0).choice(n, 400, replace=False)
    bi, bd = brute(X, rows, k)
    assert np.array_equal(idx[:, 0], np.arange(n)) and np.all(dist[:, 0] == 0)
    np.testing.assert_allclose(dist[rows], bd, rtol=1e-5, atol=1e-6)
    assert sc.knn_violations(X, rows, idx[rows], dist[rows], k, sc.gamma_of(sc.padded_dim(d))) == []
    for r in rows[:40]:
        dd = np.sqrt(((X[idx[r]].astype(np.float64) - X[r].astype(np.float64)) ** 2).sum(axis=1))
        np.testing.assert_allclose(dd, dist[r], rtol=1e-5, atol=1e-6)
    assert np.all(np.diff(dist, axis=1) >= 0)
    qi, qd = sa.query(X[rows[:64]] + 0.01, nn=5, p_work=1.0)
    Xd = X.astype(np.float64)
    for t, r in enumerate(rows[:64]):
        d_all = np.sqrt(((Xd - (X[r] + np.float32(0.01)).astype(np.float64)[None, :]) ** 2).sum(axis=1))
        np.testing.assert_allclose(qd[t], np.sort(d_all)[:5], rtol=1e-5, atol=1e-6)


def test_budgeted_recall_768_dimensions():
    """A binding budget with join passes at d = 768 (the k-blocked kernel in its tile-phase and gathered-column forms):
    recall@15 against the float64 brute force on 1 000 rows, the budget, distances at rtol 1e-5."""
    from annchor_amd import compare_neighbor_graphs
    from annchor_amd.streamed import StreamedAnnchor

    n, d, k = 60000, 768, 15
    X = latent(n, d)
    sa = StreamedAnnchor(X, n_anchors=24, n_neighbors=k, p_work=0.2).fit()
    nt = (n + 127) // 128
    assert sa.tile_evals <= int(np.ceil(0.2 * nt)) * nt
    idx, dist = sa.neighbor_graph
    rows = np.sort(np.random.default_rng(5).choice(n, 1000, replace=False))
    from test_c5_gpu import truth_f64

    bd = truth_f64(X[rows], [X], k)
    bd[:, 0] = 0.0
    err = compare_neighbor_graphs((idx[rows], bd), (idx[rows], dist[rows]), k)
    recall = 1 - err / (len(rows) * float(k))
    print("d = 768, N = %d: recall@15 %.4f, fit %.3f s" % (n, recall, sa.timings["total"]))
    assert recall >= 0.97, recall
    dd = np.sqrt(((X[idx[rows]].astype(np.float64) - X[rows].astype(np.float64)[:, None, :]) ** 2).sum(-1))
    np.testing.assert_allclose(dd, dist[rows], rtol=1e-5, atol=1e-5)


def test_budgeted_with_joins_more_than_33_neighbours():
    """n_neighbors = 48 with a binding budget and join passes (the 64-entry list kernels): the joins must help, the
    recall is that of a 48-neighbour ball in 8 dimensions cut by 128-point tiles (0.936 measured at this budget)."""
    from annchor_amd.streamed import StreamedAnnchor

    n, k = 40000, 48
    X = latent(n, 64)
    sa = StreamedAnnchor(X, n_anchors=16, n_neighbors=k, p_work=0.3).fit()
    rows = np.random.default_rng(5).choice(n, 800, replace=False)
    err, _ = _recall_rows(sa, X, rows, k)
    sa0 = StreamedAnnchor(X, n_anchors=16, n_neighbors=k, p_work=0.3, join_passes=0, join_extra=0).fit()
    err0, _ = _recall_rows(sa0, X, rows, k)
    assert err < err0 and err <= 0.08 * len(rows) * k, (err, err0)
    with pytest.raises(Exception):
        StreamedAnnchor(X[:2000], n_anchors=4, n_neighbors=129, p_work=1.0).fit()   # > 128: refused loudly
    with pytest.raises(Exception):
        StreamedAnnchor(latent(1500, 300), n_anchors=4, n_neighbors=70, p_work=1.0).fit()   # beyond 256 dimensions: <= 63


def test_budgeted_with_joins_at_100_neighbours():
    """n_neighbors = 100 (lists of 99: the exact-f32 kernels with two workgroups per row tile, each keeping 64 rows' lists) with a
    binding budget and join passes: the joins must help, the evaluation count stays within the budget, the run is deterministic."""
    from annchor_amd.streamed import StreamedAnnchor

    n, k = 30000, 100
    X = latent(n, 64)
    sa = StreamedAnnchor(X, n_anchors=16, n_neighbors=k, p_work=0.3).fit()
    rows = np.random.default_rng(7).choice(n, 400, replace=False)
    err, _ = _recall_rows(sa, X, rows, k)
    sa0 = StreamedAnnchor(X, n_anchors=16, n_neighbors=k, p_work=0.3, join_passes=0, join_extra=0).fit()
    err0, _ = _recall_rows(sa0, X, rows, k)
    assert err < err0 and err <= 0.12 * len(rows) * k, (err, err0)
    nt = (n + 127) // 128
    assert sa.tile_evals <= int(np.ceil(0.3 * nt)) * nt + nt
    sb = StreamedAnnchor(X, n_anchors=16, n_neighbors=k, p_work=0.3).fit()
    assert np.array_equal(sa.neighbor_graph[0], sb.neighbor_graph[0])


def test_budgeted_with_joins_at_62_neighbours():
    """n_neighbors = 62: the lists (61 entries + 15 reverse neighbours per row) are longer than the 64 first-hop entries per row
    the join's candidate kernel holds -- it takes the reverse neighbours and the closest 49 (before the cap the first hop overran its
    buffer and the candidates were an arbitrary subset).  The joins must help, and the pass must be deterministic."""
    from annchor_amd.streamed import StreamedAnnchor

    n, k = 40000, 62
    X = latent(n, 64)
    sa = StreamedAnnchor(X, n_anchors=16, n_neighbors=k, p_work=0.3).fit()
    rows = np.random.default_rng(6).choice(n, 600, replace=False)
    err, _ = _recall_rows(sa, X, rows, k)
    sa0 = StreamedAnnchor(X, n_anchors=16, n_neighbors=k, p_work=0.3, join_passes=0, join_extra=0).fit()
    err0, _ = _recall_rows(sa0, X, rows, k)
    assert err < err0 and err <= 0.10 * len(rows) * k, (err, err0)
    sb = StreamedAnnchor(X, n_anchors=16, n_neighbors=k, p_work=0.3).fit()
    assert np.array_equal(sa.neighbor_graph[0], sb.neighbor_graph[0])


def test_anchors_follow_the_reference_picker():
    from annchor_amd.streamed import StreamedAnnchor
    from oracle import annchor_oracle as O

    X = latent(4000, 32)
    sa = StreamedAnnchor(X, n_anchors=10, n_neighbors=5, p_work=1.0, random_seed=7)
    sa.get_anchors()

    def one_to_all(ix):
        return np.sqrt(((X.astype(np.float64) - X[ix].astype(np.float64)[None, :]) ** 2).sum(axis=1))

    A, _ = O.maxmin_anchors(one_to_all, len(X), 10, 7)
    assert np.array_equal(sa.A, A)


def test_exact_with_several_selection_rounds():
    """More column tiles (547) than one candidate-selection round takes (512): the radix selection's
    cut, the (key, tile) continuation across rounds and the second round's tiles are all needed for
    the exact result."""
    from annchor_amd.streamed import StreamedAnnchor

    n, k = 70000, 10
    X = latent(n, 32)
    sa = StreamedAnnchor(X, n_anchors=8, n_neighbors=k, p_work=1.0).fit()
    rows = np.random.default_rng(3).choice(n, 400, replace=False)
    bi, bd = brute(X, rows, k)
    np.testing.assert_allclose(sa.neighbor_graph[1][rows], bd, rtol=1e-5, atol=1e-6)
    assert sa.tile_evals <= 547 * 547


def _recall_rows(sa, X, rows, k):
    """errors of compare_neighbor_graphs on `rows` against the exact k-NN from the streamed query with the full budget"""
    from annchor_amd import compare_neighbor_graphs

    ti, td = sa.query(X[rows], nn=k, p_work=1.0)   # column 0 = the row itself at distance 0
    assert np.all(td[:, 0] <= 1e-3 * (1 + td[:, 1]))
    return compare_neighbor_graphs((ti, td), (sa.neighbor_graph[0][rows], sa.neighbor_graph[1][rows]), k), td


@pytest.mark.parametrize("n,bar", [(30100, 0.93), (100000, 0.92)])
def test_budgeted_recall(n, bar):
    """p_work = 0.1 just above the size at which Annchor switches to this form, and at 10^5 points.  The
    whole budget -- tile phase + join passes -- is ceil(p_work * n_tiles) tile evaluations per row
    tile; the join passes (an eighth of it each) must beat spending everything on the tile phase.
    A tile-granular budget is coarse at small N: below 64 tile evaluations per row tile p_work is
    raised (N = 30 100: 236 tiles, p_work 0.1 -> 0.271, announced like the reference's own p_work
    floor); at N = 10^6 the same settings reach >= 0.99 (test_c3_full_size_recall)."""
    from annchor_amd.streamed import StreamedAnnchor

    k = 15
    X = latent(n, 128)
    nt = (n + 127) // 128
    T = max(int(np.ceil(0.1 * nt)), min(nt, 64))
    rows = np.random.default_rng(1).choice(n, 2000, replace=False)
    sa0 = StreamedAnnchor(X, n_anchors=32, n_neighbors=k, p_work=0.1, join_passes=0, join_extra=0).fit()
    assert sa0.tile_evals <= T * nt
    err0, _ = _recall_rows(sa0, X, rows, k)
    sa = StreamedAnnchor(X, n_anchors=32, n_neighbors=k, p_work=0.1).fit()   # join_passes = 2
    assert sa.p_work == max(0.1, min(1.0, 64.0 / nt))
    assert sa.tile_evals <= T * nt   # the work budget covers the joins
    err, td = _recall_rows(sa, X, rows, k)
    assert err < err0
    print("N=%d: recall %.4f (tile phase only: %.4f)" % (n, 1 - err / (len(rows) * float(k)), 1 - err0 / (len(rows) * float(k))))
    assert err <= (1 - bar) * len(rows) * k, (err, err0)
    # float tolerance: float32 norms, rtol 1e-5 -- every reported distance is the reported pair's distance
    idx, dist = sa.neighbor_graph
    for r in rows[:40]:
        dd = np.sqrt(((X[idx[r]].astype(np.float64) - X[r].astype(np.float64)) ** 2).sum(axis=1))
        np.testing.assert_allclose(dd, dist[r], rtol=1e-5, atol=1e-6)


def test_c3_full_size_recall():
    """BASELINE configs[2] at its stated size: synthetic Euclidean float32 N = 1 000 000, d = 128
    (SURVEY.md section 8d recipe), n_anchors = 32, k = 15, p_work = 0.1.  Truth = exact k-NN of a fixed
    10 000-row subset (tile kernel with the full budget).  recall@15 >= 0.99; every reported distance
    equals the float32 norm of the reported pair at rtol 1e-5."""
    from annchor_amd import Annchor

    n, k = 1_000_000, 15
    X = latent(n, 128)
    ann = Annchor(X, "euclidean", n_anchors=32, n_neighbors=k, p_work=0.1, random_seed=42).fit()
    sa = ann._streamed
    assert sa is not None and sa.join_passes == 2
    idx, dist = ann.neighbor_graph
    assert idx.shape == (n, k) and np.array_equal(idx[:, 0], np.arange(n)) and np.all(dist[:, 0] == 0)
    assert np.all(np.diff(dist, axis=1) >= 0)
    nt = (n + 127) // 128
    assert sa.tile_evals <= int(np.ceil(0.1 * nt)) * nt   # the whole budget, joins included
    rows = np.sort(np.random.default_rng(99).choice(n, 10000, replace=False))
    err, td = _recall_rows(sa, X, rows, k)
    recall = 1 - err / (len(rows) * float(k))
    assert recall >= 0.99, recall
    Xr, Xn = X[rows].astype(np.float64), X[idx[rows]].astype(np.float64)
    dd = np.sqrt(((Xn - Xr[:, None, :]) ** 2).sum(-1))
    np.testing.assert_allclose(dd, dist[rows], rtol=1e-5, atol=1e-5)
    # no neighbour listed twice, never the row itself
    srt = np.sort(idx[rows], axis=1)
    assert np.all(srt[:, 1:] != srt[:, :-1])
    # HEADLINE recall: against an INDEPENDENT float64 brute force (plain torch float64 matrix products on the GPU: none of this
    # build's kernels) on 2 500 of those rows; the 10 000-row figure above uses the tile kernel itself (full budget) as truth
    # and is cross-checked here against the independent one
    from test_c5_gpu import truth_f64
    from annchor_amd import compare_neighbor_graphs

    sel = np.arange(0, len(rows), 4)
    sub = rows[sel]
    bd = truth_f64(X[sub], [X], k)
    bd[:, 0] = 0.0                                       # the row itself (cancellation noise of the expanded form)
    np.testing.assert_allclose(td[sel][:, 1:], bd[:, 1:], rtol=2e-5, atol=1e-5)   # kernel truth == float64 truth
    e_ind = compare_neighbor_graphs((idx[sub], bd), (idx[sub], dist[sub]), k)
    recall_ind = 1 - e_ind / (len(sub) * float(k))
    print("C3: recall@15 %.4f on %d rows against the independent float64 truth (%.4f on %d rows against the tile kernel's own)"
          % (recall_ind, len(sub), recall, len(rows)))
    assert recall_ind >= 0.99


def test_dispatch_rules():
    """float64 data is never narrowed behind the caller's back: it takes the pair-list form in float64 as far as the
    device holds the candidate list (2^30 pairs / 80 % of free memory: 46 341 points on a 288 GB MI355X), beyond that
    the constructor refuses -- unless the caller opts into float32 with streamed='cast'; float32 data can be forced
    either way."""
    from annchor_amd import Annchor, _native

    X32 = latent(2000, 16)
    a = Annchor(X32, "euclidean", n_anchors=6, n_neighbors=5, p_work=0.5, streamed=True).fit()
    b = Annchor(X32, "euclidean", n_anchors=6, n_neighbors=5, p_work=1.0, streamed=False).fit()
    assert a._streamed is not None and b._streamed is None
    with pytest.raises(NotImplementedError):
        a.get_sample()
    with pytest.raises(ValueError):
        Annchor(X32.astype(np.float64), "euclidean", streamed=True)
    lim = _native.pairlist_point_limit(0)
    assert 30000 < lim <= 46341
    big = np.zeros((lim + 1, 4))
    with pytest.raises(ValueError):
        Annchor(big, "euclidean")
    with pytest.raises(ValueError):
        Annchor(np.zeros((lim + 1, 4), dtype=np.float32), "euclidean", streamed=False)
    mid = latent(21000, 8).astype(np.float64)
    c = Annchor(mid, "euclidean", n_anchors=8, n_neighbors=5, p_work=0.02)
    assert c._streamed is None   # float64: pair-list form, computed in float64
    d = Annchor(latent(31000, 8).astype(np.float64), "euclidean", n_anchors=8, n_neighbors=5, p_work=0.02)
    assert d._streamed is None   # still the pair-list form above 30 000 points (float64 input is not narrowed)
    e = Annchor(latent(31000, 8).astype(np.float64), "euclidean", n_anchors=8, n_neighbors=5, p_work=0.5, streamed="cast")
    assert e._streamed is not None   # the explicit opt-in


def test_pair_list_form_above_30000_points():
    """Slow-metric-shaped use above the old 30 000-point cap: float64 Euclidean, 34 000 points (578 M candidate pairs,
    ~70 GB of pair-list state), order-free sampler; exact rows of a subset as truth."""
    from annchor_amd import Annchor, compare_neighbor_graphs
    from annchor_amd.samplers import DeviceStratifiedSampler

    n, k = 34000, 10
    X = latent(n, 24).astype(np.float64)
    ann = Annchor(X, "euclidean", n_anchors=20, n_neighbors=k, p_work=0.05, sampler=DeviceStratifiedSampler()).fit()
    assert ann._streamed is None and ann.n_pairs > 4e8
    rows = np.random.default_rng(8).choice(n, 300, replace=False)
    bi, bd = brute(X, rows, k)
    err = compare_neighbor_graphs((bi, bd), (ann.neighbor_graph[0][rows], ann.neighbor_graph[1][rows]), k)
    assert err <= 0.01 * len(rows) * k, err
    ann._engine.close()


def test_pair_list_form_beyond_the_complete_list_needs_locality(monkeypatch):
    """Above the size whose complete pair list fits the device the constructor asks for a locality filter that thins the
    candidates (refused with the default loc_thresh=1, accepted with loc_thresh >= 2: the count is checked after the anchors)."""
    import annchor_amd.annchor as A
    from annchor_amd import Annchor

    monkeypatch.setattr(A, "PAIRLIST_HARD_MAX", 31000)
    X = latent(32000, 8).astype(np.float64)
    with pytest.raises(ValueError, match="locality filter"):
        Annchor(X, "euclidean", n_anchors=8, n_neighbors=5, p_work=0.05, streamed=False)
    a = Annchor(X, "euclidean", n_anchors=8, n_neighbors=5, p_work=0.05, streamed=False, loc_thresh=2)
    assert a._streamed is None


def test_levenshtein_60000_points_with_locality():
    """Slow metric beyond 46 341 points: 60 000 clustered strings, the locality filter (3 of the 5 nearest of 40 anchors in
    common) keeps the candidate list under 2^30 pairs; recall against exact rows of a subset."""
    from annchor_amd import Annchor, compare_neighbor_graphs
    from annchor_amd.datasets import synthetic_string_clusters
    from annchor_amd.samplers import DeviceStratifiedSampler

    n, k = 60000, 15
    X = synthetic_string_clusters(n)
    ann = Annchor(X, "levenshtein", n_anchors=40, n_neighbors=k, p_work=0.02, locality=5, loc_thresh=3,
                  sampler=DeviceStratifiedSampler()).fit()
    assert ann._streamed is None and 1e8 < ann.n_pairs < 2 ** 30
    rows = np.random.default_rng(3).choice(n, 100, replace=False)
    err = 0
    for r in rows:
        d = ann._engine.metric_pairs(np.stack([np.full(n, r), np.arange(n)], axis=1))
        d[r] = -1
        want = np.sort(d)[:k]
        want[0] = 0
        z = np.zeros((1, k), dtype=np.int64)
        err += compare_neighbor_graphs((z, want[None, :]), (z, ann.neighbor_graph[1][r][None, :]), k)
    assert err <= 0.08 * len(rows) * k, err
    ann._engine.close()


def test_device_pointer_tensor_view():
    import torch

    from annchor_amd import _native
    from annchor_amd.streamed import device_tensor_u8

    eng = _native.Engine(0)
    p = eng.device_alloc(64)
    src = np.arange(64, dtype=np.uint8)
    eng.device_copy(p, src.ctypes.data, 64, "h2d")
    t = device_tensor_u8(p, 64, 0)
    assert t.is_cuda and t.data_ptr() == p and torch.equal(t.cpu(), torch.from_numpy(src))
    eng.device_free(p)


def _worker(rank, world, port, out):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from annchor_amd.streamed import StreamedAnnchor, TorchComm

    X = latent(6000, 64)
    cuts = [0, 3300, 6000]
    sa = StreamedAnnchor(X[cuts[rank]:cuts[rank + 1]], n_anchors=12, n_neighbors=10, p_work=1.0, base=cuts[rank],
                         comm=TorchComm(), device=0).fit()
    gi, gd = sa.gather_graph()
    if rank == 0:
        np.savez(out, A=sa.A, idx=gi, dist=gd)
    dist.destroy_process_group()


def test_two_ranks_row_sharded_equal_one_rank(tmp_path):
    """Row-sharded path with a real exchange step (host-staged all-gather under gloo; both
    ranks share the one GPU of the test box)."""
    import torch.multiprocessing as mp

    from annchor_amd.streamed import StreamedAnnchor

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "w2.npz")
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    R = np.load(out)
    one = StreamedAnnchor(latent(6000, 64), n_anchors=12, n_neighbors=10, p_work=1.0).fit()
    assert np.array_equal(R["A"], one.A)
    np.testing.assert_allclose(R["dist"], one.neighbor_graph[1], rtol=1e-6, atol=1e-6)
    same = (R["idx"] == one.neighbor_graph[0]).mean()
    assert same > 0.999   # identical up to exact-tie order between differently tiled runs


def _worker_budgeted(rank, world, port, out):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from annchor_amd.streamed import StreamedAnnchor, TorchComm

    X = latent(40000, 64)
    cuts = [0, 21000, 40000]
    sa = StreamedAnnchor(X[cuts[rank]:cuts[rank + 1]], n_anchors=16, n_neighbors=10, p_work=0.25, base=cuts[rank],
                         comm=TorchComm(), device=0).fit()
    gi, gd = sa.gather_graph()
    ev = sa.comm.allgather_small((sa.tile_evals,)).sum()
    if rank == 0:
        np.savez(out, idx=gi, dist=gd, tile_evals=ev, nt=sa.n_tiles_total)
    dist.destroy_process_group()


def _worker_budgeted_k80(rank, world, port, out):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from annchor_amd.streamed import StreamedAnnchor, TorchComm

    X = latent(24000, 64)
    cuts = [0, 13000, 24000]
    sa = StreamedAnnchor(X[cuts[rank]:cuts[rank + 1]], n_anchors=12, n_neighbors=80, p_work=0.3, base=cuts[rank],
                         comm=TorchComm(), device=0).fit()
    gi, gd = sa.gather_graph()
    if rank == 0:
        np.savez(out, idx=gi, dist=gd)
    dist.destroy_process_group()


def test_two_ranks_budgeted_at_80_neighbours(tmp_path):
    """The row-sharded protocol (lists all-gathered between join passes, finished rows routed to their owners) with lists of
    79 entries -- the split-list exact kernels: the two-rank graph equals the one-rank graph (one global tile order)."""
    import torch.multiprocessing as mp

    from annchor_amd.streamed import StreamedAnnchor

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "w80.npz")
    mp.spawn(_worker_budgeted_k80, args=(2, port, out), nprocs=2, join=True)
    R = np.load(out)
    one = StreamedAnnchor(latent(24000, 64), n_anchors=12, n_neighbors=80, p_work=0.3).fit()
    assert R["idx"].shape == (24000, 80)
    same = (R["idx"] == one.neighbor_graph[0]).mean()
    assert same > 0.999, same
    np.testing.assert_allclose(R["dist"], one.neighbor_graph[1], rtol=1e-6, atol=1e-6)


def test_two_ranks_budgeted_with_join_passes(tmp_path):
    """Row-sharded build with a binding budget: tile phase per rank, neighbour lists all-gathered
    before each join pass (annchor_stream_knn_begin / _join / _end), graph gathered at the end.
    The two-rank graph is not bit-equal to the one-rank graph (each rank tiles its own shard) but
    must reach the same quality inside the same budget."""
    import torch.multiprocessing as mp

    from annchor_amd import compare_neighbor_graphs
    from annchor_amd.streamed import StreamedAnnchor

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "w2b.npz")
    mp.spawn(_worker_budgeted, args=(2, port, out), nprocs=2, join=True)
    R = np.load(out)
    X = latent(40000, 64)
    k = 10
    one = StreamedAnnchor(X, n_anchors=16, n_neighbors=k, p_work=0.25).fit()
    nojoin = StreamedAnnchor(X, n_anchors=16, n_neighbors=k, p_work=0.25, join_passes=0, join_extra=0).fit()
    rows = np.random.default_rng(2).choice(40000, 1500, replace=False)
    ti, td = one.query(X[rows], nn=k, p_work=1.0)
    e_two = compare_neighbor_graphs((ti, td), (R["idx"][rows], R["dist"][rows]), k)
    e_one = compare_neighbor_graphs((ti, td), (one.neighbor_graph[0][rows], one.neighbor_graph[1][rows]), k)
    e_nojoin = compare_neighbor_graphs((ti, td), (nojoin.neighbor_graph[0][rows], nojoin.neighbor_graph[1][rows]), k)
    nt = int(R["nt"])
    assert int(R["tile_evals"]) <= int(np.ceil(0.25 * nt)) * nt
    assert np.array_equal(R["idx"][:, 0], np.arange(40000))
    assert e_two < e_nojoin and e_two <= 2.0 * e_one + 0.01 * len(rows) * k, (e_two, e_one, e_nojoin)


def test_annchor_api_dispatches_large_euclidean_to_streamed_form():
    from annchor_amd import Annchor

    X = latent(31000, 32)
    ann = Annchor(X, "euclidean", n_anchors=8, n_neighbors=6, p_work=1.0).fit()
    assert ann._streamed is not None and ann.neighbor_graph[0].shape == (31000, 6)
    rows = np.arange(0, 31000, 701)
    bi, bd = brute(X, rows, 6)
    np.testing.assert_allclose(ann.neighbor_graph[1][rows], bd, rtol=1e-5, atol=1e-6)
    assert len(ann.A) == 8 and ann.evals > 0
    assert Annchor(X[:21000], "euclidean", n_anchors=8, n_neighbors=6, p_work=0.02)._streamed is None   # by size: pair-list form


def test_nccl_collective_path_single_rank():
    """The RCCL branch of the exchange (device-pointer tensor views, all_gather_into_tensor,
    CUDA broadcast) with a one-rank `nccl` group: same graph as without collectives."""
    import torch
    import torch.distributed as dist

    from annchor_amd.streamed import StreamedAnnchor, TorchComm

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        X = latent(4000, 64)
        a = StreamedAnnchor(X, n_anchors=8, n_neighbors=10, p_work=1.0, comm=TorchComm(), force_exchange=True).fit()
        b = StreamedAnnchor(X, n_anchors=8, n_neighbors=10, p_work=1.0).fit()
        assert a.comm.backend == "nccl"
        assert np.array_equal(a.A, b.A)
        assert np.array_equal(a.neighbor_graph[0], b.neighbor_graph[0])
        assert np.array_equal(a.neighbor_graph[1], b.neighbor_graph[1])
        gi, gd = a.gather_graph()
        assert np.array_equal(gi, a.neighbor_graph[0])
    finally:
        dist.destroy_process_group()


def test_in_library_rccl_single_rank():
    """The collectives from inside the library (csrc/comm.hip: RCCL by dlopen, enqueued on the engine's stream; the anchor
    rounds as ONE C call) with a one-rank communicator made from a unique id -- no torch anywhere: every branch of the sharded
    path (candidate all-gathers inside annchor_stream_anchor_rounds, rows, neighbour lists, the all-to-all of the finished
    rows as grouped send / recv, gather_graph) gives the graph of the collective-free build."""
    from annchor_amd import _native
    from annchor_amd.streamed import RcclComm, StreamedAnnchor

    X = latent(5000, 48)
    eng = _native.Engine(0)
    comm = RcclComm(eng, 1, 0, _native.comm_unique_id())
    try:
        a = StreamedAnnchor(X, n_anchors=8, n_neighbors=10, p_work=0.5, comm=comm, engine=eng, force_exchange=True).fit()
        b = StreamedAnnchor(X, n_anchors=8, n_neighbors=10, p_work=0.5).fit()
        assert np.array_equal(a.A, b.A)
        assert np.array_equal(a.neighbor_graph[0], b.neighbor_graph[0])
        assert np.array_equal(a.neighbor_graph[1], b.neighbor_graph[1])
        gi, gd = a.gather_graph()
        assert np.array_equal(gi, a.neighbor_graph[0]) and np.array_equal(gd, a.neighbor_graph[1])
        assert np.array_equal(comm.allgather_small((3.0, 4.5)), [[3.0, 4.5]])
    finally:
        comm.close()
        eng.close()


def test_in_library_rccl_side_communicator_preflight_and_overlap():
    """RcclComm with a second communicator on a stream of its own: the pre-flight (a checked 1 KB all-gather on both communicators),
    then a fit whose rows' all-gather is started BEFORE the anchor rounds on the side stream (`allgather_begin`) and joined where
    the library first reads the gathered rows -- equal shards (joined in annchor_stream_order_end) and a shard that is not the largest
    of the declared counts cannot be made with one rank, so the compaction branch is exercised through annchor_comm_side_join by
    hand.  Same graph as the collective-free build; two fits on the same engine."""
    from annchor_amd import _native
    from annchor_amd.streamed import RcclComm, StreamedAnnchor

    X = latent(6000, 128)
    eng = _native.Engine(0)
    comm = RcclComm(eng, 1, 0, _native.comm_unique_id(), side_id=_native.comm_unique_id(), preflight=30.0, timeout=120.0)
    try:
        assert comm.overlap
        b = StreamedAnnchor(X, n_anchors=8, n_neighbors=10, p_work=0.5).fit()
        for _ in range(2):
            a = StreamedAnnchor(X, n_anchors=8, n_neighbors=10, p_work=0.5, comm=comm, engine=eng, force_exchange=True).fit()
            assert np.array_equal(a.A, b.A)
            assert np.array_equal(a.neighbor_graph[0], b.neighbor_graph[0])
            assert np.array_equal(a.neighbor_graph[1], b.neighbor_graph[1])
        # the side all-gather by hand: begin, other work on the engine stream, join, read
        n = 1 << 20
        src, dst = eng.device_alloc(n), eng.device_alloc(n)
        host = np.arange(n, dtype=np.uint8)
        eng.device_copy(src, host.ctypes.data, n, "h2d")
        comm.allgather_begin(eng, src, dst, n)
        eng.comm_side_join()
        out = np.zeros(n, dtype=np.uint8)
        eng.device_copy(out.ctypes.data, dst, n, "d2h")
        assert np.array_equal(out, host)
        eng.device_free(src); eng.device_free(dst)
    finally:
        comm.close()
        eng.close()


def test_in_library_rccl_dead_peer_guard():
    """A host wait of an engine with a communicator that lasts longer than the timeout aborts the communicators and raises
    "collective timed out" instead of blocking for good (csrc/comm.hip: the watchdog armed around every host wait).  A peer cannot be
    killed on one GPU, so the wait is made long instead: a 2 x 10^6-row build's tile phase against a 20 ms limit."""
    from annchor_amd import _native
    from annchor_amd.streamed import RcclComm, StreamedAnnchor

    X = latent(2_000_000, 128)
    eng = _native.Engine(0)
    comm = RcclComm(eng, 1, 0, _native.comm_unique_id(), preflight=30.0)
    try:
        eng.comm_set_timeout(0.02)
        with pytest.raises(Exception, match="collective timed out"):
            StreamedAnnchor(X, n_anchors=32, n_neighbors=15, p_work=0.1, comm=comm, engine=eng, force_exchange=True).fit()
    finally:
        try:
            comm.close()
        except Exception:
            pass
        eng.close()


def test_streamed_query_matches_brute_force():
    """Annchor.query for the streamed form: exact with the full budget; with a partial budget the
    recall depends on how dense the query batch is (the budget is spent per 128-query tile)."""
    from annchor_amd import Annchor, compare_neighbor_graphs
    from annchor_amd.streamed import StreamedAnnchor

    n, nq, k = 30000, 4000, 10
    Z = latent(n + nq, 64)
    X, Q = Z[:n], Z[n:]
    sa = StreamedAnnchor(X, n_anchors=16, n_neighbors=8, p_work=1.0).fit()
    Xd, Qd = X.astype(np.float64), Q.astype(np.float64)
    d2 = np.maximum((Qd ** 2).sum(1)[:, None] + (Xd ** 2).sum(1)[None, :] - 2.0 * Qd @ Xd.T, 0)
    bi = np.argsort(d2, axis=1, kind="stable")[:, :k]
    bd = np.sqrt(((Qd[:, None, :] - Xd[bi]) ** 2).sum(-1))   # exact distances of the true neighbours
    idx, dist = sa.query(Q, nn=k, p_work=1.0)
    assert idx.shape == (nq, k) and np.all(np.diff(dist, axis=1) >= 0)
    np.testing.assert_allclose(dist, bd, rtol=1e-5, atol=1e-6)
    # reported pairs are real: distance of (query, reported row) equals the reported distance
    for r in range(0, nq, 211):
        dd = np.sqrt(((Xd[idx[r]] - Qd[r]) ** 2).sum(axis=1))
        np.testing.assert_allclose(dd, dist[r], rtol=1e-5, atol=1e-6)
    idx2, dist2 = sa.query(Q, nn=k, p_work=0.25)
    err = compare_neighbor_graphs((bi, bd), (idx2, dist2), k)
    assert err <= 0.25 * nq * k, err   # 32 query tiles x 59 of 235 data tiles, tile phase only: recall >= 0.75 (0.81 measured; grows with N as in fit())
    # a single query row, and the Annchor front end (dispatches large Euclidean data to this form)
    i1, d1 = sa.query(Q[:1], nn=3, p_work=1.0)
    np.testing.assert_allclose(d1[0], bd[0, :3], rtol=1e-5, atol=1e-6)
    # 100 neighbours per query: lists beyond 64 entries (two workgroups per query tile)
    i100, d100 = sa.query(Q[:300], nn=100, p_work=1.0)
    b100 = np.sqrt(np.sort(d2[:300], axis=1)[:, :100])
    np.testing.assert_allclose(d100, b100, rtol=1e-5, atol=2e-5)
    ann = Annchor(X, "euclidean", n_anchors=16, n_neighbors=8, p_work=1.0, streamed=True).fit()
    i3, d3 = ann.query(Q[:100], nn=k, p_work=1.0)
    np.testing.assert_allclose(d3, bd[:100], rtol=1e-5, atol=1e-6)


def test_annchor_cosine_large_n_uses_streamed_form():
    """'cosine' above the pair-list size: rows normalised, streamed Euclidean form, distances
    mapped back with d_cos = d_euclid^2 / 2 (exact on the unit sphere).  Tolerance 2e-6 absolute
    (float32 rows; scipy's cosine on float32 data is no tighter)."""
    from annchor_amd import Annchor

    n, k = 21000, 8
    X = latent(n, 48) + 0.3
    ann = Annchor(X, "cosine", n_anchors=12, n_neighbors=k, p_work=1.0, streamed=True).fit()
    idx, dist = ann.neighbor_graph
    Xn = X.astype(np.float64) / np.linalg.norm(X.astype(np.float64), axis=1)[:, None]
    rows = np.random.default_rng(4).choice(n, 300, replace=False)
    C = 1.0 - Xn[rows] @ Xn.T
    C[np.arange(300), rows] = -1.0
    want = np.sort(C, axis=1)[:, :k]
    want[:, 0] = 0.0
    np.testing.assert_allclose(dist[rows], want, rtol=0, atol=2e-6)
    qi, qd = ann.query(X[:50] * 3.0, nn=4, p_work=1.0)   # scaling a query does not change its cosine distances
    assert np.array_equal(qi[:, 0], np.arange(50)) and np.all(qd[:, 0] < 2e-6)


def _worker_many(rank, world, port, out, n, cuts, p_work):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from annchor_amd.streamed import StreamedAnnchor, TorchComm

    X = latent(n, 64)
    sa = StreamedAnnchor(X[cuts[rank]:cuts[rank + 1]], n_anchors=12, n_neighbors=10, p_work=p_work, base=cuts[rank],
                         comm=TorchComm(), device=0).fit()
    own = sa.neighbor_graph
    assert np.array_equal(own[0][:, 0], np.arange(cuts[rank], cuts[rank + 1]))
    gi, gd = sa.gather_graph()
    ev = sa.comm.allgather_small((sa.tile_evals,)).sum()
    if rank == 0:
        np.savez(out, A=sa.A, idx=gi, dist=gd, tile_evals=ev, nt=sa.n_tiles_total)
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [4, 8])
def test_many_ranks_share_gpu_rehearsal(tmp_path, world):
    """4- and 8-rank rehearsal of the row-sharded build (all ranks on the one GPU of the box, gloo around the same
    device-pointer protocol) at BASELINE configs[4]'s shape ratios: N not a multiple of 128 x world, a shorter last
    shard, the tile count padded to a multiple of the rank count.  Full budget: every rank count gives the exact graph."""
    import torch.multiprocessing as mp

    from annchor_amd.streamed import StreamedAnnchor

    n = 128 * 41 + 77                       # 42 tiles -> padded to 44 (4 ranks) / 48 (8 ranks)
    per = -(-n // world)
    cuts = [min(r * per, n) for r in range(world + 1)]
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "wm.npz")
    mp.spawn(_worker_many, args=(world, port, out, n, cuts, 1.0), nprocs=world, join=True)
    R = np.load(out)
    one = StreamedAnnchor(latent(n, 64), n_anchors=12, n_neighbors=10, p_work=1.0).fit()
    assert np.array_equal(R["A"], one.A)
    np.testing.assert_allclose(R["dist"], one.neighbor_graph[1], rtol=1e-6, atol=1e-6)
    assert (R["idx"] == one.neighbor_graph[0]).mean() > 0.999


def test_four_ranks_budgeted_join_passes(tmp_path):
    """Binding budget on four ranks: tile phase per rank, lists all-gathered before every join pass, rows routed back
    to their owners; quality inside the budget as on one rank."""
    import torch.multiprocessing as mp

    from annchor_amd import compare_neighbor_graphs
    from annchor_amd.streamed import StreamedAnnchor

    n, k, world = 40000 + 53, 10, 4
    per = -(-n // world)
    cuts = [min(r * per, n) for r in range(world + 1)]
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "w4b.npz")
    mp.spawn(_worker_many, args=(world, port, out, n, cuts, 0.25), nprocs=world, join=True)
    R = np.load(out)
    X = latent(n, 64)
    one = StreamedAnnchor(X, n_anchors=12, n_neighbors=k, p_work=0.25).fit()
    rows = np.random.default_rng(2).choice(n, 1500, replace=False)
    ti, td = one.query(X[rows], nn=k, p_work=1.0)
    e_many = compare_neighbor_graphs((ti, td), (R["idx"][rows], R["dist"][rows]), k)
    e_one = compare_neighbor_graphs((ti, td), (one.neighbor_graph[0][rows], one.neighbor_graph[1][rows]), k)
    nt = int(R["nt"])
    assert int(R["tile_evals"]) <= int(np.ceil(0.25 * nt)) * nt
    assert np.array_equal(R["idx"][:, 0], np.arange(n))
    assert e_many <= 2.0 * e_one + 0.01 * len(rows) * k, (e_many, e_one)


def test_fused_anchor_distances_equal_the_sweeps():
    """Row-sharded runs recompute the anchor distances of ALL rows in one pass (k_sh_all_anchor_dists); it must
    reproduce the per-anchor sweeps bit for bit -- the global tile order is built from them."""
    from annchor_amd.streamed import StreamedAnnchor

    for n, d in ((5000, 128), (3001, 20), (1500, 200), (900, 37)):
        X = latent(n, d)
        a = StreamedAnnchor(X, n_anchors=9, n_neighbors=6, p_work=1.0, force_exchange=True).fit()
        b = StreamedAnnchor(X, n_anchors=9, n_neighbors=6, p_work=1.0).fit()
        assert np.array_equal(a.A, b.A)
        assert np.array_equal(a.neighbor_graph[0], b.neighbor_graph[0]) and np.array_equal(a.neighbor_graph[1], b.neighbor_graph[1])
        gi, gd = a.gather_graph()
        assert np.array_equal(gi, a.neighbor_graph[0]) and np.array_equal(gd, a.neighbor_graph[1])
        qa, da = a.query(X[:64], nn=4, p_work=1.0)
        qb, db = b.query(X[:64], nn=4, p_work=1.0)
        assert np.array_equal(qa, qb) and np.array_equal(da, db)


def _truth_rows(X, rows, k):
    """exact float64 distances (direct differences) of `rows` to all points, k smallest incl. the row itself"""
    Xd = X.astype(np.float64)
    out = []
    for r in rows:
        d = np.sqrt(((Xd - Xd[r][None, :]) ** 2).sum(axis=1))
        d[r] = 0.0
        out.append(np.sort(d)[:k])
    return np.array(out)


def test_split_fp16_tile_kernel_centres_the_rows():
    """The tile kernel evaluates |x|^2 + |y|^2 - 2 x.y on fp16 hi + lo halves (csrc/knnbf.hip): rows far from the origin
    would lose their neighbours' distances in |x|^2 (and leave fp16's range).  The split copy is centred on the anchors' mean
    and scaled by a power of two, so a data set shifted
    by 1000 in every coordinate gives the exact graph like the unshifted one (full budget, rtol 1e-5 against float64
    differences of the same float32 rows), on the split kernel, with (almost) no row flagged by its guard."""
    from annchor_amd.streamed import StreamedAnnchor

    n, k = 6000, 15
    X = (latent(n, 128) + 1000.0).astype(np.float32)
    sa = StreamedAnnchor(X, n_anchors=16, n_neighbors=k, p_work=1.0).fit()
    kind, flagged = sa._engine.stream_last_kernel(with_guard=True)
    assert kind == 1 and flagged <= n // 200, (kind, flagged)
    rows = np.random.default_rng(0).choice(n, 500, replace=False)
    np.testing.assert_allclose(sa.neighbor_graph[1][rows], _truth_rows(X, rows, k), rtol=1e-5, atol=1e-6)


def test_split_fp16_guard_repairs_flagged_rows_exactly(monkeypatch):
    """Tight clusters far from the centre (|x - c|^2 ~ 10^4 d^2): float32-grade products of |x|^2 (the split products are
    good to ~2^-22 |x||y|, like the f32 MFMA stream) no longer resolve the neighbours' distances.  The kernel's guard -- K-th exact
    distance within twice the measured error of the list's last approximate entry -- flags the rows, and their row tiles are done
    again with float32 DIFFERENCES (csrc/repair.hip: the reference's np.linalg.norm(x - y), distances.py:8-13): the graph is the
    float64 brute-force graph (no errors at all on 400 rows; the old fallback -- the phase repeated on the exact-f32 MFMA kernel --
    evaluates the same expanded form and was allowed 1 % errors here).  On well-conditioned data of the same size nothing is
    flagged."""
    from annchor_amd import compare_neighbor_graphs
    from annchor_amd.streamed import StreamedAnnchor

    rng = np.random.default_rng(3)
    n, k, d = 20000, 10, 16
    cent = rng.standard_normal((400, d)) * 30.0
    X = (cent[rng.integers(0, 400, n)] + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
    sa = StreamedAnnchor(X, n_anchors=12, n_neighbors=k, p_work=1.0).fit()
    kind, flagged = sa._engine.stream_last_kernel(with_guard=True)
    assert kind == 1 and flagged > n // 200, (kind, flagged)   # flagged by the split kernel, repaired in place
    rows = rng.choice(n, 400, replace=False)
    bd = _truth_rows(X, rows, k)
    err = compare_neighbor_graphs((sa.neighbor_graph[0][rows], bd), (sa.neighbor_graph[0][rows], sa.neighbor_graph[1][rows]), k)
    assert err == 0, err
    np.testing.assert_allclose(sa.neighbor_graph[1][rows], bd, rtol=1e-5, atol=1e-6)
    good = StreamedAnnchor(latent(n, 64), n_anchors=12, n_neighbors=k, p_work=0.3).fit()
    kind, flagged = good._engine.stream_last_kernel(with_guard=True)
    assert kind == 1 and flagged <= n // 1000, (kind, flagged)


@pytest.mark.parametrize("seed", [11, 77])
def test_two_stage_kernel_random_shapes_are_exact_at_full_budget(monkeypatch, seed):
    """k_st_knnh's shapes (padded dimension 128, <= 14 neighbours kept) over random N / dimension / k / anchor counts, duplicated rows,
    data far from the origin, a tight cluster beside a wide cloud, through the one-call entry point and the sharded one: with the full
    budget (and the sharded path's early stop switched off) the graph is the exact k-NN graph -- float64 brute force on 300 rows, the
    reference's definition (annchor/distances.py:8-13 on every pair) --, and two builds at a small budget agree bit for bit
    (tools/stress_knnh.py is the long form: 60 cases)."""
    from annchor_amd.streamed import StreamedAnnchor

    monkeypatch.setenv("ANNCHOR_ST_EARLY_WINDOW", "0")
    rng = np.random.default_rng(seed)
    for case in range(5):
        n = int(rng.integers(1500, 40000)); dim = int(rng.choice([65, 100, 127, 128])); k = int(rng.integers(2, 16))
        na = int(rng.integers(2, 40)); lat = int(rng.integers(2, 10))
        X = (rng.standard_normal((n, lat)) @ rng.standard_normal((lat, dim)) + 0.05 * rng.standard_normal((n, dim))).astype(np.float32)
        if case % 3 == 0:
            X[rng.integers(0, n, n // 10)] = X[rng.integers(0, n, n // 10)]
        if case % 4 == 1:
            X += (30.0 * rng.standard_normal((1, dim))).astype(np.float32)
        if case % 5 == 2:
            X[: n // 2] = (X[: n // 2] * 1e-2 + X[0]).astype(np.float32)
        sa = StreamedAnnchor(X, n_anchors=na, n_neighbors=k, p_work=1.0, force_exchange=bool(case % 2)).fit()
        assert sa._engine.stream_last_tile_kernels()[0], "the two-stage kernel did not run"
        idx, dist = sa.neighbor_graph
        Xd = X.astype(np.float64)
        rows = rng.choice(n, 300, replace=False)
        d2 = np.maximum((Xd[rows] ** 2).sum(1)[:, None] + (Xd ** 2).sum(1)[None, :] - 2.0 * Xd[rows] @ Xd.T, 0)
        d2[np.arange(len(rows)), rows] = -1
        truth = np.sqrt(np.maximum(np.sort(d2, axis=1)[:, :k], 0))
        scale = max(1.0, float(np.abs(Xd).max()))
        np.testing.assert_allclose(dist[rows], truth, rtol=3e-4, atol=3e-4 * scale, err_msg="case %d" % case)
        assert sc.knn_violations(X, rows, idx[rows], dist[rows], k, sc.gamma_of(128)) == [], "case %d" % case
        assert np.array_equal(idx[rows, 0], rows)
        rep = np.sqrt(((Xd[idx[rows]] - Xd[rows][:, None, :]) ** 2).sum(-1))
        np.testing.assert_allclose(rep, dist[rows], rtol=1e-4, atol=1e-4 * scale)
        a_ = StreamedAnnchor(X, n_anchors=na, n_neighbors=k, p_work=0.1).fit().neighbor_graph
        b_ = StreamedAnnchor(X, n_anchors=na, n_neighbors=k, p_work=0.1).fit().neighbor_graph
        assert np.array_equal(a_[0], b_[0]) and np.array_equal(a_[1], b_[1])


def test_guard_beyond_256_dimensions_repairs_exactly():
    """Beyond 256 dimensions there is no exact-f32 tile kernel: ill-conditioned data (tight clusters far from the centre) used to be
    reported and returned from the split selection.  Now the flagged rows' row tiles are evaluated again with float32 differences
    (csrc/repair.hip, any dimension): the graph equals the float64 brute force on the ill-conditioned set -- indices (no errors) and
    distances at rtol 1e-5 -- for the graph build and for queries."""
    from annchor_amd import compare_neighbor_graphs
    from annchor_amd.streamed import StreamedAnnchor

    rng = np.random.default_rng(3)
    n, k, d = 12000, 10, 300
    cent = rng.standard_normal((300, d)) * 30.0
    X = (cent[rng.integers(0, 300, n)] + 0.02 * rng.standard_normal((n, d))).astype(np.float32)
    sa = StreamedAnnchor(X, n_anchors=10, n_neighbors=k, p_work=1.0).fit()
    kind, flagged = sa._engine.stream_last_kernel(with_guard=True)
    assert kind == 1
    idx, dist = sa.neighbor_graph
    rows = rng.choice(n, 300, replace=False)
    bd = _truth_rows(X, rows, k)
    err = compare_neighbor_graphs((idx[rows], bd), (idx[rows], dist[rows]), k)
    assert err == 0, (err, flagged)
    np.testing.assert_allclose(dist[rows], bd, rtol=1e-5, atol=1e-5)
    dd = np.sqrt(((X[idx[rows]].astype(np.float64) - X[rows].astype(np.float64)[:, None, :]) ** 2).sum(-1))
    np.testing.assert_allclose(dd, dist[rows], rtol=1e-5, atol=1e-5)
    # queries: perturbed data rows against the same clusters
    Q = (X[rows[:100]] + 0.01 * rng.standard_normal((100, d))).astype(np.float32)
    qi, qd = sa.query(Q, nn=5, p_work=1.0)
    Xd = X.astype(np.float64)
    for t in range(100):
        dq = np.sqrt(((Xd - Q[t].astype(np.float64)[None, :]) ** 2).sum(axis=1))
        np.testing.assert_allclose(qd[t], np.sort(dq)[:5], rtol=1e-5, atol=1e-5)


def _worker_dims(rank, world, port, out):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from annchor_amd.streamed import StreamedAnnchor, TorchComm

    X = latent(5000, 300)
    cuts = [0, 2700, 5000]
    sa = StreamedAnnchor(X[cuts[rank]:cuts[rank + 1]], n_anchors=10, n_neighbors=10, p_work=1.0, base=cuts[rank],
                         comm=TorchComm(), device=0).fit()
    gi, gd = sa.gather_graph()
    if rank == 0:
        np.savez(out, A=sa.A, idx=gi, dist=gd)
    dist.destroy_process_group()


def test_two_ranks_beyond_256_dimensions(tmp_path):
    """The row-sharded build on rows of 300 dimensions (the k-blocked kernel in the tile phase and the join passes): two ranks
    give the one-rank graph."""
    import torch.multiprocessing as mp

    from annchor_amd.streamed import StreamedAnnchor

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "wd.npz")
    mp.spawn(_worker_dims, args=(2, port, out), nprocs=2, join=True)
    R = np.load(out)
    one = StreamedAnnchor(latent(5000, 300), n_anchors=10, n_neighbors=10, p_work=1.0).fit()
    assert np.array_equal(R["A"], one.A)
    np.testing.assert_allclose(R["dist"], one.neighbor_graph[1], rtol=1e-6, atol=1e-6)
    assert (R["idx"] == one.neighbor_graph[0]).mean() > 0.999


def test_tiled_ranking_pass_equals_the_in_kernel_ranking(monkeypatch):
    """The rank keys and bounds of all (row tile, column tile) pairs come from one tiled pass ahead of the tile kernel
    (k_st_rank_pairs: 12 bytes of table traffic per pair instead of 384 -- the O(n_tiles^2) ranking was more than half of the tile
    kernel at N = 8 x 10^6).  Same arithmetic in the same order: the graph is bit for bit the one of the in-kernel ranking
    (ANNCHOR_ST_RANK_IN_KERNEL=1), for the 128-dimension kernel, the k-blocked one, the exact-f32 one and the query path."""
    from annchor_amd.streamed import StreamedAnnchor

    for n, d, k, pw in ((150000, 128, 15, 0.1), (40000, 300, 15, 0.25), (30000, 64, 40, 0.3), (20000, 20, 8, 1.0)):
        X = latent(n, d)
        monkeypatch.delenv("ANNCHOR_ST_RANK_IN_KERNEL", raising=False)
        a = StreamedAnnchor(X, n_anchors=24, n_neighbors=k, p_work=pw).fit()
        qa = a.query(X[:300] + 0.01, nn=5, p_work=0.3)
        monkeypatch.setenv("ANNCHOR_ST_RANK_IN_KERNEL", "1")
        b = StreamedAnnchor(X, n_anchors=24, n_neighbors=k, p_work=pw).fit()
        qb = b.query(X[:300] + 0.01, nn=5, p_work=0.3)
        assert a.tile_evals == b.tile_evals, (n, d)
        assert np.array_equal(a.neighbor_graph[0], b.neighbor_graph[0]), (n, d)
        # (distances: bit for bit where the same kernels ran; at 128 dimensions the pre-ranked build continues in the two-stage kernel
        # k_st_knnh, whose float32 sums (x - y)^2 are taken in a different order -- the same neighbours, the last bit of a distance)
        if d == 128:
            np.testing.assert_allclose(a.neighbor_graph[1], b.neighbor_graph[1], rtol=3e-7, atol=0)
        else:
            assert np.array_equal(a.neighbor_graph[1], b.neighbor_graph[1]), (n, d)
        assert np.array_equal(qa[0], qb[0]) and np.array_equal(qa[1], qb[1]), (n, d)
        a._engine.close(); b._engine.close()


def test_short_list_selection_equals_the_row_sweeps(monkeypatch):
    """Beyond 8192 column tiles the selection rounds of the 128-dimension tile kernel select from a short list (one histogram
    sweep + one copy sweep of the scratch row per ~2048 eligible tiles) instead of sweeping the row four times per round: the same
    tiles in the same order, the same graph bit for bit (forced here at small sizes; ANNCHOR_ST_NO_SHORT_LIST=1 = the sweeps)."""
    import subprocess

    code = """
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from test_streamed_gpu import latent
from annchor_amd.streamed import StreamedAnnchor
out = []
for n, d, k, pw in ((200000, 128, 15, 0.1), (60000, 64, 12, 0.5), (30000, 32, 8, 1.0)):
    sa = StreamedAnnchor(latent(n, d), n_anchors=24, n_neighbors=k, p_work=pw).fit()
    out.append((sa.tile_evals, sa.neighbor_graph[0], sa.neighbor_graph[1]))
np.savez(sys.argv[1], **{"a%%d_%%d" %% (i, j): np.asarray(v) for i, o in enumerate(out) for j, v in enumerate(o)})
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    import tempfile

    res = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, env in (("list", {"ANNCHOR_ST_SHORT_LIST_MIN": "0"}), ("sweep", {"ANNCHOR_ST_NO_SHORT_LIST": "1"})):
            out = os.path.join(tmp, name + ".npz")
            r = subprocess.run([sys.executable, "-c", code, out], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            res.append(dict(np.load(out)))
    assert res[0].keys() == res[1].keys()
    for key in res[0]:
        assert np.array_equal(res[0][key], res[1][key]), key


def test_float32_finalize_equals_the_float64_pass_on_near_ties():
    """The split-fp16 kernels hand on exact float32 sums (x - y)^2 of the original rows and the reported distance is their
    square root (no float64 finalize pass: csrc/streamed.hip, knn_finish).  That rests on every surviving list entry carrying an
    exact sum through the join passes (entries a pass keeps are copied by column id).  Lattice data -- thousands of exactly
    tied distances -- through two join passes: the default output against ANNCHOR_ST_FINALIZE_F64=1 (the float64 recomputation
    of the same lists): distances agree to float32 rounding (rtol 3e-7), rows are sorted, and where the two orders differ the
    distances at those positions tie within that rounding."""
    import subprocess
    import tempfile

    code = """
import sys, numpy as np
sys.path.insert(0, %r)
from annchor_amd.streamed import StreamedAnnchor
rng = np.random.default_rng(11)
out = []
for n, d, k, pw in ((60000, 24, 15, 0.12), (40000, 100, 10, 0.2)):
    X = rng.integers(0, 4, size=(n, d)).astype(np.float32)     # lattice: squared distances are small integers, ties everywhere
    X[:, :4] += (0.001 * rng.standard_normal((n, 4))).astype(np.float32)
    sa = StreamedAnnchor(X, n_anchors=16, n_neighbors=k, p_work=pw).fit()
    out.append((sa.neighbor_graph[0], sa.neighbor_graph[1], np.array(sa._engine.stream_last_kernel(with_guard=True))))
np.savez(sys.argv[1], **{"a%%d_%%d" %% (i, j): np.asarray(v) for i, o in enumerate(out) for j, v in enumerate(o)})
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))),)
    res = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, env in (("f32", {}), ("f64", {"ANNCHOR_ST_FINALIZE_F64": "1"})):
            out = os.path.join(tmp, name + ".npz")
            envd = dict(os.environ, **env)
            if not env:
                envd.pop("ANNCHOR_ST_FINALIZE_F64", None)
            r = subprocess.run([sys.executable, "-c", code, out], env=envd, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            res.append(dict(np.load(out)))
    for i in range(2):
        ia, da, ka = res[0]["a%d_0" % i], res[0]["a%d_1" % i], res[0]["a%d_2" % i]
        ib, db = res[1]["a%d_0" % i], res[1]["a%d_1" % i]
        assert ka[0] == 1, ka            # the split kernel ran (the float32 finalize is its path)
        np.testing.assert_allclose(da, db, rtol=3e-7, atol=1e-7)
        assert np.all(np.diff(da[:, 1:], axis=1) >= 0) and np.all(np.diff(db[:, 1:], axis=1) >= 0)
        for r_ in range(len(ia)):
            assert set(ia[r_]) == set(ib[r_]) or np.allclose(np.sort(da[r_]), np.sort(db[r_]), rtol=3e-7, atol=1e-7), r_
        diff = ia != ib
        if diff.any():
            np.testing.assert_allclose(da[diff], db[diff], rtol=3e-7, atol=1e-7)


def test_lds_level_sorts_equal_the_radix_sorts():
    """The deep levels of the k-d order (segments of <= 4096 rows) are sorted by one workgroup per segment in LDS, keyed by
    (distance to the split anchor, position): a stable order, i.e. the radix sort's -- the tile structure, hence the graph, is bit for
    bit the one of ANNCHOR_ST_ORDER_RADIX_ONLY=1 (every level through the radix passes), also with many equal keys (lattice data)."""
    import subprocess
    import tempfile

    code = """
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from test_streamed_gpu import latent
from annchor_amd.streamed import StreamedAnnchor
out = []
rng = np.random.default_rng(3)
for X, k, pw in ((latent(200000, 128), 15, 0.1), (latent(70001, 48), 10, 0.2), (rng.integers(0, 3, size=(50000, 20)).astype(np.float32), 8, 0.3)):
    sa = StreamedAnnchor(X, n_anchors=16, n_neighbors=k, p_work=pw).fit()
    out.append((sa.tile_evals, sa.neighbor_graph[0], sa.neighbor_graph[1]))
np.savez(sys.argv[1], **{"a%%d_%%d" %% (i, j): np.asarray(v) for i, o in enumerate(out) for j, v in enumerate(o)})
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    res = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, env in (("lds", {}), ("radix", {"ANNCHOR_ST_ORDER_RADIX_ONLY": "1"})):
            out = os.path.join(tmp, name + ".npz")
            envd = dict(os.environ, **env)
            if not env:
                envd.pop("ANNCHOR_ST_ORDER_RADIX_ONLY", None)
            r = subprocess.run([sys.executable, "-c", code, out], env=envd, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            res.append(dict(np.load(out)))
    assert res[0].keys() == res[1].keys()
    for key in res[0]:
        assert np.array_equal(res[0][key], res[1][key]), key
