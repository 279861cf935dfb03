"""The host side of DBSCAN (tests/dbscan_cases.py, annchor_amd/radius.py) -- no GPU.

1. the reference equals sklearn.cluster.DBSCAN(metric="precomputed") on 200 seeded random planar integer point sets;
2. the reference is a function of the edge SET: order and orientation of the edges do not change it;
3. the case table holds what the kernel tests claim to cover;
4. DBSCANResult's accessors, the argument checks, and radius.cluster's host-metric route on a host stand-in for the engine."""
import numpy as np
import pytest

import dbscan_cases as DC


def _planar(seed):
    """A random planar integer point set, its distance matrix, and DBSCAN parameters drawn with it."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(5, 70))
    P = rng.integers(0, int(rng.integers(4, 14)), (n, 2)).astype(np.float64)
    D = np.sqrt(((P[:, None, :] - P[None, :, :]) ** 2).sum(axis=2))
    eps = float(rng.choice([0.5, 1.0, 1.5, 2.0, 2.5, 3.0]))   # (0.5: duplicates only; sklearn takes no eps = 0)
    return D, eps, int(rng.integers(1, 8))


def test_reference_equals_sklearn():
    sk = pytest.importorskip("sklearn.cluster")
    border = clusters = 0
    for seed in range(200):
        D, eps, ms = _planar(seed)
        n = len(D)
        i, j = np.nonzero(np.triu(D <= eps, k=1))
        labels, core, ncl = DC.reference(n, np.stack([i, j], axis=1), ms)
        want = sk.DBSCAN(eps=eps, min_samples=ms, metric="precomputed").fit(D)
        assert np.array_equal(labels, want.labels_), seed
        assert np.array_equal(np.flatnonzero(core), want.core_sample_indices_), seed
        assert ncl == (labels.max() + 1 if n else 0), seed
        border += int(((labels >= 0) & ~core).sum())
        clusters += ncl
    assert border > 200 and clusters > 400, (border, clusters)   # (the comparison saw border points and many clusters)


@pytest.mark.parametrize("name", ["bridge", "three_clusters", "star_ms301", "random_ms20", "path_perm_shuffled"])
def test_reference_is_invariant_under_edge_order(name):
    c = DC.CASES[name]
    want = DC.REFERENCE[name]
    rng = np.random.default_rng(3)
    for k in range(3):
        e = c["edges"][rng.permutation(len(c["edges"]))].copy()
        flip = rng.random(len(e)) < 0.5
        e[flip] = e[flip, ::-1]
        labels, core, ncl = DC.reference(c["nx"], e, c["min_samples"])
        assert np.array_equal(labels, want[0]) and np.array_equal(core, want[1]) and ncl == want[2]


def test_the_case_table_holds_what_it_claims():
    assert all(DC.CONDITIONS.values()), DC.CONDITIONS
    for nx in (1, 2, 63, 64, 65, 257):
        assert DC.CASES["empty%d_ms1" % nx]["nx"] == nx and len(DC.CASES["empty%d_ms1" % nx]["edges"]) == 0
        assert DC.CENSUS["empty%d_ms1" % nx]["clusters"] == nx and DC.CENSUS["empty%d_ms2" % nx]["noise"] == nx
    for num in ("id", "rev", "perm"):
        for order in ("asc", "desc", "shuffled"):
            s = DC.CENSUS["path_%s_%s" % (num, order)]
            assert (s["clusters"], s["border"], s["noise"]) == (1, 2, 0)
    assert DC.CENSUS["star_ms2"]["clusters"] == 1 and DC.CENSUS["star_ms302"]["noise"] == 301 and DC.CENSUS["star_ms301"]["border"] == 300
    for name in ("bridge", "bridge_high_first"):
        assert DC.CENSUS[name]["clusters"] == 2 and DC.REFERENCE[name][0][0] == 0 and not DC.REFERENCE[name][1][0]
    assert DC.CENSUS["three_clusters"]["clusters"] == 3 and DC.REFERENCE["three_clusters"][0][15] == 0
    assert DC.CENSUS["ms1"]["noise"] == 0 and DC.REFERENCE["ms1"][1].all() and DC.CENSUS["ms1"]["clusters"] > 1
    assert DC.CENSUS["ms_above_all"]["noise"] == 100 and DC.CENSUS["complete65"]["clusters"] == 1
    assert DC.CENSUS["random_ms30"]["clusters"] > 1 and DC.CENSUS["random_ms20"]["border"] > 0
    b = DC.batches("random_ms10_batches")
    assert len(b) == 7 and any(len(x) == 0 for x in b) and len(set(len(x) for x in b)) == 7
    assert np.array_equal(np.concatenate(b), DC.CASES["random_ms10"]["edges"])
    # groups are one graph: the same edge set
    groups = {}
    for name, c in DC.CASES.items():
        if c["group"]:
            key = set(map(tuple, np.sort(c["edges"], axis=1).tolist()))
            assert groups.setdefault(c["group"], key) == key, name


def test_the_injected_table_leaves_no_candidate():
    import radius_cases as C

    D, r = DC.sure_or_out_table()
    L = C.lists(C.classify(D, r, 0.0, True))
    assert len(L["eval"]) == 0 and len(L["sure"]) > 1000 and L["pruned"] > 0
    s = DC.census(len(D), L["sure"], 6)
    assert s["clusters"] >= 2 and s["noise"] > 0


def test_result_accessors():
    from annchor_amd import DBSCANResult

    labels = np.array([0, -1, 1, 0, -1, 1], dtype=np.int64)
    core = np.array([True, False, True, False, False, True])
    res = DBSCANResult(labels, core, 2, 1.5, 3)
    assert res.nx == 6 and res.n_clusters == 2 and res.n_noise == 2 and res.eps == 1.5 and res.min_samples == 3
    assert res.core_sample_indices.dtype == np.int64 and res.core_sample_indices.tolist() == [0, 2, 5]
    assert res.labels is labels and res.core_sample_mask is core


def test_argument_checks():
    from annchor_amd import radius

    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="eps must be a number >= 0"):
            radius.check_radius(bad, "dbscan", "eps")
    assert radius.check_radius(0, "dbscan", "eps") == 0.0
    for bad in (0, -3, 2.5, 3.0, "4", None, True):
        with pytest.raises(ValueError, match="min_samples must be an integer >= 1"):
            radius.check_min_samples(bad)
    assert radius.check_min_samples(np.int64(4)) == 4 and radius.check_min_samples(1) == 1
    with pytest.raises(ValueError, match="below 2\\^31"):
        radius.check_min_samples(1 << 31)
    with pytest.raises(ValueError, match="dbscan: max_chunk_pairs must be >= 1"):
        radius.cluster(_HostEngine(4), 4, 1.0, 2, 0.0, False, 0, host_eval=lambda IJ: np.zeros(len(IJ)))


class _HostEngine:
    """What radius.cluster asks of an engine on the host-metric route without bounds: every pair i < j is a candidate, the
    lists are row-major, a range above the cap emits nothing; the DBSCAN calls collect the edges for the reference."""

    def __init__(self, nx):
        self.nx, self.calls, self.cand = nx, 0, None

    def radius_count(self, r, rtol, conn, use_bounds):
        assert conn and not use_bounds
        return np.arange(self.nx - 1, -1, -1, dtype=np.int64), np.zeros(self.nx, dtype=np.int64)

    def radius_rows(self, rb, re, cb, ce, cap, evaluate):
        assert not evaluate
        ij = [(i, j) for i in range(rb, re) for j in range(max(i + 1, cb), ce)]
        if cap > 0 and len(ij) > cap:
            return len(ij), 0, -1
        self.calls += 1
        self.cand = np.array(ij, dtype=np.int64).reshape(-1, 2)
        return len(ij), 0, 0

    def radius_fetch(self, which, n):
        assert which == 0 and n == len(self.cand)
        return self.cand

    def dbscan_begin(self, min_samples):
        self.ms, self.edges = min_samples, []

    def dbscan_edges(self, ij):
        self.edges.append(np.asarray(ij))

    def dbscan_finish(self):
        e = np.concatenate(self.edges) if self.edges else np.zeros((0, 2), dtype=np.int64)
        labels, core, ncl = DC.reference(self.nx, e, self.ms)
        return labels.astype(np.int32), core.astype(np.uint8), ncl


def test_cluster_driver_on_the_host_route():
    from annchor_amd import radius

    D, eps, ms = _planar(7)
    n = len(D)
    i, j = np.nonzero(np.triu(D <= eps, k=1))
    want = DC.reference(n, np.stack([i, j], axis=1), ms)
    for cap in (None, 9):
        eng = _HostEngine(n)
        res, st = radius.cluster(eng, n, eps, ms, 0.0, False, cap, host_eval=lambda IJ: D[IJ[:, 0], IJ[:, 1]])
        assert res.labels.dtype == np.int64 and res.core_sample_mask.dtype == bool
        assert np.array_equal(res.labels, want[0]) and np.array_equal(res.core_sample_mask, want[1]) and res.n_clusters == want[2]
        assert (res.eps, res.min_samples) == (eps, ms)
        assert st["pairs"] == st["evals"] == n * (n - 1) // 2 and st["edges"] == len(i) and st["chunks"] == eng.calls
        assert cap is None or eng.calls > 10
