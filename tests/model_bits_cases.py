"""Inputs and driver of the bit-for-bit check of the device model kernels (csrc/model.hip: k_ols_bins, k_err_sort) against a
recorded build: tests/golden/model_bits.npz holds what one build gave on these cases (make_model_bits.py writes it),
test_model_kernels_bits_gpu.py asserts that the build under test gives the same bits.

The cases sit where a change of the kernels' layout can go wrong without changing their arithmetic: partition row counts
round the wave, the workgroup and the LDS capacity of the work matrix (OLS_LDS_ROWS), sample counts round the compaction trips
(OLS_TRIP samples of k_ols_bins, ERR_TRIP of k_err_sort), members placed in chosen lanes and trips, residual lists round the
sorter's sizes.  All on the 701-point fixture of model_cases.py (lattice points: the targets are exact); the features are
multiples of 1/2 ("half") or generic floats ("float").  Which pairs a case samples and every feature depend on the seed and
the points alone, never on a device result."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))

import model_cases as M  # noqa: E402

CLS = "mid"
OLS_TRIP = 2048           # model.hip: samples k_ols_bins compacts per trip
OLS_LDS_ROWS = 4096       # model.hip: partitions up to this many rows are factored in LDS
ERR_TRIP = 8192           # model.hip: samples k_err_sort takes per trip
N_FILL = 40
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "model_bits.npz")

ROW_COUNTS = (3, 4, 63, 64, 65, 255, 256, 257, 513, 1023, 1024, 1025, OLS_LDS_ROWS - 1, OLS_LDS_ROWS, OLS_LDS_ROWS + 1, 6000,
              M.ERR_CAP, M.ERR_CAP + 1)
SAMPLE_COUNTS = (OLS_TRIP - 1, OLS_TRIP, OLS_TRIP + 1, 2 * OLS_TRIP + 1, ERR_TRIP - 1, ERR_TRIP, ERR_TRIP + 1, 2 * ERR_TRIP + 1)
CASES = (tuple("rows_%d" % n for n in ROW_COUNTS) + tuple("m_%d" % m for m in SAMPLE_COUNTS)
         + ("c2_shape", "first_wave", "last_lane", "empty_trip", "last_sample", "err_empty_trip", "nb1", "nb64", "short_partitions",
            "ub_2dad", "inner_edge", "ties_one_value", "ties_two_values", "zeros"))


def _edges(nb, finite=False):
    """partition q is (10 q, 10 (q + 1)]; the outer edges are infinite unless `finite`."""
    e = 10.0 * np.arange(nb + 1)
    if not finite:
        e[0], e[-1] = -np.inf, np.inf
    return e


def _rows(y, part, rng, half):
    """feature rows [lb, ub, dad] of samples with targets y in partitions part (dad strictly inside the partition)."""
    X = M._generic(y, rng, 0.0, 1.0)
    X[:, 2] = 10.0 * part + 1.0 + 8.0 * X[:, 2]
    if half:
        X = np.round(2.0 * X) / 2.0
    return X


def build(name):
    """(features float64 [n][4] of every pair, sample positions int64 [m] ascending, edges float64 [nb + 1])."""
    Y = M.host_distances(CLS)
    rng = np.random.default_rng(9000 + CASES.index(name))
    n_pairs = len(Y)
    line, zero, rest = M._pair_sets(CLS)
    half, finite, fix = True, False, None

    if name.startswith("rows_"):
        n = int(name.split("_")[1])
        m, nb = n + N_FILL, 2
        part = np.ones(m, dtype=np.int64)
        part[rng.permutation(m)[:n]] = 0
        half = n % 2 == 1
    elif name.startswith("m_"):
        m, nb = int(name.split("_")[1]), 3
        part = rng.integers(0, nb, m)
        half = False
    elif name == "c2_shape":
        m, nb = 5000, 7
        part = rng.integers(0, nb, m)
        half = False
    elif name in ("first_wave", "last_lane", "empty_trip", "last_sample"):
        m, nb = 3 * OLS_TRIP, 2
        t = np.arange(m)
        if name == "first_wave":        # partition 0: the first wave's lanes of the first sub-trip of every trip
            part = np.where(t % OLS_TRIP < 64, 0, 1)
        elif name == "last_lane":       # partition 0: the last lane of every wave
            part = np.where(t % 64 == 63, 0, 1)
        elif name == "empty_trip":      # partition 0: nobody in the second trip
            part = np.where((rng.random(m) < 0.3) & (t // OLS_TRIP != 1), 0, 1)
        else:                           # partition 0: a few members, the very last sample among them; m one past a trip
            m = 2 * OLS_TRIP + 1
            part = np.where(rng.random(m) < 0.01, 0, 1)
            part[-1] = 0
    elif name == "err_empty_trip":      # three trips of k_err_sort, partition 0 absent from the second
        m, nb = 3 * ERR_TRIP, 2
        t = np.arange(m)
        part = np.where((rng.random(m) < 0.2) & (t // ERR_TRIP != 1), 0, 1)
        half = False
    elif name == "nb1":
        m, nb = 300, 1
        part = np.zeros(m, dtype=np.int64)
    elif name == "nb64":
        m, nb = 64 * 20, 64
        part = np.arange(m) % 64
    elif name == "short_partitions":    # partitions of 5, 0, 1, 2 and 8 rows
        m, nb = 16, 5
        part = rng.permutation(np.repeat([0, 2, 3, 4], [5, 1, 2, 8]))
    elif name == "ub_2dad":             # partition 0 rank deficient: ub = 2 dad bit for bit
        m, nb = 240, 2
        part = (np.arange(m) >= 200).astype(np.int64)
        fix = "ub_2dad"
    elif name == "inner_edge":          # three samples exactly on the inner edge: both residual lists, err_ptr[nb] = m + 3
        m, nb = 120, 2
        part = (np.arange(m) % 2).astype(np.int64)
        fix = "inner_edge"
    elif name in ("ties_one_value", "ties_two_values"):
        # finite outer edges, every member of the first list exactly on the lowest edge: no regression partition, prediction 0,
        # residual = the pair's distance -- pairs of distance 5 (and 10)
        m, nb, finite = 760, 2, True
        part = np.ones(m, dtype=np.int64)
        fix = name
    elif name == "zeros":               # partition 0: constant features and a constant target -- w = 0, c = y, residuals +0.0
        m, nb = 104, 2
        part = (np.arange(m) >= 64).astype(np.int64)
        fix = "zeros"
    else:
        raise KeyError(name)

    edges = _edges(nb, finite)
    if fix in ("ties_one_value", "ties_two_values", "zeros"):
        k = 700 if fix != "zeros" else 64
        five, ten = np.flatnonzero(Y == 5.0), np.flatnonzero(Y == 10.0)
        tied = rng.permutation(five)[:k] if fix != "ties_two_values" else np.concatenate([rng.permutation(five)[:k // 2],
                                                                                          rng.permutation(ten)[:k - k // 2]])
        assert len(tied) == k
        pos = np.concatenate([tied, rng.permutation(np.setdiff1d(rest, tied))[:m - k]])
    else:
        pos = rng.permutation(rest)[:m]
    order = np.argsort(pos, kind="stable")
    if fix in ("ties_one_value", "ties_two_values", "zeros"):
        part = np.r_[np.zeros(k, dtype=np.int64), np.ones(m - k, dtype=np.int64)]
        part_sorted = part[order]
    else:
        part_sorted = part                       # the placement is by sample order: assign after the sort
    pos = pos[order]
    X = _rows(Y[pos], part_sorted, rng, half)
    if fix == "ub_2dad":
        X[part_sorted == 0, 1] = 2.0 * X[part_sorted == 0, 2]
    elif fix == "inner_edge":
        X[[7, 40, 119], 2] = 10.0
    elif fix in ("ties_one_value", "ties_two_values"):
        X[part_sorted == 0, 2] = 0.0             # ON the lowest edge
    elif fix == "zeros":
        X[part_sorted == 0] = [1.25, 7.5, 4.0]
    F = M._background(CLS, rng, edges, Y)
    F[pos, :3] = X
    return F, pos.astype(np.int64), edges


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8).copy()


class Driver:
    """One engine on the fixture's complete pair list, run up to get_features(); run(name) stages a case the way
    test_model_kernels_gpu.py does and returns what is recorded of it."""

    def __init__(self):
        from annchor_amd import Annchor, _native
        self.nat = _native
        ann = Annchor(np.array(M.points(CLS)), "euclidean", n_anchors=5, n_neighbors=20, p_work=0.3, niters=1, random_seed=3)
        ann.get_anchors()
        ann.get_locality()
        ann.get_features()
        self.ann, self.eng = ann, ann._engine
        self.n = self.eng.field_size(_native.F_NCM)
        assert np.array_equal(self.eng.download(_native.F_IJS).reshape(-1, 2), M.pairs(CLS))
        self.anc = self.eng.download(_native.F_FEATURES).reshape(-1, 4)[:, 3].copy()

    def close(self):
        self.eng.close()

    def run(self, name):
        F, pos, edges = build(name)
        F[:, 3] = self.anc
        eng, nat = self.eng, self.nat
        nb, m = len(edges) - 1, len(pos)
        eng.upload(nat.F_FEATURES, F)
        eng.upload(nat.F_NCM, np.ones(self.n, dtype=np.uint8))
        assert eng.sample_pairs_device(np.array([-np.inf, np.inf]), [self.n], np.zeros(m, dtype=np.int32), pos) == m
        eng.fit_regression_device(edges, 1, 1)
        eng.fit_errors_device()
        W, c, status, ep, flags, errs = eng.model_download_with_errors(nb, 2 * m)
        _, _, _, spred = eng.download_samples(m)
        rows = np.diff(ep)            # DeviceModel.rows after the residual step: the lists' lengths (the C ABI hands out no more)
        # a list longer than the sorter takes is refused (flags[2] = 2) and its stretch of errs is left as it was: not recorded
        kept = np.concatenate([errs[ep[b]:ep[b + 1]] for b in range(nb) if rows[b] <= M.ERR_CAP] + [np.zeros(0)])
        return {"W": W.view(np.int64).copy(), "c": c.view(np.int64).copy(), "status": status.astype(np.int64), "rows": rows.astype(np.int64),
                "err_ptr": ep.astype(np.int64), "flags": flags.astype(np.int64), "spred": sha(spred), "errs": sha(kept),
                "RA": sha(eng.download(nat.F_RA)), "labels": sha(eng.download(nat.F_LABELS)),
                # not compared, for the reader of the fixture: the sizes of the case
                "shape": np.array([m, nb, int(rows.max())], dtype=np.int64)}


COMPARED = ("W", "c", "status", "rows", "err_ptr", "flags", "spred", "errs", "RA", "labels")
