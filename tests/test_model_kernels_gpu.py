"""The device model kernels on constructed inputs (tests/model_cases.py): k_ols_bins against an exact least-squares solve,
k_predict_merge / k_sample_predict_scatter against a NumPy restatement bit for bit, k_err_sort against np.sort -- partition by
partition, on the branches the bundled data reach only by luck: the minimum-norm branch (three rows, constant and collinear
columns, rank 1 and 0, a dependency the QR drops and the SVD keeps), the refusal of short partitions, empty and over-long
residual partitions, samples exactly on inner and outer edges, pairs outside every partition.

Measured on the MI355X (ratio = ||w_device - w_exact|| / (u kappa (1 + kappa rho) ||w_exact||), the bound allows GAMMA = 220;
printed by test_coefficients_against_the_exact_solution): see DESIGN.md section 3.7."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))

import model_cases as M  # noqa: E402

ONE_BIN = np.array([-np.inf, np.inf])
EXACT_CASES = M.FULL_RANK_CASES + M.DEFICIENT_CASES + ("refusals",)


class Fix:
    """One engine per fixture class, run up to get_features() on the complete pair list of model_cases.points(cls); the exact
    distance of every pair as the device computes it; the anchor state the anchor override reads."""

    def __init__(self, cls):
        from annchor_amd import Annchor, _native
        self.cls, self.nat = cls, _native
        ann = Annchor(np.array(M.points(cls)), "euclidean", n_anchors=5, n_neighbors=20, p_work=0.3, niters=1, random_seed=3)
        ann.get_anchors()
        ann.get_locality()
        ann.get_features()
        self.ann, self.eng = ann, ann._engine
        self.n = self.eng.field_size(_native.F_NCM)
        self.IJs = self.eng.download(_native.F_IJS).reshape(-1, 2)
        assert np.array_equal(self.IJs, M.pairs(cls))                      # the complete pair list, in the cases' order
        self.anc = self.eng.download(_native.F_FEATURES).reshape(-1, 4)[:, 3].copy()
        self.A = self.eng.download(_native.F_A)
        self.D = self.eng.download(_native.F_D).reshape(M.CLASSES[cls], -1)
        assert self.D.shape[1] == len(self.A)
        assert np.array_equal(self.anc != 0, np.isin(self.IJs, self.A).any(axis=1)) and self.anc.any() and not self.anc.all()
        self.Y = self.eng.evaluate_samples(np.arange(self.n, dtype=np.int64))
        self.staged = None
        self.cases = {}

    def case(self, name):
        if name not in self.cases:
            c = M.build(name, self.Y)
            c.features[:, 3] = self.anc
            self.cases[name] = c
        return self.cases[name]

    def stage(self, name):
        """The case's features on the device and its sample request the device-resident sample, in request order: with every
        pair not computed and one partition over everything, the rank of a pair is its position."""
        c = self.case(name)
        if self.staged != name:
            self.staged = None
            self.eng.upload(self.nat.F_FEATURES, c.features)
            self.eng.upload(self.nat.F_NCM, np.ones(self.n, dtype=np.uint8))
            m = self.eng.sample_pairs_device(ONE_BIN, [self.n], np.zeros(c.m, dtype=np.int32), c.pos)
            assert m == c.m
            self.staged = name
        return c

    def state(self, c):
        """A RefineApprox / not-computed state for the runs that are not a first iteration: every RA value distinct and
        negative (a pair the pass must not write keeps it), 60 % of the pairs not computed, samples on both sides."""
        rng = np.random.default_rng(c.m)
        return -(1.0 + np.arange(self.n, dtype=np.float64)), (rng.random(self.n) < 0.6).astype(np.uint8)

    def fit(self, name, first=1, is_metric=1):
        c = self.stage(name)
        eng, nat = self.eng, self.nat
        RA0 = ncm = None
        if not first:
            RA0, ncm = self.state(c)
            eng.upload(nat.F_RA, RA0)
            eng.upload(nat.F_NCM, ncm)
        eng.fit_regression_device(c.edges, first, is_metric)
        eng.fit_errors_device()
        W, cc, status, ep, flags, errs = eng.model_download_with_errors(c.nb, 2 * c.m)
        W2, cc2, status2, ep2, flags2 = eng.model_download(c.nb)
        pos, feats, y, spred = eng.download_samples(c.m)
        return dict(W=W, c=cc, status=status, err_ptr=ep, flags=flags, errs=errs, again=(W2, cc2, status2, ep2, flags2),
                    pos=pos, feats=feats, y=y, spred=spred, RA=eng.download(nat.F_RA), labels=eng.download(nat.F_LABELS),
                    RA0=RA0, ncm=ncm)


_FIX, _RUNS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    for F in _FIX.values():
        F.eng.close()
    _FIX.clear()
    _RUNS.clear()


def fix(name):
    cls = M.case_class(name)
    if cls not in _FIX:
        _FIX[cls] = Fix(cls)
    return _FIX[cls]


def run(name):
    """The case's first-iteration, is_metric run; computed once, left unchanged."""
    if name not in _RUNS:
        _RUNS[name] = fix(name).fit(name)
    return _RUNS[name]


def parts(c, r):
    X = r["feats"][:, :3]
    return X, r["y"], M.reg_bin(X[:, 2], c.edges)


# ------------------------------------------------------------------------------------------------------------ samples, statuses
@pytest.mark.parametrize("name", M.ALL_CASES)
def test_samples_statuses_and_flags(name):
    F = fix(name)
    c, r = F.case(name), run(name)
    assert np.array_equal(r["pos"], c.pos)                                   # the request, in request order
    assert np.array_equal(r["feats"], c.features[c.pos])                     # bit for bit, anchor column included
    assert np.array_equal(r["y"], F.Y[c.pos])                                # evaluate_samples' distances
    assert list(r["status"]) == list(c.status)
    assert tuple(r["flags"]) == c.flags
    W2, cc2, status2, ep2, flags2 = r["again"]
    assert not flags2.any()                                                  # cleared by the first download
    assert np.array_equal(W2, r["W"]) and np.array_equal(cc2, r["c"]) and np.array_equal(ep2, r["err_ptr"])
    for b in range(c.nb):
        if c.status[b] == 2:
            assert not r["W"][b].any() and r["c"][b] == 0.0


# ------------------------------------------------------------------------------------------------------------ coefficients
@pytest.mark.parametrize("name", EXACT_CASES)
def test_coefficients_against_the_exact_solution(name):
    F = fix(name)
    c, r = F.case(name), run(name)
    X, y, part = parts(c, r)
    worst = 0.0
    for b in range(c.nb):
        if c.rank[b] is None or c.rows[b] > M.EXACT_MAX_ROWS:
            continue
        idx = part == b
        assert idx.sum() == c.rows[b] and r["status"][b] == 0
        rank = c.ref_rank.get(b, c.rank[b])
        R = M.reference(X[idx], y[idx], rank)
        w, cc = r["W"][b], r["c"][b]
        assert np.isfinite(w).all() and np.isfinite(cc)
        if rank == 3:
            err = float(np.linalg.norm(w - R.w))
            ratio = err / (M.U * R.unit * np.linalg.norm(R.w))
            worst = max(worst, ratio)
            print("  %s[%d]: rows %d kappa %.3g rho %.3g  ||dw|| %.3g = %.3f u kappa (1 + kappa rho) ||w||;  dc %.3g (bound %.3g)"
                  % (name, b, idx.sum(), R.kappa, R.rho, err, ratio, abs(cc - R.c), R.tol_c()))
            assert err <= R.tol_w(), (name, b, ratio)
            assert abs(cc - R.c) <= R.tol_c(), (name, b, cc - R.c, R.tol_c())
        else:
            rel = M.GAMMA * M.U * R.unit
            if rank == 0:
                assert not w.any() and abs(cc - R.c) <= 4 * M.U * abs(R.mean_y)
            for v in c.null[b]:
                print("  %s[%d]: rank %d  |w.v| / (||w|| ||v||) = %.3g (bound %.3g)"
                      % (name, b, rank, abs(w @ v) / max(np.linalg.norm(w) * np.linalg.norm(v), 1e-300), rel))
                assert abs(w @ v) <= rel * np.linalg.norm(w) * np.linalg.norm(v), (name, b, v)
            dp = np.abs(r["spred"][idx] - R.pred)
            tol = R.tol_pred(X[idx], w)
            print("  %s[%d]: rank %d  prediction error / bound, largest: %.3g" % (name, b, rank, (dp / tol).max()))
            assert np.all(dp <= tol), (name, b, (dp / tol).max())
    print("  %s: largest coefficient ratio %.3f (GAMMA = %g)" % (name, worst, M.GAMMA))


# ------------------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("name", ("full_n300", "shuffled", "ub_2dad", "n3", "near_dep_1e-11", "nb64", "inner_edge", "sort_8192"))
def test_two_fits_of_one_sample_give_the_same_bits(name):
    F = fix(name)
    a, b = F.fit(name), F.fit(name)
    for k in ("W", "c", "spred", "errs", "err_ptr", "status", "RA", "labels"):
        assert np.array_equal(a[k].view(np.int64) if a[k].dtype == np.float64 else a[k],
                              b[k].view(np.int64) if b[k].dtype == np.float64 else b[k]), k


# ------------------------------------------------------------------------------------------------------------ prediction pass
@pytest.mark.parametrize("is_metric", (1, 0))
@pytest.mark.parametrize("first", (1, 0))
@pytest.mark.parametrize("name", M.ALL_CASES)
def test_prediction_pass_bit_for_bit(name, first, is_metric):
    F = fix(name)
    c = F.case(name)
    r = F.fit(name, first, is_metric)
    RA, labels, spred = M.prediction_pass(c.features, c.edges, r["W"], r["c"], c.pos, F.Y[c.pos], first, is_metric,
                                          RA0=r["RA0"], ncm=r["ncm"], IJs=F.IJs, A=F.A, D=F.D)
    assert np.array_equal(r["spred"], spred)
    assert np.array_equal(r["labels"], labels)
    assert np.array_equal(r["RA"], RA)
    assert np.array_equal(r["RA"][c.pos], F.Y[c.pos])
    if not first:
        keep = (r["ncm"] == 0)
        keep[c.pos] = False
        assert keep.any() and np.array_equal(r["RA"][keep], r["RA0"][keep])
    if not is_metric:
        assert (RA[F.anc != 0] != np.clip(M.predict(c.features, c.edges, r["W"], r["c"]), c.features[:, 0], c.features[:, 1])[F.anc != 0]).any()
    # annchor_predict_merge, handed the same coefficients by the host, is the same pass
    if not first:
        F.eng.upload(F.nat.F_RA, r["RA0"])
    sp = F.eng.predict_merge(c.edges, r["W"], r["c"], first, is_metric, c.m)
    assert np.array_equal(sp, spred)
    assert np.array_equal(F.eng.download(F.nat.F_RA), RA) and np.array_equal(F.eng.download(F.nat.F_LABELS), labels)


# ------------------------------------------------------------------------------------------------------------ residual lists
@pytest.mark.parametrize("name", M.ALL_CASES)
def test_residual_lists(name):
    F = fix(name)
    c, r = F.case(name), run(name)
    ptr, lists = M.residual_lists(r["feats"][:, 2], r["y"], r["spred"], c.edges)
    assert [len(v) for v in lists] == list(c.err_rows)
    assert np.array_equal(r["err_ptr"], ptr)
    assert r["errs"] is not None and len(r["errs"]) == ptr[-1]
    checked = 0
    for b, want in enumerate(lists):
        if len(want) > M.ERR_CAP:
            continue                                  # flags[2] == 2 (test_samples_statuses_and_flags): no list
        got = r["errs"][ptr[b]:ptr[b + 1]]
        assert np.array_equal(got, want), (name, b)
        checked += 1
    assert checked >= c.nb - 1
    if name in ("lowest_edge", "sort_ties"):
        assert (lists[0] == 0.0).any()                # the pair of distance 0 on the lowest edge: a zero residual in the list
    if name == "sort_ties":
        _, cnt = np.unique(lists[0], return_counts=True)
        assert cnt.max() >= 30


# ------------------------------------------------------------------------------------------------------------ stale sample features
def test_a_host_bound_sample_has_no_device_resident_features():
    """set_samples / sample_pairs / hash_sample_pairs / evaluate_samples replace the sample but hand its feature rows to the host:
    fit_regression_device must refuse (it used to read the rows an earlier device-resident sample left), and a fresh
    sample_pairs_device makes it work again."""
    name = "full_n300"
    F = fix(name)
    c, r = F.case(name), run(name)
    eng, nat = F.eng, F.nat
    few = c.pos[:5]
    steps = (lambda: eng.set_samples(few, F.Y[few]),
             lambda: eng.evaluate_samples(few),
             lambda: (eng.upload(nat.F_NCM, np.ones(F.n, dtype=np.uint8)), eng.sample_pairs(ONE_BIN, [F.n], np.zeros(5, dtype=np.int32), few)),
             lambda: (eng.upload(nat.F_NCM, np.ones(F.n, dtype=np.uint8)), eng.hash_sample_pairs(ONE_BIN, eng.bin_counts(ONE_BIN), [5], 12345)))
    for step in steps:
        F.stage(name)
        eng.fit_regression_device(c.edges, 1, 1)
        F.staged = None
        step()
        with pytest.raises(nat.NativeError, match="device-resident"):
            eng.fit_regression_device(c.edges, 1, 1)
        with pytest.raises(nat.NativeError):
            eng.fit_errors_device()
        with pytest.raises(nat.NativeError):
            eng.download_samples(5, predict=False)
    again = F.fit(name)
    assert np.array_equal(again["W"], r["W"]) and np.array_equal(again["c"], r["c"]) and np.array_equal(again["errs"], r["errs"])
