"""The workgroup-per-row selections (csrc/rowsel.h: k_row_thresh, k_gn_lists, k_get_nn, k_bf_rows) and the global candidate
cut on injected, adversarial state, stage by stage against the oracle's NumPy restatements.  tests/row_paths_cases.py builds the
rows and tests/test_row_paths_cases.py asserts (without a GPU) which branch each of them takes: sampled threshold too wide, too
tight, second cut too tight, fast path.  Selection is exact and a probability is one correctly rounded division on both
sides: every comparison is np.array_equal, there are no tolerances."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import row_paths_cases as C
import row_paths_worker as W
from oracle import annchor_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLS = list(C.CLASSES)
ERRS3 = [np.array([0.25]), np.sort(np.random.default_rng(1).standard_normal(7)) * 3.0,
         np.sort(np.random.default_rng(2).standard_normal(4000)) * 4.0]      # lists of 1, 7 and 4000 residuals


@pytest.fixture(scope="module")
def fixtures():
    made = {}

    def get(cls):
        if cls not in made:
            made[cls] = W.Fixture(cls)
        return made[cls]
    yield get
    for F in made.values():
        F.close()


def _labels3(F):
    return np.random.default_rng(F.nx).integers(0, 3, F.n).astype(np.int64)


@pytest.mark.parametrize("case", C.CASES)
@pytest.mark.parametrize("cls", CLS)
def test_row_thresholds(fixtures, cls, case):
    """k_row_thresh against np.partition; n_neighbors = len + 5 exercises the clamp to the row's last entry."""
    F = fixtures(cls)
    RA, ncm = F.case(case, W.N_NEIGHBORS + 1)
    assert W.thresholds(F, RA, ncm, (1, W.N_NEIGHBORS, F.len - 1, F.len + 5)) == 0


@pytest.mark.parametrize("sweep", ["rounds", "sequential"])
@pytest.mark.parametrize("case", C.CASES)
@pytest.mark.parametrize("cls", CLS)
def test_guarantee_nmin(fixtures, cls, case, sweep, monkeypatch):
    """k_gn_lists + the sweep (both ANNCHOR_GN_SWEEP forms) against the reference's sequential walk, on every mask; then the
    thresholds and the probabilities (three labels, lists of 1, 7 and 4000 residuals) on the marked state."""
    F = fixtures(cls)
    monkeypatch.setenv("ANNCHOR_GN_SWEEP", sweep)
    labels = _labels3(F)
    for mask in C.MASKS:
        RA, ncm = F.case(case, W.NMIN + 1, mask)
        assert W.guarantee_nmin(F, RA, ncm, errs=ERRS3, labels=labels) == (0, 0, 0), mask


@pytest.mark.parametrize("case", C.CASES)
@pytest.mark.parametrize("cls", CLS)
def test_final_graph(fixtures, cls, case):
    """k_get_nn against get_nn (not-computed entries keyed RA + row maximum, ties in slot order): rows with fewer than nn - 1
    computed entries and rows with none (row_counts mask), every entry not computed, 30 % computed."""
    F = fixtures(cls)
    for mask in C.MASKS:
        RA, ncm = F.case(case, W.NN - 1, mask)
        assert W.graph(F, RA, ncm, (2, W.NN, 64)) == 0, mask


@pytest.mark.parametrize("cls", CLS)
def test_graph_after_guarantee_nmin_marks(fixtures, cls):
    """The graph on a state that really carries guarantee_nmin's -1 marks on not-computed entries (the `risky` rows of k_get_nn)."""
    F = fixtures(cls)
    RA, ncm = F.case("integer_halves", W.NN - 1, "row_counts")
    marked = O.guarantee_nmin(RA.copy(), ncm.astype(bool), F.ptr, F.idx, W.NMIN)
    assert (marked == -1.0).any()
    assert W.graph(F, marked, ncm, (W.NN,)) == 0


def test_lds_copy_toggled_in_process(fixtures, monkeypatch):
    """ANNCHOR_ROW_LDS_COPY is read per call: the fallback rows with and without their LDS copy."""
    for cls in CLS:
        F = fixtures(cls)
        for keep in ("1", "0"):
            monkeypatch.setenv("ANNCHOR_ROW_LDS_COPY", keep)
            for case in ("sample_sees_large", "sample_sees_small", "shrink_too_tight", "all_equal"):
                RA, ncm = F.case(case, W.N_NEIGHBORS + 1, "random70")
                assert W.thresholds(F, RA, ncm, (W.N_NEIGHBORS,)) == 0
                assert W.guarantee_nmin(F, RA, ncm) == (0, 0, 0)
                assert W.graph(F, RA, ncm, (W.NN,)) == 0


# ----------------------------------------------------------------------------------------- probabilities and the global cut
def _prob_layout(F, kind, rng):
    """(RA, ncm, labels, errs): probabilities with the wanted tie structure, through the residual lists."""
    RA, ncm = F.case("integer_halves" if kind != "one_value" else "all_equal", W.N_NEIGHBORS + 1, "random70")
    labels = np.zeros(F.n, dtype=np.int64)
    if kind == "one_value":
        RA = np.full(F.n, 2.5)                      # every threshold 2.5, p = 0 everywhere: prob = 1 / 2 for every pair
        return RA, ncm, labels, [np.array([-1.0, 1.0])]
    thr = O.row_kth(RA, F.ptr, F.idx, W.N_NEIGHBORS)
    p = np.maximum(thr[F.IJs[:, 0]] - RA, thr[F.IJs[:, 1]] - RA)[ncm.astype(bool)]
    if kind == "third_zero":                        # p <= errs[0] on a third of the pairs
        return RA, ncm, labels, [np.sort(rng.choice(p[p >= np.quantile(p, 1 / 3)], 7, replace=False))]
    if kind == "two_values":                        # one residual: prob is 0 or 1
        return RA, ncm, labels, [np.array([np.median(p)])]
    RA = RA + rng.random(F.n) * 0.5                 # continuous: distinct p, three labels, lists of 1, 7 and 4000
    return RA, ncm, _labels3(F), ERRS3


@pytest.mark.parametrize("kind", ["one_value", "third_zero", "two_values", "continuous"])
def test_probabilities_and_candidate_cut(fixtures, kind, monkeypatch):
    """F_PROB against refine_probabilities, F_CAND / F_NEXT against select_candidates (prob descending, scrambled position,
    position): n_refine = 1, the first / middle / last member of a tie group, n_refine * lookahead just below and above the
    number of not-computed pairs, n_refine beyond it; the short-list tie route and ANNCHOR_TIE_CAP's general selection, the
    device-side cut values and ANNCHOR_CUT_FORCE_REDO's waiting repeat."""
    F = fixtures("mid")
    rng = np.random.default_rng(7)
    RA, ncm, labels, errs = _prob_layout(F, kind, rng)
    u = ncm.astype(bool)
    unc = np.flatnonzero(u)
    thr = O.row_kth(RA, F.ptr, F.idx, W.N_NEIGHBORS)
    prob = O.refine_probabilities(RA, u, F.IJs, thr, labels, errs)
    order = np.lexsort((unc, O.tie_scramble(unc), -prob))
    ps = prob[order]
    starts = np.flatnonzero(np.r_[True, ps[1:] != ps[:-1]])
    ends = np.r_[starts[1:], ps.size]
    g = int(np.argmax(ends - starts))               # the largest tie group
    lo, hi = int(starts[g]), int(ends[g])
    m, look = unc.size, 5
    n_refines = sorted({1, lo + 1, (lo + hi) // 2 + 1, hi, m // look, m // look + 1, m, m + 3} - {0})
    want = {}
    for nr in n_refines:
        c, x = O.select_candidates(prob, nr, look, positions=unc)
        want[nr] = (unc[c], unc[x])
    F.upload(RA, ncm, labels)
    for tie_cap, redo in ((None, None), ("8", None), (None, "1"), ("8", "1")):
        monkeypatch.delenv("ANNCHOR_TIE_CAP", raising=False)
        monkeypatch.delenv("ANNCHOR_CUT_FORCE_REDO", raising=False)
        if tie_cap:
            monkeypatch.setenv("ANNCHOR_TIE_CAP", tie_cap)
        if redo:
            monkeypatch.setenv("ANNCHOR_CUT_FORCE_REDO", redo)
        for nr in n_refines:
            nc, nx_ = F.eng.select_candidates(W.N_NEIGHBORS, 0, errs, nr, look)
            assert np.array_equal(F.eng.download(F.nat.F_THRESH), thr)
            assert np.array_equal(F.eng.download(F.nat.F_PROB)[u], prob)
            cand, nxt = F.eng.download(F.nat.F_CAND), F.eng.download(F.nat.F_NEXT)
            assert (nc, nx_) == (cand.size, nxt.size)
            assert np.array_equal(cand, want[nr][0]), (kind, nr, tie_cap, redo)
            assert np.array_equal(nxt, want[nr][1]), (kind, nr, tie_cap, redo)


# ------------------------------------------------------------------------------------------------------------ brute force
def _grid(kind, nx, rng):
    if kind == "duplicates":
        return rng.integers(0, max(2, nx // 8), nx).astype(np.float64)
    if kind == "identical":
        return np.full(nx, 3.0)
    return np.arange(nx, dtype=np.float64)          # sorted grid


@pytest.mark.parametrize("nx", [2, 3, 97, 701])
@pytest.mark.parametrize("kind", ["duplicates", "identical", "sorted"])
def test_brute_force_rows(kind, nx):
    """k_bf_rows on 1-coordinate integer-grid points (|x - y| is exact) against the stable sort of the full matrix."""
    from annchor_amd import _native
    x = _grid(kind, nx, np.random.default_rng(nx))
    eng = _native.Engine(0)
    eng.set_points(x[:, None])
    oi, od, _ = O.brute_force(lambda IJ: np.abs(x[IJ[:, 0]] - x[IJ[:, 1]]), nx)
    for k in sorted({1, 2, max(1, nx // 2), nx}):
        gi, gd = eng.brute_force(k)
        assert np.array_equal(gi, oi[:, :k]) and np.array_equal(gd, od[:, :k]), k
    eng.close()


def test_brute_force_rows_beyond_the_lds_cap():
    """nx = 20 011 (2 x 10^8 pairs, 3.2 GB): the smallest shape whose rows no longer fit k_bf_rows' LDS copy (just under 19 968
    keys), so every radix pass and the collection re-gather the row from the pair list.  Reference in row blocks: the k
    smallest of the exact integer key distance * nx + index, i.e. (distance, index) ascending.  The one slow case of this file."""
    from annchor_amd import _native
    nx, k = 20011, 16
    rng = np.random.default_rng(20011)
    x = rng.integers(0, 3000, nx).astype(np.float64)        # heavy duplicates: ties decided by index
    eng = _native.Engine(0)
    eng.set_points(x[:, None])
    gi, gd = eng.brute_force(k)
    eng.close()
    xi = x.astype(np.int64)
    cols = np.arange(nx, dtype=np.int64)
    for b in sorted(set(range(0, nx, 4096)) | {nx - 1024}):      # every fourth block of 1024 rows and the last rows
        key = np.abs(xi[b:b + 1024, None] - xi[None, :]) * nx + cols[None, :]
        top = np.sort(np.partition(key, k - 1, axis=1)[:, :k], axis=1)
        assert np.array_equal(gi[b:b + 1024], top % nx), b
        assert np.array_equal(gd[b:b + 1024], (top // nx).astype(np.float64)), b


# -------------------------------------------------------------------------------------------------- process-wide switches
SETTINGS = {"defaults": {}, "transposed": {"ANNCHOR_TRANSPOSE_MIN": "0"},
            "shrink16_lds_copy": {"ANNCHOR_ROWC_SHRINK_MIN": "16", "ANNCHOR_ROW_LDS_COPY": "1"}}


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_process_wide_row_switches(tmp_path, setting):
    """The row source (gather through the index / column-ordered copy) and the second cut's minimum are read once per process:
    thresholds, guarantee_nmin and graph of all classes in a fresh child per setting."""
    out = str(tmp_path / (setting + ".json"))
    env = dict(os.environ, **SETTINGS[setting])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "row_paths_worker.py"), out], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(out) as fh:
        res = json.load(fh)
    assert len(res) == 3 * len(C.CLASSES) * len(W.WORKER_CASES)
    assert {k: v for k, v in res.items() if v} == {}
