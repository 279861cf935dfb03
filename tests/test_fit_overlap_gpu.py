"""
fit() with its independent kernel chains on the engine's side stream against the same fit on one stream
(ANNCHOR_FIT_OVERLAP=0, read when the engine is created): every array the fit leaves behind is bit-identical, on the smallest
shapes that reach the overlapped chain -- update_bounds' mask-only prefix beside the statistics and the refinement launch, the
draw's trace kernel on the same stream.  Every comparison runs twice, on two fresh engines: a race between the two streams shows
up as a difference.
"""
import numpy as np
import pytest

from oracle import annchor_oracle as O
from oracle import metrics as om

pytestmark = pytest.mark.gpu

FIELDS = ("A", "D", "IJs", "features", "not_computed_mask", "RefineApprox")


def _strings():
    rng = np.random.default_rng(11)
    return ["".join(rng.choice(list("acgt"), size=int(n))) for n in rng.integers(20, 91, size=120)]


# n_samples / p_work: every partition of every draw holds its quota (the CPU pipeline on these strings: 200 samples in each of
# three iterations, 334 candidates and 1336 lookahead pairs per iteration at niters=3, 501 and 2004 at niters=2).  STR_SHORT is the
# shape next to it where the third draw runs a partition short of its quota (286 of 300 samples): a sampling step of another
# size behind a prepared update_bounds.  There the eval count of fit() is 10 above the CPU pipeline's on one stream as well, so
# that shape is compared between the two forms of fit() only.
STR_CFG = dict(n_anchors=5, n_neighbors=5, n_samples=200, p_work=0.25, random_seed=5)
STR_SHORT = dict(n_anchors=5, n_neighbors=5, n_samples=300, p_work=0.3, random_seed=5)
EUC_CFG = dict(n_anchors=5, n_neighbors=5, n_samples=600, p_work=0.2, random_seed=5)


def _data(kind):
    if kind == "strings":
        return np.array(_strings()), "levenshtein", STR_CFG
    if kind == "strings_short_quota":
        return np.array(_strings()), "levenshtein", STR_SHORT
    return np.random.default_rng(12).standard_normal((300, 8)), "euclidean", EUC_CFG


def _make(monkeypatch, kind, overlap, niters):
    """An Annchor whose engine was created with the overlap on / off (the switch is read at engine creation)."""
    from annchor_amd import Annchor

    X, metric, cfg = _data(kind)
    if overlap:
        monkeypatch.delenv("ANNCHOR_FIT_OVERLAP", raising=False)
    else:
        monkeypatch.setenv("ANNCHOR_FIT_OVERLAP", "0")
    ann = Annchor(X, metric, niters=niters, **cfg)
    monkeypatch.delenv("ANNCHOR_FIT_OVERLAP", raising=False)
    return ann


def _fit(monkeypatch, kind, overlap, niters):
    ann = _make(monkeypatch, kind, overlap, niters)
    lists = []
    select = ann._engine.select_candidates

    def recording(*a, **k):
        r = select(*a, **k)
        lists.append(r)
        return r

    ann._engine.select_candidates = recording
    ann.fit()
    out = {f: np.array(getattr(ann, f)) for f in FIELDS}
    out["errors"] = np.array(ann.errors)
    out["residuals"] = np.concatenate([np.asarray(ann.error_predictor.errs[b], dtype=np.float64) for b in ann.error_predictor.labels])
    out["evals"] = np.array(ann.evals)
    out["ng_idx"], out["ng_dist"] = (np.array(a) for a in ann.neighbor_graph)
    # the shape reaches the overlapped paths: models fitted on the device, and in every iteration a non-empty candidate list and a
    # non-empty lookahead list (no lookahead list: update_bounds returns at once and nothing is prepared)
    assert ann.__dict__.get("_model_on_device"), "the models of this fit were not fitted on the device"
    assert len(lists) == niters and all(nc > 0 and nn > 0 for nc, nn in lists), lists
    # ... and the overlapped route was the one taken: every update_bounds of the fit found its lists prepared (none on one stream)
    assert ann._engine.overlap_stats() == ((True, niters - 1) if overlap else (False, 0))
    return out


_single = {}


def _single_stream(monkeypatch, kind, niters):
    """The one-stream fit of a shape: computed once, shared, never written to."""
    if (kind, niters) not in _single:
        _single[(kind, niters)] = _fit(monkeypatch, kind, False, niters)
    return _single[(kind, niters)]


@pytest.mark.parametrize("kind,niters", [("strings", 2), ("strings", 3), ("euclid64", 2), ("euclid64", 3), ("strings_short_quota", 3)])
def test_fit_with_overlap_equals_fit_on_one_stream(monkeypatch, kind, niters):
    want = _single_stream(monkeypatch, kind, niters)
    for attempt in range(2):
        got = _fit(monkeypatch, kind, True, niters)
        for key, w in want.items():
            assert np.array_equal(got[key], w), "%s differs from the one-stream fit (engine %d)" % (key, attempt)


@pytest.mark.parametrize("niters", [2, 3])
def test_fit_with_overlap_equals_the_oracle_on_strings(monkeypatch, niters):
    X = _strings()
    P = om.PackedStrings(X)
    ora = O.OracleAnnchor(len(X), P.pairs, niters=niters, **STR_CFG).fit()
    got = _fit(monkeypatch, "strings", True, niters)
    assert np.array_equal(got["A"], ora.A)
    assert np.array_equal(got["D"], ora.D)
    assert int(got["evals"]) == ora.evals
    assert np.array_equal(got["ng_dist"], ora.neighbor_graph[1])
    assert np.array_equal(got["ng_idx"], ora.neighbor_graph[0])


def _staged_update(monkeypatch, kind, overlap, mode):
    """Iteration 0 stage by stage (one stream: the staged calls never use the side stream on their own), then update_bounds
    `mode`: plain; prepared (update_bounds_prepare first); touched (a call that clears mask bytes first); voided (prepare, then
    that call).  Returns what update_bounds leaves: the feature rows (lb, ub), the mask, RefineApprox."""
    from annchor_amd import _native

    ann = _make(monkeypatch, kind, overlap, 2)
    for stage in (ann.get_anchors, ann.get_locality, ann.get_features, ann.get_sample, ann.fit_predict_regression,
                  ann.fit_predict_errors):
        stage()
    ann.select_refine_candidate_pairs(w=0.5, it=0)
    eng = ann._engine
    assert len(ann.nextback) > 0
    if mode in ("prepared", "voided"):
        eng.update_bounds_prepare()
    if mode in ("touched", "voided"):
        pos = np.flatnonzero(eng.download(_native.F_NCM))[::3][:256].astype(np.int64)
        assert len(pos) == 256
        eng.evaluate_samples(pos)   # (256 more computed pairs: the computed-neighbour lists of their points grow)
    ann.update_anchor_points()
    assert eng.overlap_stats() == (bool(overlap), 1 if overlap and mode == "prepared" else 0)   # (voided: update_bounds built the lists itself)
    return [np.array(eng.download(f)) for f in (_native.F_FEATURES, _native.F_NCM, _native.F_RA)]


@pytest.mark.parametrize("kind", ["strings", "euclid64"])
def test_update_bounds_prepare_voided_by_a_mask_change(monkeypatch, kind):
    want = _staged_update(monkeypatch, kind, False, "touched")
    plain = _staged_update(monkeypatch, kind, False, "plain")
    assert not np.array_equal(want[0], plain[0]), "the extra computed pairs changed no bound: the case checks nothing"
    for attempt in range(2):
        got = _staged_update(monkeypatch, kind, True, "voided")
        for g, w in zip(got, want):
            assert np.array_equal(g, w)


@pytest.mark.parametrize("kind", ["strings", "euclid64"])
def test_update_bounds_with_and_without_prepare(monkeypatch, kind):
    want = _staged_update(monkeypatch, kind, False, "plain")
    for mode in ("plain", "prepared"):
        for attempt in range(2):
            got = _staged_update(monkeypatch, kind, True, mode)
            for g, w in zip(got, want):
                assert np.array_equal(g, w), mode
