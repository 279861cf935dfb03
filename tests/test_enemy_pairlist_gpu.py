"""The nearest-enemy graph on the pair list (csrc/enemies.hip) on injected states against the staged reference of
tests/enemy_pairlist_cases.py: every case through annchor_enemies_candidates / _download / _predict (model and vector) /
_first / _set_exact / _graph, every downloaded field of every stage compared bit for bit.  tests/test_enemy_pairlist_cases.py
asserts without a GPU that the reference ends where the oracle's nearest_enemies ends, that every case reaches its edges and
that the cases reach every kernel and mask width.

The enemy kernels read no environment thresholds: one process, one engine per case.  The fitted state is the device's own
(set_opaque or set_points, set_anchor_distances, build_locality, compute_features -- asserted to be the reference's before
anything else runs) with the case's RefineApprox and mask uploaded.  The todo list is compared as a sorted multiset: its
order comes from atomics.  There is no tolerance anywhere."""
import time

import numpy as np
import pytest

import enemy_pairlist_cases as P

pytestmark = pytest.mark.gpu
ESTATE, EINVAL = "error -5", "error -1"


def fitted_engine(name):
    from annchor_amd import _native as nat
    st = P.build(name)
    f = st.fit
    eng = nat.Engine()
    if st.device_metric:
        eng.set_points(P.grid_points()[0])
    else:
        eng.set_opaque(f.nx)
    eng.set_anchor_distances(f.D, f.A)
    n, shortest = eng.build_locality(f.locality, f.loc_thresh, f.fit_loc_min)
    eng.compute_features()
    assert n == len(f.IJs) and shortest == np.diff(f.I_ptr).min()
    assert np.array_equal(eng.download(nat.F_IJS).reshape(-1, 2), f.IJs)
    assert np.array_equal(eng.download(nat.F_I_PTR), f.I_ptr) and np.array_equal(eng.download(nat.F_I_IDX), f.I_idx)
    assert np.array_equal(eng.download(nat.F_FEATURES).reshape(-1, 4), f.feats)
    assert np.array_equal(eng.download(nat.F_NCM).astype(bool), f.ncm)
    return eng, nat


def inject(eng, nat, name):
    st = P.build(name)
    eng.upload(nat.F_RA, st.RA)
    eng.upload(nat.F_NCM, st.ncm.astype(np.uint8))


def sorted_pairs(todo):
    todo = np.asarray(todo, dtype=np.int64).reshape(-1, 2)
    return todo[np.lexsort((todo[:, 1], todo[:, 0]))]


def candidates(eng, name):
    st, r = P.build(name), P.stages(name)
    n = eng.enemies_candidates(st.y, st.fit.loc_thresh, st.loc_min)
    assert n == len(r["IJn"])
    ij, feats, _, ncm, ptr, idx = eng.enemies_download()
    assert np.array_equal(ptr, r["ptr_n"])                # (n == 0: the only array annchor_enemies_download fills)
    assert np.array_equal(ij, r["IJn"]) and np.array_equal(idx, r["idx_n"])
    assert np.array_equal(feats, r["feats_n"])
    assert np.array_equal(ncm, r["ncm_n0"])


def predict(eng, name, by_vector):
    st, r = P.build(name), P.stages(name)
    if by_vector:
        eng.enemies_predict(pred=r["pred_raw"])
    else:
        eng.enemies_predict(st.bins, st.W, st.c)
    got = eng.enemies_download()[2]
    assert np.array_equal(got, r["RA_n0"]), "first difference at pair %d" % np.flatnonzero(got != r["RA_n0"])[0]


def first_and_write_back(eng, nat, name):
    st, r = P.build(name), P.stages(name)
    if st.device_metric:
        assert eng.enemies_first(st.first, st.nn, True) == len(r["todo"])
    else:
        todo = eng.enemies_first(st.first, st.nn, False)
        assert np.array_equal(sorted_pairs(todo), r["todo"])
        eng.enemies_set_exact(st.E[todo[:, 0], todo[:, 1]])           # the table read in the device's order
    assert np.array_equal(eng.download(nat.F_RA), r["RA_f1"])
    assert np.array_equal(eng.download(nat.F_NCM).astype(bool), r["ncm_f1"])
    _, _, RA, ncm, _, _ = eng.enemies_download()
    assert np.array_equal(RA, r["RA_n1"]) and np.array_equal(ncm, r["ncm_n1"])


def graph(eng, name):
    st, r = P.build(name), P.stages(name)
    idx, dist = eng.enemies_graph(st.nn)
    assert np.array_equal(dist, r["ngd"])
    assert np.array_equal(idx, r["ngi"]), "rows %s" % np.flatnonzero((idx != r["ngi"]).any(axis=1))[:8]


def run_case(eng, nat, name):
    by_vector = P.build(name).by_vector
    inject(eng, nat, name)
    candidates(eng, name)
    predict(eng, name, not by_vector)      # both routes on every case, the case's own one last
    predict(eng, name, by_vector)
    first_and_write_back(eng, nat, name)
    graph(eng, name)


@pytest.mark.parametrize("name", list(P.CASES))
def test_every_stage_equals_the_reference(name):
    t0 = time.time()
    P.stages(name)
    t1 = time.time()
    eng, nat = fitted_engine(name)
    try:
        run_case(eng, nat, name)
    finally:
        eng.close()
    print("%s: reference %.2f s, device %.2f s" % (name, t1 - t0, time.time() - t1))


@pytest.mark.parametrize("before, name", [("n65_a64_clamp", "n65_a64_nothing_new"), ("n65_a64_nothing_new", "n65_a64_clamp"),
                                           ("n257_a257_wide_all_clamp", "n257_a257_wide_all_computed")])
def test_candidates_again_on_one_context_equal_a_fresh_one(before, name):
    """Another call's labels, loc_min, pair count and prediction are left behind on the context (no first list yet): the next
    call's every stage is what a fresh context gives."""
    t0 = time.time()
    assert P.CASES[before]["base"] == P.CASES[name]["base"] and len(P.stages(before)["IJn"]) != len(P.stages(name)["IJn"])
    eng, nat = fitted_engine(name)
    try:
        inject(eng, nat, before)
        candidates(eng, before)
        predict(eng, before, P.build(before).by_vector)
        run_case(eng, nat, name)
    finally:
        eng.close()
    print("%s after %s: %.2f s" % (name, before, time.time() - t0))


def test_refusals_leave_the_context_usable():
    """Each refused call returns an error and the next valid call gives the reference's result.  annchor_enemies_graph is only
    ever called where every row is long enough for the nn it is given: both of its refusals come from the host's guard."""
    t0 = time.time()
    name = "n65_a64_clamp"
    st, r = P.build(name), P.stages(name)
    eng, nat = fitted_engine(name)
    rows = np.diff(st.fit.I_ptr) + np.diff(r["ptr_n"])
    assert rows.min() > st.nn + 1
    try:
        inject(eng, nat, name)
        with pytest.raises(nat.NativeError, match=ESTATE):         # no candidates yet
            eng.enemies_predict(st.bins, st.W, st.c)
        candidates(eng, name)
        predict(eng, name, False)
        with pytest.raises(nat.NativeError, match=ESTATE):         # no first list yet: nothing has looked at the row lengths
            eng.enemies_graph(st.nn)
        with pytest.raises(nat.NativeError, match="no more than nn"):   # a row with len <= nn
            eng.enemies_first(st.first, int(rows.min()), False)
        todo = eng.enemies_first(st.first, st.nn, False)           # (the refused call's flag is not left standing)
        assert np.array_equal(sorted_pairs(todo), r["todo"])
        with pytest.raises(nat.NativeError, match=EINVAL):
            eng.enemies_set_exact(np.zeros(len(todo) + 1))
        assert np.array_equal(eng.download(nat.F_RA), st.RA)
        eng.enemies_set_exact(st.E[todo[:, 0], todo[:, 1]])
        assert np.array_equal(eng.download(nat.F_RA), r["RA_f1"]) and np.array_equal(eng.enemies_download()[2], r["RA_n1"])
        with pytest.raises(nat.NativeError, match=ESTATE):         # more neighbours than the first lists verified
            eng.enemies_graph(st.nn + 1)
        graph(eng, name)
        idx, dist = eng.enemies_graph(st.nn - 1)                   # fewer is a prefix
        assert np.array_equal(idx, r["ngi"][:, :st.nn - 1]) and np.array_equal(dist, r["ngd"][:, :st.nn - 1])
        # new candidates forget what was verified
        candidates(eng, name)
        predict(eng, name, False)
        with pytest.raises(nat.NativeError, match=ESTATE):
            eng.enemies_graph(st.nn)
    finally:
        eng.close()
    print("refusals: %.2f s" % (time.time() - t0))
