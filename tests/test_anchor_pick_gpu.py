"""The max-min anchor pick on every route that runs it, on the line family of anchor_pick_cases.py: ties in every round, one of
them between an index and a LATER index that a lower-numbered lane, wave, workgroup or trip reads, a maximal value at the last
index, a repeated anchor.  Each test calls the route directly and compares A and D with the one reference, array_equal; where
the library profiles launches, the route that ran is asserted too.

  route 1   k_runmin_argmax_one (picker.hip)                          test_one_workgroup
  route 2   k_runmin_argmax + k_argmax_final (picker.hip)             test_partials_and_final
  route 3   the pick blocks of k_lev_a2, k_lev_f, k_lev_r (lev.hip)   test_fused_levenshtein*
  route 4   k_lev_ap and its rescue form                              pinned by test_lev_column_gpu.py::test_anchor_rounds_one_launch
  route 5   emd_pick (emd.hip)                                        pinned by test_emd_maxmin_gpu.py
  route 6   k_st_runmin_argmax -> k_sh_cand -> k_sh_pick              test_streamed_*
  route 7   annchor_stream_anchor_round's host loop                   test_streamed_host_reduced
  route 8   k_sh_pick among several ranks                             test_several_ranks

test_anchor_pick_cases.py holds the conditions that keep these from passing vacuously."""
import numpy as np
import pytest

import anchor_pick_cases as ac
import pool_cases as pc

pytestmark = pytest.mark.gpu

NA = ac.NA


# ------------------------------------------------------------------------------------------------------ pair-list form
def _bind(case, kind):
    from annchor_amd import _native
    from annchor_amd.distances import euclidean, levenshtein

    if kind == "hausdorff":
        return pc.bound("hausdorff", ac.point_sets(case.p))
    eng = _native.Engine(0)
    if kind == "lev":
        levenshtein.bind(eng, ac.strings(case.p))
    else:
        euclidean.bind(eng, ac.points64(case.p) if kind == "f64" else ac.points32(case.p))
    return eng


def _pick(eng, case):
    """pick_anchors_maxmin on a bound engine -> (A, D [nx, NA], launches by profile scope)."""
    from annchor_amd import _native

    eng.prof_enable(True)
    eng.prof_reset()
    eng.pick_anchors_maxmin(NA, case.first)
    eng.synchronize()
    prof = eng.prof_get()
    eng.prof_enable(False)
    A = np.asarray(eng.download(_native.F_A)).copy()
    D = np.asarray(eng.download(_native.F_D)).reshape(case.nx, NA).copy()
    return A, D, {k: v["launches"] for k, v in prof.items()}


def _check(case, A, D, launches, want_argmax, lev_rounds=False):
    """A and D against the reference; the picker's own arg-max ran `want_argmax` times; lev_rounds: the Levenshtein rounds
    were NA launches of their own, not the one persistent launch (one profile scope)."""
    wantA, wantD = ac.case_reference(case.name)
    assert np.array_equal(A, wantA), (case.name, A, wantA)
    assert np.array_equal(D, wantD), (case.name, np.argwhere(D != wantD)[:8])
    assert launches.get("maxmin_argmax", 0) == want_argmax, (case.name, launches)
    if lev_rounds:
        assert launches.get("levenshtein_pairs", 0) == NA, (case.name, launches)


def _kind(name):
    return name.split("-")[1]


ONE = [n for n, c in ac.CASES.items() if c.route == "one"]
PARTIALS = [n for n, c in ac.CASES.items() if c.route == "partials"]
FUSED = [n for n, c in ac.CASES.items() if c.route == "fused"]
STREAM = [n for n, c in ac.CASES.items() if c.route == "stream"]


@pytest.mark.parametrize("name", ONE)
def test_one_workgroup(name):
    """Route 1: nx <= 16384 and a launch that does not fuse the pick -- Euclidean in both widths, Hausdorff, and Levenshtein
    one string past the fused limit."""
    case = ac.CASES[name]
    assert case.nx <= ac.ONE_MAX and (_kind(name) != "lev" or case.nx > ac.FUSED_MAX)
    eng = _bind(case, _kind(name))
    try:
        _check(case, *_pick(eng, case), NA - 1, lev_rounds=_kind(name) == "lev")
    finally:
        eng.close()


@pytest.mark.parametrize("name", PARTIALS)
def test_partials_and_final(name):
    """Route 2: 17 workgroups (the first size of the route) and 65 (k_argmax_final's second trip over the partials)."""
    case = ac.CASES[name]
    assert case.nx > ac.ONE_MAX
    eng = _bind(case, _kind(name))
    try:
        _check(case, *_pick(eng, case), NA - 1, lev_rounds=_kind(name) == "lev")
    finally:
        eng.close()


@pytest.mark.parametrize("name", FUSED)
def test_fused_levenshtein(name, monkeypatch):
    """Route 3, the round-by-round launches (k_lev_a2): twice on one engine -- the second call starts from the first call's
    running minimum, which round 1's reset has to discard."""
    case = ac.CASES[name]
    assert case.nx <= ac.FUSED_MAX
    monkeypatch.setenv("ANNCHOR_LEV_PERSIST", "0")
    for var in ("ANNCHOR_LEV_ANCHOR", "ANNCHOR_LEV_R"):
        monkeypatch.delenv(var, raising=False)
    eng = _bind(case, "lev")
    try:
        _check(case, *_pick(eng, case), 0, lev_rounds=True)
        _check(case, *_pick(eng, case), 0, lev_rounds=True)
    finally:
        eng.close()


@pytest.mark.parametrize("var,value", [("ANNCHOR_LEV_ANCHOR", "0"), ("ANNCHOR_LEV_R", "1")], ids=["k_lev_f", "k_lev_r"])
def test_fused_levenshtein_forced_variants(var, value, monkeypatch):
    """Route 3 in the pair-list kernels' pick blocks (trips of 512: elements 511 and 512 tie across the boundary)."""
    case = ac.CASES["fused-lev-513"]
    monkeypatch.setenv("ANNCHOR_LEV_PERSIST", "0")
    for v in ("ANNCHOR_LEV_ANCHOR", "ANNCHOR_LEV_R"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv(var, value)
    eng = _bind(case, "lev")
    try:
        _check(case, *_pick(eng, case), 0, lev_rounds=True)
        _check(case, *_pick(eng, case), 0, lev_rounds=True)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------- streamed form
def _stream_reference(X, first):
    """(A, D float32 [NA, n], anchor vectors, per-round (maximum, first maximal index)) of lattice rows."""
    A, D = ac.lattice_reference(X, first)
    return A, np.ascontiguousarray(D.T.astype(np.float32)), X[A], [(m, arg) for m, arg, _ in ac.rounds(D)]


def _stream_D(eng, n):
    """The anchor distances the sweeps left on the device, float32 [NA, n]."""
    send, _, _ = eng.stream_anchor_dists_begin([n])
    out = np.empty((NA, n), dtype=np.float32)
    eng.device_copy(out.ctypes.data, send, out.nbytes, "d2h")
    return out


def _stream_case(name, dim):
    if name == "single-row":
        return ac.single_row(dim), 0
    case = ac.CASES[name]
    return ac.lattice(case.p, dim), case.first


@pytest.fixture(scope="module")
def stream_ref():
    store = {}

    def get(name, dim):
        if (name, dim) not in store:
            X, first = _stream_case(name, dim)
            store[(name, dim)] = (X, first) + _stream_reference(X, first)
        return store[(name, dim)]

    return get


@pytest.mark.parametrize("dim", [3, 8])
@pytest.mark.parametrize("name", ["single-row"] + STREAM)
@pytest.mark.parametrize("how", ["steps", "rounds"])
def test_streamed_device_resident(how, name, dim, stream_ref):
    """Route 6, one rank: stream_anchor_step per round with the candidate buffer as its own gather, and the one-call
    stream_anchor_rounds.  dim 3 takes k_st_one_to_all's scalar branch, dim 8 its float4 branch."""
    from annchor_amd import _native

    X, first, wantA, wantD, wantV, _ = stream_ref(name, dim)
    eng = _native.Engine(0)
    try:
        eng.stream_bind(X, 0)
        cand, _, _ = eng.stream_anchor_begin(NA, first, 1)
        if how == "steps":
            for r in range(NA):
                eng.stream_anchor_step(cand, 1, r)
        else:
            eng.stream_anchor_rounds(NA)
        A, V = eng.stream_anchor_end(NA)
        D = _stream_D(eng, len(X))
    finally:
        eng.close()
    assert np.array_equal(A, wantA), (A, wantA)
    assert np.array_equal(V, wantV)
    assert np.array_equal(D, wantD), np.argwhere(D != wantD)[:8]


@pytest.mark.parametrize("dim", [3, 8])
@pytest.mark.parametrize("name", ["single-row"] + STREAM)
def test_streamed_host_reduced(name, dim, stream_ref):
    """Route 7: stream_anchor_round is handed the reference's anchor vectors; its host loop over the partials has to return the
    reference's (maximum, first maximal index) of every round."""
    from annchor_amd import _native

    X, first, wantA, wantD, wantV, want_rounds = stream_ref(name, dim)
    eng = _native.Engine(0)
    try:
        eng.stream_bind(X, 0)
        got = [eng.stream_anchor_round(wantV[r], r, NA) for r in range(NA)]
        D = _stream_D(eng, len(X))
    finally:
        eng.close()
    assert got == [(float(m), int(arg)) for m, arg in want_rounds], (got, want_rounds)
    assert [arg for _, arg in got[:-1]] == wantA[1:].tolist()
    assert np.array_equal(D, wantD)


@pytest.mark.parametrize("dim", [3, 8])
@pytest.mark.parametrize("W", sorted(ac.RANKS))
def test_several_ranks(W, dim):
    """Route 8: W engines on one device, advanced in lockstep by one thread -- StreamedAnnchor.get_anchors' protocol with the
    all-gather done by device copies.  Every rank has to report the reference's anchors of the concatenated rows."""
    from annchor_amd import _native

    case = ac.CASES["ranks-%d" % W]
    X = ac.lattice(case.p, dim)
    wantA, wantD, wantV, _ = _stream_reference(X, case.first)
    starts = np.concatenate([[0], np.cumsum(case.sizes)]).astype(np.int64)
    engines = [_native.Engine(0) for _ in range(W)]
    try:
        bufs = []
        for r, eng in enumerate(engines):
            eng.stream_bind(np.ascontiguousarray(X[starts[r]:starts[r + 1]]), int(starts[r]))
            bufs.append(eng.stream_anchor_begin(NA, case.first, W))
        nbytes = bufs[0][2]
        assert all(b[2] == nbytes for b in bufs) and nbytes == 8 * (2 + dim)
        for rnd in range(NA):
            for eng in engines:
                eng.synchronize()
            for src, (cand, _, _) in zip(engines, bufs):            # the all-gather: rank r's candidate into slot r everywhere
                r = engines.index(src)
                for _, gathered, _ in bufs:
                    src.device_copy(gathered + r * nbytes, cand, nbytes, "d2d")
            for eng, (_, gathered, _) in zip(engines, bufs):
                eng.stream_anchor_step(gathered, W, rnd)
        got = []
        for r, eng in enumerate(engines):
            A, V = eng.stream_anchor_end(NA)
            got.append((A, V, _stream_D(eng, case.sizes[r])))
    finally:
        for eng in engines:
            eng.close()
    for r, (A, V, D) in enumerate(got):
        assert np.array_equal(A, wantA), (r, A, wantA)
        assert np.array_equal(V, wantV), r
        assert np.array_equal(D, wantD[:, starts[r]:starts[r + 1]]), r
