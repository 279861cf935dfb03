"""The host restatement of the exact k-NN route (tests/exact_knn_cases.py) without a GPU: it equals the stable argsort of the
full distance matrix on every injected case and on the end-to-end data under a true, a spoiled, a random and an invalid seed;
the case set notices each deliberately wrong reference; the end-to-end data hold the ties, duplicates and pruned pairs the GPU
tests rely on; and the package's own seed radii (annchor_amd.radius.seed_radii, host code) are the reference's."""
import numpy as np
import pytest

import exact_knn_cases as K
import radius_cases as RC

_E2E = {}


def e2e(name):
    """The data set, its host matrix, max-min anchor table and true graph: computed once per session, never written."""
    if name not in _E2E:
        cfg = K.E2E[name]
        X, _, pairs = K.e2e_data(name)
        M = RC.matrix_of(len(X), pairs)
        D = K.maxmin_table(len(X), pairs, cfg["n_anchors"])
        T = K.truth(M, cfg["k"])
        for a in (M, D, T[0], T[1]):
            a.setflags(write=False)
        _E2E[name] = dict(nx=len(X), pairs=pairs, M=M, D=D, T=T, **cfg)
    return _E2E[name]


@pytest.mark.parametrize("name", list(K.CASES))
def test_reference_equals_the_sorted_matrix_on_the_injected_cases(name):
    c = K.CASES[name]
    _, u, M = K.build(name)
    ref = K.case_reference(name)
    assert K.same_graph((ref["idx"], ref["dist"]), K.truth(M, c["k"]))
    assert np.all(ref["row_entries"] >= c["k"] - 1)
    if not c["use_bounds"] or c["umode"] == "all_inf":
        assert ref["evals"] == c["nx"] * (c["nx"] - 1) // 2


def test_the_margin_is_needed_on_computed_float_distances():
    """Float positions on a line, radii at the attained k-th distances: the computed |x - a| obey the triangle inequality up to
    rounding only, so rtol = 0 prunes true neighbours and the case's 1e-9 does not."""
    name = "nx1100_line"
    c = K.CASES[name]
    D, u, M = K.build(name)
    assert c["rtol"] == 1e-9
    bare = K.route(D, K.metric(name), u, c["k"], 0.0)
    assert not K.same_graph((bare["idx"], bare["dist"]), K.truth(M, c["k"])) and bare["evals"] < K.case_reference(name)["evals"]


def test_cases_cover_the_kernel_edges():
    nxs = {c["nx"] for c in K.CASES.values()}
    nas = {c["na"] for c in K.CASES.values()}
    assert {1, 2, RC.COLS - 1, RC.COLS, RC.COLS + 1, RC.ROWS + 1, 1100} <= nxs and {1, RC.TILE, RC.TILE + 1, 65} <= nas
    for nx in (1, 2, 63, 64, 65, 129):
        assert {1, 2, 5, nx} & set(range(1, nx + 1)) <= {c["k"] for c in K.CASES.values() if c["nx"] == nx}
    # ties exactly on the test: |s - t| = R for a pair that is therefore evaluated
    D, u, _ = K.build("nx129_k5")
    R = np.maximum(u[:, None], u[None, :])
    assert np.any(np.triu(np.abs(D[:, None, 0] - D[None, :, 0]) == R, k=1))
    # radii that differ inside a pair, +inf beside finite ones, pruning under an inf anchor
    _, u, _ = K.build("nx129_loose")
    assert len(np.unique(u)) > 3
    _, u, _ = K.build("some_inf")
    assert 0 < np.isinf(u).sum() < len(u)
    n = lambda nm: K.CASES[nm]["nx"] * (K.CASES[nm]["nx"] - 1) // 2   # noqa: E731
    for nm in ("nx129_k5", "some_inf", "inf_anchor", "inf_anchor_wide", "line_rtol", "na65_rtol"):
        assert 0 < K.case_reference(nm)["evals"] < n(nm), nm
    # chunked cases: a row above the cap, and several rows under it
    for nm in ("chunked", "chunked_inf", "chunked_one"):
        tot = K.case_reference(nm)["row_eval"]
        assert tot.max() > K.CASES[nm]["cap"] and tot.sum() > 4 * K.CASES[nm]["cap"]
    # rows longer than any LDS cap the GPU test passes, and rows that end exactly at k - 1 entries
    assert K.case_reference("nx1100_k1100")["row_entries"].min() == 1099
    assert np.any(K.case_reference("line_k5")["row_entries"] == 4)   # (distinct distances: nothing ties at the radius)


def _differs(a, b):
    return any(a[f].shape != b[f].shape or a[f].tobytes() != b[f].tobytes() for f in ("eval", "row_eval", "idx", "dist", "row_entries"))


@pytest.mark.parametrize("wrong", K.WRONG)
def test_case_set_notices_a_wrong_reference(wrong):
    """Every deliberate mistake changes the lists, the entry counts or the graph of at least one injected case."""
    caught = []
    for name, c in K.CASES.items():
        if c["nx"] > 300:
            continue   # (the small cases suffice; the large ones cost seconds each)
        D, u, _ = K.build(name)
        bad = K.route(D, K.metric(name), u, c["k"], c["rtol"], c["use_bounds"], wrong=wrong)
        if _differs(K.case_reference(name), bad):
            caught.append(name)
    print(wrong, "noticed by", len(caught), "cases")
    assert caught, wrong


@pytest.mark.parametrize("name", list(K.E2E))
def test_e2e_data_hold_what_the_gpu_tests_rely_on(name):
    s = e2e(name)
    nx, k, M = s["nx"], s["k"], s["M"]
    srt = np.sort(M, axis=1)
    tied = int((srt[:, k - 1] == srt[:, k]).sum())
    lower_dup = int((s["T"][0][:, 0] != np.arange(nx)).sum())
    u = K.seed_radii(nx, k, s["T"][0], s["pairs"])
    assert np.array_equal(u, srt[:, k - 1])
    pruned = nx * (nx - 1) // 2 - int(K.classify(s["D"], u, s["rtol"]).sum())
    print("%s: %d of %d rows tied at the k-th place, %d rows start with a lower-index duplicate, %d pairs pruned under the true seed"
          % (name, tied, nx, lower_dup, pruned))
    assert tied > 0 and lower_dup > 0 and pruned > 0
    for kind in ("spoiled", "random"):
        G = K.seed_graph(kind, s["T"][0], k)
        wrong_rows = int((np.sort(G, axis=1) != np.sort(s["T"][0], axis=1)).any(axis=1).sum())
        assert wrong_rows > 0, kind
    G = K.seed_graph("invalid", s["T"][0], k)
    assert np.isinf(K.seed_radii(nx, k, G, s["pairs"])).sum() == len(range(0, nx, 3))


@pytest.mark.parametrize("kind", K.SEEDS)
@pytest.mark.parametrize("name", list(K.E2E))
def test_numpy_route_equals_the_truth(name, kind):
    s = e2e(name)
    nx, k = s["nx"], s["k"]
    G = K.seed_graph(kind, s["T"][0], k)
    u = K.seed_radii(nx, k, G, s["pairs"])
    got = K.route(s["D"], s["pairs"], u, k, s["rtol"])
    pairs = nx * (nx - 1) // 2
    print("%s, %s seed: %d of %d pairs evaluated (%.1f %%)" % (name, kind, got["evals"], pairs, 100.0 * got["evals"] / pairs))
    assert K.same_graph((got["idx"], got["dist"]), s["T"])
    assert np.all(got["row_entries"] >= k - 1)
    if kind == "true":
        assert got["evals"] < pairs // 4


@pytest.mark.parametrize("kind", K.SEEDS)
def test_package_seed_radii_are_the_reference(kind):
    """annchor_amd.radius.seed_radii is host code: the same radii, every unordered pair evaluated once."""
    from annchor_amd import radius

    s = e2e("levenshtein")
    nx, k = s["nx"], s["k"]
    G = K.seed_graph(kind, s["T"][0], k)
    asked = []

    def pairs(IJ):
        asked.append(np.array(IJ))
        return s["pairs"](IJ)

    u, evals, inf_rows = radius.seed_radii(nx, k, np.concatenate([G, G[:, :2]], axis=1), pairs)   # (columns past k are not read)
    want = K.seed_radii(nx, k, G, s["pairs"])
    assert u.dtype == np.float64 and np.array_equal(u, want)
    assert inf_rows == int(np.isinf(want).sum())
    IJ = np.concatenate(asked) if asked else np.zeros((0, 2), dtype=np.int64)
    assert evals == len(IJ) == len(np.unique(IJ[:, 0] * nx + IJ[:, 1])) and np.all(IJ[:, 0] < IJ[:, 1])
    # entries outside 0..nx-1 and a row short of k - 1 distinct entries: +inf, and nothing of such a row is evaluated
    B = G.copy()
    B[0, 1], B[1, :] = nx, B[1, 0]
    u2, _, _ = radius.seed_radii(nx, k, B, s["pairs"])
    assert np.isinf(u2[0]) and np.isinf(u2[1]) and np.array_equal(u2[2:], want[2:])
    with pytest.raises(ValueError, match="seed_graph must hold integer indices"):
        radius.seed_radii(nx, k, G[:, :k - 1], s["pairs"])
    u1, e1, _ = radius.seed_radii(nx, 1, G, s["pairs"])
    assert np.array_equal(u1, K.seed_radii(nx, 1, G, s["pairs"]))   # k = 1: the first column alone, no entry needed
    if kind == "true":
        assert np.array_equal(u1, np.zeros(nx)) and e1 == int((G[:, 0] != np.arange(nx)).sum())   # (a lower-index duplicate leads its row)
