"""The host restatement of the fixed-radius graph (tests/radius_cases.py) without a GPU: against a plain double loop on small
data under a host metric, that the case set notices each deliberately wrong reference, and that the end-to-end string case
is one on which the anchor bounds prune at least half of all pairs."""
import numpy as np
import pytest

import radius_cases as C


def maxmin_table(nx, pairs_fn, na, first=0):
    """Anchor table of the max-min picker from a fixed first anchor: float64 [nx, na]."""
    D = np.zeros((nx, na), dtype=np.float64)
    a, runmin = first, None
    for k in range(na):
        D[:, k] = pairs_fn(np.stack([np.full(nx, a), np.arange(nx)], axis=1).astype(np.int64))
        runmin = D[:, k].copy() if runmin is None else np.minimum(runmin, D[:, k])
        a = int(np.argmax(runmin))
    return D


@pytest.fixture(scope="module")
def small_strings():
    X = C.clustered_strings(60, length=30, seed=4)
    f = C.levenshtein_pairs(X)
    return dict(nx=len(X), pairs=f, M=C.matrix_of(len(X), f), D=maxmin_table(len(X), f, 4), rtol=0.0)


@pytest.fixture(scope="module")
def small_series():
    from seqdp_cases import clustered_curves, erp_pairs_host

    S = clustered_curves(40, 6, 14, 2, seed=41)
    f = lambda IJ: erp_pairs_host(S, IJ, 0.0)   # noqa: E731
    return dict(nx=len(S), pairs=f, M=C.matrix_of(len(S), f), D=maxmin_table(len(S), f, 5), rtol=1e-9)


def _check_against_loop(data):
    nx, M = data["nx"], data["M"]
    radii = C.edge_radii(M)
    assert radii[1] < M[M > 0].min() and radii[-1] > M.max() and radii[3] in M and radii[4] in M
    for r in radii:
        want = C.graph_from_matrix(M, r)
        for conn in (False, True):
            for use_bounds in (True, False):
                got = C.reference(data["D"], data["pairs"], r, data["rtol"], conn, use_bounds)
                assert C.same_graph(got["graph"], want, distances=not conn), (r, conn, use_bounds)
                assert got["evals"] + got["pruned"] + len(got["sure"]) == nx * (nx - 1) // 2
    # (the matrix form of the ground truth is the double loop)
    r = radii[3]
    assert C.same_graph(C.double_loop(nx, lambda i, j: M[i, j], r), C.graph_from_matrix(M, r))
    empty, full = C.graph_from_matrix(M, radii[1]), C.graph_from_matrix(M, radii[-1])
    assert len(empty[1]) == int((M == 0).sum()) - nx and len(full[1]) == nx * (nx - 1)


def test_reference_equals_the_double_loop_levenshtein(small_strings):
    _check_against_loop(small_strings)


def test_reference_equals_the_double_loop_erp(small_series):
    _check_against_loop(small_series)


def _differs(a, b):
    return any(a[k].tobytes() != b[k].tobytes() or a[k].shape != b[k].shape for k in ("eval", "sure", "row_eval", "row_sure"))


@pytest.mark.parametrize("wrong", C.WRONG)
def test_case_set_notices_a_wrong_reference(wrong, small_strings):
    """Every deliberate mistake changes the lists of at least one injected-table case, or the graph of the string set at one
    of the edge radii: the cases reach the comparison, the anchor reduction, the margin, the diagonal, the last anchor and
    the last column."""
    caught = []
    for name, c in C.CASES.items():
        if c["nx"] > 300:
            continue   # (the small cases suffice; the large ones cost seconds each)
        D = C.build(name)
        good = C.lists(C.classify(D, c["r"], c["rtol"], c["conn"], c["use_bounds"]))
        bad = C.lists(C.classify(D, c["r"], c["rtol"], c["conn"], c["use_bounds"], wrong=wrong))
        if _differs(good, bad):
            caught.append(name)
    s = small_strings
    for r in C.edge_radii(s["M"]):
        got = C.reference(s["D"], s["pairs"], r, s["rtol"], False, wrong=wrong)
        if not C.same_graph(got["graph"], C.graph_from_matrix(s["M"], r)):
            caught.append("strings r=%g" % r)
    assert caught, wrong


def test_cases_cover_the_kernel_edges():
    nxs = {c["nx"] for c in C.CASES.values()}
    nas = {c["na"] for c in C.CASES.values()}
    assert {1, 2, C.COLS - 1, C.COLS, C.COLS + 1, C.ROWS + 1, 1100} <= nxs
    assert {1, 2, C.TILE, C.TILE + 1, 65, 257} <= nas
    ref = {nm: C.case_reference(nm) for nm in C.CASES if C.CASES[nm]["nx"] <= 300}
    n = lambda nm: C.CASES[nm]["nx"] * (C.CASES[nm]["nx"] - 1) // 2   # noqa: E731
    assert ref["all_out"]["pruned"] == n("all_out")
    assert len(ref["all_eval"]["eval"]) == n("all_eval") and len(ref["all_sure"]["sure"]) == n("all_sure")
    assert len(ref["no_bounds"]["eval"]) == n("no_bounds")
    # ties exactly on both tests, duplicates, an inf table that still decides pairs
    D, c = C.build("nx129"), C.CASES["nx129"]
    assert np.any(np.abs(D[:, None, 0] - D[None, :, 0]) == c["r"]) and np.any(D[:, None, 0] + D[None, :, 0] == c["r"])
    assert len(ref["dups"]["eval"]) + len(ref["dups"]["sure"]) == n("dups")
    assert 0 < ref["inf"]["pruned"] < n("inf")
    # chunked cases: a row above the cap, and several rows under it
    for nm in ("chunked", "chunked_dist", "chunked_all", "islands_chunked"):
        tot = ref[nm]["row_eval"] + ref[nm]["row_sure"]
        assert tot.max() > C.CASES[nm]["cap"] and tot.sum() > 4 * C.CASES[nm]["cap"]
    # rows without candidates between rows with some
    tot = ref["islands"]["row_eval"] + ref["islands"]["row_sure"]
    assert np.all(tot[1:101:2] == 0) and np.all(tot[0:100:2] > 0)


def test_the_string_case_prunes_at_least_half():
    """The end-to-end string case (tests/test_radius_gpu.py) at its radius: the reference filter, on a max-min anchor table of
    the same width, excludes at least half of all pairs."""
    X = C.clustered_strings(C.E2E_STRINGS["n"])
    f = C.levenshtein_pairs(X)
    D = maxmin_table(len(X), f, C.E2E_STRINGS["n_anchors"])
    L = C.lists(C.classify(D, C.E2E_STRINGS["r"], 0.0, False))
    pairs = len(X) * (len(X) - 1) // 2
    print("pruned %d of %d pairs (%.1f %%), %d candidates" % (L["pruned"], pairs, 100.0 * L["pruned"] / pairs, len(L["eval"])))
    assert 2 * L["pruned"] >= pairs
