"""The host restatement of the fixed-radius query rule (tests/radius_query_cases.py) without a GPU: against a plain loop over
(q, j, a) on every case, that the case set notices each deliberately wrong reference, that the rule is the graph form's rule
(tests/radius_cases.py) wherever both apply, and that the cases reach the kernel's edges."""
import numpy as np
import pytest

import radius_cases as C
import radius_query_cases as Q


@pytest.mark.parametrize("name", list(Q.CASES))
def test_restated_rule_equals_the_plain_loop(name):
    c = Q.CASES[name]
    D, QD = Q.build(name)
    want = Q.classify_q_loop(D, QD, c["r"], c["rtol"], c["conn"], c["use_bounds"])
    got = Q.case_classes(name)
    assert got.shape == (c["nq"], c["nx"]) and np.array_equal(got, want)
    L = Q.lists_q(got)
    # the lists are the classes, query-major with ascending j, as (j, nx + q)
    for key, k in (("eval", Q.EVAL), ("sure", Q.SURE)):
        rows = [(j, c["nx"] + q) for q in range(c["nq"]) for j in range(c["nx"]) if want[q, j] == k]
        assert np.array_equal(L[key], np.array(rows, dtype=np.int64).reshape(-1, 2))
    assert L["row_eval"].sum() + L["row_sure"].sum() + L["pruned"] == c["nq"] * c["nx"]


def _differs(a, b):
    return any(a[k].tobytes() != b[k].tobytes() or a[k].shape != b[k].shape for k in ("eval", "sure", "row_eval", "row_sure"))


@pytest.mark.parametrize("wrong", Q.WRONG)
def test_case_set_notices_a_wrong_reference(wrong):
    caught = [name for name in Q.CASES if _differs(Q.case_reference(name), Q.case_reference(name, wrong))]
    assert caught, wrong


@pytest.mark.parametrize("name", [n for n in C.CASES if C.CASES[n]["nx"] <= 300])
def test_rule_is_the_graph_rule_when_the_queries_are_the_data(name):
    """QD = D: the class of (query i, data point j) is the graph form's class of the pair (min, max), for every i != j."""
    c = C.CASES[name]
    D = C.build(name)
    graph = C.classify(D, c["r"], c["rtol"], c["conn"], c["use_bounds"])           # -1 outside i < j
    rect = Q.classify_q(D, D, c["r"], c["rtol"], c["conn"], c["use_bounds"])
    upper = np.triu(np.ones(graph.shape, dtype=bool), k=1)
    assert np.array_equal(rect[upper], graph[upper])
    assert np.array_equal(rect.T[upper], graph[upper])                             # (query j, data point i), i < j
    assert np.all(np.diagonal(rect) >= 0)                                          # the diagonal is classified too


def test_cases_cover_the_kernel_edges():
    cs = Q.CASES.values()
    assert {1, 63, 64, 65, 127, 128, 129, 200} <= {c["nx"] for c in cs}
    assert {1, 2, 63, 64, 65, 130} <= {c["nq"] for c in cs}
    assert {1, 31, 32, 33, 65} <= {c["na"] for c in cs}
    ref = {nm: Q.case_reference(nm) for nm in Q.CASES}
    n = lambda nm: Q.CASES[nm]["nx"] * Q.CASES[nm]["nq"]   # noqa: E731
    assert ref["all_out"]["pruned"] == n("all_out")
    assert len(ref["all_eval"]["eval"]) == n("all_eval") and len(ref["all_sure"]["sure"]) == n("all_sure")
    assert len(ref["no_bounds"]["eval"]) == n("no_bounds") and len(ref["no_bounds_conn"]["eval"]) == n("no_bounds_conn")
    # ties exactly on both tests, with rtol 0 and with rtol > 0 (0.25 m is exact for these integers)
    for nm in ("ties", "ties_rtol"):
        c = Q.CASES[nm]
        D, QD = Q.build(nm)
        s, t = QD[:, None, :], D[None, :, :]
        tol = c["rtol"] * ((s + t) + c["r"])
        assert np.any(np.abs(s - t) - c["r"] == tol) and np.any(c["r"] - (s + t) == tol), nm
        assert len(ref[nm]["eval"]) and len(ref[nm]["sure"]) and ref[nm]["pruned"]
    # queries that are copies of data rows (a zero lower bound on the diagonal), duplicate data rows, inf that still decides
    D, QD = Q.build("copy")
    assert np.array_equal(QD, D[:70]) and np.all(np.diagonal(Q.case_classes("copy")) != Q.OUT)
    assert len(ref["dups"]["eval"]) + len(ref["dups"]["sure"]) == n("dups")
    assert 0 < ref["inf"]["pruned"] < n("inf")
    D, QD = Q.build("inf")
    assert np.isinf(D).any() and np.isinf(QD).any()
    # queries with an empty row between queries with some
    tot = ref["islands"]["row_eval"] + ref["islands"]["row_sure"]
    assert np.all(tot[1::2] == 0) and np.all(tot[0::2] > 0)
    # chunked cases: a query above the cap (bisected by column), and several calls
    for nm in ("chunked", "chunked_dist", "chunked_all", "islands_chunked"):
        tot = ref[nm]["row_eval"] + ref[nm]["row_sure"]
        assert tot.max() > Q.CASES[nm]["cap"] and tot.sum() > 4 * Q.CASES[nm]["cap"]
    # sub-ranges off the block and chunk boundaries, with something to list
    for nm in ("sub", "sub_dist", "sub_one"):
        qb, qe, cb, ce = Q.CASES[nm]["sub"]
        assert 0 <= qb < qe <= Q.CASES[nm]["nq"] and 0 <= cb < ce <= Q.CASES[nm]["nx"]
        L = Q.restrict(Q.case_classes(nm), Q.CASES[nm]["sub"])
        assert len(L["eval"]) + len(L["sure"]) > 0
    assert any(c["sub"] and (c["sub"][0] % 64 and c["sub"][1] % 64 and c["sub"][2] % 64 and c["sub"][3] % 128) for c in cs)


def test_neighbors_from_matrix_is_the_double_loop():
    rng = np.random.default_rng(3)
    R = rng.integers(0, 6, (7, 11)).astype(np.float64)
    indptr, idx, d = Q.neighbors_from_matrix(R, 2.0)
    rows = [[(j, R[q, j]) for j in range(11) if R[q, j] <= 2.0] for q in range(7)]
    assert np.array_equal(indptr, np.concatenate([[0], np.cumsum([len(x) for x in rows])]))
    assert np.array_equal(idx, [e[0] for x in rows for e in x]) and np.array_equal(d, [e[1] for x in rows for e in x])
