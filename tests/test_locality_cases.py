"""Host-side checks of tests/locality_cases.py: the cases build and are what their reason lines say, the references agree with
each other across mask widths, cases x forms reach every kernel of the candidate-generation and feature stage through the
dispatch mirror, and every deliberately wrong reference is noticed by at least one case.  Statements about the INPUTS of
tests/test_locality_gpu.py; no GPU here."""
import numpy as np
import pytest

import locality_cases as C
from oracle import annchor_oracle as O

BY_SIZE = sorted(C.CASES, key=lambda nm: C.CASES[nm]["nx"] * C.CASES[nm]["nx"] * C.CASES[nm]["na"])


def test_table_holds_the_shapes_it_promises():
    cs = list(C.CASES.values())
    assert 28 <= len(cs) <= 34 and 7 <= len(C.QUERY_CASES) <= 10
    assert {2, 31, 33, 63, 64, 65, 127, 129, 257, 1030} <= {c["nx"] for c in cs} and max(c["nx"] for c in cs) == 1030
    assert {1, 7, 8, 9, 64, 65, 128, 129, 256, 257, 300} <= {c["na"] for c in cs}
    assert {1, 3, 5, 9, 12} <= {c["locality"] for c in cs} and any(c["locality"] > c["na"] for c in cs)
    assert {1, 2, 5, 8, 9} <= {c["loc_thresh"] for c in cs} and any(c["loc_thresh"] > c["locality"] for c in cs)
    assert {0, 5, 20} <= {c["loc_min"] for c in cs}
    assert any(c["loc_min"] == c["nx"] - 1 for c in cs) and any(c["loc_min"] == c["nx"] + 70 for c in cs)
    assert {"ties", "metric", "twins"} == {c["kind"] for c in cs}
    assert {"all", "short", "repeat", "p6364", "ends"} <= {c["akind"] for c in cs}
    wide = [c for c in cs if c["na"] > 256]
    assert {31, 129, 1030} <= {c["nx"] for c in wide}
    assert any(1 <= c["loc_thresh"] <= 8 for c in wide) and any(c["loc_thresh"] == 9 and c["locality"] > 8 for c in wide)
    assert any(c["loc_thresh"] > 8 and 1 <= c["locality"] <= 8 for c in wide)
    q = list(C.QUERY_CASES.values())
    assert {1, 63, 255, 256, 257, 600} <= {c["nxb"] for c in q} and {1, 5} == {c["nq"] for c in q}
    assert any(c["na"] > 256 for c in q) and any(c["na"] <= 256 for c in q)


@pytest.mark.parametrize("name", list(C.CASES))
def test_case_builds_and_is_what_it_says(name):
    c = C.CASES[name]
    D, A = C.build(name)
    assert D.shape == (c["nx"], c["na"]) and D.dtype == np.float64 and np.isfinite(D).all() and (D >= 0).all()
    assert 1 <= len(A) <= c["na"] and A.min() >= 0 and A.max() < c["nx"]
    r = C.reference(name)
    allp = c["nx"] * (c["nx"] - 1) // 2
    assert (r["n_pairs"] == allp) == (name in C.COMPLETE), (r["n_pairs"], allp)
    assert r["n_pairs"] > 0 and r["n_pairs"] == len(r["IJs"]) and r["min_row_len"] == np.diff(r["I_ptr"]).min()
    assert 0 < r["features"][:, 3].sum() and r["n_unc"] == len(r["IJs"]) - int(r["features"][:, 3].sum())
    if c["kind"] == "ties" and c["na"] >= 8:      # exact ties in every row, often for the nearest anchor itself
        s = np.sort(D, axis=1)
        assert (s[:, 1:] == s[:, :-1]).any(axis=1).all() and (s[:, 0] == s[:, 1]).mean() > 0.3
    if c["kind"] == "twins":
        assert any(b < c["na"] and np.array_equal(D[:, a], D[:, b]) for a, b in ((63, 64), (255, 256)))
    if c["kind"] == "metric":     # anchors at distance 0 from themselves, duplicated points: identical rows
        assert (D.min(axis=1) == 0).sum() >= min(c["na"], c["nx"])
        assert len(np.unique(D, axis=0)) < c["nx"] or c["nx"] < 20
    if c["akind"] == "repeat":
        assert len(set(A.tolist())) == len(A) - 1 and r["features"][:, 3].sum() > 0
    if c["akind"] == "all":       # pairs of two anchors are in the list
        isA = np.zeros(c["nx"], dtype=bool)
        isA[A] = True
        assert (isA[r["IJs"][:, 0]] & isA[r["IJs"][:, 1]]).any()
    if name == "n1030_a64_thin":
        assert r["n_pairs"] < 0.5 * allp


@pytest.mark.parametrize("name", list(C.QUERY_CASES))
def test_query_case_builds_and_is_what_it_says(name):
    c = C.QUERY_CASES[name]
    D, A = C.build_query(name)
    assert D.shape == (c["nx"], c["na"]) and np.isfinite(D).all() and (D >= 0).all() and A.max() < c["nxb"]
    r = C.query_reference(name)
    rows = np.diff(r["I_ptr"])
    assert (rows[:c["nxb"]] == 0).all() and r["min_row_len"] == rows[c["nxb"]:].min()
    assert all(rows[c["nxb"] + q] == 0 for q in c["zero"])     # (another query may find nothing by itself)
    assert (r["n_pairs"] == 0) == (len(c["zero"]) == c["nq"])
    assert np.array_equal(r["IJs"][:, 1] >= c["nxb"], np.ones(r["n_pairs"], dtype=bool))
    assert np.array_equal(r["I_idx"], np.arange(r["n_pairs"]))
    if r["n_pairs"] and c["nxb"] > 1:
        assert 0 < r["n_unc"] <= r["n_pairs"]


def test_query_table_has_an_empty_row_case_and_an_empty_list_case():
    refs = [C.query_reference(nm) for nm in C.QUERY_CASES]
    assert any(r["min_row_len"] == 0 and r["n_pairs"] > 0 for r in refs) and any(r["n_pairs"] == 0 for r in refs)


@pytest.mark.parametrize("name", [nm for nm in C.CASES if C.CASES[nm]["na"] <= 256 and C.CASES[nm]["locality"] <= C.CASES[nm]["na"]])
def test_mask_widths_agree(name):
    """The same table padded with far-away anchors to na = 65, 129 and 257: the 2- and 4-word masks and the wide representation
    describe the same sets, pairs and (where the padded table stays small) features."""
    c = C.CASES[name]
    r = C.reference(name)
    _, A = C.build(name)
    for na_to in (65, 129, 257):
        if na_to <= c["na"]:
            continue
        Dp = C.padded(name, na_to)
        sid, IJs, I_ptr, I_idx = O.locality_pairs(Dp, c["locality"], c["loc_thresh"], c["loc_min"])
        assert sid.max() < c["na"] and np.array_equal(C.onehot(sid, c["na"]), r["sid"])
        assert np.array_equal(IJs, r["IJs"]) and np.array_equal(I_ptr, r["I_ptr"]) and np.array_equal(I_idx, r["I_idx"])
        if len(IJs) * na_to <= 6_000_000:
            feats, ncm = O.features(IJs, Dp, A, I_ptr, I_idx)
            assert C.differences(C.pack(r["sid"], IJs, I_ptr, I_idx, feats, ncm), r) == []


# ------------------------------------------------------------------------------------------------------------- coverage
def _all_launches():
    seen = {}
    for form, env in C.FORMS.items():
        for nm, c in C.CASES.items():
            for k in C.dispatch(c, env, C.reference(nm)["n_pairs"]):
                seen.setdefault(k, []).append((form, nm))
        for nm, c in C.QUERY_CASES.items():
            for k in C.dispatch_query(c, env, C.query_reference(nm)["n_pairs"]):
                seen.setdefault(k, []).append((form, nm))
    return seen


def test_forms_set_only_the_library_switches():
    assert list(C.FORMS) == ["default", "large", "dense", "older"] and C.FORMS["default"] == {}
    for env in C.FORMS.values():
        assert set(env) <= set(C.FORM_VARIABLES)


def test_every_kernel_and_template_width_is_reached():
    seen = _all_launches()
    tagged = {C.base_name(k) for k in seen}
    missing = [k for k in C.KERNELS if k not in tagged]
    assert missing == []
    for nw in (1, 2, 4):
        for k in ("k_sid<%d>", "k_loc_thresh<%d>", "k_keep_bits<%d>", "k_keep_bits_cols<%d>", "k_qloc_count<%d>", "k_qloc_emit<%d>"):
            assert k % nw in seen, k % nw
    claimed = sorted({c["loc_thresh"] for c in C.CASES.values() if c["na"] <= 256 and 1 <= c["loc_thresh"] <= 8})
    assert claimed == [1, 2, 3, 5, 8]
    small = {k for k in seen if k.startswith("k_loc_thresh_small<")}
    assert {int(k.split("<")[1].split(",")[0]) for k in small} == set(claimed)
    assert {int(k.rstrip(">").split(",")[1]) for k in small} == {1, 2, 4}
    assert {"k_loc_thresh_small_wide<%d>" % t for t in (1, 2, 3, 8)} <= set(seen)
    assert {"k_keep_bits_wide_planes<%d>" % t for t in (1, 2, 3, 8)} <= set(seen)
    assert "k_keep_bits_wide<0>" in seen and any(("k_keep_bits_wide<%d>" % lc) in seen for lc in range(1, 9))
    assert len([k for k in seen if k.startswith("k_features_tiled<")]) >= 2
    # the forms are what reach the long-list kernels at these sizes, and only `older` runs k_emit_pairs for both halves
    assert {f for f, _ in seen["k_emit_pairs[rows_only=0]"]} == {"older"}
    assert {f for f, _ in seen["k_features_dense"]} == {"dense"} and "large" in {f for f, _ in seen["k_features_tiled<8>"]}
    assert ("default", "n31_a300_wide") in seen["k_features"] and ("default", "n1030_a257_wide") in seen["k_features_wide"]
    assert ("large", "n1030_a64_thin") in seen["k_emit_cols[super]"] and ("large", "n65_a64") in seen["k_keep_bits_cols<1>"]


# ---------------------------------------------------------------------------------------------------------- sensitivity
@pytest.mark.parametrize("name", BY_SIZE[:-6])
def test_restatement_equals_the_oracle(name):
    """variant() without a mistake is the oracle's state, field by field: the mutants below differ from it by their mistake only."""
    assert C.differences(C.variant(name), C.reference(name)) == []


@pytest.mark.parametrize("name", BY_SIZE[-6:])
def test_restatement_equals_the_oracle_on_the_large_cases(name):
    fields = ("sid", "IJs", "n_pairs", "I_ptr", "I_idx", "ncm", "min_row_len", "n_unc")
    assert C.differences(C.variant(name, fields=fields), C.reference(name), fields) == []


@pytest.mark.parametrize("mutant", list(C.MUTANTS))
def test_table_notices_the_mutant(mutant):
    field = C.MUTANTS[mutant]
    fields = ("sid", "IJs", "n_pairs") if field == "IJs" else C.FIELDS if field == "features" else ("IJs", "n_unc")
    caught = []
    for nm in BY_SIZE:
        v = C.variant(nm, mutant, fields=fields)
        if field in C.differences(v, C.reference(nm), (field,)):
            if field == "features":     # the dad column, on an unchanged list
                r = C.reference(nm)
                assert np.array_equal(v["IJs"], r["IJs"]) and np.array_equal(v["features"][:, [0, 1, 3]], r["features"][:, [0, 1, 3]])
            if field == "n_unc":
                assert np.array_equal(v["IJs"], C.reference(nm)["IJs"])
            caught.append(nm)
            break
    assert caught, "no case notices %s: the table is missing one" % mutant
