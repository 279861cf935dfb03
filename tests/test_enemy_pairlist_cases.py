"""Host-side checks of tests/enemy_pairlist_cases.py: the staged reference ends where oracle.annchor_oracle.nearest_enemies
ends, every case reaches the edges it is listed for, the cases reach every kernel and template width of csrc/enemies.hip
through the dispatch mirror, and every deliberately wrong reference is noticed by at least one case.  Statements about the
INPUTS of tests/test_enemy_pairlist_gpu.py; no GPU here."""
import numpy as np
import pytest

import enemy_pairlist_cases as P

BY_SIZE = sorted(P.CASES, key=lambda nm: (P.fitted(P.CASES[nm]["base"]).nx, nm))


def test_table_holds_the_shapes_it_promises():
    shapes = {(P.fitted(c["base"]).nx, P.fitted(c["base"]).na) for c in P.CASES.values()}
    nxs, nas = {s[0] for s in shapes}, {s[1] for s in shapes}
    assert {63, 64, 65, 129, 257, 1030} <= nxs and max(nxs) == 1030
    assert {7, 64, 65, 128, 129, 256, 257, 300} <= nas
    assert {(65, 300), (257, 257), (1030, 300)} <= shapes                     # wide sets at a partial last bitmap word
    wide_L = {min(P.fitted(c["base"]).locality, P.fitted(c["base"]).na) for c in P.CASES.values() if P.sid_wide(P.fitted(c["base"]).na)}
    assert {4, 12} <= wide_L
    assert {c["nn"] for c in P.CASES.values()} >= {1, 3, 16}
    assert {1, 50} <= {P.build(nm).first for nm in P.CASES}
    claimed = {t for c in P.CASES.values() for t in c["edges"]}
    assert claimed == set(P.EDGES), set(P.EDGES) - claimed                   # every edge has a case that is checked for it
    twins = [(a, b) for a in P.CASES for b in P.CASES if P.CASES[b]["by_vector"] and not P.CASES[a]["by_vector"]
             and all(P.CASES[a][k] == P.CASES[b][k] for k in ("base", "labels", "loc_min", "first", "nn", "model"))]
    assert twins, "no case runs once through the model and once through pred="


@pytest.mark.parametrize("name", BY_SIZE)
def test_staged_reference_ends_where_the_oracle_ends(name):
    st, r = P.build(name), P.stages(name)
    o, ngi, ngd = P.oracle_end_state(name)
    f = st.fit
    n0 = len(f.IJs)
    assert np.array_equal(o.IJs, np.vstack([f.IJs, r["IJn"]]))
    assert np.array_equal(o.features, np.vstack([f.feats, r["feats_n"]]))
    assert np.array_equal(o.RA, np.concatenate([r["RA_f1"], r["RA_n1"]]))
    assert np.array_equal(o.ncm, np.concatenate([r["ncm_f1"], r["ncm_n1"]]))
    assert np.array_equal(o.I_ptr, f.I_ptr + r["ptr_n"])
    assert np.array_equal(o.I_idx, np.concatenate(r["rows"]))
    assert np.array_equal(ngi, r["ngi"]) and np.array_equal(ngd, r["ngd"])
    # the clipped prediction of the pairs nobody evaluated is still in place
    assert np.array_equal(o.RA[n0:][r["ncm_n1"]], r["RA_n0"][r["ncm_n1"]])


@pytest.mark.parametrize("name", BY_SIZE)
def test_case_reaches_its_edges(name):
    P.check_case(name)


def test_every_kernel_and_template_width_is_reached():
    seen = {k: [] for k in P.KERNELS}
    for nm in P.CASES:
        for k in P.dispatch(nm):
            seen[k].append(nm)
    for k in P.KERNELS:
        print("%-32s %s" % (k, " ".join(seen[k])))
    assert [k for k in P.KERNELS if not seen[k]] == []
    assert set(seen) == set(P.KERNELS)
    # the empty new list skips the emit, feature, prediction and pack launches
    empty = [nm for nm in P.CASES if len(P.stages(nm)["IJn"]) == 0]
    assert empty and all("k_emit_pairs" not in P.dispatch(nm) and "k_en_predict" not in P.dispatch(nm) for nm in empty)


@pytest.mark.parametrize("mutant", list(P.MUTANTS))
def test_table_notices_the_mutant(mutant):
    field = P.MUTANTS[mutant]
    caught = None
    for nm in BY_SIZE:
        v = P.stages(nm, mutant, P.STAGE_OF[field])[field]
        w = P.stages(nm)[field]
        if v.shape != w.shape or not np.array_equal(v, w):
            caught = nm
            break
    print("%s: first noticed by %s in %s" % (mutant, caught, field))
    assert caught, "no case notices %s: the table is missing one" % mutant


def test_unmutated_stages_do_not_depend_on_where_they_stop():
    nm = BY_SIZE[0]
    full = P.stages(nm)
    for upto in ("candidates", "predict", "first"):
        part = P.stages_of(P.build(nm), None, upto)
        assert all(np.array_equal(part[k], full[k]) for k in part if k in P.FIELDS)
