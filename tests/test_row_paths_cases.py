"""Which way each adversarial row of tests/row_paths_cases.py goes through the row selections, asserted on the CPU from the
restated sampling rule of csrc/rowsel.h.  A condition on the test INPUTS (they reach the branches they were built for), not a
check of the kernels: that is tests/test_row_paths_gpu.py."""
import numpy as np
import pytest

import row_paths_cases as C

AB = {"too_many": "M", "too_few": "F", "fast": "f", "shrink_short": "S"}
N_NEIGHBORS, NMIN, NN = 20, 30, 21   # the three parametrisations: want = n_neighbors + 1, L = nmin + 1, want = nn - 1

# One letter per target row (C.target_rows order), for (k_row_thresh, k_gn_lists, k_get_nn) on the all-not-computed mask.
# Row 0 owns all of its pairs; later target rows hold up to seven values of earlier ones (the shared pairs), which is what
# moves rows 2.. of the 1300-entry shrink_too_tight layout back to "fast" (a foreign value shifts the buffer positions).
EXPECTED = {
    ("long", "sample_sees_large"): ("MMMMMMMM", "MMMMMMMM", "MMMMMMMM"),
    ("long", "sample_sees_small"): ("FFFFFFFF", "FFFFFFFF", "FFFFFFFF"),
    ("long", "ties_on_cut"): ("ffMffMff", "ffMffMff", "ffMffMff"),
    ("long", "all_equal"): ("MMMMMMMM", "MMMMMMMM", "MMMMMMMM"),
    ("long", "integer_halves"): ("ffffffff", "ffffffff", "ffffffff"),
    ("long", "narrow_ulps"): ("ffffffff", "ffffffff", "ffffffff"),
    ("long", "with_marks"): ("ffffffff", "ffffffff", "MMMMMMMM"),   # graph: -1 + row maximum (inf) = inf on every entry
    ("long", "sorted_ascending"): ("ffffffff", "ffffffff", "ffffffff"),
    ("long", "sorted_descending"): ("ffffffff", "ffffffff", "ffffffff"),
    ("long", "shrink_too_tight"): ("SSffffff", "SSffffff", "SSffffff"),
    ("mid", "shrink_too_tight"): ("SSSSSSSS", "SSSSSSSS", "SSSSSSSS"),
}
ALL_FAST = ("ffffffff", "ffffffff", "ffffffff")   # rows of at most ROWC_CAP entries never sample; of at most 128 never shrink


@pytest.fixture(scope="module")
def index():
    return {cls: C.complete_index(nx) for cls, nx in C.CLASSES.items()}


def _letters(index, cls, case):
    ptr, idx, IJs = index[cls]
    rows = C.target_rows(C.CLASSES[cls])
    RA, ncm = C.build_case(ptr, idx, IJs, cls, case, want=N_NEIGHBORS + 1)
    th = "".join(AB[C.thresh_branch(RA, ncm, ptr, idx, i, N_NEIGHBORS)] for i in rows)
    RA, ncm = C.build_case(ptr, idx, IJs, cls, case, want=NMIN + 1)
    gn = "".join(AB[C.gn_branch(RA, ncm, ptr, idx, i, NMIN)] for i in rows)
    RA, ncm = C.build_case(ptr, idx, IJs, cls, case, want=NN - 1)
    gr = "".join(AB[C.graph_branch(RA, ncm, ptr, idx, i, NN)[1]] for i in rows)
    return th, gn, gr


def test_classes_and_targets():
    for cls, nx in C.CLASSES.items():
        assert nx % 8 != 0
        rows = C.target_rows(nx)
        assert len(set(rows)) == len(rows) == 8 and {0, nx // 2, nx - 1} <= set(rows)
        assert sum(1 for a in rows for b in rows if b == a + 1) >= 2      # adjacent target rows
    assert C.CLASSES["long"] - 1 > C.ROWC_CAP >= C.CLASSES["mid"] - 1 > C.SHRINK_MIN >= C.CLASSES["short"] - 1


def test_sample_sees_small_is_reachable():
    """Exactly r + 1 entries reach t0, so the case needs ceil(3 want 256 / len) + 4 < want: at 1300 entries that holds for every
    want from 16 on and not for 11, so the tests select 21, 31 and 20 smallest, never n_neighbors = 10."""
    n = C.CLASSES["long"] - 1
    assert all(C.first_rank(w, n) + 1 < w for w in range(16, 64)) and not C.first_rank(11, n) + 1 < 11
    for want in (N_NEIGHBORS + 1, NMIN + 1, NN - 1):
        assert C.first_rank(want, n) + 1 < want


@pytest.mark.parametrize("case", C.CASES)
@pytest.mark.parametrize("cls", list(C.CLASSES))
def test_branch_of_every_target_row(index, cls, case):
    assert _letters(index, cls, case) == EXPECTED.get((cls, case), ALL_FAST)


def test_every_branch_is_reached_in_every_kernel(index):
    seen = [set(), set(), set()]
    for cls in C.CLASSES:
        for case in C.CASES:
            for k, s in enumerate(_letters(index, cls, case)):
                seen[k] |= set(s)
    for k, name in enumerate(("k_row_thresh", "k_gn_lists", "k_get_nn")):
        assert seen[k] == set("MFfS"), name


def test_graph_passes_and_mask_plans(index):
    """The row_counts mask gives target rows exactly nmin - 1, nmin and 0 computed entries and one row fewer not-computed
    entries than L; the graph's first pass (computed entries alone) decides rows with nn - 1 computed entries, the second the rest."""
    for cls, nx in C.CLASSES.items():
        ptr, idx, IJs = index[cls]
        RA, ncm = C.build_case(ptr, idx, IJs, cls, "sorted_ascending", want=NN - 1, mask="row_counts", nmin=NMIN)
        plan = C.row_count_plan(nx, NMIN)
        for i, cnt in plan.items():
            u = ncm[idx[ptr[i]:ptr[i + 1]]].astype(bool)
            if cnt < 0:
                assert int(u.sum()) == NMIN - 1 < NMIN + 1
            else:
                assert int((~u).sum()) == cnt
            assert C.graph_branch(RA, ncm, ptr, idx, i, NN)[0] == (0 if int((~u).sum()) >= NN - 1 else 1)
        assert C.gn_branch(RA, ncm, ptr, idx, C.target_rows(nx)[3], NMIN) in C.BRANCHES
        r70 = C.build_case(ptr, idx, IJs, cls, "sorted_ascending", mask="random70")[1]
        assert 0.6 < r70.mean() < 0.8


def test_shrink_min_16_reaches_the_short_rows(index):
    """ANNCHOR_ROWC_SHRINK_MIN=16 (the worker's third setting) lets the 96-entry rows take the second cut as well.  It can drop
    candidates there but never too many: r2 + 1 = ceil(192 want / c) + 3 >= want for every c <= 192."""
    ptr, idx, IJs = index["short"]
    RA, ncm = C.build_case(ptr, idx, IJs, "short", "shrink_too_tight", want=N_NEIGHBORS + 1)
    i = C.target_rows(C.CLASSES["short"])[0]
    keys = C.key_asc(RA[idx[ptr[i]:ptr[i + 1]]])
    assert C.shrink_cut(keys, N_NEIGHBORS + 1) == keys.size                       # default: no second cut
    assert N_NEIGHBORS + 1 <= C.shrink_cut(keys, N_NEIGHBORS + 1, shrink_min=16) < keys.size
    assert all(C.shrink_rank(w, c) + 1 >= w for c in range(17, 193) for w in range(1, c + 1))


def test_restated_keys_order_like_floats():
    v = np.array([-np.inf, -1.0, -0.0, 0.0, 5e-324, 1.5, np.inf])
    k = C.key_asc(v)
    assert (np.diff(k.astype(object)) >= 0).all() and k[2] == k[3] and k[1] < k[2] < k[4]
