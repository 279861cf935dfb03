"""The constructed inputs of tests/model_cases.py and its exact least-squares reference, checked on the CPU: every case has the
partition populations, ranks, null vectors and edge coincidences it claims; exact_ols is right; and scipy's dgelsd -- the
reference's solver -- stays inside the coefficient bound the device test applies, which is what fixes the bound's constant."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import model_cases as M  # noqa: E402

EXACT_CASES = M.FULL_RANK_CASES + M.DEFICIENT_CASES + ("refusals",)


@functools.lru_cache(maxsize=None)
def case(name):
    return M.build(name)


def sample_parts(c, y=None):
    """(sample rows [m][3], y [m], regression partition of every sample)."""
    X = c.features[c.pos, :3]
    y = M.host_distances(c.cls)[c.pos] if y is None else y
    return X, y, M.reg_bin(X[:, 2], c.edges)


@functools.lru_cache(maxsize=None)
def ref(name, b):
    c = case(name)
    X, y, part = sample_parts(c)
    rank = c.ref_rank.get(b, c.rank[b])
    return M.reference(X[part == b], y[part == b], rank)


def exact_partitions(name):
    c = case(name)
    return [b for b in range(c.nb) if c.rank[b] is not None and c.rows[b] <= M.EXACT_MAX_ROWS]


# ------------------------------------------------------------------------------------------------------------ the fixtures
@pytest.mark.parametrize("cls", sorted(M.CLASSES))
def test_fixture_points_give_exact_distances(cls):
    P, IJ, Y = M.points(cls), M.pairs(cls), M.host_distances(cls)
    assert P.shape == (M.CLASSES[cls], 2) and np.array_equal(P * 2, np.round(P * 2))
    n = IJ.shape[0]
    assert n == M.CLASSES[cls] * (M.CLASSES[cls] - 1) // 2 and n % 1024 != 0      # PM_U * 256 pairs per workgroup
    line, zero, rest = M._pair_sets(cls)
    assert len(zero) >= 1 and np.all(Y[zero] == 0.0) and np.all(Y[rest] > 0.0)
    assert len(line) + len(zero) + len(rest) == n
    if cls == "short":
        assert len(line) == M.N_LINE * (M.N_LINE - 1) // 2
        assert np.array_equal(Y[line] * 2, np.round(Y[line] * 2)) and np.all(Y[line] > 0)
        assert len(np.unique(Y[line])) < len(line) // 10          # massive ties
    else:
        assert len(np.unique(Y)) < n // 100                       # a lattice: few distinct distances


# ------------------------------------------------------------------------------------------------------------ the cases' claims
@pytest.mark.parametrize("name", M.ALL_CASES)
def test_case_has_the_structure_it_claims(name):
    c = case(name)
    n = M.pairs(c.cls).shape[0]
    assert c.features.shape == (n, 4) and np.isfinite(c.features).all() and not c.features[:, 3].any()
    assert c.pos.dtype == np.int64 and len(np.unique(c.pos)) == c.m and c.pos.min() >= 0 and c.pos.max() < n
    assert (c.order == "shuffled") == (not np.array_equal(c.pos, np.sort(c.pos)))
    assert 1 <= c.nb <= M.MAXBINS and np.all(np.diff(c.edges) > 0)
    X, y, part = sample_parts(c)
    d = X[:, 2]
    # populations, by exact comparisons on the edges
    assert [int(((d > c.edges[b]) & (d <= c.edges[b + 1])).sum()) for b in range(c.nb)] == list(c.rows)
    assert [int(((d >= c.edges[b]) & (d <= c.edges[b + 1])).sum()) for b in range(c.nb)] == list(c.err_rows)
    assert list(c.status) == [2 if r < 3 else 0 for r in c.rows]
    assert c.flags == (0, 2 if min(c.rows) < 3 else 0, 2 if max(c.err_rows) > M.ERR_CAP else 1 if min(c.err_rows) == 0 else 0)
    # ranks and null vectors, by the singular values of the (exactly) centred partition
    for b in exact_partitions(name):
        Xc = M.centred_exact(X[part == b], y[part == b])[0]
        s = np.linalg.svd(Xc, compute_uv=False)
        r = c.rank[b]
        if r > 0:
            assert s[r - 1] > 3 * M.OLS_RCOND * s[0], (name, b, s)
        if r < 3:
            assert s[r] <= 1e-14 * max(s[0], np.abs(X[part == b]).max()), (name, b, s)
        nulls = c.null.get(b, [])
        assert len(nulls) == 3 - r
        if nulls:
            V = np.stack(nulls)
            assert np.linalg.matrix_rank(V) == len(nulls)
            assert np.abs(Xc @ V.T).max() <= 1e-14 * max(s[0], np.abs(X[part == b]).max()) * np.linalg.norm(V, axis=1).max()
        # which branch of k_ols_bins the partition takes: the diagonal of an unpivoted Householder R against the kernel's line,
        # a factor 3 away from it on either side so that no rounding moves it across
        R = np.abs(np.diag(np.linalg.qr(Xc, mode="r")))
        if c.qr_deficient.get(b, False):
            assert R.min() <= M.QR_LINE / 3 * R.max(), (name, b, R)
        else:
            assert R.min() > 3 * M.QR_LINE * R.max(), (name, b, R)
    # the background: pairs on every finite edge, inside every partition and outside all of them where there is an outside
    bd = np.delete(c.features[:, 2], c.pos)
    for e in c.edges[np.isfinite(c.edges)]:
        assert (bd == e).sum() >= 3
    bb = M.reg_bin(bd, c.edges)
    assert set(bb[bb >= 0]) == set(range(c.nb))
    if np.isfinite(c.edges[0]):
        assert (bd < c.edges[0]).any() and (bd > c.edges[-1]).any() and (bb < 0).any()


def test_what_the_single_cases_were_built_for():
    for name in M.SHORT_CASES:
        assert case(name).m % 256 != 0
    assert case("full_n257").rows[0] == 257 and case("full_n300").rows[0] == 300 and case("full_n4").rows[0] == 4
    assert case("n3").rows[0] == 3 and case("dup_rows").rows[0] == 6
    X, y, part = sample_parts(case("dup_rows"))
    assert len(np.unique(X[part == 0], axis=0)) == 2
    assert case("nb1").nb == 1 and np.array_equal(case("nb1").edges, [-np.inf, np.inf])
    assert case("nb64").nb == M.MAXBINS
    X, y, part = sample_parts(case("ub_2dad"))
    assert np.array_equal(X[part == 0, 1], 2.0 * X[part == 0, 2])
    X, y, part = sample_parts(case("lb_zero"))
    assert not X[part == 0, 0].any() and X[part == 1, 0].any()
    c = case("half_integer")
    X, y, part = sample_parts(c)
    assert np.array_equal(X[part == 0] * 2, np.round(X[part == 0] * 2)) and np.array_equal(y[part == 0] * 2, np.round(y[part == 0] * 2))
    c = case("offset_1e6")
    X, y, part = sample_parts(c)
    assert X[part == 0].min() > 999990 and np.ptp(X[part == 0], axis=0).max() < 20
    # condition numbers of the nearly dependent cases
    for name, lo, hi in (("near_dep_1e-6", 3e5, 3e6), ("near_dep_1e-9", 3e8, 3e9), ("near_dep_1e-11", 3e10, 3e11)):
        assert lo < ref(name, 0).kappa < hi, (name, ref(name, 0).kappa)
        assert ref(name, 0).kappa * ref(name, 0).rho < 1e-3       # the targets lie on a plane: the bound is u kappa
    # edges
    c = case("inner_edge")
    X, y, part = sample_parts(c)
    on = X[:, 2] == c.edges[1]
    assert on.sum() == 3 and np.all(part[on] == 0) and sum(c.err_rows) == c.m + 3
    c = case("lowest_edge")
    X, y, part = sample_parts(c)
    on = X[:, 2] == c.edges[0]
    assert on.sum() == 2 and np.all(part[on] == -1) and np.all(M.err_bin(X[on, 2], c.edges) == 0) and (y[on] == 0).sum() == 1
    assert (X[:, 2] == c.edges[-1]).sum() == 1 and part[X[:, 2] == c.edges[-1]][0] == 1
    c = case("finite_outer")
    X, y, part = sample_parts(c)
    assert (X[:, 2] < c.edges[0]).sum() == 3 and (X[:, 2] > c.edges[-1]).sum() == 3 and (part < 0).sum() == 6
    assert np.all(M.err_bin(X[part < 0, 2], c.edges) == M.NO_LABEL)
    # the sorter
    assert case("sort_8192").err_rows[0] == M.ERR_CAP == 1 << 13 and case("sort_8193").err_rows[0] == M.ERR_CAP + 1
    k = case("sort_5000").err_rows[0]
    assert k == 5000 and k & (k - 1) != 0
    c = case("sort_ties")
    X, y, part = sample_parts(c)
    rows0 = np.c_[X[part == 0], y[part == 0]]
    _, cnt = np.unique(rows0, axis=0, return_counts=True)
    assert cnt.max() >= 30 and (cnt > 1).sum() >= 20                 # groups of identical (row, target): tied residuals
    on = X[:, 2] == c.edges[0]
    assert on.sum() == 5 and (y[on] == 0).sum() == 1 and np.all(part[on] == -1)


def test_cases_tell_the_interval_conventions_apart():
    """The restatements with one comparison changed -- `>=` for `>` in the regression partition, an open interval in the
    residual lists -- give other results on the edge cases: the inputs can see these mistakes."""
    for name in ("inner_edge", "lowest_edge"):
        c = case(name)
        W, cc = np.arange(1.0, 3 * c.nb + 1).reshape(c.nb, 3) / 7, np.arange(1.0, c.nb + 1)
        assert not np.array_equal(M.predict(c.features, c.edges, W, cc), M.predict(c.features, c.edges, W, cc, closed_lo=True))
        sp = M.predict(c.features, c.edges, W, cc)[c.pos]
        assert not np.array_equal(sp, M.predict(c.features, c.edges, W, cc, closed_lo=True)[c.pos])
        X, y, _ = sample_parts(c)
        a, b = M.residual_lists(X[:, 2], y, sp, c.edges), M.residual_lists(X[:, 2], y, sp, c.edges, open_=True)
        assert not np.array_equal(a[0], b[0])
        assert not np.array_equal(M.err_bin(c.features[:, 2], c.edges), M.err_bin(c.features[:, 2], c.edges, open_=True))


def test_clip_binds_on_both_sides():
    c = case("full_n300")
    W = np.stack([ref("full_n300", b).w for b in range(2)])
    cc = np.array([ref("full_n300", b).c for b in range(2)])
    pred = M.predict(c.features, c.edges, W, cc)
    lo, hi = pred < c.features[:, 0], pred > c.features[:, 1]
    assert lo.sum() >= 10 and hi.sum() >= 10 and (~lo & ~hi).sum() >= 10


# ------------------------------------------------------------------------------------------------------------ exact_ols
def test_exact_ols_reproduces_a_hand_computed_answer():
    import mpmath as mp
    # four rows, y = 3 + 1 lb - 2 ub + 0.5 dad on them: four equations, four unknowns, the rows affinely independent
    # (det [[1, -1, 1], [-1, -1, 2], [0, -2, 1]] = 4, the rows minus the first), so the fit interpolates
    X = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 1.0], [0.0, 1.0, 2.0], [1.0, 0.0, 1.0]])
    y = np.array([0.0, 3.5, 2.0, 4.5])
    assert np.array_equal(3 + X @ np.array([1.0, -2.0, 0.5]), y)
    w, c = M.exact_ols(X, y)
    with mp.workdps(60):
        assert max(abs(w[0] - 1), abs(w[1] + 2), abs(w[2] - mp.mpf("0.5")), abs(c - 3)) < mp.mpf(10) ** -50
    # and one with a residual: rows (0,0,0), (1,0,0), (0,1,0), (0,0,1), (1,1,1), y = (0, 1, 1, 1, 0).  By symmetry w_k = a; a centred
    # column is (-.4, .6, -.4, -.4, .6) up to the order of its entries, so x.x = 1.2, x.x' = 0.2 (k != k'), and with
    # yc = (-.6, .4, .4, .4, -.6), x.yc = -0.2: 1.6 a = -0.2, a = -1/8; c = mean_y - 3 a mean_x = 0.6 + 3/8 * 0.4 = 3/4
    X = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]])
    y = np.array([0.0, 1, 1, 1, 0])
    w, c = M.exact_ols(X, y)
    with mp.workdps(60):
        assert max(abs(w[k] + mp.mpf(1) / 8) for k in range(3)) < mp.mpf(10) ** -50 and abs(c - mp.mpf(3) / 4) < mp.mpf(10) ** -50


@pytest.mark.parametrize("name", EXACT_CASES)
def test_exact_ols_satisfies_the_normal_equations(name):
    import mpmath as mp
    c = case(name)
    X, y, part = sample_parts(c)
    for b in exact_partitions(name):
        Xb, yb = X[part == b], y[part == b]
        rank = c.ref_rank.get(b, c.rank[b])
        w, cc = M.exact_ols(Xb, yb, rank)
        with mp.workdps(60):
            n = len(yb)
            mx = [sum(mp.mpf(float(v)) for v in Xb[:, k]) / n for k in range(3)]
            r = [mp.mpf(float(yb[i])) - cc - sum(mp.mpf(float(Xb[i, k])) * w[k] for k in range(3)) for i in range(n)]
            scale = max(float(np.abs(Xb).max()), 1.0) * max(float(np.abs(yb).max()), 1.0) * n
            assert abs(sum(r)) <= mp.mpf(10) ** -40 * scale               # the intercept's equation
            for k in range(3):
                g = sum((mp.mpf(float(Xb[i, k])) - mx[k]) * r[i] for i in range(n))
                assert abs(g) <= mp.mpf(10) ** -40 * scale, (name, b, k, g)


@pytest.mark.parametrize("name", M.DEFICIENT_CASES)
def test_minimum_norm_answers_are_orthogonal_to_the_null_vectors(name):
    c = case(name)
    R = ref(name, 0)
    assert R.rank == c.rank[0] < 3
    for v in c.null[0]:
        assert abs(R.w @ v) <= 8 * M.U * np.linalg.norm(R.w) * np.linalg.norm(v)
    if c.rank[0] == 0:
        X, y, part = sample_parts(c)
        assert not R.w.any() and R.c == pytest.approx(y[part == 0].mean(), rel=1e-15)


def test_three_rows_interpolate():
    c = case("n3")
    X, y, part = sample_parts(c)
    R = ref("n3", 0)
    assert np.abs(R.pred - y[part == 0]).max() <= 2 * M.U * np.abs(y[part == 0]).max()
    assert R.rho < 1e-30


# ------------------------------------------------------------------------------------------------------------ gamma
def dgelsd_ratios():
    """{(case, partition): ||w_dgelsd - w|| / (u kappa (1 + kappa rho) ||w||)} over the full-rank partitions of the full-rank cases."""
    out = {}
    for name in M.FULL_RANK_CASES:
        c = case(name)
        X, y, part = sample_parts(c)
        for b in exact_partitions(name):
            R = ref(name, b)
            w, _ = M.dgelsd(X[part == b], y[part == b])
            out[(name, b)] = float(np.linalg.norm(w - R.w) / (M.U * R.unit * np.linalg.norm(R.w)))
    return out


def test_dgelsd_stays_inside_the_bound_and_fixes_gamma(capsys):
    """The reference's own solver against the exact answer, in units of the first-order bound u kappa (1 + kappa rho) ||w||.
    GAMMA is 8 x the largest ratio it attains here and not less than 1 (QR and the SVD solver are both backward stable with
    different modest constants, and the device's tree sums differ from a sequential sum).  Measured with scipy 1.15 / OpenBLAS:
    27.5 (the seven-row filler partition of full_n4) and 13.6 (full_n300), every other partition 0.08 .. 1.7."""
    ratios = dgelsd_ratios()
    worst = max(ratios, key=ratios.get)
    with capsys.disabled():
        for name in M.FULL_RANK_CASES:
            print("\n  dgelsd ratio %-16s %.3f" % (name, max(v for (k, b), v in ratios.items() if k == name)), end="")
        print("\n  largest: %s %.3f; GAMMA = %g" % (worst, ratios[worst], M.GAMMA))
    for key, v in ratios.items():
        assert v <= M.GAMMA, (key, v)
        c = case(key[0])
        X, y, part = sample_parts(c)
        R = ref(*key)
        w, cc = M.dgelsd(X[part == key[1]], y[part == key[1]])
        assert abs(cc - R.c) <= R.tol_c(), (key, cc - R.c, R.tol_c())
    assert M.GAMMA >= 1.0
