"""The nearest-enemy checker of enemy_cases.py proves on the CPU that it bites before any kernel is held to it: the float64
brute force and the reference's own arithmetic (float32 differences) pass on every data family under every label scheme,
every planted defect is reported, and the uncentred expanded form in float32 is caught on the ill-conditioned families."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import enemy_cases as ec   # noqa: E402
import streamed_cases as sc   # noqa: E402

N, NROWS = 1500, 100
DIMS = [(20, 32), (128, 128)]   # (dimension, the dimp gamma is taken at)
NNS = (3, 31)
CASES = [(f, s) for f in sorted(sc.FAMILIES) for s in sorted(ec.SCHEMES)]


def _rows():
    return np.sort(np.random.default_rng(9).choice(N, NROWS, replace=False))


@pytest.mark.parametrize("scheme", sorted(ec.SCHEMES))
def test_schemes_are_seeded_and_shaped(scheme):
    X = sc.family("plain", 1777, 20)
    for nn in (3, 40):
        y = ec.labels(scheme, X, nn)
        assert np.array_equal(y, ec.labels(scheme, X, nn))
        cnt = np.unique(y, return_counts=True)[1]
        if scheme == "seven_uneven":
            assert len(cnt) == 7 and {nn, 128, 129} <= set(cnt.tolist())
        if scheme == "many":
            assert len(cnt) == 1777 // 128 and np.sum((cnt + 127) // 128 * 128) <= 2 * 1777
        if scheme == "two_random":
            assert len(cnt) == 2 and abs(int(cnt[0]) - int(cnt[1])) <= 1
    assert len(np.unique(ec.labels("by_half_space", sc.family("duplicates_all", 300, 20), 3))) == 2


@pytest.mark.parametrize("name,scheme", CASES)
def test_float64_brute_force_passes(name, scheme):
    rows = _rows()
    for d, dimp in DIMS:
        X = sc.family(name, N, d)
        for nn in NNS:
            y = ec.labels(scheme, X, nn)
            idx, dist = ec.brute_enemies_f64(X, y, rows, nn)
            assert ec.enemy_violations(X, y, rows, idx, dist, nn, sc.gamma_of(dimp)) == []


@pytest.mark.parametrize("name,scheme", CASES)
def test_float32_difference_selection_stays_within_the_margin(name, scheme):
    """The reference's arithmetic alone stays within 3 gamma on every family and scheme: a case that failed here would be
    wrong, not the kernels.  (Run on every family x scheme at d = 20 and 128, nn = 3 and 31: all pass, the checker's
    statement stands as written.)"""
    rows = _rows()
    for d, dimp in DIMS:
        X = sc.family(name, N, d)
        D = sc.select_f32_differences(X, rows)
        for nn in NNS:
            y = ec.labels(scheme, X, nn)
            idx, dist = ec.enemies_selected_by(D, X, y, rows, nn)
            assert ec.enemy_violations(X, y, rows, idx, dist, nn, sc.gamma_of(dimp)) == []


@pytest.mark.parametrize("d,dimp", DIMS)
@pytest.mark.parametrize("name", sorted(sc.FAMILIES))
def test_uncentred_expanded_form_is_caught_where_it_is_wrong(name, d, dimp):
    """|x|^2 + |y|^2 - 2 x.y in float32 on the uncentred rows, masked by label: caught (rows are reported, and only for
    what was left out) on every ill-conditioned family under interleaved labels; how many rows, and what it reports elsewhere,
    is printed, not asserted (short lists of nn = 3 go wrong on fewer rows than the k-NN lists of 14 and 40 do)."""
    X = sc.family(name, N, d)
    rows = _rows()
    D = sc.select_f32_expanded(X, rows)
    for nn in NNS:
        y = ec.labels("two_random", X, nn)
        idx, dist = ec.enemies_selected_by(D, X, y, rows, nn)
        bad = ec.enemy_violations(X, y, rows, idx, dist, nn, sc.gamma_of(dimp))
        print("%s d=%d nn=%d: %d of %d rows reported" % (name, d, nn, len(bad), len(rows)))
        if name in sc.ILL_CONDITIONED:
            assert len(bad) >= 1, (name, d, nn)
            assert all("left out" in b[1] for b in bad)   # the pairs it lists are real enemies: only the selection is wrong


def test_planted_defects_are_reported():
    X = sc.family("plain", N, 20)
    rows, nn, g = _rows(), 5, sc.gamma_of(32)
    y = ec.labels("two_random", X, nn)
    idx, dist = ec.brute_enemies_f64(X, y, rows, nn + 1)
    good_i, good_d = idx[:, :nn].copy(), dist[:, :nn].copy()
    assert ec.enemy_violations(X, y, rows, good_i, good_d, nn, g) == []
    # a same-label entry: the row's nearest FRIEND in place of its second enemy (closer than what it replaces or not: refused)
    ki, _ = sc.brute_f64(X, rows, 30)
    friend = np.array([next(j for j in ki[t, 1:] if y[j] == y[r]) for t, r in enumerate(rows)])
    bi = good_i.copy()
    bi[:, 1] = friend
    bi, bd = ec._ascending(X, rows, bi)
    bad = ec.enemy_violations(X, y, rows, bi, bd, nn, g)
    assert len(bad) == len(rows) and all("own label" in b[1] for b in bad)
    # a closer enemy left out: a listed entry swapped for the (nn+1)-th: reported wherever the gap exceeds the margin, and only there
    for e in (0, nn - 1):
        si = good_i.copy()
        si[:, e] = idx[:, nn]
        si, sd = ec._ascending(X, rows, si)
        bad = {b[0] for b in ec.enemy_violations(X, y, rows, si, sd, nn, g)}
        gap = (dist[:, e] ** 2) < (1 - 3 * g) * dist[:, nn] ** 2
        assert bad == set(rows[gap].tolist()) and gap.sum() > len(rows) // 2
    assert all("left out" in b[1] for b in ec.enemy_violations(X, y, rows, si, sd, nn, g))
    # a duplicated index, an index out of range, a wrong distance, lines that do not ascend, an unfilled entry
    for kind, edit in [("twice", lambda i, d: i.__setitem__((slice(None), 3), i[:, 2])),
                       ("out of range", lambda i, d: i.__setitem__((slice(None), 3), N)),
                       ("out of range", lambda i, d: i.__setitem__((slice(None), nn - 1), -1)),
                       ("not that of the listed pair", lambda i, d: d.__setitem__((slice(None), 3), d[:, 3] * (1 + 3e-5))),
                       ("not ascending", lambda i, d: d.__setitem__((slice(None), 3), d[:, 4] * (1 + 2e-6))),
                       ("not ascending", lambda i, d: d.__setitem__((slice(None), nn - 1), np.inf))]:
        bi, bd = good_i.copy(), good_d.copy()
        edit(bi, bd)
        bad = ec.enemy_violations(X, y, rows, bi, bd, nn, g)
        assert len(bad) == len(rows) and all(kind in b[1] for b in bad), (kind, bad[:2])
    # a budgeted run's lines: the listed pairs are checked (label included), completeness is not
    assert ec.enemy_violations(X, y, rows, si, sd, nn, g, complete=False) == []
    assert len(ec.enemy_violations(X, y, rows, bi * 0 + friend[:, None], bd, nn, g, complete=False)) == len(rows)


def test_swap_inside_an_exact_tie_is_not_reported():
    X = sc.family("lattice", N, 20)
    rows, nn, g = _rows(), 14, sc.gamma_of(32)
    y = ec.labels("two_random", X, nn)
    idx, dist = ec.brute_enemies_f64(X, y, rows, nn + 1)
    tie = dist[:, nn - 1] == dist[:, nn]
    assert tie.sum() > len(rows) // 2
    si, sd = idx[:, :nn].copy(), dist[:, :nn].copy()
    si[:, nn - 1], sd[:, nn - 1] = idx[:, nn], dist[:, nn]
    bad = {b[0] for b in ec.enemy_violations(X, y, rows, si, sd, nn, g)}
    assert bad == set(rows[~tie].tolist())


def test_cosine_brute_force_agrees_with_the_euclidean_one_on_unit_rows():
    X = sc.family("plain", 600, 20)
    y = ec.labels("two_random", X, 3)
    rows = np.arange(0, 600, 7)
    ci, cd = ec.brute_cosine_enemies_f64(X, y, rows, 3)
    U = (X.astype(np.float64) / np.linalg.norm(X.astype(np.float64), axis=1)[:, None])
    D = ((U[None, :, :] - U[rows][:, None, :]) ** 2).sum(-1)
    D[y[rows][:, None] == y[None, :]] = np.inf
    assert np.array_equal(ci, np.argsort(D, axis=1, kind="stable")[:, :3])
    assert np.allclose(cd, np.take_along_axis(D, ci, 1) / 2.0, rtol=1e-9, atol=1e-12)
