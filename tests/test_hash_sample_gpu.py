"""The hashed stratified choice on the device -- k_hs_collect, k_hs_finish, k_hs_check and the host loop of
hash_sample_device (csrc/features.hip) -- against the NumPy reference of tests/hash_sample_cases.py, through its three entry
points: annchor_hash_sample, annchor_hash_sample_pairs and the no-wait annchor_hash_sample_pairs_device.

Every comparison is exact: positions, feature rows and distances bit for bit.  A case uploads its own four feature columns
and not-computed mask over the complete pair list of 450 bundled strings (101 025 pairs), so the partition feature is whatever
the case needs (continuous, half-integers on the edges, constant, NaN) while the distances stay those of the strings.  The
retry loop is reached through DECLARED populations that differ from the true ones; before such a call the restatement of the
host loop says how many attempts it takes.
"""
import numpy as np
import pytest

import hash_sample_cases as H

pytestmark = pytest.mark.gpu

ROUTES = ("hash_sample", "hash_sample_pairs", "hash_sample_pairs_device")


@pytest.fixture(scope="module")
def engine():
    from annchor_amd import Annchor, _native
    from annchor_amd.datasets import load_strings
    X = load_strings()["X"][:H.N_STRINGS]
    ann = Annchor(X, "levenshtein", n_anchors=10, n_neighbors=10, p_work=0.3, niters=1, random_seed=3)
    ann.get_anchors()
    ann.get_locality()
    ann.get_features()
    eng = ann._engine
    n = eng.field_size(_native.F_NCM)
    assert n == H.N_PAIRS and n % 2048 != 0
    Y = eng.evaluate_samples(np.arange(n, dtype=np.int64))
    Y.setflags(write=False)
    yield eng, _native, Y
    eng.close()


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = H.build(name)
    return _CASES[name]


def _upload(eng, nat, c):
    eng.upload(nat.F_FEATURES, c.feats)
    eng.upload(nat.F_NCM, c.ncm.astype(np.uint8))
    assert eng.count_uncomputed() == int(c.ncm.sum())    # (from here on the library keeps the number up to date itself)


def _call(eng, nat, c, route):
    """(positions, feature rows, distances) of one sampling step by that route.  annchor_hash_sample hands back positions
    only and leaves the mask alone (fit() follows it with gather_features and evaluate_samples, which clears it): the same
    here."""
    if route == "hash_sample":
        pos = eng.hash_sample(c.edges, c.declared, c.want, c.seed_key)
        assert np.array_equal(eng.download(nat.F_NCM), c.ncm.astype(np.uint8))
        return pos, eng.gather_features(pos), eng.evaluate_samples(pos)
    if route == "hash_sample_pairs":
        return eng.hash_sample_pairs(c.edges, c.declared, c.want, c.seed_key)
    m = eng.hash_sample_pairs_device(c.edges, c.declared, c.want, c.seed_key)
    assert m == c.total
    pos, feats, y, _ = eng.download_samples(m, predict=False)
    return pos, feats, y


def _check(eng, nat, Y, c, route, expect=None):
    expect = c.reference() if expect is None else expect
    _upload(eng, nat, c)
    pos, feats, y = _call(eng, nat, c, route)
    assert pos.dtype == np.int64 and np.array_equal(pos, expect), (c.name, route)
    assert np.array_equal(feats, c.feats[expect], equal_nan=True), (c.name, route)
    assert np.array_equal(y, Y[expect]), (c.name, route)
    left = c.ncm.copy()
    left[expect] = False
    assert np.array_equal(eng.download(nat.F_NCM), left.astype(np.uint8)), (c.name, route)
    assert eng.count_uncomputed() == int(left.sum()), (c.name, route)
    return left


def _attempts(c):
    """What the restatement of the host loop says about the case, checked against what the case is there for."""
    loop = H.host_loop(c)
    if c.attempts == "refused":
        assert not loop.settled and loop.attempts == H.ATTEMPTS
        return loop
    lo, hi = c.attempts if isinstance(c.attempts, tuple) else (c.attempts, c.attempts)
    assert loop.settled and lo <= loop.attempts <= hi, (c.name, loop.attempts)
    print("%s: %d attempt(s), list lengths %s" % (c.name, loop.attempts, [list(map(int, L)) for L in loop.lengths]))
    return loop


# ------------------------------------------------------------------------------------------------ one attempt
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", H.SETTLING)
def test_one_attempt_equals_reference(engine, name, route):
    eng, nat, Y = engine
    c = case(name)
    assert _attempts(c).attempts == 1
    _check(eng, nat, Y, c, route)


@pytest.mark.parametrize("route", ROUTES)
def test_second_step_on_the_reduced_mask(engine, route):
    """Two steps of one fit: the second with the next loop_num's key on the mask the first one left."""
    eng, nat, Y = engine
    c = H.build("halfint_p7")
    c.seed_key = H.step_key(42, 0)
    left = _check(eng, nat, Y, c, route)
    nxt = c.after(left, H.step_key(42, 1))
    ref2 = nxt.reference()
    assert not np.intersect1d(ref2, c.reference()).size
    # (no upload in between: the device's own mask and count are what the second step draws from)
    pos, feats, y = _call(eng, nat, nxt, route)
    assert np.array_equal(pos, ref2) and np.array_equal(feats, c.feats[ref2]) and np.array_equal(y, Y[ref2])
    left[ref2] = False
    assert np.array_equal(eng.download(nat.F_NCM), left.astype(np.uint8))
    assert eng.count_uncomputed() == int(left.sum())


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("blocks", ["1", "3"])
@pytest.mark.parametrize("name", ["halfint_p7", "want2048", "finite_outer_edges"])
def test_grid_stride_loop(engine, name, blocks, route, monkeypatch):
    """k_hs_collect sizes its grid for the list and strides only above 256 * 8 * 8 * CUs pairs; with the block count capped,
    one workgroup (or three: a tail that not every workgroup sees) walks the whole list."""
    eng, nat, Y = engine
    monkeypatch.setenv("ANNCHOR_HS_MAX_BLOCKS", blocks)
    _check(eng, nat, Y, case(name), route)


# ------------------------------------------------------------------------------------------------ the retry loop
@pytest.mark.parametrize("route", ROUTES[:2])
@pytest.mark.parametrize("name", H.RETRY)
def test_retry_loop_settles(engine, name, route):
    """Short lists double the threshold, overflowing lists halve it; the attempt that settles gives the reference's choice."""
    eng, nat, Y = engine
    c = case(name)
    assert _attempts(c).attempts >= 2
    _check(eng, nat, Y, c, route)


@pytest.mark.parametrize("route", ROUTES[:2])
def test_retry_loop_refuses_after_eight_attempts(engine, route):
    eng, nat, Y = engine
    c = case(H.REFUSED[0])
    _attempts(c)
    _upload(eng, nat, c)
    with pytest.raises(nat.NativeError, match="did not settle"):
        _call(eng, nat, c, route)
    _check(eng, nat, Y, case("halfint_p7"), route)     # the engine is none the worse for it


# ------------------------------------------------------------------------------------------------ the no-wait form
def _sticky_flags(eng, c):
    """The sticky flags the way fit() reads them: after the device-side model fit, with the model."""
    eng.fit_regression_device(c.edges, 1, 1)
    return eng.model_download(c.nb, with_errors=False)[4]


def test_no_wait_form_on_a_short_list_leaves_defined_positions(engine):
    """annchor_hash_sample_pairs_device makes one attempt and raises sticky flag 2 on the device when a list came out short;
    by then the positions have been gathered at, evaluated and cleared in the mask.  Every slot is a member all the same: a
    short list's last position repeated (k_hs_finish), never what an earlier call left in the buffer."""
    eng, nat, Y = engine
    before = H.build("continuous_p7")          # a correct call with another key first: stale slots would hold ITS positions
    assert before.total == case(H.SHORT_NO_WAIT).total
    _check(eng, nat, Y, before, ROUTES[2])
    assert _sticky_flags(eng, before)[0] == 0
    c = case(H.SHORT_NO_WAIT)
    assert c.seed_key != before.seed_key
    expect, settled = H.first_attempt_output(c)
    assert not settled and expect.size == c.total and np.unique(expect).size < expect.size
    _upload(eng, nat, c)
    m = eng.hash_sample_pairs_device(c.edges, c.declared, c.want, c.seed_key)
    assert m == c.total
    assert _sticky_flags(eng, c)[0] == 2
    pos, feats, y, _ = eng.download_samples(m, predict=False)
    assert np.array_equal(pos, expect)
    assert np.array_equal(feats, c.feats[expect]) and np.array_equal(y, Y[expect])
    left = c.ncm.copy()
    left[expect] = False
    assert np.array_equal(eng.download(nat.F_NCM), left.astype(np.uint8))
    after = case("halfint_p9")
    _check(eng, nat, Y, after, ROUTES[2])
    assert _sticky_flags(eng, after)[0] == 0
