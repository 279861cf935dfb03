"""The reference and the cases of tests/hash_sample_cases.py, checked without a GPU: the reference is the sampler's own
NumPy choice and the oracle's, deliberate mistakes in it are told apart by the cases, and every case reaches the branch of
the host loop that it is built for."""
import numpy as np
import pytest

import hash_sample_cases as H

ALL = H.SETTLING + H.RETRY + H.REFUSED


@pytest.fixture(scope="module")
def cases():
    return {name: H.build(name) for name in ALL}


def test_reference_equals_the_sampler_and_the_oracle():
    """On random inputs: choose() == DeviceStratifiedSampler.sample_partition (through sample()) ==
    oracle.hashed_stratified_sample, over two steps (loop_num 0 and 1) with the mask reduced in between."""
    from annchor_amd.samplers import DeviceStratifiedSampler, splitmix64
    from oracle import annchor_oracle as O

    x = np.arange(1000, dtype=np.uint64) * np.uint64(0x123456789ABCDEF)
    assert np.array_equal(H.splitmix64(x), splitmix64(x))
    names = ["lower bound", "upper bound", "double anchor distance", "is anchor"]
    rng = np.random.default_rng(17)
    for trial in range(8):
        n = int(rng.integers(4000, 30000))
        f = np.round(rng.normal(10, 4, (n, 4)), int(rng.integers(0, 3)))
        m = rng.random(n) < 0.85
        s = DeviceStratifiedSampler()
        for loop in range(2):
            ns = int(rng.integers(60, 900))
            assert s.loop_num == loop and s.seed_key(42) == H.step_key(42, loop)
            got = s.sample(f, names, ns, m, 42)
            ora = O.hashed_stratified_sample(f, m, ns, 42, loop)
            edges = got[2]
            granted = s._quantile_ranks(int(m.sum()), ns, 7)[2]
            want = granted // 7 + (np.arange(7) < granted % 7)
            mine = H.choose(f[:, 2], m, edges, H.true_counts(f[:, 2], m, edges), want, H.step_key(42, loop))
            assert np.array_equal(mine, got[0]) and np.array_equal(mine, ora[0]), (trial, loop)
            m = m.copy()
            m[mine] = False


def test_keys_are_distinct(cases):
    """(what the module docstring argues: no two positions share a key, so no tie case exists)"""
    for seed in H.SEEDS:
        assert np.unique(H.keys_of(seed, H.N_PAIRS)).size == H.N_PAIRS
    assert {c.seed_key for c in cases.values()} == set(H.SEEDS)


@pytest.mark.parametrize("c,w,thr", [(417, 100, 9466674416723846632), (333, 100, 11854664359681213350), (160304, 100, 24625731309099236),
                                     (41041920, 100, 96184662700327), (3137, 2048, 18440863696255388545),
                                     (6272, 2048, 9223372036854775807), (12544, 2048, 4611686018427387903),
                                     (1000003, 2, 1235928145154104), (214, 100, H.M64), (215, 100, 18360945264064390910),
                                     (99999999999, 2048, 578489894157), (3136, 2048, H.M64), (100, 100, H.M64), (0, 5, H.M64)])
def test_first_threshold_is_the_long_double_expression(c, w, thr):
    """Values printed by the C++ expression of hash_sample_device, compiled for x86-64 (80-bit long double)."""
    assert H.first_thresholds([c], [w]) == [thr]


@pytest.mark.parametrize("mutation", H.MUTATIONS)
def test_a_mutated_reference_is_caught(cases, mutation):
    caught = [name for name in H.SETTLING if not np.array_equal(cases[name].reference(), cases[name].reference(mutation))]
    assert caught, mutation
    # where a mistake must show: the edge rule on tied values, the order and the side of the choice wherever a partition is
    # sampled, the quota where fewer are declared than there are
    must = {"upper_le": "halfint_p7", "key_order": "continuous_p7", "largest": "continuous_p7", "no_xor": "continuous_p7",
            "want_not_min": "under_declared"}[mutation]
    assert must in caught


def test_cases_reach_what_they_are_built_for(cases):
    for name, c in cases.items():
        assert c.n == H.N_PAIRS and (c.want <= H.HS_CAP // 2).all()
        loop = H.host_loop(c)
        if c.attempts == "refused":
            assert not loop.settled and loop.attempts == H.ATTEMPTS, name
            continue
        assert loop.settled, name
        lo, hi = c.attempts if isinstance(c.attempts, tuple) else (c.attempts, c.attempts)
        assert lo <= loop.attempts <= hi, (name, loop.attempts)
        # the attempt that settles holds the wanted members, and then the two restatements are one
        ref = c.reference()
        assert ref.size == c.total and c.ncm[ref].all() and np.unique(ref).size == ref.size, name
        if loop.attempts == 1:
            out, ok = H.first_attempt_output(c)
            assert ok and np.array_equal(out, ref), name
    for name in H.SETTLING:
        if name not in ("under_declared", "cap_exactly_full"):
            assert np.array_equal(cases[name].declared, cases[name].true), name
    assert 0.55 < cases["halfint_p7"].ncm.mean() < 0.65


def test_case_shapes(cases):
    c = cases["whole_partitions"]
    assert list(c.true[:6]) == [0, 1, 2, 49, 50, 51] and (c.true[6:] > 1000).all() and c.want[0] == 50
    ref = c.reference()
    assert ref[0] == 0 and ref[2] == H.N_PAIRS - 1     # pair 0 is the partition of one, pair n - 1 the larger of the two
    c = cases["sort_sizes"]
    assert list(c.true[:6]) == [63, 64, 65, 1024, 1025, 3136] and list(c.want[6:]) == [64, 65]
    L = H.host_loop(c).lengths[0]
    assert list(L[:6]) == [63, 64, 65, 1024, 1025, 3136] and (L[6:] > 65).all() and (L[6:] <= 512).all()
    c = cases["small_partitions_last"]
    thr = H.first_thresholds(c.declared, c.want)
    assert list(c.true[8:]) == [30, 150, 400, 1000] and max(thr[:8]) < min(thr[8:]) // 4 and thr[8] == thr[9] == H.M64
    c = cases["constant_equal_edges"]
    assert list(c.true[:6]) == [0] * 6 and c.true[6] == c.ncm.sum()
    c = cases["finite_outer_edges"]
    ref = c.reference()
    assert np.isnan(c.dad).sum() > 500 and np.isinf(c.dad).sum() > 50 and c.true.sum() < c.ncm.sum()
    assert (c.dad[ref] >= 5.0).all() and (c.dad[ref] < 55.0).all() and (c.dad[ref] == 5.0).any() and (c.dad[c.ncm] == 55.0).any()
    for p in (7, 64):       # many members exactly on every edge, the last finite one included
        c = cases["halfint_p%d" % p]
        for e in c.edges[1:-1]:
            assert ((c.dad == e) & c.ncm).sum() > 100
        ref = c.reference()
        assert (c.dad[ref] == c.edges[-2]).any() and (c.dad[ref] == c.edges[1]).any()
    c = cases["want2048"]
    L = H.host_loop(c).lengths[0]
    assert (L > 2048).all() and (L <= H.HS_CAP).all()
    assert H.host_loop(cases["cap_exactly_full"]).lengths == [[H.HS_CAP]]
    loop = H.host_loop(cases["cap_plus_one"])
    assert [list(x) for x in loop.lengths] == [[H.HS_CAP + 1], [2100]]
    loop = H.host_loop(cases["declared_div24"])
    assert (loop.lengths[0] > H.HS_CAP).all() and (loop.lengths[1] <= H.HS_CAP).all()
    loop = H.host_loop(cases["declared_x16"])
    assert (loop.lengths[0] < 100).all() and (loop.lengths[-1] >= 100).all()
    out, ok = H.first_attempt_output(cases["declared_x16"])
    assert not ok and out.size == 700 and np.unique(out).size < 700 and cases["declared_x16"].ncm[out].all()
    assert (H.host_loop(cases["declared_x4096"]).lengths[-1] < 100).any()


def test_second_step_differs_and_is_disjoint(cases):
    c = cases["halfint_p7"]
    ref = c.reference()
    ncm = c.ncm.copy()
    ncm[ref] = False
    nxt = c.after(ncm, H.step_key(c.seed_key, 1))
    ref2 = nxt.reference()
    assert ref2.size == ref.size and not np.intersect1d(ref, ref2).size and H.host_loop(nxt).attempts == 1
