"""Conditions on the line family (anchor_pick_cases.py), from the reference alone: they keep test_anchor_pick_gpu.py from
passing vacuously.  Nothing here touches a device."""
import numpy as np
import pytest

import anchor_pick_cases as ac
import hausdorff_cases as hc
from oracle import annchor_oracle as O
from oracle import metrics as om

NAMES = list(ac.CASES)


def test_reference_is_the_oracle_picker_with_the_first_index_given():
    """`reference` against the oracle run on a seed whose draw is the case's first index, and against the loop written out."""
    c = ac.CASES["one-f64-65"]
    seed = next(s for s in range(10000) if O.maxmin_first_index(c.nx, s) == c.first)
    p = c.p.astype(np.int64)
    A, D = O.maxmin_anchors(lambda ix: np.abs(p - p[ix]).astype(np.float64), c.nx, ac.NA, seed)
    gotA, gotD = ac.case_reference(c.name)
    assert np.array_equal(gotA, A) and np.array_equal(gotD, D)
    ix, rows = c.first, []
    for i in range(ac.NA):   # pickers.py:44-50
        assert A[i] == ix
        rows.append(np.abs(p - p[ix]).astype(np.float64))
        ix = int(np.argmax(rows[0])) if i == 0 else int(np.argmax(np.min(rows[1:], axis=0)))


@pytest.mark.parametrize("name", NAMES)
def test_positions_are_what_the_module_says(name):
    c = ac.CASES[name]
    p = c.p
    assert len(p) == c.nx and p.min() == ac.LO and p.max() == ac.HI
    planted = set(c.hi) | set(c.lo)
    assert len(planted) == len(c.hi) + len(c.lo) and c.first not in planted
    assert sorted(np.flatnonzero(p == ac.HI)) == sorted(c.hi) and sorted(np.flatnonzero(p == ac.LO)) == sorted(c.lo)
    bulk = np.delete(p, sorted(planted))
    assert bulk.min() >= ac.BULK_LO and bulk.max() <= ac.BULK_HI
    assert p[c.first] == ac.MID and np.flatnonzero(p == ac.MID)[0] == c.first
    assert c.nx - 1 in planted            # a maximal value at the last index (rounds 0 and 1 check that it is maximal)
    assert len(c.hi) >= 2 and len(c.lo) >= 2


@pytest.mark.parametrize("name", NAMES)
def test_every_round_is_tied(name):
    c = ac.CASES[name]
    A, D = ac.case_reference(name)
    rr = ac.rounds(D)
    for r, (_, arg, top) in enumerate(rr):
        if r + 1 < ac.NA:
            assert A[r + 1] == arg
        if (name, r) in ac.UNIQUE_MAXIMUM:
            assert len(top) == 1 and c.nx == 5   # the exception is exactly what the module says, not a licence
        else:
            assert len(top) >= 2, (name, r, top)
    # round 0 ties the 36s with the 0s; round 1 the other kind; both include the last index in one of them
    assert sorted(rr[0][2]) == sorted(c.hi + c.lo)
    assert sorted(rr[1][2]) in (sorted(c.hi), sorted(c.lo))
    assert c.nx - 1 in rr[0][2] and (c.nx - 1 in rr[1][2] or c.nx - 1 in c.hi + c.lo)
    if c.nx > 1000:
        assert max(len(top) for _, _, top in rr) > 100


@pytest.mark.parametrize("name", NAMES)
def test_the_adversarial_tie_decides_a_round(name):
    c = ac.CASES[name]
    _, D = ac.case_reference(name)
    rr = ac.rounds(D)
    if name in ac.NO_ADVERSARIAL:
        # no pair can be adversarial: the unit that reads an element grows with its index
        assert not c.adversarial and c.nx <= ac.WAVE
        assert all(c.reader(j)["lane"] == j and c.reader(j)["thread"] == j for j in range(c.nx))
        return
    assert c.adversarial
    for j1, j2, unit in c.adversarial:
        assert j1 < j2 and c.reader(j2)[unit] < c.reader(j1)[unit], (j1, j2, unit, c.reader(j1), c.reader(j2))
        if c.route == "ranks":
            assert c.reader(j1)["rank"] == c.reader(j2)["rank"]   # the streamed reader's units are per rank
        decided = [r for r, (_, arg, top) in enumerate(rr) if arg == j1 and j2 in top]
        assert decided, (name, j1, j2)


@pytest.mark.parametrize("name", NAMES)
def test_an_anchor_repeats(name):
    c = ac.CASES[name]
    A, _ = ac.case_reference(name)
    assert len(set(A.tolist())) < len(A)
    assert A[0] == c.first and A[3] == c.first   # round 2 restarts without row 0


def test_no_two_cases_share_positions():
    seen = {}
    for name, c in ac.CASES.items():
        key = c.p.tobytes()
        assert key not in seen, (name, seen.get(key))
        seen[key] = name
    # each route's adversarial plants come from its own table entry
    for (route, nx), t in ac.PLANTS.items():
        assert any(c.route == route and c.nx == nx for c in ac.CASES.values()), (route, nx)
    by_route = {}
    for c in ac.CASES.values():
        by_route.setdefault(c.route, set()).add((c.hi, c.lo))
    routes = list(by_route)
    for i, a in enumerate(routes):
        for b in routes[i + 1:]:
            if {a, b} == {"fused", "stream"} or {a, b} == {"one", "fused"} or {a, b} == {"one", "stream"}:
                continue   # lane j mod 64 is common to them: (63, 64) is adversarial in each, on purpose
            assert not (by_route[a] & by_route[b]), (a, b)


def test_lane_arithmetic_of_the_tables():
    """The readers against the constants the kernels' sources quote: 1024, 256, 64, 512."""
    assert (ac.ONE_THREADS, ac.RED_THREADS, ac.WAVE, ac.FUSED_TRIP, ac.FINAL_THREADS, ac.CAND_THREADS) == (1024, 256, 64, 512, 64, 256)
    assert (ac.ONE_MAX, ac.FUSED_MAX, ac.RED_PER_BLOCK) == (16384, 8192, 1024)
    # route 1
    assert ac.reader_one(1023, 1025) == dict(trip=0, thread=1023, wave=15, lane=63)
    assert ac.reader_one(1024, 1025) == dict(trip=1, thread=0, wave=0, lane=0)
    assert ac.reader_one(64, 65)["wave"] == 1 and ac.reader_one(64, 65)["lane"] == 0
    # route 2: rblocks = min(1024, ceil(nx / 1024)); partial b -> thread b mod 64 of the final
    assert [ac.rblocks(n) for n in (1, 1024, 1025, 16385, 65537, 1 << 21)] == [1, 1, 2, 17, 65, 1024]
    r = ac.reader_partials(4351, 16385)
    assert (r["block"], r["thread"], r["trip"]) == (16, 255, 0)
    r = ac.reader_partials(4352, 16385)
    assert (r["block"], r["thread"], r["trip"]) == (0, 0, 1)
    r = ac.reader_partials(16384, 65537)
    assert (r["block"], r["final_thread"], r["final_trip"]) == (64, 0, 1)
    r = ac.reader_partials(16640, 65537)
    assert (r["block"], r["final_thread"], r["final_trip"]) == (0, 0, 0)
    assert ac.reader_partials(65536, 65537)["block"] == 61 and ac.reader_partials(49408, 65537)["block"] == 63
    # route 3
    assert ac.reader_fused(511, 513) == dict(trip=0, trip_a2=0, lane=63)
    assert ac.reader_fused(512, 513) == dict(trip=1, trip_a2=0, lane=0)
    assert ac.reader_fused(4096, 8192) == dict(trip=8, trip_a2=4, lane=0)
    # route 6: five partials at 4097 rows, all in the first trip of k_sh_cand's 256 threads
    r = ac.reader_stream(4096, 4097)
    assert (r["block"], r["final_thread"], r["final_trip"]) == (1, 1, 0) and ac.rblocks(4097) == 5
    # route 8
    sizes = ac.RANKS[5]["sizes"]
    assert [ac.reader_ranks(j, sizes)["rank"] for j in (0, 256, 257, 259, 260, 261, 1290, 1291, 1790)] == [0, 0, 1, 1, 2, 3, 3, 4, 4]
    r = ac.reader_ranks(772, sizes)
    assert (r["rank"], r["local"], r["block"]) == (3, 511, 1)
    assert ac.reader_ranks(773, sizes)["block"] == 0
    # the sizes at which a route hands over to its neighbour are in the cases
    sizes_of = lambda route: {c.nx for c in ac.CASES.values() if c.route == route}   # noqa: E731
    assert {5, 65, 1025, ac.ONE_MAX, ac.FUSED_MAX + 1} <= sizes_of("one")
    assert {ac.ONE_MAX + 1, 65537} <= sizes_of("partials")
    assert {ac.FUSED_TRIP - 1, ac.FUSED_TRIP, ac.FUSED_TRIP + 1, ac.FUSED_MAX} <= sizes_of("fused")


def test_rank_layouts():
    for W, t in ac.RANKS.items():
        c = ac.CASES["ranks-%d" % W]
        sizes = t["sizes"]
        assert len(sizes) == W and len(set(sizes)) == W and 1 in sizes   # unequal, one shard of exactly one row
        _, D = ac.case_reference(c.name)
        rr = ac.rounds(D)
        rank = lambda j: c.reader(int(j))["rank"]   # noqa: E731
        # some round's maximum is tied across ranks and the winner is not in the last of them
        across = [r for r, (_, arg, top) in enumerate(rr) if len({rank(j) for j in top}) >= 2]
        assert across
        # ... and some round's is tied within a rank and across ranks at once
        both = [r for r in across if max(np.bincount([rank(j) for j in rr[r][2]])) >= 2]
        assert both
    # the first anchor in the last rank: every other rank's first candidate has row -1
    assert sum(ac.CASES["ranks-%d" % W].reader(t["first"])["rank"] == W - 1 for W, t in ac.RANKS.items()) >= 2
    # a shard that holds only copies of rows that become anchors: its running minimum is all zero from some round on
    for W, shard in ((2, 0), (3, 1), (5, 1)):
        c = ac.CASES["ranks-%d" % W]
        A, D = ac.case_reference(c.name)
        starts = np.concatenate([[0], np.cumsum(c.sizes)])
        rows = np.arange(starts[shard], starts[shard + 1])
        assert all(any(c.p[j] == c.p[a] for a in A) for j in rows)
        assert D[rows, 1:3].min(axis=1).max() == 0


# ------------------------------------------------------------------------------------------- the encoders are exact
def _pairs(nx, seed):
    return np.random.default_rng(seed).integers(0, nx, (200, 2))


def _want(p, IJ):
    return np.abs(p[IJ[:, 0]] - p[IJ[:, 1]]).astype(np.float64)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_euclidean_encoder(dtype):
    c = ac.CASES["one-f64-1025" if dtype == "f64" else "one-f32-1025"]
    X = ac.points64(c.p) if dtype == "f64" else ac.points32(c.p)
    assert X.dtype == (np.float64 if dtype == "f64" else np.float32)
    IJ = _pairs(c.nx, 1)
    assert np.array_equal(om.euclidean_pairs(X, IJ), _want(c.p, IJ))


def test_levenshtein_encoder():
    c = ac.CASES["one-lev-8193"]
    IJ = _pairs(c.nx, 2)
    IJ[0] = (c.hi[0], c.lo[0])   # 36 symbols against the empty string
    assert np.array_equal(om.PackedStrings(ac.strings(c.p)).pairs(IJ), _want(c.p, IJ))


def test_hausdorff_encoder():
    c = ac.CASES["one-hausdorff-1025"]
    IJ = _pairs(c.nx, 3)
    assert np.array_equal(hc.hausdorff_pairs_host(ac.point_sets(c.p), IJ), _want(c.p, IJ))


@pytest.mark.parametrize("dim", [3, 8])
def test_lattice_encoder(dim):
    c = ac.CASES["stream-1025"]
    X = ac.lattice(c.p, dim)
    assert X.dtype == np.float32 and X.shape == (c.nx, dim)
    assert int((ac.LATTICE_U[dim] ** 2).sum()) == ac.LATTICE_SCALE[dim] ** 2
    IJ = _pairs(c.nx, 4)
    assert np.array_equal(om.euclidean_pairs(X, IJ), ac.LATTICE_SCALE[dim] * _want(c.p, IJ))
    # the reference the streamed tests use is the line reference, scaled
    A, D = ac.lattice_reference(X, c.first)
    wantA, wantD = ac.case_reference(c.name)
    assert np.array_equal(A, wantA) and np.array_equal(D, ac.LATTICE_SCALE[dim] * wantD)
    assert np.array_equal(D.astype(np.float32).astype(np.float64), D)


def test_single_row_is_degenerate():
    X = ac.single_row(3)
    A, D = ac.lattice_reference(X, 0)
    assert X.shape == (1, 3) and not A.any() and not D.any()
