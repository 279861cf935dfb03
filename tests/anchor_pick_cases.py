"""The "line family": the data sets of the max-min pick tests (test_anchor_pick_cases.py, test_anchor_pick_gpu.py), their
encoders and the one reference all routes share.

A case is a vector of integer positions p[j] in 0 .. 36.  Every route gets an encoder under which its bundled metric returns
exactly |p[j] - p[k]| (the lattice rows of the streamed routes: exactly LATTICE_SCALE[dim] * |p[j] - p[k]|), so one reference
serves all routes and every comparison is array_equal.

Positions: a bulk drawn from 15 .. 21; the value 36 at the indices `hi` and the value 0 at the indices `lo` (two of each,
more where a rank needs copies); the first anchor at a bulk member with p = 18 that is the LOWEST index holding 18 (earlier
18s become 17).  Then, whatever the bulk draws (p = 18 at `first`; HI one of the 36s, LO one of the 0s):

    round 0   row |p - 18|: every 36 and every 0 is at 18, the bulk at most at 3      -> the first of hi + lo wins
    round 1   restarts from row 1 alone: the other planted kind is at 36              -> its first index wins, >= 2 maximal
    round 2   restarts WITHOUT row 0 (the D[1:] quirk): min(|p - 36|, |p|) is 18 at every bulk 18, `first` included
              -> `first` is picked again: a repeated anchor, and from then on a zero column in the running minimum
    round 3+  the bulk values 15 / 21 (at 3), then 16 / 17 / 19 / 20 (at 1): hundreds to thousands of maximal indices

The planted indices come from the tables below.  Each route's table is stated as element -> lane / wave / workgroup of the
kernel that reads it (`READERS`), and each case names at least one tie j1 < j2 in which j2 is read by a LOWER-numbered unit
than j1 (`adversarial`: (j1, j2, unit)): a reduction that prefers the lower lane, the earlier trip or the first partial it
saw picks j2, the reference picks j1.  One maximal value sits at index nx - 1 (a lost tail element).

Two things the construction cannot give, stated here so that no test passes by accident:
  * nx = 5 (route 1, fewer points than one wave): element j is read by lane j, so no tie can be adversarial, and round 2 has
    ONE maximal index (the only 18 is `first`).  Both are pinned in test_anchor_pick_cases.py as exactly that.
  * one row (streamed n = 1, `single_row`): nothing can tie; it is a degenerate shape of the kernels, not a case."""
import functools
from unittest import mock

import numpy as np

from oracle import annchor_oracle as O

NA = 8
BULK_LO, BULK_HI, MID, HI, LO = 15, 21, 18, 36, 0

# --------------------------------------------------------------------------------------------------- who reads element j
ONE_THREADS = 1024        # k_runmin_argmax_one: one workgroup, thread j mod 1024, waves of 64
ONE_MAX = 16384           # the last nx of route 1
RED_THREADS = 256         # k_runmin_argmax / k_st_runmin_argmax: workgroups of 256, grid stride rblocks * 256
RED_PER_BLOCK = 1024      # rblocks = min(1024, ceil(nx / 1024))
FINAL_THREADS = 64        # k_argmax_final: partial b -> thread b mod 64
CAND_THREADS = 256        # k_sh_cand: partial b -> thread b mod 256
WAVE = 64
FUSED_TRIP = 512          # k_lev_r / k_lev_f: lane j mod 64, 8 elements per lane and trip (k_lev_a2: 16, trips of 1024)
FUSED_MAX = 8192          # the last nx of route 3


def rblocks(nx):
    return min(1024, -(-nx // RED_PER_BLOCK))


def reader_one(j, nx):
    t = j % ONE_THREADS
    return dict(trip=j // ONE_THREADS, thread=t, wave=t // WAVE, lane=t % WAVE)


def reader_partials(j, nx, final_threads=FINAL_THREADS):
    g = j % (rblocks(nx) * RED_THREADS)
    b, t = g // RED_THREADS, g % RED_THREADS
    return dict(trip=j // (rblocks(nx) * RED_THREADS), block=b, thread=t, wave=t // WAVE, lane=t % WAVE,
                final_thread=b % final_threads, final_trip=b // final_threads)


def reader_fused(j, nx):
    return dict(trip=j // FUSED_TRIP, trip_a2=j // (2 * FUSED_TRIP), lane=j % WAVE)


def reader_stream(j, nx):
    return reader_partials(j, nx, CAND_THREADS)


def reader_ranks(j, sizes):
    """Global row j of contiguous shards -> its rank, and the streamed reader of its local index there."""
    starts = np.concatenate([[0], np.cumsum(sizes)])
    r = int(np.searchsorted(starts, j, side="right") - 1)
    return dict(rank=r, local=j - int(starts[r]), **reader_stream(j - int(starts[r]), int(sizes[r])))


READERS = dict(one=reader_one, partials=reader_partials, fused=reader_fused, stream=reader_stream)

# ------------------------------------------------------------------------------------------------------------ the tables
# (route, nx) -> first, hi (the 36s), lo (the 0s), adversarial [(j1, j2, unit)]: j1 < j2, READERS[route](j2)[unit] < ...(j1)[unit]
PLANTS = {
    # route 1: thread j mod 1024
    ("one", 5): dict(first=1, hi=(0, 3), lo=(2, 4), adversarial=[]),                      # lane j: none possible
    ("one", 65): dict(first=1, hi=(3, 40), lo=(63, 64), adversarial=[(63, 64, "lane")]),  # lane 63 of wave 0, lane 0 of wave 1
    ("one", 1025): dict(first=2, hi=(63, 64), lo=(1023, 1024), adversarial=[(63, 64, "lane"), (1023, 1024, "thread")]),
    ("one", 8193): dict(first=2, hi=(1023, 1024), lo=(8191, 8192), adversarial=[(1023, 1024, "thread"), (8191, 8192, "thread")]),
    ("one", 16384): dict(first=2, hi=(1023, 1024), lo=(15359, 16383), adversarial=[(1023, 1024, "thread")]),
    # route 2: 17 workgroups, stride 4352; element 4351 is workgroup 16's, 4352 workgroup 0's; 12800 workgroup 16's, 16384 workgroup 13's
    ("partials", 16385): dict(first=2, hi=(4351, 4352), lo=(12800, 16384),
                              adversarial=[(4351, 4352, "block"), (12800, 16384, "block")]),
    # 65 workgroups, stride 16640: partial 64 is thread 0's SECOND trip in k_argmax_final, after partial 0.  16384 is
    # workgroup 64's, 16640 workgroup 0's; 49408 workgroup 63's, 65536 workgroup 61's
    ("partials", 65537): dict(first=2, hi=(16384, 16640), lo=(49408, 65536),
                              adversarial=[(16384, 16640, "block"), (16384, 16640, "final_trip"), (49408, 65536, "block")]),
    # route 3: lane j mod 64, trips of 512 (k_lev_a2: 1024)
    ("fused", 511): dict(first=2, hi=(63, 64), lo=(447, 510), adversarial=[(63, 64, "lane"), (447, 510, "lane")]),
    ("fused", 512): dict(first=2, hi=(63, 64), lo=(500, 511), adversarial=[(63, 64, "lane")]),
    ("fused", 513): dict(first=2, hi=(63, 64), lo=(511, 512), adversarial=[(63, 64, "lane"), (511, 512, "lane")]),
    ("fused", 8192): dict(first=2, hi=(4095, 4096), lo=(8127, 8191), adversarial=[(4095, 4096, "lane")]),
    # routes 6 and 7: as route 2 in float32; 255 rows: one workgroup; 1025: two, stride 512; 4097: five, stride 1280
    ("stream", 255): dict(first=2, hi=(63, 64), lo=(191, 254), adversarial=[(63, 64, "lane"), (191, 254, "lane")]),
    ("stream", 1025): dict(first=2, hi=(511, 512), lo=(1023, 1024), adversarial=[(511, 512, "block"), (1023, 1024, "block")]),
    ("stream", 4097): dict(first=2, hi=(1279, 1280), lo=(3839, 4096), adversarial=[(1279, 1280, "block"), (3839, 4096, "block")]),
}

# route 8: contiguous shards, bases increasing with rank (so a lower rank always holds the lower rows: across ranks the rule is
# "the earlier rank wins a tie", within a rank the streamed reader's)
RANKS = {
    # rank 0 is ONE row, a 36: round 0 ties it with 1300 (a 36, the last row) and 512, 513 (the 0s) of rank 1 -- across ranks and within rank 1
    # at once; it becomes anchor 1, so its shard's maximum is 0 from round 1 on.  `first` is in the last rank: rank 0's first
    # candidate has row -1.  Round 1 ties 512 and 513 inside rank 1: local 511 (workgroup 1) and 512 (workgroup 0)
    2: dict(sizes=(1, 1300), first=6, hi=(0, 1300), lo=(512, 513), adversarial=[(512, 513, "block")]),
    # rank 1 is ONE row (300), a copy of row 255, which becomes anchor 1.  Round 0 ties 255 and 299 in rank 0 (thread 255 of
    # trip 0, thread 43 of trip 1), row 300 of rank 1 and row 1400 of rank 2; round 1 ties 299 (rank 0) with 1400 (rank 2)
    3: dict(sizes=(300, 1, 1100), first=1, hi=(255, 300), lo=(299, 1400), adversarial=[(255, 299, "thread")]),
    # rank 1 (rows 257 .. 259) holds 36, 0, 36: copies of anchors 1 and 2, maximum 0 from round 2 on; rank 2 is ONE row;
    # round 0 ties rows of ranks 0, 1, 3 and 4; round 1 ties 258 (rank 1) with 772, 773 (rank 3: local 511 and 512, workgroups
    # 1 and 0) and 1790 (rank 4, the last row); `first` is in the last rank
    5: dict(sizes=(257, 3, 1, 1030, 500), first=1298, hi=(63, 64, 257, 259), lo=(258, 772, 773, 1790),
            adversarial=[(63, 64, "lane")]),
}


# ------------------------------------------------------------------------------------------------------------- the cases
class Case:
    def __init__(self, name, route, nx, seed, plants, sizes=None):
        self.name, self.route, self.nx, self.sizes = name, route, nx, sizes
        self.first, self.hi, self.lo = plants["first"], tuple(plants["hi"]), tuple(plants["lo"])
        self.adversarial = list(plants["adversarial"])
        p = np.random.default_rng(seed).integers(BULK_LO, BULK_HI + 1, nx)
        p[self.first] = MID
        head = p[:self.first]
        head[head == MID] = MID - 1
        p[list(self.hi)] = HI
        p[list(self.lo)] = LO
        p.setflags(write=False)
        self.p = p

    def reader(self, j):
        return reader_ranks(j, self.sizes) if self.route == "ranks" else READERS[self.route](j, self.nx)

    def __repr__(self):
        return self.name


def _cases():
    out, seed = [], 1000
    names = [("one-f64-5", "one", 5), ("one-f64-65", "one", 65), ("one-f64-1025", "one", 1025), ("one-f64-16384", "one", 16384),
             ("one-f32-1025", "one", 1025), ("one-lev-8193", "one", 8193), ("one-hausdorff-1025", "one", 1025),
             ("partials-f64-16385", "partials", 16385), ("partials-f64-65537", "partials", 65537),
             ("partials-lev-16385", "partials", 16385),
             ("fused-lev-511", "fused", 511), ("fused-lev-512", "fused", 512), ("fused-lev-513", "fused", 513),
             ("fused-lev-8192", "fused", 8192),
             ("stream-255", "stream", 255), ("stream-1025", "stream", 1025), ("stream-4097", "stream", 4097)]
    for name, route, nx in names:
        seed += 1
        out.append(Case(name, route, nx, seed, PLANTS[(route, nx)]))
    for W, t in RANKS.items():
        seed += 1
        out.append(Case("ranks-%d" % W, "ranks", int(sum(t["sizes"])), seed, t, sizes=tuple(t["sizes"])))
    return {c.name: c for c in out}


CASES = _cases()
NO_ADVERSARIAL = {"one-f64-5"}          # lane j reads element j
UNIQUE_MAXIMUM = {("one-f64-5", 2)}     # (case, round): five points hold one 18


# ---------------------------------------------------------------------------------------------------------- the encoders
def points64(p):
    """1-D float64 points: Euclidean is sqrt((p - q)^2) = |p - q| exactly."""
    return np.asarray(p, dtype=np.float64)[:, None]


def points32(p):
    return np.asarray(p, dtype=np.float32)[:, None]


def strings(p):
    """Levenshtein("a" * p, "a" * q) = |p - q|; p = 0 is the empty string."""
    return ["a" * int(v) for v in p]


def point_sets(p):
    """Hausdorff on one-point sets of dim 1: sqrt((p - q)^2)."""
    return [np.array([[float(v)]]) for v in p]


# rows p * u + b with |u| a whole number: the distance is |u| * |p - q|, every coordinate takes part, and the sums of
# squares (at most 16 * 36^2 = 20736) are exact in float32 in any summation order
LATTICE_U = {3: np.array([1, 2, 2]), 8: np.array([1, 1, 1, 1, 1, 1, 1, 3])}
LATTICE_SCALE = {3: 3, 8: 4}


def lattice(p, dim):
    b = np.arange(dim) - 2
    return (np.outer(np.asarray(p), LATTICE_U[dim]) + b[None, :]).astype(np.float32)


# --------------------------------------------------------------------------------------------------------- the reference
def reference(one_to_all, nx, first, na=NA):
    """oracle.annchor_oracle.maxmin_anchors with the first index given (its one random draw returns `first`): (A, D [nx, na])."""
    with mock.patch.object(O.np.random, "randint", return_value=int(first)):
        A, D = O.maxmin_anchors(one_to_all, nx, na, 0)
    assert A[0] == first
    return A, D


def line_reference(p, first, na=NA):
    p = np.asarray(p, dtype=np.int64)
    return reference(lambda ix: np.abs(p - p[ix]).astype(np.float64), len(p), first, na)


def lattice_reference(X, first, na=NA):
    """The streamed routes: distances np.sqrt(np.float32(s)), s the sum of squares of the (integer) differences."""
    Xi = np.asarray(X).astype(np.int64)
    assert np.array_equal(Xi.astype(np.float32), X)

    def one_to_all(ix):
        s = ((Xi - Xi[ix][None, :]) ** 2).sum(axis=1)
        assert s.max() < 1 << 24
        return np.sqrt(np.float32(s)).astype(np.float64)

    return reference(one_to_all, len(X), first, na)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """(A, D) of a case on |p - p[a]|, computed once and read-only."""
    c = CASES[name]
    A, D = line_reference(c.p, c.first)
    A.setflags(write=False)
    D.setflags(write=False)
    return A, D


def rounds(D):
    """What the pick of every round saw, from the reference's rows alone: per round r the running minimum's (maximum, first
    maximal index, every maximal index) -- over row 0 for r = 0, over rows 1 .. r afterwards."""
    out = []
    for r in range(D.shape[1]):
        m = D[:, 0] if r == 0 else D[:, 1:r + 1].min(axis=1)
        top = np.flatnonzero(m == m.max())
        out.append((float(m.max()), int(top[0]), top))
    return out


def single_row(dim):
    """The degenerate shape n = 1 of the streamed routes: one lattice row, picked eight times, distances 0."""
    return lattice(np.array([MID]), dim)
