"""Reference and cases for the hashed stratified choice (k_hs_collect / k_hs_finish / k_hs_check behind
hash_sample_device, csrc/features.hip), shared by tests/test_hash_sample_cases.py (CPU) and
tests/test_hash_sample_gpu.py (GPU).

The choice, in plain NumPy (`choose`):
  * the partition of a not-computed pair is the b with edges[b] <= dad < edges[b + 1] (none: never chosen);
  * its key is splitmix64(seed_key ^ position);
  * partition b yields its min(want[b], declared[b]) smallest (key, position) members;
  * members are written in ascending position, partitions in order.

splitmix64 is a bijection of the 64-bit integers (an odd-constant add, two xor-shifts and two odd multiplications, each
invertible), and so is x -> seed_key ^ x: two positions NEVER share a key under one seed.  The position tie-break of
k_hs_finish's first sort can therefore not be reached by any input, and there is no tie case here -- do not look for one.

The host loop, restated (`host_loop`): hash_sample_device collects the members whose key is at most a per-partition
threshold into lists of HS_CAP entries and repeats the step, up to 8 times, with a halved threshold where a list
overflowed and a doubled one (saturating at all ones) where it came out short.  The first threshold is computed in
np.longdouble as the C++ computes it in long double.  With the true populations declared, a second attempt is a 1e-9
event; the cases reach the loop's branches deterministically by DECLARING counts that differ from the true ones, and the
restatement says how many attempts such a case takes, so that a GPU test can assert that it reaches the branch it is
there for.

`first_attempt_output` is the contract of the no-wait form (annchor_hash_sample_pairs_device: one attempt, checked on
the device): every one of the sum(min(want, declared)) slots is defined -- behind a short list's members its last
(largest) position repeated, position 0 for a list without members.
"""
import numpy as np

HS_CAP = 4096          # list entries per partition (features.hip)
ATTEMPTS = 8
M64 = (1 << 64) - 1

# the GPU fixture: the complete pair list of this many bundled strings (about 10^5 pairs, no multiple of 2048); the CPU
# tests build every case at the same length, so that what they establish holds for the arrays the kernels see
N_STRINGS = 450
N_PAIRS = N_STRINGS * (N_STRINGS - 1) // 2
assert N_PAIRS % 2048 != 0

SEEDS = (1, (1 << 63) + 5, M64)


def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def step_key(random_seed, loop_num):
    """DeviceStratifiedSampler.seed_key: the hash key of one sampling step."""
    return int(splitmix64(np.uint64((int(random_seed) + int(loop_num)) & M64)))


def keys_of(seed_key, n):
    return splitmix64(np.uint64(int(seed_key) & M64) ^ np.arange(n, dtype=np.uint64))


def partition_of(dad, edges, upper_le=False):
    """The first b with edges[b] <= dad < edges[b + 1]; -1 where there is none (outside finite outer edges, NaN)."""
    part = np.full(dad.shape, -1, dtype=np.int64)
    for b in range(len(edges) - 2, -1, -1):
        inside = (dad >= edges[b]) & ((dad <= edges[b + 1]) if upper_le else (dad < edges[b + 1]))
        part[inside] = b
    return part


def true_counts(dad, ncm, edges):
    part = partition_of(dad, edges)
    return np.bincount(part[ncm & (part >= 0)], minlength=len(edges) - 1).astype(np.int64)


MUTATIONS = ("upper_le", "key_order", "want_not_min", "largest", "no_xor")


def choose(dad, ncm, edges, declared, want, seed_key, mutation=None):
    """Positions of the samples (int64), partition by partition.  `mutation` names one deliberate mistake (MUTATIONS): the
    CPU tests show that the cases tell each of them from the right answer."""
    assert mutation is None or mutation in MUTATIONS
    n = dad.size
    part = partition_of(dad, edges, upper_le=mutation == "upper_le")
    part[~ncm] = -1
    keys = splitmix64(np.arange(n, dtype=np.uint64)) if mutation == "no_xor" else keys_of(seed_key, n)
    out = []
    for b in range(len(edges) - 1):
        members = np.flatnonzero(part == b)                          # ascending position
        order = np.lexsort((members, keys[members]))                 # by (key, position)
        if mutation == "largest":
            order = order[::-1]
        k = int(want[b]) if mutation == "want_not_min" else int(min(want[b], declared[b]))
        taken = members[order[:k]]
        out.append(taken if mutation == "key_order" else np.sort(taken))
    return np.concatenate(out).astype(np.int64)


# ---------------------------------------------------------------------------------------------- the host loop
_LD = np.longdouble
assert np.finfo(_LD).nmant == 63, "the restatement needs the 80-bit long double the C++ host code computes in"
_TWO32 = _LD(4294967296.0)
_ALL_ONES = _TWO32 * _TWO32 - _LD(1)      # 18446744073709551615.0L, exact in a 64-bit significand


def _ld_to_int(x):
    """Truncation of a long double in [0, 2^64) to an integer, as the C++ cast does (two exact halves)."""
    hi = np.floor(x / _TWO32)
    lo = np.floor(x - hi * _TWO32)
    return (int(float(hi)) << 32) + int(float(lo))


def first_thresholds(declared, want):
    thr = []
    for c, w in zip(declared, want):
        if c <= w or c <= 0:
            thr.append(M64)          # the whole partition
            continue
        frac = min(_LD(1), (_LD(1.5) * _LD(int(w)) + _LD(64)) / _LD(int(c)))
        thr.append(M64 if frac >= 1 else _ld_to_int(frac * _ALL_ONES))
    return thr


class Loop:
    """attempts: how many collect / finish rounds ran; lengths[a][b]: the true list length of partition b in attempt a (a
    list holds min(length, HS_CAP) entries); settled: the last attempt was accepted (False: the library refuses with
    "did not settle")."""

    def __init__(self, attempts, lengths, thresholds, settled):
        self.attempts, self.lengths, self.thresholds, self.settled = attempts, lengths, thresholds, settled


def _sorted_member_keys(case):
    part = partition_of(case.dad, case.edges)
    part[~case.ncm] = -1
    keys = keys_of(case.seed_key, case.dad.size)
    return [np.sort(keys[part == b]) for b in range(case.nb)]


def host_loop(case):
    h_want = np.minimum(case.want, case.declared)
    thr = first_thresholds(case.declared, case.want)
    skeys = _sorted_member_keys(case)
    lengths, thresholds = [], []
    for attempt in range(ATTEMPTS):
        L = np.array([int(np.searchsorted(skeys[b], np.uint64(thr[b]), side="right")) for b in range(case.nb)], dtype=np.int64)
        lengths.append(L)
        thresholds.append(list(thr))
        redo = False
        for b in range(case.nb):
            if L[b] > HS_CAP:
                thr[b] //= 2
                redo = True
            elif L[b] < h_want[b]:
                thr[b] = M64 if thr[b] > (M64 >> 1) else thr[b] * 2
                redo = True
        if not redo:
            return Loop(attempt + 1, lengths, thresholds, True)
    return Loop(ATTEMPTS, lengths, thresholds, False)


def first_attempt_output(case):
    """What the no-wait form leaves in its sum(min(want, declared)) slots after its single attempt, and whether that
    attempt settled.  Defined for attempts without an overflowing list (which 4096 of an overflowing list's members reach
    the list depends on the order of the atomics)."""
    h_want = np.minimum(case.want, case.declared)
    thr = first_thresholds(case.declared, case.want)
    part = partition_of(case.dad, case.edges)
    part[~case.ncm] = -1
    keys = keys_of(case.seed_key, case.dad.size)
    out, settled = [], True
    for b in range(case.nb):
        members = np.flatnonzero((part == b) & (keys <= np.uint64(thr[b])))
        assert members.size <= HS_CAP, "overflowing list: the attempt's output is not determined"
        order = np.lexsort((members, keys[members]))
        taken = np.sort(members[order[:h_want[b]]])
        settled &= taken.size == h_want[b]
        fill = taken[-1] if taken.size else 0
        out.append(np.concatenate([taken, np.full(int(h_want[b]) - taken.size, fill, dtype=np.int64)]))
    return np.concatenate(out).astype(np.int64), bool(settled)


# ---------------------------------------------------------------------------------------------- the cases
class Case:
    """One call: the four feature columns (lb, ub, dad, anc) and the not-computed mask to upload, the edges, the DECLARED
    populations, the quotas and the step's key.  attempts: what the restatement must say for this case -- an int, a
    (lo, hi) range, or "refused"."""

    def __init__(self, name, feats, ncm, edges, want, seed_key, declared=None, attempts=1):
        self.name = name
        self.feats = np.ascontiguousarray(feats, dtype=np.float64)
        self.dad = self.feats[:, 2]
        self.ncm = np.asarray(ncm, dtype=bool)
        self.edges = np.asarray(edges, dtype=np.float64)
        self.nb = self.edges.size - 1
        self.true = true_counts(self.dad, self.ncm, self.edges)
        self.declared = self.true.copy() if declared is None else np.asarray(declared, dtype=np.int64)
        self.want = np.broadcast_to(np.asarray(want, dtype=np.int64), (self.nb,)).copy()
        self.seed_key = int(seed_key) & M64
        self.attempts = attempts
        self._ref = None

    @property
    def n(self):
        return self.dad.size

    @property
    def total(self):
        return int(np.minimum(self.want, self.declared).sum())

    def reference(self, mutation=None):
        if mutation is not None:
            return choose(self.dad, self.ncm, self.edges, self.declared, self.want, self.seed_key, mutation)
        at = (self.seed_key, tuple(self.declared))
        if self._ref is None or self._ref[0] != at:     # (computed once per case, shared by the routes)
            ref = choose(self.dad, self.ncm, self.edges, self.declared, self.want, self.seed_key)
            ref.setflags(write=False)
            self._ref = (at, ref)
        return self._ref[1]

    def after(self, ncm, seed_key):
        """The next step on a reduced mask: same features and edges, the true populations declared."""
        return Case(self.name + "+next", self.feats, ncm, self.edges, self.want, seed_key)


def _features(rng, dad):
    n = dad.size
    lb = rng.rand(n) * 20.0
    return np.stack([lb, lb + rng.rand(n) * 20.0, dad, (rng.rand(n) < 0.1).astype(np.float64)], axis=1)


def _sampler_edges(dad, ncm, nparts):
    """What SimpleStratifiedSampler.get_partition makes of the 1 % / 99 % order statistics."""
    if nparts == 1:
        return np.array([-np.inf, np.inf])
    q1, q3 = np.quantile(dad[ncm], [0.01, 0.99])
    return np.hstack([-np.inf, np.linspace(q1, q3, nparts - 1), np.inf])


def _halfint_edges(nparts):
    """Every inner edge a half-integer that the column holds many times (values 0, 0.5 .. 60)."""
    if nparts == 1:
        return np.array([-np.inf, np.inf])
    inner = 15.0 + 0.5 * np.arange(nparts - 1) if nparts > 9 else np.round(2.0 * np.linspace(10.0, 50.0, nparts - 1)) / 2.0
    return np.hstack([-np.inf, inner, np.inf])


def _halfint(rng, n):
    return rng.randint(0, 121, n) / 2.0


def _whole_partitions(n, rng, sizes, want, seed_key, name, rest_want=None):
    """Partition b = [b, b + 1) with exactly sizes[b] members (None: every remaining pair of a 60 % mask); pair 0 and
    pair n - 1 are the first members handed out, so they sit in the first partitions that have any."""
    nb = len(sizes)
    perm = rng.permutation(np.arange(1, n - 1))
    pool = np.concatenate([[0, n - 1], perm])
    cls = np.full(n, -1, dtype=np.int64)
    at = 0
    for b, s in enumerate(sizes):
        if s is not None:
            cls[pool[at:at + s]] = b
            at += s
    rest = pool[at:]
    big = [b for b, s in enumerate(sizes) if s is None]
    for i, b in enumerate(big):
        cls[rest[i::len(big)]] = b
    dad = np.where(cls >= 0, cls + rng.randint(0, 2, n) * 0.5, -3.0)    # members sit ON the lower edge or half way
    ncm = cls >= 0
    for b in big:
        drop = np.flatnonzero(cls == b)
        ncm[drop[rng.rand(drop.size) < 0.4]] = False
    return Case(name, _features(rng, dad), ncm, np.arange(nb + 1, dtype=np.float64), want, seed_key)


SETTLING = (["continuous_p%d" % p for p in (1, 7, 8, 9, 64)] + ["halfint_p%d" % p for p in (1, 7, 8, 9, 64)]
            + ["constant_equal_edges", "want2", "want2048", "whole_partitions", "sort_sizes", "small_partitions_last", "finite_outer_edges", "under_declared",
               "cap_exactly_full"])
RETRY = ["declared_x16", "declared_div24", "cap_plus_one"]
REFUSED = ["declared_x4096"]
SHORT_NO_WAIT = "declared_x16"


def build(name, n=N_PAIRS):
    """The case of that name on a pair list of n entries (deterministic)."""
    rng = np.random.RandomState(sum(name.encode()) * 7919 % (1 << 31))
    seed = SEEDS[sum(name.encode()) % 3]
    if name.startswith("continuous_p"):
        p = int(name[len("continuous_p"):])
        dad = rng.rand(n) * 37.0
        ncm = rng.rand(n) < 0.6
        return Case(name, _features(rng, dad), ncm, _sampler_edges(dad, ncm, p), 100, seed)
    if name.startswith("halfint_p"):
        p = int(name[len("halfint_p"):])
        dad = _halfint(rng, n)
        return Case(name, _features(rng, dad), rng.rand(n) < 0.6, _halfint_edges(p), 100, seed)
    if name == "constant_equal_edges":
        # q1 == q3: the sampler's linspace gives six equal edges, partitions 1 .. 5 are empty by construction and 0 by content
        dad = np.full(n, 2.5)
        return Case(name, _features(rng, dad), rng.rand(n) < 0.6, np.hstack([-np.inf, np.full(6, 2.5), np.inf]), 100, seed)
    if name == "want2":
        dad = _halfint(rng, n)
        return Case(name, _features(rng, dad), rng.rand(n) < 0.6, _halfint_edges(7), 2, seed)
    if name == "want2048":
        dad = rng.rand(n) * 37.0
        ncm = rng.rand(n) < 0.6
        return Case(name, _features(rng, dad), ncm, np.hstack([-np.inf, np.linspace(6.0, 31.0, 6), np.inf]), 2048, seed)
    if name == "whole_partitions":
        # counts 0, 1, 2, want - 1, want, want + 1 (the first that is chosen by key) and two large ones; pair 0 is the
        # partition of one, pair n - 1 in the partition of two
        return _whole_partitions(n, rng, [0, 1, 2, 49, 50, 51, None, None], 50, seed, name)
    if name == "sort_sizes":
        # lists around the padded sort sizes P (64, 128, 1024, 2048, 4096) and Q (64, 128, 1024, 2048): whole partitions of
        # 63 .. 1025 members, 3136 members under want = 2048 (the largest population whose threshold is all ones), and
        # w = 64 and 65 out of sampled lists
        return _whole_partitions(n, rng, [63, 64, 65, 1024, 1025, 3136, None, None], [2048] * 6 + [64, 65], seed, name)
    if name == "small_partitions_last":
        # eight large partitions with thresholds near 3 % of the key range, then four small ones taken whole or nearly: the
        # largest threshold -- above which k_hs_collect drops a pair before looking its partition up -- belongs to the last ones
        return _whole_partitions(n, rng, [None] * 8 + [30, 150, 400, 1000], 100, seed, name)
    if name == "finite_outer_edges":
        dad = _halfint(rng, n)
        dad[rng.rand(n) < 0.01] = np.nan
        dad[rng.randint(0, n, 40)] = np.inf
        dad[rng.randint(0, n, 40)] = -np.inf
        dad[0], dad[n - 1] = np.nan, 55.0     # (the last finite edge itself is outside)
        return Case(name, _features(rng, dad), rng.rand(n) < 0.6, [5.0, 12.5, 20.0, 27.5, 35.0, 42.5, 50.0, 55.0], 100, seed)
    if name == "under_declared":
        # fewer declared than there are (a stale count): min(want, declared) of them, by key, in one attempt
        dad = _halfint(rng, n)
        ncm = rng.rand(n) < 0.006
        c = Case(name, _features(rng, dad), ncm, _halfint_edges(7), 100, seed)
        c.declared = np.minimum(c.true, 40)
        return c
    if name in ("cap_exactly_full", "cap_plus_one"):
        # one partition over everything, declared 3136 under want = 2048: the threshold is all ones and the list takes every
        # member.  4096 members fill it to the brim (accepted); 4097 overflow it, and the halved threshold keeps the 2100 of
        # them whose key lies in the lower half of the range (chosen that way: a second attempt that settles)
        dad = _halfint(rng, n)
        keys = keys_of(seed, n)
        low = rng.permutation(np.flatnonzero(keys <= np.uint64(M64 // 2)))
        high = rng.permutation(np.flatnonzero(keys > np.uint64(M64 // 2)))
        members = 4096 if name == "cap_exactly_full" else 4097
        ncm = np.zeros(n, dtype=bool)
        ncm[low[:2100]] = True
        ncm[high[:members - 2100]] = True
        return Case(name, _features(rng, dad), ncm, [-np.inf, np.inf], 2048, seed, declared=[3136],
                    attempts=1 if name == "cap_exactly_full" else 2)
    if name in ("declared_x16", "declared_div24", "declared_x4096"):
        dad = _halfint(rng, n)
        c = Case(name, _features(rng, dad), rng.rand(n) < 0.6, _halfint_edges(7), 100, seed)
        if name == "declared_x16":        # ~13 keys under the first threshold where 100 are wanted: it doubles until they are
            c.declared, c.attempts = c.true * 16, (2, 7)
        elif name == "declared_div24":    # ~5100 keys under it: the list overflows, one halving settles
            c.declared, c.attempts = np.maximum(c.true // 24, 150), 2
        else:                             # 2^7 doublings short of the wanted number
            c.declared, c.attempts = c.true * 4096, "refused"
        return c
    raise KeyError(name)
