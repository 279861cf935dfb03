"""Adversarial row states for the workgroup-per-row selections (csrc/rowsel.h: k_row_thresh, k_gn_lists, k_get_nn), host only.

build_case() writes, through the CSR index, a chosen value layout into a few TARGET rows of a complete pair list and plain
random values everywhere else; the layouts decide on purpose which way a row goes through the kernels:

    too_many      the sampled threshold t0 lets more than ROWC_CAP entries through  -> radix descent
    too_few       fewer than `want` eligible entries reach t0                      -> radix descent
    shrink_short  the second, 64-sample cut keeps fewer than `want` candidates     -> radix descent
    fast          both cuts keep at least `want`                                   -> ranked inside LDS

Beside the data the module restates the sampling rule of rowsel.h in NumPy (first_cut, shrink_cut, row_branch and the three
kernels' parametrisations of it), so that tests/test_row_paths_cases.py can assert on the CPU that a layout takes the branch
it was built for.  That is a statement about the INPUTS; the kernels are compared with the oracle in test_row_paths_gpu.py.

One thing the restatement has to assume: the candidate buffer is filled through an LDS atomic counter, so its order is the
hardware's.  The shrink samples buffer positions, hence `shrink_short` is predicted under the model "candidates sit in slot
order".  In the 1300-entry class the shrink_too_tight layout keeps every candidate in slots that ONE wavefront visits (slot mod
256 < 64), where program order (trip by trip, lanes ascending) is slot order; in the 700-entry class every entry is a
candidate and four wavefronts interleave, so there the model is only the likeliest order.  Correctness never depends on it.
"""
import numpy as np

ROW_THREADS = 256
ROWC_CAP = 1024
SHRINK_MIN = 128
KEY_LAST = np.uint64(0xFFFFFFFFFFFFFFFF)

CLASSES = {"long": 1301, "mid": 701, "short": 97}   # nx; rows of nx - 1 entries.  None is a multiple of 8 (row_of_block's bands)
CASES = ("sample_sees_large", "sample_sees_small", "ties_on_cut", "all_equal", "integer_halves", "narrow_ulps", "with_marks",
         "sorted_ascending", "sorted_descending", "shrink_too_tight")
MASKS = ("all", "random70", "row_counts")
BRANCHES = ("too_many", "too_few", "fast", "shrink_short")


def points(cls):
    """nx float64 points of 2 coordinates (fixed seed)."""
    return np.random.default_rng(CLASSES[cls]).standard_normal((CLASSES[cls], 2))


def target_rows(nx):
    """First, middle and last row, two adjacent pairs, three random rows; in the order in which they claim shared pairs."""
    fixed = [0, 1, nx // 2, nx // 2 + 1, nx - 1]
    rng = np.random.default_rng(nx + 1)
    rest = [int(r) for r in rng.permutation(np.arange(3, nx - 3)) if all(abs(int(r) - f) > 1 for f in fixed)][:3]
    return fixed + rest


def sample_slots(n):
    return (np.arange(ROW_THREADS, dtype=np.int64) * n) // ROW_THREADS


def shrink_slots(c):
    return (np.arange(64, dtype=np.int64) * c) >> 6


def first_rank(want, n):
    """r of row_candidates: t0 is the sample's r-th smallest key (0-based)."""
    return int((3 * want * ROW_THREADS + n - 1) // n) + 3


def shrink_rank(want, c):
    return int((3 * want * 64 + c - 1) // c) + 2


def key_asc(v):
    """The kernels' order-preserving uint64 key of a float64 (a zero's sign dropped first, as row_key_asc does)."""
    u = (np.asarray(v, dtype=np.float64) + 0.0).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


# ------------------------------------------------------------------------------------------- the sampling rule, restated
def first_cut(keys, elig, want):
    """row_candidates: slots of the eligible entries with key <= t0, or None when there are more than ROWC_CAP."""
    n = keys.shape[0]
    t0 = KEY_LAST
    if n > ROWC_CAP:
        s0 = sample_slots(n)
        samp = np.where(elig[s0], keys[s0], KEY_LAST)
        r = first_rank(want, n)
        if r < ROW_THREADS:
            t0 = samp[np.argsort(samp, kind="stable")[r]]
    slots = np.flatnonzero(elig & (keys <= t0))
    return None if slots.size > ROWC_CAP else slots


def shrink_cut(ckeys, want, shrink_min=SHRINK_MIN):
    """row_cand_shrink on the candidate keys in buffer order: how many stay."""
    c = ckeys.shape[0]
    if c <= shrink_min or c > ROWC_CAP:
        return c
    r2 = shrink_rank(want, c)
    if r2 >= 64:
        return c
    t1 = np.sort(ckeys[shrink_slots(c)])[r2]
    return int((ckeys <= t1).sum())


def row_branch(keys, elig, want, shrink_min=SHRINK_MIN):
    slots = first_cut(keys, elig, want)
    if slots is None:
        return "too_many"
    if slots.size < want:
        return "too_few"
    if shrink_cut(keys[slots], want, shrink_min) < want:
        return "shrink_short"
    return "fast"


def _row(RA, ncm, I_ptr, I_idx, i):
    pos = I_idx[I_ptr[i]:I_ptr[i + 1]]
    return RA[pos], ncm[pos].astype(bool)


def thresh_branch(RA, ncm, I_ptr, I_idx, i, n_neighbors, shrink_min=SHRINK_MIN):
    """k_row_thresh: every entry eligible, want = min(n_neighbors, len - 1) + 1."""
    v, _ = _row(RA, ncm, I_ptr, I_idx, i)
    return row_branch(key_asc(v), np.ones(v.shape[0], dtype=bool), min(n_neighbors, v.shape[0] - 1) + 1, shrink_min)


def gn_branch(RA, ncm, I_ptr, I_idx, i, nmin, shrink_min=SHRINK_MIN):
    """k_gn_lists: the not-computed entries are eligible, the sample is taken with L = nmin + 1, the list wants min(L, n_unc)."""
    v, u = _row(RA, ncm, I_ptr, I_idx, i)
    L, keys = nmin + 1, key_asc(v)
    want = min(L, int(u.sum()))
    if want == 0:
        return "empty"
    slots = first_cut(keys, u, L)
    if slots is None:
        return "too_many"
    if slots.size < want:
        return "too_few"
    return "shrink_short" if shrink_cut(keys[slots], want, shrink_min) < want else "fast"


def graph_branch(RA, ncm, I_ptr, I_idx, i, nn, shrink_min=SHRINK_MIN):
    """k_get_nn: (pass, branch).  Pass 0 ranks the computed entries alone and is final when the row has nn - 1 of them, no
    not-computed entry <= 0 and both cuts keep enough; otherwise pass 1 keys every entry by RA (+ row maximum if not computed)."""
    v, u = _row(RA, ncm, I_ptr, I_idx, i)
    want = min(nn - 1, v.shape[0])
    b0 = row_branch(key_asc(v), ~u, want, shrink_min)
    if b0 == "fast" and int((~u).sum()) >= want and not (u & ~(v > 0.0)).any():
        return 0, "fast"
    with np.errstate(invalid="ignore"):
        d = np.where(u, v + v.max(), v)
    return 1, row_branch(key_asc(d), np.ones(v.shape[0], dtype=bool), want, shrink_min)


# -------------------------------------------------------------------------------------------------------------- layouts
def _distinct(rng, m, lo, hi):
    """m distinct values in (lo, hi), shuffled."""
    return rng.permutation(lo + (hi - lo) * (np.arange(m) + rng.random(m) * 0.5 + 0.25) / max(m, 1))


def tie_variant(n, t, want):
    """Size of the tie group on the cut for target number t -- (a) 3, (b) about 300, (c) more than ROWC_CAP, scaled down where
    the row is shorter -- and which member of the group the cut falls on (first, middle, last)."""
    g = (3, min(300, (2 * n) // 5), min(1100, (5 * n) // 6))[t % 3]
    g = min(g, n - want - 5)                 # room for the `want` smaller values of the "last member" variant
    return g, (0, g // 2, g - 1)[(t // 3) % 3]


def _layout(case, n, want, t, rng):
    if case == "sample_sees_large":
        # the sample slots hold the largest values; the n - 256 distinct smaller ones (1044 of 1300) all pass t0
        v = _distinct(rng, n, 1.0, 2.0)
        if n > ROWC_CAP:
            s0 = sample_slots(n)
            v[s0] = _distinct(rng, s0.size, 1000.0, 2000.0)
        return v
    if case == "sample_sees_small":
        # the sample slots hold the smallest values: exactly r + 1 entries reach t0, fewer than want once want >= 16
        v = _distinct(rng, n, 1000.0, 2000.0)
        if n > ROWC_CAP:
            s0 = sample_slots(n)
            v[s0] = _distinct(rng, s0.size, 1.0, 2.0)
        return v
    if case == "ties_on_cut":
        g, off = tie_variant(n, t, want)
        below = max(0, want - 1 - off)          # the want-th smallest is member `off` of the group
        tie = ((np.arange(g) + 0.5) * n / g).astype(np.int64)   # spread over the slot range: the tie loop ends in a later trip
        rest = np.setdiff1d(np.arange(n), tie)
        rest = rng.permutation(rest)
        v = np.full(n, 5.0)
        v[rest[:below]] = _distinct(rng, below, 1.0, 4.0)
        v[rest[below:]] = _distinct(rng, rest.size - below, 6.0, 9.0)
        return v
    if case == "all_equal":
        return np.full(n, 2.5)
    if case == "integer_halves":
        return rng.integers(0, 40, n) / 2.0
    if case == "narrow_ulps":
        return (np.full(n, 1.5).view(np.uint64) + rng.integers(0, 1 << 20, n).astype(np.uint64)).view(np.float64)
    if case == "with_marks":
        # what guarantee_nmin leaves (-1.0: negative keys), some +inf, and a -0.0 one slot AFTER a +0.0: to NumPy the two are
        # equal and the earlier slot wins; a key that orders -0.0 first would swap them
        v = _distinct(rng, n, 0.5, 9.0)
        v[rng.permutation(n)[: n // 4]] = -1.0
        free = np.flatnonzero(v > 0)
        v[free[[3, free.size // 2, free.size - 2]]] = np.inf
        a = int(free[free.size // 3])
        v[a] = 0.0
        v[min(a + 1, n - 1)] = -0.0
        return v
    if case == "sorted_ascending":
        return np.sort(_distinct(rng, n, 1.0, 9.0))
    if case == "sorted_descending":
        return np.sort(_distinct(rng, n, 1.0, 9.0))[::-1].copy()
    if case == "shrink_too_tight":
        v = _distinct(rng, n, 1000.0, 2000.0)
        if n > ROWC_CAP:
            # candidates only in the slots of wavefront 0 (slot mod 256 < 64): its r + 1 lowest sample slots A carry t0, its
            # other sample slots stay large, everything else it visits lies below t0
            r = first_rank(want, n)
            s0 = sample_slots(n)
            w0 = np.flatnonzero(np.arange(n) % ROW_THREADS < 64)
            s0w = s0[np.isin(s0, w0)]
            A = s0w[: r + 1]
            cand = np.setdiff1d(w0, s0w[r + 1:])           # buffer order = slot order
        else:
            cand = np.arange(n)                            # no sampling: every entry is a candidate
            A = cand[:0]
        c = cand.size
        hit = cand[shrink_slots(c)]                        # what the 64 shrink samples read
        other = np.setdiff1d(cand, hit)
        v[hit] = _distinct(rng, hit.size, 1.0, 2.0)        # the 64 smallest: t1 is the r2-th of them, r2 + 1 survive
        v[other] = _distinct(rng, other.size, 10.0, 20.0)
        if A.size:
            top = [a for a in A if a not in set(hit.tolist())][-1]
            v[top] = 30.0                                  # t0: the largest of A, above every other candidate
        return v
    raise ValueError(case)


def row_count_plan(nx, nmin):
    """{target row: number of computed entries} of the "row_counts" mask; -1: all computed but nmin - 1 entries (fewer not-computed
    entries than the list length L = nmin + 1)."""
    rows = target_rows(nx)
    return {rows[0]: nmin - 1, rows[1]: nmin, rows[2]: 0, rows[3]: -1, rows[4]: nmin - 1, rows[5]: 0}


def _mask(mask, I_ptr, I_idx, nx, n, nmin, rng):
    if mask == "all":
        return np.ones(n, dtype=np.uint8)
    if mask == "random70":
        return (rng.random(n) < 0.7).astype(np.uint8)
    assert mask == "row_counts"
    ncm = np.ones(n, dtype=np.uint8)
    rows = target_rows(nx)
    shared = np.zeros(n, dtype=bool)     # pairs between two target rows stay not computed
    seen = np.zeros(n, dtype=np.int8)
    for i in rows:
        seen[I_idx[I_ptr[i]:I_ptr[i + 1]]] += 1
    shared[seen > 1] = True
    for i, cnt in row_count_plan(nx, nmin).items():
        pos = I_idx[I_ptr[i]:I_ptr[i + 1]]
        own = rng.permutation(pos[~shared[pos]])
        assert own.size + len(rows) - 1 == pos.size
        if cnt < 0:
            keep = nmin - 1 - (len(rows) - 1)            # not-computed entries besides the shared ones
            assert keep >= 0 and pos.size - (nmin - 1) >= nmin
            ncm[own[keep:]] = 0
        else:
            assert cnt <= own.size
            ncm[own[:cnt]] = 0
    return ncm


def build_case(I_ptr, I_idx, IJs, cls, case, want=21, mask="all", nmin=30, seed=0):
    """(RA float64 [n], ncm uint8 [n]) for the whole pair list: target rows laid out for `case`, built for a selection of the
    `want` smallest; every other pair plain random.  A pair that two target rows share keeps the first row's value."""
    nx = CLASSES[cls]
    I_ptr, I_idx = np.asarray(I_ptr, dtype=np.int64), np.asarray(I_idx, dtype=np.int64)
    n = np.asarray(IJs).reshape(-1, 2).shape[0]
    assert I_ptr.shape[0] == nx + 1 and n == nx * (nx - 1) // 2 and I_idx.shape[0] == 2 * n
    rng = np.random.default_rng([seed, nx, CASES.index(case), want])
    RA = 1.0 + 9.0 * rng.random(n)
    claimed = np.zeros(n, dtype=bool)
    for t, i in enumerate(target_rows(nx)):
        pos = I_idx[I_ptr[i]:I_ptr[i + 1]]
        assert pos.size == nx - 1
        v = _layout(case, pos.size, want, t, rng)
        free = ~claimed[pos]
        RA[pos[free]] = v[free]
        claimed[pos] = True
    ncm = _mask(mask, I_ptr, I_idx, nx, n, nmin, np.random.default_rng([seed, nx, MASKS.index(mask)]))
    return RA, ncm


def complete_index(nx):
    """(I_ptr, I_idx, IJs) of the complete pair list as the library lays it out (pairs (i, j), i < j, row-major; row i lists
    its pairs by the other endpoint ascending) -- for the CPU tests, which have no engine to download it from."""
    iu = np.triu_indices(nx, k=1)
    IJs = np.stack(iu, axis=1).astype(np.int64)
    n = IJs.shape[0]
    P = np.zeros((nx, nx), dtype=np.int64)
    P[iu] = np.arange(n)
    P = P + P.T
    off = ~np.eye(nx, dtype=bool)
    I_idx = P[off].reshape(nx, nx - 1).reshape(-1)
    I_ptr = np.arange(nx + 1, dtype=np.int64) * (nx - 1)
    return I_ptr, I_idx, IJs
