"""States for update_bounds (csrc/refine.hip: the computed-neighbour CSR kernels, k_update_bounds<G>, k_update_bounds_bits) that
put its kernels on the edges they were written for, and an exact host reference; host only.

update_bounds_ref() restates O.update_bounds on arrays: the computed neighbours of every point as one sorted CSR, every lookahead
pair's shorter list looked up in the other's by one np.searchsorted over (owner * nx + neighbour).  Each candidate bound is one
IEEE addition, or one subtraction and a fabs, of two stored doubles, and min / max do not depend on the order: the result is
bit-identical to O.update_bounds (tests/test_refine_cases.py asserts it) and to what the kernels must leave.

build_case() lays out, on a given index, the mask, RefineApprox and the feature rows of one named case together with the
parameters of the select_candidates call that produces the lookahead list (it cannot be uploaded).  The not-computed entries
of RefineApprox have no part in update_bounds, so they steer the selection: 2^-6 .. 2^-5 on the pairs the case wants in the
list, 10^6 on the others; with n_neighbors beyond every row's length a row's threshold is its largest entry, a wanted pair
gets probability 1 and any other 0 (the one residual list is [0.0]), and n_refine = 1 with lookahead = the number of wanted
pairs lists the wanted pairs but the one that becomes the candidate.  check_case() asserts on the list that was really
produced (on the GPU: the downloaded one) that the case still has the property it is named for.

    empty_lists      points without any computed neighbour, as first point and as partner; non-empty lists without a common key
    match_ends       matches at the first and the last position of both lists; lists of equal length
    tail_groups      a list length that is no multiple of 4 (nor of 8 or 16): dead groups in the last workgroup
    csr_edges        computed entries on the positions the vectorised CSR kernels split a row on, each the only common
                     neighbour of one lookahead pair (a dropped or displaced entry changes a bound)
    past_stage_G     longer lists of exactly 16 G, 16 G + 1 and more entries (G lanes per pair keep 16 G keys in LDS)
    list_steps       partner lists of 0, 1, 511, 512, 513, 1024 and more entries, lengths that are no multiples of 4
    run_rebuild      three and more runs of different first points in one 2048-entry chunk, one run across the chunk's end
    long_run         one run of more than 512 pairs
    dense_matches    more than 64 matches inside one 512-entry step, more than 128 in two consecutive ones
    high_keys        just above 65 536 points on a thinned list: lists below, above and across the 2-byte keys' split
"""
from types import SimpleNamespace

import numpy as np

from oracle import annchor_oracle as O

# points per fixture.  1129: room for a 1061-entry list, the points it is paired with and spare hubs.  69 632 = 65 536 + 4096: a
# point's ~140 candidates are spread over the index range, so 6 % of the points above the split is what gives most lists a few keys
# and most lookahead pairs a match up there
SMALL, MID, HIGH = 97, 1129, 69632
SMALL_CASES = ("empty_lists", "match_ends", "tail_groups", "csr_edges")
MID_CASES = ("past_stage_16", "past_stage_32", "past_stage_64", "list_steps", "run_rebuild", "long_run", "dense_matches")
HIGH_CASES = ("high_keys",)
CASES = SMALL_CASES + MID_CASES + HIGH_CASES
SIZES = dict([(c, SMALL) for c in SMALL_CASES] + [(c, MID) for c in MID_CASES] + [(c, HIGH) for c in HIGH_CASES])
FORMS = ("pairs16", "pairs32", "pairs", "bits16", "bits32", None)     # ANNCHOR_UPDATE_BOUNDS; None: the dispatcher's choice
ONE_LIST = [np.array([0.0])]
SPLIT = 65536
CHUNK, STEP, RUN_ROUND = 2048, 512, 512      # UBB_CHUNK; keys per step (8 per lane); pairs per round of a workgroup's eight waves


# ------------------------------------------------------------------------------------------------------------ the index
class Index:
    def __init__(self, I_ptr, I_idx, IJs):
        self.ptr = np.asarray(I_ptr, dtype=np.int64)
        self.idx = np.asarray(I_idx, dtype=np.int64)
        self.IJs = np.asarray(IJs, dtype=np.int64).reshape(-1, 2)
        self.nx, self.n = self.ptr.shape[0] - 1, self.IJs.shape[0]
        self.key = self.IJs[:, 0] * self.nx + self.IJs[:, 1]
        assert (np.diff(self.key) > 0).all() and (self.IJs[:, 0] < self.IJs[:, 1]).all()

    def pos(self, a, b):
        """Pair-list positions of the pairs {a, b} (arrays), which must be in the list."""
        a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
        k = np.minimum(a, b) * self.nx + np.maximum(a, b)
        p = np.minimum(np.searchsorted(self.key, k), self.n - 1)
        assert (self.key[p] == k).all(), "pair not in the list"
        return p


class Lists:
    """The computed neighbours of every point: ptr [nx + 1], idx (neighbours, ascending per point), pos (their pairs)."""

    def __init__(self, ix, ncm):
        owner = np.repeat(np.arange(ix.nx, dtype=np.int64), np.diff(ix.ptr))
        comp = np.asarray(ncm)[ix.idx] == 0
        pos, own = ix.idx[comp], owner[comp]
        pr = ix.IJs[pos]
        other = np.where(pr[:, 0] == own, pr[:, 1], pr[:, 0])
        o = np.lexsort((other, own))
        self.nx, self.idx, self.pos = ix.nx, other[o], pos[o]
        self.key = own[o] * ix.nx + self.idx
        self.ptr = np.zeros(ix.nx + 1, dtype=np.int64)
        np.cumsum(np.bincount(own, minlength=ix.nx), out=self.ptr[1:])
        self.len = np.diff(self.ptr)

    def of(self, y):
        return self.idx[self.ptr[y]:self.ptr[y + 1]]

    def hits(self, a, b, budget=1 << 22):
        """Every common neighbour of the pairs (a[t], b[t]), found by walking a[t]'s list: yields (t, entry of a[t]'s list,
        entry of b[t]'s list) in batches, t ascending."""
        la = self.len[a]
        cum = np.cumsum(la)
        start = 0
        while start < a.shape[0]:
            base = cum[start - 1] if start else 0
            stop = max(int(np.searchsorted(cum, base + budget, side="right")), start + 1)
            l = la[start:stop]
            tot = int(l.sum())
            if tot and self.key.shape[0]:
                seg = np.repeat(np.arange(start, stop, dtype=np.int64), l)
                e = self.ptr[a][seg] + (np.arange(tot, dtype=np.int64) - np.repeat(np.cumsum(l) - l, l))
                k = b[seg] * self.nx + self.idx[e]
                loc = np.minimum(np.searchsorted(self.key, k), self.key.shape[0] - 1)
                hit = self.key[loc] == k
                yield seg[hit], e[hit], loc[hit]
            start = stop


def update_bounds_ref(IJs, RA, ncm, I_ptr, I_idx, nxt, lb, ub):
    """O.update_bounds, vectorised: (lb, ub) after tightening the pairs of `nxt` by their common computed neighbours."""
    ix = I_ptr if isinstance(I_ptr, Index) else Index(I_ptr, I_idx, IJs)
    L = Lists(ix, ncm)
    val = np.asarray(RA, dtype=np.float64)[L.pos]
    lb, ub = np.array(lb, dtype=np.float64), np.array(ub, dtype=np.float64)
    nxt = np.asarray(nxt, dtype=np.int64)
    i, j = ix.IJs[nxt, 0], ix.IJs[nxt, 1]
    swap = L.len[i] > L.len[j]
    for seg, ea, eb in L.hits(np.where(swap, j, i), np.where(swap, i, j)):
        if seg.shape[0] == 0:
            continue
        x, y = np.where(swap[seg], val[eb], val[ea]), np.where(swap[seg], val[ea], val[eb])     # (x: the first point's value)
        first = np.flatnonzero(np.r_[True, seg[1:] != seg[:-1]])
        t = nxt[seg[first]]
        ub[t] = np.minimum(ub[t], np.minimum.reduceat(x + y, first))
        lb[t] = np.maximum(lb[t], np.maximum.reduceat(np.abs(x - y), first))
    return lb, ub


def host_next(ix, RA, ncm, sel):
    """The lookahead list of select_candidates(k, 0, [[0.0]], n_refine, lookahead) by the oracle (k beyond every row: a row's
    threshold is its largest entry)."""
    k, n_refine, lookahead = sel
    assert np.diff(ix.ptr).min() > 0 and k >= np.diff(ix.ptr).max()
    thr = np.maximum.reduceat(RA[ix.idx], ix.ptr[:-1])
    u = ncm.astype(bool)
    unc = np.flatnonzero(u)
    prob = O.refine_probabilities(RA, u, ix.IJs, thr, np.zeros(ix.n, dtype=np.int64), ONE_LIST)
    return unc[O.select_candidates(prob, n_refine, lookahead, positions=unc)[1]]


# ------------------------------------------------------------------------------------------------------------ the cases
def _values(rng, n):
    return 0.5 + 9.0 * rng.random(n)


def _finish(ix, name, rng, ncm, wanted, sel_all=False, info=None):
    """RefineApprox, the feature rows and the selection of a case whose mask and wanted lookahead pairs (positions; None: every
    not-computed pair) are chosen."""
    n, nx = ix.n, ix.nx
    RA = _values(rng, n)
    L = Lists(ix, ncm)
    # special values on common neighbours of wanted pairs, each kind on three pairs: equal on both sides (difference exactly
    # 0), 0.0 on one side, 0.0 on both (sum exactly 0), a subnormal
    unc = np.flatnonzero(ncm)
    wpos = unc if wanted is None else np.asarray(wanted, dtype=np.int64)
    special, used = [], set()
    for t in wpos[rng.permutation(wpos.shape[0])[:4000]]:
        i, j = ix.IJs[t]
        both = np.intersect1d(L.of(i), L.of(j))
        both = [c for c in both if (i, c) not in used and (j, c) not in used]
        if not both:
            continue
        c = int(both[len(both) // 2])
        kind = len(special) % 4
        pi, pj = ix.pos([i], [c])[0], ix.pos([j], [c])[0]
        if kind == 0:
            RA[pj] = RA[pi]
        elif kind == 1:
            RA[pi] = 0.0
        elif kind == 2:
            RA[pi] = RA[pj] = 0.0
        else:
            RA[pj] = 5e-324
        used.update([(i, c), (c, i), (j, c), (c, j)])
        special.append((int(t), kind))
        if len(special) == 12:
            break
    assert len(special) == 12, "no room for the special values"
    # the not-computed entries steer the selection
    if sel_all:
        RA[unc] = 0.015625 * (1.0 + rng.random(unc.shape[0]))
        sel = (int(np.diff(ix.ptr).max()) + 5, n, 1)                 # n_refine >= the not-computed pairs: every one is listed
    else:
        RA[unc] = 1.0e6
        RA[wpos] = 0.015625 * (1.0 + rng.random(wpos.shape[0]))
        sel = (int(np.diff(ix.ptr).max()) + 5, 1, int(wpos.shape[0]))
    # bounds: loose on both sides, lb0 above every |x - y| (values <= 9.5), ub0 below every x + y (>= 1 but for the zeros)
    cls = rng.integers(0, 4, n)
    lb0 = np.where(cls & 1, 20.0 + rng.random(n), 0.01 * rng.random(n))
    ub0 = np.where(cls & 2, 1.0e-3 * rng.random(n), 1000.0 + rng.random(n))
    feats = np.stack([lb0, ub0, rng.random(n) * 7.0, (rng.random(n) < 0.1).astype(np.float64)], axis=1)
    return SimpleNamespace(name=name, nx=nx, RA=RA, ncm=ncm, feats=feats, sel=sel, wanted=wpos, special=special,
                           info=info or {})


def _mask_of_lists(ix, lists):
    """Mask with exactly the pairs {y, c}, c in lists[y], computed."""
    ncm = np.ones(ix.n, dtype=np.uint8)
    for y, cs in lists.items():
        if len(cs):
            ncm[ix.pos(np.full(len(cs), y), cs)] = 0
    return ncm


def _pairs(ix, firsts, partners):
    f, p = np.meshgrid(np.asarray(firsts), np.asarray(partners), indexing="ij")
    assert (f < p).all()
    return ix.pos(f.ravel(), p.ravel())


def _roles(nx, rng, n_first, n_partner):
    """Random points in three roles: first points (all below the partners), partners, and hubs (everything else) that the
    computed lists are drawn from."""
    s = np.sort(rng.choice(nx, n_first + n_partner, replace=False))
    return s[:n_first], s[n_first:], np.setdiff1d(np.arange(nx), s)


def _designed(ix, name, rng, flen, plen, common=None, background=0.0):
    """First points with lists of flen[] hubs, partners with plen[] hubs, every (first, partner) wanted.  background: the share of the pairs between two hubs that is computed as well -- no part of any wanted
    pair's lists, but the mean list length the dispatcher chooses the form by."""
    F, P, H = _roles(ix.nx, rng, len(flen), len(plen))
    lists = {}
    for y, l in zip(np.r_[F, P], list(flen) + list(plen)):
        lists[int(y)] = np.sort(rng.choice(H, l, replace=False))
    if common is not None:
        common(lists, F, P, H)
    ncm = _mask_of_lists(ix, lists)
    if background:
        hub = np.zeros(ix.nx, dtype=bool)
        hub[H] = True
        ncm[hub[ix.IJs[:, 0]] & hub[ix.IJs[:, 1]] & (rng.random(ix.n) < background)] = 0
    return _finish(ix, name, rng, ncm, np.sort(_pairs(ix, F, P)), info=dict(F=F, P=P))


def build_case(I_ptr, I_idx, IJs, name, seed=0):
    ix = I_ptr if isinstance(I_ptr, Index) else Index(I_ptr, I_idx, IJs)
    nx, n = ix.nx, ix.n
    rng = np.random.default_rng([seed, CASES.index(name)])
    if name in SMALL_CASES:
        assert n == nx * (nx - 1) // 2 and nx >= 90
    if name == "empty_lists":
        M = np.triu(rng.random((nx, nx)) < 0.3, 1)
        M = M | M.T
        E = np.array([0, 1, nx // 2, nx - 2, nx - 1] + [int(v) for v in rng.choice(np.arange(5, nx - 5), 3, replace=False)])
        u, v = [int(y) for y in np.setdiff1d(np.arange(3, nx - 3), E)[[4, 9]]]
        M[E, :] = M[:, E] = False
        M[u, 1::2] = M[1::2, u] = False        # u keeps even neighbours, v odd ones
        M[v, 0::2] = M[0::2, v] = False
        M[u, v] = M[v, u] = False
        ncm = (~M[ix.IJs[:, 0], ix.IJs[:, 1]]).astype(np.uint8)
        return _finish(ix, name, rng, ncm, None, sel_all=True, info=dict(E=E, uv=(min(u, v), max(u, v))))
    if name == "match_ends":
        M = np.triu(rng.random((nx, nx)) < 0.25, 1)
        M = M | M.T
        # (a, b): equal lengths, (c, d): 9 and 23 entries; both pairs share their lists' first and last key
        a, b, c, d = 10, 40, 11, 70
        sp = np.array([a, b, c, d])
        M[sp, :] = M[:, sp] = False
        rest = np.setdiff1d(np.arange(nx), sp)
        lists = {}
        for (p, q, lp, lq) in ((a, b, 14, 14), (c, d, 9, 23)):
            lo, hi = int(rest[2]), int(rest[-3])
            mid = rest[3:-3]
            lists[p] = np.r_[lo, np.sort(rng.choice(mid, lp - 2, replace=False)), hi]
            lists[q] = np.r_[lo, np.sort(rng.choice(mid, lq - 2, replace=False)), hi]
        for y, cs in lists.items():
            M[y, cs] = M[cs, y] = True
        ncm = (~M[ix.IJs[:, 0], ix.IJs[:, 1]]).astype(np.uint8)
        return _finish(ix, name, rng, ncm, None, sel_all=True, info=dict(pairs=((a, b), (c, d))))
    if name == "tail_groups":
        ncm = (rng.random(n) < 0.6).astype(np.uint8)
        while int(ncm.sum()) % 16 != 5:        # 5 mod 16: 3 of 4, 3 of 8 and 11 of 16 groups of the last workgroup are dead
            ncm[np.flatnonzero(ncm)[int(rng.integers(0, int(ncm.sum())))]] = 0
        return _finish(ix, name, rng, ncm, None, sel_all=True)
    if name == "csr_edges":
        return _csr_edges(ix, name, rng)
    assert n == nx * (nx - 1) // 2 or name == "high_keys"
    if name.startswith("past_stage"):
        S = 16 * int(name.rsplit("_", 1)[1])
        assert nx >= S + 80
        # (mean list lengths of ~2, ~220 and ~390: the dispatcher takes 16 lanes per pair, 32, and the row-grouped form)
        return _designed(ix, name, rng, [S, S + 1, S + 37, 10, S - 1], [S, S + 1, S + 33, 7, max(S // 2, 9), S],
                         background={256: 0.0, 512: 0.2, 1024: 0.35}[S])
    if name == "list_steps":
        return _designed(ix, name, rng, [300, 1025, 5, 0], [0, 1, 3, 510, 511, 512, 513, 1023, 1024, 1025, 1030],
                         background=0.35)
    if name in ("run_rebuild", "long_run"):
        runs = (700, 500, 300, 900, 400, 200) if name == "run_rebuild" else (600, 10)
        F, P, H = _roles(nx, rng, len(runs), max(runs))
        lists = {}
        w = H.shape[0] // 2
        for t, f in enumerate(F):               # half of a window of the hubs that slides with the first point
            lo = t * (H.shape[0] - w) // (len(runs) - 1)
            lists[int(f)] = np.sort(rng.choice(H[lo:lo + w], w // 2, replace=False))
        for p in P:
            lists[int(p)] = np.sort(rng.choice(H, int(rng.integers(0, 120)), replace=False))
        ncm = _mask_of_lists(ix, lists)
        wanted = np.concatenate([_pairs(ix, [f], np.sort(rng.choice(P, r, replace=False))) for f, r in zip(F, runs)])
        return _finish(ix, name, rng, ncm, np.sort(wanted), info=dict(F=F, P=P))
    if name == "dense_matches":
        def common(lists, F, P, H):
            # partners 0 .. 11 take 600 of the first list's 700 keys and 300 others: ~340 matches per 512-entry step
            for p in P[:12]:
                lists[int(p)] = np.sort(np.r_[rng.choice(lists[int(F[0])], 600, replace=False),
                                              rng.choice(np.setdiff1d(H, lists[int(F[0])]), 300, replace=False)])
        return _designed(ix, name, rng, [700, 40], [0] * 12 + [30, 200, 5, 64, 90, 11, 300, 2], common=common,
                         background=0.35)
    if name == "high_keys":
        assert SPLIT < nx <= 2 * SPLIT and n < nx * (nx - 1) // 2
        role = rng.random(nx)
        above_only, below_only = role < 0.04, (role >= 0.04) & (role < 0.08)
        i, j = ix.IJs[:, 0], ix.IJs[:, 1]
        comp = rng.random(n) < 0.5
        comp &= ~(above_only[i] & (j < SPLIT)) & ~(above_only[j] & (i < SPLIT))
        comp &= ~(below_only[i] & (j >= SPLIT)) & ~(below_only[j] & (i >= SPLIT))
        ncm = (~comp).astype(np.uint8)
        wanted = np.sort(rng.choice(np.flatnonzero(ncm), 30000, replace=False))
        return _finish(ix, name, rng, ncm, wanted, info=dict(above_only=above_only, below_only=below_only))
    raise ValueError(name)


# ---------------------------------------------------------------------------------------- rows of the vectorised CSR kernels
def _row_geometry(ix, r):
    """(low, head of the column half, head of the row half) of row r as k_comp_*_direct see it: the column half's flags start
    at byte Iptr[r] - rowstart[r] of the column-ordered copy, the row half's at byte rowstart[r] of the mask (both buffers are
    16-byte aligned); head = entries in front of the first 16-byte boundary."""
    others = np.where(ix.IJs[ix.idx[ix.ptr[r]:ix.ptr[r + 1]], 0] == r, ix.IJs[ix.idx[ix.ptr[r]:ix.ptr[r + 1]], 1],
                      ix.IJs[ix.idx[ix.ptr[r]:ix.ptr[r + 1]], 0])
    low = int((others < r).sum())
    rowstart = int(np.searchsorted(ix.IJs[:, 0], r))
    return others, low, (-(int(ix.ptr[r]) - rowstart)) % 16, (-rowstart) % 16


def marked_entries(ix, rows):
    """{(row, slot)}: the row's first and last entry, the last of its column half and the first of its row half, and the
    entries on both sides of each half's first 16-byte boundary."""
    out = []
    for r in rows:
        others, low, hc, hr = _row_geometry(ix, r)
        ln = others.shape[0]
        slots = {0, ln - 1, low - 1, low}
        if 0 < hc < low:
            slots |= {hc - 1, hc}
        if 0 < hr < ln - low:
            slots |= {low + hr - 1, low + hr}
        out += [(r, s, int(others[s])) for s in sorted(slots) if 0 <= s < ln]
    return out


CSR_ROWS = (0, 1, 21, 38, 55, 72, 95, 96)


def _csr_edges(ix, name, rng):
    nx = ix.nx
    rows = [r if r < 90 else nx - (97 - r) for r in CSR_ROWS]
    marks = marked_entries(ix, rows)
    busy = set(rows) | {c for _, _, c in marks}
    free = [int(y) for y in np.arange(nx) if y not in busy]
    ncm = np.ones(ix.n, dtype=np.uint8)
    wanted, partner = [], {}
    for r, s, c in marks:
        # one partner of its own per marked entry: c is the partner's only computed neighbour, so the only common one
        j = free.pop(int(rng.integers(0, len(free))))
        partner[(r, s)] = j
        ncm[ix.pos([r, j], [c, c])] = 0
        wanted.append(int(ix.pos([r], [j])[0]))
    case = _finish(ix, name, rng, ncm, np.sort(np.array(wanted)), info=dict(marks=marks, partner=partner, rows=rows))
    # a wanted pair's bounds are loose on one side at least (on both where its match carries a special value, whose difference
    # may be 0): losing its one match leaves that bound untouched
    kind = np.arange(case.wanted.shape[0]) % 3
    kind[np.isin(case.wanted, [t for t, _ in case.special])] = 0
    case.feats[case.wanted, 0] = np.where(kind == 1, 20.5, 0.001)
    case.feats[case.wanted, 1] = np.where(kind == 2, 0.0005, 1000.5)
    # two pairs per marked entry would survive the candidate's choice; here the lookahead list takes every not-computed pair of
    # the marked rows' partners instead: all pairs wanted, none stolen
    case.RA[np.flatnonzero(ncm)] = 0.015625 * (1.0 + rng.random(int(ncm.sum())))
    case.sel = (case.sel[0], ix.n, 1)
    return case


# ------------------------------------------------------------------------------------------------------------ the checks
def _runs(first):
    """(start, length) of the runs of equal values."""
    s = np.flatnonzero(np.r_[True, first[1:] != first[:-1]])
    return s, np.diff(np.r_[s, first.shape[0]])


def check_case(case, ix, nxt, deep=True):
    """The list really produced still exercises what the case is named for.  Returns the reference (lb, ub)."""
    name, nx = case.name, ix.nx
    nxt = np.asarray(nxt, dtype=np.int64)
    assert nxt.shape[0] > 0 and (np.diff(nxt) > 0).all() and (case.ncm[nxt] == 1).all()
    if case.sel[1] >= int(case.ncm.sum()):
        assert np.array_equal(nxt, np.flatnonzero(case.ncm))
    elif name != "high_keys":
        assert nxt.shape[0] == case.wanted.shape[0] - 1 and np.isin(nxt, case.wanted).all()
    L = Lists(ix, case.ncm)
    i, j = ix.IJs[nxt, 0], ix.IJs[nxt, 1]
    li, lj = L.len[i], L.len[j]
    # values: no negative one, no NaN; the zeros, the equal pair and the subnormal sit on matches of listed pairs
    comp = case.RA[case.ncm == 0]
    assert (comp >= 0.0).all() and (comp == 0.0).any() and (comp == 5e-324).any()
    kinds = {k for t, k in case.special if t in set(nxt.tolist())}
    assert kinds == {0, 1, 2, 3}, kinds
    lb0, ub0 = case.feats[:, 0], case.feats[:, 1]
    lb, ub = update_bounds_ref(ix.IJs, case.RA, case.ncm, ix, None, nxt, lb0, ub0)
    rest = np.setdiff1d(np.arange(ix.n), nxt)
    assert np.array_equal(lb[rest], lb0[rest]) and np.array_equal(ub[rest], ub0[rest])
    dl, du = lb[nxt] != lb0[nxt], ub[nxt] != ub0[nxt]
    assert (lb >= lb0).all() and (ub <= ub0).all()
    assert (dl & du).any() and (dl & ~du).any() and (~dl & du).any() and (~dl & ~du).any()
    if name == "empty_lists":
        E = case.info["E"]
        assert (L.len[E] == 0).all() and np.isin(i, E).any() and np.isin(j, E).any()
        u, v = case.info["uv"]
        assert ((i == u) & (j == v)).any() and L.len[u] > 0 and L.len[v] > 0 and np.intersect1d(L.of(u), L.of(v)).size == 0
    elif name == "match_ends":
        for (a, b), same in zip(case.info["pairs"], (True, False)):
            A, B = L.of(a), L.of(b)
            assert ((i == a) & (j == b)).any() and A[0] == B[0] and A[-1] == B[-1] and (A.size == B.size) == same
            assert np.intersect1d(A, B).size < min(A.size, B.size)
    elif name == "tail_groups":
        assert nxt.shape[0] % 4 != 0 and nxt.shape[0] % 8 != 0 and nxt.shape[0] % 16 != 0
    elif name.startswith("past_stage"):
        S = 16 * int(name.rsplit("_", 1)[1])
        longer = np.maximum(li, lj)
        for want in (S, S + 1):
            assert ((longer == want) & (lj > li)).any() and ((longer == want) & (li > lj)).any(), want
        assert (longer > S + 1).any() and (longer < S).any() and ((li == S) & (lj == S)).any()
    elif name == "list_steps":
        assert {0, 1, 511, 512, 513, 1024} <= set(lj.tolist()) and (lj > 1024).any() and (lj % 4 != 0).any()
        assert (li == 0).any() and (li > 1024).any()
    elif name == "run_rebuild":
        s, ln = _runs(i)
        inside = s[s < CHUNK]
        assert inside.shape[0] >= 3 and nxt.shape[0] > CHUNK and i[CHUNK - 1] == i[CHUNK]      # (a run across the chunk's end)
        for r in range(1, inside.shape[0]):
            # keys of the previous first point that the new one does not have, in partner lists of the new run: bits left in
            # the table would match
            stale = np.setdiff1d(L.of(i[s[r - 1]]), L.of(i[s[r]]))
            seen = np.concatenate([L.of(p) for p in j[s[r]:s[r] + ln[r]]])
            assert np.isin(stale, seen).any(), r
    elif name == "long_run":
        s, ln = _runs(i)
        assert ln[0] > RUN_ROUND and ln[0] < CHUNK
    elif name == "dense_matches":
        best1 = best2 = 0
        for seg, ea, eb in L.hits(i, j):
            for t in np.unique(seg):
                at = (eb[seg == t] - L.ptr[j[t]]) // STEP
                cnt = np.bincount(at, minlength=3)
                best1, best2 = max(best1, int(cnt.max())), max(best2, int((cnt[:-1] + cnt[1:]).max()))
        assert best1 > 64 and best2 > 128, (best1, best2)
    elif name == "high_keys":
        assert SPLIT < nx <= 2 * SPLIT and ix.n < nx * (nx - 1) // 2
        bnd = np.bincount(np.repeat(np.arange(nx), L.len), weights=L.idx < SPLIT, minlength=nx).astype(np.int64)   # cbnd
        for l, b in ((li, bnd[i]), (lj, bnd[j])):      # first points' lists (the table) and partners' (the 2-byte stream)
            assert ((b == l) & (l > 0)).any() and ((b == 0) & (l > 0)).any() and ((b > 0) & (b < l)).any()
        lo = hi = 0
        for seg, ea, eb in L.hits(i, j):
            lo, hi = lo + int((L.idx[ea] < SPLIT).sum()), hi + int((L.idx[ea] >= SPLIT).sum())
        assert lo > 100 and hi > 100, (lo, hi)
    elif name == "csr_edges" and deep:
        # the CSR is seen through the bounds only: without any ONE of the marked entries the reference result differs
        for r, s, c in case.info["marks"]:
            ncm1 = case.ncm.copy()
            ncm1[ix.pos([r], [c])] = 1
            l1, u1 = update_bounds_ref(ix.IJs, case.RA, ncm1, ix, None, nxt, lb0, ub0)
            assert not (np.array_equal(l1, lb) and np.array_equal(u1, ub)), (r, s, c)
        rows = case.info["rows"]
        assert 0 in rows and nx - 1 in rows
    return lb, ub


# ------------------------------------------------------------------------------------- the thinned index of `high_keys`
HIGH_CFG = dict(n_anchors=96, n_neighbors=5, locality=4, loc_thresh=4, random_seed=3)
HIGH_CLUSTERS = 640


def high_points():
    """HIGH points in tight, well separated clusters; a point's cluster is drawn at random, so a cluster's members -- a
    point's candidates under the locality filter -- are spread over the whole index range."""
    rng = np.random.default_rng(HIGH)
    cent = rng.standard_normal((HIGH_CLUSTERS, 6)) * 4.0
    member = rng.integers(0, HIGH_CLUSTERS, HIGH)
    return cent[member] + 1.0e-4 * rng.standard_normal((HIGH, 6)), member


def high_index_host():
    """The index the locality filter gives on high_points() under HIGH_CFG, without the nx x nx count matrix of
    O.locality_pairs: with loc_thresh == locality two points are candidates of each other iff their sets of nearest anchors
    are equal (every such group is larger than loc_min + 1, asserted, so no row lowers its threshold)."""
    X, member = high_points()
    A, D = O.maxmin_anchors(lambda a: np.sqrt(((X - X[a]) ** 2).sum(axis=1)), HIGH, HIGH_CFG["n_anchors"], HIGH_CFG["random_seed"])
    sid = np.sort(O.nearest_anchor_sets(D, HIGH_CFG["locality"]), axis=1)
    # no cluster straddles a boundary between two sets
    first = np.zeros(HIGH_CLUSTERS, dtype=np.int64)
    first[member] = np.arange(HIGH)
    assert (sid == sid[first[member]]).all()
    _, group = np.unique(sid, axis=0, return_inverse=True)
    group = group.reshape(-1)
    size = np.bincount(group)
    assert size.min() > 10 * HIGH_CFG["n_neighbors"] + 1
    order = np.argsort(group, kind="stable")
    starts = np.r_[0, np.cumsum(size)]
    I0, J0 = [], []
    for g in range(size.shape[0]):
        m = order[starts[g]:starts[g + 1]]              # ascending
        a, b = np.triu_indices(m.shape[0], k=1)
        I0.append(m[a])
        J0.append(m[b])
    I0, J0 = np.concatenate(I0), np.concatenate(J0)
    o = np.argsort(I0 * HIGH + J0)
    IJs = np.stack([I0[o], J0[o]], axis=1).astype(np.int64)
    I_ptr, I_idx = O.build_I(IJs, HIGH)
    return I_ptr, I_idx, IJs
