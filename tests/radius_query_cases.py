"""Fixed-radius queries for new points on the host: the rule of the rectangle queries x data restated in NumPy, the plain triple
loop it is checked against, the injected anchor tables of the kernel tests and the data of the end-to-end tests.

The rule (include/annchor_hip.h), float64, for a query q, a data point j and every anchor a:
    s = QD[q, a]   t = D[j, a]   m = (s + t) + r
    out(a): (|s - t| - r) > rtol * m          in(a): (r - (s + t)) > rtol * m
    OUT if any out(a);  else SURE if connectivity mode and any in(a);  else EVAL
Every (q, j) of the rectangle is a valid pair: there is no i < j cut and no self-exclusion.  NumPy evaluates every operation on
its own (no fused multiply-add), as the library does (-ffp-contract=off): the classes are the kernel's bit for bit.  The lists
hold the pairs as (j, nx + q), query-major with ascending j.

`classify_q(..., wrong=...)` / `lists_q(..., wrong=...)` are the same code with one deliberate mistake;
tests/test_radius_query_cases.py shows that the case set notices each of them."""
import numpy as np

import radius_cases as C

OUT, EVAL, SURE = C.OUT, C.EVAL, C.SURE
# lt_for_le: the neighbours taken as d < r -- a pair whose lower bound EQUALS r is pruned (>= for > in the out test).
# keep_triangle / self_excluded: the graph form's diagonal cut / a k-NN query's "self" carried over to the rectangle.
WRONG = ("lt_for_le", "max_for_min", "no_rtol", "drop_last_anchor", "drop_last_column", "drop_last_query", "keep_triangle",
         "self_excluded", "column_major_order")


# ------------------------------------------------------------------------------------------------------ the reference
def classify_q(D, QD, r, rtol, conn, use_bounds=True, wrong=None):
    """Class of every (query, data point): int8 [nq, nx]; -1 where a wrong variant declares the pair invalid."""
    D, QD = np.asarray(D, dtype=np.float64), np.asarray(QD, dtype=np.float64)
    nx, nq = D.shape[0], QD.shape[0]
    na = D.shape[1] if use_bounds else 0
    if wrong == "drop_last_anchor" and na > 0:
        na -= 1
    r = np.float64(r)
    rtol = np.float64(0.0 if wrong == "no_rtol" else rtol)
    out = np.zeros((nq, nx), dtype=bool)
    any_in = np.zeros((nq, nx), dtype=bool)
    all_in = np.ones((nq, nx), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(na):
            s, t = QD[:, a][:, None], D[:, a][None, :]
            sm = s + t
            tol = rtol * (sm + r)
            lb = np.abs(s - t) - r
            out |= (lb >= tol) if wrong == "lt_for_le" else (lb > tol)
            inn = (r - sm) > tol
            any_in |= inn
            all_in &= inn
    inside = (all_in & (na > 0)) if wrong == "max_for_min" else any_in   # (the upper bound is the MIN over anchors of s + t)
    cls = np.full((nq, nx), EVAL, dtype=np.int8)
    if conn:
        cls[inside] = SURE
    cls[out] = OUT
    valid = np.ones((nq, nx), dtype=bool)
    qi, ji = np.arange(nq)[:, None], np.arange(nx)[None, :]
    if wrong == "drop_last_column":
        valid[:, nx - 1] = False
    if wrong == "drop_last_query":
        valid[nq - 1, :] = False
    if wrong == "keep_triangle":
        valid &= ji > qi
    if wrong == "self_excluded":
        valid &= ji != qi
    cls[~valid] = -1
    return cls


def lists_q(cls, wrong=None):
    """EVAL and SURE pairs as rows (j, nx + q), query-major with ascending j (int64 [n, 2]), and the per-query counts."""
    nq, nx = cls.shape

    def pairs(k):
        qj = np.argwhere(cls == k).astype(np.int64)            # (q, j), q-major, ascending j
        if wrong == "column_major_order":
            qj = qj[np.lexsort((qj[:, 0], qj[:, 1]))]
        return np.stack([qj[:, 1], nx + qj[:, 0]], axis=1).reshape(-1, 2)

    return dict(eval=pairs(EVAL), sure=pairs(SURE), row_eval=(cls == EVAL).sum(axis=1).astype(np.int64),
                row_sure=(cls == SURE).sum(axis=1).astype(np.int64), pruned=int((cls == OUT).sum()))


def classify_q_loop(D, QD, r, rtol, conn, use_bounds=True):
    """The rule as a plain Python loop over (q, j, a), one float64 operation at a time."""
    D, QD = np.asarray(D, dtype=np.float64), np.asarray(QD, dtype=np.float64)
    nx, nq = D.shape[0], QD.shape[0]
    na = D.shape[1] if use_bounds else 0
    r, rtol = np.float64(r), np.float64(rtol)
    cls = np.empty((nq, nx), dtype=np.int8)
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(nq):
            for j in range(nx):
                o = n = False
                for a in range(na):
                    s, t = QD[q, a], D[j, a]
                    m = (s + t) + r
                    if (np.abs(s - t) - r) > rtol * m:
                        o = True
                    if (r - (s + t)) > rtol * m:
                        n = True
                cls[q, j] = OUT if o else (SURE if (conn and n) else EVAL)
    return cls


def neighbors_from_matrix(R, r):
    """Ground truth from the rectangle R [nq, nx] of distances: (indptr, indices, distances), rows ascending by index."""
    keep = R <= r
    indptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    q, j = np.nonzero(keep)
    return indptr, j.astype(np.int64), R[q, j].astype(np.float64)


def rectangle_of(nx, nq, pairs_fn):
    """Every (Q[q], X[j]) through pairs_fn (IJ over X followed by Q -> float64) as a matrix [nq, nx]: the host double loop."""
    q, j = np.meshgrid(np.arange(nq), np.arange(nx), indexing="ij")
    IJ = np.stack([j.ravel(), nx + q.ravel()], axis=1).astype(np.int64)
    return np.asarray(pairs_fn(IJ), dtype=np.float64).reshape(nq, nx)


# ------------------------------------------------------------------------------------- injected anchor tables (kernel tests)
# The kernel's own sizes (csrc/radius.hip, k_rad_classify_q): 64 queries per block, 64 columns per chunk, two chunks per
# workgroup, 32 anchors per tile.
QB, COLS, TILE = 64, 64, 32


def tables(kind, nx, nq, na, seed):
    """(D [nx, na], QD [nq, na]).  The kinds of radius_cases.table, drawn for nx + nq points and cut in two; `copy`: ints whose
    queries are copies of data rows (query q is data point q while q < nx, a drawn one after that)."""
    if kind == "copy":
        D = C.table("ints", nx, na, seed)
        idx = np.arange(nq) if nq <= nx else np.concatenate([np.arange(nx), np.random.default_rng(seed).integers(0, nx, nq - nx)])
        return D, np.ascontiguousarray(D[idx])
    T = C.table(kind, nx + nq, na, seed)
    return np.ascontiguousarray(T[:nx]), np.ascontiguousarray(T[nx:])


def _case(kind, nx, nq, na, r, rtol=0.0, conn=False, use_bounds=True, cap=None, sub=None, seed=1):
    """cap: max_pairs of the planned calls (forced chunking); sub: (q_begin, q_end, col_begin, col_end) of one extra call."""
    return dict(kind=kind, nx=nx, nq=nq, na=na, r=r, rtol=rtol, conn=conn, use_bounds=use_bounds, cap=cap, sub=sub, seed=seed)


CASES = {}
for _nx in (1, 63, 64, 65, 127, 128, 129, 200):           # data columns on the chunk and chunk-pair edges
    CASES["nx%d" % _nx] = _case("ints", _nx, 3, 2, 3.0, conn=True, seed=_nx)
    CASES["nx%d_dist" % _nx] = _case("ints", _nx, 66, 3, 2.0, seed=100 + _nx)
for _nq in (1, 2, 63, 64, 65, 130):                       # queries on the block edges
    CASES["nq%d" % _nq] = _case("ints", 129, _nq, 2, 3.0, conn=True, seed=200 + _nq)
    CASES["nq%d_dist" % _nq] = _case("ints", 70, _nq, 3, 2.0, seed=300 + _nq)
for _na in (1, 31, 32, 33, 65):                           # anchor counts on the tile edges
    CASES["na%d" % _na] = _case("ints", 129, 5, _na, 3.0, conn=True, seed=400 + _na)
    CASES["na%d_rtol" % _na] = _case("ints", 67, 65, _na, 4.0, rtol=0.05, conn=True, seed=500 + _na)
CASES["ties"] = _case("ints", 130, 66, 3, 3.0, conn=True, seed=5)                   # |s - t| = r and s + t = r, rtol 0
CASES["ties_rtol"] = _case("ints", 130, 66, 3, 5.0, rtol=0.25, conn=True, seed=4)  # (|s - t| - r) = rtol m (s 10, t 1) and (r - (s + t)) = rtol m (s + t = 3), exactly
CASES["copy"] = _case("copy", 129, 70, 3, 3.0, conn=True, seed=6)                   # QD = D[:70]
CASES["copy_dist"] = _case("copy", 65, 130, 2, 2.0, seed=7)                         # more queries than data points
CASES["dups"] = _case("dups", 70, 5, 4, 0.0, conn=True)
CASES["r0"] = _case("ints", 130, 7, 3, 0.0, conn=True, seed=11)
CASES["r0_copy"] = _case("copy", 130, 7, 3, 0.0, seed=12)
CASES["all_out"] = _case("line", 140, 9, 2, 1e-6, conn=True, seed=13)
CASES["all_eval"] = _case("ints", 140, 9, 2, 1e9, seed=14)
CASES["all_sure"] = _case("ints", 140, 9, 2, 1e9, conn=True, seed=14)
CASES["inf"] = _case("inf", 131, 67, 5, 3.0, conn=True, seed=16)
CASES["inf_wide"] = _case("inf", 66, 3, TILE + 2, 3.0, rtol=0.01, conn=True, seed=17)
CASES["no_bounds"] = _case("ints", 131, 3, 3, 3.0, use_bounds=False, seed=18)
CASES["no_bounds_conn"] = _case("ints", 65, 66, 3, 3.0, conn=True, use_bounds=False, seed=19)
CASES["islands"] = _case("islands", 140, 10, 2, 5.0, conn=True, seed=23)            # every other query has an empty row
CASES["chunked"] = _case("ints", 200, 9, 3, 3.0, conn=True, cap=37, seed=20)        # queries of > 37 candidates are split by column
CASES["chunked_dist"] = _case("ints", 150, 70, 2, 5.0, cap=10, seed=21)
CASES["chunked_all"] = _case("ints", 129, 5, 2, 1e9, cap=50, seed=22)               # every query above the cap
CASES["islands_chunked"] = _case("islands", 140, 10, 2, 5.0, cap=16, seed=24)
CASES["sub"] = _case("ints", 200, 130, 3, 3.0, conn=True, sub=(3, 129, 5, 197), seed=25)     # off the 64 and 128 boundaries
CASES["sub_dist"] = _case("ints", 200, 130, 33, 4.0, sub=(65, 66, 63, 129), seed=26)         # one query, one column past a chunk pair
CASES["sub_one"] = _case("copy", 129, 70, 2, 3.0, conn=True, sub=(69, 70, 128, 129), seed=27)  # last query x last column


def build(name):
    c = CASES[name]
    return tables(c["kind"], c["nx"], c["nq"], c["na"], c["seed"])


def case_classes(name, wrong=None):
    c = CASES[name]
    D, QD = build(name)
    return classify_q(D, QD, c["r"], c["rtol"], c["conn"], c["use_bounds"], wrong)


def case_reference(name, wrong=None):
    return lists_q(case_classes(name, wrong), wrong)


def restrict(cls, sub):
    """The lists of one call on (q_begin, q_end, col_begin, col_end): the same rows, pairs outside the range left out."""
    qb, qe, cb, ce = sub
    cut = np.full_like(cls, -1)
    cut[qb:qe, cb:ce] = cls[qb:qe, cb:ce]
    return lists_q(cut)


# ------------------------------------------------------------------------------------------------ end-to-end queries
def fresh_strings(X, n, seed):
    """n new members of X's clusters, made as annchor_amd.datasets.synthetic_string_clusters makes them: 1 .. 6 random edits of
    a drawn member.  Then members longer and shorter than any in X, and two verbatim copies of members of X."""
    rng = np.random.default_rng(seed)
    letters = list("abcdefghijklmnopqrstuvwxyz")
    out = []
    for _ in range(n):
        b = list(str(X[int(rng.integers(len(X)))]))
        for _ in range(int(rng.integers(1, 7))):
            p = int(rng.integers(0, len(b)))
            u = rng.random()
            if u < 0.4:
                b[p] = letters[int(rng.integers(26))]
            elif u < 0.7 and len(b) > 10:
                b.pop(p)
            else:
                b.insert(p, letters[int(rng.integers(26))])
        out.append("".join(b))
    lens = [len(str(x)) for x in X]
    long_one = str(X[int(np.argmax(lens))]) + "qzqzqzq"
    short_one = str(X[int(np.argmin(lens))])[:min(lens) // 2]
    return out + [long_one, short_one, str(X[17]), str(X[len(X) - 1])]


def fresh_points(X, n, seed):
    """n new integer rows around members of X (the lattice of radius_cases.lattice_points: every distance stays the correctly
    rounded square root of an exact integer), then two verbatim copies."""
    rng = np.random.default_rng(seed)
    Q = X[rng.integers(0, len(X), n)].astype(np.int64) + rng.integers(-3, 4, (n, X.shape[1]))
    return np.ascontiguousarray(np.concatenate([Q.astype(X.dtype), X[[17, len(X) - 1]]]), dtype=X.dtype)
