"""Edge cases for candidate generation (csrc/locality.hip) and the pair features (the k_features* kernels of csrc/features.hip),
host only: no GPU import.

A case is an injected anchor table D [nx, na] (no metric is bound, so the table is exactly what the test uploads), an anchor
list A and the three locality parameters; the device is driven by tests/locality_worker.py through set_opaque /
set_anchor_distances / build_locality / compute_features, and everything it leaves behind -- nearest-anchor masks, IJs, the CSR
index, lb / ub / dad / is_anchor, the not-computed mask and the cached not-computed count -- is compared bit for bit with
oracle/annchor_oracle.py (nearest_anchor_sets, locality_pairs, features; query_locality, query_features on the query side).
The only float operations are |a - b|, a + b, max, min and / 2 in float64, exact on both sides: no tolerance appears anywhere.

Which kernel runs depends on nx, na, loc_thresh, locality, the list length and seven environment thresholds that the library
reads once per process: FORMS holds the four settings (one worker process each) and dispatch() restates the host code's
selection (annchor_build_locality, wide_keep_bitmap, annchor_compute_features, annchor_build_query_locality), so that
tests/test_locality_cases.py can show on the CPU that cases x forms reach every kernel and every template width.

variant() restates the reference with one deliberate mistake at a time (MUTANTS); the host test asserts that every mistake
changes its field on at least one case, i.e. that the table would notice it.  Two of the eight need a word:

  loc_min_unclamped   counting from the top without the clamp gives thr = 0 on every row, and with it thr_i = the row's smallest
                      count -- both keep every pair (C_ij >= min_j C_ij), so that form of the mistake cannot be seen in any
                      output.  The mutant is the other way an unclamped loc_min goes wrong: a row that has no (loc_min + 1)-th
                      entry is not widened and keeps loc_thresh.
  locality_unclamped  with locality >= na every set is all anchors and the list is complete however the picks are made; the
                      mutant is a rank loop that wraps around after na picks and lists the nearest locality - na anchors twice,
                      with shared anchors counted from the lists (multiplicities multiply).

Run as a script, the module prints the case table with the oracle's pair counts and shortest rows.
"""
import functools
import zlib

import numpy as np

from oracle import annchor_oracle as O

# --------------------------------------------------------------------------------------------------------------- cases
# name: (nx, na, table kind, A kind, locality, loc_thresh, loc_min, reason).  loc_min "nx-1" / "nx+70" are resolved below.
_T = [
    ("n2_a1", 2, 1, "ties", "last", 1, 1, 0, "smallest table: one pair, one anchor, loc_min 0 == nx - 1"),
    ("n31_a7", 31, 7, "metric", "all", 3, 2, 5, "nx < 32 (no dense / wide feature form), na < 8: k_features' repeated-anchor tail"),
    ("n31_a300_wide", 31, 300, "ties", "short", 5, 2, 5, "wide sets at nx < 32: k_features takes over from k_features_wide"),
    ("n33_a8", 33, 8, "ties", "ends", 3, 1, 0, "na == 8 (one full step of k_features), nx - 32 re-read of the dense form, A at nx - 1 and 0"),
    ("n33_a7_locality_over", 33, 7, "metric", "short", 9, 12, 5, "locality 9 > na (clamped to 7) and loc_thresh 12 above both: complete list"),
    ("n33_a65_locmin_over", 33, 65, "ties", "repeat", 5, 5, "nx+70", "loc_min = nx + 70 (clamped to nx - 1): complete list; loc_thresh == locality"),
    ("n63_a9", 63, 9, "metric", "repeat", 5, 5, 20, "nx = 63 (one partial bitmap word), na = 9: the a0 += 8 tail; repeated anchor id"),
    ("n63_a256_twins", 63, 256, "twins", "short", 1, 1, 0, "locality 1 on twin columns 63 / 64: the tie rule across a mask word, 4-word masks"),
    ("n64_a1_locmin_last", 64, 1, "ties", "last", 1, 1, "nx-1", "na = 1, loc_min == nx - 1 exactly, nx a whole bitmap word: complete list"),
    ("n64_a64", 64, 64, "ties", "short", 5, 2, 20, "nx = 64 (smallest k_keep_bits_cols), na = 64: last bit of the 1-word mask"),
    ("n65_a64", 65, 64, "ties", "p6364", 5, 1, 20, "nx = 65: i_base = min(i0, nx - 64) re-walk of k_keep_bits_cols; anchors at points 63 and 64"),
    ("n65_a65_twins", 65, 65, "twins", "p6364", 3, 2, 5, "na = 65: first bit of the second mask word, twin columns 63 / 64"),
    ("n65_a9_thresh_over", 65, 9, "ties", "ends", 3, 5, 5, "loc_thresh 5 > locality 3 (not clamped: every row falls back to its loc_min cut)"),
    ("n65_a300_wide_t8", 65, 300, "ties", "p6364", 9, 8, 20, "wide sets, loc_thresh 8: the last planes form, k_loc_thresh_small_wide<8>"),
    ("n127_a128", 127, 128, "metric", "short", 5, 5, 5, "na = 128 (last bit of the 2-word mask) > nx: anchor points repeat, twin columns"),
    ("n127_a257_wide_t1", 127, 257, "twins", "ends", 3, 1, 0, "wide sets, loc_thresh 1 (first planes form), twin columns 255 / 256, loc_min 0"),
    ("n129_a7_dups", 129, 7, "metric", "all", 3, 2, 20, "duplicated points: identical rows, zero distances; anchor-anchor pairs"),
    ("n129_a65", 129, 65, "ties", "repeat", 5, 3, 20, "nx = 129: third bitmap word of one bit; 2-word masks; repeated anchor id"),
    ("n129_a129", 129, 129, "ties", "repeat", 9, 8, 10, "na = 129: first bit of the third of four mask words; k_loc_thresh_small<8, 4>"),
    ("n129_a257_wide", 129, 257, "twins", "ends", 5, 3, 20, "wide sets at nx = 129 (nx - 32 re-read of k_features_wide), twin columns 255 / 256"),
    ("n257_a8_locality1", 257, 8, "ties", "short", 1, 1, 0, "locality 1 on tied rows: the tie rule alone decides every set"),
    ("n257_a129_t9", 257, 129, "ties", "p6364", 9, 9, 10, "loc_thresh 9: the histogram threshold form by default, 4-word masks"),
    ("n257_a256_twins", 257, 256, "twins", "all", 12, 5, 20, "na = 256: last bit of the 4-word mask, locality 12, 256 anchors in A"),
    ("n257_a257_wide_t9", 257, 257, "twins", "all", 12, 9, 5, "na = 257: narrow-to-wide switch; loc_thresh 9, locality 12: k_keep_bits_wide<0>"),
    ("n1030_a8_complete", 1030, 8, "metric", "all", 3, 2, "nx+70", "complete list at nx = 1030: the row-outer tiled feature kernel's case; 17 bitmap words"),
    ("n1030_a9_t1", 1030, 9, "metric", "repeat", 3, 1, 0, "nx > 1024: second trip of k_loc_thresh_small's 4 x 256 columns; loc_thresh 1"),
    ("n1030_a64_thin", 1030, 64, "ties", "p6364", 5, 2, 20, "thin list (density < 0.5) at na <= 64: the anchor-outer feature form's case; kw = 17 > 16"),
    ("n1030_a257_wide", 1030, 257, "ties", "short", 5, 2, 20, "wide sets at nx = 1030, planes form; two super-tiles in k_emit_cols"),
    ("n1030_a300_wide_l12", 1030, 300, "ties", "repeat", 12, 9, 20, "wide sets, loc_thresh 9 at locality 12: k_loc_thresh_wide, k_keep_bits_wide<0>; partial anchor chunk (300 = 9 x 32 + 12)"),
    ("n1030_a300_wide_l4", 1030, 300, "ties", "ends", 4, 9, 20, "wide sets, locality 4 at loc_thresh 9 (reachable through the clamp only): k_keep_bits_wide<4>"),
]
CASES = {}
for _name, _nx, _na, _kind, _akind, _loc, _lt, _lm, _why in _T:
    CASES[_name] = dict(name=_name, nx=_nx, na=_na, kind=_kind, akind=_akind, locality=_loc, loc_thresh=_lt,
                        loc_min={"nx-1": _nx - 1, "nx+70": _nx + 70}.get(_lm, _lm), reason=_why)
COMPLETE = ("n2_a1", "n33_a7_locality_over", "n33_a65_locmin_over", "n64_a1_locmin_last", "n1030_a8_complete")

# name: (nxb, nq, na, kind, locality, loc_thresh, queries without candidates, reason)
_Q = [
    ("q_n1", 1, 1, 7, "ties", 3, 1, (), "one data point, one query"),
    ("q_n63_a65", 63, 5, 65, "ties", 5, 2, (), "nxb = 63: one partial wavefront; 2-word masks"),
    ("q_n255_a9", 255, 5, 9, "metric", 3, 2, (), "nxb = 255: one short of the emit loop's block"),
    ("q_n256_a257_wide", 256, 1, 257, "ties", 5, 2, (), "nxb = 256: exactly one block; wide sets, one query"),
    ("q_n257_a300_wide_zero", 257, 5, 300, "ties", 5, 2, (2,), "nxb = 257: second block of one point, wide emit's clamped word; query 2 has no candidate"),
    ("q_n600_a129_zero", 600, 5, 129, "ties", 5, 3, (0, 4), "three emit blocks, 4-word masks; the first and the last query have no candidate: min_row_len = 0"),
    ("q_n600_a300_wide", 600, 5, 300, "ties", 5, 2, (), "wide sets over three blocks: words 8..11 clamped to kw - 1 = 9"),
    ("q_n257_a129_none", 257, 5, 129, "ties", 5, 2, (0, 1, 2, 3, 4), "no query has a candidate: n = 0, narrow"),
    ("q_n63_a257_wide_none", 63, 1, 257, "ties", 5, 2, (0,), "no candidate at all with wide sets: n = 0"),
]
QUERY_CASES = {}
for _name, _nxb, _nq, _na, _kind, _loc, _lt, _zero, _why in _Q:
    QUERY_CASES[_name] = dict(name=_name, nxb=_nxb, nq=_nq, nx=_nxb + _nq, na=_na, kind=_kind, locality=_loc, loc_thresh=_lt,
                              zero=tuple(_zero), reason=_why)

FORMS = {
    "default": {},
    "large": {"ANNCHOR_KEEP_COLS_MIN": "0", "ANNCHOR_EMIT_RUN_MIN": "0", "ANNCHOR_EMIT_SUPER_MIN": "1",
              "ANNCHOR_FEATURES_TILED_MIN": "0", "ANNCHOR_FEATURES_FORM": "tiled"},
    "dense": {"ANNCHOR_KEEP_COLS_MIN": "0", "ANNCHOR_EMIT_RUN_MIN": "0", "ANNCHOR_EMIT_SUPER_MIN": "1",
              "ANNCHOR_FEATURES_TILED_MIN": "0", "ANNCHOR_FEATURES_FORM": "dense"},
    "older": {"ANNCHOR_LOC_THRESH_HIST": "1", "ANNCHOR_EMIT_TILED_MIN": str(1 << 60), "ANNCHOR_KEEP_COLS_MIN": str(1 << 60),
              "ANNCHOR_EMIT_RUN_MIN": str(1 << 60)},
}
FORM_VARIABLES = ("ANNCHOR_LOC_THRESH_HIST", "ANNCHOR_KEEP_COLS_MIN", "ANNCHOR_EMIT_TILED_MIN", "ANNCHOR_EMIT_RUN_MIN",
                  "ANNCHOR_EMIT_SUPER_MIN", "ANNCHOR_FEATURES_TILED_MIN", "ANNCHOR_FEATURES_FORM")


# ------------------------------------------------------------------------------------------------------------ builders
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _anchor_points(rng, nx, na):
    """Ids of the points the columns of a metric table measure from: distinct while nx allows, repeating beyond."""
    perm = rng.permutation(nx)
    return perm[np.arange(na) % nx]


def _table(rng, kind, nx, na):
    """(D [nx, na] float64 finite non-negative, ids of the anchor points for a metric table or None)."""
    if kind == "ties":          # six values: every row has many equal distances
        return rng.integers(0, 6, (nx, na)).astype(np.float64), None
    if kind == "twins":         # two bitwise equal columns on each side of a mask-word boundary, the nearest for half the points
        D = rng.random((nx, na)) + 0.5
        for a, b in ((63, 64), (255, 256)):
            if b < na:
                D[rng.random(nx) < 0.5, a] *= 0.1
                D[:, b] = D[:, a]
        return D, None
    assert kind == "metric"     # Euclidean distances between a few clustered points, a tenth of them exact duplicates
    cent = rng.standard_normal((4, 3)) * 3.0
    P = cent[rng.integers(0, 4, nx)] + 0.5 * rng.standard_normal((nx, 3))
    ndup = nx // 10
    if ndup:
        dst = rng.choice(nx, ndup, replace=False)
        P[dst] = P[rng.integers(0, nx, ndup)]
    ids = _anchor_points(rng, nx, na)
    diff = P[:, None, :] - P[ids][None, :, :]
    return np.sqrt((diff * diff).sum(axis=2)), ids


def _anchor_list(rng, akind, nx, na, ids):
    if akind == "all":          # every anchor point once (na distinct points where the table has them)
        src = ids if ids is not None else rng.permutation(nx)[:min(na, nx)]
        _, first = np.unique(src, return_index=True)
        return np.asarray(src)[np.sort(first)].astype(np.int64)
    if akind == "short":        # fewer entries than na
        return rng.choice(nx, min(3, nx, max(1, na - 1)), replace=False).astype(np.int64)
    if akind == "repeat":       # one id twice, the other ids between its two slots
        a = rng.choice(nx, 3, replace=False).astype(np.int64)
        return np.array([a[0], a[1], a[2], a[0]], dtype=np.int64)
    if akind == "p6364":
        return np.array([63, 64], dtype=np.int64)
    if akind == "ends":
        return np.array([nx - 1, 0], dtype=np.int64)
    assert akind == "last"
    return np.array([nx - 1], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def build(name):
    """(D, A) of a pair-list case; arrays are shared between callers and must not be written."""
    c = CASES[name]
    rng = _rng(name)
    D, ids = _table(rng, c["kind"], c["nx"], c["na"])
    A = _anchor_list(rng, c["akind"], c["nx"], c["na"], ids)
    assert len(A) <= c["na"] and np.isfinite(D).all() and (D >= 0).all()
    D.setflags(write=False)
    A.setflags(write=False)
    return D, A


@functools.lru_cache(maxsize=None)
def build_query(name):
    """(D_all [nxb + nq, na], A): nxb data rows stacked on nq query rows.  A query listed in `zero` shares no nearest anchor
    with any data point: the last `locality` columns are far (50) for every data point and 0 for that query."""
    c = QUERY_CASES[name]
    rng = _rng(name)
    D, ids = _table(rng, c["kind"], c["nx"], c["na"])
    if c["zero"]:
        L = c["locality"]
        assert c["na"] >= 2 * L
        D[:c["nxb"], -L:] = 50.0
        for q in c["zero"]:
            D[c["nxb"] + q, -L:] = 0.0
            D[c["nxb"] + q, :-L] += 1.0
    A = rng.choice(c["nxb"], min(3, c["nxb"]), replace=False).astype(np.int64)
    D.setflags(write=False)
    A.setflags(write=False)
    return D, A


# ----------------------------------------------------------------------------------------------------------- reference
FIELDS = ("sid", "IJs", "I_ptr", "I_idx", "features", "ncm", "n_pairs", "min_row_len", "n_unc")


def onehot(sid, na):
    m = np.zeros((sid.shape[0], na), dtype=bool)
    np.put_along_axis(m, np.asarray(sid, dtype=np.int64), True, axis=1)
    return m


def pack(sid_bits, IJs, I_ptr, I_idx, feats, ncm, rows=None):
    rows = np.diff(I_ptr) if rows is None else rows
    return dict(sid=sid_bits, IJs=IJs.astype(np.int64).reshape(-1, 2), I_ptr=I_ptr.astype(np.int64), I_idx=I_idx.astype(np.int64),
                features=np.ascontiguousarray(feats, dtype=np.float64).reshape(-1, 4), ncm=np.asarray(ncm).astype(np.uint8),
                n_pairs=int(IJs.shape[0]), min_row_len=int(rows.min()), n_unc=int(np.asarray(ncm).astype(bool).sum()))


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's state of a pair-list case, as it stands: nearest_anchor_sets / locality_pairs / features."""
    c = CASES[name]
    D, A = build(name)
    sid, IJs, I_ptr, I_idx = O.locality_pairs(D, c["locality"], c["loc_thresh"], c["loc_min"])
    feats, ncm = O.features(IJs, D, A, I_ptr, I_idx)
    return pack(onehot(sid, c["na"]), IJs, I_ptr, I_idx, feats, ncm)


@functools.lru_cache(maxsize=None)
def query_reference(name):
    """O.query_locality / O.query_features in the device's frame: pair (i, nxb + j), rows of data points empty, the index
    the identity."""
    c = QUERY_CASES[name]
    Dall, A = build_query(name)
    nxb, nq, na = c["nxb"], c["nq"], c["na"]
    D, QD = Dall[:nxb], Dall[nxb:]
    sid_x = O.nearest_anchor_sets(D, c["locality"])
    sid_q, IJs, QI_ptr = O.query_locality(sid_x, QD, c["locality"], c["loc_thresh"], na)
    feats, ncm = O.query_features(IJs, D, QD, A)
    I_ptr = np.concatenate([np.zeros(nxb, dtype=np.int64), QI_ptr])
    dev = IJs.copy()
    dev[:, 1] += nxb
    return pack(np.vstack([onehot(sid_x, na), onehot(sid_q, na)]), dev, I_ptr, np.arange(len(IJs), dtype=np.int64),
                 feats.reshape(-1, 4), ncm, rows=np.diff(QI_ptr))


# ------------------------------------------------------------------------------------------------------- device decoding
def decode_sid(words, nx, na):
    """F_SID mask words -> bool [nx, na], bit a of row i <=> anchor a in sid[i] (as Annchor.sid reads them); bits >= na must be 0."""
    w = np.ascontiguousarray(words, dtype=np.uint64).reshape(nx, -1)
    bits = np.unpackbits(w.view(np.uint8), axis=1, bitorder="little").astype(bool)
    assert not bits[:, na:].any(), "mask bits set beyond the last anchor"
    return bits[:, :na]


def decode(npz, name, nx, na):
    """A case's downloads, as the worker stored them, in reference() form.  n == 0: the library holds no list, every field empty."""
    g = lambda k: npz["%s__%s" % (name, k)]  # noqa: E731
    n_pairs, min_row_len, n_unc = (int(v) for v in g("meta"))
    sid = g("sid")
    return dict(sid=decode_sid(sid, nx, na) if sid.size else sid, IJs=g("ijs").reshape(-1, 2), I_ptr=g("iptr"), I_idx=g("iidx"),
                features=g("feat").reshape(-1, 4), ncm=g("ncm"), n_pairs=n_pairs, min_row_len=min_row_len, n_unc=n_unc)


def _same(a, b):
    if isinstance(a, (int, np.integer)):
        return int(a) == int(b)
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return a.tobytes() == b.tobytes()      # bit for bit, floats included


def differences(got, want, fields=FIELDS):
    """Names of the fields that are not bit-identical."""
    return [f for f in fields if not _same(got[f], want[f])]


# ------------------------------------------------------------------------------------------------------ dispatch mirror
KERNELS = ("k_sid", "k_sid_wide", "k_loc_thresh", "k_loc_thresh_small", "k_loc_thresh_wide", "k_loc_thresh_small_wide",
           "k_keep_bits", "k_keep_bits_cols", "k_keep_bits_wide", "k_keep_bits_wide_planes", "k_row_prefix",
           "k_emit_pairs[rows_only=0]", "k_emit_pairs[rows_only=1]", "k_emit_rows_run", "k_emit_cols[plain]", "k_emit_cols[super]",
           "k_count_anchor_pairs", "k_anchor_flags", "k_features", "k_features_tiled", "k_features_dense", "k_features_wide",
           "k_qloc_count", "k_qloc_emit", "k_qloc_count_wide", "k_qloc_emit_wide")


def _words(na):
    return 1 if na <= 64 else 2 if na <= 128 else 4 if na <= 256 else (na + 63) // 64


def _env_int(env, key, default):
    return int(env[key]) if key in env else default


def _features_kernels(env, nx, na, nA, n, have_bitmap):
    """annchor_compute_features' choice (n > 0)."""
    out = []
    if have_bitmap and na > 256 and nx >= 32:
        return (["k_anchor_flags"] if nA else []) + ["k_features_wide"]
    if have_bitmap and n >= _env_int(env, "ANNCHOR_FEATURES_TILED_MIN", 8 << 20) and na <= 64:
        out += ["k_anchor_flags"] if nA else []
        form = env.get("ANNCHOR_FEATURES_FORM")
        density = n / (0.5 * nx * (nx - 1))
        if nx >= 32 and ((form == "dense") if form else density < 0.5):
            return out + ["k_features_dense"]
        return out + ["k_features_tiled<%d>" % next(m for m in (8, 16, 24, 32, 48, 64) if na <= m)]
    return ["k_features"]


def dispatch(case, env, n):
    """Kernels the host code launches for a pair-list case of n pairs under a form's environment, template arguments included."""
    nx, na, lt = case["nx"], case["na"], case["loc_thresh"]
    kw, L, nw = (nx + 63) // 64, min(case["locality"], na), _words(na)
    nA = len(build(case["name"])[1])
    hist = "ANNCHOR_LOC_THRESH_HIST" in env
    small = 1 <= lt <= 8 and not hist
    if na > 256:
        out = ["k_sid_wide", "k_loc_thresh_small_wide<%d>" % lt if small else "k_loc_thresh_wide"]
        out.append("k_keep_bits_wide_planes<%d>" % lt if 1 <= lt <= 8 else "k_keep_bits_wide<%d>" % (L if L <= 8 else 0))
    else:
        out = ["k_sid<%d>" % nw, "k_loc_thresh_small<%d,%d>" % (lt, nw) if small else "k_loc_thresh<%d>" % nw]
        cols = nx >= 64 and nx * kw >= _env_int(env, "ANNCHOR_KEEP_COLS_MIN", 1 << 20)
        out.append(("k_keep_bits_cols<%d>" if cols else "k_keep_bits<%d>") % nw)
    out.append("k_row_prefix")
    if nA:
        out.append("k_count_anchor_pairs")
    tiled = n >= _env_int(env, "ANNCHOR_EMIT_TILED_MIN", 0)
    if tiled and nx * kw >= _env_int(env, "ANNCHOR_EMIT_RUN_MIN", 1 << 20):
        out.append("k_emit_rows_run")
    else:
        out.append("k_emit_pairs[rows_only=%d]" % tiled)
    if tiled:
        out.append("k_emit_cols[super]" if kw >= _env_int(env, "ANNCHOR_EMIT_SUPER_MIN", 64) else "k_emit_cols[plain]")
    if n > 0:
        out += _features_kernels(env, nx, na, nA, n, True)
    return out


def dispatch_query(case, env, n):
    na, nw = case["na"], _words(case["na"])
    if na > 256:
        out = ["k_sid_wide", "k_qloc_count_wide"] + (["k_qloc_emit_wide"] if n else [])
    else:
        out = ["k_sid<%d>" % nw, "k_qloc_count<%d>" % nw] + (["k_qloc_emit<%d>" % nw] if n else [])
    return out + (_features_kernels(env, case["nx"], na, 1, n, False) if n else [])


def base_name(kernel):
    return kernel.split("<")[0]


# ------------------------------------------------------------------------------------------------------------- mutants
MUTANTS = {   # mistake: the field it must change
    "ties_to_larger_index": "IJs",
    "closest_anchor_last_minimum": "features",     # (the dad column)
    "keep_strict": "IJs",
    "symmetrise_with_max": "IJs",
    "loc_min_unclamped": "IJs",
    "locality_unclamped": "IJs",
    "repeated_anchor_twice": "n_unc",
    "phantom_columns": "IJs",
}


def variant(name, mutant=None, fields=FIELDS):
    """The reference restated from the definitions (not through the oracle), with at most one deliberate mistake.
    variant(name) == reference(name) on every case; `fields` limits the work to what the caller compares."""
    c = CASES[name]
    D, A = build(name)
    nx, na = D.shape
    locality, loc_thresh, loc_min = c["locality"], c["loc_thresh"], c["loc_min"]
    if mutant == "ties_to_larger_index":
        order = (na - 1 - np.argsort(D[:, ::-1], axis=1, kind="stable"))
    else:
        order = np.argsort(D, axis=1, kind="stable")
    L = min(locality, na)
    M = np.zeros((nx, na), dtype=np.int64)
    np.put_along_axis(M, order[:, :L], 1, axis=1)
    sid_bits = M.astype(bool)
    if mutant == "locality_unclamped" and locality > na:
        np.put_along_axis(M, order[:, :min(locality - na, na)], 2, axis=1)       # listed twice: the loop wrapped around
    C = M @ M.T
    lm = min(loc_min, nx - 1)
    Ct = C
    if mutant == "phantom_columns":     # the 4 x 256-column trips counted to their end: columns >= nx read as column nx - 1
        pad = -nx % 1024
        Ct = np.hstack([C, np.repeat(C[:, -1:], pad, axis=1)])
    kth = -np.partition(-Ct, lm, axis=1)[:, lm]
    thr = np.minimum(loc_thresh, kth)
    if mutant == "loc_min_unclamped" and loc_min > nx - 1:
        thr = np.full(nx, loc_thresh, dtype=kth.dtype)
    if mutant == "keep_strict":
        keep = (C > thr[:, None]) | (C > thr[None, :])
    elif mutant == "symmetrise_with_max":
        keep = C >= np.maximum(thr[:, None], thr[None, :])
    else:
        keep = C >= np.minimum(thr[:, None], thr[None, :])
    I0, J0 = np.nonzero(np.triu(keep, k=1))
    IJs = np.stack([I0, J0], axis=1).astype(np.int64)
    out = dict(sid=sid_bits, IJs=IJs, n_pairs=len(IJs))
    if set(fields) <= set(out):
        return out
    n = len(IJs)
    deg = np.bincount(IJs.ravel(), minlength=nx)
    I_ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    pos = np.arange(n, dtype=np.int64)
    owner, other, p2 = np.concatenate([J0, I0]), np.concatenate([I0, J0]), np.concatenate([pos, pos])
    I_idx = p2[np.lexsort((other, owner))]
    isA = np.zeros(nx, dtype=bool)
    isA[A] = True
    anc = isA[I0] | isA[J0]
    ncm = ~anc
    n_unc = int(ncm.sum())
    if mutant == "repeated_anchor_twice":   # a count per slot of A, anchor-anchor pairs once
        n_unc = n - (int(deg[A].sum()) - int((isA[I0] & isA[J0]).sum()))
    out.update(I_ptr=I_ptr, I_idx=I_idx, ncm=ncm.astype(np.uint8), min_row_len=int(deg.min()), n_unc=n_unc)
    if "features" in fields:
        Di, Dj = D[I0], D[J0]
        lb, ub = np.abs(Di - Dj).max(axis=1), (Di + Dj).min(axis=1)
        cA = (na - 1 - np.argmin(D[:, ::-1], axis=1)) if mutant == "closest_anchor_last_minimum" else np.argmin(D, axis=1)
        dad = (D[I0, cA[J0]] + D[J0, cA[I0]]) / 2
        out["features"] = np.ascontiguousarray(np.vstack([lb, ub, dad, anc.astype(np.float64)]).T).reshape(-1, 4)
    return out


def padded(name, na_to):
    """The case's table padded with far-away anchors (1e6 + a, the same for every point) up to na_to columns: sets, pairs and
    features are unchanged while the masks take another width.  Only for cases whose locality is not clamped."""
    D, _ = build(name)
    nx, na = D.shape
    assert na_to > na and CASES[name]["locality"] <= na
    far = 1e6 + np.arange(na, na_to, dtype=np.float64)
    return np.hstack([D, np.broadcast_to(far, (nx, na_to - na))])


if __name__ == "__main__":
    print("| case | nx | na | table | A | locality | loc_thresh | loc_min | pairs kept | all pairs | shortest row |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for nm, cs in CASES.items():
        r = reference(nm)
        print("| %s | %d | %d | %s | %s | %d | %d | %d | %d | %d | %d |" % (
            nm, cs["nx"], cs["na"], cs["kind"], cs["akind"], cs["locality"], cs["loc_thresh"], cs["loc_min"], r["n_pairs"],
            cs["nx"] * (cs["nx"] - 1) // 2, r["min_row_len"]))
    print()
    print("| query case | nxb | nq | na | locality | loc_thresh | pairs | fewest candidates | not computed |")
    print("|---|---|---|---|---|---|---|---|---|")
    for nm, cs in QUERY_CASES.items():
        r = query_reference(nm)
        print("| %s | %d | %d | %d | %d | %d | %d | %d | %d |" % (nm, cs["nxb"], cs["nq"], cs["na"], cs["locality"], cs["loc_thresh"],
                                                              r["n_pairs"], r["min_row_len"], r["n_unc"]))
