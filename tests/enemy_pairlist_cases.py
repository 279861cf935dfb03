"""Edge cases for the nearest-enemy graph on the pair list (csrc/enemies.hip), host only: no GPU import.

A case is a fitted state -- the injected anchor table D, the anchor list A and the fit's locality / loc_thresh / loc_min of a
case of tests/locality_cases.py (its build() and table kinds, not copies of them), with the fitted RefineApprox and
not-computed mask filled per case --, labels y, the call's (loc_min, first, nn), a regression (bins with infinite outer edges,
W, c; or the same model's predictions handed over as a vector, the custom-regression route) and a symmetric table E of "exact"
values that stands in for the metric.  One case (`grid129_a7_device_metric`) holds points on an integer grid, duplicated across
labels, for the device-metric route: Euclidean distances of integer coordinates are exact on both sides.

stages() restates oracle.annchor_oracle.nearest_enemies stage by stage, keeps the fitted and the new arrays apart as the
device does, and returns every intermediate: per-row thresholds and the lowered flag, the new pairs with their CSR, feature
rows and mask, the clipped prediction, the todo list as a sorted multiset of pairs (a pair two rows ask for is listed twice),
both RefineApprox / mask pairs after the write-back and the graph.  tests/test_enemy_pairlist_cases.py asserts that its end
state is the oracle's, tests/test_enemy_pairlist_gpu.py compares every field of every stage with the device, bit for bit.

Every float operation is fixed: |a - b|, a + b, max, min, / 2 for the features, ((w0 * lb + w1 * ub) + w2 * dad) + c for the
prediction (the library is built without contraction), one addition of the row maximum per penalty for the graph keys.  No
tolerance appears anywhere.  All values are non-negative, so no -0.0 can reorder keys.

check_case() asserts, on the reference's own arrays, the properties a case is listed for (EDGES: tag -> predicate); stages()
takes one deliberate mistake at a time (MUTANTS: mistake -> the field it must change), and the host test asserts that every
mistake is noticed by at least one case.  All thirteen are visible; none needed an exception.

Run as a script, the module prints the case table with the reference's counts.
"""
import functools
import types
import zlib

import numpy as np

import locality_cases as C
from oracle import annchor_oracle as O
from oracle import metrics as om

INF = float("inf")
MODELS = {
    # bin 0 predicts below every lb, bin 2 above every ub, bin 1 in general position (coefficients that are no binary fractions:
    # a contracted multiply-add or another order of the sum shows in the last bit)
    "edges": (np.array([-INF, 1.0, 2.5, INF]), np.array([[0.0, 0.0, 0.0], [0.3, 0.6, 0.1], [0.0, 2.0, 0.0]]),
              np.array([-1.0, 0.05, 1.0])),
    # every interior edge the same: bins 1 and 2 are empty, dad == 2.0 belongs to bin 0
    "equal_edges": (np.array([-INF, 2.0, 2.0, 2.0, INF]),
                    np.array([[0.7, 0.2, 0.1], [9.0, 9.0, 9.0], [-9.0, -9.0, 9.0], [0.1, 0.8, 0.1]]), np.array([0.01, 50.0, -50.0, 0.3])),
    # integer predictions on integer tables: the new entries tie with the fitted ones
    "int": (np.array([-INF, 2.0, INF]), np.zeros((2, 3)), np.array([2.0, 3.0])),
}
# "data_edges" / "data_equal": the coefficients of "edges" / "equal_edges" with interior edges taken from the dad values of the
# case's own new pairs that have lb < ub (a random table leaves most pairs with lb >= ub, where the clip returns ub whatever
# the model says): the values at one and two thirds of their sorted distinct list, resp. the middle one three times
MODELS["data_edges"], MODELS["data_equal"] = MODELS["edges"], MODELS["equal_edges"]

# name: (base case of locality_cases or "grid", labels, loc_min, first, nn, model, by vector, fill of RA, fill of the mask, edges)
_T = [
    ("n65_a64_nothing_new", "n65_a64", "three", 3, 50, 3, "edges", False, "zero_rows", "feat",
     "no_lowered n_new_zero zero_row class_of_nn unsorted_codes first_50 nn3 listed_twice"),
    ("n65_a64_clamp", "n65_a64", "three", 44, "median", 3, "int", False, "int", "feat",
     "some_clamp first_equal_ne listed_twice idle_rows"),
    ("n63_a9_two_labels", "n63_a9", "two", 45, 50, 1, "edges", False, "float", "feat", "two_labels nn1 all_clamp new_pairs"),
    ("n63_a256_first1", "n63_a256_twins", "three", 10, 1, 3, "data_edges", False, "float", "ones", "first_1 few_computed clip_both clip_idle dad_on_edge"),
    ("n64_a64_all_clamp", "n64_a64", "two", 100, 100, 16, "int", False, "int", "feat", "all_clamp first_over nn16 two_labels"),
    ("n65_a65_model", "n65_a65_twins", "three", 5, 50, 3, "data_edges", False, "float", "feat",
     "first_above_below lowered_only_larger clip_both dad_on_edge"),
    ("n65_a65_by_vector", "n65_a65_twins", "three", 5, 50, 3, "data_edges", True, "float", "feat", "pred_route clip_both dad_on_edge"),
    ("n127_a128_pinned", "n127_a128", "three", 20, 50, 3, "edges", False, "float", "feat", "class_of_nn"),
    ("n129_a65_crossed_bounds", "n129_a65", "three", 20, 50, 3, "edges", False, "float", "feat", "crossed_bounds lowered_only_larger"),
    ("n129_a65_same_low", "n129_a65", "three", 20, 50, 3, "int", False, "same_low", "feat", "same_label_smallest first_equal_ne"),
    ("n129_a129_nn16", "n129_a129", "two", 40, 50, 16, "int", False, "int", "feat", "nn16 lowered_only_larger first_above_below"),
    ("n257_a129_uncomputed", "n257_a129_t9", "three", 3, 50, 3, "edges", False, "int", "ones", "all_uncomputed lowered_only_larger"),
    ("n257_a256_equal_edges", "n257_a256_twins", "three", 40, 50, 3, "data_equal", False, "float", "feat", "todo_empty equal_edges"),
    ("n65_a300_wide", "n65_a300_wide_t8", "three", 44, 50, 3, "int", False, "int", "feat", "some_clamp"),
    ("n257_a257_wide_all_computed", "n257_a257_wide_t9", "three", 40, 50, 3, "edges", False, "int", "feat", "todo_empty lowered_only_larger"),
    ("n257_a257_wide_all_clamp", "n257_a257_wide_t9", "three", 300, 50, 3, "int", False, "int", "feat", "all_clamp"),
    ("n1030_a64_long_rows", "n1030_a64_thin", "three", 40, 50, 3, "int", False, "int", "feat",
     "long_row_ties wave_ties lowered_only_larger listed_twice idle_rows"),
    ("n1030_a300_wide_l4", "n1030_a300_wide_l4", "three", 40, 50, 3, "int", False, "int", "feat", "wave_ties long_row_ties"),
    ("n1030_a300_wide_l12", "n1030_a300_wide_l12", "two", 40, 50, 1, "edges", False, "int", "feat", "nn1 lowered_only_larger"),
    ("grid129_a7_device_metric", "grid", "three", 60, 50, 3, "data_edges", False, "float", "feat", "device_metric enemy_at_zero new_pairs clip_both clip_idle dad_on_edge"),
    ("grid129_a7_halves", "grid", "halves", 0, 50, 5, "edges", False, "float", "feat", "few_enemies two_labels"),
]
CASES = {}
for _r in _T:
    CASES[_r[0]] = dict(zip(("name", "base", "labels", "loc_min", "first", "nn", "model", "by_vector", "fill", "mask", "edges"), _r))
    CASES[_r[0]]["edges"] = tuple(_r[-1].split())
GRID = dict(nx=129, na=7, locality=3, loc_thresh=2, loc_min=10)


def _rng(name):
    return np.random.default_rng(zlib.crc32(("enemy/" + name).encode()))


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def grid_points():
    """129 points on a 7 x 7 integer grid: most sites are taken more than once, many under more than one label."""
    rng = _rng("grid")
    X = rng.integers(0, 7, (GRID["nx"], 2)).astype(np.float64)
    A = rng.choice(GRID["nx"], GRID["na"], replace=False).astype(np.int64)
    IJ = np.stack([np.repeat(np.arange(GRID["nx"]), GRID["na"]), np.tile(A, GRID["nx"])], axis=1)
    D = om.euclidean_pairs(X, IJ).reshape(GRID["nx"], GRID["na"])
    _freeze(X, A, D)
    return X, A, D


@functools.lru_cache(maxsize=None)
def fitted(base):
    """The fit's state of a base case, from the oracle: D, A, parameters, sid (bool [nx, na]), IJs, CSR, features, mask."""
    if base == "grid":
        _, A, D = grid_points()
        p = GRID
        sid, IJs, I_ptr, I_idx = O.locality_pairs(D, p["locality"], p["loc_thresh"], p["loc_min"])
        feats, ncm = O.features(IJs, D, A, I_ptr, I_idx)
        r = C.pack(C.onehot(sid, p["na"]), IJs, I_ptr, I_idx, feats, ncm)
    else:
        p = C.CASES[base]
        D, A = C.build(base)
        r = C.reference(base)
    out = types.SimpleNamespace(D=D, A=A, nx=D.shape[0], na=D.shape[1], locality=p["locality"], loc_thresh=p["loc_thresh"],
                                fit_loc_min=p["loc_min"], sid=r["sid"], IJs=r["IJs"], I_ptr=r["I_ptr"], I_idx=r["I_idx"],
                                feats=r["features"], ncm=r["ncm"].astype(bool))
    _freeze(out.IJs, out.I_ptr, out.I_idx, out.feats, out.ncm)
    return out


@functools.lru_cache(maxsize=None)
def build(name):
    """The case's state: fitted(base) plus y, E, RA, ncm (fitted, before the call), first, nn, loc_min, the model."""
    cs = CASES[name]
    f = fitted(cs["base"])
    rng = _rng(name)
    nx, nn = f.nx, cs["nn"]
    y = rng.integers(0, 2 if cs["labels"] == "two" else 3, nx).astype(np.int32)
    if cs["labels"] == "halves":         # the grid's left and right half: most rows of the fit hold their own label only
        y = (grid_points()[0][:, 0] >= 4).astype(np.int32)
    if cs["labels"] == "three":          # plus a class of exactly nn points; the codes are dense and in no order
        y[rng.choice(nx, nn, replace=False)] = 3
        y = np.array([2, 0, 3, 1], dtype=np.int32)[y]
    integer = cs["fill"] in ("int", "same_low", "zero_rows")
    if cs["base"] == "grid":
        X = grid_points()[0]
        allp = np.stack(np.meshgrid(np.arange(nx), np.arange(nx), indexing="ij"), axis=-1).reshape(-1, 2)
        E = om.euclidean_pairs(X, allp).reshape(nx, nx)
    else:
        E = np.triu(rng.integers(0, 7, (nx, nx)).astype(np.float64) if integer else 6.0 * rng.random((nx, nx)), 1)
        E = E + E.T
    i, j = f.IJs[:, 0], f.IJs[:, 1]
    n = len(i)
    ncm = {"feat": f.ncm & (rng.random(n) < 0.5), "ones": np.ones(n, dtype=bool)}[cs["mask"]]
    lb, ub = f.feats[:, 0], f.feats[:, 1]
    guess = rng.integers(0, 7, n).astype(np.float64) if integer else lb + (ub - lb) * rng.random(n)
    RA = np.where(ncm, guess, E[i, j])
    if cs["fill"] == "same_low":         # same-label entries look closer than every enemy
        same = y[i] == y[j]
        RA[same] = 0.0
        RA[~same] = np.maximum(RA[~same], 1.0)
        E = np.maximum(E, 1.0)
    if cs["fill"] == "zero_rows":        # the first and the last point: every entry of their rows is 0 and stays 0
        rows = np.array([0, nx - 1])
        E[rows, :] = 0.0
        E[:, rows] = 0.0
        RA[np.isin(i, rows) | np.isin(j, rows)] = 0.0
    first = cs["first"]
    bins, W, c = MODELS[cs["model"]]
    out = types.SimpleNamespace(name=name, fit=f, y=y, E=E, RA=RA, ncm=ncm, nn=nn, loc_min=cs["loc_min"], first=first, bins=bins, W=W, c=c,
                                by_vector=cs["by_vector"], device_metric="device_metric" in cs["edges"])
    if cs["model"].startswith("data_"):
        fn = stages_of(out, upto="candidates")["feats_n"]
        u = np.unique(fn[fn[:, 0] < fn[:, 1], 2])
        inner = [u[len(u) // 3], u[2 * len(u) // 3]] if cs["model"] == "data_edges" else [u[len(u) // 2]] * 3
        out.bins = np.array([-INF] + inner + [INF])
    if first == "median":                # the middle one of the rows' enemy counts: rows with fewer, as many and more enemies than `first`
        out.first = 1
        u = np.unique(_enemy_counts(out, stages_of(out, upto="candidates")))
        out.first = int(u[len(u) // 2])
    _freeze(y, E, RA, ncm)
    return out


def _enemy_counts(st, r):
    f = st.fit
    ne = np.zeros(f.nx, dtype=np.int64)
    for IJ in (f.IJs, r["IJn"]):
        e = IJ[st.y[IJ[:, 0]] != st.y[IJ[:, 1]]]
        ne += np.bincount(e.ravel(), minlength=f.nx)
    return ne


# ------------------------------------------------------------------------------------------------------------ reference
MUTANTS = {   # mistake: the field of stages() it must change
    "symmetrisation_ignored": "IJn",
    "clamp_over_all_points": "thr",
    "same_label_in_histogram": "thr",
    "fitted_pairs_kept": "IJn",
    "bin_rule_left_closed": "RA_n0",
    "no_clip": "RA_n0",
    "same_label_among_first": "todo",
    "cut_ties_reversed": "todo",
    "cut_ties_new_first": "todo",
    "mx_over_enemies": "ngi",
    "uncomputed_not_pushed": "ngi",
    "same_label_not_pushed": "ngi",
    "graph_ties_reversed": "ngi",
}
STAGE_OF = {"thr": "candidates", "IJn": "candidates", "RA_n0": "predict", "todo": "first", "ngi": "graph"}
FIELDS = ("thr", "lowered", "IJn", "ptr_n", "idx_n", "feats_n", "ncm_n0", "RA_n0", "todo", "RA_f1", "ncm_f1", "RA_n1", "ncm_n1", "ngi", "ngd")


def predict_raw(feats, bins, W, c, left_closed=False):
    """The stratified regression before the clip: bin b with bins[b] < dad <= bins[b + 1], ((w0 lb + w1 ub) + w2 dad) + c."""
    F = feats[:, 2]
    b = np.zeros(len(F), dtype=np.int64)
    for k in range(len(bins) - 1):       # the last bin that holds the value, as the kernel's loop leaves it
        m = ((F >= bins[k]) & (F < bins[k + 1])) if left_closed else ((F > bins[k]) & (F <= bins[k + 1]))
        b[m] = k
    w = W[b]
    return ((w[:, 0] * feats[:, 0] + w[:, 1] * feats[:, 1]) + w[:, 2] * feats[:, 2]) + c[b]


def _cut(vals, want, is_new, mutant):
    """Positions (into vals) of the `want` smallest, ties on the cut in list order."""
    if want <= 0:
        return np.zeros(0, dtype=np.int64)
    cut = np.sort(vals)[want - 1]
    below = np.flatnonzero(vals < cut)
    eq = np.flatnonzero(vals == cut)
    room = want - len(below)
    if mutant == "cut_ties_reversed":
        eq = eq[::-1]
    if mutant == "cut_ties_new_first":
        eq = np.concatenate([eq[is_new[eq]], eq[~is_new[eq]]])
    return np.sort(np.concatenate([below, eq[:room]]))


def stages_of(st, mutant=None, upto="graph"):
    f, y = st.fit, st.y
    nx, n0 = f.nx, len(f.IJs)
    Am = f.sid.astype(np.int32)
    Cm = Am @ Am.T
    enemy = y[:, None] != y[None, :]
    # ---- candidates
    thr = np.empty(nx, dtype=np.int32)
    low = np.zeros(nx, dtype=bool)
    for i in range(nx):
        pool = Cm[i] if mutant == "same_label_in_histogram" else Cm[i][enemy[i]]
        pool = np.sort(pool)[::-1]
        lm = min(st.loc_min, (nx if mutant == "clamp_over_all_points" else len(pool)) - 1)
        kth = pool[lm] if lm < len(pool) else 0         # counting from the top and running out ends at 0
        low[i] = kth < f.loc_thresh
        thr[i] = min(kth, f.loc_thresh)
    new = enemy & (Cm >= thr[:, None])                   # new[i, j]: row i admits j
    lowered = bool(low.any())
    only_larger = np.triu(new.T & ~new, 1)               # (i < j) admitted by row j alone
    if lowered and mutant != "symmetrisation_ignored":
        new = new | np.tril(new, -1).T
    keep_fit = np.zeros((nx, nx), dtype=bool)
    keep_fit[f.IJs[:, 0], f.IJs[:, 1]] = True
    if mutant != "fitted_pairs_kept":
        new = new & ~keep_fit
    I0, J0 = np.nonzero(np.triu(new, 1))
    IJn = np.stack([I0, J0], axis=1).astype(np.int64)
    ptr_n, idx_n = O.build_I(IJn, nx)
    feats_n, ncm_n = O.features(IJn, f.D, f.A, ptr_n, idx_n)
    feats_n = np.ascontiguousarray(feats_n).reshape(-1, 4)
    out = dict(thr=thr, lowered=lowered, low=low, IJn=IJn, ptr_n=ptr_n, idx_n=idx_n, feats_n=feats_n, ncm_n0=ncm_n.copy(),
               only_larger=int((only_larger & new).sum()) if lowered else 0)
    if upto == "candidates":
        return out
    # ---- prediction
    raw = predict_raw(feats_n, st.bins, st.W, st.c, left_closed=mutant == "bin_rule_left_closed")
    RA_n = raw.copy() if mutant == "no_clip" else _clip(feats_n, raw)     # lb > ub (no metric behind the table): ub, as np.clip has it
    out.update(pred_raw=raw, RA_n0=RA_n.copy())
    if upto == "predict":
        return out
    # ---- first lists over the merged rows: fitted entries, then new entries, each by other endpoint
    IJa = np.vstack([f.IJs, IJn])
    RA = np.concatenate([st.RA, RA_n])
    ncm = np.concatenate([st.ncm, ncm_n])
    rows, others = [], []
    for i in range(nx):
        Ii = np.concatenate([f.I_idx[f.I_ptr[i]:f.I_ptr[i + 1]], idx_n[ptr_n[i]:ptr_n[i + 1]] + n0])
        q = IJa[Ii]
        rows.append(Ii)
        others.append(np.where(q[:, 0] == i, q[:, 1], q[:, 0]))
    todo, picked = [], []
    for i in range(nx):
        Ii = rows[i]
        en = np.ones(len(Ii), dtype=bool) if mutant == "same_label_among_first" else y[others[i]] != y[i]
        slots = np.flatnonzero(en)
        sel = slots[_cut(RA[Ii][en], min(st.first, len(slots)), (Ii >= n0)[en], mutant)]
        picked.append(sel)
        todo.append(Ii[sel][ncm[Ii[sel]]])
    todo = np.concatenate(todo)
    pairs = IJa[todo]
    pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
    out.update(rows=rows, others=others, picked=picked, todo_pos=todo, todo=pairs, RA_before=RA.copy(), ncm_before=ncm.copy())
    if upto == "first":
        return out
    RA[todo] = st.E[IJa[todo, 0], IJa[todo, 1]]
    ncm[todo] = False
    out.update(RA_f1=RA[:n0].copy(), ncm_f1=ncm[:n0].copy(), RA_n1=RA[n0:].copy(), ncm_n1=ncm[n0:].copy())
    # ---- graph
    nn = st.nn
    ngi, ngd = np.zeros((nx, nn), dtype=np.int64), np.zeros((nx, nn))
    keys = []
    for i in range(nx):
        Ii = rows[i]
        same = y[others[i]] == y[i]
        d = RA[Ii].copy()
        mx = d[~same].max() if mutant == "mx_over_enemies" and (~same).any() else d.max()
        if mutant != "uncomputed_not_pushed":
            d[ncm[Ii]] += mx
        if mutant != "same_label_not_pushed":
            d[same] += mx
        slot = np.arange(len(d))
        pick = np.lexsort((-slot if mutant == "graph_ties_reversed" else slot, d))[:nn]
        keys.append(d)
        ngi[i], ngd[i] = others[i][pick], RA[Ii[pick]]
    out.update(ngi=ngi, ngd=ngd, keys=keys)
    return out


@functools.lru_cache(maxsize=None)
def stages(name, mutant=None, upto="graph"):
    return stages_of(build(name), mutant, upto)


def oracle_end_state(name):
    """O.nearest_enemies on the case's state: (fitted object afterwards, idx, dist)."""
    st = build(name)
    f = st.fit
    o = types.SimpleNamespace(nx=f.nx, D=f.D, A=f.A, sid=O.nearest_anchor_sets(f.D, f.locality), loc_thresh=f.loc_thresh, IJs=f.IJs.copy(),
                              I_ptr=f.I_ptr.copy(), I_idx=f.I_idx.copy(), features=f.feats.copy(), RA=st.RA.copy(), ncm=st.ncm.copy(),
                              bins=st.bins, W=st.W, c=st.c, metric_pairs=lambda IJ: st.E[IJ[:, 0], IJ[:, 1]])
    ngi, ngd = O.nearest_enemies(o, st.y, nn=st.nn, loc_min=st.loc_min, first=st.first)
    return o, ngi, ngd


# ---------------------------------------------------------------------------------------------------------------- edges
def _row_stats(st, r):
    f = st.fit
    len_f = np.diff(f.I_ptr)
    ln = len_f + np.diff(r["ptr_n"])
    ne = np.array([(st.y[o] != st.y[i]).sum() for i, o in enumerate(r["others"])])
    return len_f, ln, ne


def _long_row_ties(st, r):
    """A row of more than 256 entries whose ties on the cut exceed the room and sit in both trips of the block loop and on both
    sides of the fitted / new boundary."""
    len_f, ln, ne = _row_stats(st, r)
    for i in np.flatnonzero(ln > 256):
        en = st.y[r["others"][i]] != st.y[i]
        v = np.where(en, r["RA_before"][r["rows"][i]], np.inf)
        want = min(st.first, int(en.sum()))
        if want == 0:
            continue
        cut = np.sort(v)[want - 1]
        eq = np.flatnonzero(v == cut)
        room = want - int((v < cut).sum())
        if len(eq) > room and (eq < 256).any() and (eq >= 256).any() and (eq < len_f[i]).any() and (eq >= len_f[i]).any():
            return True
    return False


def _wave_ties(st, r):
    """A row where the last pick of the graph and the first entry left out hold the same key, at slots at least 64 apart that
    different wavefronts of the block own."""
    for i, d in enumerate(r["keys"]):
        order = np.lexsort((np.arange(len(d)), d))
        if len(d) > st.nn:
            a, b = order[st.nn - 1], order[st.nn]
            if d[a] == d[b] and abs(int(a) - int(b)) >= 64 and (a % 256) // 64 != (b % 256) // 64:
                return True
    return False


def _few_computed(st, r):
    ncm = np.concatenate([r["ncm_f1"], r["ncm_n1"]])
    for i, Ii in enumerate(r["rows"]):
        en = st.y[r["others"][i]] != st.y[i]
        if (en & ~ncm[Ii]).sum() < st.nn:
            return True
    return False


def _same_label_smallest(st, r):
    for i, Ii in enumerate(r["rows"]):
        en = st.y[r["others"][i]] != st.y[i]
        v = r["RA_before"][Ii]
        if en.any() and (~en).any() and v[~en].min() < v[en].min():
            return True
    return False


def _clamped(st, r):
    ne = np.array([(st.y != st.y[i]).sum() for i in range(st.fit.nx)])
    return st.loc_min > ne - 1


def _interior(st):
    return st.bins[1:-1]


def _sane(r):
    return r["feats_n"][:, 0] < r["feats_n"][:, 1]


def _clip(feats, raw):
    return np.minimum(np.maximum(raw, feats[:, 0]), feats[:, 1])


EDGES = {
    "no_lowered": lambda st, r: not r["lowered"] and not r["low"].any(),
    "lowered_only_larger": lambda st, r: r["lowered"] and r["only_larger"] > 0,
    "all_clamp": lambda st, r: _clamped(st, r).all(),
    "some_clamp": lambda st, r: _clamped(st, r).any() and not _clamped(st, r).all(),
    "n_new_zero": lambda st, r: len(r["IJn"]) == 0 and len(r["todo"]) > 0,
    "first_1": lambda st, r: st.first == 1,
    "first_50": lambda st, r: st.first == 50,
    "first_over": lambda st, r: st.first > _row_stats(st, r)[1].max(),
    "first_above_below": lambda st, r: (_row_stats(st, r)[2] < st.first).any() and (_row_stats(st, r)[2] > st.first).any(),
    "first_equal_ne": lambda st, r: all((np.sign(_row_stats(st, r)[2] - st.first) == s).any() for s in (-1, 0, 1)),
    "long_row_ties": _long_row_ties,
    "same_label_smallest": _same_label_smallest,
    "todo_empty": lambda st, r: len(r["todo"]) == 0 and len(r["IJn"]) > 0 and not r["ncm_before"].any(),
    "all_uncomputed": lambda st, r: st.ncm.all() and len(r["todo"]) > 0,
    "listed_twice": lambda st, r: len(np.unique(r["todo_pos"])) < len(r["todo_pos"]),
    "idle_rows": lambda st, r: any(len(p) > 0 and not r["ncm_before"][r["rows"][i][p]].any() for i, p in enumerate(r["picked"])) and len(r["todo"]) > 0,
    "nn1": lambda st, r: st.nn == 1,
    "nn3": lambda st, r: st.nn == 3,
    "nn16": lambda st, r: st.nn == 16,
    "few_computed": _few_computed,
    # a row with fewer than nn enemy entries, computed or not, next to same-label entries of both kinds: the graph reaches them
    "few_enemies": lambda st, r: any((st.y[o] != st.y[i]).sum() < st.nn for i, o in enumerate(r["others"])),
    "zero_row": lambda st, r: any(len(Ii) > st.nn and not np.concatenate([r["RA_f1"], r["RA_n1"]])[Ii].any() for Ii in r["rows"]),
    "wave_ties": _wave_ties,
    # a pair whose dad is an interior edge and whose clipped prediction the other bin rule would change
    "dad_on_edge": lambda st, r: (np.isin(r["feats_n"][:, 2], _interior(st)) & (_clip(r["feats_n"], r["pred_raw"]) != _clip(
        r["feats_n"], predict_raw(r["feats_n"], st.bins, st.W, st.c, left_closed=True)))).any(),
    "equal_edges": lambda st, r: len(set(_interior(st))) == 1 and len(_interior(st)) >= 3 and all(
        (m & _sane(r)).any() for m in (r["feats_n"][:, 2] < st.bins[1], r["feats_n"][:, 2] == st.bins[1], r["feats_n"][:, 2] > st.bins[1])),
    "clip_both": lambda st, r: ((r["pred_raw"] < r["feats_n"][:, 0]) & _sane(r)).any() and ((r["pred_raw"] > r["feats_n"][:, 1]) & _sane(r)).any(),
    "crossed_bounds": lambda st, r: (r["feats_n"][:, 0] > r["feats_n"][:, 1]).any() and np.array_equal(
        r["RA_n0"][r["feats_n"][:, 0] > r["feats_n"][:, 1]], r["feats_n"][r["feats_n"][:, 0] > r["feats_n"][:, 1], 1]),
    "clip_idle": lambda st, r: ((r["pred_raw"] > r["feats_n"][:, 0]) & (r["pred_raw"] < r["feats_n"][:, 1])).any(),
    "pred_route": lambda st, r: st.by_vector and len(r["IJn"]) > 0,
    "class_of_nn": lambda st, r: (np.bincount(st.y) == st.nn).any() and len(np.unique(st.y)) == 4,
    "two_labels": lambda st, r: len(np.unique(st.y)) == 2,
    "unsorted_codes": lambda st, r: (np.diff(st.y) < 0).any(),
    "new_pairs": lambda st, r: len(r["IJn"]) > 0,
    "device_metric": lambda st, r: st.device_metric and len(r["todo"]) > 0,
    "enemy_at_zero": lambda st, r: (r["ngd"][:, 0] == 0).any() and (r["ngd"][:, 0] > 0).any(),
}


def check_case(name, r=None):
    """Asserts that the case still reaches the edges it is listed for, on the reference's arrays (r: another run's arrays of the
    same form, e.g. assembled from the device's downloads)."""
    st = build(name)
    r = stages(name) if r is None else r
    len_f, ln, ne = _row_stats(st, r)
    assert ln.min() > st.nn, "%s: a row has no more than nn entries" % name
    assert np.bincount(st.y).min() >= st.nn and st.fit.nx <= 1030
    for tag in CASES[name]["edges"]:
        assert EDGES[tag](st, r), "%s no longer reaches its edge %s" % (name, tag)


# ------------------------------------------------------------------------------------------------------ dispatch mirror
KERNELS = ("k_en_thresh<1>", "k_en_thresh<2>", "k_en_thresh<4>", "k_en_thresh_wide", "k_en_keep_bits<1>", "k_en_keep_bits<2>",
           "k_en_keep_bits<4>", "k_en_keep_bits_wide", "k_row_prefix", "k_emit_pairs", "k_features", "k_en_predict", "k_en_clip",
           "k_en_first", "k_en_todo_pairs", "k_en_writeback[set_exact]", "k_en_writeback[device metric]", "k_en_graph", "k_en_pack")


def sid_words(na):       # ann_sid_words
    return 1 if na <= 64 else 2 if na <= 128 else 4 if na <= 256 else (na + 63) // 64


def sid_wide(na):        # ann_sid_wide
    return na > 256


def dispatch(name):
    """Kernels the host code launches for a case through candidates, download, predict, first, set_exact and graph."""
    st, r = build(name), stages(name)
    na, n, m = st.fit.na, len(r["IJn"]), len(r["todo"])
    out = ["k_en_thresh_wide", "k_en_keep_bits_wide"] if sid_wide(na) else ["k_en_thresh<%d>" % sid_words(na), "k_en_keep_bits<%d>" % sid_words(na)]
    out.append("k_row_prefix")
    if n > 0:
        out += ["k_emit_pairs", "k_features", "k_en_pack", "k_en_clip" if st.by_vector else "k_en_predict"]
    out.append("k_en_first")
    if m > 0:
        out += ["k_en_todo_pairs", "k_en_writeback[device metric]" if st.device_metric else "k_en_writeback[set_exact]"]
    out.append("k_en_graph")
    return out


if __name__ == "__main__":
    print("| case | nx | na | labels | loc_min | first | nn | new pairs | by larger row only | longest row | todo | edges |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for nm, cs in CASES.items():
        s, rr = build(nm), stages(nm)
        hit = [t for t in EDGES if EDGES[t](s, rr)]
        print("| %s | %d | %d | %s | %d | %d | %d | %d | %d | %d | %d | %s |" % (
            nm, s.fit.nx, s.fit.na, cs["labels"], s.loc_min, s.first, s.nn, len(rr["IJn"]), rr["only_larger"], _row_stats(s, rr)[1].max(),
            len(rr["todo"]), " ".join(hit)))
