"""
annchor_amd.radius -- host side of the exact fixed-radius graph (csrc/radius.hip; DESIGN.md, "Fixed-radius graphs").

The device classifies every pair i < j from the anchor table, emits the candidates (and, in connectivity mode, the pairs an
anchor proves inside) in row-major order, evaluates the candidates and keeps d <= r.  What is left for the host is the plan of
row ranges that respects `max_chunk_pairs`, the evaluation of the candidates when the metric is a Python callable, and
mirroring the upper triangle into a symmetric CSR.  `cluster` walks the same ranges for DBSCAN (csrc/dbscan.hip): the kept and
sure lists stay on the device, and labels and a core mask are all that comes back.  `exact_knn` walks them with one radius per
row for the exact k-NN graph (csrc/knnexact.hip): the radii come from a guess of the graph (`seed_radii`), the entries stay on the
device, and the rows' k smallest are all that comes back.

The second half of the file is the same for new points (`radius_query`): the engine holds X followed by Q, the device
classifies the rectangle queries x data (k_rad_classify_q) and the lists arrive query-major with ascending data index, so the
CSR over the queries is a counting sort.
"""
import numpy as np

from . import _native

DEFAULT_MAX_CHUNK_PAIRS = 1 << 26


class RadiusGraph:
    """Symmetric fixed-radius graph in CSR form: row i lists the points within r of i, ascending by index, no diagonal.
    indptr int64 [nx + 1], indices int64 [nnz], distances float64 [nnz] (None in connectivity mode)."""

    __slots__ = ("indptr", "indices", "distances")

    def __init__(self, indptr, indices, distances):
        self.indptr, self.indices, self.distances = indptr, indices, distances

    @property
    def nx(self):
        return len(self.indptr) - 1

    @property
    def nnz(self):
        return len(self.indices)

    def neighbors(self, i):
        """(indices, distances) of row i; distances is None in connectivity mode."""
        a, b = self.indptr[i], self.indptr[i + 1]
        return self.indices[a:b], (None if self.distances is None else self.distances[a:b])

    def degrees(self):
        return np.diff(self.indptr)

    def to_sparse_matrix(self):
        """DOK sparse matrix, symmetric.  As Annchor.to_sparse_matrix: every stored distance carries eps = nextafter(0, 1), so
        that pairs at distance 0 (duplicates) survive as explicit entries; in connectivity mode every entry is 1.0."""
        from scipy.sparse import csr_matrix

        nx = self.nx
        if self.distances is None:
            vals = np.ones(self.nnz, dtype=np.float64)
        else:
            vals = self.distances + np.nextafter(0, 1, dtype=np.float64)
        return csr_matrix((vals, self.indices, self.indptr), shape=(nx, nx), dtype=np.float64).todok()


class RadiusNeighbors:
    """Fixed-radius neighbours of new points in CSR form over the queries: row q lists the members of X within r of Q[q],
    ascending by index.  indptr int64 [nq + 1], indices int64 [nnz] (into X), distances float64 [nnz] (None in connectivity
    mode), nx = len(X)."""

    __slots__ = ("indptr", "indices", "distances", "nx")

    def __init__(self, indptr, indices, distances, nx):
        self.indptr, self.indices, self.distances, self.nx = indptr, indices, distances, int(nx)

    @property
    def nq(self):
        return len(self.indptr) - 1

    @property
    def nnz(self):
        return len(self.indices)

    def neighbors(self, q):
        """(indices, distances) of query q; distances is None in connectivity mode."""
        a, b = self.indptr[q], self.indptr[q + 1]
        return self.indices[a:b], (None if self.distances is None else self.distances[a:b])

    def degrees(self):
        return np.diff(self.indptr)

    def to_sparse_matrix(self):
        """DOK sparse matrix [nq, nx].  As RadiusGraph.to_sparse_matrix: every stored distance carries eps = nextafter(0, 1), so
        that a query equal to a data point keeps it as an explicit entry; in connectivity mode every entry is 1.0."""
        from scipy.sparse import csr_matrix

        if self.distances is None:
            vals = np.ones(self.nnz, dtype=np.float64)
        else:
            vals = self.distances + np.nextafter(0, 1, dtype=np.float64)
        return csr_matrix((vals, self.indices, self.indptr), shape=(self.nq, self.nx), dtype=np.float64).todok()

    def sorted_by_distance(self):
        """The same neighbours with every row ordered by (distance, index): nearest first, ties by ascending index."""
        if self.distances is None:
            raise ValueError("sorted_by_distance: a connectivity-mode result holds no distances; use mode='distance'")
        row = np.repeat(np.arange(self.nq, dtype=np.int64), self.degrees())
        order = np.lexsort((self.indices, self.distances, row))   # (last key first: row, then distance, then index)
        return RadiusNeighbors(self.indptr, self.indices[order], self.distances[order], self.nx)


def default_rtol(f, X):
    """The margin of the bound tests for a bundled metric: 0 where the computed distances are exact integers (the triangle
    inequality then holds exactly), 1e-4 for Euclidean distances of float32 rows, 1e-9 for anything computed in float64."""
    name = getattr(f, "name", None)
    if name == "levenshtein":
        return 0.0
    if name == "euclidean" and isinstance(X, np.ndarray) and X.dtype == np.float32:
        return 1e-4
    return 1e-9


def _plan(row_total, cap, stop, ncols):
    """Ranges [begin, end) of the rows [0, stop) in ascending order whose candidate totals stay within `cap` (a single row may
    exceed it: the caller splits that row by column range) and whose (row, column chunk) table stays within what one call
    takes; ncols(begin) is the number of columns of a range's table.  Ranges without candidates are left out."""
    n = len(row_total)
    cum = np.concatenate([[0], np.cumsum(row_total, dtype=np.int64)])
    out, start = [], 0
    while start < stop:
        nch = max(1, -(-int(ncols(start)) // _native.RADIUS_CHUNK_COLS))
        max_rows = max(1, _native.RADIUS_TABLE_MAX // nch)
        end = int(np.searchsorted(cum, cum[start] + cap, side="right")) - 1
        end = min(max(end, start + 1), start + max_rows, n)
        if cum[end] > cum[start]:
            out.append((start, end))
        start = end
    return out


def plan_ranges(row_total, cap):
    """The row ranges of the graph form (`_plan`): row i pairs with the columns behind it, and the last row with none."""
    nx = len(row_total)
    return _plan(row_total, cap, nx - 1, lambda start: nx - start - 1)


def plan_query_ranges(row_total, ncols, cap):
    """The query ranges of the query form (`_plan`): every query pairs with all `ncols` data columns."""
    return _plan(row_total, cap, len(row_total), lambda start: ncols)


def assemble_csr(nx, ij, d):
    """Upper-triangle pairs (int64 [n, 2], i < j, each once) and their values (or None) -> symmetric CSR, rows ascending."""
    from scipy.sparse import coo_matrix

    n = len(ij)
    if n == 0:
        return RadiusGraph(np.zeros(nx + 1, dtype=np.int64), np.zeros(0, dtype=np.int64), None if d is None else np.zeros(0, dtype=np.float64))
    i, j = ij[:, 0], ij[:, 1]
    # COO -> CSR is a counting sort by row and sort_indices orders the short rows: O(nnz) for bounded degrees.  The payload is
    # the entry's position (1-based: an explicit 0 would be a structural zero), so the distances are gathered, never summed.
    m = coo_matrix((np.arange(1, 2 * n + 1, dtype=np.int64), (np.concatenate([i, j]), np.concatenate([j, i]))), shape=(nx, nx)).tocsr()
    m.sort_indices()
    indptr = m.indptr.astype(np.int64)
    indices = m.indices.astype(np.int64)
    distances = None if d is None else np.ascontiguousarray(np.concatenate([d, d])[m.data - 1], dtype=np.float64)
    return RadiusGraph(indptr, indices, distances)


def check_radius(r, what="radius_graph", name="r"):
    r = float(r)
    if not r >= 0.0:   # (NaN included)
        raise ValueError("%s: %s must be a number >= 0 (got %r); a negative or NaN radius has no graph" % (what, name, r))
    return r


def walk_rows(row_total, nx, cap, rows_call, consume, what, query=False):
    """One rows_call(rb, re, cb, ce) per planned row range; a call whose last answer is negative emitted nothing (its range
    exceeds `cap`): a single over-full row is then bisected by column range.  consume(*answer) runs after every call that emitted
    its lists, while they are the engine's current ones.  A row range starts from the columns (rb + 1, nx) -- the graph form,
    pairs i < j of nx points -- or, with `query`, from (0, nx): the rows are queries and the columns the nx data points."""
    for rb, re in plan_query_ranges(row_total, nx, cap) if query else plan_ranges(row_total, cap):
        cols = (0, nx) if query else (rb + 1, nx)
        ans = rows_call(rb, re, *cols)
        if ans[-1] >= 0:
            consume(*ans)
            continue
        if re - rb > 1:
            raise RuntimeError("%s: a planned %s range exceeded max_chunk_pairs" % (what, "query" if query else "row"))   # (the plan sums the same counts)
        pieces = [cols]   # one row above the cap: column ranges, left to right
        while pieces:
            cb, ce = pieces.pop()
            ans = rows_call(rb, re, cb, ce)
            if ans[-1] < 0:
                mid = (cb + ce) // 2
                pieces += [(mid, ce), (cb, mid)]
            else:
                consume(*ans)


def check_cap(max_chunk_pairs, what):
    cap = DEFAULT_MAX_CHUNK_PAIRS if max_chunk_pairs is None else int(max_chunk_pairs)
    if cap < 1:
        raise ValueError("%s: max_chunk_pairs must be >= 1" % what)
    return cap


def walk_ranges(engine, nx, r, rtol, conn, use_bounds, max_chunk_pairs, on_device, consume, what="radius_graph"):
    """The range walk of `build` and `cluster`: count, plan the row ranges that respect `max_chunk_pairs`, one radius_rows call
    per range, a single over-full row bisected by column range.  consume(n_eval, n_sure, n_kept) runs after every call that
    emitted its lists, while they are the engine's current ones."""
    cap = check_cap(max_chunk_pairs, what)
    row_eval, row_sure = engine.radius_count(r, rtol, conn, use_bounds)
    walk_rows(row_eval + row_sure, nx, cap, lambda rb, re, cb, ce: engine.radius_rows(rb, re, cb, ce, cap, on_device), consume, what)


class PairCollector:
    """consume(n_eval, n_sure, n_kept) of `build` and `build_query`: fetches every range's kept pairs with their distances (or its
    candidates, which host_eval evaluates and r thresholds) and its sure pairs, and keeps the walk's accounting.  shift: the
    query form's pairs arrive as (j, nx_data + q) and are kept as (j, q)."""

    def __init__(self, engine, r, host_eval, shift=0):
        self.engine, self.r, self.host_eval, self.shift = engine, r, host_eval, shift
        self.kept_ij, self.kept_d, self.sure_ij = [], [], []
        self.n_eval = self.n_sure = self.chunks = 0

    def local(self, ij):   # (j, nx_data + q) -> (j, q)
        if self.shift:
            ij[:, 1] -= self.shift
        return ij

    def __call__(self, ne, ns, nk):
        self.n_eval, self.n_sure, self.chunks = self.n_eval + ne, self.n_sure + ns, self.chunks + 1
        if self.host_eval is None:
            if nk > 0:
                ij, d = self.engine.radius_fetch(_native.RADIUS_KEPT, nk, distances=True)
                self.kept_ij.append(self.local(ij))
                self.kept_d.append(d)
        elif ne > 0:
            cand = self.local(self.engine.radius_fetch(_native.RADIUS_EVAL, ne))
            d = np.asarray(self.host_eval(cand), dtype=np.float64)
            keep = d <= self.r
            self.kept_ij.append(cand[keep])
            self.kept_d.append(d[keep])
        if ns > 0:
            self.sure_ij.append(self.local(self.engine.radius_fetch(_native.RADIUS_SURE, ns)))

    def stats(self, pairs):
        return dict(pairs=pairs, evals=int(self.n_eval), sure=int(self.n_sure), pruned=int(pairs - self.n_eval - self.n_sure), chunks=self.chunks)


def build(engine, nx, r, mode, rtol, use_bounds, max_chunk_pairs, host_eval=None):
    """The graph and its accounting.  host_eval: None -- the engine's device metric evaluates the candidates; otherwise a
    callable IJ (int64 [n, 2]) -> float64 [n], and the candidates are downloaded for it."""
    if mode not in ("distance", "connectivity"):
        raise ValueError("radius_graph: mode must be 'distance' or 'connectivity'")
    conn = mode == "connectivity"
    got = PairCollector(engine, r, host_eval)
    walk_ranges(engine, nx, r, rtol, conn, use_bounds, max_chunk_pairs, host_eval is None, got)

    empty = np.zeros((0, 2), dtype=np.int64)
    ij = np.concatenate(got.kept_ij + got.sure_ij) if (got.kept_ij or got.sure_ij) else empty
    d = None if conn else (np.concatenate(got.kept_d) if got.kept_d else np.zeros(0, dtype=np.float64))
    return assemble_csr(nx, ij, d), got.stats(nx * (nx - 1) // 2)


# ------------------------------------------------------------------------------------------------------------ DBSCAN
class DBSCANResult:
    """DBSCAN labels of the fixed-radius graph at eps (csrc/dbscan.hip): labels int64 [nx] (-1: noise; clusters
    numbered by ascending smallest core index), core_sample_mask bool [nx], and the parameters they were computed for."""

    __slots__ = ("labels", "core_sample_mask", "n_clusters", "eps", "min_samples")

    def __init__(self, labels, core_sample_mask, n_clusters, eps, min_samples):
        self.labels, self.core_sample_mask = labels, core_sample_mask
        self.n_clusters, self.eps, self.min_samples = int(n_clusters), float(eps), int(min_samples)

    @property
    def nx(self):
        return len(self.labels)

    @property
    def core_sample_indices(self):
        """Ascending indices of the core points (sklearn's core_sample_indices_)."""
        return np.flatnonzero(self.core_sample_mask).astype(np.int64)

    @property
    def n_noise(self):
        return int(np.count_nonzero(self.labels < 0))


def check_min_samples(min_samples, what="dbscan"):
    """An integer >= 1 (the neighbourhood of a point includes the point); anything that is not an integer is refused, not rounded."""
    import numbers

    if isinstance(min_samples, bool) or not isinstance(min_samples, (numbers.Integral, np.integer)) or int(min_samples) < 1:
        raise ValueError("%s: min_samples must be an integer >= 1 (got %r)" % (what, min_samples))
    if int(min_samples) >= 1 << 31:
        raise ValueError("%s: min_samples must be below 2^31 (got %r)" % (what, min_samples))
    return int(min_samples)


def cluster(engine, nx, eps, min_samples, rtol, use_bounds, max_chunk_pairs, host_eval=None):
    """DBSCAN of the nx points and the accounting of the walk.  Always connectivity mode: no distance leaves the device, and the
    pairs an anchor proves inside are not evaluated.  host_eval None: every range's kept and sure lists go from the radius
    buffers to the device edge list (dbscan_absorb); otherwise the candidates are downloaded, evaluated by host_eval and
    thresholded here, and the kept and sure pairs are uploaded (dbscan_edges)."""
    on_device = host_eval is None
    n_eval = n_sure = n_edges = chunks = 0
    engine.dbscan_begin(min_samples)

    def consume(ne, ns, nk):
        nonlocal n_eval, n_sure, n_edges, chunks
        n_eval, n_sure, chunks = n_eval + ne, n_sure + ns, chunks + 1
        if on_device:
            if nk + ns > 0:
                n_edges += engine.dbscan_absorb()
            return
        parts = []
        if ne > 0:
            cand = engine.radius_fetch(_native.RADIUS_EVAL, ne)
            d = np.asarray(host_eval(cand), dtype=np.float64)
            parts.append(cand[d <= eps])
        if ns > 0:
            parts.append(engine.radius_fetch(_native.RADIUS_SURE, ns))
        if parts:
            ij = np.concatenate(parts)
            engine.dbscan_edges(ij)
            n_edges += len(ij)

    walk_ranges(engine, nx, eps, rtol, True, use_bounds, max_chunk_pairs, on_device, consume, what="dbscan")
    labels, core, n_clusters = engine.dbscan_finish()
    pairs = nx * (nx - 1) // 2
    stats = dict(pairs=pairs, evals=int(n_eval), sure=int(n_sure), pruned=int(pairs - n_eval - n_sure), chunks=chunks, edges=int(n_edges))
    return DBSCANResult(labels.astype(np.int64), core.astype(bool), n_clusters, eps, min_samples), stats


# ------------------------------------------------------------------------------------------------ exact k-NN graph
def seed_radii(nx, k, seed_idx, pairs_fn):
    """Per-row radii from a guess of the graph (int64 [nx, >= k]; the first k columns are read).  u[i] = the largest exact
    distance among row i's distinct entries != i when there are at least k - 1 of them, all in [0, nx): with i these are k
    distinct points within u[i], so the row's true k-th distance is <= u[i].  Any other row gets +inf (and so does a row whose
    distances hold a NaN).  Every unordered pair is evaluated once, as (smaller index, larger index) -- the orientation of the
    walk's candidates.  Returns (u float64 [nx], evaluations, rows with u = +inf)."""
    G = np.asarray(seed_idx)
    if G.ndim != 2 or G.shape[0] != nx or G.shape[1] < k or G.dtype.kind not in "iu":
        raise ValueError("exact_neighbor_graph: seed_graph must hold integer indices [nx=%d, >= %d], got %s %r" % (nx, k, G.dtype, G.shape))
    G = np.sort(G[:, :k].astype(np.int64), axis=1)
    own = np.arange(nx, dtype=np.int64)[:, None]
    use = G != own
    use[:, 1:] &= G[:, 1:] != G[:, :-1]
    valid = ~(use & ((G < 0) | (G >= nx))).any(axis=1) & (use.sum(axis=1) >= k - 1)
    use &= valid[:, None]
    i, j = np.broadcast_to(own, G.shape)[use], G[use]
    key, inv = np.unique(np.minimum(i, j) * nx + np.maximum(i, j), return_inverse=True)
    u = np.where(valid, 0.0, np.inf)
    if len(key):
        d = np.asarray(pairs_fn(np.stack([key // nx, key % nx], axis=1)), dtype=np.float64)
        with np.errstate(invalid="ignore"):
            np.maximum.at(u, i, d[inv.reshape(-1)])   # (np.maximum keeps a NaN)
    u[~(u >= 0.0)] = np.inf
    return u, int(len(key)), int(np.count_nonzero(np.isinf(u)))


def exact_knn(engine, nx, k, u, rtol, use_bounds, max_chunk_pairs, host_eval=None):
    """The exact k-NN graph of the nx points from upper bounds u[i] of the rows' k-th distances (csrc/knnexact.hip; DESIGN.md
    3.22), and the accounting of the walk.  host_eval None: the engine's device metric evaluates every range's candidates and
    they are absorbed where they are; otherwise the candidates are downloaded, evaluated by host_eval and uploaded with their
    distances (knn_exact_edges).  Returns ((idx int64 [nx, k], dist float64 [nx, k]), stats)."""
    what = "exact_neighbor_graph"
    cap = check_cap(max_chunk_pairs, what)
    on_device = host_eval is None
    n_eval = chunks = 0
    row_eval = engine.knn_exact_begin(k, u, rtol, use_bounds)

    def consume(ne, nn):
        nonlocal n_eval, chunks
        n_eval, chunks = n_eval + ne, chunks + 1
        if not on_device and ne > 0:
            cand = engine.knn_exact_fetch(ne)
            engine.knn_exact_edges(cand, np.asarray(host_eval(cand), dtype=np.float64))

    walk_rows(row_eval, nx, cap, lambda rb, re, cb, ce: engine.knn_exact_rows(rb, re, cb, ce, cap, on_device), consume, what)
    idx, dist, row_entries = engine.knn_exact_finish()
    pairs = nx * (nx - 1) // 2
    stats = dict(pairs=pairs, evals=int(n_eval), pruned=int(pairs - n_eval), chunks=chunks, entries=int(row_entries.sum()))
    return (idx, dist), stats


# ------------------------------------------------------------------------------------------- queries for new points
def assemble_query_csr(nq, nx, kept, kept_d, sure):
    """Pairs (j, q), q 0-based, as they were fetched -- query-major, ascending j inside a query -- to the CSR over the queries.
    A counting sort by query: the order inside a row is the order of arrival, which is checked, not produced.  Only a
    connectivity-mode result with both kinds of pairs is merged (two ascending lists per query)."""
    def key_of(parts):
        ij = np.concatenate(parts) if parts else np.zeros((0, 2), dtype=np.int64)
        key = ij[:, 1] * np.int64(max(nx, 1)) + ij[:, 0]
        assert np.all(key[1:] > key[:-1]), "radius_query: a fetched list is not query-major with ascending data index"
        return ij, key

    ij, key = key_of(kept)
    d = None if kept_d is None else (np.concatenate(kept_d) if kept_d else np.zeros(0, dtype=np.float64))
    if sure:
        sj, skey = key_of(sure)
        order = np.argsort(np.concatenate([key, skey]), kind="stable")
        ij = np.concatenate([ij, sj])[order]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(ij[:, 1], minlength=nq))]).astype(np.int64)
    return RadiusNeighbors(indptr, np.ascontiguousarray(ij[:, 0], dtype=np.int64), d, nx)


def build_query(engine, nx_data, nq, r, mode, rtol, use_bounds, max_chunk_pairs, host_eval=None):
    """The neighbours of the nq queries the engine holds after its nx_data data points, and the accounting.  Mirrors `build`:
    the same walk (`walk_rows`, query form) and collector, its own assembly.  host_eval: None -- the
    engine's device metric evaluates the candidates; otherwise a callable on int64 [n, 2] pairs (j, q), q 0-based, that
    returns float64 [n], and the candidates are downloaded for it."""
    if mode not in ("distance", "connectivity"):
        raise ValueError("radius_query: mode must be 'distance' or 'connectivity'")
    conn = mode == "connectivity"
    cap = check_cap(max_chunk_pairs, "radius_query")
    row_eval, row_sure = engine.radius_query_count(nx_data, r, rtol, conn, use_bounds)
    on_device = host_eval is None
    got = PairCollector(engine, r, host_eval, shift=nx_data)
    walk_rows(row_eval + row_sure, nx_data, cap, lambda qb, qe, cb, ce: engine.radius_query_rows(nx_data, qb, qe, cb, ce, cap, on_device), got,
              "radius_query", query=True)
    return assemble_query_csr(nq, nx_data, got.kept_ij, None if conn else got.kept_d, got.sure_ij), got.stats(nq * nx_data)
