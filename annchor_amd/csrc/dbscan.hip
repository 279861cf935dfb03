// dbscan.hip -- DBSCAN on the device from the edge list of the fixed-radius graph (no reference counterpart).
// The rule (include/annchor_hip.h states it; tests/dbscan_cases.py restates it in NumPy): a point is core iff degree + 1 >=
// min_samples; clusters are the connected components of the core-core edges, numbered by ascending smallest core index; a
// non-core point with core neighbours takes the smallest cluster number among them; everything else is -1.  The result is a
// pure function of the edge SET: every stage below is either an integer sum, a minimum, or a union-find whose roots are fixed
// by an invariant, so neither the order of the edges nor the scheduling of the threads changes a label.
//   absorb     a range's int2 pairs are appended to the edge list (device to device) and both end points' degrees counted
//   core       core[v] = deg[v] + 1 >= min_samples;  parent[v] = v;  label[v] = the sentinel
//   hook       lock-free union-find over the core-core edges: the larger root is hung under the smaller one by a compare-and-swap
//              on the larger root's own parent word.  parent[v] <= v always: no cycle can form, and a component's root is its
//              smallest core index whatever the interleaving
//   flatten    parent[v] = find(v) for core points, flag[v] = (v is its own root)
//   number     exclusive scan of the flags = the clusters' numbers;  label[v] = rank[parent[v]] for core points
//   border     every edge with exactly one core end: atomicMin of the core end's number into the other end's label
// Labels are kept as uint32 with the sentinel 0xffffffff: the minimum over unsigned values leaves it where no core neighbour
// wrote, and read as int32 it is the -1 of a noise point.
// Every access to `parent` inside hook and flatten is an agent-scope atomic (relaxed): the workgroups of one launch sit on
// different XCDs, whose L2s do not see each other's plain stores.
#include "common.h"

#define DB_THREADS 256
#define DB_MIN_EDGES (1ll << 12)          // first reservation of the edge list (32 KiB; doubled from there)
#define DB_MAX_EDGES ((1ll << 31) - 1)    // 16 GiB of int2; the per-edge grids stay below 2^23 workgroups
#define DB_NOISE 0xffffffffu

// out[t] = in[t] (COPY) and deg[x]++, deg[y]++ for every edge.  The radius lists are row-major, so the lanes of a wave mostly
// share x: a run of equal x inside the wave is one atomicAdd of its length by the run's first lane (integer sums: the totals do
// not depend on how they were grouped).  y ascends inside a row: one add per lane.
template <bool COPY>
__global__ __launch_bounds__(DB_THREADS) void k_db_absorb(const int2 *in, int2 *out, int64_t n, int32_t *__restrict__ deg)
{
    const int64_t t = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool ok = t < n;
    const int2 e = in[ok ? t : n - 1];
    if (COPY && ok) out[t] = e;
    int end;
    const bool lead = ann_wave_run(e.x, ok, lane, end);
    if (!ok) return;
    if (lead) atomicAdd(deg + e.x, end - lane);
    atomicAdd(deg + e.y, 1);
}

__global__ __launch_bounds__(DB_THREADS) void k_db_core(const int32_t *__restrict__ deg, int64_t nx, int32_t min_samples,
                                                        uint8_t *__restrict__ core, int32_t *__restrict__ parent, uint32_t *__restrict__ label)
{
    const int64_t v = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    if (v >= nx) return;
    core[v] = (int64_t)deg[v] + 1 >= (int64_t)min_samples ? 1 : 0;
    parent[v] = (int32_t)v;
    label[v] = DB_NOISE;
}

__device__ __forceinline__ int32_t db_ld(int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Root of v's tree, with path halving: every other node on the way is re-hung under its grandparent.  The re-hanging is an
// atomicMin: a parent word only ever decreases, and only to an ancestor, so concurrent finds and hooks never undo each other's work.
__device__ __forceinline__ int32_t db_find(int32_t *parent, int32_t v)
{
    for (;;) {
        const int32_t p = db_ld(parent + v);
        if (p == v) return v;
        const int32_t g = db_ld(parent + p);
        if (g == p) return p;
        (void)__hip_atomic_fetch_min(parent + v, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v = g;
    }
}

__global__ __launch_bounds__(DB_THREADS) void k_db_hook(const int2 *__restrict__ edges, int64_t n, const uint8_t *__restrict__ core, int32_t *parent)
{
    const int64_t t = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    if (t >= n) return;
    const int2 e = edges[t];
    if (!core[e.x] || !core[e.y]) return;
    int32_t a = db_find(parent, e.x), b = db_find(parent, e.y);
    while (a != b) {
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        // hi was a root when it was found; if it still is, it now hangs under lo < hi.  Otherwise somebody else hung it
        // elsewhere in between: find both roots again and retry (every failure is another thread's success: no livelock)
        int32_t expect = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &expect, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        a = db_find(parent, hi);
        b = db_find(parent, lo);
    }
}

__global__ __launch_bounds__(DB_THREADS) void k_db_flatten(const uint8_t *__restrict__ core, int64_t nx, int32_t *parent, int32_t *__restrict__ flag)
{
    const int64_t v = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    if (v >= nx) return;
    int32_t f = 0;
    if (core[v]) {
        const int32_t r = db_find(parent, (int32_t)v);
        // (the root is the smallest value parent[v] can take: after this minimum the word holds the root, whoever else halves)
        if (r != (int32_t)v) (void)__hip_atomic_fetch_min(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        f = r == (int32_t)v ? 1 : 0;
    }
    flag[v] = f;
}

// out: int64 n_clusters, then the labels
__global__ __launch_bounds__(DB_THREADS) void k_db_number(const uint8_t *__restrict__ core, int64_t nx, const int32_t *__restrict__ parent,
                                                          const int64_t *__restrict__ rank, uint32_t *__restrict__ label,
                                                          int64_t *__restrict__ n_clusters)
{
    const int64_t v = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    if (v >= nx) return;
    if (v == 0) *n_clusters = rank[nx];
    if (core[v]) label[v] = (uint32_t)rank[parent[v]];
}

__global__ __launch_bounds__(DB_THREADS) void k_db_border(const int2 *__restrict__ edges, int64_t n, const uint8_t *__restrict__ core, uint32_t *label)
{
    const int64_t t = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    if (t >= n) return;
    const int2 e = edges[t];
    const bool cx = core[e.x] != 0, cy = core[e.y] != 0;
    if (cx == cy) return;
    // (a core point's label was written by the previous launch and no thread of this one writes it)
    const int c = cx ? e.x : e.y, o = cx ? e.y : e.x;
    atomicMin(label + o, label[c]);
}

// Room for `more` edges behind the db_n_edges the list holds.
static int db_room(annchor_ctx *c, int64_t more)
{
    return rad_grow(c, c->db_edges, sizeof(int2), c->db_n_edges, more, DB_MIN_EDGES, DB_MAX_EDGES, "DBSCAN edge", "edges", "", __func__);
}

static bool db_ready(const annchor_ctx *c) { return c->db_begun && c->db_nx == c->nx && c->db_deg.p; }

extern "C" int annchor_dbscan_begin(annchor_ctx *c, int32_t min_samples)
{
    if (!c) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, c->nx >= 1, ANNCHOR_EINVAL, "no data set bound");
    ANN_REQUIRE(c, min_samples >= 1, ANNCHOR_EINVAL, "min_samples must be >= 1 (got %d)", (int)min_samples);
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    ANN_TRY(ann_side_join(c));
    c->db_begun = false;
    ANN_TRY(rad_reserve(c, c->db_deg, sizeof(int32_t) * (size_t)c->nx));
    ANN_CHECK_HIP(c, hipMemsetAsync(c->db_deg.p, 0, sizeof(int32_t) * (size_t)c->nx, c->stream));
    c->db_nx = c->nx;
    c->db_min_samples = min_samples;
    c->db_n_edges = 0;
    c->db_absorbed_serial = 0;
    c->db_begun = true;
    return ANNCHOR_OK;
}

extern "C" int annchor_dbscan_absorb(annchor_ctx *c, int64_t *n_edges)
{
    if (!c || !n_edges) return ANNCHOR_EINVAL;
    *n_edges = 0;
    ANN_REQUIRE(c, db_ready(c), ANNCHOR_EINVAL, "annchor_dbscan_begin has not run on this data set");
    ANN_REQUIRE(c, c->rad_params && c->rad_nx == c->nx && c->rad_serial > 0, ANNCHOR_EINVAL, "no radius range has been processed on this data set");
    ANN_REQUIRE(c, c->rad_nxd == 0, ANNCHOR_EINVAL,
                "the last radius range is of the query form (queries x data): its pairs are not edges between the points of one data set");
    ANN_REQUIRE(c, c->rad_evaluated || c->rad_n_eval == 0, ANNCHOR_EINVAL,
                "the last radius range was not evaluated and holds %lld candidates: their membership is unknown (evaluate them on the "
                "host and pass the pairs to annchor_dbscan_edges)", (long long)c->rad_n_eval);
    ANN_REQUIRE(c, c->db_absorbed_serial != c->rad_serial, ANNCHOR_EINVAL, "the last radius range has been absorbed already");
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    const int64_t nk = c->rad_n_kept, ns = c->rad_n_sure;
    if (nk + ns > 0) {
        ANN_TRY(db_room(c, nk + ns));
        int2 *tail = c->db_edges.as<int2>() + c->db_n_edges;
        ProfScope ps(c, "dbscan_absorb", (double)(nk + ns) * 16.0);
        if (nk > 0) k_db_absorb<true><<<ann_blocks(nk, DB_THREADS), DB_THREADS, 0, c->stream>>>(c->rad_kept.as<int2>(), tail, nk, c->db_deg.as<int32_t>());
        if (ns > 0) k_db_absorb<true><<<ann_blocks(ns, DB_THREADS), DB_THREADS, 0, c->stream>>>(c->rad_sure.as<int2>(), tail + nk, ns, c->db_deg.as<int32_t>());
        ANN_CHECK_HIP(c, hipGetLastError());
        c->db_n_edges += nk + ns;
    }
    c->db_absorbed_serial = c->rad_serial;
    *n_edges = nk + ns;
    return ANNCHOR_OK;
}

extern "C" int annchor_dbscan_edges(annchor_ctx *c, const int64_t *ij, int64_t n)
{
    if (!c || n < 0 || (n > 0 && !ij)) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, db_ready(c), ANNCHOR_EINVAL, "annchor_dbscan_begin has not run on this data set");
    if (n == 0) return ANNCHOR_OK;
    std::vector<int2> tmp;
    ANN_TRY(rad_pairs_in(c, ij, n, c->nx, "edge", tmp));
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    ANN_TRY(db_room(c, n));
    int2 *tail = c->db_edges.as<int2>() + c->db_n_edges;
    ANN_TRY(ann_h2d(c, tail, tmp.data(), sizeof(int2) * (size_t)n));
    {
        ProfScope ps(c, "dbscan_absorb", (double)n * 8.0);   // (the degree count alone: the upload is not a kernel)
        k_db_absorb<false><<<ann_blocks(n, DB_THREADS), DB_THREADS, 0, c->stream>>>(tail, nullptr, n, c->db_deg.as<int32_t>());
    }
    ANN_CHECK_HIP(c, hipGetLastError());
    c->db_n_edges += n;
    return ANNCHOR_OK;
}

extern "C" int annchor_dbscan_finish(annchor_ctx *c, int32_t *labels, uint8_t *core, int64_t *n_clusters)
{
    if (!c || !labels || !core || !n_clusters) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, db_ready(c), ANNCHOR_EINVAL, "annchor_dbscan_begin has not run on this data set");
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    ANN_TRY(ann_side_join(c));
    const int64_t nx = c->nx, n = c->db_n_edges;
    // one block for the download: int64 n_clusters | uint32 labels [nx] | uint8 core [nx]
    const size_t lab_off = sizeof(int64_t), core_off = lab_off + sizeof(uint32_t) * (size_t)nx, out_bytes = core_off + (size_t)nx;
    ANN_TRY(rad_reserve(c, c->db_out, out_bytes));
    ANN_TRY(rad_reserve(c, c->db_parent, sizeof(int32_t) * 2 * (size_t)nx));
    ANN_TRY(rad_reserve(c, c->db_rank, sizeof(int64_t) * (size_t)(nx + 1)));
    // (the scan's block sums, one per 2048 items -- room for one per 1024: reserved here so that the scan finds them and
    // carves nothing from the slab)
    ANN_TRY(rad_reserve(c, c->scan_tmp, sizeof(int64_t) * (size_t)(nx / 1024 + 2)));
    char *out = c->db_out.as<char>();
    int64_t *d_ncl = reinterpret_cast<int64_t *>(out);
    uint32_t *d_label = reinterpret_cast<uint32_t *>(out + lab_off);
    uint8_t *d_core = reinterpret_cast<uint8_t *>(out + core_off);
    int32_t *parent = c->db_parent.as<int32_t>(), *flag = parent + nx;
    const int2 *edges = c->db_edges.as<int2>();
    const int vb = ann_blocks(nx, DB_THREADS), eb = ann_blocks(n, DB_THREADS);
    ANN_CHECK_HIP(c, hipEventRecord(c->call_a, c->stream));
    {
        ProfScope ps(c, "dbscan_core", (double)nx * 13.0);
        k_db_core<<<vb, DB_THREADS, 0, c->stream>>>(c->db_deg.as<int32_t>(), nx, c->db_min_samples, d_core, parent, d_label);
    }
    if (n > 0) {
        ProfScope ps(c, "dbscan_hook", (double)n * 10.0);
        k_db_hook<<<eb, DB_THREADS, 0, c->stream>>>(edges, n, d_core, parent);
    }
    {
        ProfScope ps(c, "dbscan_flatten", (double)nx * 9.0);
        k_db_flatten<<<vb, DB_THREADS, 0, c->stream>>>(d_core, nx, parent, flag);
    }
    ANN_CHECK_HIP(c, hipGetLastError());
    ANN_TRY(ann_exclusive_scan_i32_to_i64(c, flag, c->db_rank.as<int64_t>(), nx));
    {
        ProfScope ps(c, "dbscan_number", (double)nx * 17.0);
        k_db_number<<<vb, DB_THREADS, 0, c->stream>>>(d_core, nx, parent, c->db_rank.as<int64_t>(), d_label, d_ncl);
    }
    if (n > 0) {
        ProfScope ps(c, "dbscan_border", (double)n * 10.0);
        k_db_border<<<eb, DB_THREADS, 0, c->stream>>>(edges, n, d_core, d_label);
    }
    ANN_CHECK_HIP(c, hipEventRecord(c->call_b, c->stream));
    c->call_timed = true;
    ANN_CHECK_HIP(c, hipGetLastError());
    std::vector<unsigned char> host(out_bytes);
    ANN_TRY(ann_d2h(c, host.data(), out, out_bytes));
    memcpy(n_clusters, host.data(), sizeof(int64_t));
    memcpy(labels, host.data() + lab_off, sizeof(int32_t) * (size_t)nx);
    memcpy(core, host.data() + core_off, (size_t)nx);
    return ANNCHOR_OK;
}
