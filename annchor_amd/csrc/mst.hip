// mst.hip -- the exact minimum spanning tree of the complete distance graph by Boruvka rounds on the device (no
// reference counterpart).  Edge weights are d(i, j) as the metric computes them for (smaller index, larger index); ties are
// broken by the strict total order (ann_key_asc(d), i, j), i < j, under which the tree is unique: the result is a pure function
// of X and the metric, whatever the scheduling.  The state is comp[v], the smallest index of v's component.  A round:
//   bridges    every component c gets one real crossing pair: the (i, A[a]), i in c, comp[A[a]] != c, that minimises Dt[a][i], then
//              i, then a (k_mst_guide: points on lanes, anchors looped, the anchors' components in LDS; two passes of 64-bit
//              atomicMin per component, the key and then the packed indices) -- Dt is a GUIDE here, never a weight.  A component
//              with no anchor outside it takes (its smallest member, the smallest member of the next component, cyclically).
//              Round 0 adds the seed partners' pairs.  The pairs are evaluated and go into the pool unconditionally.
//   bounds     ub[c] = the smallest evaluated distance among the pool's entries that cross out of c (a rigorous upper bound of
//              c's lightest outgoing edge: it IS an outgoing edge), U[v] = ub[comp[v]]
//   classify   the row classifier of radius.h under RadComponent: OUT if comp[i] == comp[j], else the per-row-radius rule
//              with R = max(U[i], U[j]); the same table, scan and k_rad_emit as the fixed-radius and exact k-NN walks
//   absorb     an evaluated candidate with d <= max(U[i], U[j]) is appended to the pool (one tail add per workgroup); a NaN
//              passes no test.  The pool persists across rounds
//   pick       pass one: atomicMin of the key into both sides' components for every crossing entry; pass two: the entries at
//              a side's key atomicMin (i << 32 | j) there.  Every component now holds its lightest outgoing edge under the total
//              order: that edge has d* <= ub[c] <= R, so no anchor excluded it and its absorb test passed, and so did every
//              other crossing edge of weight <= ub[c] -- ties are decided over all of them
//   take       one thread per component appends its edge to the tree (the end with the smaller comp when both chose it) and
//              hooks the two roots (unionfind.h); flatten sets comp[v] = root and the roots are counted and listed by a scan
// Under a strict order the chosen edges form a forest and each is a tree edge by the cut property; a round at least halves
// the components.  The pool may hold a pair more than once (a bridge is also a candidate of its round, and candidates are
// re-evaluated in later rounds): minima over equal values are the same values.  Entries that became internal are skipped by
// every pass and are not compacted away (DESIGN.md 3.23 has the measurement behind that choice).
//
// The reach form (annchor_mst_begin_reach) is the same rounds over mutual-reachability weights
// w(i, j) = max(d(i, j), core[i], core[j]) -- HDBSCAN*'s tree -- under the order (ann_key_asc(w), i, j).  What differs:
//   seeds      round 0 takes every entry of an integer seed graph [nx, cols] that is another point (k_mst_seed: one thread per
//              slot), not one partner per point: with the exact k-NN graph that gave the core distances every bound is tight
//              from round 0
//   absorb     k_mst_absorb<true> forms w from the evaluated d and the two core distances, tests w <= max(U[i], U[j]) and stores
//              w: the pool, ub and U hold weights, so bounds, pick, take and flatten run unchanged
//   classify   RadReach (radius.h): RadComponent's veto, or max(core[i], core[j]) > max(U[i], U[j]) -- exact, no rtol, no
//              anchor, no triangle inequality; the anchors' rule runs on d as before, and d <= w
// A component's lightest outgoing edge e* has max(core) <= w* <= ub[c] <= R and d* <= w* <= R: neither the veto nor an anchor
// excludes it and its absorb test passes, as does that of every other crossing edge of weight <= ub[c].
#include "common.h"
#include "radius.h"
#include "unionfind.h"

#include <algorithm>
#include <cmath>

#define MST_THREADS 256
#define MST_MIN_POOL (1ll << 12)          // first reservation of the pool (64 KiB; doubled from there)
#define MST_MAX_POOL ((1ll << 31) - 1)    // the per-entry grids stay below 2^23 workgroups
#define MST_NONE (~0ull)

struct __attribute__((aligned(16))) MstEdge {
    int32_t i, j;   // i < j
    double d;
};

__global__ __launch_bounds__(MST_THREADS) void k_mst_init(int64_t nx, int32_t *__restrict__ comp, int32_t *__restrict__ parent,
                                                         int32_t *__restrict__ flag)
{
    const int64_t v = (int64_t)blockIdx.x * MST_THREADS + threadIdx.x;
    if (v >= nx) return;
    comp[v] = parent[v] = (int32_t)v;
    flag[v] = 1;
}

__global__ __launch_bounds__(MST_THREADS) void k_mst_fill(uint64_t *__restrict__ p, int64_t n, uint64_t v)
{
    const int64_t t = (int64_t)blockIdx.x * MST_THREADS + threadIdx.x;
    if (t < n) p[t] = v;
}

// roots[rank[v]] = v for every root: the components' smallest members in ascending order
__global__ __launch_bounds__(MST_THREADS) void k_mst_roots(const int32_t *__restrict__ flag, const int64_t *__restrict__ rank, int64_t nx,
                                                          int32_t *__restrict__ roots)
{
    const int64_t v = (int64_t)blockIdx.x * MST_THREADS + threadIdx.x;
    if (v < nx && flag[v]) roots[rank[v]] = (int32_t)v;
}

// Bridge pass one.  Lane = point i: Dt[a][i] is a coalesced load for every anchor a; the anchors' components sit in LDS and are
// read as broadcasts.  The lane keeps the smallest (key, a) among the anchors outside its component (strict <: the smallest a
// at equal keys), writes it for pass two and lowers its component's key.  A key is clamped below the "none" word.
__global__ __launch_bounds__(MST_THREADS) void k_mst_guide(const double *__restrict__ Dt, const int32_t *__restrict__ A, int nA, int64_t nx,
                                                          const int32_t *__restrict__ comp, uint64_t *__restrict__ gkey,
                                                          int32_t *__restrict__ ganc, uint64_t *bkey)
{
    __shared__ int32_t shA[ANN_MAX_ANCHORS];
    for (int a = threadIdx.x; a < nA; a += MST_THREADS) shA[a] = comp[A[a]];
    __syncthreads();
    const int64_t v = (int64_t)blockIdx.x * MST_THREADS + threadIdx.x;
    const bool ok = v < nx;
    const int64_t vc = ok ? v : nx - 1;
    const int32_t ci = comp[vc];
    uint64_t best = MST_NONE;
    int32_t ba = 0;
#pragma unroll 4
    for (int a = 0; a < nA; ++a) {
        uint64_t k = ann_key_asc(Dt[(size_t)a * (size_t)nx + (size_t)vc]);
        if (k == MST_NONE) k = MST_NONE - 1ull;
        if (shA[a] != ci && k < best) { best = k; ba = a; }
    }
    if (!ok) return;
    gkey[v] = best;
    ganc[v] = ba;
    if (best != MST_NONE) atomicMin((unsigned long long *)bkey + ci, (unsigned long long)best);
}

// Bridge pass two: the points at their component's key lower its packed (point, anchor) word: the smallest i, then the smallest a
__global__ __launch_bounds__(MST_THREADS) void k_mst_bridge_pick(int64_t nx, const int32_t *__restrict__ comp, const uint64_t *__restrict__ gkey,
                                                                const int32_t *__restrict__ ganc, const uint64_t *__restrict__ bkey,
                                                                uint64_t *bpair)
{
    const int64_t v = (int64_t)blockIdx.x * MST_THREADS + threadIdx.x;
    if (v >= nx) return;
    const uint64_t k = gkey[v];
    const int32_t ci = comp[v];
    if (k != MST_NONE && k == bkey[ci]) atomicMin((unsigned long long *)bpair + ci, ((unsigned long long)v << 32) | (unsigned long long)(uint32_t)ganc[v]);
}

// One thread per component, at the position of its rank: its bridge (i, A[a]), or -- no anchor outside it -- (its smallest
// member, the next component's smallest member, cyclically), as (min, max).  ncomp >= 2: the two ends differ.
__global__ __launch_bounds__(MST_THREADS) void k_mst_bridge_emit(const int32_t *__restrict__ roots, int64_t ncomp, const uint64_t *__restrict__ bpair,
                                                                const int32_t *__restrict__ A, int2 *__restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * MST_THREADS + threadIdx.x;
    if (r >= ncomp) return;
    const int32_t v = roots[r];
    const uint64_t bp = bpair[v];
    int32_t i = v, j;
    if (bp != MST_NONE) {
        i = (int32_t)(bp >> 32);
        j = A[(uint32_t)bp];
    } else {
        j = roots[r + 1 < ncomp ? r + 1 : 0];
    }
    out[r] = make_int2(i < j ? i : j, i < j ? j : i);
}

// The kept lanes of a workgroup take consecutive places behind *tail with one agent-scope add: the waves' counts meet in LDS,
// thread 0 reserves the workgroup's places, and a lane's place is the workgroup's base + the counts of the waves before its own
// + its rank in the wave's ballot.  Every thread of the workgroup calls it; -1 for a lane that keeps nothing.
__device__ __forceinline__ int64_t mst_place(bool keep, unsigned long long *tail)
{
    __shared__ int wcnt[MST_THREADS / 64];
    __shared__ unsigned long long base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t m = __ballot(keep);
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int w = 0; w < MST_THREADS / 64; ++w) tot += wcnt[w];
        base = tot ? atomicAdd(tail, (unsigned long long)tot) : 0ull;
    }
    __syncthreads();
    if (!keep) return -1;
    int before = 0;
    for (int w = 0; w < wave; ++w) before += wcnt[w];
    return (int64_t)base + before + __popcll(m & ((1ull << lane) - 1ull));
}

// One pass over evaluated pairs: those with w <= max(u[i], u[j]) -- every pair that is not NaN when u is null (the bridges) -- are
// appended behind *tail as (min, max, w), one tail add per workgroup (mst_place).  w = d, or in the reach form (REACH)
// max(d, core[i], core[j]): a NaN d stays a NaN (no comparison with it is true) and passes no test.
template <bool REACH>
__global__ __launch_bounds__(MST_THREADS) void k_mst_absorb(const int2 *__restrict__ ij, const double *__restrict__ d, int64_t n,
                                                           const double *__restrict__ u, const double *__restrict__ core,
                                                           MstEdge *__restrict__ pool, int64_t cap, unsigned long long *tail)
{
    const int64_t t = (int64_t)blockIdx.x * MST_THREADS + threadIdx.x;
    const bool ok = t < n;
    const int2 e = ij[ok ? t : n - 1];
    double v = d[ok ? t : n - 1];
    if (REACH) {
        const double a = core[e.x], b = core[e.y];
        if (a > v) v = a;
        if (b > v) v = b;
    }
    double R = __longlong_as_double(0x7ff0000000000000ll);
    if (u) {
        const double a = u[e.x], b = u[e.y];
        R = a > b ? a : b;
    }
    const int64_t p = mst_place(ok && v <= R, tail);   // (v <= R: false for a NaN)
    if (p >= 0 && p < cap) {   // (p < cap always: the pool has room for every pair of the pass)
        MstEdge o;
        o.i = e.x < e.y ? e.x : e.y;
        o.j = e.x < e.y ? e.y : e.x;
        o.d = v;
        pool[p] = o;
    }
}

// The reach form's seeds.  One thread per (row, slot) of the seed graph G (int64 [nx][cols], any values): an entry that is
// another point of 0..nx-1 becomes the pair (min, max) behind *tail, one tail add per workgroup.  A mutual pair arrives twice:
// the pool tolerates duplicates.
__global__ __launch_bounds__(MST_THREADS) void k_mst_seed(const int64_t *__restrict__ G, int64_t nx, int64_t cols, int2 *__restrict__ out,
                                                         unsigned long long *tail)
{
    const int64_t n = nx * cols, t = (int64_t)blockIdx.x * MST_THREADS + threadIdx.x;
    const bool ok = t < n;
    const int64_t tc = ok ? t : n - 1, i = tc / cols, g = G[tc];
    const int64_t p = mst_place(ok && g >= 0 && g < nx && g != i, tail);
    if (p >= 0 && p < n) out[p] = make_int2((int)(i < g ? i : g), (int)(i < g ? g : i));   // (p < n always: at most one pair per slot)
}

__device__ __forceinline__ uint64_t mst_ld(uint64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Every crossing entry lowers both sides' keys (the bounds pass and the pick's pass one).  A word only ever decreases, so a
// key that is not below what the word holds now needs no atomic.
__global__ __launch_bounds__(MST_THREADS) void k_mst_cross_min(const MstEdge *__restrict__ pool, int64_t n, const int32_t *__restrict__ comp,
                                                              uint64_t *mkey)
{
    const int64_t t = (int64_t)blockIdx.x * MST_THREADS + threadIdx.x;
    if (t >= n) return;
    const MstEdge e = pool[t];
    const int32_t ci = comp[e.i], cj = comp[e.j];
    if (ci == cj) return;
    const uint64_t k = ann_key_asc(e.d);
    if (k < mst_ld(mkey + ci)) atomicMin((unsigned long long *)mkey + ci, (unsigned long long)k);
    if (k < mst_ld(mkey + cj)) atomicMin((unsigned long long *)mkey + cj, (unsigned long long)k);
}

// U[v] = ub[comp[v]]; +inf where nothing crosses out of the component
__global__ __launch_bounds__(MST_THREADS) void k_mst_radii(int64_t nx, const int32_t *__restrict__ comp, const uint64_t *__restrict__ mkey,
                                                          double *__restrict__ u)
{
    const int64_t v = (int64_t)blockIdx.x * MST_THREADS + threadIdx.x;
    if (v >= nx) return;
    const uint64_t k = mkey[comp[v]];
    u[v] = k == MST_NONE ? __longlong_as_double(0x7ff0000000000000ll) : ann_key_asc_inv(k);
}

// The row classifier of radius.h with one radius per point and the component veto; no SURE class.
template <bool TABLE>
__global__ __launch_bounds__(RAD_ROWS) void k_mst_classify(const double *__restrict__ Dt, const double *__restrict__ u,
                                                          const int32_t *__restrict__ comp, int64_t nx, int na, double rtol, int64_t row_begin,
                                                          int64_t row_end, int64_t col_begin, int64_t col_end, int64_t nchunks,
                                                          uint64_t *__restrict__ mask_eval, int32_t *__restrict__ cnt_eval,
                                                          unsigned long long *__restrict__ row_eval)
{
    __shared__ double shu[RAD_COLS];
    __shared__ int32_t shc[RAD_COLS];
    rad_classify_rows<false, TABLE>(RadComponent{u, comp, shu, shc, 0.0, 0}, Dt, nx, na, rtol, row_begin, row_end, col_begin, col_end, nchunks,
                                    mask_eval, nullptr, cnt_eval, nullptr, row_eval, nullptr);
}

// The reach form: the same body under RadReach -- the component veto or the core veto, then the anchors on d.
template <bool TABLE>
__global__ __launch_bounds__(RAD_ROWS) void k_mst_classify_reach(const double *__restrict__ Dt, const double *__restrict__ u,
                                                                const int32_t *__restrict__ comp, const double *__restrict__ core, int64_t nx,
                                                                int na, double rtol, int64_t row_begin, int64_t row_end, int64_t col_begin,
                                                                int64_t col_end, int64_t nchunks, uint64_t *__restrict__ mask_eval,
                                                                int32_t *__restrict__ cnt_eval, unsigned long long *__restrict__ row_eval)
{
    __shared__ double shu[RAD_COLS], shk[RAD_COLS];
    __shared__ int32_t shc[RAD_COLS];
    rad_classify_rows<false, TABLE>(RadReach{u, comp, core, shu, shc, shk, 0.0, 0.0, 0}, Dt, nx, na, rtol, row_begin, row_end, col_begin, col_end,
                                    nchunks, mask_eval, nullptr, cnt_eval, nullptr, row_eval, nullptr);
}

// Pick pass two: a crossing entry at a side's key lowers that side's packed edge word
__global__ __launch_bounds__(MST_THREADS) void k_mst_cross_edge(const MstEdge *__restrict__ pool, int64_t n, const int32_t *__restrict__ comp,
                                                               const uint64_t *__restrict__ mkey, uint64_t *medge)
{
    const int64_t t = (int64_t)blockIdx.x * MST_THREADS + threadIdx.x;
    if (t >= n) return;
    const MstEdge e = pool[t];
    const int32_t ci = comp[e.i], cj = comp[e.j];
    if (ci == cj) return;
    const uint64_t k = ann_key_asc(e.d);
    const unsigned long long w = ((unsigned long long)(uint32_t)e.i << 32) | (unsigned long long)(uint32_t)e.j;
    if (k == mkey[ci]) atomicMin((unsigned long long *)medge + ci, w);
    if (k == mkey[cj]) atomicMin((unsigned long long *)medge + cj, w);
}

// One thread per component: its edge goes to the tree -- one tail add per wave -- unless the other end chose the same edge and
// has the smaller comp; the two roots are hooked.  stat[1]: the tree's tail; stat[2]: components left without an edge.
__global__ __launch_bounds__(MST_THREADS) void k_mst_take(const int32_t *__restrict__ roots, int64_t ncomp, const int32_t *__restrict__ comp,
                                                         const uint64_t *__restrict__ mkey, const uint64_t *__restrict__ medge,
                                                         int32_t *parent, MstEdge *__restrict__ tree, int64_t cap, unsigned long long *stat)
{
    const int64_t r = (int64_t)blockIdx.x * MST_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool ok = r < ncomp;
    const int32_t v = roots[ok ? r : ncomp - 1];
    const uint64_t e = medge[v];
    const bool has = ok && e != MST_NONE;
    int32_t i = 0, j = 0, other = v;
    bool append = false;
    if (has) {
        i = (int32_t)(e >> 32);
        j = (int32_t)(uint32_t)e;
        const int32_t ci = comp[i];
        other = ci == v ? comp[j] : ci;
        append = !(medge[other] == e && other < v);
    }
    const uint64_t ma = __ballot(append), mo = __ballot(ok && !has);
    if (ma) {
        const int first = __ffsll((long long)ma) - 1;
        unsigned long long base = 0ull;
        if (lane == first) base = atomicAdd(stat + 1, (unsigned long long)__popcll(ma));
        base = __shfl(base, first);
        const int64_t p = (int64_t)base + __popcll(ma & ((1ull << lane) - 1ull));
        if (append && p < cap) {   // (always: the chosen edges form a forest)
            MstEdge o;
            o.i = i; o.j = j; o.d = ann_key_asc_inv(mkey[v]);
            tree[p] = o;
        }
    }
    if (mo && lane == __ffsll((long long)mo) - 1) atomicAdd(stat + 2, (unsigned long long)__popcll(mo));
    if (has) uf_union(parent, v, other);
}

__global__ __launch_bounds__(MST_THREADS) void k_mst_flatten(int64_t nx, int32_t *parent, int32_t *__restrict__ comp, int32_t *__restrict__ flag)
{
    const int64_t v = (int64_t)blockIdx.x * MST_THREADS + threadIdx.x;
    if (v >= nx) return;
    const int32_t r = uf_flatten(parent, (int32_t)v);
    comp[v] = r;
    flag[v] = r == (int32_t)v ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------ host side
static bool mst_ready(const annchor_ctx *c) { return c->mst_begun && c->mst_nx == c->nx && c->mst_comp.p && c->mst_key.p; }
#define MST_REQUIRE_BEGUN(c) ANN_REQUIRE(c, mst_ready(c), ANNCHOR_EINVAL, "annchor_mst_begin has not run on this data set")

static int mst_na(const annchor_ctx *c) { return c->mst_use_bounds ? c->na : 0; }

// the components' ranks, their roots in ascending order and their number
static int mst_number(annchor_ctx *c)
{
    const int64_t nx = c->nx;
    int32_t *flag = c->mst_comp.as<int32_t>() + 2 * nx;
    int64_t *rank = c->mst_rank.as<int64_t>();
    ANN_TRY(ann_exclusive_scan_i32_to_i64(c, flag, rank, nx));
    k_mst_roots<<<ann_blocks(nx, MST_THREADS), MST_THREADS, 0, c->stream>>>(flag, rank, nx, reinterpret_cast<int32_t *>(rank + nx + 1));
    ANN_CHECK_HIP(c, hipGetLastError());
    return ann_d2h(c, &c->mst_n_comp, rank + nx, sizeof(int64_t));
}

// the n pairs of rad_eval with the distances of rad_d into the pool; bridge: no test but "is a number"
static int mst_absorb(annchor_ctx *c, int64_t n, bool bridge, int64_t *added)
{
    *added = 0;
    if (n == 0) return ANNCHOR_OK;
    ANN_TRY(rad_grow(c, c->mst_pool, sizeof(MstEdge), c->mst_n_pool, n, MST_MIN_POOL, MST_MAX_POOL, "spanning-tree pool", "entries",
                     ": pass a smaller max_pairs", __func__));
    const int64_t cap = (int64_t)(c->mst_pool.cap / sizeof(MstEdge));
    unsigned long long *tail = c->mst_stat.as<unsigned long long>();
    {
        ProfScope ps(c, "mst_absorb", (double)n * 32.0);
        const double *u = bridge ? nullptr : c->mst_u.as<double>();
        const unsigned grid = ann_blocks(n, MST_THREADS);
        if (c->mst_reach)
            k_mst_absorb<true><<<grid, MST_THREADS, 0, c->stream>>>(c->rad_eval.as<int2>(), c->rad_d.as<double>(), n, u, c->mst_core.as<double>(),
                                                                   c->mst_pool.as<MstEdge>(), cap, tail);
        else
            k_mst_absorb<false><<<grid, MST_THREADS, 0, c->stream>>>(c->rad_eval.as<int2>(), c->rad_d.as<double>(), n, u, nullptr,
                                                                    c->mst_pool.as<MstEdge>(), cap, tail);
    }
    ANN_CHECK_HIP(c, hipGetLastError());
    int64_t total = 0;
    ANN_TRY(ann_d2h(c, &total, tail, sizeof(int64_t)));
    ANN_REQUIRE(c, total >= c->mst_n_pool && total - c->mst_n_pool <= n && total <= cap, ANNCHOR_ESTATE,
                "the absorb pass left %lld pool entries behind %lld from %lld pairs", (long long)total, (long long)c->mst_n_pool, (long long)n);
    *added = total - c->mst_n_pool;
    c->mst_n_pool = total;
    return ANNCHOR_OK;
}

static int mst_evaluate(annchor_ctx *c, int64_t n)
{
    ANN_TRY(rad_reserve(c, c->rad_d, sizeof(double) * (size_t)n));
    PairSource src;
    src.ij = c->rad_eval.as<int2>();
    src.n = n;
    return ann_metric_launch(c, src, c->rad_d.as<double>(), nullptr, nullptr);
}

// slots [first, first + count) of mst_key (uint64 [4][nx]) back to "none"
static int mst_clear_keys(annchor_ctx *c, int first, int count)
{
    const int64_t n = (int64_t)count * c->nx;
    k_mst_fill<<<ann_blocks(n, MST_THREADS), MST_THREADS, 0, c->stream>>>(c->mst_key.as<uint64_t>() + (int64_t)first * c->nx, n, MST_NONE);
    ANN_CHECK_HIP(c, hipGetLastError());
    return ANNCHOR_OK;
}

// Both begins.  core null: the plain form, seeds from one partner per point.  Otherwise the reach form: core (HOST double [nx])
// goes to the device and the seeds are the valid entries of graph (HOST int64 [nx][cols]; cols = 0: none).
static int mst_begin(annchor_ctx *c, double rtol, int32_t use_bounds, const int64_t *partner, const double *core, const int64_t *graph,
                     int64_t cols, int64_t *n_seeds)
{
    const int64_t nx = c->nx;
    ANN_REQUIRE(c, nx >= 1, ANNCHOR_EINVAL, "no data set bound");
    ANN_REQUIRE(c, nx < (1ll << 31), ANNCHOR_ELIMIT, "%lld points: indices are packed as 32-bit halves", (long long)nx);
    ANN_REQUIRE(c, rtol >= 0.0 && rtol < 1.0, ANNCHOR_EINVAL, "rtol must be in [0, 1)");
    ANN_REQUIRE(c, !use_bounds || (c->na >= 1 && c->Dt.p), ANNCHOR_EINVAL, "use_bounds needs an anchor table (pick anchors first)");
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    ANN_TRY(ann_side_join(c));
    c->mst_begun = false;
    rad_buffers_taken(c);
    const int64_t nchunks = (nx + RAD_COLS - 1) / RAD_COLS, rblocks = (nx + RAD_ROWS - 1) / RAD_ROWS;
    ANN_REQUIRE(c, rblocks * nchunks < (1ll << 31), ANNCHOR_ELIMIT, "%lld points exceed the classify grid", (long long)nx);
    // a seed partner that is no other point of the set is dropped; of a mutual pair the smaller index keeps it
    if (core) {
        ANN_REQUIRE(c, cols >= 0 && (graph || cols == 0), ANNCHOR_EINVAL, "a seed graph of %lld columns needs its entries", (long long)cols);
        ANN_REQUIRE(c, cols == 0 || nx * cols < (1ll << 30), ANNCHOR_ELIMIT, "%lld seed entries: pass fewer columns", (long long)(nx * cols));
        for (int64_t i = 0; i < nx; ++i)
            ANN_REQUIRE(c, core[i] >= 0.0, ANNCHOR_EINVAL, "core distance %lld is %g: core distances are numbers >= 0", (long long)i, core[i]);
    }
    std::vector<int2> seeds;
    if (partner)
        for (int64_t i = 0; i < nx; ++i) {
            const int64_t g = partner[i];
            if (g < 0 || g >= nx || g == i || (g < i && partner[g] == i)) continue;
            seeds.push_back(make_int2((int)(i < g ? i : g), (int)(i < g ? g : i)));
        }
    ANN_TRY(rad_reserve(c, c->mst_comp, sizeof(int32_t) * 3 * (size_t)nx));
    ANN_TRY(rad_reserve(c, c->mst_rank, sizeof(int64_t) * (size_t)(nx + 1) + sizeof(int32_t) * (size_t)nx));
    ANN_TRY(rad_reserve(c, c->mst_u, sizeof(double) * (size_t)nx));
    ANN_TRY(rad_reserve(c, c->mst_key, sizeof(uint64_t) * 4 * (size_t)nx));
    ANN_TRY(rad_reserve(c, c->mst_guide, 12 * (size_t)nx));
    ANN_TRY(rad_reserve(c, c->mst_tree, sizeof(MstEdge) * (size_t)nx));
    ANN_TRY(rad_reserve(c, c->mst_row, sizeof(unsigned long long) * (size_t)nx));
    ANN_TRY(rad_reserve(c, c->mst_stat, sizeof(uint64_t) * 4));
    ANN_TRY(rad_reserve(c, c->scan_tmp, sizeof(int64_t) * (size_t)(nx / 1024 + 2)));   // (the scan's block sums: found here, not carved from the slab)
    if (!seeds.empty()) {
        ANN_TRY(rad_reserve(c, c->mst_seed, sizeof(int2) * seeds.size()));
        ANN_TRY(ann_h2d(c, c->mst_seed.p, seeds.data(), sizeof(int2) * seeds.size()));
    }
    if (core) {
        ANN_TRY(rad_reserve(c, c->mst_core, sizeof(double) * (size_t)nx));
        ANN_TRY(ann_h2d(c, c->mst_core.p, core, sizeof(double) * (size_t)nx));
    }
    if (core && cols > 0) {   // (the graph waits in the walk's offset buffer, which no walk has filled yet)
        ANN_TRY(rad_reserve(c, c->rad_off, sizeof(int64_t) * (size_t)(nx * cols)));
        ANN_TRY(rad_reserve(c, c->mst_seed, sizeof(int2) * (size_t)(nx * cols)));
        ANN_TRY(ann_h2d(c, c->rad_off.p, graph, sizeof(int64_t) * (size_t)(nx * cols)));
    }
    ANN_CHECK_HIP(c, hipMemsetAsync(c->mst_stat.p, 0, sizeof(uint64_t) * 4, c->stream));
    int32_t *comp = c->mst_comp.as<int32_t>();
    k_mst_init<<<ann_blocks(nx, MST_THREADS), MST_THREADS, 0, c->stream>>>(nx, comp, comp + nx, comp + 2 * nx);
    ANN_CHECK_HIP(c, hipGetLastError());
    c->mst_nx = nx; c->mst_rtol = rtol; c->mst_use_bounds = use_bounds ? 1 : 0;
    c->mst_reach = core ? 1 : 0;
    c->mst_n_pool = c->mst_n_list = c->mst_n_tree = 0;
    c->mst_n_seed = (int64_t)seeds.size();
    if (core && cols > 0) {
        unsigned long long *tail = c->mst_stat.as<unsigned long long>() + 3;
        k_mst_seed<<<ann_blocks(nx * cols, MST_THREADS), MST_THREADS, 0, c->stream>>>(c->rad_off.as<int64_t>(), nx, cols, c->mst_seed.as<int2>(), tail);
        ANN_CHECK_HIP(c, hipGetLastError());
        ANN_TRY(ann_d2h(c, &c->mst_n_seed, tail, sizeof(int64_t)));
        ANN_REQUIRE(c, c->mst_n_seed >= 0 && c->mst_n_seed <= nx * cols, ANNCHOR_ESTATE, "the seed pass left %lld pairs from %lld entries",
                    (long long)c->mst_n_seed, (long long)(nx * cols));
    }
    c->mst_round = 0; c->mst_phase = 0; c->mst_pending = false;
    ANN_TRY(mst_number(c));
    ANN_REQUIRE(c, c->mst_n_comp == nx, ANNCHOR_ESTATE, "%lld components of %lld single points", (long long)c->mst_n_comp, (long long)nx);
    if (n_seeds) *n_seeds = c->mst_n_seed;
    c->mst_begun = true;
    return ANNCHOR_OK;
}

extern "C" int annchor_mst_begin(annchor_ctx *c, double rtol, int32_t use_bounds, const int64_t *partner, int64_t *n_seeds)
{
    if (!c) return ANNCHOR_EINVAL;
    return mst_begin(c, rtol, use_bounds, partner, nullptr, nullptr, 0, n_seeds);
}

extern "C" int annchor_mst_begin_reach(annchor_ctx *c, double rtol, int32_t use_bounds, const double *core, const int64_t *seed_idx,
                                       int64_t seed_cols, int64_t *n_seeds)
{
    if (!c || !core) return ANNCHOR_EINVAL;
    return mst_begin(c, rtol, use_bounds, nullptr, core, seed_idx, seed_cols, n_seeds);
}

extern "C" int annchor_mst_round_begin(annchor_ctx *c, int32_t evaluate, int64_t *n_bridges)
{
    if (!c || !n_bridges) return ANNCHOR_EINVAL;
    *n_bridges = 0;
    MST_REQUIRE_BEGUN(c);
    ANN_REQUIRE(c, c->mst_phase == 0, ANNCHOR_EINVAL, "a round is open: finish it with annchor_mst_round_end");
    ANN_REQUIRE(c, c->mst_n_comp >= 2, ANNCHOR_EINVAL, "one component is left: the tree is complete");
    ANN_REQUIRE(c, !evaluate || c->metric != ANNCHOR_METRIC_NONE, ANNCHOR_EINVAL,
                "no device metric bound to this context: pass evaluate = 0, fetch the pairs and hand their distances to annchor_mst_edges");
    const int na = mst_na(c), nA = c->nA < na ? c->nA : na;   // (anchor a of the table is point A[a] for a < nA)
    ANN_REQUIRE(c, !c->mst_use_bounds || (na >= 1 && c->Dt.p), ANNCHOR_EINVAL, "the anchor table is gone: pick anchors and call annchor_mst_begin again");
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    ANN_TRY(ann_side_join(c));
    rad_buffers_taken(c);
    const int64_t nx = c->nx, ncomp = c->mst_n_comp, nseed = c->mst_round == 0 ? c->mst_n_seed : 0, n = ncomp + nseed;
    const int32_t *comp = c->mst_comp.as<int32_t>();
    uint64_t *bkey = c->mst_key.as<uint64_t>(), *bpair = bkey + nx;
    uint64_t *gkey = c->mst_guide.as<uint64_t>();
    int32_t *ganc = reinterpret_cast<int32_t *>(gkey + nx);
    const int32_t *roots = reinterpret_cast<const int32_t *>(c->mst_rank.as<int64_t>() + nx + 1);
    ANN_TRY(rad_reserve(c, c->rad_eval, sizeof(int2) * (size_t)n));
    {
        ProfScope ps(c, "mst_bridge", (double)nA * (double)nx * 8.0 + (double)nx * 60.0);
        ANN_TRY(mst_clear_keys(c, 0, 2));
        const int vb = ann_blocks(nx, MST_THREADS);
        if (nA > 0) {
            k_mst_guide<<<vb, MST_THREADS, 0, c->stream>>>(c->Dt.as<double>(), c->A.as<int32_t>(), nA, nx, comp, gkey, ganc, bkey);
            k_mst_bridge_pick<<<vb, MST_THREADS, 0, c->stream>>>(nx, comp, gkey, ganc, bkey, bpair);
        }
        k_mst_bridge_emit<<<ann_blocks(ncomp, MST_THREADS), MST_THREADS, 0, c->stream>>>(roots, ncomp, bpair, c->A.as<int32_t>(), c->rad_eval.as<int2>());
    }
    ANN_CHECK_HIP(c, hipGetLastError());
    if (nseed > 0)
        ANN_CHECK_HIP(c, hipMemcpyAsync(c->rad_eval.as<int2>() + ncomp, c->mst_seed.p, sizeof(int2) * (size_t)nseed, hipMemcpyDeviceToDevice, c->stream));
    c->mst_n_list = n;
    c->mst_phase = 1;
    c->mst_pending = true;
    *n_bridges = n;
    if (!evaluate) return ANNCHOR_OK;
    ANN_TRY(mst_evaluate(c, n));
    int64_t added = 0;
    ANN_TRY(mst_absorb(c, n, true, &added));
    c->mst_phase = 2;
    c->mst_pending = false;
    return ANNCHOR_OK;
}

extern "C" int annchor_mst_fetch(annchor_ctx *c, int64_t *ij)
{
    if (!c) return ANNCHOR_EINVAL;
    MST_REQUIRE_BEGUN(c);
    ANN_REQUIRE(c, c->mst_pending, ANNCHOR_EINVAL, "no emitted list waits for its distances");
    if (c->mst_n_list == 0) return ANNCHOR_OK;
    if (!ij) return ANNCHOR_EINVAL;
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    return rad_pairs_out(c, c->rad_eval.p, c->mst_n_list, ij);
}

extern "C" int annchor_mst_edges(annchor_ctx *c, const int64_t *ij, const double *d, int64_t n)
{
    if (!c || n < 0 || (n > 0 && (!ij || !d))) return ANNCHOR_EINVAL;
    MST_REQUIRE_BEGUN(c);
    ANN_REQUIRE(c, c->mst_phase == 1 || c->mst_phase == 3, ANNCHOR_EINVAL,
                "annchor_mst_edges takes a round's bridges (after annchor_mst_round_begin) or a range's candidates (after annchor_mst_rows)");
    ANN_REQUIRE(c, n < (1ll << 30), ANNCHOR_ELIMIT, "%lld pairs in one call: pass them in parts", (long long)n);
    const bool bridge = c->mst_phase == 1;
    std::vector<int2> tmp;
    ANN_TRY(rad_pairs_in(c, ij, n, c->nx, bridge ? "bridge" : "candidate", tmp));
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    ANN_TRY(ann_side_join(c));
    // (the walk's own list buffers: the host has fetched what they held)
    c->mst_pending = false;
    c->mst_n_list = 0;
    if (bridge) c->mst_phase = 2;
    if (n == 0) return ANNCHOR_OK;
    ANN_TRY(rad_reserve(c, c->rad_eval, sizeof(int2) * (size_t)n));
    ANN_TRY(rad_reserve(c, c->rad_d, sizeof(double) * (size_t)n));
    ANN_TRY(ann_h2d(c, c->rad_eval.p, tmp.data(), sizeof(int2) * (size_t)n));
    ANN_TRY(ann_h2d(c, c->rad_d.p, d, sizeof(double) * (size_t)n));
    int64_t added = 0;
    return mst_absorb(c, n, bridge, &added);
}

template <bool TABLE>
static void mst_launch_classify(annchor_ctx *c, int na, int64_t rb, int64_t re, int64_t cb, int64_t ce, int64_t nchunks, uint64_t *me, int32_t *cn,
                                unsigned long long *row)
{
    const unsigned grid = (unsigned)(((re - rb + RAD_ROWS - 1) / RAD_ROWS) * nchunks);
    const double *Dt = na > 0 ? c->Dt.as<double>() : nullptr;
    if (c->mst_reach)
        k_mst_classify_reach<TABLE><<<grid, RAD_ROWS, 0, c->stream>>>(Dt, c->mst_u.as<double>(), c->mst_comp.as<int32_t>(), c->mst_core.as<double>(),
                                                                      c->nx, na, c->mst_rtol, rb, re, cb, ce, nchunks, me, cn, row);
    else
        k_mst_classify<TABLE><<<grid, RAD_ROWS, 0, c->stream>>>(Dt, c->mst_u.as<double>(), c->mst_comp.as<int32_t>(), c->nx, na, c->mst_rtol, rb, re,
                                                                cb, ce, nchunks, me, cn, row);
}

extern "C" int annchor_mst_round_bounds(annchor_ctx *c, int64_t *row_eval)
{
    if (!c || !row_eval) return ANNCHOR_EINVAL;
    MST_REQUIRE_BEGUN(c);
    ANN_REQUIRE(c, c->mst_phase == 2, ANNCHOR_EINVAL, "%s",
                c->mst_phase == 1 ? "the round's bridges were emitted and never absorbed: evaluate them and pass them to annchor_mst_edges"
                                  : "annchor_mst_round_bounds follows annchor_mst_round_begin");
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    const int64_t nx = c->nx, np = c->mst_n_pool;
    const int na = mst_na(c);
    const int32_t *comp = c->mst_comp.as<int32_t>();
    uint64_t *mkey = c->mst_key.as<uint64_t>() + 2 * nx;
    unsigned long long *row = c->mst_row.as<unsigned long long>();
    {
        ProfScope ps(c, "mst_bounds", (double)np * 24.0 + (double)nx * 20.0);
        ANN_TRY(mst_clear_keys(c, 2, 1));
        if (np > 0) k_mst_cross_min<<<ann_blocks(np, MST_THREADS), MST_THREADS, 0, c->stream>>>(c->mst_pool.as<MstEdge>(), np, comp, mkey);
        k_mst_radii<<<ann_blocks(nx, MST_THREADS), MST_THREADS, 0, c->stream>>>(nx, comp, mkey, c->mst_u.as<double>());
    }
    ANN_CHECK_HIP(c, hipMemsetAsync(row, 0, sizeof(unsigned long long) * (size_t)nx, c->stream));
    const int64_t nchunks = (nx + RAD_COLS - 1) / RAD_COLS, rblocks = (nx + RAD_ROWS - 1) / RAD_ROWS;
    {
        ProfScope ps(c, "mst_classify", (double)na * (double)nx * 8.0 * (double)(rblocks + nchunks));
        mst_launch_classify<false>(c, na, 0, nx, 0, nx, nchunks, nullptr, nullptr, row);
    }
    ANN_CHECK_HIP(c, hipGetLastError());
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "row totals are downloaded as int64");
    ANN_TRY(ann_d2h(c, row_eval, row, sizeof(int64_t) * (size_t)nx));
    c->mst_phase = 3;
    return ANNCHOR_OK;
}

extern "C" int annchor_mst_rows(annchor_ctx *c, int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end, int64_t max_pairs,
                                int32_t evaluate, int64_t *n_eval, int64_t *n_added)
{
    if (!c || !n_eval || !n_added) return ANNCHOR_EINVAL;
    *n_eval = *n_added = 0;
    MST_REQUIRE_BEGUN(c);
    ANN_REQUIRE(c, c->mst_phase == 3, ANNCHOR_EINVAL, "annchor_mst_round_bounds has not fixed this round's radii");
    ANN_REQUIRE(c, !c->mst_pending, ANNCHOR_EINVAL,
                "the last range's %lld candidates were emitted and never absorbed: evaluate them and pass them to annchor_mst_edges",
                (long long)c->mst_n_list);
    const int64_t nx = c->nx;
    ANN_TRY(rad_range_check(c, nx, nx, row_begin, row_end, col_begin, col_end));
    ANN_REQUIRE(c, !evaluate || c->metric != ANNCHOR_METRIC_NONE, ANNCHOR_EINVAL,
                "no device metric bound to this context: pass evaluate = 0, fetch the candidates and hand their distances to annchor_mst_edges");
    const int na = mst_na(c);
    ANN_REQUIRE(c, !c->mst_use_bounds || (na >= 1 && c->Dt.p), ANNCHOR_EINVAL, "the anchor table is gone: pick anchors and call annchor_mst_begin again");
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    ANN_TRY(ann_side_join(c));
    rad_buffers_taken(c);
    c->mst_n_list = 0;
    if (col_begin == col_end) return ANNCHOR_OK;
    int64_t tot = 0;
    bool emitted = true;
    ANN_TRY(rad_range_candidates(c, "mst_classify", "mst_emit", na, row_begin, row_end, col_begin, col_end, max_pairs,
                                 [&](int64_t rb, int64_t re, int64_t cb, int64_t ce, int64_t nchunks, uint64_t *me, int32_t *cn) {
                                     mst_launch_classify<true>(c, na, rb, re, cb, ce, nchunks, me, cn, nullptr);
                                 }, &tot, &emitted));
    *n_eval = tot;
    if (!emitted) {
        *n_added = -1;
        return ANNCHOR_OK;
    }
    if (tot == 0) return ANNCHOR_OK;
    c->mst_n_list = tot;
    if (!evaluate) {
        c->mst_pending = true;
        return ANNCHOR_OK;
    }
    ANN_TRY(mst_evaluate(c, tot));
    return mst_absorb(c, tot, false, n_added);
}

extern "C" int annchor_mst_round_end(annchor_ctx *c, int64_t *n_components, int64_t *n_tree, int64_t *n_pool)
{
    if (!c || !n_components || !n_tree || !n_pool) return ANNCHOR_EINVAL;
    MST_REQUIRE_BEGUN(c);
    ANN_REQUIRE(c, c->mst_phase == 3, ANNCHOR_EINVAL, "no round is open behind annchor_mst_round_bounds");
    ANN_REQUIRE(c, !c->mst_pending, ANNCHOR_EINVAL,
                "the last range's %lld candidates were emitted and never absorbed: evaluate them and pass them to annchor_mst_edges",
                (long long)c->mst_n_list);
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    ANN_TRY(ann_side_join(c));
    const int64_t nx = c->nx, np = c->mst_n_pool, ncomp = c->mst_n_comp;
    int32_t *comp = c->mst_comp.as<int32_t>(), *parent = comp + nx, *flag = comp + 2 * nx;
    uint64_t *mkey = c->mst_key.as<uint64_t>() + 2 * nx, *medge = mkey + nx;
    const int32_t *roots = reinterpret_cast<const int32_t *>(c->mst_rank.as<int64_t>() + nx + 1);
    const MstEdge *pool = c->mst_pool.as<MstEdge>();
    unsigned long long *stat = c->mst_stat.as<unsigned long long>();
    {
        ProfScope ps(c, "mst_pick", (double)np * 48.0 + (double)nx * 16.0);
        ANN_TRY(mst_clear_keys(c, 2, 2));
        if (np > 0) {
            k_mst_cross_min<<<ann_blocks(np, MST_THREADS), MST_THREADS, 0, c->stream>>>(pool, np, comp, mkey);
            k_mst_cross_edge<<<ann_blocks(np, MST_THREADS), MST_THREADS, 0, c->stream>>>(pool, np, comp, mkey, medge);
        }
    }
    {
        ProfScope ps(c, "mst_take", (double)ncomp * 40.0 + (double)nx * 12.0);
        k_mst_take<<<ann_blocks(ncomp, MST_THREADS), MST_THREADS, 0, c->stream>>>(roots, ncomp, comp, mkey, medge, parent, c->mst_tree.as<MstEdge>(),
                                                                                 nx - 1, stat);
        k_mst_flatten<<<ann_blocks(nx, MST_THREADS), MST_THREADS, 0, c->stream>>>(nx, parent, comp, flag);
    }
    ANN_CHECK_HIP(c, hipGetLastError());
    ANN_TRY(mst_number(c));
    int64_t hstat[3] = {0, 0, 0};
    ANN_TRY(ann_d2h(c, hstat, stat, sizeof hstat));
    c->mst_n_tree = hstat[1];
    c->mst_round += 1;
    c->mst_phase = 0;
    *n_components = c->mst_n_comp;
    *n_tree = c->mst_n_tree;
    *n_pool = np;
    ANN_REQUIRE(c, hstat[2] == 0, ANNCHOR_ESTATE,
                "round %d left %lld of %lld components without an outgoing edge: a bridge's distance was NaN, or a range of the walk was "
                "never absorbed", c->mst_round - 1, (long long)hstat[2], (long long)ncomp);
    ANN_REQUIRE(c, c->mst_n_comp < ncomp && c->mst_n_comp + c->mst_n_tree == nx, ANNCHOR_ESTATE,
                "round %d: %lld components and %lld tree edges over %lld points", c->mst_round - 1, (long long)c->mst_n_comp,
                (long long)c->mst_n_tree, (long long)nx);
    return ANNCHOR_OK;
}

static inline uint64_t mst_host_key(double v)
{
    uint64_t u;
    memcpy(&u, &v, sizeof u);
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}

extern "C" int annchor_mst_finish(annchor_ctx *c, int64_t *edges, double *dist)
{
    if (!c) return ANNCHOR_EINVAL;
    MST_REQUIRE_BEGUN(c);
    ANN_REQUIRE(c, c->mst_phase == 0, ANNCHOR_EINVAL, "a round is open: finish it with annchor_mst_round_end");
    const int64_t nx = c->nx, n = nx - 1;
    ANN_REQUIRE(c, c->mst_n_comp == 1 && c->mst_n_tree == n, ANNCHOR_ESTATE, "%lld components and %lld tree edges over %lld points: the rounds have not ended",
                (long long)c->mst_n_comp, (long long)c->mst_n_tree, (long long)nx);
    if (n == 0) return ANNCHOR_OK;
    if (!edges || !dist) return ANNCHOR_EINVAL;
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    std::vector<MstEdge> t((size_t)n);
    ANN_TRY(ann_d2h(c, t.data(), c->mst_tree.p, sizeof(MstEdge) * (size_t)n));
    // (nx - 1 edges on the host: the order of arrival is replaced by the total order)
    std::sort(t.begin(), t.end(), [](const MstEdge &a, const MstEdge &b) {
        const uint64_t ka = mst_host_key(a.d), kb = mst_host_key(b.d);
        return ka != kb ? ka < kb : a.i != b.i ? a.i < b.i : a.j < b.j;
    });
    for (int64_t e = 0; e < n; ++e) {
        edges[2 * e] = t[(size_t)e].i;
        edges[2 * e + 1] = t[(size_t)e].j;
        dist[e] = t[(size_t)e].d;
    }
    return ANNCHOR_OK;
}
