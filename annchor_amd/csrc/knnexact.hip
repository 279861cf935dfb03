// knnexact.hip -- the exact k-NN graph from the anchor table and one radius per row (no reference counterpart).
// u[i] is an upper bound of row i's true k-th neighbour distance (a fitted graph supplies it: the largest exact distance among
// the k points it lists).  A pair (i, j) matters to neither row once an anchor proves d(i, j) > max(u[i], u[j]); every other
// pair is evaluated, and each row takes its k smallest.  The stages:
//   classify   the row classifier of radius.h with R = max(u[i], u[j]) in place of r: the same (row, 64-column chunk)
//              table, the same two forms (per-row totals for the plan, masks and counts for a range), no SURE class
//   emit       the radius stages' scan and k_rad_emit: the EVAL list in row-major order, ascending column inside a row
//   evaluate   ann_metric_launch on the device-resident list (or the host, for a Python callable: fetch, then edges)
//   absorb     one pass: (i -> j, d) if d <= u[i], (j -> i, d) if d <= u[j]; entries are appended to a device list, counted per row
//   finish     scan of the per-row counts, scatter by row through per-row cursors, one workgroup per row selects the k smallest
//              of its entries plus the diagonal (0.0, i) by (ann_key_asc(d), index) and writes them in that order
// The rule (include/annchor_hip.h states it; tests/exact_knn_cases.py restates it in NumPy):
//   s = Dt[a][i], t = Dt[a][j], R = max(u[i], u[j]);   out(a): (fabs(s - t) - R) > rtol * ((s + t) + R)
// The result is a pure function of the entry SET: every unordered pair is classified in exactly one range of a walk, so no entry
// repeats; the per-row counts are integer sums; the order of the entry list and of a row's segment (both decided by atomics)
// is never read -- the selection takes order statistics of (key, column), a total order on a row's entries since its columns
// are distinct.
#include "common.h"
#include "radius.h"
#include "rowsel.h"

#define KX_THREADS 256
#define KX_MIN_ENTRIES (1ll << 12)          // first reservation of the entry list (64 KiB; doubled from there)
#define KX_MAX_ENTRIES ((1ll << 31) - 1)    // the per-entry grids stay below 2^23 workgroups

struct __attribute__((aligned(16))) KxEntry {
    int32_t row, col;
    double d;
};

// The row classifier of radius.h with one radius per row, R = max(u[i], u[j]) per pair, and no SURE class.  R = +inf leaves
// the pair EVAL (rad_rule).
template <bool TABLE>
__global__ __launch_bounds__(RAD_ROWS) void k_kx_classify(const double *__restrict__ Dt, const double *__restrict__ u, int64_t nx, int na,
                                                         double rtol, int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end,
                                                         int64_t nchunks, uint64_t *__restrict__ mask_eval, int32_t *__restrict__ cnt_eval,
                                                         unsigned long long *__restrict__ row_eval)
{
    __shared__ double shu[RAD_COLS];
    rad_classify_rows<false, TABLE>(RadPerRow{u, shu, 0.0}, Dt, nx, na, rtol, row_begin, row_end, col_begin, col_end, nchunks, mask_eval, nullptr,
                                    cnt_eval, nullptr, row_eval, nullptr);
}

// One pass over a range's candidates and distances: the directed tests d <= u[i] and d <= u[j] (a NaN passes neither), the
// surviving entries appended behind *tail -- one agent-scope add per wave reserves the wave's places, the i -> j entries first --
// and counted per row.  The lists are row-major, so the lanes of a wave mostly share i: a run of equal i inside the wave is one
// add of its surviving entries by the run's first lane; j differs from lane to lane.  Every word is its own: no two counters
// share an add, and nothing reads them before the launch ends.
__global__ __launch_bounds__(KX_THREADS) void k_kx_absorb(const int2 *__restrict__ ij, const double *__restrict__ d, int64_t n,
                                                         const double *__restrict__ u, KxEntry *__restrict__ ent, int64_t cap,
                                                         unsigned long long *tail, int32_t *cnt)
{
    const int64_t t = (int64_t)blockIdx.x * KX_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool ok = t < n;
    const int2 e = ij[ok ? t : n - 1];
    const double v = d[ok ? t : n - 1];
    const bool a = ok && v <= u[e.x], b = ok && v <= u[e.y];
    const uint64_t ma = __ballot(a), mb = __ballot(b);
    int end;
    if (ann_wave_run(e.x, ok, lane, end)) {
        const uint64_t run = (end == 64 ? ~0ull : ((1ull << end) - 1ull)) & ~((1ull << lane) - 1ull);
        const int r = __popcll(ma & run);
        if (r) atomicAdd(cnt + e.x, r);
    }
    if (b) atomicAdd(cnt + e.y, 1);
    const int ca = __popcll(ma), cb = __popcll(mb);
    if (ca + cb == 0) return;   // (uniform)
    unsigned long long base = 0ull;
    if (lane == 0) base = atomicAdd(tail, (unsigned long long)(ca + cb));
    base = __shfl(base, 0);
    const uint64_t below = (1ull << lane) - 1ull;
    if (a) {
        const int64_t p = (int64_t)base + __popcll(ma & below);
        if (p < cap) { KxEntry o; o.row = e.x; o.col = e.y; o.d = v; ent[p] = o; }   // (p < cap always: the list has room for two entries per candidate)
    }
    if (b) {
        const int64_t p = (int64_t)base + ca + __popcll(mb & below);
        if (p < cap) { KxEntry o; o.row = e.y; o.col = e.x; o.d = v; ent[p] = o; }
    }
}

// stat[0] = the longest row's entry count, stat[1] = the rows with fewer than `need` entries (one add of each per wave)
__global__ __launch_bounds__(KX_THREADS) void k_kx_rowstat(const int32_t *__restrict__ cnt, int64_t nx, int32_t need, uint32_t *stat)
{
    const int64_t v = (int64_t)blockIdx.x * KX_THREADS + threadIdx.x;
    const int c = v < nx ? cnt[v] : 0;
    const uint64_t few = __ballot(v < nx && c < need);
    int mx = c;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) mx = max(mx, __shfl_xor(mx, s));
    if ((threadIdx.x & 63) == 0) {
        if (mx > 0) atomicMax(stat, (uint32_t)mx);
        if (few) atomicAdd(stat + 1, (uint32_t)__popcll(few));
    }
}

// by row: entry t goes to off[row] + (the row's cursor, taken by an agent-scope add on the row's own word).  The order inside a
// row's segment is the order of arrival; k_kx_rows never reads it.
__global__ __launch_bounds__(KX_THREADS) void k_kx_scatter(const KxEntry *__restrict__ ent, int64_t n, const int64_t *__restrict__ off,
                                                          int32_t *cur, uint64_t *__restrict__ skey, int32_t *__restrict__ scol)
{
    const int64_t t = (int64_t)blockIdx.x * KX_THREADS + threadIdx.x;
    if (t >= n) return;
    const KxEntry e = ent[t];
    const int64_t p = off[e.row] + atomicAdd(cur + e.row, 1);
    if (p < n) { skey[p] = ann_key_asc(e.d); scol[p] = e.col; }   // (p < off[row + 1] always: the counts are of these entries)
}

// One workgroup per row: the k smallest of the row's entries and the diagonal (0.0, i) by (key, column), written in that order
// -- k_bf_rows' selection (rowsel.h) on a row whose slots are in no particular order.  The k-th key t comes from the radix
// descent; everything below t is taken; among the entries AT t the smallest columns are, and which those are is a second
// descent over the columns of the tied entries (the others read as the largest key).  Keys and columns sit in LDS when the row
// fits `cap` slots and are read from memory on every pass when not.
__global__ __launch_bounds__(ROW_THREADS) void k_kx_rows(const uint64_t *__restrict__ skey, const int32_t *__restrict__ scol,
                                                        const int64_t *__restrict__ off, int k, int64_t *__restrict__ oidx,
                                                        double *__restrict__ odist, int cap)
{
    __shared__ RowSelShared sh;
    __shared__ uint32_t cnt_sel;
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    uint64_t *keys = reinterpret_cast<uint64_t *>(dyn);      // [cap]
    uint64_t *lkey = keys + cap;                             // [k]
    int32_t *cols = reinterpret_cast<int32_t *>(lkey + k);   // [cap]
    int32_t *lcol = cols + cap;                              // [k]
    const int64_t i = blockIdx.x;
    const int64_t b = off[i];
    const int m = (int)(off[i + 1] - b);
    const int len = m + 1;                                   // slot m: the diagonal
    const bool in_lds = len <= cap;
    const uint64_t kdiag = ann_key_asc(0.0);
    auto key_g = [&](int s) -> uint64_t { return skey[b + (s < m ? s : 0)]; };
    auto col_g = [&](int s) -> int32_t { return scol[b + (s < m ? s : 0)]; };
    if (threadIdx.x == 0) cnt_sel = 0;
    if (in_lds)
        for (int s = threadIdx.x; s < len; s += ROW_THREADS) {
            keys[s] = s < m ? key_g(s) : kdiag;
            cols[s] = s < m ? col_g(s) : (int32_t)i;
        }
    __syncthreads();
    auto kf = [&](int s) -> uint64_t { return in_lds ? keys[s] : (s < m ? key_g(s) : kdiag); };
    auto cf = [&](int s) -> int32_t { return in_lds ? cols[s] : (s < m ? col_g(s) : (int32_t)i); };
    const int want = min(k, len);
    const uint64_t t = row_kth_key(sh, len, (uint32_t)(want - 1), kf);
    for (int s = threadIdx.x; s < len; s += ROW_THREADS) {
        const uint64_t kk = kf(s);
        if (kk < t) { const uint32_t o = atomicAdd(&cnt_sel, 1u); lkey[o] = kk; lcol[o] = cf(s); }   // (fewer than want keys lie below the want-th)
    }
    __syncthreads();
    const uint32_t nlt = cnt_sel;
    auto tf = [&](int s) -> uint64_t { return kf(s) == t ? (uint64_t)(uint32_t)cf(s) : ~0ull; };
    const uint64_t cstar = row_kth_key(sh, len, (uint32_t)want - nlt - 1u, tf);   // (at least want - nlt entries sit at t; every thread has read nlt behind the descent's first barrier)
    for (int s = threadIdx.x; s < len; s += ROW_THREADS)
        if (kf(s) == t) {
            const int32_t cs = cf(s);
            if ((uint64_t)(uint32_t)cs <= cstar) {
                const uint32_t o = atomicAdd(&cnt_sel, 1u);
                if (o < (uint32_t)want) { lkey[o] = t; lcol[o] = cs; }   // (always: a row's columns are distinct)
            }
        }
    __syncthreads();
    for (int e = threadIdx.x; e < want; e += ROW_THREADS) {
        const uint64_t ke = lkey[e];
        const int32_t ce = lcol[e];
        int r = 0;
        for (int o = 0; o < want; ++o) r += (lkey[o] < ke) || (lkey[o] == ke && lcol[o] < ce);
        oidx[i * k + r] = ce;
        odist[i * k + r] = ann_key_asc_inv(ke);
    }
}

// Room for `more` entries behind the kx_n_entries the list holds.
static int kx_room(annchor_ctx *c, int64_t more)
{
    return rad_grow(c, c->kx_ent, sizeof(KxEntry), c->kx_n_entries, more, KX_MIN_ENTRIES, KX_MAX_ENTRIES, "exact k-NN entry", "entries",
                    ": pass a smaller max_pairs, or better radii", __func__);
}

static bool kx_ready(const annchor_ctx *c) { return c->kx_begun && c->kx_nx == c->nx && c->kx_u.p && c->kx_cnt.p; }

template <bool TABLE>
static void kx_launch_classify(annchor_ctx *c, int na, int64_t rb, int64_t re, int64_t cb, int64_t ce, int64_t nchunks, uint64_t *me, int32_t *cn,
                               unsigned long long *row)
{
    const unsigned grid = (unsigned)(((re - rb + RAD_ROWS - 1) / RAD_ROWS) * nchunks);
    k_kx_classify<TABLE><<<grid, RAD_ROWS, 0, c->stream>>>(na > 0 ? c->Dt.as<double>() : nullptr, c->kx_u.as<double>(), c->nx, na, c->kx_rtol, rb, re,
                                                           cb, ce, nchunks, me, cn, row);
}

// The walk writes the radius stages' table, scans and lists: what annchor_radius_count fixed no longer describes them.
static void kx_take_radius_buffers(annchor_ctx *c)
{
    c->rad_params = false;
    c->rad_evaluated = false;
    c->rad_n_eval = c->rad_n_sure = c->rad_n_kept = 0;
}

extern "C" int annchor_knn_exact_begin(annchor_ctx *c, int32_t k, const double *u, double rtol, int32_t use_bounds, int64_t *row_eval)
{
    if (!c || !u || !row_eval) return ANNCHOR_EINVAL;
    const int64_t nx = c->nx;
    ANN_REQUIRE(c, nx >= 1, ANNCHOR_EINVAL, "no data set bound");
    ANN_REQUIRE(c, k >= 1 && k <= nx, ANNCHOR_EINVAL, "k=%d out of range 1..%lld (k counts the point itself)", k, (long long)nx);
    ANN_REQUIRE(c, (size_t)k * 12 <= 100 * 1024, ANNCHOR_ELIMIT, "k=%d: at most 8533 columns per row", k);
    ANN_REQUIRE(c, rtol >= 0.0 && rtol < 1.0, ANNCHOR_EINVAL, "rtol must be in [0, 1)");
    ANN_REQUIRE(c, !use_bounds || (c->na >= 1 && c->Dt.p), ANNCHOR_EINVAL, "use_bounds needs an anchor table (pick anchors first)");
    for (int64_t i = 0; i < nx; ++i)
        ANN_REQUIRE(c, u[i] >= 0.0, ANNCHOR_EINVAL, "u[%lld] must be a number >= 0: pass +inf for a row whose radius is unknown", (long long)i);   // (false for NaN)
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    ANN_TRY(ann_side_join(c));
    c->kx_begun = false;
    kx_take_radius_buffers(c);
    const int64_t nchunks = (nx + RAD_COLS - 1) / RAD_COLS, rblocks = (nx + RAD_ROWS - 1) / RAD_ROWS;
    ANN_REQUIRE(c, rblocks * nchunks < (1ll << 31), ANNCHOR_ELIMIT, "%lld points exceed the classify grid", (long long)nx);
    ANN_TRY(rad_reserve(c, c->kx_u, sizeof(double) * (size_t)nx));
    ANN_TRY(rad_reserve(c, c->kx_row, sizeof(unsigned long long) * (size_t)nx));
    ANN_TRY(rad_reserve(c, c->kx_cnt, sizeof(int32_t) * 2 * (size_t)nx));
    ANN_TRY(rad_reserve(c, c->kx_stat, sizeof(uint64_t) * 2));
    ANN_TRY(ann_h2d(c, c->kx_u.p, u, sizeof(double) * (size_t)nx));
    unsigned long long *row = c->kx_row.as<unsigned long long>();
    ANN_CHECK_HIP(c, hipMemsetAsync(row, 0, sizeof(unsigned long long) * (size_t)nx, c->stream));
    ANN_CHECK_HIP(c, hipMemsetAsync(c->kx_cnt.p, 0, sizeof(int32_t) * 2 * (size_t)nx, c->stream));
    ANN_CHECK_HIP(c, hipMemsetAsync(c->kx_stat.p, 0, sizeof(uint64_t) * 2, c->stream));
    c->kx_nx = nx; c->kx_k = k; c->kx_rtol = rtol; c->kx_use_bounds = use_bounds ? 1 : 0;
    c->kx_n_entries = c->kx_n_eval = 0;
    c->kx_pending = false;
    const int na = use_bounds ? c->na : 0;
    ANN_CHECK_HIP(c, hipEventRecord(c->call_a, c->stream));
    {
        ProfScope ps(c, "knn_exact_classify", (double)na * (double)nx * 8.0 * (double)(rblocks + nchunks));
        kx_launch_classify<false>(c, na, 0, nx, 0, nx, nchunks, nullptr, nullptr, row);
    }
    ANN_CHECK_HIP(c, hipEventRecord(c->call_b, c->stream));
    c->call_timed = true;
    ANN_CHECK_HIP(c, hipGetLastError());
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "row totals are downloaded as int64");
    ANN_TRY(ann_d2h(c, row_eval, row, sizeof(int64_t) * (size_t)nx));
    c->kx_begun = true;
    return ANNCHOR_OK;
}

// n candidates (device int2 pairs and their distances) through the directed tests into the entry list
static int kx_absorb(annchor_ctx *c, const int2 *ij, const double *d, int64_t n, int64_t *added)
{
    *added = 0;
    if (n == 0) return ANNCHOR_OK;
    ANN_TRY(kx_room(c, 2 * n));
    const int64_t cap = (int64_t)(c->kx_ent.cap / sizeof(KxEntry));
    unsigned long long *tail = c->kx_stat.as<unsigned long long>();
    {
        ProfScope ps(c, "knn_exact_absorb", (double)n * 32.0);
        k_kx_absorb<<<ann_blocks(n, KX_THREADS), KX_THREADS, 0, c->stream>>>(ij, d, n, c->kx_u.as<double>(), c->kx_ent.as<KxEntry>(), cap, tail,
                                                                            c->kx_cnt.as<int32_t>());
    }
    ANN_CHECK_HIP(c, hipGetLastError());
    int64_t total = 0;
    ANN_TRY(ann_d2h(c, &total, tail, sizeof(int64_t)));
    ANN_REQUIRE(c, total >= c->kx_n_entries && total - c->kx_n_entries <= 2 * n && total <= cap, ANNCHOR_ESTATE,
                "the absorb pass left %lld entries behind %lld from %lld candidates", (long long)total, (long long)c->kx_n_entries, (long long)n);
    *added = total - c->kx_n_entries;
    c->kx_n_entries = total;
    return ANNCHOR_OK;
}

extern "C" int annchor_knn_exact_rows(annchor_ctx *c, int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end, int64_t max_pairs,
                                      int32_t evaluate, int64_t *n_eval, int64_t *n_entries)
{
    if (!c || !n_eval || !n_entries) return ANNCHOR_EINVAL;
    *n_eval = *n_entries = 0;
    ANN_REQUIRE(c, kx_ready(c), ANNCHOR_EINVAL, "annchor_knn_exact_begin has not run on this data set");
    const int64_t nx = c->nx;
    ANN_TRY(rad_range_check(c, nx, nx, row_begin, row_end, col_begin, col_end));
    ANN_REQUIRE(c, !evaluate || c->metric != ANNCHOR_METRIC_NONE, ANNCHOR_EINVAL,
                "no device metric bound to this context: pass evaluate = 0, fetch the candidates and hand their distances to annchor_knn_exact_edges");
    const int na = c->kx_use_bounds ? c->na : 0;
    ANN_REQUIRE(c, !c->kx_use_bounds || (na >= 1 && c->Dt.p), ANNCHOR_EINVAL, "the anchor table is gone: pick anchors and call annchor_knn_exact_begin again");
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    ANN_TRY(ann_side_join(c));
    kx_take_radius_buffers(c);
    c->kx_n_eval = 0;
    c->kx_pending = false;
    if (col_begin == col_end) return ANNCHOR_OK;
    RadTable tb;
    ANN_TRY(rad_table(c, 0, row_begin, row_end, col_begin, col_end, tb));
    const int64_t rows = tb.rows, nchunks = tb.nchunks, entries = tb.entries;
    ANN_TRY(rad_reserve(c, c->rad_mask, sizeof(uint64_t) * (size_t)entries));
    ANN_TRY(rad_reserve(c, c->rad_cnt, sizeof(int32_t) * (size_t)entries));
    ANN_TRY(rad_reserve(c, c->rad_off, sizeof(int64_t) * (size_t)(entries + 1)));
    ANN_TRY(rad_reserve(c, c->scan_tmp, sizeof(int64_t) * (size_t)(entries / 1024 + 2)));   // (the scan's block sums: found here, not carved from the slab)
    uint64_t *me = c->rad_mask.as<uint64_t>();
    int32_t *cn = c->rad_cnt.as<int32_t>();
    int64_t *oe = c->rad_off.as<int64_t>();
    ANN_CHECK_HIP(c, hipEventRecord(c->call_a, c->stream));
    {
        ProfScope ps(c, "knn_exact_classify", (double)na * 8.0 * ((double)rows * (double)nchunks + (double)(col_end - col_begin) * (double)tb.rblocks));
        kx_launch_classify<true>(c, na, row_begin, row_end, col_begin, col_end, nchunks, me, cn, nullptr);
    }
    ANN_CHECK_HIP(c, hipGetLastError());
    ANN_TRY(ann_exclusive_scan_i32_to_i64(c, cn, oe, entries));
    int64_t tot = 0;
    ANN_TRY(ann_d2h(c, &tot, oe + entries, sizeof(int64_t)));
    *n_eval = tot;
    if (max_pairs > 0 && tot > max_pairs) {
        *n_entries = -1;
        return ANNCHOR_OK;
    }
    ANN_REQUIRE(c, tot < (1ll << 30), ANNCHOR_ELIMIT, "%lld candidate pairs in one range: pass max_pairs", (long long)tot);
    if (tot == 0) return ANNCHOR_OK;
    ANN_TRY(rad_emit<false>(c, "knn_exact_emit", tb, me, oe, row_begin, col_begin, c->rad_eval, tot));
    ANN_CHECK_HIP(c, hipGetLastError());
    c->kx_n_eval = tot;
    if (!evaluate) {
        c->kx_pending = true;
        ANN_CHECK_HIP(c, hipEventRecord(c->call_b, c->stream));
        c->call_timed = true;
        return ANNCHOR_OK;
    }
    ANN_TRY(rad_reserve(c, c->rad_d, sizeof(double) * (size_t)tot));
    PairSource src;
    src.ij = c->rad_eval.as<int2>();
    src.n = tot;
    ANN_TRY(ann_metric_launch(c, src, c->rad_d.as<double>(), nullptr, nullptr));
    ANN_CHECK_HIP(c, hipEventRecord(c->call_b, c->stream));
    c->call_timed = true;
    return kx_absorb(c, c->rad_eval.as<int2>(), c->rad_d.as<double>(), tot, n_entries);
}

extern "C" int annchor_knn_exact_fetch(annchor_ctx *c, int64_t *ij)
{
    if (!c) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, kx_ready(c), ANNCHOR_EINVAL, "annchor_knn_exact_begin has not run on this data set");
    const int64_t n = c->kx_n_eval;
    if (n == 0) return ANNCHOR_OK;
    if (!ij) return ANNCHOR_EINVAL;
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    return rad_pairs_out(c, c->rad_eval.p, n, ij);
}

extern "C" int annchor_knn_exact_edges(annchor_ctx *c, const int64_t *ij, const double *d, int64_t n)
{
    if (!c || n < 0 || (n > 0 && (!ij || !d))) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, kx_ready(c), ANNCHOR_EINVAL, "annchor_knn_exact_begin has not run on this data set");
    ANN_REQUIRE(c, n < (1ll << 30), ANNCHOR_ELIMIT, "%lld candidates in one call: pass them in parts", (long long)n);
    c->kx_pending = false;
    if (n == 0) return ANNCHOR_OK;
    std::vector<int2> tmp;
    ANN_TRY(rad_pairs_in(c, ij, n, c->nx, "candidate", tmp));
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    ANN_TRY(ann_side_join(c));
    // (the walk's own list buffers: the host has fetched what they held)
    c->kx_n_eval = 0;
    ANN_TRY(rad_reserve(c, c->rad_eval, sizeof(int2) * (size_t)n));
    ANN_TRY(rad_reserve(c, c->rad_d, sizeof(double) * (size_t)n));
    ANN_TRY(ann_h2d(c, c->rad_eval.p, tmp.data(), sizeof(int2) * (size_t)n));
    ANN_TRY(ann_h2d(c, c->rad_d.p, d, sizeof(double) * (size_t)n));
    int64_t added = 0;
    return kx_absorb(c, c->rad_eval.as<int2>(), c->rad_d.as<double>(), n, &added);
}

extern "C" int annchor_knn_exact_finish(annchor_ctx *c, int64_t *idx, double *dist, int64_t *row_entries, int32_t row_cap)
{
    if (!c || !idx || !dist) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, kx_ready(c), ANNCHOR_EINVAL, "annchor_knn_exact_begin has not run on this data set");
    ANN_REQUIRE(c, !c->kx_pending, ANNCHOR_EINVAL,
                "the last range's %lld candidates were emitted and never absorbed: evaluate them and pass them to annchor_knn_exact_edges",
                (long long)c->kx_n_eval);
    ANN_REQUIRE(c, row_cap >= 0, ANNCHOR_EINVAL, "row_cap must be >= 0 (0: as many slots as the workgroup's LDS holds)");
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    ANN_TRY(ann_side_join(c));
    const int64_t nx = c->nx, n = c->kx_n_entries;
    const int k = c->kx_k;
    const size_t cells = (size_t)nx * (size_t)k;
    ANN_TRY(rad_reserve(c, c->kx_off, sizeof(int64_t) * (size_t)(nx + 1)));
    ANN_TRY(rad_reserve(c, c->kx_seg, 12 * (size_t)(n > 0 ? n : 1)));
    ANN_TRY(rad_reserve(c, c->kx_out, cells * 16));
    ANN_TRY(rad_reserve(c, c->scan_tmp, sizeof(int64_t) * (size_t)(nx / 1024 + 2)));   // (the scan's block sums: found here, not carved from the slab)
    int32_t *cnt = c->kx_cnt.as<int32_t>(), *cur = cnt + nx;
    int64_t *off = c->kx_off.as<int64_t>();
    uint64_t *skey = c->kx_seg.as<uint64_t>();
    int32_t *scol = reinterpret_cast<int32_t *>(skey + (n > 0 ? n : 1));
    uint32_t *stat = reinterpret_cast<uint32_t *>(c->kx_stat.as<uint64_t>() + 1);
    int64_t *d_i = c->kx_out.as<int64_t>();
    double *d_d = reinterpret_cast<double *>(d_i + cells);
    ANN_CHECK_HIP(c, hipMemsetAsync(cur, 0, sizeof(int32_t) * (size_t)nx, c->stream));
    ANN_CHECK_HIP(c, hipMemsetAsync(stat, 0, sizeof(uint64_t), c->stream));
    ANN_CHECK_HIP(c, hipEventRecord(c->call_a, c->stream));
    k_kx_rowstat<<<ann_blocks(nx, KX_THREADS), KX_THREADS, 0, c->stream>>>(cnt, nx, k - 1, stat);
    ANN_CHECK_HIP(c, hipGetLastError());
    ANN_TRY(ann_exclusive_scan_i32_to_i64(c, cnt, off, nx));
    uint32_t hstat[2] = {0, 0};
    int64_t total = 0;
    ANN_TRY(ann_d2h2(c, hstat, stat, sizeof(hstat), &total, off + nx, sizeof(int64_t)));
    ANN_REQUIRE(c, total == n, ANNCHOR_ESTATE, "the per-row counts sum to %lld, the entry list holds %lld", (long long)total, (long long)n);
    ANN_REQUIRE(c, hstat[1] == 0, ANNCHOR_ESTATE,
                "%u rows hold fewer than k - 1 = %d entries: a radius passed to annchor_knn_exact_begin was not an upper bound of its row's k-th "
                "neighbour distance, or a range of the walk was never absorbed", hstat[1], k - 1);
    if (n > 0) {
        ProfScope ps(c, "knn_exact_scatter", (double)n * 28.0);
        k_kx_scatter<<<ann_blocks(n, KX_THREADS), KX_THREADS, 0, c->stream>>>(c->kx_ent.as<KxEntry>(), n, off, cur, skey, scol);
    }
    const int64_t max_len = (int64_t)hstat[0] + 1;
    const size_t tail = (size_t)k * 12;
    int64_t cap = (int64_t)((ROW_LDS_LIMIT - tail) / 12);
    if (cap > max_len) cap = max_len;
    if (row_cap > 0 && cap > row_cap) cap = row_cap;
    if (cap < 1) cap = 1;
    const size_t dyn = ((size_t)cap * 12 + tail + 15) & ~(size_t)15;
    ANN_TRY(row_lds_prepare(c, k_kx_rows, dyn));
    {
        ProfScope ps(c, "knn_exact_rows", (double)n * 12.0 + (double)cells * 16.0);
        k_kx_rows<<<(int)nx, ROW_THREADS, dyn, c->stream>>>(skey, scol, off, k, d_i, d_d, (int)cap);
    }
    ANN_CHECK_HIP(c, hipEventRecord(c->call_b, c->stream));
    c->call_timed = true;
    ANN_CHECK_HIP(c, hipGetLastError());
    ANN_TRY(ann_d2h(c, idx, d_i, cells * 8));
    ANN_TRY(ann_d2h(c, dist, d_d, cells * 8));
    if (row_entries) {
        std::vector<int32_t> tmp((size_t)nx);
        ANN_TRY(ann_d2h(c, tmp.data(), cnt, sizeof(int32_t) * (size_t)nx));
        for (int64_t i = 0; i < nx; ++i) row_entries[i] = tmp[(size_t)i];
    }
    return ANNCHOR_OK;
}
