// radius.hip -- the exact fixed-radius graph {(i, j), i < j : d(i, j) <= r} from the anchor table ("Fixed-radius
// graphs"; no reference counterpart).  Four stages:
//   classify   every pair i < j gets a class from Dt alone -- OUT (an anchor proves d > r), SURE (connectivity mode: an anchor
//              proves d < r) or EVAL -- as one bit per pair in per-(row, 64-column chunk) masks; the pair list is never built
//   emit       an exclusive scan of the masks' popcounts over the row-major [rows x chunks] table gives every pair's position:
//              EVAL and SURE lists in row-major order, ascending column inside a row, no atomic involved
//   evaluate   ann_metric_launch on the device-resident EVAL list
//   keep       d <= r, compacted in the same order with the distances (block counts, scan, emit)
// The rule (include/annchor_hip.h states it; tests/radius_cases.py restates it in NumPy, bit for bit):
//   s = Dt[a][i], t = Dt[a][j], m = (s + t) + r;   out(a): (fabs(s - t) - r) > rtol * m;   in(a): (r - (s + t)) > rtol * m
// The query form (annchor_radius_query_*) answers {(q, j) : d(Q[q], X[j]) <= r} for new points: the context holds X followed
// by Q, a classifier of its own (k_rad_classify_q) fills the same table for the rectangle queries x data, and the scan, emit,
// evaluate and keep stages are the graph form's.
#include "common.h"
#include "radius.h"   // the table's shape and k_rad_emit, shared with knnexact.hip

// Buffers of the radius stages (and of dbscan.hip) never come from the context's slab: a fit on the same context finds it as it left it.
int rad_reserve(annchor_ctx *c, DevBuf &b, size_t bytes)
{
    if (b.cap >= bytes && b.p) return ANNCHOR_OK;
    char *arena = c->arena;
    c->arena = nullptr;
    const int rc = ann_reserve(c, b, bytes);
    c->arena = arena;
    return rc;
}

// Room for `more` elements behind the `held` ones of a list that grows across calls (the DBSCAN edge list, the exact k-NN entry
// list).  Growth is geometric and a device-to-device copy of what is held.
int rad_grow(annchor_ctx *c, DevBuf &b, size_t elem, int64_t held, int64_t more, int64_t min_n, int64_t max_n, const char *list,
             const char *nouns, const char *hint, const char *where)
{
    const int64_t need = held + more;
    ANN_REQUIRE(c, need <= max_n, ANNCHOR_ELIMIT, "the %s list cannot grow to %lld %s (at most %lld)%s", list, (long long)need, nouns,
                (long long)max_n, hint);
    if (b.p && b.cap >= elem * (size_t)need) return ANNCHOR_OK;
    const bool keep = b.p && held > 0;   // (nothing to keep: the reservation of the context's own member, annchor_destroy finds it)
    int64_t want = keep ? 2 * (int64_t)(b.cap / elem) : min_n;
    if (want < need) want = need;
    if (want > max_n) want = max_n;
    void *p = nullptr;
    size_t got = 0;
    if ((keep ? ann_dev_alloc(c, &p, (elem * (size_t)want + 255) & ~(size_t)255, &got) : rad_reserve(c, b, elem * (size_t)want)) != ANNCHOR_OK) {
        ann_set_err(c, "the %s list cannot grow to %lld %s: the device allocation failed", list, (long long)want, nouns);
        return ANNCHOR_ELIMIT;
    }
    if (!keep) return ANNCHOR_OK;
    const hipError_t e = hipMemcpyAsync(p, b.p, elem * (size_t)held, hipMemcpyDeviceToDevice, c->stream);
    if (e != hipSuccess) {
        ann_dev_free(c, p, got);
        ANN_CHECK_HIP(c, e);
    }
    ANN_CHECK_HIP(c, ann_sync(c, where));   // (the old block goes back while nothing reads it)
    ann_dev_free(c, b.p, b.cap);
    b.p = p;
    b.cap = got;
    b.in_arena = false;
    return ANNCHOR_OK;
}

int rad_pairs_in(annchor_ctx *c, const int64_t *ij, int64_t n, int64_t nx, const char *noun, std::vector<int2> &out)
{
    out.resize((size_t)n);
    for (int64_t t = 0; t < n; ++t) {
        const int64_t i = ij[2 * t], j = ij[2 * t + 1];
        ANN_REQUIRE(c, i >= 0 && i < nx && j >= 0 && j < nx && i != j, ANNCHOR_EINVAL,
                    "%s %lld = (%lld, %lld): end points must be two different points of 0..%lld", noun, (long long)t, (long long)i, (long long)j,
                    (long long)(nx - 1));
        out[(size_t)t] = make_int2((int)i, (int)j);
    }
    return ANNCHOR_OK;
}

int rad_pairs_out(annchor_ctx *c, const void *dev, int64_t n, int64_t *ij)
{
    std::vector<int2> tmp((size_t)n);
    ANN_TRY(ann_d2h(c, tmp.data(), dev, sizeof(int2) * (size_t)n));
    for (int64_t t = 0; t < n; ++t) { ij[2 * t] = tmp[(size_t)t].x; ij[2 * t + 1] = tmp[(size_t)t].y; }
    return ANNCHOR_OK;
}

// The graph form's classifier: the row body of radius.h with one radius for every pair.
template <bool CONN, bool TABLE>
__global__ __launch_bounds__(RAD_ROWS) void k_rad_classify(const double *__restrict__ Dt, int64_t nx, int na, double r, double rtol,
                                                          int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end,
                                                          int64_t nchunks, uint64_t *__restrict__ mask_eval,
                                                          uint64_t *__restrict__ mask_sure, int32_t *__restrict__ cnt_eval,
                                                          int32_t *__restrict__ cnt_sure, unsigned long long *__restrict__ row_eval,
                                                          unsigned long long *__restrict__ row_sure)
{
    rad_classify_rows<CONN, TABLE>(RadUniform{r}, Dt, nx, na, rtol, row_begin, row_end, col_begin, col_end, nchunks, mask_eval, mask_sure, cnt_eval,
                                   cnt_sure, row_eval, row_sure);
}

// The rectangle queries x data: the context holds nxd data points followed by the queries (Dt is [na][nx], nx = nxd + nq), and
// every (q, j) is a valid pair -- no diagonal.  The row kernel above does not serve it: one row per lane leaves 127 of 128 lanes
// idle for a single query, and from a row at pool index >= nxd every chunk of data columns lies left of the diagonal.  Here the
// roles are swapped.  Lane = data column j, wave = one 64-column chunk, the workgroup's two waves = two adjacent chunks:
// t = Dt[a][j] is a coalesced load into registers; the block of up to RAD_QB queries is staged in LDS and read as wave-uniform
// broadcasts, and the loop runs over the block's real queries only (one query costs one iteration per tile).  A lane's verdicts
// are two 64-bit masks over the QUERIES of the block; after the last tile the ballot of bit qq across the wave is the column
// mask of (query qq, this chunk) -- the (row, chunk) entry the scan and k_rad_emit take -- and lane qq keeps it.
// s = Dt[a][nxd + q], t = Dt[a][j]: the rule's expressions as they stand.
#define RAD_QB 64        // queries per block: one verdict bit each

template <bool CONN, bool TABLE>
__global__ __launch_bounds__(2 * RAD_COLS) void k_rad_classify_q(const double *__restrict__ Dt, int64_t nx, int64_t nxd, int na, double r,
                                                                double rtol, int64_t q_begin, int64_t q_end, int64_t col_begin,
                                                                int64_t col_end, int64_t nchunks, int64_t cpairs,
                                                                uint64_t *__restrict__ mask_eval, uint64_t *__restrict__ mask_sure,
                                                                int32_t *__restrict__ cnt_eval, int32_t *__restrict__ cnt_sure,
                                                                unsigned long long *__restrict__ row_eval,
                                                                unsigned long long *__restrict__ row_sure)
{
    __shared__ double sh[RAD_QB][RAD_TA];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t qb = (int64_t)blockIdx.x / cpairs, cp = (int64_t)blockIdx.x - qb * cpairs;
    const int64_t chunk = cp * 2 + wave;
    const bool chunk_ok = chunk < nchunks;                     // (an odd chunk count: the last workgroup's second wave only helps staging)
    const int64_t q0 = q_begin + qb * RAD_QB;
    const int qn = (int)(q_end - q0 < RAD_QB ? q_end - q0 : RAD_QB);   // 1 .. 64 queries in this block
    const int64_t j = col_begin + chunk * RAD_COLS + lane;
    const bool col_ok = chunk_ok && j < col_end;
    const int64_t jc = col_ok ? j : col_end - 1;
    uint64_t outm = 0ull, inm = 0ull;
    for (int a0 = 0; a0 < na; a0 += RAD_TA) {
        const int ta = na - a0 < RAD_TA ? na - a0 : RAD_TA;
        __syncthreads();   // (the previous tile has been read)
        // (loads at clamped indices, values masked afterwards, as in k_rad_classify)
        for (int e = threadIdx.x; e < RAD_QB * RAD_TA; e += 2 * RAD_COLS) {
            const int qq = e & (RAD_QB - 1), aa = e / RAD_QB;   // qq fastest: coalesced along a row of Dt
            const double v = Dt[(size_t)(a0 + (aa < ta ? aa : ta - 1)) * (size_t)nx + (size_t)(nxd + q0 + (qq < qn ? qq : qn - 1))];
            sh[qq][aa] = (qq < qn && aa < ta) ? v : 0.0;
        }
        double t[RAD_TA];
#pragma unroll
        for (int aa = 0; aa < RAD_TA; ++aa) {
            const double v = Dt[(size_t)(a0 + (aa < ta ? aa : ta - 1)) * (size_t)nx + (size_t)jc];
            t[aa] = (col_ok && aa < ta) ? v : __longlong_as_double(0x7ff8000000000000ll);
        }
        __syncthreads();
        for (int qq = 0; qq < qn; ++qq) {
            bool o = false, n = false;
#pragma unroll
            for (int aa = 0; aa < RAD_TA; ++aa) rad_rule<CONN>(sh[qq][aa], t[aa], r, rtol, o, n);
            outm |= (uint64_t)o << qq;
            if (CONN) inm |= (uint64_t)n << qq;
        }
    }
    // transpose by ballots: lane qq takes the column masks of query qq (qn is uniform: every lane reaches every ballot)
    uint64_t em = 0ull, sm = 0ull;
    for (int qq = 0; qq < qn; ++qq) {
        const bool o = (outm >> qq) & 1ull, n = (inm >> qq) & 1ull;
        const uint64_t be = __ballot(col_ok && !o && !n);
        const uint64_t bs = CONN ? __ballot(col_ok && !o && n) : 0ull;
        if (lane == qq) { em = be; sm = bs; }
    }
    if (!chunk_ok || lane >= qn) return;
    if (TABLE) {
        const int64_t tpos = (qb * RAD_QB + lane) * nchunks + chunk;
        mask_eval[tpos] = em; mask_sure[tpos] = sm; cnt_eval[tpos] = __popcll(em); cnt_sure[tpos] = __popcll(sm);
    } else {
        const int64_t q = q0 + lane;
        if (em) atomicAdd(row_eval + q, (unsigned long long)__popcll(em));
        if (sm) atomicAdd(row_sure + q, (unsigned long long)__popcll(sm));
    }
}

#define KEEP_THREADS 256
#define KEEP_ITEMS 8
#define KEEP_TILE (KEEP_THREADS * KEEP_ITEMS)

// d <= r per candidate (a NaN is not kept); a workgroup covers KEEP_TILE consecutive candidates, a thread KEEP_ITEMS consecutive ones
__global__ __launch_bounds__(KEEP_THREADS) void k_rad_keep_count(const double *__restrict__ d, int64_t n, double r, int32_t *__restrict__ bcnt)
{
    __shared__ int wsum[KEEP_THREADS / 64];
    const int64_t base = (int64_t)blockIdx.x * KEEP_TILE + (int64_t)threadIdx.x * KEEP_ITEMS;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < KEEP_ITEMS; ++k) {
        const double v = ann_ldc(d, base + k, n);
        cnt += (base + k < n && v <= r) ? 1 : 0;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) cnt += __shfl_xor(cnt, s);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int w = 0; w < KEEP_THREADS / 64; ++w) tot += wsum[w];
        bcnt[blockIdx.x] = tot;
    }
}

__global__ __launch_bounds__(KEEP_THREADS) void k_rad_keep_emit(const double *__restrict__ d, const int2 *__restrict__ ij, int64_t n, double r,
                                                                const int64_t *__restrict__ boff, int2 *__restrict__ kij,
                                                                double *__restrict__ kd, int64_t n_kept)
{
    __shared__ int wsum[KEEP_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * KEEP_TILE + (int64_t)threadIdx.x * KEEP_ITEMS;
    double v[KEEP_ITEMS];
    bool keep[KEEP_ITEMS];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < KEEP_ITEMS; ++k) {
        v[k] = ann_ldc(d, base + k, n);
        keep[k] = base + k < n && v[k] <= r;
        cnt += keep[k] ? 1 : 0;
    }
    int inc = cnt;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int o = __shfl_up(inc, s);
        if (lane >= s) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int pre = 0;
    for (int w = 0; w < wave; ++w) pre += wsum[w];
    int64_t o = boff[blockIdx.x] + pre + inc - cnt;
#pragma unroll
    for (int k = 0; k < KEEP_ITEMS; ++k)
        if (keep[k]) {
            if (o < n_kept) { kij[o] = ij[base + k]; kd[o] = v[k]; }   // (always: boff is the scan of these counts)
            ++o;
        }
}

// Workgroups of the classify launch: the graph form (nxd == 0) takes RAD_ROWS rows x one chunk each, the query form RAD_QB
// queries x two chunks.
static int64_t rad_classify_grid(int64_t nxd, int64_t rows, int64_t nchunks)
{
    return nxd ? ((rows + RAD_QB - 1) / RAD_QB) * ((nchunks + 1) / 2) : ((rows + RAD_ROWS - 1) / RAD_ROWS) * nchunks;
}

int rad_range_check(annchor_ctx *c, int64_t nrows, int64_t ncols, int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end)
{
    ANN_REQUIRE(c, row_begin >= 0 && row_begin < row_end && row_end <= nrows, ANNCHOR_EINVAL, "row range [%lld, %lld) outside 0..%lld",
                (long long)row_begin, (long long)row_end, (long long)nrows);
    ANN_REQUIRE(c, col_begin >= 0 && col_begin <= col_end && col_end <= ncols, ANNCHOR_EINVAL, "column range [%lld, %lld) outside 0..%lld",
                (long long)col_begin, (long long)col_end, (long long)ncols);
    return ANNCHOR_OK;
}

int rad_table(annchor_ctx *c, int64_t nxd, int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end, RadTable &t)
{
    t.rows = row_end - row_begin;
    t.nchunks = (col_end - col_begin + RAD_COLS - 1) / RAD_COLS;
    t.rblocks = nxd ? (t.rows + RAD_QB - 1) / RAD_QB : (t.rows + RAD_ROWS - 1) / RAD_ROWS;
    t.entries = t.rows * t.nchunks;
    ANN_REQUIRE(c, t.entries <= RAD_TABLE_MAX && rad_classify_grid(nxd, t.rows, t.nchunks) < (1ll << 31), ANNCHOR_ELIMIT,
                "%lld rows x %lld column chunks exceed the %lld table entries of one call: take fewer rows", (long long)t.rows,
                (long long)t.nchunks, (long long)RAD_TABLE_MAX);
    return ANNCHOR_OK;
}

// nxd == 0: the pairs i < j of one data set, rows [rb, re); nxd > 0: the queries [rb, re) (pool index nxd + q) x the data columns
template <bool TABLE>
static void rad_launch_classify(annchor_ctx *c, int64_t nxd, int mode, int na, int64_t rb, int64_t re, int64_t cb, int64_t ce, int64_t nchunks,
                                uint64_t *me, uint64_t *ms, int32_t *ce_, int32_t *cs_, unsigned long long *row_e, unsigned long long *row_s)
{
    const unsigned grid = (unsigned)rad_classify_grid(nxd, re - rb, nchunks);
    const double *Dt = na > 0 ? c->Dt.as<double>() : nullptr;
    if (nxd) {
        const int64_t cpairs = (nchunks + 1) / 2;
        if (mode == 1)
            k_rad_classify_q<true, TABLE><<<grid, 2 * RAD_COLS, 0, c->stream>>>(Dt, c->nx, nxd, na, c->rad_r, c->rad_rtol, rb, re, cb, ce, nchunks,
                                                                              cpairs, me, ms, ce_, cs_, row_e, row_s);
        else
            k_rad_classify_q<false, TABLE><<<grid, 2 * RAD_COLS, 0, c->stream>>>(Dt, c->nx, nxd, na, c->rad_r, c->rad_rtol, rb, re, cb, ce, nchunks,
                                                                               cpairs, me, ms, ce_, cs_, row_e, row_s);
        return;
    }
    if (mode == 1)
        k_rad_classify<true, TABLE><<<grid, RAD_ROWS, 0, c->stream>>>(Dt, c->nx, na, c->rad_r, c->rad_rtol, rb, re, cb, ce, nchunks, me, ms, ce_, cs_,
                                                                      row_e, row_s);
    else
        k_rad_classify<false, TABLE><<<grid, RAD_ROWS, 0, c->stream>>>(Dt, c->nx, na, c->rad_r, c->rad_rtol, rb, re, cb, ce, nchunks, me, ms, ce_, cs_,
                                                                       row_e, row_s);
}

// Both count entry points.  nxd == 0: the graph form, rows = columns = the data set; nxd > 0: the query form, the rows are the
// nx - nxd queries and the columns the nxd data points.
static int rad_count(annchor_ctx *c, int64_t nxd, double r, double rtol, int32_t mode, int32_t use_bounds, int64_t *row_eval,
                     int64_t *row_sure)
{
    ANN_REQUIRE(c, c->nx >= 1, ANNCHOR_EINVAL, "no data set bound");
    ANN_REQUIRE(c, nxd >= 0 && nxd < c->nx, ANNCHOR_EINVAL, "nx_data must be in 1..%lld (data points first, at least one query after them)",
                (long long)(c->nx - 1));
    ANN_REQUIRE(c, r >= 0.0, ANNCHOR_EINVAL, "radius must be a number >= 0");          // (false for NaN)
    ANN_REQUIRE(c, rtol >= 0.0 && rtol < 1.0, ANNCHOR_EINVAL, "rtol must be in [0, 1)");
    ANN_REQUIRE(c, mode == 0 || mode == 1, ANNCHOR_EINVAL, "mode must be 0 (distance) or 1 (connectivity)");
    ANN_REQUIRE(c, !use_bounds || (c->na >= 1 && c->Dt.p), ANNCHOR_EINVAL, "use_bounds needs an anchor table (pick anchors first)");
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    ANN_TRY(ann_side_join(c));
    const int64_t nx = c->nx;
    const int64_t rows = nxd ? nx - nxd : nx, cols = nxd ? nxd : nx;
    c->rad_r = r; c->rad_rtol = rtol; c->rad_mode = mode; c->rad_use_bounds = use_bounds ? 1 : 0;
    c->rad_params = true; c->rad_nx = nx; c->rad_nxd = nxd; c->rad_evaluated = false;
    c->rad_n_eval = c->rad_n_sure = c->rad_n_kept = 0;
    const int64_t nchunks = (cols + RAD_COLS - 1) / RAD_COLS;
    const int64_t rblocks = nxd ? (rows + RAD_QB - 1) / RAD_QB : (rows + RAD_ROWS - 1) / RAD_ROWS;
    ANN_REQUIRE(c, rad_classify_grid(nxd, rows, nchunks) < (1ll << 31), ANNCHOR_ELIMIT, "%lld x %lld points exceed the classify grid",
                (long long)rows, (long long)cols);
    ANN_TRY(rad_reserve(c, c->rad_row, sizeof(unsigned long long) * 2 * (size_t)rows));
    unsigned long long *row = c->rad_row.as<unsigned long long>();
    ANN_CHECK_HIP(c, hipMemsetAsync(row, 0, sizeof(unsigned long long) * 2 * (size_t)rows, c->stream));
    const int na = use_bounds ? c->na : 0;
    ANN_CHECK_HIP(c, hipEventRecord(c->call_a, c->stream));
    {
        ProfScope ps(c, nxd ? "radius_classify_q" : "radius_classify",
                     nxd ? (double)na * 8.0 * ((double)rows * (double)((nchunks + 1) / 2) + (double)cols * (double)rblocks)
                         : (double)na * (double)nx * 8.0 * (double)(rblocks + nchunks));
        rad_launch_classify<false>(c, nxd, mode, na, 0, rows, 0, cols, nchunks, nullptr, nullptr, nullptr, nullptr, row, row + rows);
    }
    ANN_CHECK_HIP(c, hipEventRecord(c->call_b, c->stream));
    c->call_timed = true;
    ANN_CHECK_HIP(c, hipGetLastError());
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "row totals are downloaded as int64");
    ANN_TRY(ann_d2h(c, row_eval, row, sizeof(int64_t) * (size_t)rows));
    return ann_d2h(c, row_sure, row + rows, sizeof(int64_t) * (size_t)rows);
}

extern "C" int annchor_radius_count(annchor_ctx *c, double r, double rtol, int32_t mode, int32_t use_bounds, int64_t *row_eval,
                                    int64_t *row_sure)
{
    if (!c || !row_eval || !row_sure) return ANNCHOR_EINVAL;
    return rad_count(c, 0, r, rtol, mode, use_bounds, row_eval, row_sure);
}

extern "C" int annchor_radius_query_count(annchor_ctx *c, int64_t nx_data, double r, double rtol, int32_t mode, int32_t use_bounds,
                                          int64_t *row_eval, int64_t *row_sure)
{
    if (!c || !row_eval || !row_sure) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, nx_data >= 1, ANNCHOR_EINVAL, "nx_data must be >= 1");
    return rad_count(c, nx_data, r, rtol, mode, use_bounds, row_eval, row_sure);
}

// Both *_rows entry points: classify into the table, scan, emit, evaluate, keep.  nxd == 0: the graph form; nxd > 0: the rows
// are queries (pool index nxd + q), the columns data points, and the pairs are written (j, nxd + q).
static int rad_rows(annchor_ctx *c, int64_t nxd, int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end, int64_t max_pairs,
                    int32_t evaluate, int64_t *n_eval, int64_t *n_sure, int64_t *n_kept)
{
    ANN_REQUIRE(c, c->rad_params && c->rad_nx == c->nx && c->rad_nxd == nxd, ANNCHOR_EINVAL,
                nxd ? "annchor_radius_query_count has not run on this data set with this nx_data"
                    : "annchor_radius_count has not run on this data set");
    const int64_t nx = c->nx;
    const int64_t nrows = nxd ? nx - nxd : nx, ncols = nxd ? nxd : nx;
    ANN_TRY(rad_range_check(c, nrows, ncols, row_begin, row_end, col_begin, col_end));
    ANN_REQUIRE(c, !evaluate || c->metric != ANNCHOR_METRIC_NONE, ANNCHOR_EINVAL, "no device metric bound to this context");
    const int na = c->rad_use_bounds ? c->na : 0;
    ANN_REQUIRE(c, !c->rad_use_bounds || (na >= 1 && c->Dt.p), ANNCHOR_EINVAL, "the anchor table is gone");
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    ANN_TRY(ann_side_join(c));
    c->rad_n_eval = c->rad_n_sure = c->rad_n_kept = 0;
    c->rad_evaluated = false;
    ++c->rad_serial;
    *n_eval = *n_sure = *n_kept = 0;
    if (col_begin == col_end) return ANNCHOR_OK;
    RadTable tb;
    ANN_TRY(rad_table(c, nxd, row_begin, row_end, col_begin, col_end, tb));
    const int64_t rows = tb.rows, nchunks = tb.nchunks, entries = tb.entries;
    ANN_TRY(rad_reserve(c, c->rad_mask, sizeof(uint64_t) * 2 * (size_t)entries));
    ANN_TRY(rad_reserve(c, c->rad_cnt, sizeof(int32_t) * 2 * (size_t)entries));
    ANN_TRY(rad_reserve(c, c->rad_off, sizeof(int64_t) * 2 * (size_t)(entries + 1)));
    uint64_t *me = c->rad_mask.as<uint64_t>(), *ms = me + entries;
    int32_t *ce = c->rad_cnt.as<int32_t>(), *cs = ce + entries;
    int64_t *oe = c->rad_off.as<int64_t>(), *os = oe + entries + 1;
    const bool conn = c->rad_mode == 1;
    ANN_CHECK_HIP(c, hipEventRecord(c->call_a, c->stream));
    {
        ProfScope ps(c, nxd ? "radius_classify_q" : "radius_classify",
                     (double)na * 8.0 * ((double)rows * (double)(nxd ? (nchunks + 1) / 2 : nchunks) + (double)(col_end - col_begin) * (double)tb.rblocks));
        rad_launch_classify<true>(c, nxd, c->rad_mode, na, row_begin, row_end, col_begin, col_end, nchunks, me, ms, ce, cs, nullptr, nullptr);
    }
    ANN_CHECK_HIP(c, hipGetLastError());
    ANN_TRY(ann_exclusive_scan_i32_to_i64(c, ce, oe, entries));
    int64_t tot[2] = {0, 0};
    if (conn) {
        ANN_TRY(ann_exclusive_scan_i32_to_i64(c, cs, os, entries));
        ANN_TRY(ann_d2h2(c, &tot[0], oe + entries, sizeof(int64_t), &tot[1], os + entries, sizeof(int64_t)));
    } else {
        ANN_TRY(ann_d2h(c, &tot[0], oe + entries, sizeof(int64_t)));
    }
    *n_eval = tot[0];
    *n_sure = tot[1];
    if (max_pairs > 0 && tot[0] + tot[1] > max_pairs) {
        *n_kept = -1;
        return ANNCHOR_OK;
    }
    ANN_REQUIRE(c, tot[0] < (1ll << 31) && tot[1] < (1ll << 31), ANNCHOR_ELIMIT, "%lld candidate pairs in one range: pass max_pairs",
                (long long)(tot[0] + tot[1]));
    const int64_t row0 = nxd + row_begin;
    ANN_TRY(nxd ? rad_emit<true>(c, "radius_emit", tb, me, oe, row0, col_begin, c->rad_eval, tot[0])
                : rad_emit<false>(c, "radius_emit", tb, me, oe, row0, col_begin, c->rad_eval, tot[0]));
    ANN_TRY(nxd ? rad_emit<true>(c, "radius_emit", tb, ms, os, row0, col_begin, c->rad_sure, tot[1])
                : rad_emit<false>(c, "radius_emit", tb, ms, os, row0, col_begin, c->rad_sure, tot[1]));
    ANN_CHECK_HIP(c, hipGetLastError());
    c->rad_n_eval = tot[0];
    c->rad_n_sure = tot[1];
    if (!evaluate || tot[0] == 0) {
        c->rad_evaluated = evaluate != 0;
        ANN_CHECK_HIP(c, hipEventRecord(c->call_b, c->stream));
        c->call_timed = true;
        return ANNCHOR_OK;
    }
    // ---- evaluate the candidates, keep d <= r
    const int64_t n = tot[0];
    ANN_TRY(rad_reserve(c, c->rad_d, sizeof(double) * (size_t)n));
    PairSource src;
    src.ij = c->rad_eval.as<int2>();
    src.n = n;
    ANN_TRY(ann_metric_launch(c, src, c->rad_d.as<double>(), nullptr, nullptr));
    const int nb = ann_blocks(n, KEEP_TILE);
    ANN_TRY(rad_reserve(c, c->rad_bcnt, sizeof(int32_t) * (size_t)nb));
    ANN_TRY(rad_reserve(c, c->rad_boff, sizeof(int64_t) * (size_t)(nb + 1)));
    {
        ProfScope ps(c, "radius_keep", (double)n * 8.0);
        k_rad_keep_count<<<nb, KEEP_THREADS, 0, c->stream>>>(c->rad_d.as<double>(), n, c->rad_r, c->rad_bcnt.as<int32_t>());
    }
    ANN_CHECK_HIP(c, hipGetLastError());
    ANN_TRY(ann_exclusive_scan_i32_to_i64(c, c->rad_bcnt.as<int32_t>(), c->rad_boff.as<int64_t>(), nb));
    int64_t kept = 0;
    ANN_TRY(ann_d2h(c, &kept, c->rad_boff.as<int64_t>() + nb, sizeof(int64_t)));
    ANN_REQUIRE(c, kept >= 0 && kept <= n, ANNCHOR_ESTATE, "threshold pass counted %lld of %lld candidates", (long long)kept, (long long)n);
    if (kept > 0) {
        ANN_TRY(rad_reserve(c, c->rad_kept, sizeof(int2) * (size_t)kept));
        ANN_TRY(rad_reserve(c, c->rad_kd, sizeof(double) * (size_t)kept));
        ProfScope ps(c, "radius_keep", (double)n * 16.0 + (double)kept * 16.0);
        k_rad_keep_emit<<<nb, KEEP_THREADS, 0, c->stream>>>(c->rad_d.as<double>(), c->rad_eval.as<int2>(), n, c->rad_r, c->rad_boff.as<int64_t>(),
                                                            c->rad_kept.as<int2>(), c->rad_kd.as<double>(), kept);
        ANN_CHECK_HIP(c, hipGetLastError());
    }
    ANN_CHECK_HIP(c, hipEventRecord(c->call_b, c->stream));
    c->call_timed = true;
    c->rad_n_kept = kept;
    c->rad_evaluated = true;
    *n_kept = kept;
    return ANNCHOR_OK;
}

extern "C" int annchor_radius_rows(annchor_ctx *c, int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end,
                                   int64_t max_pairs, int32_t evaluate, int64_t *n_eval, int64_t *n_sure, int64_t *n_kept)
{
    if (!c || !n_eval || !n_sure || !n_kept) return ANNCHOR_EINVAL;
    return rad_rows(c, 0, row_begin, row_end, col_begin, col_end, max_pairs, evaluate, n_eval, n_sure, n_kept);
}

extern "C" int annchor_radius_query_rows(annchor_ctx *c, int64_t nx_data, int64_t q_begin, int64_t q_end, int64_t col_begin, int64_t col_end,
                                         int64_t max_pairs, int32_t evaluate, int64_t *n_eval, int64_t *n_sure, int64_t *n_kept)
{
    if (!c || !n_eval || !n_sure || !n_kept) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, nx_data >= 1 && nx_data < c->nx, ANNCHOR_EINVAL, "nx_data must be in 1..%lld", (long long)(c->nx - 1));
    return rad_rows(c, nx_data, q_begin, q_end, col_begin, col_end, max_pairs, evaluate, n_eval, n_sure, n_kept);
}

extern "C" int annchor_radius_fetch(annchor_ctx *c, int32_t which, int64_t *ij, double *d)
{
    if (!c) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, which >= 0 && which <= 2, ANNCHOR_EINVAL, "which must be 0 (candidates), 1 (sure pairs) or 2 (kept pairs)");
    ANN_REQUIRE(c, c->rad_params, ANNCHOR_EINVAL, "no radius range has been processed");
    ANN_REQUIRE(c, which != 2 || c->rad_evaluated, ANNCHOR_EINVAL, "the last range was not evaluated: there are no kept pairs");
    const int64_t n = which == 0 ? c->rad_n_eval : which == 1 ? c->rad_n_sure : c->rad_n_kept;
    if (n == 0) return ANNCHOR_OK;
    if (!ij) return ANNCHOR_EINVAL;
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    const DevBuf &src = which == 0 ? c->rad_eval : which == 1 ? c->rad_sure : c->rad_kept;
    ANN_TRY(rad_pairs_out(c, src.p, n, ij));
    if (d && which == 2) return ann_d2h(c, d, c->rad_kd.p, sizeof(double) * (size_t)n);
    if (d && which == 0 && c->rad_evaluated) return ann_d2h(c, d, c->rad_d.p, sizeof(double) * (size_t)n);
    return ANNCHOR_OK;
}
