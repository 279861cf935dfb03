// radius.h -- what the pair classifiers of radius.hip and knnexact.hip share: the pruning rule, the row classifier's body, the
// shape of the (row, 64-column chunk) table, the kernel that turns its masks into a pair list, and the host steps of a range
// (range checks, table arithmetic, emit).
#pragma once
#include "common.h"

#define RAD_ROWS 128     // rows per workgroup: one row per lane, two waves
#define RAD_COLS 64      // columns per chunk: one mask bit each
#define RAD_TA 32        // anchors per tile: a lane's s values in registers, the chunk's t values in LDS
#define RAD_TABLE_MAX (1ll << 23)   // (row, chunk) entries per annchor_radius_rows call: 24 B each

// The rule, for one anchor (include/annchor_hip.h states it; tests/radius_cases.py restates it in NumPy, bit for bit):
//   s = Dt[a][i], t = Dt[a][j], m = (s + t) + R;   out: (fabs(s - t) - R) > rtol * m;   in (CONN): (R - (s + t)) > rtol * m
// A verdict is or-ed into o / n.  A NaN in s or t makes neither comparison true.  R = +inf: -inf > rtol * inf is false (and so
// is -inf > NaN at rtol = 0), so the pair is neither out nor in.
template <bool CONN>
__device__ __forceinline__ void rad_rule(double s, double t, double R, double rtol, bool &o, bool &n)
{
    const double sum = s + t;
    const double m = sum + R;
    const double tol = rtol * m;
    o |= (fabs(s - t) - R) > tol;
    if (CONN) n |= (R - sum) > tol;
}

// The radius of a pair, four policies.  begin() runs once per workgroup, before the tile loop and on every lane (what it leaves
// in LDS is read behind a barrier); at(jj) is the radius of (the lane's row, column jj of the chunk); veto(jj): the pair is OUT
// whatever the anchors say (read where VETO is set, behind the tile loop -- with no anchors at all it is the only verdict).
// SURE: the kernel has SURE outputs (they are written whether or not CONN can set a bit in them).
struct RadUniform {   // one r for every pair
    static constexpr bool SURE = true, VETO = false;
    double r;
    __device__ __forceinline__ void begin(int64_t, int64_t, int) {}
    __device__ __forceinline__ double at(int) const { return r; }
    __device__ __forceinline__ bool veto(int) const { return false; }
};
struct RadPerRow {    // R = max(u[i], u[j]): the lane's u[i] in a register, the chunk's 64 u[j] in LDS
    static constexpr bool SURE = false, VETO = false;
    const double *__restrict__ u;
    double *shu;      // [RAD_COLS], LDS
    double ui;
    __device__ __forceinline__ void begin(int64_t ic, int64_t jc0, int jn)
    {
        ui = u[ic];
        if (threadIdx.x < RAD_COLS) shu[threadIdx.x] = u[jc0 + ((int)threadIdx.x < jn ? (int)threadIdx.x : jn - 1)];
    }
    __device__ __forceinline__ double at(int jj) const
    {
        const double uj = shu[jj];
        return ui > uj ? ui : uj;
    }
    __device__ __forceinline__ bool veto(int) const { return false; }
};
// RadPerRow's radius, and a pair inside one component is OUT (mst.hip): the lane's comp[i] in a register, the chunk's 64
// comp[j] in LDS beside the radii.  (The veto is a verdict of its own, not R = -inf: at rtol = 0 the margin 0 * -inf is NaN
// and no comparison with it is true.)
struct RadComponent {
    static constexpr bool SURE = false, VETO = true;
    const double *__restrict__ u;
    const int32_t *__restrict__ comp;
    double *shu;      // [RAD_COLS], LDS
    int32_t *shc;     // [RAD_COLS], LDS
    double ui;
    int32_t ci;
    __device__ __forceinline__ void begin(int64_t ic, int64_t jc0, int jn)
    {
        ui = u[ic];
        ci = comp[ic];
        if (threadIdx.x < RAD_COLS) {
            const int64_t j = jc0 + ((int)threadIdx.x < jn ? (int)threadIdx.x : jn - 1);
            shu[threadIdx.x] = u[j];
            shc[threadIdx.x] = comp[j];
        }
    }
    __device__ __forceinline__ double at(int jj) const
    {
        const double uj = shu[jj];
        return ui > uj ? ui : uj;
    }
    __device__ __forceinline__ bool veto(int jj) const { return shc[jj] == ci; }
};
// RadComponent for mutual-reachability weights w = max(d, core[i], core[j]) (mst.hip, the reach form): u bounds w, and a pair
// whose max(core[i], core[j]) exceeds both ends' bounds is OUT before any anchor is asked -- its weight can be the lightest
// outgoing edge of neither end.  The comparison is exact (no rtol: both sides are computed values) and needs no triangle
// inequality.  The lane's core[i] in a register, the chunk's 64 core[j] in LDS beside the radii and components.  The anchor
// rule stays the one on d: d <= w, so "d > R" proves "w > R".
struct RadReach {
    static constexpr bool SURE = false, VETO = true;
    const double *__restrict__ u;
    const int32_t *__restrict__ comp;
    const double *__restrict__ core;
    double *shu;      // [RAD_COLS], LDS
    int32_t *shc;     // [RAD_COLS], LDS
    double *shk;      // [RAD_COLS], LDS: core[j]
    double ui, ki;
    int32_t ci;
    __device__ __forceinline__ void begin(int64_t ic, int64_t jc0, int jn)
    {
        ui = u[ic];
        ci = comp[ic];
        ki = core[ic];
        if (threadIdx.x < RAD_COLS) {
            const int64_t j = jc0 + ((int)threadIdx.x < jn ? (int)threadIdx.x : jn - 1);
            shu[threadIdx.x] = u[j];
            shc[threadIdx.x] = comp[j];
            shk[threadIdx.x] = core[j];
        }
    }
    __device__ __forceinline__ double at(int jj) const
    {
        const double uj = shu[jj];
        return ui > uj ? ui : uj;
    }
    __device__ __forceinline__ bool veto(int jj) const
    {
        const double kj = shk[jj];
        return shc[jj] == ci || (ki > kj ? ki : kj) > at(jj);
    }
};

// The row classifier's body (k_rad_classify, k_kx_classify).  One workgroup = RAD_ROWS rows x one chunk of RAD_COLS columns.
// Lane = row i: Dt[a][i] is a coalesced load; the chunk's columns are wave-uniform per iteration and come from LDS as
// broadcasts.  Anchors in tiles of RAD_TA; the lane's verdicts so far live in two 64-bit masks, so any anchor count is a loop
// over tiles.  A tile's missing anchors are NaN in s: neither comparison is true for them.
// TABLE: masks and counts go to the [rows x nchunks] table; otherwise the popcounts are added to the per-row totals (integer
// sums: the totals do not depend on the order of the additions).
template <bool CONN, bool TABLE, typename RADIUS>
__device__ __forceinline__ void rad_classify_rows(RADIUS rad, const double *__restrict__ Dt, int64_t nx, int na, double rtol, int64_t row_begin,
                                                  int64_t row_end, int64_t col_begin, int64_t col_end, int64_t nchunks,
                                                  uint64_t *__restrict__ mask_eval, uint64_t *__restrict__ mask_sure,
                                                  int32_t *__restrict__ cnt_eval, int32_t *__restrict__ cnt_sure,
                                                  unsigned long long *__restrict__ row_eval, unsigned long long *__restrict__ row_sure)
{
    __shared__ double sh[RAD_COLS][RAD_TA];
    const int64_t rb = (int64_t)blockIdx.x / nchunks, chunk = (int64_t)blockIdx.x - rb * nchunks;
    const int64_t ridx = rb * RAD_ROWS + threadIdx.x;          // row inside the range
    const int64_t i = row_begin + ridx;
    const bool row_ok = i < row_end;
    const int64_t jc0 = col_begin + chunk * RAD_COLS;
    const int jn = (int)(col_end - jc0 < RAD_COLS ? col_end - jc0 : RAD_COLS);   // 1 .. 64 columns in this chunk
    const int64_t tpos = ridx * nchunks + chunk;
    if (jc0 + jn - 1 <= row_begin + rb * RAD_ROWS) {
        // the chunk lies on or left of the diagonal for every row of the workgroup (uniform: before any barrier)
        if (TABLE && row_ok) {
            mask_eval[tpos] = 0ull; cnt_eval[tpos] = 0;
            if (RADIUS::SURE) { mask_sure[tpos] = 0ull; cnt_sure[tpos] = 0; }
        }
        return;
    }
    const int64_t ic = row_ok ? i : row_end - 1;
    rad.begin(ic, jc0, jn);
    uint64_t outm = 0ull, inm = 0ull;
    for (int a0 = 0; a0 < na; a0 += RAD_TA) {
        const int ta = na - a0 < RAD_TA ? na - a0 : RAD_TA;
        __syncthreads();   // (the previous tile has been read)
        // (loads at clamped indices, values masked afterwards: a load inside a branch would wait for memory once per element)
        for (int e = threadIdx.x; e < RAD_COLS * RAD_TA; e += RAD_ROWS) {
            const int jj = e & (RAD_COLS - 1), aa = e / RAD_COLS;   // jj fastest: coalesced along a row of Dt
            const double v = Dt[(size_t)(a0 + (aa < ta ? aa : ta - 1)) * (size_t)nx + (size_t)(jc0 + (jj < jn ? jj : jn - 1))];
            sh[jj][aa] = (jj < jn && aa < ta) ? v : 0.0;
        }
        double s[RAD_TA];
#pragma unroll
        for (int aa = 0; aa < RAD_TA; ++aa) {
            const double v = Dt[(size_t)(a0 + (aa < ta ? aa : ta - 1)) * (size_t)nx + (size_t)ic];
            s[aa] = (row_ok && aa < ta) ? v : __longlong_as_double(0x7ff8000000000000ll);
        }
        __syncthreads();
        for (int jj = 0; jj < jn; ++jj) {
            const double R = rad.at(jj);
            bool o = false, n = false;
#pragma unroll
            for (int aa = 0; aa < RAD_TA; ++aa) rad_rule<CONN>(s[aa], sh[jj][aa], R, rtol, o, n);
            outm |= (uint64_t)o << jj;
            if (CONN) inm |= (uint64_t)n << jj;
        }
    }
    if (RADIUS::VETO) {
        __syncthreads();   // (what begin() left in LDS: no barrier has run yet when there are no anchors)
        for (int jj = 0; jj < jn; ++jj) outm |= (uint64_t)rad.veto(jj) << jj;
    }
    // valid columns of this lane: jj < jn and jc0 + jj > i
    uint64_t vm = 0ull;
    if (row_ok) {
        vm = jn == RAD_COLS ? ~0ull : ((1ull << jn) - 1ull);
        const int64_t lo = i + 1 - jc0;   // first valid bit
        if (lo >= RAD_COLS) vm = 0ull;
        else if (lo > 0) vm &= ~0ull << lo;
    }
    const uint64_t em = vm & ~outm & ~inm, sm = vm & ~outm & inm;
    if (TABLE) {
        if (row_ok) {
            mask_eval[tpos] = em; cnt_eval[tpos] = __popcll(em);
            if (RADIUS::SURE) { mask_sure[tpos] = sm; cnt_sure[tpos] = __popcll(sm); }
        }
    } else {
        if (em) atomicAdd(row_eval + i, (unsigned long long)__popcll(em));
        if (RADIUS::SURE && sm) atomicAdd(row_sure + i, (unsigned long long)__popcll(sm));
    }
}

// one thread per (row, chunk): the pairs of its mask, ascending column, at the scan's offset.  SWAP (the query form: a row is
// a query at pool index row_begin + ridx): the pair is written column first, (j, row)
template <bool SWAP>
__global__ __launch_bounds__(256) void k_rad_emit(const uint64_t *__restrict__ mask, const int64_t *__restrict__ off, int64_t entries,
                                                  int64_t nchunks, int64_t row_begin, int64_t col_begin, int2 *__restrict__ out,
                                                  int64_t n_out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= entries) return;
    uint64_t m = mask[t];
    if (!m) return;
    const int64_t ridx = t / nchunks, chunk = t - ridx * nchunks;
    const int i = (int)(row_begin + ridx);
    const int64_t j0 = col_begin + chunk * RAD_COLS;
    int64_t o = off[t];
    while (m) {
        const int b = __ffsll((long long)m) - 1;
        m &= m - 1ull;
        if (o < n_out) out[o] = SWAP ? make_int2((int)(j0 + b), i) : make_int2(i, (int)(j0 + b));   // (o < n_out always: the offsets are the scan of these popcounts)
        ++o;
    }
}

// ---- the host steps every *_rows entry point takes for its range [row_begin, row_end) x [col_begin, col_end)
struct RadTable {   // the range's (row, chunk) table
    int64_t rows, nchunks, rblocks, entries;
};
// radius.hip.  rad_range_check: the ranges lie inside nrows x ncols.  rad_table: the table's arithmetic and what one call
// takes (nxd > 0: the query form's workgroups).
int rad_range_check(annchor_ctx *c, int64_t nrows, int64_t ncols, int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end);
int rad_table(annchor_ctx *c, int64_t nxd, int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end, RadTable &t);

// A walk of another stage (knnexact.hip, mst.hip) writes the radius stages' table, scans and lists: what annchor_radius_count
// fixed no longer describes them.
static inline void rad_buffers_taken(annchor_ctx *c)
{
    c->rad_params = false;
    c->rad_evaluated = false;
    c->rad_n_eval = c->rad_n_sure = c->rad_n_kept = 0;
}

// One class of the table to its pair list: room for the scan's total in `out`, then k_rad_emit.  row0: the pool index of the
// table's first row.
template <bool SWAP>
static int rad_emit(annchor_ctx *c, const char *scope, const RadTable &t, const uint64_t *mask, const int64_t *off, int64_t row0, int64_t col_begin,
                    DevBuf &out, int64_t tot)
{
    if (tot == 0) return ANNCHOR_OK;
    ANN_TRY(rad_reserve(c, out, sizeof(int2) * (size_t)tot));
    ProfScope ps(c, scope, (double)t.entries * 16.0 + (double)tot * 8.0);
    k_rad_emit<SWAP><<<ann_blocks(t.entries, 256), 256, 0, c->stream>>>(mask, off, t.entries, t.nchunks, row0, col_begin, out.as<int2>(), tot);
    return ANNCHOR_OK;
}

// The classify, scan and emit stages of a range whose only class is EVAL (knnexact.hip, mst.hip): the table in rad_mask /
// rad_cnt / rad_off, the candidates in rad_eval.  classify(row_begin, row_end, col_begin, col_end, nchunks, mask, cnt) queues
// the caller's TABLE kernel.  *tot = the candidates; *emitted = false: more than max_pairs (> 0) of them, nothing was written.
template <typename CLASSIFY>
static int rad_range_candidates(annchor_ctx *c, const char *classify_scope, const char *emit_scope, int na, int64_t row_begin, int64_t row_end,
                                int64_t col_begin, int64_t col_end, int64_t max_pairs, CLASSIFY classify, int64_t *tot, bool *emitted)
{
    *tot = 0;
    *emitted = true;
    RadTable tb;
    ANN_TRY(rad_table(c, 0, row_begin, row_end, col_begin, col_end, tb));
    const int64_t entries = tb.entries;
    ANN_TRY(rad_reserve(c, c->rad_mask, sizeof(uint64_t) * (size_t)entries));
    ANN_TRY(rad_reserve(c, c->rad_cnt, sizeof(int32_t) * (size_t)entries));
    ANN_TRY(rad_reserve(c, c->rad_off, sizeof(int64_t) * (size_t)(entries + 1)));
    ANN_TRY(rad_reserve(c, c->scan_tmp, sizeof(int64_t) * (size_t)(entries / 1024 + 2)));   // (the scan's block sums: found here, not carved from the slab)
    uint64_t *me = c->rad_mask.as<uint64_t>();
    int32_t *cn = c->rad_cnt.as<int32_t>();
    int64_t *oe = c->rad_off.as<int64_t>();
    {
        ProfScope ps(c, classify_scope, (double)na * 8.0 * ((double)tb.rows * (double)tb.nchunks + (double)(col_end - col_begin) * (double)tb.rblocks));
        classify(row_begin, row_end, col_begin, col_end, tb.nchunks, me, cn);
    }
    ANN_CHECK_HIP(c, hipGetLastError());
    ANN_TRY(ann_exclusive_scan_i32_to_i64(c, cn, oe, entries));
    ANN_TRY(ann_d2h(c, tot, oe + entries, sizeof(int64_t)));
    if (max_pairs > 0 && *tot > max_pairs) {
        *emitted = false;
        return ANNCHOR_OK;
    }
    ANN_REQUIRE(c, *tot < (1ll << 30), ANNCHOR_ELIMIT, "%lld candidate pairs in one range: pass max_pairs", (long long)*tot);
    ANN_TRY(rad_emit<false>(c, emit_scope, tb, me, oe, row_begin, col_begin, c->rad_eval, *tot));
    ANN_CHECK_HIP(c, hipGetLastError());
    return ANNCHOR_OK;
}
