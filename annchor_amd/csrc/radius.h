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

// The radius of a pair, two policies.  begin() runs once per workgroup, before the tile loop and on every lane (what it leaves
// in LDS is read behind the loop's barriers); at(jj) is the radius of (the lane's row, column jj of the chunk).
// SURE: the kernel has SURE outputs (they are written whether or not CONN can set a bit in them).
struct RadUniform {   // one r for every pair
    static constexpr bool SURE = true;
    double r;
    __device__ __forceinline__ void begin(int64_t, int64_t, int) {}
    __device__ __forceinline__ double at(int) const { return r; }
};
struct RadPerRow {    // R = max(u[i], u[j]): the lane's u[i] in a register, the chunk's 64 u[j] in LDS
    static constexpr bool SURE = false;
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
