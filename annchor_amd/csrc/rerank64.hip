// rerank64.hip -- float64 rows in the streamed form: the float32 pipeline is the filter, float64 differences decide.
//
// The reference computes `euclidean` in the dtype of X (annchor/distances.py:8-13: np.linalg.norm(x - y)); for float64 rows that
// is float64 DIFFERENCES.  The streamed form computes in float32.  Nothing of it changes here: annchor_stream_bind_f64 keeps the
// float64 rows resident, subtracts a float64 centre (the column means) and hands the CENTRED rows, narrowed to float32, to the
// pipeline as if annchor_stream_bind had been given them -- anchors, k-d order, split copy, tile phase, joins run on that copy
// with lists a few entries longer than asked for (K' = K + margin).  Then, per row (k_r64_rerank, one wavefront per row):
//   gather   the K' listed columns' float64 rows (K' dim 8 bytes per row: the kernel is a gather at memory speed)
//   re-rank  d^2 = sum (x_k - y_k)^2 in float64, ordered by (d^2, index); the first K are the row's list
//   guard    every column the float32 search left out is at least d_last (1 - 3 gamma32) away ON THE FLOAT32 COPY (d_last: the
//            K'-th float32 entry; gamma32 = (dimp + 4) 2^-24: the search's own completeness bound), the copy moved row i by at
//            most e_i and column c by at most u (|x~_i| + d): a row whose exact K-th distance stays below
//            L = (d_last (1 - 3 gamma32) - 2 e_i) / (1 + u) is certified -- DESIGN.md, "float64 rows", has the derivation
//   repair   every other row is flagged (a bit per row in a word per 32 rows, as guard_tiles) and done again against EVERY
//            column by float64 differences (k_r64_repair, the float64 sibling of k_st_repair)
// With the tile budget not binding the result is the float64 k-NN graph; with a binding budget the lists are float64-exact
// re-rankings of what the budget found and nothing is flagged or repaired.
//
// Why one wavefront per row and not one workgroup per 128-row tile: the rows of a tile share no candidate row that is worth
// keeping on chip (K' distinct columns each, overlapping only by accident; L2 catches that), so a tile-wide workgroup would buy
// barriers and nothing else.  A wave reads one candidate row of up to 128 dimensions as ONE 1 KB request (64 lanes x 16 bytes,
// whole 128-byte lines), keeps the row operand in registers (<= 16 doubles per lane at 1024 dimensions), reduces with
// cross-lane shuffles and sorts its K' <= 128 entries by rank counting in 2 KB of LDS behind wave-local fences; no block barrier
// anywhere, four independent rows per workgroup, enough waves per SIMD to cover the gather's latency.
#include "streamed.h"

#define R64_U 0x1p-24                 // unit roundoff of float32
#define R64_UP (0x1p-24 * (1.0 + 0x1p-20))   // ... with room for the float64 roundings of centring and of the norm
#define R64_KMAX 128
#define R64_MAXDIM 1024
#define R64_ID_NONE 0x7fffffffffffffffll

// ------------------------------------------------------------------------------------------------------------------ bind
// column sums in a fixed order (the centre decides the float32 copy: it must not depend on the order atomics land in)
__global__ __launch_bounds__(256) void k_r64_colsum(const double *__restrict__ X, int64_t n, int dim, int64_t rows_per_block, double *__restrict__ part)
{
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block, r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
    for (int k = threadIdx.x; k < dim; k += 256) {
        double s = 0.0;
        for (int64_t r = r0; r < r1; ++r) s += X[(size_t)r * dim + k];
        part[(size_t)blockIdx.x * dim + k] = s;
    }
}

__global__ void k_r64_centre(const double *__restrict__ part, int nblk, int dim, int64_t n, double *__restrict__ centre)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= dim) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += part[(size_t)b * dim + k];
    centre[k] = s / (double)n;
}

// smallest float >= v (v >= 0)
__device__ __forceinline__ float r64_float_up(double v)
{
    float f = (float)v;
    if ((double)f < v) f = nextafterf(f, INFINITY);
    return f;
}

// one wavefront per row: x~ = x - centre in float64, narrowed to float32 into the buffer annchor_stream_bind fills; e = bound of
// |x~ - float32(x~)|: 2^-24 |x~| per coordinate in the normal range, 2^-150 below it
__global__ __launch_bounds__(256) void k_r64_narrow(const double *__restrict__ X, const double *__restrict__ centre, int64_t n, int dim,
                                                    float *__restrict__ X32, float *__restrict__ e)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    double s = 0.0;
    for (int k = lane; k < dim; k += 64) {
        const double v = X[(size_t)r * dim + k] - centre[k];
        X32[(size_t)r * dim + k] = (float)v;
        s += v * v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) e[r] = r64_float_up(R64_UP * sqrt(s) + sqrt((double)dim) * 0x1p-149);   // (NaN / inf rows: never certified)
}

// ------------------------------------------------------------------------------------------------------- distances
// A wave's share of sum (x_k - y_k)^2: lane l takes the 16-byte pairs l, l + 64, ... (VEC: even dim, rows 16-byte aligned) or the
// single coordinates l, l + 64, ...; xr holds the row operand's share in registers.
template <bool VEC> __device__ __forceinline__ void r64_load_row(const double *__restrict__ x, int dim, int lane, double (&xr)[16])
{
    if (VEC) {
        const double2 *x2 = reinterpret_cast<const double2 *>(x);
        const int h = dim >> 1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int t = lane + 64 * j;
            const double2 v = t < h ? x2[t] : make_double2(0.0, 0.0);
            xr[2 * j] = v.x; xr[2 * j + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int t = lane + 64 * j;
            xr[j] = t < dim ? x[t] : 0.0;
        }
    }
}

template <bool VEC> __device__ __forceinline__ double r64_sqdist(const double (&xr)[16], const double *__restrict__ y, int dim, int lane)
{
    double s0 = 0.0, s1 = 0.0;
    if (VEC) {
        const double2 *y2 = reinterpret_cast<const double2 *>(y);
        const int h = dim >> 1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int t = lane + 64 * j;
            if (t < h) {
                const double2 v = y2[t];
                const double a = xr[2 * j] - v.x, b = xr[2 * j + 1] - v.y;
                s0 += a * a; s1 += b * b;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int t = lane + 64 * j;
            if (t < dim) { const double a = xr[j] - y[t]; s0 += a * a; }
        }
    }
    double s = s0 + s1;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

__device__ __forceinline__ bool r64_before(double da, int64_t ia, double db, int64_t ib) { return da < db || (da == db && ia < ib); }

struct R64Args {
    const double *Xr;        // [n_rows][dim] float64 rows of the row side (graph: the data; query: the queries)
    const float *er;         // [n_rows] their narrowing bounds
    const int64_t *perm_r;   // [rows] global id of each tile-order row (-1 padding)
    int64_t rows, n_rows, base_r;
    const double *Xc;        // [n_cols][dim] float64 rows of the column side (the data)
    int64_t n_cols, base_c;
    int dim, Kp, Kout, self; // K' listed columns per row; Kout emitted (after the self column when self = 1)
    const int64_t *cidx;     // [rows][Kp] global ids of the float32 lists (-1: none)
    const float *cdist;      // [rows][Kp] their float32 distances, ascending
    int64_t *oidx;           // [n_rows][self + Kout]
    double *odist;
    double gamma32;          // (dimp + 4) 2^-24
    double gamma64;          // (dimp + 4) 2^-52
    int exact;               // 1: the tile budget did not bind -- guard the rows
    uint32_t *flags;         // [ceil(rows / 128)][4]
    unsigned long long *nflag;
};

// -------------------------------------------------------------------------------------------------------- re-rank + guard
template <bool VEC> __global__ __launch_bounds__(256) void k_r64_rerank(R64Args a)
{
    __shared__ double sd[4][R64_KMAX];
    __shared__ int64_t si[4][R64_KMAX];
    __shared__ double sk[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * 4 + w;
    if (r >= a.rows) return;                       // (wave-uniform, and no block barrier below)
    const int64_t g = a.perm_r[r];
    const int64_t loc = g - a.base_r;
    if (g < 0 || loc < 0 || loc >= a.n_rows) return;   // padding row
    double xr[16];
    r64_load_row<VEC>(a.Xr + (size_t)loc * a.dim, a.dim, lane, xr);
    const int Kp = a.Kp;
    for (int e = 0; e < Kp; ++e) {
        const int64_t cid = a.cidx[(size_t)r * Kp + e];    // (uniform)
        const int64_t cl = cid - a.base_c;
        const bool ok = cid >= 0 && cl >= 0 && cl < a.n_cols && !(a.self && cid == g);
        double d2 = INFINITY;
        if (ok) d2 = r64_sqdist<VEC>(xr, a.Xc + (size_t)cl * a.dim, a.dim, lane);
        if (lane == 0) { sd[w][e] = ok ? d2 : INFINITY; si[w][e] = ok ? cid : R64_ID_NONE; }
    }
    if (lane == 0) sk[w] = INFINITY;
    wave_fence_lds();
    // a column listed twice counts once (the float32 lists hold none; a re-rank must not depend on it)
    bool dup[2] = {false, false};
    for (int q = 0; q < 2; ++q) {
        const int e = lane + 64 * q;
        if (e < Kp && si[w][e] != R64_ID_NONE)
            for (int f = 0; f < e; ++f) dup[q] |= si[w][f] == si[w][e];
    }
    wave_fence_lds();
    for (int q = 0; q < 2; ++q)
        if (dup[q]) { sd[w][lane + 64 * q] = INFINITY; si[w][lane + 64 * q] = R64_ID_NONE; }
    wave_fence_lds();
    const int kk = a.self + a.Kout;
    for (int q = 0; q < 2; ++q) {
        const int e = lane + 64 * q;
        if (e >= Kp) continue;
        const double d = sd[w][e];
        const int64_t id = si[w][e];
        int rank = 0;
        for (int f = 0; f < Kp; ++f) {
            const double df = sd[w][f];
            const int64_t idf = si[w][f];
            rank += (r64_before(df, idf, d, id) || (df == d && idf == id && f < e)) ? 1 : 0;
        }
        if (rank < a.Kout) {
            const bool ok = id != R64_ID_NONE;
            a.oidx[(size_t)loc * kk + a.self + rank] = ok ? id : -1;
            a.odist[(size_t)loc * kk + a.self + rank] = ok ? sqrt(d) : INFINITY;
            if (rank == a.Kout - 1) sk[w] = ok ? sqrt(d) : INFINITY;
        }
    }
    if (a.self && lane == 0) { a.oidx[(size_t)loc * kk] = g; a.odist[(size_t)loc * kk] = 0.0; }
    if (Kp < a.Kout && lane == 0)
        for (int e = Kp; e < a.Kout; ++e) { a.oidx[(size_t)loc * kk + a.self + e] = -1; a.odist[(size_t)loc * kk + a.self + e] = INFINITY; }
    if (!a.exact) return;
    wave_fence_lds();
    if (lane == 0) {
        // certified: every unlisted column is provably farther than the K-th exact entry (strictly: ties cannot cross the boundary)
        const double dlast = (double)a.cdist[(size_t)r * Kp + Kp - 1];   // (+inf: the list holds every column there is)
        const double L = (dlast * (1.0 - 3.0 * a.gamma32) - 2.0 * (double)a.er[loc]) / (1.0 + R64_UP);
        const bool certified = Kp >= a.Kout && sk[w] * (1.0 + a.gamma64) < L;   // (NaN: not certified)
        if (!certified) {
            atomicOr(&a.flags[(size_t)(r >> 7) * 4 + ((r & 127) >> 5)], 1u << (r & 31));
            atomicAdd(a.nflag, 1ull);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- repair
// the flagged rows as a list: one thread per flag word, tile-order row numbers appended in any order
__global__ void k_r64_list(const uint32_t *__restrict__ flags, int64_t nwords, uint32_t *__restrict__ list, uint32_t *__restrict__ count, uint32_t cap)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwords) return;
    uint32_t bits = flags[w];
    while (bits) {
        const int b = __builtin_ctz(bits);
        bits &= bits - 1;
        const uint32_t slot = atomicAdd(count, 1u);
        if (slot < cap) list[slot] = (uint32_t)(w * 32 + b);
    }
}

// One workgroup per flagged row against EVERY column: 16 lanes per column sum (x - y)^2 in float64 (16-byte loads where the
// dimension is even), 256 columns per round; the columns that beat the row's K-th entry are collected and inserted in
// (d^2, index) order.  n dim 8 bytes per flagged row: the price of a row the float32 copy cannot decide.
#define R64_ROUND 256
template <bool VEC> __global__ __launch_bounds__(256) void k_r64_repair(R64Args a, const uint32_t *__restrict__ list, const uint32_t *__restrict__ count)
{
    if (blockIdx.x >= *count) return;
    const int64_t r = list[blockIdx.x];
    const int64_t g = a.perm_r[r];
    const int64_t loc = g - a.base_r;
    if (g < 0 || loc < 0 || loc >= a.n_rows) return;   // (uniform)
    __shared__ double xrow[R64_MAXDIM];
    __shared__ double ld[R64_KMAX];        // the row's list: d^2 ascending by (d^2, index)
    __shared__ int64_t lc[R64_KMAX];
    __shared__ double cd[R64_ROUND];       // candidates of one round
    __shared__ int64_t cc[R64_ROUND];
    __shared__ int ncand;
    const int tid = threadIdx.x, sub = tid & 15, grp = tid >> 4;
    const int K = a.Kout, dim = a.dim;
    for (int k = tid; k < dim; k += 256) xrow[k] = a.Xr[(size_t)loc * dim + k];
    if (tid < K) { ld[tid] = INFINITY; lc[tid] = R64_ID_NONE; }
    if (tid == 0) ncand = 0;
    __syncthreads();
    for (int64_t c0 = 0; c0 < a.n_cols; c0 += R64_ROUND) {
        const double thr = ld[K - 1];
        const int64_t thc = lc[K - 1];
        for (int step = 0; step < R64_ROUND / 16; ++step) {
            const int64_t col = c0 + step * 16 + grp;     // (uniform over the 16 lanes of a group)
            if (col >= a.n_cols) continue;
            const double *y = a.Xc + (size_t)col * dim;
            double s0 = 0.0, s1 = 0.0;
            if (VEC) {
                const double2 *y2 = reinterpret_cast<const double2 *>(y), *x2 = reinterpret_cast<const double2 *>(xrow);
                for (int t = sub; t < (dim >> 1); t += 16) {
                    const double2 u = x2[t], v = y2[t];
                    const double p = u.x - v.x, q = u.y - v.y;
                    s0 += p * p; s1 += q * q;
                }
            } else {
                for (int t = sub; t < dim; t += 16) { const double p = xrow[t] - y[t]; s0 += p * p; }
            }
            double d = s0 + s1;
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) d += __shfl_xor(d, off, 16);
            const int64_t id = col + a.base_c;
            if (sub == 0 && !(a.self && id == g) && r64_before(d, id, thr, thc)) {   // (NaN distances never enter)
                const int slot = atomicAdd(&ncand, 1);     // (at most one append per column: slot < R64_ROUND)
                cd[slot] = d; cc[slot] = id;
            }
        }
        // the count is taken between two barriers: every wave reads the same value before thread 0 may reset it
        __syncthreads();
        const int nc = ncand;
        __syncthreads();
        if (nc) {   // (uniform)
            if (tid == 0) {
                for (int q = 0; q < nc; ++q) {
                    const double dq = cd[q];
                    const int64_t cq = cc[q];
                    if (!r64_before(dq, cq, ld[K - 1], lc[K - 1])) continue;
                    int p = K - 1;
                    while (p > 0 && r64_before(dq, cq, ld[p - 1], lc[p - 1])) { ld[p] = ld[p - 1]; lc[p] = lc[p - 1]; --p; }
                    ld[p] = dq; lc[p] = cq;
                }
                ncand = 0;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    const int kk = a.self + K;
    if (tid < K) {
        const bool ok = lc[tid] != R64_ID_NONE;
        a.oidx[(size_t)loc * kk + a.self + tid] = ok ? lc[tid] : -1;
        a.odist[(size_t)loc * kk + a.self + tid] = ok ? sqrt(ld[tid]) : INFINITY;
    }
    if (a.self && tid == 0) { a.oidx[(size_t)loc * kk] = g; a.odist[(size_t)loc * kk] = 0.0; }
}

// ------------------------------------------------------------------------------------------------------------ host side
// re-rank (+ guard + repair when `exact`) of the lists in a: results in s->emit_idx / s->emit_dist, [n_rows][self + Kout]
static int r64_run(annchor_ctx *c, StreamState *s, R64Args &a, int dim_padded)
{
    ANN_REQUIRE(c, a.Kp >= 1 && a.Kp <= R64_KMAX && a.Kout >= 1 && a.Kout <= R64_KMAX && a.dim <= R64_MAXDIM, ANNCHOR_ELIMIT,
                "float64 re-rank: %d listed, %d kept entries, %d dimensions", a.Kp, a.Kout, a.dim);
    const int kk = a.self + a.Kout;
    const int64_t ntile = (a.rows + ST_T - 1) / ST_T;
    ANN_TRY(ann_stream_reserve(c, s->emit_idx, sizeof(int64_t) * (size_t)a.n_rows * kk));
    ANN_TRY(ann_stream_reserve(c, s->emit_dist, sizeof(double) * (size_t)a.n_rows * kk));
    // (the counter sits behind the flag words, 8-byte aligned)
    const size_t cnt_off = (sizeof(uint32_t) * 4 * (size_t)ntile + 7) & ~(size_t)7;
    ANN_TRY(ann_stream_reserve(c, s->g64_tiles, cnt_off + 8));
    ANN_CHECK_HIP(c, hipMemsetAsync(s->g64_tiles.p, 0, cnt_off + 8, c->stream));
    a.oidx = s->emit_idx.as<int64_t>(); a.odist = s->emit_dist.as<double>();
    a.flags = s->g64_tiles.as<uint32_t>();
    a.nflag = reinterpret_cast<unsigned long long *>(s->g64_tiles.as<char>() + cnt_off);
    a.gamma32 = (double)(dim_padded + 4) * 0x1p-24;
    a.gamma64 = (double)(dim_padded + 4) * 0x1p-52;
    const bool vec = (a.dim & 1) == 0;   // (rows of an even dimension start on 16-byte boundaries)
    s->last_flagged64 = 0;
    s->last_repaired64 = false;
    {
        ProfScope ps(c, "stream_rerank64", (double)a.rows * a.Kp * a.dim * 8.0);
        const unsigned grid = (unsigned)((a.rows + 3) / 4);
        if (vec) k_r64_rerank<true><<<grid, 256, 0, c->stream>>>(a);
        else k_r64_rerank<false><<<grid, 256, 0, c->stream>>>(a);
        ANN_CHECK_HIP(c, hipGetLastError());
    }
    if (!a.exact) return ANNCHOR_OK;
    unsigned long long flagged = 0;
    ANN_TRY(ann_d2h(c, &flagged, a.nflag, 8));
    s->last_flagged64 = (int64_t)flagged;
    if (flagged == 0) return ANNCHOR_OK;
    if ((int64_t)flagged > std::max<int64_t>(8, a.n_rows / 200))
        fprintf(stderr, "annchor: float64 re-rank: %llu of %lld rows have a list boundary the float32 copy cannot decide; they are "
                        "evaluated again against every row by float64 differences (exact, slower)\n", flagged, (long long)a.n_rows);
    const int64_t cap = std::min<int64_t>((int64_t)flagged, a.rows);
    ANN_TRY(ann_stream_reserve(c, s->g64_list, sizeof(uint32_t) * (size_t)(cap + 1)));
    uint32_t *cnt = s->g64_list.as<uint32_t>(), *list = cnt + 1;
    ANN_CHECK_HIP(c, hipMemsetAsync(cnt, 0, sizeof(uint32_t), c->stream));
    const int64_t nwords = ntile * 4;
    ProfScope ps(c, "stream_repair64", (double)cap * a.n_cols * a.dim * 8.0);
    k_r64_list<<<ann_blocks(nwords, 256), 256, 0, c->stream>>>(a.flags, nwords, list, cnt, (uint32_t)cap);
    if (vec) k_r64_repair<true><<<(unsigned)cap, 256, 0, c->stream>>>(a, list, cnt);
    else k_r64_repair<false><<<(unsigned)cap, 256, 0, c->stream>>>(a, list, cnt);
    ANN_CHECK_HIP(c, hipGetLastError());
    s->last_repaired64 = true;
    return ANNCHOR_OK;
}

extern "C" int annchor_stream_bind_f64(annchor_ctx *c, const double *X, int64_t n_local, int32_t dim, int64_t global_base,
                                       const double *centre_in, double *centre_out, void **rows64)
{
    if (!c || !X) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, n_local >= 1 && n_local < (1ll << 31), ANNCHOR_ELIMIT, "n_local=%lld out of range", (long long)n_local);
    ANN_REQUIRE(c, dim >= 1 && ann_stream_padded_dim(dim) > 0, ANNCHOR_ELIMIT, "streamed form supports dim <= 1024 (got %d)", dim);
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    StreamState *s = ann_stream_state(c, true);
    const size_t n = (size_t)n_local;
    ANN_TRY(ann_stream_reserve(c, s->X64, sizeof(double) * n * dim));
    ANN_TRY(ann_stream_reserve(c, s->e64, sizeof(float) * n));
    ANN_TRY(ann_stream_reserve(c, s->centre64, sizeof(double) * dim));
    ANN_TRY(ann_stream_reserve(c, s->X, sizeof(float) * n * dim));
    ANN_TRY(ann_h2d(c, s->X64.p, X, sizeof(double) * n * dim));
    if (centre_in) {
        ANN_TRY(ann_h2d(c, s->centre64.p, centre_in, sizeof(double) * dim));
    } else {
        const int nblk = (int)std::min<int64_t>(1024, (n_local + 63) / 64);
        const int64_t rpb = (n_local + nblk - 1) / nblk;
        ANN_TRY(ann_stream_reserve(c, s->part64, sizeof(double) * (size_t)nblk * dim));
        ProfScope ps(c, "stream_bind64_centre", (double)n * dim * 8.0);
        k_r64_colsum<<<nblk, 256, 0, c->stream>>>(s->X64.as<double>(), n_local, dim, rpb, s->part64.as<double>());
        k_r64_centre<<<ann_blocks(dim, 256), 256, 0, c->stream>>>(s->part64.as<double>(), nblk, dim, n_local, s->centre64.as<double>());
        ANN_CHECK_HIP(c, hipGetLastError());
    }
    {
        ProfScope ps(c, "stream_bind64_narrow", (double)n * dim * 12.0);
        k_r64_narrow<<<(unsigned)((n_local + 3) / 4), 256, 0, c->stream>>>(s->X64.as<double>(), s->centre64.as<double>(), n_local, dim,
                                                                           s->X.as<float>(), s->e64.as<float>());
        ANN_CHECK_HIP(c, hipGetLastError());
    }
    // the rest is annchor_stream_bind's, on the float32 copy the kernel just wrote (a device-to-device copy onto itself is skipped)
    ANN_TRY(annchor_stream_bind(c, s->X.as<float>(), n_local, dim, global_base, 1));
    s->bound64 = true;
    if (centre_out) ANN_TRY(ann_d2h(c, centre_out, s->centre64.p, sizeof(double) * dim));
    if (rows64) *rows64 = s->X64.p;
    return ANNCHOR_OK;
}

extern "C" int annchor_stream_rerank64(annchor_ctx *c, int32_t k, int64_t *ng_idx, double *ng_dist)
{
    if (!c || !ng_idx || !ng_dist) return ANNCHOR_EINVAL;
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    StreamState *s = ann_stream_state(c, false);
    ANN_REQUIRE(c, s && s->run && s->run_finished, ANNCHOR_ESTATE, "annchor_stream_knn_run not called");
    ANN_REQUIRE(c, s->bound64, ANNCHOR_ESTATE, "the rows were not bound with annchor_stream_bind_f64");
    const KnnArgs &ka = *s->run;
    ANN_REQUIRE(c, ka.tile_begin == 0 && ka.tile_count == ka.nt_all, ANNCHOR_EINVAL, "the float64 re-rank needs every row's list on one rank");
    ANN_REQUIRE(c, k >= 2 && k - 1 <= ka.K, ANNCHOR_EINVAL, "n_neighbors = %d of lists of %d", k, ka.K + 1);
    R64Args a;
    a.Xr = a.Xc = s->X64.as<double>(); a.er = s->e64.as<float>();
    a.perm_r = (const int64_t *)s->run_perm; a.rows = (int64_t)ka.tile_count * ST_T;
    a.n_rows = a.n_cols = s->n_local; a.base_r = a.base_c = s->base;
    a.dim = s->dim; a.Kp = ka.K; a.Kout = k - 1; a.self = 1;
    a.cidx = s->fin_idx; a.cdist = s->fin_dist;
    a.exact = (ka.max_tiles >= ka.nt_all && ka.early_window == 0) ? 1 : 0;
    int rc = r64_run(c, s, a, s->run_dimp);
    if (rc == ANNCHOR_OK) rc = ann_d2h(c, ng_idx, s->emit_idx.p, sizeof(int64_t) * (size_t)s->n_local * k);
    if (rc == ANNCHOR_OK) rc = ann_d2h(c, ng_dist, s->emit_dist.p, sizeof(double) * (size_t)s->n_local * k);
    ann_stream_free_run(s);
    return rc;
}

extern "C" int annchor_stream_query64(annchor_ctx *c, const void *Xs_all, const void *rs_all, const void *perm_all, const void *lo_all,
                                      const void *hi_all, const void *mid_all, int64_t n_all, int32_t nt_all, int32_t n_anchors,
                                      int32_t dim_padded, int32_t nn, int32_t nn_search, double p_work, const void *rows64_data,
                                      int64_t n_data, int64_t data_base, int64_t *out_idx, double *out_dist, int64_t *tile_evals)
{
    if (!c || !rows64_data || !out_idx || !out_dist) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, nn >= 1 && nn_search >= nn && n_data >= 1, ANNCHOR_EINVAL, "nn = %d of %d searched, %lld data rows", nn, nn_search, (long long)n_data);
    StreamState *s = ann_stream_state(c, false);
    ANN_REQUIRE(c, s && s->bound64, ANNCHOR_ESTATE, "the queries were not bound with annchor_stream_bind_f64");
    KnnArgs ka;
    int64_t *d_idx = nullptr;
    float *d_dist = nullptr;
    ANN_TRY(ann_stream_query_search(c, Xs_all, rs_all, perm_all, lo_all, hi_all, mid_all, n_all, nt_all, n_anchors, dim_padded, nn_search,
                                    p_work, ka, &d_idx, &d_dist, tile_evals));
    R64Args a;
    a.Xr = s->X64.as<double>(); a.er = s->e64.as<float>();
    a.perm_r = s->perm.as<int64_t>(); a.rows = (int64_t)s->nt * ST_T; a.n_rows = s->n_local; a.base_r = 0;
    a.Xc = (const double *)rows64_data; a.n_cols = n_data; a.base_c = data_base;
    a.dim = s->dim; a.Kp = nn_search; a.Kout = nn; a.self = 0;
    a.cidx = d_idx; a.cdist = d_dist;
    a.exact = ka.max_tiles >= ka.nt_all ? 1 : 0;
    ANN_TRY(r64_run(c, s, a, dim_padded));
    ANN_TRY(ann_d2h(c, out_idx, s->emit_idx.p, sizeof(int64_t) * (size_t)s->n_local * nn));
    return ann_d2h(c, out_dist, s->emit_dist.p, sizeof(double) * (size_t)s->n_local * nn);
}

extern "C" int annchor_stream_last_rerank64(annchor_ctx *c, int64_t *flagged_rows, int32_t *repaired)
{
    if (!c || !flagged_rows || !repaired) return ANNCHOR_EINVAL;
    StreamState *s = ann_stream_state(c, false);
    ANN_REQUIRE(c, s, ANNCHOR_ESTATE, "no streamed build on this context");
    *flagged_rows = s->last_flagged64;
    *repaired = s->last_repaired64 ? 1 : 0;
    return ANNCHOR_OK;
}
