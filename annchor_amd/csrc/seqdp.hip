// seqdp.hip -- the seven sequence measures with a dynamic programme over the pair's cost matrix, over a pair list: dynamic time
// warping between series, the discrete Frechet distance between curves, the edit distance with real penalty (ERP),
// Move-Split-Merge (MSM), the time warp edit distance (TWE), the edit distance on real sequences (EDR) and the
// longest-common-subsequence distance (LCSS) between series (no reference counterpart: the reference bundles no sequence
// measure; its is_metric=False switch exists for measures like DTW).  A member is 1 .. L points of `dim` coordinates
// (MSM: dim 1; the others: dim in 1 .. 4); all arithmetic is float64 (float32 input widens exactly).
//
//   c(i, j) = sum over k = 0 .. dim-1, in that order, of t_k * t_k,  t_k = x[i][k] - y[j][k]
//             (every subtraction, product and addition rounded on its own: -ffp-contract=off, never an fma;
//              the sum starts from the k = 0 product, not from 0.0 + ...)
//
//   DTW      D(i, j) = c(i, j) + min(D(i-1, j), D(i, j-1), D(i-1, j-1)),   D(-1, -1) = 0, +inf outside the matrix
//            window >= 0: cells with |i - j| > max(window, |n - m|) are +inf
//            dtw(x, y) = sqrt(D(n-1, m-1)), correctly rounded
//   Frechet  F(i, j) = max(c(i, j), min(F(i-1, j), F(i, j-1), F(i-1, j-1))),   F(-1, -1) = 0, +inf outside the matrix
//            frechet(x, y) = sqrt(F(n-1, m-1)), correctly rounded
//
// max and min are exact and every cell has fixed operands, so a cell holds the same bits under any evaluation order: the kernel
// equals the sequential double loop bit for bit.  (x - y)^2 = (y - x)^2 exactly and the order of k is fixed, so the transposed
// matrix has the same cells and the kernel is free to put the LONGER member of a pair on the lanes.  Frechet has no window: a
// banded Frechet distance loses the triangle inequality, which is the reason to have that metric.
//
//   ERP      g the gap value, a finite float64 scalar; the gap point is (g, ..., g)
//            dist(a, b)  dim 1:   |a[0] - b[0]|
//                        dim > 1: sqrt( sum over k = 0 .. dim-1, in that order, of t_k * t_k ),  t_k = a[k] - b[k],  correctly rounded sqrt
//                        (every subtraction, product and addition rounded on its own, never an fma; the sum starts from the k = 0 product)
//            gx(i) = dist(x[i], gap point)        gy(j) = dist(y[j], gap point)
//            E(-1, -1) = 0     E(i, -1) = E(i-1, -1) + gx(i)     E(-1, j) = E(-1, j-1) + gy(j)        (left to right, one addition per step)
//            E(i, j) = min( E(i-1, j-1) + dist(x[i], y[j]),   E(i-1, j) + gx(i),   E(i, j-1) + gy(j) )
//            erp(x, y) = E(n-1, m-1)                                                                    (no square root at the end)
//
// ERP's cells are the min of three sums of fixed operands: min is exact and the additions commutative, so again any evaluation
// order gives the same bits, and dist is symmetric bit for bit, so the transposed matrix holds the same cells.  Its row -1 and
// column -1 are not +inf but running sums of gap costs.  A running sum is a left-to-right float sum, which no scan across lanes
// reproduces: the loader (ctx.hip) computes them once per data set, sequentially, into `gapsum` -- shaped like the pool,
// gapsum[off + i] = E(i, -1) of that member -- and the kernel only loads them.  ERP has no band either, for Frechet's reason.
//
// MSM and TWE read the PREVIOUS points x[i-1] and y[j-1] as well.  Both share one boundary: T(-1, -1) = 0, T(i, -1) = T(-1, j) =
// +inf, and the virtual previous points x[-1] and y[-1] are the origin (they only ever meet +inf or each other).
//
//   MSM      dim 1, c the cost of a split or merge, finite, > 0
//            C(v, a, b) = c                              if a <= v <= b or a >= v >= b
//                       = c + min(|v - a|, |v - b|)      otherwise
//            M(i, j) = min( M(i-1, j-1) + |x[i] - y[j]|,   M(i-1, j) + C(x[i], x[i-1], y[j]),   M(i, j-1) + C(y[j], x[i], y[j-1]) )
//            msm(x, y) = M(n-1, m-1)
//   TWE      nu >= 0 the stiffness, lam >= 0 the penalty of a delete, both finite; point i has time i + 1; dist is ERP's;
//            nl = nu + lam and nu2 = 2.0 * nu are formed once on the host
//            dx(i) = dist(x[i], x[i-1]) + nl        dy(j) = dist(y[j], y[j-1]) + nl
//            T(i, j) = min( T(i-1, j-1) + ((dist(x[i], y[j]) + dist(x[i-1], y[j-1])) + nu2 * (double)|i - j|),
//                           T(i-1, j) + dx(i),   T(i, j-1) + dy(j) )
//            twe(x, y) = T(n-1, m-1)
//
// Their cells are again the min of three sums of fixed operands, C is symmetric in (a, b), dist and |i - j| are symmetric: the same
// bits under any evaluation order and in the transposed matrix.  Neither has a band, for Frechet's reason.
//
// EDR and LCSS count instead of summing distances; eps >= 0 is the matching threshold, finite.
//
//   match(p, q) iff fabs(p[k] - q[k]) <= eps for every k = 0 .. dim-1      (each subtraction rounded on its own; no products)
//   EDR      E(-1, -1) = 0     E(i, -1) = i + 1     E(-1, j) = j + 1
//            E(i, j) = min( E(i-1, j-1) + (match(x[i], y[j]) ? 0.0 : 1.0),   E(i-1, j) + 1.0,   E(i, j-1) + 1.0 )
//            edr(x, y) = E(n-1, m-1), divided by (double)max(n, m) if `normalize`
//   LCSS     delta < 0: none.  L(-1, -1) = L(i, -1) = L(-1, j) = 0
//            L(i, j) = L(i-1, j-1) + 1.0 if match(x[i], y[j]) and (delta < 0 or |i - j| <= delta), else max(L(i-1, j), L(i, j-1))
//            lcss(x, y) = 1.0 - L(n-1, m-1) / (double)min(n, m)
//
// Every cell is an integer of at most 4096, exact in float64: the same bits under any evaluation order and in the transposed
// matrix (fabs(p - q) = fabs(q - p)).  Their edges are counts, which the kernel computes where ERP loads `gapsum` (Op::thresh):
// EDR's column -1 of row i is (double)(i + 1) and lane 0's row -1 at step s is (double)(s + 1); LCSS starts from 0.0 wherever
// the others start from +inf.  LCSS's delta is tested on the i - j the band forms and rides SeqArgs::window; it is never widened
// to n - m.  The division happens in the store: results go straight to the pipeline's buffers.
//
// k_seqdp<T, DIM, R, G, Op>: one pair per group of G lanes, 64 / G pairs per wavefront.  Lane l of a group keeps rows
// l R .. l R + R - 1 of its pair: their R DIM coordinates of x and the R cells of the column it worked on last.  At step s it
// works on column s - l: the current point of y (DIM doubles) moves down the lanes one lane per step by DPP wave_shr:1 -- two
// 32-bit moves per double, which cross the 16-lane rows by themselves -- so a group sweeps anti-diagonals, and the bottom cell of
// lane l - 1 is the top boundary of lane l one step later (and its diagonal boundary the step after).  Lane 0 of a group
// overwrites what it receives from the group above; it is fed from a strip of G points of y (one per lane, loaded a block of G
// steps ahead) that moves UP the lanes by wave_shl:1.  Op is the cell: the recurrence's expression, whether it has a band, and
// whether it is ERP's (Op::erp; everything under it compiles away for the other two).  Under ERP a lane also keeps the R gap costs
// of its rows, computes its column's gap cost once per step from the point of y it holds, starts its cells from the rows' entries
// of `gapsum` (column -1) and its bottom cell from the last of them (the diagonal boundary of the lane below at its column 0);
// lane 0's row -1 rides the strip as one more double: E(-1, s) is its top boundary at step s and, a step later, its diagonal one.
// Under Op::prev (MSM, TWE; everything under it compiles away for the other three) a lane also holds the point above its first
// row, x[l R - 1] (lane 0: the origin), loaded once per pair, and the previous column's point: the value its point of y had before
// this step's move down the lanes, which is y[jc - 1] because a lane advances one column per step, and which starts as the origin.
// No cross-lane traffic is added.  TWE's dist(x[i-1], y[j-1]) is what row r - 1 computed one step earlier: a lane carries the R
// distances of its last step (and its rows' dx) in registers, except at dim 1 on the widest shape, where it recomputes them.
// No LDS, no barriers, no atomics; waves take pairs grid-stride; results leave by plain vector stores.  Work per pair:
// (m + ceil(n / R) - 1) steps of R cells, 3 DIM + 2 float64 operations per cell (ERP: 6 at dim 1, 3 DIM + 4 and a square root beyond;
// MSM: 17 -- two subtractions, five additions, four min and six max; TWE: 10 at dim 1, 3 DIM + 8 and a square root beyond).
#include "pairkern.h"

#define DTW_MAXLEN 2048

template <typename T> struct SeqArgs : PairArgs {
    const T *val;
    const int32_t *off, *len;   // counted in points
    int window;                 // DTW's band; LCSS's delta (-1: none); others: unused
    const double *gapsum;       // ERP: [points of the pool] running sums of gap costs, E(i, -1) of each member; others: unused
    double gap;                 // ERP: the gap value
    double msm_c;               // MSM: the cost of a split or merge
    double twe_nl, twe_nu2;     // TWE: nu + lam and 2 nu
    double eps;                 // EDR, LCSS: the matching threshold, per coordinate
    int normalize;              // EDR: whether the store divides by the longer member's length
};

// An Op is the cell and, as compile-time traits, what its launch needs: `profile`, the profile scope's name; `max_dim`, the
// largest dim (1: univariate members, whatever curve_dim holds); max_len(dim), the longest member its widest shape takes;
// point_bytes(dim, elem), what a point costs to read (the profile's traffic figure); `member`, the noun of its refusals.  Op::erp
// also says that `gapsum` must be bound.
template <bool BAND> struct DtwOp {
    static constexpr bool band = BAND, erp = false, prev = false, msm = false, thresh = false, lcss = false;
    static constexpr const char *profile = "dtw_pairs", *member = "series";
    static constexpr int max_dim = 4;
    static constexpr int max_len(int dim) { return (dim <= 2 ? 32 : 16) * 64; }
    static constexpr size_t point_bytes(int dim, size_t elem) { return dim * elem; }
    static __device__ __forceinline__ double cell(double cost, double left, double up, double dg) { return cost + fmin(fmin(left, up), dg); }
};
struct FrechetOp {
    static constexpr bool band = false, erp = false, prev = false, msm = false, thresh = false, lcss = false;
    static constexpr const char *profile = "frechet_pairs", *member = "curve";
    static constexpr int max_dim = 4;
    static constexpr int max_len(int dim) { return (dim <= 2 ? 32 : 16) * 64; }
    static constexpr size_t point_bytes(int dim, size_t elem) { return dim * elem; }
    static __device__ __forceinline__ double cell(double cost, double left, double up, double dg) { return fmax(cost, fmin(fmin(left, dg), up)); }
};
// (its cell takes the three neighbours with their three costs already added)
struct ErpOp {
    static constexpr bool band = false, erp = true, prev = false, msm = false, thresh = false, lcss = false;
    static constexpr const char *profile = "erp_pairs", *member = "series";
    static constexpr int max_dim = 4;
    static constexpr int max_len(int dim) { return (dim == 1 ? 32 : 16) * 64; }
    static constexpr size_t point_bytes(int dim, size_t elem) { return dim * elem + sizeof(double); }   // (and its entry of gapsum)
    static __device__ __forceinline__ double cell(double match, double gap_row, double gap_col) { return fmin(fmin(match, gap_row), gap_col); }
};

// MSM and TWE: the cell reads x[i-1] and y[j-1] (Op::prev); `msm` tells the two apart.  MSM's C(v, a, b) from the two differences
// da = v - a and db = v - b, without a comparison: with lo = min(da, db) and hi = max(da, db), v lies outside [a, b] iff lo > 0
// (then min(|da|, |db|) = lo) or hi < 0 (then it is -hi), and max(lo, -hi) <= 0 iff v lies between them.  So
// C = c + max(max(lo, -hi), 0.0): the definition's sum outside, and c + 0.0 = c bit for bit between them.  A float64 difference is
// zero only for equal operands, so every tie (v == a, v == b, a == b) has lo <= 0 <= hi, the definition's first case.
struct MsmOp {
    static constexpr bool band = false, erp = false, prev = true, msm = true, thresh = false, lcss = false;
    static constexpr const char *profile = "msm_pairs", *member = "series";
    static constexpr int max_dim = 1;
    static constexpr int max_len(int) { return DTW_MAXLEN; }
    static constexpr size_t point_bytes(int, size_t elem) { return elem; }
    static __device__ __forceinline__ double cost(double da, double db, double c)
    {
        return c + fmax(fmax(fmin(da, db), -fmax(da, db)), 0.0);
    }
    static __device__ __forceinline__ double cell(double match, double up, double left) { return fmin(fmin(match, up), left); }
};
struct TweOp {
    static constexpr bool band = false, erp = false, prev = true, msm = false, thresh = false, lcss = false;
    static constexpr const char *profile = "twe_pairs", *member = "series";
    static constexpr int max_dim = 4;
    static constexpr int max_len(int dim) { return (dim == 1 ? 32 : 16) * 64; }
    static constexpr size_t point_bytes(int dim, size_t elem) { return dim * elem; }
    static __device__ __forceinline__ double cell(double match, double up, double left) { return fmin(fmin(match, up), left); }
};

// EDR and LCSS (Op::thresh; `lcss` tells the two apart): the cell takes `hit`, whether the two points match, and for LCSS whether
// |i - j| is within delta as well.  Their cells are counts, and so are their edges, which the kernel computes: no pool array.
struct EdrOp {
    static constexpr bool band = false, erp = false, prev = false, msm = false, thresh = true, lcss = false;
    static constexpr const char *profile = "edr_pairs", *member = "series";
    static constexpr int max_dim = 4;
    static constexpr int max_len(int dim) { return (dim <= 2 ? 32 : 16) * 64; }
    static constexpr size_t point_bytes(int dim, size_t elem) { return dim * elem; }
    static __device__ __forceinline__ double cell(bool hit, double left, double up, double dg)
    {
        return fmin(fmin(dg + (hit ? 0.0 : 1.0), up + 1.0), left + 1.0);
    }
};
struct LcssOp {
    static constexpr bool band = false, erp = false, prev = false, msm = false, thresh = true, lcss = true;
    static constexpr const char *profile = "lcss_pairs", *member = "series";
    static constexpr int max_dim = 4;
    static constexpr int max_len(int dim) { return (dim <= 2 ? 32 : 16) * 64; }
    static constexpr size_t point_bytes(int dim, size_t elem) { return dim * elem; }
    static __device__ __forceinline__ double cell(bool hit, double left, double up, double dg) { return hit ? dg + 1.0 : fmax(up, left); }
};

// TWE's dist between two points (the same arithmetic as ERP's, which the kernel's cell loop spells out)
template <int DIM> __device__ __forceinline__ double point_dist(const double (&p)[DIM], const double (&q)[DIM])
{
    double df = p[0] - q[0];
    if (DIM == 1) return fabs(df);
    double c = df * df;
#pragma unroll
    for (int k = 1; k < DIM; ++k) {
        df = p[k] - q[k];
        c = c + df * df;
    }
    return __dsqrt_rn(c);
}

// ERP's dist(p, gap point)
template <int DIM> __device__ __forceinline__ double erp_gap_cost(const double (&p)[DIM], double g)
{
    double df = p[0] - g;
    if (DIM == 1) return fabs(df);
    double c = df * df;
#pragma unroll
    for (int k = 1; k < DIM; ++k) {
        df = p[k] - g;
        c = c + df * df;
    }
    return __dsqrt_rn(c);
}

template <typename T, int DIM, int R, int G, typename Op> __global__ __launch_bounds__(PAIR_THREADS) void k_seqdp(SeqArgs<T> a)
{
    constexpr int PPW = ANN_WAVE / G;   // pairs per wavefront
    const int lane = threadIdx.x & (ANN_WAVE - 1), gl = lane & (G - 1), slot = lane / G;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / ANN_WAVE;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / ANN_WAVE;
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    const double OUT = Op::lcss ? 0.0 : INF;   // outside the matrix: +inf; LCSS: a count of 0
    for (int64_t base = wave * PPW; base < a.n; base += nwaves * PPW) {   // (wave-uniform: the DPP moves run with every lane on)
        const int64_t t = base + slot;
        const PairSlot ps = pair_decode(a, t);
        const bool active = ps.active;
        const int i = ps.i, j = ps.j;
        const int64_t opos = ps.opos;
        int n = a.len[i], m = a.len[j];
        const T *x = a.val + (int64_t)a.off[i] * DIM, *y = a.val + (int64_t)a.off[j] * DIM;
        const double *gsx = nullptr, *gsy = nullptr;   // ERP: E(., -1) of the member on the lanes, E(-1, .) of the other
        if constexpr (Op::erp) { gsx = a.gapsum + a.off[i]; gsy = a.gapsum + a.off[j]; }
        if (n < m) {   // the longer member on the lanes
            const T *p = x; x = y; y = p; const int k = n; n = m; m = k;
            if constexpr (Op::erp) { const double *q = gsx; gsx = gsy; gsy = q; }
        }
        // (LCSS: delta is plain, never widened to n - m; none: every |i - j| is within it)
        const int w = Op::band ? max(a.window, n - m) : Op::lcss ? (a.window < 0 ? 0x7fffffff : a.window) : 0;
        // ERP keeps the R gap costs of its rows, except at dim 1 on the widest shape: there a gap cost is one subtraction, and
        // 32 more doubles would put the lane's state at 192 VGPRs and the kernel beyond the 256 a wave can address directly
        constexpr bool KEEP_GX = Op::erp && !(DIM == 1 && R > 16);
        // TWE keeps dx of its R rows (in gxr) and the R distances of its last step under the same rule: at dim 1 each is a subtraction
        constexpr bool TWE = Op::prev && !Op::msm, KEEP_TW = TWE && !(DIM == 1 && R > 16);
        double xr[R][DIM], d[R], gxr[KEEP_GX || KEEP_TW ? R : 1];
        double xab[DIM], pd[KEEP_TW ? R : 1];    // Op::prev: the point above the lane's first row; TWE: dist(x[row], y[jc - 1])
        if constexpr (Op::prev) {
            const T *xp = x + (int64_t)min(max(gl * R - 1, 0), n - 1) * DIM;
#pragma unroll
            for (int k = 0; k < DIM; ++k) xab[k] = gl == 0 ? 0.0 : (double)xp[k];   // (lane 0: x[-1], the origin)
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int row = min(gl * R + r, n - 1);                    // (rows >= n: cells nobody reads)
            const T *xp = x + (int64_t)row * DIM;
#pragma unroll
            for (int k = 0; k < DIM; ++k) xr[r][k] = (double)xp[k];
            if constexpr (Op::erp) {
                if constexpr (KEEP_GX) gxr[r] = erp_gap_cost<DIM>(xr[r], a.gap);
                d[r] = gsx[row];                                       // column -1: E(row, -1)
            } else if constexpr (Op::thresh && !Op::lcss)
                d[r] = (double)(row + 1);                              // column -1: EDR's E(row, -1), row + 1 deletions
            else
                d[r] = OUT;                                            // column -1
            if constexpr (KEEP_TW) {
                gxr[r] = point_dist<DIM>(xr[r], r == 0 ? xab : xr[r > 0 ? r - 1 : 0]) + a.twe_nl;   // dx(row)
                double org[DIM];
#pragma unroll
                for (int k = 0; k < DIM; ++k) org[k] = 0.0;
                pd[r] = point_dist<DIM>(xr[r], org);                   // dist(x[row], y[-1]): what column 0 of row + 1 reads
            }
        }
        int steps = m + (n - 1) / R;   // the lane of row n - 1 works on column m - 1 at step m - 1 + (n - 1) / R
#pragma unroll
        for (int o = G; o < ANN_WAVE; o <<= 1) steps = max(steps, __shfl_xor(steps, o));
        double ycur[DIM], ynext[DIM], ybuf[DIM], yprev[DIM];   // yprev (Op::prev): y[jc - 1]
        // Op::prev, per step: MSM's y[jc] - y[jc - 1]; TWE's dist(x[i-1], y[jc-1]) on its way down the lane's rows, and l R - jc.
        // (Declared here and not in the step loop: there, though unused, they reorder two moves in the other measures' prologues.)
        double ydf = 0.0, carry = 0.0, e0 = 0.0;
        double gnext = 0.0, gbuf = 0.0;          // ERP: the strip's E(-1, .), beside its points of y
        double bottom = OUT;
        if constexpr (Op::thresh) bottom = d[R - 1];   // EDR: E(l R + R - 1, -1), as under ERP
        if constexpr (Op::erp) {
            bottom = d[R - 1];                   // E(l R + R - 1, -1): the lane below takes it as its diagonal boundary at column 0
            gnext = gsy[min(gl, m - 1)];
        }
        double top_prev = gl == 0 ? 0.0 : OUT;   // lane 0's diagonal boundary at column 0 is the cell (-1, -1) = 0
#pragma unroll
        for (int k = 0; k < DIM; ++k) {
            ycur[k] = 0.0;
            ynext[k] = (double)y[(int64_t)min(gl, m - 1) * DIM + k];
        }
        for (int s0 = 0; s0 < steps; s0 += G) {
            const T *yp = y + (int64_t)min(s0 + G + gl, m - 1) * DIM;
#pragma unroll
            for (int k = 0; k < DIM; ++k) {
                ybuf[k] = ynext[k];            // y[s0 + gl]
                ynext[k] = (double)yp[k];      // the next block's, on its way while this block runs
            }
            if constexpr (Op::erp) {
                gbuf = gnext;                  // E(-1, s0 + gl)
                gnext = gsy[min(s0 + G + gl, m - 1)];
            }
            const int s1 = min(s0 + G, steps);
            for (int s = s0; s < s1; ++s) {
                double top = lane_down(bottom);
#pragma unroll
                for (int k = 0; k < DIM; ++k) {
                    if constexpr (Op::prev) yprev[k] = ycur[k];    // y[jc - 1]; at jc = 0 the 0.0 that ycur started from
                    const double yv = lane_down(ycur[k]);
                    ycur[k] = gl == 0 ? ybuf[k] : yv;              // lane 0: y[s]
                    ybuf[k] = lane_up(ybuf[k]);
                }
                if constexpr (Op::erp) {
                    if (gl == 0) top = gbuf;                       // row -1: E(-1, s)
                    gbuf = lane_up(gbuf);
                } else if constexpr (Op::thresh && !Op::lcss) {
                    if (gl == 0) top = (double)(s + 1);            // row -1: EDR's E(-1, s), s + 1 insertions
                } else if (gl == 0)
                    top = OUT;                                     // row -1
                const double diag = top_prev;
                top_prev = top;
                const int jc = s - gl;                             // this lane's column
                if (jc >= 0 && jc < m) {
                    double up = top, dg = diag;
                    double gy = 0.0;
                    if constexpr (Op::erp) gy = erp_gap_cost<DIM>(ycur, a.gap);
                    if constexpr (TWE) {
                        gy = point_dist<DIM>(ycur, yprev) + a.twe_nl;            // dy(jc)
                        if constexpr (KEEP_TW) carry = point_dist<DIM>(xab, yprev);   // row 0 of the lane: dist(x[l R - 1], y[jc - 1])
                        e0 = (double)(gl * R - jc);                              // (small integers: e0 + r is (double)(i - j) exactly)
                    } else if constexpr (Op::prev)
                        ydf = ycur[0] - yprev[0];                                // MSM: y[jc] - y[jc - 1]
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        double df = xr[r][0] - ycur[0];
                        double cost = 0.0;
                        bool hit = true;                           // Op::thresh: match(x[i], y[jc]), a comparison per coordinate
                        if constexpr (Op::thresh) {
                            hit = fabs(df) <= a.eps;
#pragma unroll
                            for (int k = 1; k < DIM; ++k) hit = hit && fabs(xr[r][k] - ycur[k]) <= a.eps;
                            if constexpr (Op::lcss) {
                                const int e = gl * R + r - jc;     // i - j
                                hit = hit && e <= w && e >= -w;
                            }
                        } else {
                            cost = df * df;
#pragma unroll
                            for (int k = 1; k < DIM; ++k) {
                                df = xr[r][k] - ycur[k];
                                cost = cost + df * df;
                            }
                        }
                        const double left = d[r];
                        double v;
                        if constexpr (Op::thresh)
                            v = Op::cell(hit, left, up, dg);
                        else if constexpr (Op::erp) {
                            const double dist = DIM == 1 ? fabs(df) : __dsqrt_rn(cost);
                            const double gx = KEEP_GX ? gxr[r] : erp_gap_cost<DIM>(xr[r], a.gap);
                            v = Op::cell(dg + dist, up + gx, left + gy);
                        } else if constexpr (TWE) {
                            const double(&xp)[DIM] = r == 0 ? xab : xr[r > 0 ? r - 1 : 0];   // x[i - 1]
                            const double dist = DIM == 1 ? fabs(df) : __dsqrt_rn(cost);
                            double dprev, dxi;
                            if constexpr (KEEP_TW) {
                                dprev = carry;                     // what row r - 1 computed one step earlier
                                carry = pd[r];
                                pd[r] = dist;
                                dxi = gxr[r];
                            } else {
                                dprev = point_dist<DIM>(xp, yprev);
                                dxi = point_dist<DIM>(xr[r], xp) + a.twe_nl;
                            }
                            v = Op::cell(dg + ((dist + dprev) + a.twe_nu2 * fabs(e0 + (double)r)), up + dxi, left + gy);
                        } else if constexpr (Op::prev) {
                            const double xdf = xr[r][0] - (r == 0 ? xab[0] : xr[r > 0 ? r - 1 : 0][0]);   // x[i] - x[i - 1]
                            v = Op::cell(dg + fabs(df), up + Op::cost(xdf, df, a.msm_c), left + Op::cost(-df, ydf, a.msm_c));
                        } else
                            v = Op::cell(cost, left, up, dg);
                        if (Op::band) {
                            const int e = gl * R + r - jc;         // i - j
                            if (e > w || e < -w) v = INF;
                        }
                        dg = left;
                        up = v;
                        d[r] = v;
                    }
                    bottom = up;
                }
            }
        }
        double res = INF;
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r == (n - 1) % R) res = d[r];
        if constexpr (Op::lcss)
            res = 1.0 - res / (double)m;                   // (after the swap m = min(n, m))
        else if constexpr (Op::thresh) {
            if (a.normalize) res = res / (double)n;        // (and n = max(n, m))
        }
        if (active && gl == (n - 1) / R) pair_store(a, t, opos, Op::erp || Op::prev || Op::thresh ? res : __dsqrt_rn(res));
    }
}

template <typename T, int DIM, int R, int G, typename Op> static int launch_shape(annchor_ctx *c, const SeqArgs<T> &a)
{
    static_assert(R * DIM <= 64 && R * G <= DTW_MAXLEN && (G & (G - 1)) == 0 && G <= ANN_WAVE,
                  "a lane holds R x DIM coordinates of x, a group R x G rows");
    static_assert(!Op::erp || R * DIM + 2 * R <= 96, "ERP: a lane holds R gap costs as well");
    static_assert(!Op::prev || Op::msm || (DIM == 1 && R > 16) || R * DIM + 3 * R <= 112, "TWE: a lane holds R dx and R distances as well");
    k_seqdp<T, DIM, R, G, Op><<<pair_grid(c, a.n, G), PAIR_THREADS, 0, c->stream>>>(a);
    ANN_CHECK_HIP(c, hipGetLastError());
    return ANNCHOR_OK;
}

// by the data set's longest member: 4 pairs per wavefront up to 128 points, one pair on 64 lanes beyond; the widest shape keeps
// R x DIM <= 64 coordinates of x per lane, hence RW = 32 (2048 points) at dim <= 2 and 16 (1024 points) at dim 3, 4.  ERP keeps
// R gap costs more, R x DIM + 2 R <= 96 doubles with the cells (what Frechet's widest shape holds): RW = 32 at dim 1 only
template <typename T, int DIM, typename Op> static int launch_len(annchor_ctx *c, const SeqArgs<T> &a)
{
    constexpr int RW = DIM <= (Op::erp || Op::prev ? 1 : 2) ? 32 : 16;
    if (c->maxlen <= 8 * 16) return launch_shape<T, DIM, 8, 16, Op>(c, a);
    if (c->maxlen <= 8 * 64) return launch_shape<T, DIM, 8, 64, Op>(c, a);
    return launch_shape<T, DIM, RW, 64, Op>(c, a);
}

template <typename T> static SeqArgs<T> seq_args(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    SeqArgs<T> a;
    pair_fill(a, src, d_out, d_RA, d_ncm);
    a.val = c->sym.as<T>();
    a.off = c->soff.as<int32_t>(); a.len = c->slen.as<int32_t>();
    a.window = c->dtw_window;
    a.gapsum = c->gapsum.as<double>();
    a.gap = c->erp_gap;
    a.msm_c = c->msm_c;
    a.twe_nl = c->twe_nl; a.twe_nu2 = c->twe_nu2;
    a.eps = c->match_eps;
    a.normalize = c->edr_normalize;
    return a;
}

template <typename T, typename Op, int DIM> static int launch_dim(annchor_ctx *c, const SeqArgs<T> &a)
{
    constexpr int limit = Op::max_len(DIM);
    if constexpr (Op::max_dim == 1)
        ANN_REQUIRE(c, c->maxlen >= 1 && c->maxlen <= limit, ANNCHOR_ELIMIT, "series length %d outside 1..%d", c->maxlen, limit);
    else
        ANN_REQUIRE(c, c->maxlen >= 1 && c->maxlen <= limit, ANNCHOR_ELIMIT, "%s length %d outside 1..%d at dim %d", Op::member, c->maxlen,
                    limit, DIM);
    return launch_len<T, DIM, Op>(c, a);
}

// every measure's launch: the Op's traits say what is checked and what the profile records
template <typename T, typename Op> static int launch_measure(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    const SeqArgs<T> a = seq_args<T>(c, src, d_out, d_RA, d_ncm);
    if constexpr (Op::erp) ANN_REQUIRE(c, a.gapsum != nullptr, ANNCHOR_EINVAL, "erp: no gap sums bound to this context");
    const int dim = Op::max_dim == 1 ? 1 : c->curve_dim;
    ProfScope ps(c, Op::profile, (double)src.n * (2.0 * c->maxlen * Op::point_bytes(dim, sizeof(T)) + 16));
    if constexpr (Op::max_dim == 1)   // (no DIM > 1 is instantiated for a univariate measure)
        return launch_dim<T, Op, 1>(c, a);
    else
        switch (dim) {
        case 1: return launch_dim<T, Op, 1>(c, a);
        case 2: return launch_dim<T, Op, 2>(c, a);
        case 3: return launch_dim<T, Op, 3>(c, a);
        case 4: return launch_dim<T, Op, 4>(c, a);
        default: ann_set_err(c, "%s dim %d outside 1..4", Op::member, dim); return ANNCHOR_EINVAL;
        }
}

int ann_seqdp_launch(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    if (src.n == 0) return ANNCHOR_OK;
    switch (c->metric) {
    case ANNCHOR_METRIC_DTW_F32:
        return c->dtw_window >= 0 ? launch_measure<float, DtwOp<true>>(c, src, d_out, d_RA, d_ncm)
                                  : launch_measure<float, DtwOp<false>>(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_DTW_F64:
        return c->dtw_window >= 0 ? launch_measure<double, DtwOp<true>>(c, src, d_out, d_RA, d_ncm)
                                  : launch_measure<double, DtwOp<false>>(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_FRECHET_F32: return launch_measure<float, FrechetOp>(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_FRECHET_F64: return launch_measure<double, FrechetOp>(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_ERP_F32: return launch_measure<float, ErpOp>(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_ERP_F64: return launch_measure<double, ErpOp>(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_MSM_F32: return launch_measure<float, MsmOp>(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_MSM_F64: return launch_measure<double, MsmOp>(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_TWE_F32: return launch_measure<float, TweOp>(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_TWE_F64: return launch_measure<double, TweOp>(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_EDR_F32: return launch_measure<float, EdrOp>(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_EDR_F64: return launch_measure<double, EdrOp>(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_LCSS_F32: return launch_measure<float, LcssOp>(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_LCSS_F64: return launch_measure<double, LcssOp>(c, src, d_out, d_RA, d_ncm);
    default: ann_set_err(c, "no sequence measure bound to this context"); return ANNCHOR_EINVAL;
    }
}
