// dtw.hip -- dynamic time warping between univariate series over a pair list (no reference counterpart: the
// reference bundles no DTW; its is_metric=False switch exists for measures like this one).
//
//   c(i, j) = t * t, t = x_i - y_j                       (two roundings: -ffp-contract=off, never an fma)
//   D(i, j) = c(i, j) + min(D(i-1, j), D(i, j-1), D(i-1, j-1)),   D(-1, -1) = 0, +inf outside the matrix
//   window >= 0: cells with |i - j| > max(window, |n - m|) are +inf
//   dtw(x, y) = sqrt(D(n-1, m-1)), correctly rounded
//
// Every cell has fixed operands and min is exact, so a cell holds the same bits under any evaluation order: the kernel
// equals the sequential double loop bit for bit.  The transposed matrix has the same cells ((x_i - y_j)^2 = (y_j - x_i)^2
// exactly), so the kernel is free to put the LONGER series of a pair on the lanes.
//
// k_dtw<T, R, G, BAND>: one pair per group of G lanes, 64 / G pairs per wavefront.  Lane l of a group keeps rows
// l R .. l R + R - 1 of its pair: their R elements of x and their R cells of the column it worked on last.  At step s it
// works on column s - l: the elements of y move down the lanes one lane per step, so a group sweeps anti-diagonals, and
// the bottom cell of lane l - 1 is the top boundary of lane l one step later (and its diagonal boundary the step after).
// Both travel by DPP wave_shr:1 -- a 64-bit value as two 32-bit moves -- which crosses the 16-lane rows by itself; lane 0
// of a group overwrites what it receives from the group above.  Lane 0 is fed from a strip of G elements of y (one per lane,
// loaded a block of G steps ahead) that moves UP the lanes one lane per step.  No LDS, no barriers, no atomics; waves take
// pairs grid-stride.  Work per pair: (m + ceil(n / R) - 1) steps of R cells, 5 float64 operations per cell.
#include "common.h"

#define DTW_THREADS 256
#define DTW_MAXLEN 2048

template <typename T> struct DtwArgs {
    const T *val;
    const int32_t *off, *len;
    const int2 *ij;
    const int32_t *idx;
    const int32_t *anchor;
    int64_t n;
    int window;
    double *out;
    double *RA;
    uint8_t *ncm;
};

// lane l receives lane l - 1's value; lane 0 of the wavefront keeps its own
__device__ __forceinline__ double dtw_lane_down(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// lane l receives lane l + 1's value; lane 63 keeps its own
__device__ __forceinline__ double dtw_lane_up(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, 0x130, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

template <typename T, int R, int G, bool BAND> __global__ __launch_bounds__(DTW_THREADS) void k_dtw(DtwArgs<T> a)
{
    constexpr int PPW = ANN_WAVE / G;   // pairs per wavefront
    const int lane = threadIdx.x & (ANN_WAVE - 1), gl = lane & (G - 1), slot = lane / G;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / ANN_WAVE;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / ANN_WAVE;
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    for (int64_t base = wave * PPW; base < a.n; base += nwaves * PPW) {   // (wave-uniform: the DPP moves run with every lane on)
        const int64_t t = base + slot;
        const bool active = t < a.n;
        int i = 0, j = 0;
        int64_t opos = t;
        if (active) {
            if (a.anchor) { i = *a.anchor; j = (int)t; }
            else {
                int64_t q = a.idx ? a.idx[t] : t;
                int2 p = a.ij[q];
                i = p.x; j = p.y;
                if (a.idx) opos = q;
            }
        }
        // (a slot past the end of the list works on the pair (0, 0) and stores nothing)
        int n = a.len[i], m = a.len[j];
        const T *x = a.val + a.off[i], *y = a.val + a.off[j];
        if (n < m) { const T *p = x; x = y; y = p; const int k = n; n = m; m = k; }   // the longer series on the lanes
        const int w = BAND ? max(a.window, n - m) : 0;
        double xr[R], d[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            xr[r] = (double)x[min(gl * R + r, n - 1)];   // (rows >= n: cells nobody reads)
            d[r] = INF;                                  // column -1
        }
        int steps = m + (n - 1) / R;   // the lane of row n - 1 works on column m - 1 at step m - 1 + (n - 1) / R
#pragma unroll
        for (int o = G; o < ANN_WAVE; o <<= 1) steps = max(steps, __shfl_xor(steps, o));
        double ycur = 0.0, bottom = INF;
        double top_prev = gl == 0 ? 0.0 : INF;   // lane 0's diagonal boundary at column 0 is D(-1, -1) = 0
        double ynext = (double)y[min(gl, m - 1)];
        for (int s0 = 0; s0 < steps; s0 += G) {
            double ybuf = ynext;                               // y[s0 + gl]
            ynext = (double)y[min(s0 + G + gl, m - 1)];        // the next block's, on its way while this block runs
            const int s1 = min(s0 + G, steps);
            for (int s = s0; s < s1; ++s) {
                double yv = dtw_lane_down(ycur), top = dtw_lane_down(bottom);
                if (gl == 0) { yv = ybuf; top = INF; }         // y[s]; row -1
                ybuf = dtw_lane_up(ybuf);
                ycur = yv;
                const double diag = top_prev;
                top_prev = top;
                const int jc = s - gl;                         // this lane's column
                if (jc >= 0 && jc < m) {
                    double up = top, dg = diag;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const double df = xr[r] - yv;
                        const double left = d[r];
                        double v = df * df + fmin(fmin(left, up), dg);
                        if (BAND) {
                            const int e = gl * R + r - jc;     // i - j
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
        if (active && gl == (n - 1) / R) {
            const double dist = __dsqrt_rn(res);
            if (a.out) a.out[t] = dist;
            if (a.RA) { a.RA[opos] = dist; a.ncm[opos] = 0; }
        }
    }
}

template <typename T, int R, int G> static int launch_shape(annchor_ctx *c, const DtwArgs<T> &a)
{
    static_assert(R * G <= DTW_MAXLEN && (G & (G - 1)) == 0 && G <= ANN_WAVE, "a group holds R x G rows");
    const int64_t waves = (a.n + ANN_WAVE / G - 1) / (ANN_WAVE / G);
    const int64_t cap = (int64_t)c->prop.multiProcessorCount * 64;   // beyond that the waves take further pairs grid-stride
    int64_t blocks = (waves + DTW_THREADS / ANN_WAVE - 1) / (DTW_THREADS / ANN_WAVE);
    if (blocks > cap) blocks = cap;
    if (a.window >= 0) k_dtw<T, R, G, true><<<(int)blocks, DTW_THREADS, 0, c->stream>>>(a);
    else k_dtw<T, R, G, false><<<(int)blocks, DTW_THREADS, 0, c->stream>>>(a);
    ANN_CHECK_HIP(c, hipGetLastError());
    return ANNCHOR_OK;
}

template <typename T> static int launch(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    DtwArgs<T> a;
    a.val = c->sym.as<T>();
    a.off = c->soff.as<int32_t>(); a.len = c->slen.as<int32_t>();
    a.ij = src.ij; a.idx = src.idx; a.anchor = src.anchor; a.n = src.n;
    a.window = c->dtw_window;
    a.out = d_out; a.RA = d_RA; a.ncm = d_ncm;
    ANN_REQUIRE(c, c->maxlen >= 1 && c->maxlen <= DTW_MAXLEN, ANNCHOR_ELIMIT, "series length %d outside 1..%d", c->maxlen, DTW_MAXLEN);
    ProfScope ps(c, "dtw_pairs", (double)src.n * (2.0 * c->maxlen * sizeof(T) + 16));
    // by the data set's longest series: 4 pairs per wavefront up to 128 values, one pair on 64 lanes beyond
    if (c->maxlen <= 8 * 16) return launch_shape<T, 8, 16>(c, a);
    if (c->maxlen <= 8 * 64) return launch_shape<T, 8, 64>(c, a);
    return launch_shape<T, 32, 64>(c, a);
}

int ann_dtw_launch(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    if (src.n == 0) return ANNCHOR_OK;
    return c->metric == ANNCHOR_METRIC_DTW_F32 ? launch<float>(c, src, d_out, d_RA, d_ncm) : launch<double>(c, src, d_out, d_RA, d_ncm);
}
