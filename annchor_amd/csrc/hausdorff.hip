// hausdorff.hip -- Hausdorff distance between point sets over a pair list (no reference counterpart: the reference bundles no
// measure on unordered collections).  A point set is 1 .. 4096 points of `dim` coordinates, with `dim` in 1 .. 4.  All arithmetic
// is float64.  float32 input widens exactly.
//
//   c(i, j)  = sum over k = 0 .. dim-1, in that order, of t_k * t_k,   t_k = x[i][k] - y[j][k]
//              (every subtraction, product and addition rounded on its own: -ffp-contract=off, never an fma;
//               the sum starts from the k = 0 product, not from 0.0 + ...)
//   h(x, y)  = max over i of ( min over j of c(i, j) )          -- directed, x to y
//   hausdorff(x, y) = sqrt( max( h(x, y), h(y, x) ) ), correctly rounded
//
// (x - y)^2 == (y - x)^2 exactly and the order of k is fixed, so c(j, i) computed with the roles swapped has the same bits as
// c(i, j).  min and max are exact and associative: any evaluation order, strip order or lane assignment gives the same bits, and
// hausdorff(x, y) equals hausdorff(y, x) bit for bit.  A duplicated point changes nothing, so rows and columns past the end of a
// set are clamped to the set's last point instead of masked.
//
// k_hausdorff<T, DIM, R, G>: one pair per group of G lanes, 64 / G pairs per wavefront.  A directed pass h(x, y) walks x in strips
// of G R points: lane l of a group keeps points l R .. l R + R - 1 of the strip (R DIM doubles) and their R running minima in
// registers, and the lanes of a group sweep all m points of y together -- at step j every lane of a group reads the same y[j]
// (one address per group, loaded one step ahead; two steps per trip of the loop) and updates its R minima: 3 DIM - 1 operations per cell for the cost and one
// fmin.  After the sweep a lane folds its R minima into a running fmax.  The second pass swaps the roles into the same running
// fmax (max(h(x, y), h(y, x)) is one max over both passes), one cross-lane fmax over the G lanes follows (__shfl_xor on the two
// 32-bit halves), and lane 0 of the group stores the square root.  No LDS, no barriers, no atomics, no length bounded by
// registers; waves take pairs grid-stride; results leave by plain vector stores.  The strip and sweep counts are the largest of the
// wavefront's pairs (clamping makes the surplus harmless), so the loops are wave-uniform.  Work per pair, in cells, clamped ones
// included: ceil(n / (G R)) G R m + ceil(m / (G R)) G R n, which is 2 n m when G R divides both.
#include "pairkern.h"

template <typename T> struct HausdorffArgs : PairArgs {
    const T *val;
    const int32_t *off, *len;   // counted in points
};

__device__ __forceinline__ double haus_xor_max(double v, int o)
{
    const int lo = __shfl_xor(__double2loint(v), o), hi = __shfl_xor(__double2hiint(v), o);
    return fmax(v, __hiloint2double(hi, lo));
}

// min of a running minimum and a fresh cost.  Neither is ever a NaN (finite input; a cost is a sum of squares, +inf at worst), so
// the instruction is given as it is: fmin() would first quieten the running minimum, one more float64 operation per cell.
__device__ __forceinline__ double haus_min(double a, double b)
{
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// one point of y against a lane's R points of x
template <int DIM, int R> __device__ __forceinline__ void haus_step(const double (&xr)[R][DIM], const double (&yc)[DIM], double (&mn)[R])
{
#pragma unroll
    for (int r = 0; r < R; ++r) {
        double df = xr[r][0] - yc[0];
        double cost = df * df;
#pragma unroll
        for (int k = 1; k < DIM; ++k) {
            df = xr[r][k] - yc[k];
            cost = cost + df * df;
        }
        mn[r] = haus_min(mn[r], cost);
    }
}

template <typename T, int DIM, int R, int G> __global__ __launch_bounds__(PAIR_THREADS) void k_hausdorff(HausdorffArgs<T> a)
{
    constexpr int PPW = ANN_WAVE / G;   // pairs per wavefront
    const int lane = threadIdx.x & (ANN_WAVE - 1), gl = lane & (G - 1), slot = lane / G;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / ANN_WAVE;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / ANN_WAVE;
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    for (int64_t base = wave * PPW; base < a.n; base += nwaves * PPW) {   // (wave-uniform: the shuffles run with every lane on)
        const int64_t t = base + slot;
        const PairSlot ps = pair_decode(a, t);
        const bool active = ps.active;
        const int i = ps.i, j = ps.j;
        const int64_t opos = ps.opos;
        int n = a.len[i], m = a.len[j];
        const T *x = a.val + (int64_t)a.off[i] * DIM, *y = a.val + (int64_t)a.off[j] * DIM;
        int nu = n, mu = m;        // the largest of the wavefront's pairs: the bounds of the loops below
#pragma unroll
        for (int o = G; o < ANN_WAVE; o <<= 1) {
            nu = max(nu, __shfl_xor(nu, o));
            mu = max(mu, __shfl_xor(mu, o));
        }
        nu = __builtin_amdgcn_readfirstlane(nu);   // (every lane holds the same two values by now: scalar loop counters)
        mu = __builtin_amdgcn_readfirstlane(mu);
        double best = 0.0;         // every c(i, j) is >= +0
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll 1
            for (int s0 = 0; s0 < nu; s0 += G * R) {
                double xr[R][DIM], mn[R];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const T *xp = x + (int64_t)min(s0 + gl * R + r, n - 1) * DIM;   // (past the end: the last point again)
#pragma unroll
                    for (int k = 0; k < DIM; ++k) xr[r][k] = (double)xp[k];
                    mn[r] = INF;
                }
                // two steps per trip, each on a point loaded one step ahead; past the end of y the last point again
                double ya[DIM], yb[DIM];
#pragma unroll
                for (int k = 0; k < DIM; ++k) ya[k] = (double)y[k];
                for (int jc = 0; jc < mu; jc += 2) {
                    const T *yp = y + min(jc + 1, m - 1) * DIM;
#pragma unroll
                    for (int k = 0; k < DIM; ++k) yb[k] = (double)yp[k];
                    haus_step<DIM, R>(xr, ya, mn);
                    yp = y + min(jc + 2, m - 1) * DIM;
#pragma unroll
                    for (int k = 0; k < DIM; ++k) ya[k] = (double)yp[k];
                    haus_step<DIM, R>(xr, yb, mn);
                }
#pragma unroll
                for (int r = 0; r < R; ++r) best = fmax(best, mn[r]);
            }
            { const T *p = x; x = y; y = p; int k = n; n = m; m = k; k = nu; nu = mu; mu = k; }   // the other direction
        }
#pragma unroll
        for (int o = 1; o < G; o <<= 1) best = haus_xor_max(best, o);
        if (active && gl == 0) pair_store(a, t, opos, __dsqrt_rn(best));
    }
}

template <typename T, int DIM, int R, int G> static int launch_shape(annchor_ctx *c, const HausdorffArgs<T> &a)
{
    static_assert((G & (G - 1)) == 0 && G <= ANN_WAVE, "a pair takes a power-of-two group of lanes");
    k_hausdorff<T, DIM, R, G><<<pair_grid(c, a.n, G), PAIR_THREADS, 0, c->stream>>>(a);
    ANN_CHECK_HIP(c, hipGetLastError());
    return ANNCHOR_OK;
}

// by the data set's longest set: 4 pairs per wavefront (strips of 128 points) up to HAUS_SHORT points, one pair on 64 lanes
// (strips of 512 points) beyond
#define HAUS_SHORT 512
template <typename T, int DIM> static int launch_dim(annchor_ctx *c, const HausdorffArgs<T> &a)
{
    ANN_REQUIRE(c, c->maxlen >= 1 && c->maxlen <= 4096, ANNCHOR_ELIMIT, "point set size %d outside 1..4096", c->maxlen);
    if (c->maxlen <= HAUS_SHORT) return launch_shape<T, DIM, 8, 16>(c, a);
    return launch_shape<T, DIM, 8, 64>(c, a);
}

template <typename T> static int launch(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    HausdorffArgs<T> a;
    pair_fill(a, src, d_out, d_RA, d_ncm);
    a.val = c->sym.as<T>();
    a.off = c->soff.as<int32_t>(); a.len = c->slen.as<int32_t>();
    ProfScope ps(c, "hausdorff_pairs", (double)src.n * (2.0 * c->maxlen * c->curve_dim * sizeof(T) + 16));
    switch (c->curve_dim) {
    case 1: return launch_dim<T, 1>(c, a);
    case 2: return launch_dim<T, 2>(c, a);
    case 3: return launch_dim<T, 3>(c, a);
    case 4: return launch_dim<T, 4>(c, a);
    default: ann_set_err(c, "point set dim %d outside 1..4", c->curve_dim); return ANNCHOR_EINVAL;
    }
}

int ann_hausdorff_launch(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    if (src.n == 0) return ANNCHOR_OK;
    return c->metric == ANNCHOR_METRIC_HAUSDORFF_F32 ? launch<float>(c, src, d_out, d_RA, d_ncm)
                                                     : launch<double>(c, src, d_out, d_RA, d_ncm);
}
