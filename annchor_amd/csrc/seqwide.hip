// seqwide.hip -- DTW and the discrete Frechet distance on members of 5 .. 64 coordinates per point, over a pair list.  The
// definitions are seqdp.hip's (its head, "c(i, j)", "DTW", "Frechet") and so is the contract: every subtraction, product and
// addition of c(i, j) rounded on its own in float64, the sum taken over k = 0 .. dim-1 in that order starting from the k = 0
// product, float32 input widened exactly, the correctly rounded sqrt of the corner cell; min and max are exact, so the kernel
// equals the sequential double loop bit for bit, in both orders of a pair, and is free to put the longer member on the rows.
//
// At these dims a cell is 3 dim + 2 float64 operations of which all but two belong to c(i, j), which depends on no other cell.
// k_seqdp keeps a lane's coordinates of x in registers and cannot grow with dim; here the work is split in two phases instead.
//
// k_seqwide<T, Op>: one pair per workgroup of four waves, pairs taken grid-stride; dim is a runtime argument.  The longer
// member is on the rows, which are cut into strips of SW_ROWS = 64; a strip is swept in anti-diagonal steps, lane l of the sweep
// wave on row l and, at step s, on column s - l.  The steps of a strip are cut into PHASES of SW_STEPS = 48; phase p is the
// parallelogram of cells {(l, s - l): l in 0 .. 63, s in 48 p .. 48 p + 47}, exactly what the sweep consumes in those steps.
//
//   cost phase (waves 1 .. 3, 192 threads): the strip's 64 points of x and the phase's 111 points of y (columns 48 p - 63 ..
//   48 p + 47, clamped into the member: cells nobody reads) are staged in LDS as T, SW_KC = 16 coordinates at a time, laid out
//   [coordinate][point].  A thread owns 4 rows x 4 steps of the parallelogram: per coordinate it reads 4 values of x and the 7
//   values of y its 16 cells touch (cell (dr, ds) reads y[3 + ds - dr]), widens them, and does 48 operations on 16 partial sums
//   kept in registers across the chunks of k.  The finished c goes to LDS as float64 at [step][lane].
//
//   sweep phase (wave 0): k_seqdp's schedule at R = 1 with the cost read from LDS: the top and diagonal neighbours come from
//   lane l - 1 by wave_shr:1, c from [step][lane] -- 64 consecutive doubles, free of bank conflicts without padding -- and the
//   strip's bottom row (<= 1024 doubles) stays in LDS as the next strip's top boundary.
//
// The cost tiles form a ring of two: while wave 0 sweeps phase p, waves 1 .. 3 produce phase p + 1.  Because the tile is the
// sweep's own parallelogram, a sweep step never touches two tiles.  Every __syncthreads() is met by all four waves in uniform
// control flow: an iteration of the pipeline is, per chunk of k, {stage | sweep a slice} barrier {accumulate | sweep a slice}
// barrier, the sweep's 48 steps being cut into as many slices as there are barriers.
//
// DTW's band: a phase whose every cell lies outside |i - j| <= w is neither produced nor swept (a strip at rows R0 .. R0 + 63
// meets the band in steps R0 - w .. R0 + 126 + w only), so window = 0 on equal lengths touches O(n) cells.  A skipped cell is
// +inf, which is what the sweep's registers start from; lane 0 reads the previous strip's bottom row under the band's test, so
// an entry no strip wrote is never used.  Matrix instructions are not used: MFMA fuses and reorders the sum the contract fixes.
// No atomics; results leave by plain vector stores from the lane that computed the corner cell.
#include "seqops.h"

#define SW_ROWS 64                          // rows of a strip: the lanes of the sweep wave
#define SW_STEPS 48                         // steps of a phase: 64 x 48 cells = 192 producer threads x 16
#define SW_KC 16                            // coordinates staged at a time
#define SW_YPTS (SW_STEPS + SW_ROWS - 1)    // points of y a phase touches
#define SW_MAXLEN 1024
#define SW_PRODUCERS (PAIR_THREADS - ANN_WAVE)

// pitches of the staged chunks in elements of T: +4 banks per coordinate, so the staging stores of one point's coordinates
// spread over the banks, and a multiple of 16 bytes, so four consecutive points are one aligned 128-bit read
template <typename T> struct SwPitch {
    static constexpr int x = sizeof(T) == 8 ? SW_ROWS + 2 : SW_ROWS + 4;
    static constexpr int y = sizeof(T) == 8 ? SW_YPTS + 3 : SW_YPTS + 21;
};

static inline size_t sw_lds_bytes(int dim, size_t elem, int xpitch, int ypitch)
{
    const int kc = dim < SW_KC ? dim : SW_KC;
    return sizeof(double) * (2 * SW_STEPS * SW_ROWS + SW_MAXLEN) + elem * (size_t)kc * (size_t)(xpitch + ypitch);
}

template <typename T, typename Op> __global__ __launch_bounds__(PAIR_THREADS) void k_seqwide(SeqArgs<T> a, int dim)
{
    extern __shared__ double sw_lds[];
    double *const cost = sw_lds;                                // [2][SW_STEPS][SW_ROWS]
    double *const brow = cost + 2 * SW_STEPS * SW_ROWS;         // [SW_MAXLEN] the previous strip's bottom row
    T *const xs = reinterpret_cast<T *>(brow + SW_MAXLEN);      // [kc][XP]
    constexpr int XP = SwPitch<T>::x, YP = SwPitch<T>::y;
    const int kc0 = dim < SW_KC ? dim : SW_KC;
    T *const ys = xs + kc0 * XP;                                // [kc][YP]
    const int tid = threadIdx.x, lane = tid & (ANN_WAVE - 1);
    const bool sweeper = tid < ANN_WAVE;
    const int ptid = tid - ANN_WAVE, rg = ptid & 15, sg = ptid >> 4;   // producers: rows 4 rg .. + 3, steps 4 sg .. + 3 of the phase
    const int nch = (dim + SW_KC - 1) / SW_KC, nslices = 2 * nch;
    const double INF = __longlong_as_double(0x7ff0000000000000ll);

    for (int64_t t = blockIdx.x; t < a.n; t += gridDim.x) {
        const PairSlot ps = pair_decode(a, t);
        int n = a.len[ps.i], m = a.len[ps.j];
        const T *x = a.val + (int64_t)a.off[ps.i] * dim, *y = a.val + (int64_t)a.off[ps.j] * dim;
        if (n < m) {   // the longer member on the rows
            const T *p = x; x = y; y = p; const int k = n; n = m; m = k;
        }
        const int w = Op::band ? min(max(a.window, n - m), 2 * SW_MAXLEN) : 0;   // (beyond the matrix every band is the same)

        double corner = INF;   // the cell (n - 1, m - 1), on the lane that computes it
        for (int R0 = 0; R0 < n; R0 += SW_ROWS) {
            const int nr = min(SW_ROWS, n - R0);
            int plo = 0, phi = (m + nr - 2) / SW_STEPS;          // the strip's last step is m - 1 + nr - 1
            if (Op::band) {
                plo = max(R0 - w, 0) / SW_STEPS;
                phi = min(phi, (R0 + 2 * (SW_ROWS - 1) + w) / SW_STEPS);
            }
            // the sweep's registers: the lane's last cell (its left neighbour, and the lane below's top), the top it received
            // last (its diagonal neighbour).  Before the first step all of it is outside the matrix or the band: +inf, but for
            // the cell (-1, -1) = 0 and what lane 0 reads from the strip above.
            double d = INF, top_prev = INF;
            const int row = R0 + lane;
            auto above = [&](int c) -> double {   // D(R0 - 1, c) as lane 0 sees it
                if (R0 == 0 || c < 0 || c >= m) return INF;
                if (Op::band && (R0 - 1 - c > w || c - (R0 - 1) > w)) return INF;
                return brow[c];
            };
            if (sweeper && lane == 0) top_prev = R0 == 0 ? 0.0 : above(plo * SW_STEPS - 1);

            for (int it = 0; it <= phi - plo + 1; ++it) {
                const int pp = plo + it, pc = pp - 1;            // the phase produced, the phase swept
                const bool produce = !sweeper && pp <= phi, sweep = sweeper && it > 0;
                const int s0p = pp * SW_STEPS, s0c = pc * SW_STEPS;
                double *const cp = cost + (it & 1) * SW_STEPS * SW_ROWS;
                const double *const cc = cost + ((it + 1) & 1) * SW_STEPS * SW_ROWS;
                double acc[4][4];
                for (int sl = 0; sl < nslices; ++sl) {
                    const int ch = sl >> 1, k0 = ch * SW_KC, kc = min(SW_KC, dim - k0);
                    if (sweep) {
                        const int sb = s0c + SW_STEPS * sl / nslices, se = s0c + SW_STEPS * (sl + 1) / nslices;
                        // the next step's cost and row above are read a step ahead: no LDS latency on the chain from cell to cell
                        double cnext = cc[(sb - s0c) * SW_ROWS + lane], anext = lane == 0 ? above(sb) : INF;
                        for (int s = sb; s < se; ++s) {
                            const double c = cnext;
                            double top = lane_down(d);
                            if (lane == 0) top = anext;
                            if (s + 1 < se) {
                                cnext = cc[(s + 1 - s0c) * SW_ROWS + lane];
                                if (lane == 0) anext = above(s + 1);
                            }
                            const double diag = top_prev;
                            top_prev = top;
                            const int jc = s - lane;
                            if (jc >= 0 && jc < m && lane < nr) {
                                double v = Op::cell(c, d, top, diag);
                                if (Op::band && (row - jc > w || jc - row > w)) v = INF;
                                d = v;
                                if (lane == SW_ROWS - 1) brow[jc] = v;
                                if (row == n - 1 && jc == m - 1) corner = v;
                            }
                        }
                    } else if (produce && !(sl & 1)) {
                        // stage chunk ch: the strip's points of x and the phase's points of y, [coordinate][point]
                        for (int e = ptid; e < SW_ROWS * kc; e += SW_PRODUCERS) {
                            const int pt = e / kc, kk = e - pt * kc;
                            xs[kk * XP + pt] = x[(int64_t)min(R0 + pt, n - 1) * dim + k0 + kk];
                        }
                        for (int e = ptid; e < SW_YPTS * kc; e += SW_PRODUCERS) {
                            const int pt = e / kc, kk = e - pt * kc;
                            ys[kk * YP + pt] = y[(int64_t)min(max(s0p - (SW_ROWS - 1) + pt, 0), m - 1) * dim + k0 + kk];
                        }
                    } else if (produce) {
                        // accumulate chunk ch into the 16 partial sums, k in order; the sum starts from the k = 0 product
                        const T *xp = xs + 4 * rg, *yp = ys + 4 * (sg - rg) + (SW_ROWS - 4);
                        for (int kk = 0; kk < kc; ++kk, xp += XP, yp += YP) {
                            double xv[4], yv[7];
#pragma unroll
                            for (int q = 0; q < 4; ++q) xv[q] = (double)xp[q];
#pragma unroll
                            for (int q = 0; q < 7; ++q) yv[q] = (double)yp[q];
                            if (k0 + kk == 0) {
#pragma unroll
                                for (int dr = 0; dr < 4; ++dr)
#pragma unroll
                                    for (int ds = 0; ds < 4; ++ds) {
                                        const double df = xv[dr] - yv[3 + ds - dr];
                                        acc[dr][ds] = df * df;
                                    }
                            } else {
#pragma unroll
                                for (int dr = 0; dr < 4; ++dr)
#pragma unroll
                                    for (int ds = 0; ds < 4; ++ds) {
                                        const double df = xv[dr] - yv[3 + ds - dr];
                                        acc[dr][ds] = acc[dr][ds] + df * df;
                                    }
                            }
                        }
                        if (ch == nch - 1) {
#pragma unroll
                            for (int ds = 0; ds < 4; ++ds)
#pragma unroll
                                for (int dr = 0; dr < 4; ++dr) cp[(4 * sg + ds) * SW_ROWS + 4 * rg + dr] = acc[dr][ds];
                        }
                    }
                    __syncthreads();
                }
            }
        }
        if (sweeper && lane == (n - 1) % SW_ROWS) pair_store(a, t, ps.opos, __dsqrt_rn(corner));
    }
}

template <typename T, typename Op> static int sw_launch(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    const int dim = c->curve_dim;
    ANN_REQUIRE(c, dim > 4 && dim <= 64, ANNCHOR_ELIMIT, "%s dim %d outside 5..64", Op::member, dim);
    ANN_REQUIRE(c, c->maxlen >= 1 && c->maxlen <= SW_MAXLEN, ANNCHOR_ELIMIT, "%s length %d outside 1..%d at dim %d", Op::member, c->maxlen,
                SW_MAXLEN, dim);
    SeqArgs<T> a = {};
    pair_fill(a, src, d_out, d_RA, d_ncm);
    a.val = c->sym.as<T>();
    a.off = c->soff.as<int32_t>(); a.len = c->slen.as<int32_t>();
    a.window = c->dtw_window;
    const size_t lds = sw_lds_bytes(dim, sizeof(T), SwPitch<T>::x, SwPitch<T>::y);
    ANN_REQUIRE(c, lds <= 160 * 1024, ANNCHOR_ELIMIT, "%s dim %d needs %zu B of LDS (> 160 KiB)", Op::member, dim, lds);
    if (lds > 64 * 1024)
        ANN_CHECK_HIP(c, hipFuncSetAttribute((const void *)k_seqwide<T, Op>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ProfScope ps(c, Op::profile, (double)src.n * (2.0 * c->maxlen * Op::point_bytes(dim, sizeof(T)) + 16));
    // one pair per workgroup; two workgroups share a CU's LDS, and beyond that the workgroups take further pairs grid-stride
    const int64_t cap = (int64_t)c->prop.multiProcessorCount * 8;
    k_seqwide<T, Op><<<(int)(src.n < cap ? src.n : cap), PAIR_THREADS, lds, c->stream>>>(a, dim);
    ANN_CHECK_HIP(c, hipGetLastError());
    return ANNCHOR_OK;
}

int ann_seqwide_launch(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    if (src.n == 0) return ANNCHOR_OK;
    switch (c->metric) {
    case ANNCHOR_METRIC_DTW_F32:
        return c->dtw_window >= 0 ? sw_launch<float, DtwOp<true>>(c, src, d_out, d_RA, d_ncm)
                                  : sw_launch<float, DtwOp<false>>(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_DTW_F64:
        return c->dtw_window >= 0 ? sw_launch<double, DtwOp<true>>(c, src, d_out, d_RA, d_ncm)
                                  : sw_launch<double, DtwOp<false>>(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_FRECHET_F32: return sw_launch<float, FrechetOp>(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_FRECHET_F64: return sw_launch<double, FrechetOp>(c, src, d_out, d_RA, d_ncm);
    default: ann_set_err(c, "no measure of 5 .. 64 coordinates per point bound to this context"); return ANNCHOR_EINVAL;
    }
}
