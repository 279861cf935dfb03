// editwide.hip -- the edit distance with real penalty (ERP) and the time warp edit distance (TWE) on members of 5 .. 64
// coordinates per point, over a pair list.  The definitions are seqdp.hip's (its head, "ERP", "TWE") and so is the contract:
// dist(a, b) = sqrt(sum over k = 0 .. dim-1, in that order, of t_k * t_k), every subtraction, product and addition rounded on its
// own in float64, the sum started from the k = 0 product, the square root correctly rounded, float32 input widened exactly; a cell
// is the min of three sums of fixed operands, so the kernel equals the sequential double loop bit for bit, in both orders of a
// pair, and is free to put the longer member on the rows.  The result is the corner cell; there is no square root at the end.
//
// k_editwide<T, Op> keeps k_seqwide's split (seqwide.hip): one pair per workgroup of four waves, pairs taken grid-stride, rows
// cut into strips of EW_ROWS = 64, a strip's anti-diagonal steps cut into phases of EW_STEPS = 48, the phase's parallelogram
// {(l, s - l)} as the cost tile [step][lane] in a ring of two, waves 1 .. 3 producing phase p + 1 while wave 0 sweeps phase p,
// every __syncthreads() met by all four waves in uniform control flow.  What differs is the data flow:
//
//   the tile holds dist, not its square: a producer takes one __dsqrt_rn per cell before the store.
//
//   three costs per cell.  dg + match, up + (the row's cost), left + (the column's cost).  The row's and column's costs are
//   properties of a point of the pool -- ERP: gx(i) = dist(x[i], gap point); TWE: dx(i) = dist(x[i], x[i-1]) + nl, x[-1] the
//   origin -- which the loader (bind.hip) computes once per data set into `ptcost`, laid out like the pool, beside ERP's
//   `gapsum`.  A lane loads its row's cost once per strip.  The column's costs of a phase, the 111 points of y its tile touches,
//   are staged by the producers in a window in LDS beside the tile, in the same ring of two; lane l at step s reads entry
//   63 + (s - s0) - l -- 64 consecutive doubles -- a step ahead, as the tile entry is read.
//
//   boundaries.  The row above a strip, `brow`, is filled before the first strip with E(-1, j) = gapsum_y[j] (ERP) or +inf
//   (TWE); from then on lane 63 overwrites entry j, 63 entries behind lane 0's reads, with the strip's bottom row.  ERP's lanes
//   start from E(row, -1) = gapsum_x[row], and lane 0's first diagonal is 0 in the first strip and gapsum_x[R0 - 1] below it.
//
//   TWE's dist(x[i-1], y[j-1]) is what lane l - 1 read two steps earlier, possibly from the ring slot the producers are
//   overwriting now: every lane keeps the dist it read last and hands it down with the lane move, exactly as the cell goes
//   down as `top` and is kept a step as `diag`.  Lane 0 takes it from `bdist`, the previous strip's bottom-row dist values
//   (written by lane 63 beside `brow`), which start as 0.0: dist(origin, origin) for the cell (0, 0), and elsewhere in row 0 and
//   column 0 a finite placeholder that only ever meets +inf.
//
// LDS: the ring of tiles 48 KiB, brow 8 KiB, TWE's bdist 8 KiB, the windows 1.7 KiB, and the staged chunk of coordinates, 16 at a
// time for float32 and 8 for float64: at most 78.3 KiB per workgroup (ew_lds_bytes), so that two workgroups share a CU's 160 KiB.
// Neither measure has a band (a banded ERP or TWE loses the triangle inequality) or uses matrix instructions (MFMA fuses and
// reorders the sum the contract fixes).  No atomics; results leave by plain vector stores from the lane of the corner cell.
#include "seqops.h"

#define EW_ROWS 64                          // rows of a strip: the lanes of the sweep wave
#define EW_STEPS 48                         // steps of a phase: 64 x 48 cells = 192 producer threads x 16
#define EW_YPTS (EW_STEPS + EW_ROWS - 1)    // points of y a phase touches
#define EW_WIN 112                          // doubles per window of column costs (EW_YPTS rounded up)
#define EW_MAXLEN 1024
#define EW_PRODUCERS (PAIR_THREADS - ANN_WAVE)

// coordinates staged at a time, and the pitches of the staged chunks in elements of T (seqwide.hip's: +4 banks per coordinate,
// a multiple of 16 bytes)
template <typename T> struct EwShape {
    static constexpr int kc = sizeof(T) == 8 ? 8 : 16;
    static constexpr int x = sizeof(T) == 8 ? EW_ROWS + 2 : EW_ROWS + 4;
    static constexpr int y = sizeof(T) == 8 ? EW_YPTS + 3 : EW_YPTS + 21;
};

struct ErpWideOp {
    static constexpr bool twe = false;
    static constexpr const char *profile = "erp_pairs", *name = "wide erp";
};
struct TweWideOp {
    static constexpr bool twe = true;
    static constexpr const char *profile = "twe_pairs", *name = "wide twe";
};

template <typename T> struct EditArgs : SeqArgs<T> {
    const double *ptcost;   // [points of the pool] ERP: gx of every point; TWE: dx of every point
};

template <typename T, typename Op> static inline size_t ew_lds_bytes(int dim)
{
    const int kc = dim < EwShape<T>::kc ? dim : EwShape<T>::kc;
    return sizeof(double) * (2 * EW_STEPS * EW_ROWS + 2 * EW_WIN + (Op::twe ? 2 : 1) * EW_MAXLEN) +
           sizeof(T) * (size_t)kc * (size_t)(EwShape<T>::x + EwShape<T>::y);
}

template <typename T, typename Op> __global__ __launch_bounds__(PAIR_THREADS) void k_editwide(EditArgs<T> a, int dim)
{
    extern __shared__ double ew_lds[];
    constexpr int KC = EwShape<T>::kc, XP = EwShape<T>::x, YP = EwShape<T>::y;
    double *const cost = ew_lds;                                // [2][EW_STEPS][EW_ROWS] dist
    double *const win = cost + 2 * EW_STEPS * EW_ROWS;          // [2][EW_WIN] the column costs of a phase's points of y
    double *const brow = win + 2 * EW_WIN;                      // [EW_MAXLEN] the row above the strip
    double *const bdist = brow + EW_MAXLEN;                     // TWE: [EW_MAXLEN] dist(x[R0 - 1], y[.])
    T *const xs = reinterpret_cast<T *>(bdist + (Op::twe ? EW_MAXLEN : 0));   // [kc][XP]
    const int kc0 = dim < KC ? dim : KC;
    T *const ys = xs + kc0 * XP;                                // [kc][YP]
    const int tid = threadIdx.x, lane = tid & (ANN_WAVE - 1);
    const bool sweeper = tid < ANN_WAVE;
    const int ptid = tid - ANN_WAVE, rg = ptid & 15, sg = ptid >> 4;   // producers: rows 4 rg .. + 3, steps 4 sg .. + 3 of the phase
    const int nch = (dim + KC - 1) / KC, nslices = 2 * nch;
    const double INF = __longlong_as_double(0x7ff0000000000000ll);

    for (int64_t t = blockIdx.x; t < a.n; t += gridDim.x) {
        const PairSlot ps = pair_decode(a, t);
        int n = a.len[ps.i], m = a.len[ps.j];
        int xo = a.off[ps.i], yo = a.off[ps.j];
        if (n < m) {   // the longer member on the rows
            const int k = n; n = m; m = k;
            const int o = xo; xo = yo; yo = o;
        }
        const T *x = a.val + (int64_t)xo * dim, *y = a.val + (int64_t)yo * dim;
        const double *pcx = a.ptcost + xo, *pcy = a.ptcost + yo;
        const double *gsx = nullptr;   // ERP: E(., -1) of the member on the rows
        if constexpr (!Op::twe) gsx = a.gapsum + xo;

        // row -1 (the last pair's sweep ended at a barrier)
        for (int c = tid; c < m; c += PAIR_THREADS) {
            if constexpr (Op::twe) { brow[c] = INF; bdist[c] = 0.0; }
            else brow[c] = a.gapsum[yo + c];
        }
        __syncthreads();

        double corner = INF;   // the cell (n - 1, m - 1), on the lane that computes it
        for (int R0 = 0; R0 < n; R0 += EW_ROWS) {
            const int nr = min(EW_ROWS, n - R0);
            const int phi = (m + nr - 2) / EW_STEPS;             // the strip's last step is m - 1 + nr - 1
            const int row = R0 + lane, rowc = min(row, n - 1);   // (rows >= n: cells nobody reads)
            // the sweep's registers: the lane's last cell (its left neighbour, and the lane below's top) starts as column -1; the
            // top it received last (its diagonal neighbour); the row's cost.  TWE: the dist it read last and the one received last.
            double d = INF, top_prev = INF;
            if constexpr (!Op::twe) d = gsx[rowc];               // E(row, -1)
            const double rcost = pcx[rowc];
            double clast = 0.0, ctop_prev = 0.0;
            if (lane == 0) {                                     // the cell (R0 - 1, -1)
                if (R0 == 0) top_prev = 0.0;
                else if constexpr (!Op::twe) top_prev = gsx[R0 - 1];
            }

            for (int it = 0; it <= phi + 1; ++it) {
                const int pp = it, pc = pp - 1;                  // the phase produced, the phase swept
                const bool produce = !sweeper && pp <= phi, sweep = sweeper && it > 0;
                const int s0p = pp * EW_STEPS, s0c = pc * EW_STEPS;
                double *const cp = cost + (it & 1) * EW_STEPS * EW_ROWS, *const wp = win + (it & 1) * EW_WIN;
                const double *const cc = cost + ((it + 1) & 1) * EW_STEPS * EW_ROWS;
                const double *const wc = win + ((it + 1) & 1) * EW_WIN + (EW_ROWS - 1) - lane;   // [step of the phase]
                double acc[4][4];
                for (int sl = 0; sl < nslices; ++sl) {
                    const int ch = sl >> 1, k0 = ch * KC, kc = min(KC, dim - k0);
                    if (sweep) {
                        const int sb = s0c + EW_STEPS * sl / nslices, se = s0c + EW_STEPS * (sl + 1) / nslices;
                        // the next step's dist, column cost and row above are read a step ahead: no LDS latency from cell to cell
                        double cnext = cc[(sb - s0c) * EW_ROWS + lane], ynext = wc[sb - s0c];
                        double anext = lane == 0 && sb < m ? brow[sb] : INF, bnext = 0.0;
                        if constexpr (Op::twe) bnext = lane == 0 && sb < m ? bdist[sb] : 0.0;
                        for (int s = sb; s < se; ++s) {
                            const double c = cnext, ycost = ynext;
                            double top = lane_down(d), ctop = 0.0;
                            if (lane == 0) top = anext;
                            if constexpr (Op::twe) {
                                ctop = lane_down(clast);         // dist(x[row - 1], y[jc])
                                if (lane == 0) ctop = bnext;
                            }
                            if (s + 1 < se) {
                                cnext = cc[(s + 1 - s0c) * EW_ROWS + lane];
                                ynext = wc[s + 1 - s0c];
                                if (lane == 0 && s + 1 < m) {
                                    anext = brow[s + 1];
                                    if constexpr (Op::twe) bnext = bdist[s + 1];
                                }
                            }
                            const double diag = top_prev, cdiag = ctop_prev;   // cdiag: dist(x[row - 1], y[jc - 1])
                            top_prev = top;
                            ctop_prev = ctop;
                            clast = c;
                            const int jc = s - lane;
                            if (jc >= 0 && jc < m && lane < nr) {
                                double match = c;
                                if constexpr (Op::twe) match = (c + cdiag) + a.twe_nu2 * fabs((double)(row - jc));
                                const double v = fmin(fmin(diag + match, top + rcost), d + ycost);
                                d = v;
                                if (lane == EW_ROWS - 1) {
                                    brow[jc] = v;
                                    if constexpr (Op::twe) bdist[jc] = c;
                                }
                                if (row == n - 1 && jc == m - 1) corner = v;
                            }
                        }
                    } else if (produce && !(sl & 1)) {
                        // stage chunk ch: the strip's points of x and the phase's points of y, [coordinate][point]; with chunk 0
                        // the column costs of those points of y
                        for (int e = ptid; e < EW_ROWS * kc; e += EW_PRODUCERS) {
                            const int pt = e / kc, kk = e - pt * kc;
                            xs[kk * XP + pt] = x[(int64_t)min(R0 + pt, n - 1) * dim + k0 + kk];
                        }
                        for (int e = ptid; e < EW_YPTS * kc; e += EW_PRODUCERS) {
                            const int pt = e / kc, kk = e - pt * kc;
                            ys[kk * YP + pt] = y[(int64_t)min(max(s0p - (EW_ROWS - 1) + pt, 0), m - 1) * dim + k0 + kk];
                        }
                        if (ch == 0 && ptid < EW_YPTS) wp[ptid] = pcy[min(max(s0p - (EW_ROWS - 1) + ptid, 0), m - 1)];
                    } else if (produce) {
                        // accumulate chunk ch into the 16 partial sums, k in order; the sum starts from the k = 0 product
                        const T *xp = xs + 4 * rg, *yp = ys + 4 * (sg - rg) + (EW_ROWS - 4);
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
                                for (int dr = 0; dr < 4; ++dr) cp[(4 * sg + ds) * EW_ROWS + 4 * rg + dr] = __dsqrt_rn(acc[dr][ds]);
                        }
                    }
                    __syncthreads();
                }
            }
        }
        if (sweeper && lane == (n - 1) % EW_ROWS) pair_store(a, t, ps.opos, corner);
    }
}

template <typename T, typename Op> static int ew_launch(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    const int dim = c->curve_dim;
    ANN_REQUIRE(c, dim > 4 && dim <= 64, ANNCHOR_ELIMIT, "%s: series dim %d outside 5..64", Op::name, dim);
    ANN_REQUIRE(c, c->maxlen >= 1 && c->maxlen <= EW_MAXLEN, ANNCHOR_ELIMIT, "%s: series length %d outside 1..%d at dim %d", Op::name,
                c->maxlen, EW_MAXLEN, dim);
    ANN_REQUIRE(c, c->have_ptcost && c->ptcost.p, ANNCHOR_EINVAL, "%s: no per-point costs bound to this context", Op::name);
    EditArgs<T> a = {};
    pair_fill(a, src, d_out, d_RA, d_ncm);
    a.val = c->sym.as<T>();
    a.off = c->soff.as<int32_t>(); a.len = c->slen.as<int32_t>();
    a.gapsum = Op::twe ? nullptr : c->gapsum.as<double>();
    a.ptcost = c->ptcost.as<double>();
    a.twe_nl = c->twe_nl; a.twe_nu2 = c->twe_nu2;
    const size_t lds = ew_lds_bytes<T, Op>(dim);
    ANN_REQUIRE(c, lds <= 80 * 1024, ANNCHOR_ELIMIT, "%s: dim %d needs %zu B of LDS (> 80 KiB)", Op::name, dim, lds);
    if (lds > 64 * 1024)
        ANN_CHECK_HIP(c, hipFuncSetAttribute((const void *)k_editwide<T, Op>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // (a point: its coordinates, its cost and, under ERP, its entry of gapsum)
    ProfScope ps(c, Op::profile, (double)src.n * (2.0 * c->maxlen * (dim * sizeof(T) + (Op::twe ? 1 : 2) * sizeof(double)) + 16));
    // one pair per workgroup; two workgroups share a CU's LDS, and beyond that the workgroups take further pairs grid-stride
    const int64_t cap = (int64_t)c->prop.multiProcessorCount * 8;
    k_editwide<T, Op><<<(int)(src.n < cap ? src.n : cap), PAIR_THREADS, lds, c->stream>>>(a, dim);
    ANN_CHECK_HIP(c, hipGetLastError());
    return ANNCHOR_OK;
}

int ann_editwide_launch(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    if (src.n == 0) return ANNCHOR_OK;
    switch (c->metric) {
    case ANNCHOR_METRIC_ERP_F32: return ew_launch<float, ErpWideOp>(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_ERP_F64: return ew_launch<double, ErpWideOp>(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_TWE_F32: return ew_launch<float, TweWideOp>(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_TWE_F64: return ew_launch<double, TweWideOp>(c, src, d_out, d_RA, d_ncm);
    default: ann_set_err(c, "no edit measure of 5 .. 64 coordinates per point bound to this context"); return ANNCHOR_EINVAL;
    }
}
