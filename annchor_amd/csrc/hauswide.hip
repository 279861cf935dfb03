// hauswide.hip -- Hausdorff distance between point sets of 5 .. 512 coordinates per point, over a pair list.  The definition and
// the contract are hausdorff.hip's (its head): c(i, j) the sum over k = 0 .. dim-1, in that order, of t_k * t_k with every
// subtraction, product and addition rounded on its own in float64 and the sum starting from the k = 0 product, float32 input
// widened exactly, the correctly rounded sqrt of max(h(x, y), h(y, x)).  min and max are exact and associative, and a duplicated
// point changes nothing, so the kernel equals the cell-by-cell loop bit for bit in both orders of a pair, and rows and columns
// past the end of a set are clamped to the set's last point, never masked.
//
// k_hausdorff keeps a lane's points of x in registers (R x DIM doubles, DIM a template argument) and cannot grow with dim; it
// also evaluates every c(i, j) twice, once per directed pass.  Here the cost matrix of a pair is evaluated ONCE, in tiles through
// LDS, and both directed distances are taken from it: a GEMM-shaped tile with a min epilogue along the rows and along the columns.
//
// k_hauswide<T, S>: one pair per workgroup of S/4 x S/4 threads, pairs taken grid-stride; dim is a runtime argument.  The cost
// matrix is cut into tiles of S x S cells, walked strip by strip (S rows), column tile by column tile, chunk by chunk of
// HW_KC = 16 coordinates.  Thread (rg, cg) = (tid mod S/4, tid / (S/4)) owns 4 rows x 4 columns of the tile: 16 partial sums in
// registers across the chunks of k.  Two instantiations: S = 64 (256 threads, four waves) and S = 32 (64 threads: a single wave,
// whose barriers cost nothing; data sets of short sets, see HAUSW_SHORT).
//
//   staging: the tile's S points of x and S points of y, 16 coordinates at a time, in LDS as T (not widened: float32 costs half
//   the LDS traffic), laid out [coordinate][point] at a pitch of S + 4 banks.  A ring of two chunk buffers: the global loads of
//   step s + 1 (the next chunk, or the first chunk of the next tile) are issued into registers before step s is accumulated and
//   stored to the other buffer after it; one barrier per step.
//
//   accumulate: per coordinate a thread reads its 4 values of x and 4 of y by 128-bit LDS reads (float32: one each, points
//   4 g .. 4 g + 3; float64: two each, points 2 g, 2 g + 1 and S/2 + 2 g, S/2 + 2 g + 1, so that the lanes of one read are 16 B
//   apart in both), widens them, and does 48 float64 operations on its 16 sums.
//
//   epilogue, at a tile's last chunk, no atomics: the 16 costs fold into 4 running row minima, which stay in registers over the
//   strip's column tiles; at the strip's end they are reduced over the S/4 threads that share rg (__shfl_xor at 16 and 32 / 8, 16
//   and 32; S = 64: one exchange of 4 x 64 doubles between the four waves, in a buffer of the strip's parity, read after the
//   step's barrier) and folded into the pair's running max.  The same 16 costs give 4 column minima, reduced over the S/4 threads
//   that share cg -- consecutive lanes of one wave -- and the rg = 0 lane folds them into colmin[column], an LDS array of the
//   pair's columns: column c belongs to one lane through all strips, so no barrier or atomic guards it, and the first strip
//   assigns, so nothing initialises it.  At the end of the pair one block reduction takes the max over colmin[0 .. m) into the
//   running max and thread 0 stores the square root.
//
// Matrix instructions are not used: MFMA fuses and reorders the sum the contract fixes.
#include "hausops.h"

#define HW_KC 16   // coordinates staged at a time

// pitch of a staged coordinate in elements of T: S points + 4 banks, so the staging stores of one point's 16 coordinates spread
// over the banks; a multiple of 16 bytes, so every 128-bit read is aligned
template <typename T, int S> struct HwTile {
    static constexpr int G = S / 4, NT = G * G, NW = NT / ANN_WAVE, E = S * HW_KC / NT;
    static constexpr int pitch = sizeof(T) == 8 ? S + 2 : S + 4;
    static constexpr int xch = NW > 1 ? 2 * NW * S + NW : 0;   // doubles: the row minima's exchange [2][NW][S], the final max [NW]
    static size_t lds_bytes(int cmax) { return sizeof(double) * (size_t)(cmax + xch) + sizeof(T) * (size_t)(2 * 2 * HW_KC * pitch); }
};

// the q-th of the 4 points of group g, in the tile
template <typename T, int S> __device__ __forceinline__ int hw_point(int g, int q)
{
    return sizeof(T) == 8 ? (q >> 1) * (S / 2) + 2 * g + (q & 1) : 4 * g + q;
}

// those 4 points of one staged coordinate, widened
template <int S> __device__ __forceinline__ void hw_read4(const float *row, int g, double (&v)[4])
{
    const float4 p = *reinterpret_cast<const float4 *>(row + 4 * g);
    v[0] = (double)p.x; v[1] = (double)p.y; v[2] = (double)p.z; v[3] = (double)p.w;
}
template <int S> __device__ __forceinline__ void hw_read4(const double *row, int g, double (&v)[4])
{
    const double2 lo = *reinterpret_cast<const double2 *>(row + 2 * g), hi = *reinterpret_cast<const double2 *>(row + S / 2 + 2 * g);
    v[0] = lo.x; v[1] = lo.y; v[2] = hi.x; v[3] = hi.y;
}

template <typename T, int S> __global__ __launch_bounds__(S * S / 16) void k_hauswide(HausdorffArgs<T> a, int dim, int cmax)
{
    using Tile = HwTile<T, S>;
    constexpr int G = Tile::G, NT = Tile::NT, NW = Tile::NW, E = Tile::E, P = Tile::pitch;
    extern __shared__ double hw_lds[];
    double *const colmin = hw_lds;                                // [cmax] (cmax even: what follows stays 16-byte aligned)
    double *const xch = colmin + cmax;                            // [2][NW][S]
    double *const red = xch + 2 * NW * S;                         // [NW]           (both: S = 64 only)
    T *const stage = reinterpret_cast<T *>(xch + Tile::xch);      // [2][x, y][HW_KC][P]
    const int tid = threadIdx.x, lane = tid & (ANN_WAVE - 1), wave = tid / ANN_WAVE;
    const int rg = tid & (G - 1), cg = tid / G;
    const int skk = tid & (HW_KC - 1), spt = tid / HW_KC;         // staging: coordinate skk of points spt + q NT / 16
    const int nch = (dim + HW_KC - 1) / HW_KC;
    const double INF = __longlong_as_double(0x7ff0000000000000ll);

    for (int64_t t = blockIdx.x; t < a.n; t += gridDim.x) {
        const PairSlot ps = pair_decode(a, t);
        const int n = a.len[ps.i], m = a.len[ps.j];
        const T *const x = a.val + (int64_t)a.off[ps.i] * dim, *const y = a.val + (int64_t)a.off[ps.j] * dim;
        const int nct = (m + S - 1) / S, total = ((n + S - 1) / S) * nct * nch;

        // a step's points, global -> registers (past the end of a set: its last point again; past dim: never read)
        T xr[E], yr[E];
        auto fetch = [&](int st, int ct, int ch) {
            const int k = ch * HW_KC + skk;
#pragma unroll
            for (int q = 0; q < E; ++q) {
                const int pt = spt + q * (NT / HW_KC);
                xr[q] = k < dim ? x[(int64_t)min(st * S + pt, n - 1) * dim + k] : (T)0;
                yr[q] = k < dim ? y[(int64_t)min(ct * S + pt, m - 1) * dim + k] : (T)0;
            }
        };
        // registers -> buffer b of the ring
        auto put = [&](int b) {
            T *const xs = stage + b * 2 * HW_KC * P + skk * P, *const ys = xs + HW_KC * P;
#pragma unroll
            for (int q = 0; q < E; ++q) {
                const int pt = spt + q * (NT / HW_KC);
                xs[pt] = xr[q];
                ys[pt] = yr[q];
            }
        };

        int lst = 0, lct = 0, lch = 0;   // the step in flight
        fetch(0, 0, 0);
        put(0);
        __syncthreads();

        double acc[4][4], rowmin[4] = {INF, INF, INF, INF};
        double best = 0.0;               // every c(i, j) is >= +0
        int st = 0, ct = 0, ch = 0;      // the step accumulated
        for (int s = 0; s < total; ++s) {
            const bool more = s + 1 < total;
            if (more) {
                if (++lch == nch) {
                    lch = 0;
                    if (++lct == nct) { lct = 0; ++lst; }
                }
                fetch(lst, lct, lch);
            }

            // chunk ch into the 16 partial sums, k in order; the sum starts from the k = 0 product
            const int kc = min(HW_KC, dim - ch * HW_KC);
            const T *xp = stage + (s & 1) * 2 * HW_KC * P, *yp = xp + HW_KC * P;
            double xv[4], yv[4];
            int kk = 0;
            if (ch == 0) {
                hw_read4<S>(xp, rg, xv);
                hw_read4<S>(yp, cg, yv);
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const double df = xv[r] - yv[c];
                        acc[r][c] = df * df;
                    }
                kk = 1; xp += P; yp += P;
            }
#pragma unroll 2
            for (; kk < kc; ++kk, xp += P, yp += P) {
                hw_read4<S>(xp, rg, xv);
                hw_read4<S>(yp, cg, yv);
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const double df = xv[r] - yv[c];
                        acc[r][c] = acc[r][c] + df * df;
                    }
            }

            const bool tile_end = ch == nch - 1, strip_end = tile_end && ct == nct - 1;
            if (tile_end) {
                double cm[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    rowmin[q] = haus_min(rowmin[q], haus_min(haus_min(acc[q][0], acc[q][1]), haus_min(acc[q][2], acc[q][3])));
                    cm[q] = haus_min(haus_min(acc[0][q], acc[1][q]), haus_min(acc[2][q], acc[3][q]));
                }
#pragma unroll
                for (int o = 1; o < G; o <<= 1)   // over rg: the G consecutive lanes that share cg
#pragma unroll
                    for (int q = 0; q < 4; ++q) cm[q] = haus_xor_min(cm[q], o);
                if (rg == 0) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int col = ct * S + hw_point<T, S>(cg, q);
                        if (col < m) colmin[col] = st == 0 ? cm[q] : haus_min(colmin[col], cm[q]);
                    }
                }
                if (strip_end) {
#pragma unroll
                    for (int o = G; o < ANN_WAVE; o <<= 1)   // over the wave's cg
#pragma unroll
                        for (int q = 0; q < 4; ++q) rowmin[q] = haus_xor_min(rowmin[q], o);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (NW == 1) best = fmax(best, rowmin[q]);
                        else if (lane < G) xch[((st & 1) * NW + wave) * S + 4 * rg + q] = rowmin[q];
                        rowmin[q] = INF;
                    }
                }
            }
            if (more) put((s + 1) & 1);
            __syncthreads();
            if (NW > 1 && strip_end && tid < S) {   // the four waves' minima of row slot tid
                const double *const e = xch + (st & 1) * NW * S + tid;
                double v = e[0];
#pragma unroll
                for (int w = 1; w < NW; ++w) v = haus_min(v, e[w * S]);
                best = fmax(best, v);
            }
            if (++ch == nch) {
                ch = 0;
                if (++ct == nct) { ct = 0; ++st; }
            }
        }

        for (int c = tid; c < m; c += NT) best = fmax(best, colmin[c]);
#pragma unroll
        for (int o = 1; o < ANN_WAVE; o <<= 1) best = haus_xor_max(best, o);
        if (NW > 1) {
            if (lane == 0) red[wave] = best;
            __syncthreads();
            best = red[0];
#pragma unroll
            for (int w = 1; w < NW; ++w) best = fmax(best, red[w]);
        }
        if (tid == 0) pair_store(a, t, ps.opos, __dsqrt_rn(best));
    }
}

template <typename T, int S> static int hw_launch_shape(annchor_ctx *c, const HausdorffArgs<T> &a)
{
    using Tile = HwTile<T, S>;
    const int cmax = (c->maxlen + 1) & ~1;
    const size_t lds = Tile::lds_bytes(cmax);
    if (lds > 64 * 1024)
        ANN_CHECK_HIP(c, hipFuncSetAttribute((const void *)k_hauswide<T, S>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // as many workgroups as a CU's LDS and wave slots hold (four waves: 4, one wave: 16); beyond that pairs are taken grid-stride
    const int64_t fit = (int64_t)(160 * 1024 / lds), slots = Tile::NW > 1 ? 4 : 16;
    const int64_t cap = (int64_t)c->prop.multiProcessorCount * (fit < 1 ? 1 : fit < slots ? fit : slots);
    k_hauswide<T, S><<<(int)(a.n < cap ? a.n : cap), Tile::NT, lds, c->stream>>>(a, c->curve_dim, cmax);
    ANN_CHECK_HIP(c, hipGetLastError());
    return ANNCHOR_OK;
}

// by the data set's longest set: tiles of 32 x 32 on one wave up to HAUSW_SHORT points, of 64 x 64 on four waves beyond
// (measured: DESIGN.md 3.11a).  ANNCHOR_HAUSW_SHAPE = 32 or 64 forces a shape (tools/hauswide_rates.py measures both on the
// same data; every data set can take either); read per launch.
#define HAUSW_SHORT 192
template <typename T> static int hw_launch(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    const int dim = c->curve_dim;
    ANN_REQUIRE(c, dim > 4 && dim <= 512, ANNCHOR_ELIMIT, "point set dim %d outside 5..512", dim);
    ANN_REQUIRE(c, c->maxlen >= 1 && c->maxlen <= 4096, ANNCHOR_ELIMIT, "point set size %d outside 1..4096", c->maxlen);
    HausdorffArgs<T> a;
    pair_fill(a, src, d_out, d_RA, d_ncm);
    a.val = c->sym.as<T>();
    a.off = c->soff.as<int32_t>(); a.len = c->slen.as<int32_t>();
    ProfScope ps(c, "hausdorff_pairs", (double)src.n * (2.0 * c->maxlen * dim * sizeof(T) + 16));
    const char *e = getenv("ANNCHOR_HAUSW_SHAPE");
    const int shape = e ? atoi(e) : 0;
    ANN_REQUIRE(c, shape == 0 || shape == 32 || shape == 64, ANNCHOR_EINVAL, "ANNCHOR_HAUSW_SHAPE=%s: 32 or 64", e);
    if (shape ? shape == 32 : c->maxlen <= HAUSW_SHORT) return hw_launch_shape<T, 32>(c, a);
    return hw_launch_shape<T, 64>(c, a);
}

int ann_hauswide_launch(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    if (src.n == 0) return ANNCHOR_OK;
    return c->metric == ANNCHOR_METRIC_HAUSDORFF_F32 ? hw_launch<float>(c, src, d_out, d_RA, d_ncm)
                                                     : hw_launch<double>(c, src, d_out, d_RA, d_ncm);
}
