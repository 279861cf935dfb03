// wed.hip -- weighted Levenshtein distance between strings over a pair list: the edit distance whose substitution and insert /
// delete costs come from a table of the data set (no reference counterpart: the reference answers every cost model but unit
// costs with a user-supplied host function), the same distance under affine gap costs (k_affine, further down), and the same
// distance with swaps of two adjacent symbols (optimal string alignment, k_osa, last).
//
//   alphabet of A distinct symbols, 1 <= A <= 128; a string is 0 .. 2048 dense codes 0 .. A-1
//   S   float64 [A][A]  substitution costs: finite, >= 0, zero diagonal, S[a][b] == S[b][a] bit for bit
//   g   float64 [A]     insert / delete cost per symbol: finite, >= 0
//
//   E(-1, -1) = 0     E(i, -1) = E(i-1, -1) + g[x_i]     E(-1, j) = E(-1, j-1) + g[y_j]        (left to right, one addition per step)
//   E(i, j) = min( E(i-1, j-1) + S[x_i][y_j],   E(i-1, j) + g[x_i],   E(i, j-1) + g[y_j] )
//   wed(x, y) = E(n-1, m-1)            wed(x, "") = E(n-1, -1)            wed("", "") = 0.0
//
// All arithmetic is float64.  Every cell is the min of three sums of fixed operands; min is exact and the additions are
// commutative, so any evaluation order gives the same bits: the kernel equals the sequential double loop bit for bit.  S is
// symmetric bit for bit, so the transposed matrix holds the same cells, wed(x, y) == wed(y, x) exactly, and the kernel is free to
// put the LONGER string of a pair on the lanes.  This is ERP's recurrence (seqdp.hip) with another source of costs: row -1 and
// column -1 are running sums, which no scan across lanes reproduces, so the loader (ctx.hip) sums them once per data set,
// sequentially, into `gapsum` -- gapsum[off + i] = E(i, -1) of that member -- and the kernel only loads them.
//
// k_wed<R, G, MAXT> follows k_seqdp's schedule: one pair per group of G lanes, 64 / G pairs per wavefront.  Lane l of a group keeps rows
// l R .. l R + R - 1 of its pair: per row the code of x (kept as code x 8, the byte offset of its g in LDS), the cell of the column
// it worked on last and g[x_i] (the widest shape reads g[x_i] from LDS instead: see KEEP_GX).  At step s it works on column s - l: the current code of y moves down the lanes one lane per
// step by DPP wave_shr:1 -- ONE 32-bit move, where ERP moves a double -- so a group sweeps anti-diagonals, and the bottom cell of
// lane l - 1 is the top boundary of lane l one step later (and its diagonal boundary the step after).  Lane 0 of a group is fed
// from a strip of G codes of y with the matching E(-1, .) (one per lane, loaded a block of G steps ahead) that moves UP the lanes
// by wave_shl:1.  g[y_j] is looked up once per step and lane; it does not ride along.
//
// The cost table lives in LDS: each block copies g and then S, (A + A A) doubles, into dynamic LDS once, before its grid-stride
// loop, followed by the kernel's only __syncthreads(); after it the waves run independent trip counts and the loop stays
// wave-uniform for the DPP moves.  The layout is g [A] followed by the square table with stride A -- code A-1 as row and column is
// entry A + A A - 1, the last of the image -- so a cell is one 8-byte LDS read at byte (code x 8) A + (8 A + code y 8): one 24-bit
// multiply-add from what the lane holds, then three additions and two minima.  8 (A + A A) bytes per block: 160 B at A = 4, 5616 B at
// A = 26, 132 096 B (129 KiB, one block per CU; hipFuncAttributeMaxDynamicSharedMemorySize) at A = 128.  Small tables keep several
// blocks of PAIR_THREADS threads per CU; a large one is shared by one block of up to MAXT threads (launch_shape).
//
// Empty strings are members.  n >= m after the swap; with m = 0 the sweep has no step (decided before it, per pair: the other
// pairs of the wavefront run on and every lane stays on for the DPP moves) and the result is what column -1 holds, E(n-1, -1), or
// 0.0 when both are empty.  Every index into the pool is clamped to 0 .. len-1 from BOTH sides: an empty member's clamped index is
// 0, and the loader ends the pool and `gapsum` with one slack entry, so that address is valid even for an empty last member.
// No atomics; waves take pairs grid-stride; results leave by plain vector stores.  Work per pair: (m + ceil(n / R) - 1) steps of
// R cells.
//
// k_affine<R, G, MAXT> is the same sweep under affine gap costs (Gotoh's three states): a run of k symbols against a gap costs
// open + the sum of their g, not k independent indels.  o = open, a finite double >= 0 (the kernel's argument), strings of 0 .. 1024:
//
//   H(-1,-1) = 0     P(-1, j) = +inf     Q(i, -1) = +inf     P(-1,-1) = Q(-1,-1) = +inf
//   P(i, j) = min( P(i-1, j), H(i-1, j) + o ) + g[x_i]                                     (x_i against a gap)
//   Q(i, j) = min( Q(i, j-1), H(i, j-1) + o ) + g[y_j]                                     (y_j against a gap)
//   H(i, j) = min( H(i-1, j-1) + S[x_i][y_j],   P(i, j),   Q(i, j) )
//   affine(x, y) = H(n-1, m-1)          affine(x, "") = P(n-1, -1) = ((o + g[x_0]) + g[x_1]) + ...          affine("", "") = 0.0
//
// Again every cell is a min of sums of fixed operands, so any order gives the same bits; the transposed matrix swaps P and Q and
// holds the same H, so affine(x, y) == affine(y, x) exactly and the longer string goes on the lanes here too.  With o = 0.0 the
// value is wed's bit for bit (H + 0.0 == H and P(i-1, j) >= H(i-1, j)).  Column -1 and row -1 are H = P (resp. Q) = the running
// sum that STARTS FROM o: for this metric the loader puts that into `gapsum`, and the kernel only loads it.  Beside what k_wed
// keeps per row -- code x 8, the H of the column it worked on last, g[x_i] -- a lane keeps the Q of that column, +inf at first.
// P is never stored: it flows down the rows inside a step and crosses to the lane below beside the bottom H, so TWO doubles move
// per step on lane_down; lane 0's top is H = E(-1, s) from the strip with P = +inf, and the diagonal boundary tracks H only.  Per
// cell 5 additions and 4 minima (H + o is recomputed for the row below and for the next column: keeping it costs R more doubles)
// against wed's 3 and 2.  The limit of 1024 is the registers': R = 32 cannot hold q[32] beside d[32].
//
// k_osa<R, G, MAXT> is the same sweep with a fourth term, the swap of two adjacent symbols at the cost T (the kernel's argument; a
// double >= 0, +inf for "no transpositions"), strings of 0 .. 1024.  This is OPTIMAL STRING ALIGNMENT -- no substring is edited
// twice -- not the unrestricted Damerau-Levenshtein distance, whose cells read arbitrarily far back:
//
//   E(i, j) = min( wed's three terms,   E(i-2, j-2) + T   if i >= 1 and j >= 1 and x_i == y_{j-1} and x_{i-1} == y_j )
//
// Row -1 and column -1 are legal sources of the fourth term (i = 1, j = 1 reads E(-1, -1) = 0).  The condition is symmetric in the
// two strings, so osa(x, y) == osa(y, x) exactly and the longer string stays on the lanes; with T = +inf the value is wed's bit
// for bit (min(v, E + inf) = v).  Beside what k_wed keeps per row a lane keeps d2[r], the cell of that row TWO columns back, E(row,
// j-2) while the lane is on column j; it takes d[r] as the column is finished, and row r reads the OLD d2[r-2], so two values are
// carried down the unrolled row loop.  Rows 0 and 1 of a lane read E(l R - 2, j-2) and E(l R - 1, j-2).  The second is `top` two
// steps ago (top_prev2 beside top_prev).  The first needs a second word on the boundary: the lane above sends its d[R-2] down
// beside `bottom`, TWO doubles per step on lane_down as in k_affine, and the receiver keeps the two values before the newest.
// Before a lane's first step what arrives is column -1 of the lane above, which is what columns 0 and 1 need.  x_{i-1} of a
// lane's row 0 is the last code of the lane above, moved down once before the step loop (lane 0: a sentinel that matches no code,
// so row 0 never transposes: row -2 does not exist); y_{j-1} is the lane's `ycur` of the step before, kept in a register and
// replaced by a second sentinel while the lane is on column 0.  The two codes of a row and the two of a column are packed into
// one word each, so the condition is one integer compare per cell.  The term is a select, not a branch: match ? src + T : +inf.
// Per cell 4 additions and 3 minima, one integer compare, a 64-bit select (two v_cndmask) and the 64-bit move that ages d[r]
// into d2[r].  The limit of 1024 is the registers', as for k_affine.
#include <algorithm>

#include "pairkern.h"

#define WED_MAXLEN 2048
#define WED_MAX_ALPHABET 128

struct WedArgs : PairArgs {
    const uint8_t *sym;         // codes, the members end to end
    const int32_t *off, *len;   // counted in symbols
    const double *gapsum;       // [symbols of the pool + 1] E(i, -1) of each member
    const double *table;        // g [A], then S [A][A]
    int A;
    double open;                // k_affine: the cost of opening a gap; k_osa: T, the cost of a transposition; k_wed: unused
};

// the 32-bit forms of pairkern.h's lane shifts
__device__ __forceinline__ int lane_down_i(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false); }
__device__ __forceinline__ int lane_up_i(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x130 /* wave_shl:1 */, 0xf, 0xf, false); }

// index k of a member of `len` symbols, clamped to its symbols; 0 for an empty member
__device__ __forceinline__ int wed_at(int k, int len) { return max(min(k, len - 1), 0); }

extern __shared__ double wed_lds[];   // g [A], then S [A][A]

__device__ __forceinline__ double wed_ld(const char *lds, int byte) { return *reinterpret_cast<const double *>(lds + byte); }

template <int R, int G, int MAXT> __global__ __launch_bounds__(MAXT) void k_wed(WedArgs a)
{
    constexpr int PPW = ANN_WAVE / G;   // pairs per wavefront
    const int A = a.A;
    for (int k = threadIdx.x; k < A + A * A; k += blockDim.x) wed_lds[k] = a.table[k];
    __syncthreads();   // (the only one: from here on the waves of a block go their own ways)
    const char *lds = reinterpret_cast<const char *>(wed_lds);
    const int A8 = A * 8;   // bytes of g, which S follows
    const int lane = threadIdx.x & (ANN_WAVE - 1), gl = lane & (G - 1), slot = lane / G;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / ANN_WAVE;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / ANN_WAVE;
    for (int64_t base = wave * PPW; base < a.n; base += nwaves * PPW) {   // (wave-uniform: the DPP moves run with every lane on)
        const int64_t t = base + slot;
        const PairSlot ps = pair_decode(a, t);
        int n = a.len[ps.i], m = a.len[ps.j];
        const uint8_t *x = a.sym + a.off[ps.i], *y = a.sym + a.off[ps.j];
        const double *gsx = a.gapsum + a.off[ps.i], *gsy = a.gapsum + a.off[ps.j];   // E(., -1) of the string on the lanes, E(-1, .) of the other
        if (n < m) {   // the longer string on the lanes
            const uint8_t *p = x; x = y; y = p;
            const double *q = gsx; gsx = gsy; gsy = q;
            const int k = n; n = m; m = k;
        }
        // the widest shape keeps no indel costs of its rows: 32 more doubles put the kernel past the 256 registers a wave addresses
        // directly and at one wave per SIMD; it reads g[x_i] from LDS with the cell's S, at the address it holds anyway
        constexpr bool KEEP_GX = R <= 16;
        int xc[R];              // code of the row x 8: the byte offset of its g, and 1 / A of its row's in S
        double d[R], gxr[KEEP_GX ? R : 1];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int row = wed_at(gl * R + r, n);   // (rows >= n: cells nobody reads)
            xc[r] = x[row] * 8;
            if constexpr (KEEP_GX) gxr[r] = wed_ld(lds, xc[r]);
            d[r] = gsx[row];                          // column -1: E(row, -1)
        }
        // an empty shorter string: no step, the result is column -1's entry (the lane of row n - 1 holds it), 0.0 under n = 0
        int steps = m > 0 ? m + (n - 1) / R : 0;   // the lane of row n - 1 works on column m - 1 at step m - 1 + (n - 1) / R
#pragma unroll
        for (int o = G; o < ANN_WAVE; o <<= 1) steps = max(steps, __shfl_xor(steps, o));
        int ycur = 0, ynext = y[wed_at(gl, m)], ybuf;
        double gnext = gsy[wed_at(gl, m)], gbuf;       // the strip's E(-1, .), beside its codes of y
        double bottom = d[R - 1];                      // E(l R + R - 1, -1): the lane below takes it as its diagonal boundary at column 0
        double top_prev = 0.0;                         // lane 0's diagonal boundary at column 0 is the cell (-1, -1) = 0
        for (int s0 = 0; s0 < steps; s0 += G) {
            const int at = wed_at(s0 + G + gl, m);
            ybuf = ynext;                              // y[s0 + gl]
            ynext = y[at];                             // the next block's, on its way while this block runs
            gbuf = gnext;                              // E(-1, s0 + gl)
            gnext = gsy[at];
            const int s1 = min(s0 + G, steps);
            for (int s = s0; s < s1; ++s) {
                double top = lane_down(bottom);
                const int yv = lane_down_i(ycur);
                ycur = gl == 0 ? ybuf : yv;            // lane 0: y[s]
                ybuf = lane_up_i(ybuf);
                if (gl == 0) top = gbuf;               // row -1: E(-1, s)
                gbuf = lane_up(gbuf);
                const double diag = top_prev;
                top_prev = top;
                const int jc = s - gl;                 // this lane's column
                if (jc >= 0 && jc < m) {
                    const double gy = wed_ld(lds, ycur * 8);
                    const int yo = A8 + ycur * 8;      // S[0][y]
                    double up = top, dg = diag;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const double left = d[r];
                        const double gx = KEEP_GX ? gxr[r] : wed_ld(lds, xc[r]);
                        const double v = fmin(fmin(dg + wed_ld(lds, __mul24(xc[r], A) + yo), up + gx), left + gy);
                        dg = left;
                        up = v;
                        d[r] = v;
                    }
                    bottom = up;
                }
            }
        }
        double res = 0.0;   // n = 0 (then m = 0 too)
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r == (n - 1) % R) res = d[r];
        if (ps.active && gl == max(n - 1, 0) / R) pair_store(a, t, ps.opos, res);
    }
}

#define AFFINE_MAXLEN 1024
#define AFFINE_MAXT16 512   // blocks of the (16, 64) shape

// k_wed's sweep with the three states of an affine gap: what differs is marked (affine)
template <int R, int G, int MAXT> __global__ __launch_bounds__(MAXT) void k_affine(WedArgs a)
{
    constexpr int PPW = ANN_WAVE / G;   // pairs per wavefront
    const int A = a.A;
    for (int k = threadIdx.x; k < A + A * A; k += blockDim.x) wed_lds[k] = a.table[k];
    __syncthreads();   // (the only one: from here on the waves of a block go their own ways)
    const char *lds = reinterpret_cast<const char *>(wed_lds);
    const int A8 = A * 8;   // bytes of g, which S follows
    const double go = a.open;
    const double inf = __builtin_huge_val();
    const int lane = threadIdx.x & (ANN_WAVE - 1), gl = lane & (G - 1), slot = lane / G;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / ANN_WAVE;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / ANN_WAVE;
    for (int64_t base = wave * PPW; base < a.n; base += nwaves * PPW) {   // (wave-uniform: the DPP moves run with every lane on)
        const int64_t t = base + slot;
        const PairSlot ps = pair_decode(a, t);
        int n = a.len[ps.i], m = a.len[ps.j];
        const uint8_t *x = a.sym + a.off[ps.i], *y = a.sym + a.off[ps.j];
        const double *gsx = a.gapsum + a.off[ps.i], *gsy = a.gapsum + a.off[ps.j];   // H(., -1) of the string on the lanes, H(-1, .) of the other
        if (n < m) {   // the longer string on the lanes
            const uint8_t *p = x; x = y; y = p;
            const double *q = gsx; gsx = gsy; gsy = q;
            const int k = n; n = m; m = k;
        }
        int xc[R];              // code of the row x 8: the byte offset of its g, and 1 / A of its row's in S
        double h[R], q[R], gxr[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int row = wed_at(gl * R + r, n);   // (rows >= n: cells nobody reads)
            xc[r] = x[row] * 8;
            gxr[r] = wed_ld(lds, xc[r]);
            h[r] = gsx[row];                          // column -1: H(row, -1) = P(row, -1), the sum that starts from o
            q[r] = inf;                               // (affine) Q(row, -1)
        }
        // an empty shorter string: no step, the result is column -1's entry (the lane of row n - 1 holds it), 0.0 under n = 0
        int steps = m > 0 ? m + (n - 1) / R : 0;   // the lane of row n - 1 works on column m - 1 at step m - 1 + (n - 1) / R
#pragma unroll
        for (int o = G; o < ANN_WAVE; o <<= 1) steps = max(steps, __shfl_xor(steps, o));
        int ycur = 0, ynext = y[wed_at(gl, m)], ybuf;
        double gnext = gsy[wed_at(gl, m)], gbuf;       // the strip's H(-1, .), beside its codes of y
        double bottom = h[R - 1];                      // H(l R + R - 1, -1): the lane below takes it as its diagonal boundary at column 0
        double bottom_p = inf;                         // (affine) P of the bottom row at the column worked on last; read only after a step wrote it
        double top_prev = 0.0;                         // lane 0's diagonal boundary at column 0 is the cell (-1, -1) = 0
        for (int s0 = 0; s0 < steps; s0 += G) {
            const int at = wed_at(s0 + G + gl, m);
            ybuf = ynext;                              // y[s0 + gl]
            ynext = y[at];                             // the next block's, on its way while this block runs
            gbuf = gnext;                              // H(-1, s0 + gl)
            gnext = gsy[at];
            const int s1 = min(s0 + G, steps);
            for (int s = s0; s < s1; ++s) {
                double top = lane_down(bottom);
                double top_p = lane_down(bottom_p);    // (affine) the second word of the boundary between lanes
                const int yv = lane_down_i(ycur);
                ycur = gl == 0 ? ybuf : yv;            // lane 0: y[s]
                ybuf = lane_up_i(ybuf);
                if (gl == 0) { top = gbuf; top_p = inf; }   // row -1: H(-1, s), P(-1, s) = +inf
                gbuf = lane_up(gbuf);
                const double diag = top_prev;
                top_prev = top;
                const int jc = s - gl;                 // this lane's column
                if (jc >= 0 && jc < m) {
                    const double gy = wed_ld(lds, ycur * 8);
                    const int yo = A8 + ycur * 8;      // S[0][y]
                    double up = top, up_p = top_p, dg = diag;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const double left = h[r];
                        const double p = fmin(up_p, up + go) + gxr[r];
                        const double qq = fmin(q[r], left + go) + gy;
                        const double v = fmin(fmin(dg + wed_ld(lds, __mul24(xc[r], A) + yo), p), qq);
                        dg = left;
                        up = v;
                        up_p = p;
                        h[r] = v;
                        q[r] = qq;
                    }
                    bottom = up;
                    bottom_p = up_p;
                }
            }
        }
        double res = 0.0;   // n = 0 (then m = 0 too)
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r == (n - 1) % R) res = h[r];
        if (ps.active && gl == max(n - 1, 0) / R) pair_store(a, t, ps.opos, res);
    }
}

#define OSA_MAXLEN 1024
#define OSA_MAXT16 512   // blocks of the (16, 64) shape

// k_wed's sweep with the swap of two adjacent symbols as a fourth term: what differs is marked (osa)
template <int R, int G, int MAXT> __global__ __launch_bounds__(MAXT) void k_osa(WedArgs a)
{
    static_assert(R >= 2, "rows 0 and 1 of a lane take their sources from the lane above");
    constexpr int PPW = ANN_WAVE / G;   // pairs per wavefront
    const int A = a.A;
    for (int k = threadIdx.x; k < A + A * A; k += blockDim.x) wed_lds[k] = a.table[k];
    __syncthreads();   // (the only one: from here on the waves of a block go their own ways)
    const char *lds = reinterpret_cast<const char *>(wed_lds);
    const int A8 = A * 8;   // bytes of g, which S follows
    const double T = a.open;   // (osa) the cost of a transposition; +inf: none
    const double inf = __builtin_huge_val();
    const int lane = threadIdx.x & (ANN_WAVE - 1), gl = lane & (G - 1), slot = lane / G;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / ANN_WAVE;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / ANN_WAVE;
    for (int64_t base = wave * PPW; base < a.n; base += nwaves * PPW) {   // (wave-uniform: the DPP moves run with every lane on)
        const int64_t t = base + slot;
        const PairSlot ps = pair_decode(a, t);
        int n = a.len[ps.i], m = a.len[ps.j];
        const uint8_t *x = a.sym + a.off[ps.i], *y = a.sym + a.off[ps.j];
        const double *gsx = a.gapsum + a.off[ps.i], *gsy = a.gapsum + a.off[ps.j];   // E(., -1) of the string on the lanes, E(-1, .) of the other
        if (n < m) {   // the longer string on the lanes
            const uint8_t *p = x; x = y; y = p;
            const double *q = gsx; gsx = gsy; gsy = q;
            const int k = n; n = m; m = k;
        }
        int xc[R];              // code of the row x 8: the byte offset of its g, and 1 / A of its row's in S
        double d[R], d2[R], gxr[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int row = wed_at(gl * R + r, n);   // (rows >= n: cells nobody reads)
            xc[r] = x[row] * 8;
            gxr[r] = wed_ld(lds, xc[r]);
            d[r] = gsx[row];                          // column -1: E(row, -1)
            d2[r] = inf;                              // (osa) E(row, j - 2): read from column 1 on, when it holds column -1
        }
        // (osa) x of the row above this lane's first: the last code of the lane above; lane 0 has none and matches nothing.  The
        // move comes first and on its own: inside the ?: it would run with lane 0 off, and lane 1 would read its own value
        const int xmoved = lane_down_i(xc[R - 1]);
        const int xabove = gl == 0 ? 0xfff8 : xmoved;
        // (osa) both halves of the condition in ONE compare per cell: a row's key is its code x 8 with the code x 8 of the row above
        // in the high half; a column's key, per step, is y_{j-1} x 8 with y_j x 8 in the high half.  Codes x 8 stay below 1024, so
        // the two sentinels, 0xfff8 and 0xfff0, equal no code and the halves do not touch
        int xk[R];
#pragma unroll
        for (int r = 0; r < R; ++r) xk[r] = xc[r] | ((r == 0 ? xabove : xc[r - 1]) << 16);
        // an empty shorter string: no step, the result is column -1's entry (the lane of row n - 1 holds it), 0.0 under n = 0
        int steps = m > 0 ? m + (n - 1) / R : 0;   // the lane of row n - 1 works on column m - 1 at step m - 1 + (n - 1) / R
#pragma unroll
        for (int o = G; o < ANN_WAVE; o <<= 1) steps = max(steps, __shfl_xor(steps, o));
        int ycur = 0, ynext = y[wed_at(gl, m)], ybuf;
        double gnext = gsy[wed_at(gl, m)], gbuf;       // the strip's E(-1, .), beside its codes of y
        double bottom = d[R - 1];                      // E(l R + R - 1, -1): the lane below takes it as its diagonal boundary at column 0
        double top_prev = 0.0;                         // lane 0's diagonal boundary at column 0 is the cell (-1, -1) = 0
        double top_prev2 = inf;                        // (osa) `top` two steps ago: E(l R - 1, j - 2); first read at column 1
        double top2_prev = inf, top2_prev2 = inf;      // (osa) the second boundary word one and two steps ago: E(l R - 2, j - 2)
        for (int s0 = 0; s0 < steps; s0 += G) {
            const int at = wed_at(s0 + G + gl, m);
            ybuf = ynext;                              // y[s0 + gl]
            ynext = y[at];                             // the next block's, on its way while this block runs
            gbuf = gnext;                              // E(-1, s0 + gl)
            gnext = gsy[at];
            const int s1 = min(s0 + G, steps);
            for (int s = s0; s < s1; ++s) {
                double top = lane_down(bottom);
                const double top2 = lane_down(d[R - 2]);   // (osa) the second word of the boundary between lanes: E(l R - 2, .)
                const int yv = lane_down_i(ycur);
                const int yprev = ycur;                // (osa) y_{j-1}, where this lane's column j is >= 1
                ycur = gl == 0 ? ybuf : yv;            // lane 0: y[s]
                ybuf = lane_up_i(ybuf);
                if (gl == 0) top = gbuf;               // row -1: E(-1, s)
                gbuf = lane_up(gbuf);
                const double diag = top_prev;
                const double src0 = top2_prev2, src1 = top_prev2;   // (osa) E(l R - 2, j - 2) and E(l R - 1, j - 2)
                top_prev2 = top_prev;
                top_prev = top;
                top2_prev2 = top2_prev;
                top2_prev = top2;
                const int jc = s - gl;                 // this lane's column
                if (jc >= 0 && jc < m) {
                    const double gy = wed_ld(lds, ycur * 8);
                    const int yo = A8 + ycur * 8;      // S[0][y]
                    const int yk = (jc >= 1 ? yprev * 8 : 0xfff0) | (ycur * 8 << 16);   // (osa) column 0 has no y_{j-1}: a sentinel
                    double up = top, dg = diag;
                    double t0 = src0, t1 = src1;       // (osa) the old d2 of the two rows above
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const double left = d[r];
                        double v = fmin(fmin(dg + wed_ld(lds, __mul24(xc[r], A) + yo), up + gxr[r]), left + gy);
                        const bool swap = xk[r] == yk;   // (osa) x_i == y_{j-1} and x_{i-1} == y_j
                        v = fmin(v, swap ? t0 + T : inf);
                        t0 = t1;
                        t1 = d2[r];
                        d2[r] = left;
                        dg = left;
                        up = v;
                        d[r] = v;
                    }
                    bottom = up;
                }
            }
        }
        double res = 0.0;   // n = 0 (then m = 0 too)
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r == (n - 1) % R) res = d[r];
        if (ps.active && gl == max(n - 1, 0) / R) pair_store(a, t, ps.opos, res);
    }
}

// MAXT: the largest block the shape's registers allow (1024 threads: 128 VGPRs per lane, 512: 256).  A block is PAIR_THREADS threads unless the
// table leaves room for fewer than four of those on a CU; then it is MAXT, and up to MAXT / 64 waves share the one copy a CU holds.
enum { WED_PLAIN, WED_AFFINE, WED_OSA };   // the three kernels of this file

template <int KIND, int R, int G, int MAXT> static int launch_shape(annchor_ctx *c, const WedArgs &a)
{
    static_assert(R * G <= WED_MAXLEN && (G & (G - 1)) == 0 && G <= ANN_WAVE, "a group holds R x G rows");
    static_assert(MAXT % PAIR_THREADS == 0 && MAXT <= 1024, "blocks are whole multiples of PAIR_THREADS");
    void (*kernel)(WedArgs);   // (if constexpr: a shape instantiates the one kernel it runs)
    if constexpr (KIND == WED_AFFINE) kernel = k_affine<R, G, MAXT>;
    else if constexpr (KIND == WED_OSA) kernel = k_osa<R, G, MAXT>;
    else kernel = k_wed<R, G, MAXT>;
    const char *name = KIND == WED_AFFINE ? "affine_gap" : KIND == WED_OSA ? "osa" : "weighted_levenshtein";
    const size_t lds = sizeof(double) * ((size_t)a.A * a.A + a.A);
    const size_t lds_cu = 160 * 1024;
    ANN_REQUIRE(c, lds <= lds_cu, ANNCHOR_ELIMIT, "%s: alphabet %d needs %zu B of LDS (> 160 KiB)", name, a.A, lds);
    if (lds > 64 * 1024)
        ANN_CHECK_HIP(c, hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int threads = 4 * lds > lds_cu ? MAXT : PAIR_THREADS;
    // every block copies the table first: no more blocks than four rounds of what a CU holds at a time
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(2048 / threads, (int64_t)(lds_cu / lds)));
    const int64_t cap = (int64_t)c->prop.multiProcessorCount * 4 * per_cu;
    const int64_t blocks = ((int64_t)pair_grid(c, a.n, G) + threads / PAIR_THREADS - 1) / (threads / PAIR_THREADS);
    kernel<<<(int)std::min(blocks, cap), threads, lds, c->stream>>>(a);
    ANN_CHECK_HIP(c, hipGetLastError());
    return ANNCHOR_OK;
}

// the three string metrics: the kernel follows the bound metric, the shape the data set's longest string
int ann_wed_launch(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    if (src.n == 0) return ANNCHOR_OK;
    const bool affine = c->metric == ANNCHOR_METRIC_AFFINE_GAP, osa = c->metric == ANNCHOR_METRIC_OSA;
    const char *name = affine ? "affine_gap" : osa ? "osa" : "weighted_levenshtein";
    const int limit = affine ? AFFINE_MAXLEN : osa ? OSA_MAXLEN : WED_MAXLEN;
    ANN_REQUIRE(c, c->wedtab.p != nullptr && c->gapsum.p != nullptr, ANNCHOR_EINVAL, "%s: no cost table bound to this context", name);
    ANN_REQUIRE(c, c->alphabet >= 1 && c->alphabet <= WED_MAX_ALPHABET, ANNCHOR_ELIMIT, "%s: alphabet %d outside 1..%d", name,
                c->alphabet, WED_MAX_ALPHABET);
    ANN_REQUIRE(c, c->maxlen >= 0 && c->maxlen <= limit, ANNCHOR_ELIMIT, "string length %d outside 0..%d", c->maxlen, limit);
    WedArgs a;
    pair_fill(a, src, d_out, d_RA, d_ncm);
    a.sym = c->sym.as<uint8_t>();
    a.off = c->soff.as<int32_t>(); a.len = c->slen.as<int32_t>();
    a.gapsum = c->gapsum.as<double>();
    a.table = c->wedtab.as<double>();
    a.A = c->alphabet;
    a.open = osa ? c->osa_transpose : c->affine_open;
    ProfScope ps(c, affine ? "affine_gap_pairs" : osa ? "osa_pairs" : "weighted_levenshtein_pairs", (double)src.n * (2.0 * c->maxlen * (1 + sizeof(double)) + 16));
    // by the data set's longest string: 4 pairs per wavefront up to 128 symbols, one pair on 64 lanes beyond
    if (affine) {
        if (c->maxlen <= 8 * 16) return launch_shape<WED_AFFINE, 8, 16, 1024>(c, a);
        if (c->maxlen <= 8 * 64) return launch_shape<WED_AFFINE, 8, 64, 1024>(c, a);
        return launch_shape<WED_AFFINE, 16, 64, AFFINE_MAXT16>(c, a);
    }
    if (osa) {
        if (c->maxlen <= 8 * 16) return launch_shape<WED_OSA, 8, 16, 1024>(c, a);
        if (c->maxlen <= 8 * 64) return launch_shape<WED_OSA, 8, 64, 1024>(c, a);
        return launch_shape<WED_OSA, 16, 64, OSA_MAXT16>(c, a);
    }
    if (c->maxlen <= 8 * 16) return launch_shape<WED_PLAIN, 8, 16, 1024>(c, a);
    if (c->maxlen <= 8 * 64) return launch_shape<WED_PLAIN, 8, 64, 1024>(c, a);
    return launch_shape<WED_PLAIN, 32, 64, 512>(c, a);
}
