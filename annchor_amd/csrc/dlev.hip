// dlev.hip -- the unrestricted Damerau-Levenshtein distance between strings over a pair list, at unit costs: insert, delete,
// substitute and the swap of two adjacent symbols, where a swapped pair may be edited again (no reference counterpart).  Unlike
// optimal string alignment (wed.hip, k_osa) it is a true metric: dl("ca", "abc") = 2, where osa gives 3.
//
//   strings of 0 .. DLEV_MAXLEN 16-bit codes; only the equality of two codes matters, so there is no table and no alphabet limit
//
//   H(-1,-1) = 0     H(i,-1) = i + 1     H(-1,j) = j + 1
//   k = the largest k' < i with x[k'] == y[j]      l = the largest l' < j with y[l'] == x[i]
//   H(i,j) = min( H(i-1,j-1) + (x[i] != y[j]),   H(i-1,j) + 1,   H(i,j-1) + 1,
//                 H(k-1,l-1) + (i-k-1) + 1 + (j-l-1)        if k and l both exist )
//   dl(x,y) = H(n-1,m-1)      dl(x,"") = n      dl("","") = 0
//
// (Lowrance and Wagner 1975.)  The value is a small integer; every cell is a min of integer sums, so any evaluation order gives
// the same value, and the recurrence is symmetric in the two strings: the longer one goes on the lanes, as in wed.hip.
//
// The fourth term reads arbitrarily far back, which is why k_osa stopped short of it.  At unit costs it reduces to running
// values (Zhao and Sahni's linear-space form): the term can lower a cell only when one of the two matches is adjacent,
//   (a) l == j-1:  H(k-1, j-2) + (i-k)          (b) k == i-1:  H(i-2, l-1) + (j-l)
// (with k < i-1 and l < j-1 the term never undercuts what the three plain terms reach; DESIGN 3.15c has the check against the
// full-matrix loop).  So beside left, up and diag a cell needs
//   per COLUMN j, flowing down the rows:  K(j), the last row whose symbol equals y[j], and F(j) = H(K(j)-1, j-2)
//   per ROW i, flowing along the columns: L(i), the last column whose symbol equals x[i], and T(i) = H(i-2, L(i)-1)
// all four updated where x[i] == y[j]: F <- H(i-1, j-2), K <- i, T <- H(i-2, j-1), L <- j.  A large integer in F and T and a
// far-away index in K and L stand for "no such row / column"; the terms they form are too large to win.
//
// k_dlev<R, G, MAXT> follows k_wed's schedule: one pair per group of G lanes, 64 / G pairs per wavefront; lane l of a group keeps
// rows l R .. l R + R - 1 and works on column s - l at step s; y's code moves down one lane per step by DPP wave_shr:1; lane 0 is
// fed from a strip of G codes that moves up the lanes.  What is its own: cells are 32-bit integers, there is no cost table, no
// LDS and no barrier, and row -1 / column -1 are index + 1, formed in the kernel.  Per row a lane keeps the code, d = H(row, the
// column worked on last), d2 = H(row, the column before that), T and L -- 5 R registers.  Inside the unrolled row loop H(i-1, j-2)
// is the OLD d2 of the row above and H(i-2, j-1) the OLD d of the row two above: two values carried down the loop.  The column
// state F, K enters a lane from the lane above and leaves it at the bottom row, so FOUR words cross each lane boundary per step:
// the bottom cell, d[R-2] (rows 0 and 1 of the lane below read two rows up), F and K.  The receiver keeps `top` one and two steps
// back (H(l R - 1, j-1) = diag and H(l R - 1, j-2)) and the second word one step back (H(l R - 2, j-1)).  K travels relative to
// the sending lane's first row, so the receiver subtracts R and a row compares it with its own r - 1, a constant of the unrolled
// loop.  Lane 0 takes top = j + 1, F = none, K = none: no row above exists.  Before a lane's first step what arrives is column
// -1 of the lane above, which is what column 0 needs; `top` two steps back is then not H(., -2), but F(0) is never read (case (a)
// at column 0 would need L = -1).  Both extra terms are selects, not branches, and the step loop stays wave-uniform for the DPP
// moves.  Rows >= n compute cells nobody reads: every state flows down or along its own row.
#include <algorithm>

#include "pairkern.h"

struct DlevArgs : PairArgs {
    const uint16_t *sym;        // codes, the members end to end; one slack entry at the end
    const int32_t *off, *len;   // counted in symbols
};

#define DLEV_BIG (1 << 20)      // "no such cell" in F and T; real cells stay below 2 DLEV_MAXLEN
#define DLEV_NONE (-(1 << 20))  // "no such row / column" in K and L

// lane l receives lane l - 1's value (lane 0 of the wavefront keeps its own) / lane l + 1's (lane 63 keeps its own)
__device__ __forceinline__ int dlev_down(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false); }
__device__ __forceinline__ int dlev_up(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x130 /* wave_shl:1 */, 0xf, 0xf, false); }

// index k of a member of `len` symbols, clamped to its symbols; 0 for an empty member (the pool's slack entry keeps that valid)
__device__ __forceinline__ int dlev_at(int k, int len) { return max(min(k, len - 1), 0); }

template <int R, int G, int MAXT> __global__ __launch_bounds__(MAXT) void k_dlev(DlevArgs a)
{
    static_assert(R >= 2, "rows 0 and 1 of a lane take their sources from the lane above");
    constexpr int PPW = ANN_WAVE / G;   // pairs per wavefront
    const int lane = threadIdx.x & (ANN_WAVE - 1), gl = lane & (G - 1), slot = lane / G;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / ANN_WAVE;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / ANN_WAVE;
    for (int64_t base = wave * PPW; base < a.n; base += nwaves * PPW) {   // (wave-uniform: the DPP moves run with every lane on)
        const int64_t t = base + slot;
        const PairSlot ps = pair_decode(a, t);
        int n = a.len[ps.i], m = a.len[ps.j];
        const uint16_t *x = a.sym + a.off[ps.i], *y = a.sym + a.off[ps.j];
        if (n < m) {   // the longer string on the lanes
            const uint16_t *p = x; x = y; y = p;
            const int k = n; n = m; m = k;
        }
        int xc[R], d[R], d2[R], T[R], L[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            xc[r] = x[dlev_at(gl * R + r, n)];   // (rows >= n: cells nobody reads)
            d[r] = gl * R + r + 1;               // column -1: H(row, -1)
            d2[r] = DLEV_BIG;                    // H(row, -2); from column 1 on it holds a real column
            T[r] = DLEV_BIG;
            L[r] = DLEV_NONE;
        }
        // an empty shorter string: no step, the result is column -1's entry (the lane of row n - 1 holds it), 0 under n = 0
        int steps = m > 0 ? m + (n - 1) / R : 0;   // the lane of row n - 1 works on column m - 1 at step m - 1 + (n - 1) / R
#pragma unroll
        for (int o = G; o < ANN_WAVE; o <<= 1) steps = max(steps, __shfl_xor(steps, o));
        int ycur = 0, ynext = y[dlev_at(gl, m)], ybuf;
        int bottom = d[R - 1];                     // H(l R + R - 1, -1): the lane below takes it as its diagonal boundary at column 0
        int fbot = DLEV_BIG, kbot = DLEV_NONE;     // the column state below this lane's last row; read only after a step wrote it
        int top_prev = 0;                          // lane 0's diagonal boundary at column 0 is the cell (-1, -1) = 0
        int top_prev2 = DLEV_BIG;                  // `top` two steps ago: H(l R - 1, j - 2)
        int top2_prev = DLEV_BIG;                  // the second boundary word one step ago: H(l R - 2, j - 1)
        for (int s0 = 0; s0 < steps; s0 += G) {
            ybuf = ynext;                          // y[s0 + gl]
            ynext = y[dlev_at(s0 + G + gl, m)];    // the next block's, on its way while this block runs
            const int s1 = min(s0 + G, steps);
            for (int s = s0; s < s1; ++s) {
                // the boundary between lanes, four words; every move on its own, outside any ?: (a move inside one runs with
                // lane 0 masked off)
                int top = dlev_down(bottom);
                const int top2 = dlev_down(d[R - 2]);
                int fin = dlev_down(fbot);
                int kin = dlev_down(kbot);
                const int yv = dlev_down(ycur);
                ycur = gl == 0 ? ybuf : yv;        // lane 0: y[s]
                ybuf = dlev_up(ybuf);
                if (gl == 0) { top = s + 1; fin = DLEV_BIG; kin = DLEV_NONE; }   // row -1: H(-1, s); no row above holds y[s]
                const int diag = top_prev;
                const int src_p2 = top_prev2, src_g2 = top2_prev;
                top_prev2 = top_prev;
                top_prev = top;
                top2_prev = top2;
                const int jc = s - gl;             // this lane's column
                if (jc >= 0 && jc < m) {
                    int up = top, dg = diag;
                    int p2 = src_p2;               // the old d2 of the row above: H(i-1, j-2)
                    int g2 = src_g2;               // the old d of the row two above: H(i-2, j-1)
                    int F = fin, K = kin - R;      // K counts from this lane's first row
                    const int jm1 = jc - 1;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int left = d[r];
                        const bool eq = xc[r] == ycur;
                        const int ca = L[r] == jm1 ? F + (r - K) : DLEV_BIG;         // (a) y[j-1] == x[i]
                        const int cb = K == r - 1 ? T[r] + (jc - L[r]) : DLEV_BIG;   // (b) x[i-1] == y[j]
                        const int v = min(min(min(dg + (eq ? 0 : 1), up + 1), left + 1), min(ca, cb));
                        F = eq ? p2 : F;
                        K = eq ? r : K;
                        T[r] = eq ? g2 : T[r];
                        L[r] = eq ? jc : L[r];
                        p2 = d2[r];
                        g2 = dg;
                        dg = left;
                        d2[r] = left;
                        d[r] = v;
                        up = v;
                    }
                    bottom = up;
                    fbot = F;
                    kbot = K;
                }
            }
        }
        int res = 0;   // n = 0 (then m = 0 too)
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r == (n - 1) % R) res = d[r];
        if (ps.active && gl == max(n - 1, 0) / R) pair_store(a, t, ps.opos, (double)res);
    }
}

template <int R, int G, int MAXT> static int launch_shape(annchor_ctx *c, const DlevArgs &a)
{
    static_assert(R * G <= DLEV_MAXLEN && (G & (G - 1)) == 0 && G <= ANN_WAVE, "a group holds R x G rows");
    static_assert(MAXT >= PAIR_THREADS, "blocks are PAIR_THREADS threads");
    k_dlev<R, G, MAXT><<<pair_grid(c, a.n, G), PAIR_THREADS, 0, c->stream>>>(a);
    ANN_CHECK_HIP(c, hipGetLastError());
    return ANNCHOR_OK;
}

// the shape follows the data set's longest string: 4 pairs per wavefront up to 128 symbols, one pair on 64 lanes beyond
int ann_dlev_launch(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    if (src.n == 0) return ANNCHOR_OK;
    ANN_REQUIRE(c, c->maxlen >= 0 && c->maxlen <= DLEV_MAXLEN, ANNCHOR_ELIMIT, "string length %d outside 0..%d", c->maxlen, DLEV_MAXLEN);
    DlevArgs a;
    pair_fill(a, src, d_out, d_RA, d_ncm);
    a.sym = c->sym.as<uint16_t>();
    a.off = c->soff.as<int32_t>(); a.len = c->slen.as<int32_t>();
    ProfScope ps(c, "damerau_levenshtein_pairs", (double)src.n * (2.0 * c->maxlen * sizeof(uint16_t) + 16));
    if (c->maxlen <= 8 * 16) return launch_shape<8, 16, 1024>(c, a);
    if (c->maxlen <= 8 * 64) return launch_shape<8, 64, 1024>(c, a);
    return launch_shape<32, 64, 512>(c, a);
}
