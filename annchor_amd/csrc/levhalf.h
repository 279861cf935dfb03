// levhalf.h -- what the kernels of lev.hip share around levcol.h's column: staging, the match-mask build, the rows mask of a
// lane's last word, the fused max-min pick, and the forward / backward ("half-chain") machinery of k_lev_a2, k_lev_p2 and
// k_lev_ap -- a lane's place in its wave, the step bounds, the one-deep column walk and the F / B' join.
//
// A half-chain wave holds four chains: the pair (pattern, text) is walked from both ends, the forward half over the first
// h = ceil(n / 2) text columns, the backward half over the other n - h columns of the reversed strings, and the distance is
// min_i F[i] + B'[m - i] over the DP column where they meet.  Packed waves hold two pairs in slots of 16 lanes (the pattern
// has <= 16 words), the others one pair in slots of 32.
//
// Include after common.h (argmax_combine).  Every helper is inlined into its kernel and takes plain values and references.
#pragma once
#include <type_traits>

#include "levcol.h"

#define LEVF_ROW 128   // bytes per symbol row of one half-wave's match-mask table (32 lanes x 4 B)

// LDS traffic of one wave is ordered by the hardware; this only stops the compiler
// from moving LDS accesses of different lanes across the phase boundary.
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// 16-byte copies of a string's `len` symbols (strings start 16-byte aligned and are padded to 16), lanes first, first + stride, ...
__device__ __forceinline__ void lev_stage(uint8_t *dst, const uint8_t *src, int len, int first, int stride = 64)
{
    for (int ch = first; ch < ((len + 15) >> 4); ch += stride) reinterpret_cast<uint4 *>(dst)[ch] = reinterpret_cast<const uint4 *>(src)[ch];
}

// The rows of a pattern of m symbols (Wp words) that word w holds: all 32, the last word's m - 32 (Wp - 1), or none.
__device__ __forceinline__ uint32_t lev_rows_mask(int w, int Wp, int m)
{
    return w < Wp - 1 ? 0xffffffffu : (w == Wp - 1 ? (0xffffffffu >> (31 - ((m - 1) & 31))) : 0u);
}

// Match masks of word w of a pattern of m symbols into this lane's column of PM[half-wave][symbol][lane % 32] (pm_col):
// bit k of PM[c] = (pattern[32 w + k] == c), the pattern read backwards when `reversed`.  Every lane clears its column
// (lanes without a word too: their reads must stay defined).  The column is private to the lane; LDS OR without return:
// the 32 updates go out back to back instead of 32 dependent read-modify-write round trips (370 -> 329 us per 65 536 pairs).
__device__ __forceinline__ void lev_build_masks(unsigned char *pm_col, int A, const uint8_t *pat, int m, int w, bool reversed, bool have)
{
    for (int c = 0; c < A; ++c) *reinterpret_cast<uint32_t *>(pm_col + (size_t)c * LEVF_ROW) = 0u;
    if (have && w < ((m + 31) >> 5)) {
        const int valid = min(32, m - w * 32);
        uint32_t sy[32];
        if (!reversed) {
            const uint4 *p16 = reinterpret_cast<const uint4 *>(pat + w * 32);
            const uint4 q0 = p16[0], q1 = p16[1];
            const uint32_t wd[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
            for (int k = 0; k < 32; ++k) sy[k] = (wd[k >> 2] >> ((k & 3) * 8)) & 0xffu;
        } else {
#pragma unroll
            for (int k = 0; k < 32; ++k) sy[k] = pat[max(m - 1 - (w * 32 + k), 0)];
        }
#pragma unroll
        for (int k = 0; k < 32; ++k)
            if (k < valid) atomicOr(reinterpret_cast<uint32_t *>(pm_col + (size_t)sy[k] * LEVF_ROW), 1u << k);
    }
}

// Fused max-min pick: runmin = min(runmin, row) (or row itself on `reset`) and its first arg-max over the (small) data set,
// by every wave for itself, loads batched BATCH deep; workgroup 0 also stores the running minimum and the anchor.  Other
// workgroups may read runmin[j] before or after that store: min(min(r, d), d) == min(r, d).
template <int BATCH>
__device__ __forceinline__ int lev_fused_pick(const double *row, double *runmin, int32_t *out, int reset, int nx, int lane)
{
    double bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int j0 = 0; j0 < nx; j0 += 64 * BATCH) {
        double d[BATCH], rm[BATCH];
#pragma unroll
        for (int e = 0; e < BATCH; ++e) {
            const int j = min(j0 + e * 64 + lane, nx - 1);
            d[e] = row[j];
            rm[e] = reset ? 0.0 : runmin[j];
        }
#pragma unroll
        for (int e = 0; e < BATCH; ++e) {
            const int j = j0 + e * 64 + lane;
            if (j < nx) {
                const double v = reset ? d[e] : fmin(rm[e], d[e]);
                if (blockIdx.x == 0) runmin[j] = v;
                argmax_combine(bv, bi, v, j);
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        argmax_combine(bv, bi, ov, oi);
    }
    if (blockIdx.x == 0 && lane == 0) *out = bi;
    return bi;
}

// ---- half-chain kernels ----------------------------------------------------------------------------------------------

// A lane's place in a half-chain wave: word w of half `half` (0 forward, 1 backward) of the wave's pair `pair`, which
// spreads over LP lanes.  pair < 2 always: 4 slots of 16 lanes in a packed wave, 2 of 32 (pair 0 alone) otherwise.
struct LevLane {
    int w, pair, half, LP;
    __device__ __forceinline__ void bind(int lane, bool packed)
    {
        const int GL = packed ? 16 : 32;
        const int slot = lane / GL;
        w = lane - slot * GL; pair = slot >> 1; half = slot & 1; LP = packed ? 32 : 64;
    }
};

// The one or two entries of `list` (string ids: lev_order; list positions: the class permutation) that task `task` works
// on: the n_short short entries two to a task (packed waves; .y = -1 for the odd one out), then one task per long entry.
__device__ __forceinline__ bool lev_task_packed(int n_short, int task) { return task < ((n_short + 1) >> 1); }
__device__ __forceinline__ int2 lev_task_entries(const int32_t *list, int n_short, int task)
{
    int2 t = make_int2(-1, -1);
    if (lev_task_packed(n_short, task)) {
        t.x = list[2 * task];
        if (2 * task + 1 < n_short) t.y = list[2 * task + 1];
    } else {
        t.x = list[n_short + (task - ((n_short + 1) >> 1))];
    }
    return t;
}

// Steps of a half's walk, wave-uniform where the loops need them: lane w works on column k - w of its half's `un` columns
// (un = h forward, n - h backward; 0 without a pair or a pattern); columns k_lo <= k < k_hi are in range for every lane of
// every chain of the wave and run unchecked, max_steps ends the longest chain.
struct LevHalfBounds {
    int h;
    uint32_t un;
    int max_steps, k_lo, k_hi;
};
__device__ __forceinline__ LevHalfBounds lev_half_bounds(bool have, int m, int n, int Wp, int half)
{
    LevHalfBounds b;
    const bool walk = have && m > 0;
    b.h = (n + 1) >> 1;
    b.un = walk ? (uint32_t)(half ? n - b.h : b.h) : 0u;
    b.max_steps = walk ? b.h + Wp - 1 : 0;
    b.k_lo = walk ? Wp - 1 : 0;
    b.k_hi = walk ? n - b.h : 0x7fffffff;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        b.max_steps = max(b.max_steps, __shfl_xor(b.max_steps, off));
        b.k_lo = max(b.k_lo, __shfl_xor(b.k_lo, off));
        b.k_hi = min(b.k_hi, __shfl_xor(b.k_hi, off));
    }
    b.max_steps = __builtin_amdgcn_readfirstlane(b.max_steps);
    b.k_lo = min(__builtin_amdgcn_readfirstlane(b.k_lo), b.max_steps);
    b.k_hi = max(b.k_lo, min(__builtin_amdgcn_readfirstlane(b.k_hi), b.max_steps));
    return b;
}

// The walk of k_lev_a2 and k_lev_p2: this lane's word through its half of the text (txt[0 .. n), forward from the front or
// backward from the end), the symbol of column k + 2 and the match mask of column k + 1 in flight while column k computes,
// two unchecked columns per trip.  Leaves the vertical deltas of the half's last column in vp / vn.
template <int CARRY>
__device__ __forceinline__ void lev_half_walk(LevCarry<CARRY> &cs, const unsigned char *pm_col, const uint8_t *txt, int n, int w, int half,
                                              const LevHalfBounds &b, uint32_t &vp, uint32_t &vn)
{
    const int dir = half ? -1 : 1;
    const uint8_t *tp = txt + (half ? n - 1 + w : -w);
    vp = 0xffffffffu; vn = 0u;
    uint32_t c1 = tp[dir];
    uint32_t eq = *reinterpret_cast<const uint32_t *>(pm_col + (uint32_t)tp[0] * LEVF_ROW);
    cs.reset();
    const uint8_t *tnext = tp + 2 * dir;
    auto column = [&](int k, auto checked) {
        uint32_t c2, eq_n;
        constexpr bool CHECKED = decltype(checked)::value;
        lev_column<CARRY, CHECKED>(cs, vp, vn, eq, !CHECKED || (uint32_t)(k - w) < b.un, [&] {
            c2 = *tnext;
            tnext += dir;
            eq_n = *reinterpret_cast<const uint32_t *>(pm_col + c1 * LEVF_ROW);
        });
        eq = eq_n;
        c1 = c2;
    };
    int k = 0;
    for (; k < b.k_lo; ++k) column(k, std::true_type());
    for (; k + 2 <= b.k_hi; k += 2) { column(k, std::false_type()); column(k + 1, std::false_type()); }
    for (; k < b.k_hi; ++k) column(k, std::false_type());
    for (; k < b.max_steps; ++k) column(k, std::true_type());
}

// F / B' (prefix sums of the vertical deltas down this half's rows) into FB[pair][half][fb_stride], then
// min_i F[i] + B'[m - i] per pair, in every lane of the pair.  `rows` = lev_rows_mask of this lane's word, 0 without a pair.
// The caller fences again before FB is rewritten.
__device__ __forceinline__ int lev_half_join(const LevLane &L, int lane, bool have, int m, int n, const LevHalfBounds &b, uint32_t vp,
                                             uint32_t vn, uint32_t rows, int16_t *FB, int fb_stride)
{
    const int part = __popc(vp & rows) - __popc(vn & rows);
    int incl = part;
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) {
        const int o = __shfl_up(incl, off, 32);
        if (L.w >= off) incl += o;
    }
    int val = (int)b.un + incl - part;
    if (m == 0) val = L.half ? n - b.h : b.h;
    int16_t *fbp = FB + (size_t)L.pair * 2 * fb_stride;
    int16_t *fb = fbp + (size_t)L.half * fb_stride;
    if (have && L.w == 0) fb[0] = (int16_t)val;
#pragma unroll
    for (int bit = 0; bit < 32; ++bit) {
        val += (int)((vp >> bit) & 1u) - (int)((vn >> bit) & 1u);
        if ((rows >> bit) & 1u) fb[L.w * 32 + bit + 1] = (int16_t)val;
    }
    wave_lds_fence();
    int best = 0x7fffffff;
    if (have)
        for (int i = lane & (L.LP - 1); i <= m; i += L.LP) best = min(best, (int)fbp[i] + (int)fbp[fb_stride + m - i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        if (off < L.LP) best = min(best, __shfl_xor(best, off));
    return best;
}
