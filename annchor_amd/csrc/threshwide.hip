// threshwide.hip -- the edit distance on real sequences (EDR) and the longest-common-subsequence distance (LCSS) on members of
// 5 .. 64 coordinates per point, over a pair list.  The definitions are seqdp.hip's (its head, "EDR and LCSS") and so is the
// contract: match(p, q) iff fabs(p[k] - q[k]) <= eps for every k, each subtraction rounded on its own in float64, float32 input
// widened exactly, a difference of exactly eps a match; every cell a small integer, so the value equals the sequential double loop
// bit for bit, in both orders of a pair, and the kernel is free to put the longer member on the rows.
//
// A cell of either measure is decided by one boolean, so there is no cost tile, no square root and no float64 sweep here
// (seqwide.hip, editwide.hip): the match relation of a pair is a bit matrix, and both recurrences have exact bit-vector forms on
// an arbitrary bit matrix -- EDR is the Levenshtein recurrence (levcol.h's lev_column, Myers / Hyyro: E(i, -1) = i + 1 is the hp
// carry-in 1 of the first lane), LCSS the LCS recurrence (indelcol.h's indel_column, Allison-Dix / Hyyro: a matched cell takes
// diagonal + 1, which is never below its upper and left neighbours).  The shorter member y lies along the bit axis, the longer
// member x on the rows, which the recurrences walk as lev.hip and indel.hip walk a text.
//
// k_threshwide<T, Op>: one pair per workgroup of four waves, pairs taken grid-stride; rows cut into strips of TW_ROWS = 64.  In
// iteration `it` all four waves stage strip it's points of x in LDS as float64 [row][coordinate]; then
//
//   waves 1 .. 3 build the strip's match words.  Each owns a third of the strip's rows and walks the 64-column blocks of y: a
//   lane holds TW_KC = 16 coordinates of its column's point of y in registers, and for a row the 16 differences against the row's
//   coordinates -- wave-uniform, broadcast LDS reads -- are compared with eps; the comparisons' lane masks are ANDed on the scalar
//   unit and one ballot is the 64-bit partial match word of (row, block), ANDed into the word the earlier chunks of coordinates
//   left.  The words of the wave's rows live in one 64-bit register across its lanes, lane r the word of strip row r, read and
//   written back by v_readlane and a select: no LDS traffic between chunks.  The word starts as the block's columns < m, under
//   LCSS's delta ANDed with the band |i - j| <= delta of its row (plain, never widened to n - m); a word that has become 0 skips
//   the row's remaining chunks by a uniform branch (TW_EARLY_EXIT; the bits do not change).  After the last chunk the lanes store
//   their rows' words as 32-bit halves, [row][word], into a ring of four strips.
//
//   wave 0 runs the bit-vector recurrence as a systolic array: lane w holds 32-bit word w of the vector over y's columns (at most
//   32 lanes for 1024 columns) and at step k works on row k - w, its match word read from the ring a step ahead.  Iteration `it`
//   sweeps steps (it - 1) 64 .. it 64 - 1, which touch the strips it - 2 and it - 1, while the producers write strip it: three
//   live strips in a ring of four, and the vectors and carries stay in registers from strip to strip.  All 64 lanes are enabled
//   in the column loop, as the column helpers require (the checked column throughout); lanes past y's last word compute on whatever the ring holds and hand
//   their carries to nobody.  At the end the lanes count -- EDR: n + popc(vp) - popc(vn) over the columns < m, LCSS: the zero
//   bits of V there -- a butterfly adds the counts and lane 0 converts, divides and stores.
//
// Two barriers per iteration (after staging, after producing), met by all four waves in uniform control flow.  LDS: the ring,
// 256 rows x 2 ceil(maxlen / 64) words, at most 32 KiB, and the staged strip, 64 x dim doubles, at most 32 KiB: 64 KiB at the
// ceiling, so that at least two workgroups share a CU's 160 KiB.  No floating point in the sweep before the final conversion, no
// atomics, no matrix instructions (there is no product to fuse); results leave by plain vector stores from lane 0 of wave 0.
#include <type_traits>

#include "seqops.h"
#include "indelcol.h"
#include "levhalf.h"

#ifndef TW_ROWS
#define TW_ROWS 64          // rows of a strip (32 or 64: the sweep's lanes reach 31 rows back, into one earlier strip only)
#endif
#ifndef TW_EARLY_EXIT
#define TW_EARLY_EXIT 1     // skip a row's remaining chunks of coordinates once its match word is 0
#endif
#define TW_RING 4                            // strips of match words in LDS
#define TW_SLOTS (TW_RING * TW_ROWS)         // rows of the ring; row i lives in slot i % TW_SLOTS
#define TW_KC 16                             // coordinates of y a lane holds at a time
#define TW_MAXLEN 1024
#define TW_PRODUCERS (PAIR_THREADS / ANN_WAVE - 1)
#define TW_PART ((TW_ROWS + TW_PRODUCERS - 1) / TW_PRODUCERS)   // rows of a strip a producer wave owns
static_assert(TW_ROWS == 32 || TW_ROWS == 64, "a strip's rows: one bit matrix row per lane, and at least the 32 lanes of the sweep");

struct EdrWideOp {
    static constexpr bool lcss = false;
    static constexpr const char *profile = "edr_pairs", *name = "wide edr";
};
struct LcssWideOp {
    static constexpr bool lcss = true;
    static constexpr const char *profile = "lcss_pairs", *name = "wide lcss";
};

// words of a ring row (two per 64-column block of the longest member) and doubles of a staged row (dim rounded up to four)
static inline int tw_pitch(int maxlen) { return 2 * ((maxlen + 63) / 64); }
static inline int tw_xpitch(int dim) { return (dim + 3) & ~3; }
static inline size_t tw_lds_bytes(int dim, int maxlen)
{
    return sizeof(uint32_t) * TW_SLOTS * (size_t)tw_pitch(maxlen) + sizeof(double) * TW_ROWS * (size_t)tw_xpitch(dim);
}

__device__ __forceinline__ uint64_t tw_readlane(uint64_t v, int l)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), l);
    return (uint64_t)hi << 32 | lo;
}

template <typename T, typename Op> __global__ __launch_bounds__(PAIR_THREADS) void k_threshwide(SeqArgs<T> a, int dim, int pitch)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char tw_lds[];
    uint32_t *const words = reinterpret_cast<uint32_t *>(tw_lds);                                          // [TW_SLOTS][pitch]
    const int xp = (dim + 3) & ~3;
    double *const xs = reinterpret_cast<double *>(tw_lds + sizeof(uint32_t) * TW_SLOTS * (size_t)pitch);   // [TW_ROWS][xp]
    const int tid = threadIdx.x, lane = tid & (ANN_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / ANN_WAVE);
    const double eps = a.eps;
    const int delta = a.window;
    std::conditional_t<Op::lcss, IndelCarry, LevCarry<LEV_CARRY_MASK>> cs;
    cs.bind(lane);   // one slot of 64 lanes
    const uint32_t *const wp = words + min(lane, pitch - 1);   // the sweep's word of a ring row

    for (int64_t t = blockIdx.x; t < a.n; t += gridDim.x) {
        const PairSlot ps = pair_decode(a, t);
        // (the pair is the workgroup's: scalar values, so that every loop bound and the sweep's carry masks stay on the scalar unit)
        int n = __builtin_amdgcn_readfirstlane(a.len[ps.i]), m = __builtin_amdgcn_readfirstlane(a.len[ps.j]);
        int xo = __builtin_amdgcn_readfirstlane(a.off[ps.i]), yo = __builtin_amdgcn_readfirstlane(a.off[ps.j]);
        if (n < m) {   // the longer member on the rows
            const int k = n; n = m; m = k;
            const int o = xo; xo = yo; yo = o;
        }
        const T *x = a.val + (int64_t)xo * dim, *y = a.val + (int64_t)yo * dim;
        const int NB = (m + 63) >> 6, W32 = (m + 31) >> 5;
        const int nstrips = (n + TW_ROWS - 1) / TW_ROWS;
        const int total = n + W32 - 1;                               // steps of the sweep
        const int niters = (total + TW_ROWS - 1) / TW_ROWS + 1;      // (> nstrips: the sweep runs a strip behind)

        uint32_t vp = 0xffffffffu, vn = 0u, V[1] = {0xffffffffu}, eq = 0u;
        cs.reset();

        for (int it = 0; it < niters; ++it) {
            const int R0 = it * TW_ROWS, nr = min(TW_ROWS, n - R0);
            if (it < nstrips)
                for (int e = tid; e < TW_ROWS * xp; e += PAIR_THREADS) {
                    const int r = e / xp, k = e - r * xp;
                    xs[e] = (double)x[(int64_t)min(R0 + r, n - 1) * dim + min(k, dim - 1)];
                }
            __syncthreads();

            if (wave == 0) {
                if (it > 0) {
                    const int kb = R0 - TW_ROWS, ke = min(R0, total);
                    if (kb < ke) eq = wp[((kb - lane) & (TW_SLOTS - 1)) * pitch];
                    for (int k = kb; k < ke; ++k) {
                        uint32_t eq_n = 0u;
                        auto fetch = [&] {
                            if (k + 1 < ke) eq_n = wp[((k + 1 - lane) & (TW_SLOTS - 1)) * pitch];   // (the next phase reads its first itself)
                        };
                        // a lane off the rows of x keeps its vector (the checked column throughout: the sweep is a small share
                        // of a pair's work, and one body keeps the carry masks in scalar registers across the strips)
                        const bool valid = (uint32_t)(k - lane) < (uint32_t)n;
                        if constexpr (Op::lcss) {
                            fetch();
                            const uint32_t e1[1] = {eq};
                            indel_column<1, true>(cs, V, e1, valid);
                        } else
                            lev_column<LEV_CARRY_MASK, true>(cs, vp, vn, eq, valid, fetch);
                        eq = eq_n;
                    }
                }
            } else if (it < nstrips) {
                const int r_lo = (wave - 1) * TW_PART, r_hi = min(r_lo + TW_PART, nr);
                const int i = R0 + lane;
                for (int b = 0; b < NB && r_lo < r_hi; ++b) {
                    const int c0 = 64 * b;
                    const T *yp = y + (int64_t)min(c0 + lane, m - 1) * dim;
                    // the words of this wave's rows, lane r the row R0 + r: the block's columns < m, under delta its band
                    uint64_t acc = m - c0 >= 64 ? ~0ull : ~0ull >> (64 - (m - c0));
                    if (Op::lcss && delta >= 0) {
                        const int lo = max(i - delta - c0, 0), hi = min(i + delta - c0, 63);
                        acc = lo > hi ? 0ull : acc & (~0ull >> (63 - max(hi, 0))) & (~0ull << min(lo, 63));
                    }
                    for (int k0 = 0; k0 < dim; k0 += TW_KC) {
                        const int kc = min(TW_KC, dim - k0);
                        double yv[TW_KC];
#pragma unroll
                        for (int kk = 0; kk < TW_KC; ++kk) yv[kk] = (double)yp[min(k0 + kk, dim - 1)];
                        // FULL: 16 coordinates; otherwise the chunk's groups of four (a row is padded to a multiple of four with
                        // copies of its last coordinate, here and in xs), each behind a uniform branch
                        auto rows = [&](auto full) {
                            constexpr bool FULL = decltype(full)::value;
                            for (int r = r_lo; r < r_hi; ++r) {
                                uint64_t w = tw_readlane(acc, r);
                                if (TW_EARLY_EXIT && w == 0) continue;
                                const double *xr = xs + r * xp + k0;
#pragma unroll
                                for (int g = 0; g < TW_KC; g += 4)
                                    if (FULL || g < kc) {
#pragma unroll
                                        for (int kk = g; kk < g + 4; ++kk) w &= __builtin_amdgcn_ballot_w64(fabs(xr[kk] - yv[kk]) <= eps);
                                    }
                                acc = lane == r ? w : acc;
                            }
                        };
                        if (kc == TW_KC) rows(std::true_type());
                        else rows(std::false_type());
                    }
                    if (lane >= r_lo && lane < r_hi)
                        *reinterpret_cast<uint2 *>(words + ((R0 + lane) & (TW_SLOTS - 1)) * pitch + 2 * b) =
                            make_uint2((uint32_t)acc, (uint32_t)(acc >> 32));
                }
            }
            __syncthreads();
        }

        if (wave == 0) {
            const uint32_t cols = lev_rows_mask(lane, W32, m);
            int cnt = Op::lcss ? __popc(~V[0] & cols) : __popc(vp & cols) - __popc(vn & cols);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
            if (lane == 0) {
                double res;
                if constexpr (Op::lcss)
                    res = 1.0 - (double)cnt / (double)m;           // (after the swap m = min(n, m))
                else {
                    res = (double)(n + cnt);
                    if (a.normalize) res = res / (double)n;        // (and n = max(n, m))
                }
                pair_store(a, t, ps.opos, res);
            }
        }
    }
}

template <typename T, typename Op> static int tw_launch(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    const int dim = c->curve_dim;
    ANN_REQUIRE(c, dim > 4 && dim <= 64, ANNCHOR_ELIMIT, "%s: series dim %d outside 5..64", Op::name, dim);
    ANN_REQUIRE(c, c->maxlen >= 1 && c->maxlen <= TW_MAXLEN, ANNCHOR_ELIMIT, "%s: series length %d outside 1..%d at dim %d", Op::name,
                c->maxlen, TW_MAXLEN, dim);
    SeqArgs<T> a = {};
    pair_fill(a, src, d_out, d_RA, d_ncm);
    a.val = c->sym.as<T>();
    a.off = c->soff.as<int32_t>(); a.len = c->slen.as<int32_t>();
    a.window = c->dtw_window < 0 ? -1 : (c->dtw_window < 2 * TW_MAXLEN ? c->dtw_window : 2 * TW_MAXLEN);   // (beyond: every cell)
    a.eps = c->match_eps;
    a.normalize = c->edr_normalize;
    const size_t lds = tw_lds_bytes(dim, c->maxlen);   // <= 64 KiB
    ProfScope ps(c, Op::profile, (double)src.n * (2.0 * c->maxlen * dim * sizeof(T) + 16));
    // one pair per workgroup; at least two workgroups share a CU's LDS, and beyond the cap the workgroups take further pairs grid-stride
    const int64_t cap = (int64_t)c->prop.multiProcessorCount * 8;
    k_threshwide<T, Op><<<(int)(src.n < cap ? src.n : cap), PAIR_THREADS, lds, c->stream>>>(a, dim, tw_pitch(c->maxlen));
    ANN_CHECK_HIP(c, hipGetLastError());
    return ANNCHOR_OK;
}

int ann_threshwide_launch(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    if (src.n == 0) return ANNCHOR_OK;
    switch (c->metric) {
    case ANNCHOR_METRIC_EDR_F32: return tw_launch<float, EdrWideOp>(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_EDR_F64: return tw_launch<double, EdrWideOp>(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_LCSS_F32: return tw_launch<float, LcssWideOp>(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_LCSS_F64: return tw_launch<double, LcssWideOp>(c, src, d_out, d_RA, d_ncm);
    default: ann_set_err(c, "no threshold measure of 5 .. 64 coordinates per point bound to this context"); return ANNCHOR_EINVAL;
    }
}
