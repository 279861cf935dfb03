// jaccard.hip -- Jaccard (Tanimoto) distance between finite sets of integers over a pair list (no reference counterpart: the
// reference bundles no measure on bags of discrete items).
//
//   i = |A n B|      u = |A| + |B| - i
//   jaccard(A, B) = 0.0                           if u == 0   (both empty)
//                 = (double)(u - i) / (double)u   otherwise   (one IEEE float64 division of two exact integers)
//
// |A| and |B| come from `slen`; a kernel counts only the intersection, in int32.  The count is an integer, so lane assignment,
// probe side and reduction order cannot change it, and the one division has fixed operands: the value is the definition's bit for
// bit, and jaccard(A, B) == jaccard(B, A) exactly.
//
// Two layouts of the same sets (ctx.hip), one kernel each, both in k_hausdorff's frame: one pair per group of G lanes, 64 / G
// pairs per wavefront, waves take pairs grid-stride, a slot past the end of the list works on pair (0, 0) and stores nothing, the
// cross-lane sum runs with every lane on, lane 0 of the group divides and stores.  No LDS, no barriers, no atomics.
//
// k_jaccard_bits<G>: member s is row s of `sym`, W uint32 words (W a multiple of 4, rows 16-byte aligned, padding bits zero).
// Lane gl of a group loads uint4 number gl, gl + G, ... of both rows and adds up the popcounts of the four "and" words: every
// word of a pair is read once.
//
// k_jaccard_tokens<G>: member s is lens[s] strictly ascending int32 codes at sym + soff[s].  The smaller member is the probe
// side: lane gl takes probes gl, gl + G, ... and looks each up by lower_bound in the larger member.  A lane's probes ascend, so
// its next search starts where the last one ended.  About min(n, m) log2(max(n, m)) loads per pair; an empty member makes no trip.
#include "pairkern.h"

struct JaccardArgs : PairArgs {
    const int32_t *sym;
    const int32_t *off, *len;
    int w4;   // bits form: uint4 per row
};

__device__ __forceinline__ double jaccard_value(int n, int m, int common)
{
    const int u = n + m - common;
    return u == 0 ? 0.0 : __ddiv_rn((double)(u - common), (double)u);
}

template <int G> __device__ __forceinline__ int group_sum(int v)
{
#pragma unroll
    for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

template <int G> __global__ __launch_bounds__(PAIR_THREADS) void k_jaccard_bits(JaccardArgs a)
{
    constexpr int PPW = ANN_WAVE / G;   // pairs per wavefront
    const int lane = threadIdx.x & (ANN_WAVE - 1), gl = lane & (G - 1), slot = lane / G;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / ANN_WAVE;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / ANN_WAVE;
    const uint4 *rows = reinterpret_cast<const uint4 *>(a.sym);
    for (int64_t base = wave * PPW; base < a.n; base += nwaves * PPW) {   // (wave-uniform: the shuffles run with every lane on)
        const int64_t t = base + slot;
        const PairSlot ps = pair_decode(a, t);
        const uint4 *x = rows + (int64_t)ps.i * a.w4, *y = rows + (int64_t)ps.j * a.w4;
        int common = 0;
        for (int q = gl; q < a.w4; q += G) {
            const uint4 u = x[q], v = y[q];
            common += __popc(u.x & v.x) + __popc(u.y & v.y) + __popc(u.z & v.z) + __popc(u.w & v.w);
        }
        common = group_sum<G>(common);
        if (ps.active && gl == 0) pair_store(a, t, ps.opos, jaccard_value(a.len[ps.i], a.len[ps.j], common));
    }
}

template <int G> __global__ __launch_bounds__(PAIR_THREADS) void k_jaccard_tokens(JaccardArgs a)
{
    constexpr int PPW = ANN_WAVE / G;
    const int lane = threadIdx.x & (ANN_WAVE - 1), gl = lane & (G - 1), slot = lane / G;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / ANN_WAVE;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / ANN_WAVE;
    for (int64_t base = wave * PPW; base < a.n; base += nwaves * PPW) {   // (wave-uniform)
        const int64_t t = base + slot;
        const PairSlot ps = pair_decode(a, t);
        int n = a.len[ps.i], m = a.len[ps.j];
        const int32_t *p = a.sym + a.off[ps.i], *s = a.sym + a.off[ps.j];   // probes, searched
        if (n > m) {
            const int32_t *q = p; p = s; s = q;
            const int k = n; n = m; m = k;
        }
        int common = 0, lo = 0;
        for (int q = gl; q < n; q += G) {   // (the lanes' trips differ; they meet again before the sum)
            const int32_t v = p[q];
            int hi = m;                     // lower_bound of v in s[lo, m)
            while (lo < hi) {
                const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
                if (s[mid] < v) lo = mid + 1;
                else hi = mid;
            }
            if (lo < m && s[lo] == v) { ++common; ++lo; }
        }
        common = group_sum<G>(common);
        if (ps.active && gl == 0) pair_store(a, t, ps.opos, jaccard_value(n, m, common));
    }
}

template <int G> static int launch_bits(annchor_ctx *c, const JaccardArgs &a)
{
    static_assert((G & (G - 1)) == 0 && G <= ANN_WAVE, "a pair takes a power-of-two group of lanes");
    k_jaccard_bits<G><<<pair_grid(c, a.n, G), PAIR_THREADS, 0, c->stream>>>(a);
    ANN_CHECK_HIP(c, hipGetLastError());
    return ANNCHOR_OK;
}

template <int G> static int launch_tokens(annchor_ctx *c, const JaccardArgs &a)
{
    static_assert((G & (G - 1)) == 0 && G <= ANN_WAVE, "a pair takes a power-of-two group of lanes");
    k_jaccard_tokens<G><<<pair_grid(c, a.n, G), PAIR_THREADS, 0, c->stream>>>(a);
    ANN_CHECK_HIP(c, hipGetLastError());
    return ANNCHOR_OK;
}

// tokens form, by the data set's largest member: a lane makes up to 16 searches at G = 4 and up to 64 at G = 16.  Measured on
// 20 .. 200-token members: G = 16 takes 20 % less time than G = 4 and 24 % less than G = 64; 1024 is not swept.
#define JACCARD_TOKENS_G4 64
#define JACCARD_TOKENS_G16 1024

int ann_jaccard_launch(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    if (src.n == 0) return ANNCHOR_OK;
    JaccardArgs a;
    pair_fill(a, src, d_out, d_RA, d_ncm);
    a.sym = c->sym.as<int32_t>();
    a.off = c->soff.as<int32_t>(); a.len = c->slen.as<int32_t>();
    a.w4 = 0;
    if (c->metric == ANNCHOR_METRIC_JACCARD_BITS) {
        const int W = c->set_words;
        ANN_REQUIRE(c, W >= 4 && W <= 256 && W % 4 == 0, ANNCHOR_EINVAL, "bitset rows of %d words", W);
        a.w4 = W / 4;
        ProfScope ps(c, "jaccard_pairs", (double)src.n * (2.0 * W * sizeof(uint32_t) + 16));
        if (a.w4 <= 4) return launch_bits<4>(c, a);     // one uint4 per lane
        if (a.w4 <= 16) return launch_bits<16>(c, a);
        return launch_bits<64>(c, a);
    }
    ANN_REQUIRE(c, c->maxlen >= 0 && c->maxlen <= 65536, ANNCHOR_ELIMIT, "token set size %d outside 0..65536", c->maxlen);
    // (no byte count: a pair's searches touch about min(n, m) log2(max(n, m)) words, which no bound from maxlen describes)
    ProfScope ps(c, "jaccard_pairs", 0);
    if (c->maxlen <= JACCARD_TOKENS_G4) return launch_tokens<4>(c, a);
    if (c->maxlen <= JACCARD_TOKENS_G16) return launch_tokens<16>(c, a);
    return launch_tokens<64>(c, a);
}
