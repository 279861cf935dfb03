// indel.hip -- the indel (LCS) distance between strings on gfx950: insertions and deletions only,
//   indel(x, y) = |x| + |y| - 2 LCS(x, y),
// by the bit-vector LCS recurrence (Allison-Dix / Hyyro) as a systolic array across the lanes of a wavefront.  No reference
// counterpart; what rapidfuzz's Indel / ratio and a diff's size compute.
//
// The longer string of a pair is the "pattern", cut into 32-bit words; V holds one bit per pattern row, all ones at the
// start, and a text symbol with match mask eq advances it by
//   u  = V & eq
//   V' = (V + u + carry_in) | (V & ~eq)          carry_out = carry of the addition
// LCS = the zero bits of V on the pattern's rows after the last column.  Only the carry of the addition crosses a word
// boundary: lane w works on text column k - w at step k, and the carry-out of lane w - 1 at step k is the carry-in of lane w
// at step k + 1 -- levcol.h's LEV_CARRY_MASK hand-over: v_addc_co_u32 yields the sum and, as its carry-out lane mask, every
// lane's carry; s_lshl_b64 moves the mask up a lane and an and-not clears the first lane of every pair slot.  The column
// loops therefore run with all 64 lanes enabled (a disabled lane's carry-out reads 0); a lane outside its column range keeps
// V through a select in the head and tail steps, and the steady part has no select.  Bits above row m - 1 need no care: a
// carry never travels downwards, and the end masks them out.
//
// Kernels (ann_indel_launch chooses):
//   k_indel_f<1>   alphabets up to 256 symbols, strings up to 1024 symbols: one word per lane;
//   k_indel_f<2>   the same alphabets, 1025 .. 2048 symbols: two words per lane, the low word's carry feeds the high word's
//                  v_addc in the same step and only the high word's carry goes to the next lane;
//   k_indel_w      alphabets beyond 256 symbols: 16-bit codes, the match word computed from the lane's 32 pattern symbols.
// One slot class: a wave holds P = 64 / GL pairs in slots of GL lanes, GL from the data set's longest string (k_lev_f's second,
// tighter class for short pairs is not built).  All three serve the three pair forms of PairSource (explicit pairs, positions
// into a built list, one-to-all) and write `out`, and `RA` with `ncm`.  No floating point before the final conversion.
#include "common.h"
#include "indelcol.h"
#include "levhalf.h"

struct IndelArgs {
    const void *sym;       // uint8 codes (k_indel_f: 16-byte aligned starts) or uint16 codes (k_indel_w: starts at multiples of 8)
    const int32_t *soff;
    const int32_t *slen;
    const int2 *ij;
    const int32_t *idx;
    const int32_t *anchor;
    int64_t n;
    double *out;
    double *RA;
    uint8_t *ncm;
    int GL, P;         // lanes per pair slot, slots per wave
    int alphabet;
    int pad;           // text entries of padding either side of a slot's text (a multiple of 16, >= GL + 2)
    int text_stride;   // text entries per slot (a multiple of 16)
    int pm_bytes;      // bytes of match masks per wave (k_indel_f)
};

// The LDS of one wave: match masks, the slots' texts, 256 B of per-slot sums.
struct IndelLayout {
    int R, GL, P, pad, text_stride, pm_bytes;
    size_t bytes;
};
static IndelLayout indel_layout(int alphabet, int maxlen, bool wide)
{
    IndelLayout L;
    const int W = std::max(1, (maxlen + 31) / 32);
    L.R = (wide || W <= 32) ? 1 : 2;
    L.GL = (W + L.R - 1) / L.R;
    L.P = 64 / L.GL;
    // a lane reads its text at [pad - w + k], w < GL, k < maxlen + GL + 1 (two columns ahead of the last step)
    L.pad = (L.GL + 2 + 15) & ~15;
    L.text_stride = 2 * L.pad + ((maxlen + 15) & ~15);
    L.pm_bytes = wide ? 0 : 2 * L.R * alphabet * LEVF_ROW;
    L.bytes = (size_t)L.pm_bytes + (size_t)L.P * L.text_stride * (wide ? 2 : 1) + 256;
    return L;
}
size_t ann_indel_lds_bytes(int alphabet, int maxlen) { return indel_layout(alphabet, maxlen, alphabet > 256).bytes; }

// (IndelCarry and indel_column, the column and its carry state: indelcol.h, shared with threshwide.hip)

// The pair of slot position t_pair: string ids, and where RA / ncm take the result.
struct IndelPair {
    int si, sj;
    int64_t opos;
};
__device__ __forceinline__ IndelPair indel_pair(const IndelArgs &a, int64_t t_pair, bool active)
{
    IndelPair p = {0, 0, t_pair};
    if (active) {
        if (a.anchor) { p.si = *a.anchor; p.sj = (int)t_pair; }
        else {
            const int64_t q = a.idx ? a.idx[t_pair] : t_pair;
            const int2 e = a.ij[q];
            p.si = e.x; p.sj = e.y;
            if (a.idx) p.opos = q;
        }
    }
    return p;
}

// Wave-uniform step bounds: lane w works on column k - w of its slot's `n` columns (0 without a pair or a pattern).  Steps
// k_lo <= k < k_hi are in range for every lane of every pair of the wave; max_steps ends the longest chain.
struct IndelBounds {
    int max_steps, k_lo, k_hi;
};
__device__ __forceinline__ IndelBounds indel_bounds(bool walk, int n, int lanes_used, int GL)
{
    IndelBounds b;
    b.max_steps = walk ? n + lanes_used - 1 : 0;
    b.k_hi = walk ? n : 0x7fffffff;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        b.max_steps = max(b.max_steps, __shfl_xor(b.max_steps, off));
        b.k_hi = min(b.k_hi, __shfl_xor(b.k_hi, off));
    }
    b.max_steps = __builtin_amdgcn_readfirstlane(b.max_steps);
    b.k_lo = min(GL - 1, b.max_steps);
    b.k_hi = max(b.k_lo, min(__builtin_amdgcn_readfirstlane(b.k_hi), b.max_steps));
    return b;
}

// The end of a pair: the slot's lanes add their zero bits, the first lane stores d = m + n - 2 lcs.
__device__ __forceinline__ void indel_finish(const IndelArgs &a, int *ssum, int g, int w, bool active, int lcs_part, int m, int n,
                                             int64_t t_pair, int64_t opos)
{
    if (active && lcs_part) atomicAdd(&ssum[g], lcs_part);
    wave_lds_fence();
    if (active && w == 0) {
        const double d = (double)(m + n - 2 * ssum[g]);
        if (a.out) a.out[t_pair] = d;
        if (a.RA) { a.RA[opos] = d; a.ncm[opos] = 0; }
    }
    wave_lds_fence();
}

// ---------------------------------------------------------------------------------------------------------------------
// k_indel_f<R>: one wave per workgroup (waves never synchronise with each other; small workgroups let the LDS allocator
// pack as many waves per CU as the tables allow), P = 64 / GL pair slots, lane w of a slot owns words w R .. w R + R - 1.
// LDS: match masks PM[half-wave][word r][symbol][lane % 32] (uint32; k_lev_f's bank-interleaved table, one per word of a
// lane: the 32 lanes an LDS cycle serves never collide whatever symbols they look up), then a text per slot as byte codes
// with `pad` zero bytes either side, then the per-slot sums.  Per column a lane reads the symbol of column k + 2 and the R
// match words of column k + 1 while column k computes.
// ISA of this build (--save-temps), steady loop (two columns per trip), per column and lane:
//   R = 1: 4.5 VALU (v_and, v_addc_co, v_bitop3, v_lshl_add for the next match-mask row, half a v_add for the text pointer)
//          + 2 SALU for the carry (s_lshl_b64, s_and_b64 with the inverted first-lane mask) + 2.5 SALU of loop bookkeeping
//          + 2 LDS reads (ds_read_u8, ds_read_b32).  k_lev_f: 12.5 VALU + 4 SALU and the same two reads.
//   R = 2: 8.5 VALU (2 x the three, v_lshl_add, a v_add for the second word's table, half a v_add), the same SALU, 3 LDS
//          reads (ds_read_u8, 2 x ds_read_b32): 4.25 VALU per word-column.
// The head and tail steps add a v_cmp, a v_cndmask per word and a v_add.
// Registers: 80 VGPRs (R = 1) and 86 (R = 2) -- the 32 symbols of the match-mask build, not the column loop -- no scratch: 6 and
// 5 waves per SIMD.  The LDS request is the tighter bound: over 26 symbols a wave asks for 9.8 / 9.0 / 8.9 KiB with strings of up
// to 60 / 500 / 1000 symbols, 16 or 17 waves per CU = 4 per SIMD, and 17.3 KiB at 2000 symbols (2 per SIMD); 256 symbols x 2048
// symbols is the largest request, 132.4 KiB: one wave per CU, and nothing for the loader to refuse below the 160 KiB ceiling.
template <int R> __global__ __launch_bounds__(ANN_WAVE) void k_indel_f(IndelArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x, A = a.alphabet, GL = a.GL, P = a.P;
    const uint8_t *sym = reinterpret_cast<const uint8_t *>(a.sym);
    unsigned char *pm_col = smem + (size_t)(lane >> 5) * R * A * LEVF_ROW + (size_t)(lane & 31) * 4;   // word r: + r A LEVF_ROW
    const uint32_t word_bytes = (uint32_t)A * LEVF_ROW;
    int *ssum = reinterpret_cast<int *>(smem + a.pm_bytes + (size_t)P * a.text_stride);
    const int g = lane / GL;         // pair slot of this lane
    const int w = lane - g * GL;     // lane of the slot
    const bool slot_ok = g < P;
    uint8_t *txt_g = smem + a.pm_bytes + (size_t)(slot_ok ? g : 0) * a.text_stride;
    const int64_t n_tasks = (a.n + P - 1) / P;
    if (slot_ok)
        for (int e = w * 16; e < a.text_stride; e += GL * 16) *reinterpret_cast<uint4 *>(txt_g + e) = make_uint4(0, 0, 0, 0);
    IndelCarry cs;
    cs.bind(w);

    for (int64_t task = blockIdx.x; task < n_tasks; task += gridDim.x) {
        const int64_t t_pair = task * P + g;
        const bool active = slot_ok && t_pair < a.n;
        const IndelPair pr = indel_pair(a, t_pair, active);
        const int li = active ? a.slen[pr.si] : 0, lj = active ? a.slen[pr.sj] : 0;
        const bool swap = li < lj;   // the pattern is the longer string: fewer text columns to walk
        const int m = swap ? lj : li, n = swap ? li : lj;
        const uint8_t *pat = sym + (active ? a.soff[swap ? pr.sj : pr.si] : 0);
        const uint8_t *tex = sym + (active ? a.soff[swap ? pr.si : pr.sj] : 0);
        const int Wp = (m + 31) >> 5;          // pattern words
        const int Gp = (Wp + R - 1) / R;       // lanes that hold pattern words
        if (slot_ok && w == 0) ssum[g] = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) lev_build_masks(pm_col + r * word_bytes, A, pat, m, w * R + r, false, active);
        if (active) lev_stage(txt_g + a.pad, tex, n, w, GL);
        wave_lds_fence();

        const bool walk = active && m > 0;
        const uint32_t un = walk ? (uint32_t)n : 0u;
        const IndelBounds b = indel_bounds(walk, n, Gp, GL);
        uint32_t V[R], eq[R];
        const uint8_t *tp = txt_g + a.pad - w;   // tp[k] = this lane's symbol at step k
        uint32_t c1 = tp[1];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            V[r] = 0xffffffffu;
            eq[r] = *reinterpret_cast<const uint32_t *>(pm_col + r * word_bytes + (uint32_t)tp[0] * LEVF_ROW);
        }
        cs.reset();
        auto column = [&](int k, auto checked) {
            constexpr bool CHECKED = decltype(checked)::value;
            const uint32_t c2 = tp[k + 2];
            uint32_t eq_n[R];
#pragma unroll
            for (int r = 0; r < R; ++r) eq_n[r] = *reinterpret_cast<const uint32_t *>(pm_col + r * word_bytes + c1 * LEVF_ROW);
            indel_column<R, CHECKED>(cs, V, eq, !CHECKED || (uint32_t)(k - w) < un);
#pragma unroll
            for (int r = 0; r < R; ++r) eq[r] = eq_n[r];
            c1 = c2;
        };
        int k = 0;
        for (; k < b.k_lo; ++k) column(k, std::true_type());
        for (; k + 2 <= b.k_hi; k += 2) { column(k, std::false_type()); column(k + 1, std::false_type()); }
        for (; k < b.k_hi; ++k) column(k, std::false_type());
        for (; k < b.max_steps; ++k) column(k, std::true_type());
        int part = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) part += __popc(~V[r] & lev_rows_mask(w * R + r, Wp, m));
        indel_finish(a, ssum, g, w, active, part, m, n, t_pair, pr.opos);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_indel_w: alphabets beyond 256 symbols.  A match-mask table would be alphabet x 128 B per half-wave, so the match word of
// a column is computed: a lane keeps the 32 symbols of its pattern word in 16 registers, two 16-bit codes each, and compares
// them with the column's text symbol (both halves of cc): x = pr ^ cc is zero in a half that matches, the saturating packed
// subtraction 1 - x (v_pk_sub_u16 clamp) turns each half into "matches" (1 / 0), and shift-and-or steps gather the 32 flags.
// Register r holds rows 15 - r (low half) and 31 - r (high half), so that flag (r, half) shifted left 15 - r times lands on
// its row's bit: no permutation after the compare.  (k_lev_w's compare-and-select form costs about 80 VALU.)
// ISA of this build, steady loop, per word-column: 56 VALU -- 16 v_xor, 16 v_pk_sub_u16, 15 shifts / ors (v_lshl_or, v_or3,
// v_lshlrev), 2 for cc, so 49 for the match word; then the column's v_and (a v_bitop3 here), v_addc_co, v_bitop3, one v_or
// and the text pointer's v_add -- + 2 SALU for the carry, 3 of loop bookkeeping and one LDS read (ds_read_u16): the compare is
// 7/8 of the issue.  One word per lane up to 2048 symbols (slots of up to 64 lanes: no table, no banks to respect); text in
// LDS as 16-bit codes; rows past the pattern's end hold 0xffff, which no text symbol has (alphabets stop at 65 535 symbols) --
// the text's padding has it, and is only ever read by a lane outside its column range.
// 62 VGPRs, no scratch: 8 waves per SIMD; LDS holds the texts alone (4.6 KiB per wave at 1000 symbols), which allows as many.
__global__ __launch_bounds__(ANN_WAVE) void k_indel_w(IndelArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    const int lane = threadIdx.x, GL = a.GL, P = a.P;
    const uint16_t *sym = reinterpret_cast<const uint16_t *>(a.sym);
    const int g = lane / GL, w = lane - g * GL;
    const bool slot_ok = g < P;
    uint16_t *txt_g = reinterpret_cast<uint16_t *>(smem) + (size_t)(slot_ok ? g : 0) * a.text_stride;
    int *ssum = reinterpret_cast<int *>(smem + (size_t)P * a.text_stride * 2);
    const int64_t n_tasks = (a.n + P - 1) / P;
    if (slot_ok)
        for (int e = w * 8; e < a.text_stride; e += GL * 8)
            *reinterpret_cast<uint4 *>(txt_g + e) = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
    IndelCarry cs;
    cs.bind(w);
    uint32_t one = 0x00010001u;
    asm volatile("" : "+v"(one));   // opaque: keeps 1 - x a saturating packed subtraction (not two compares and selects)

    for (int64_t task = blockIdx.x; task < n_tasks; task += gridDim.x) {
        const int64_t t_pair = task * P + g;
        const bool active = slot_ok && t_pair < a.n;
        const IndelPair pq = indel_pair(a, t_pair, active);
        const int li = active ? a.slen[pq.si] : 0, lj = active ? a.slen[pq.sj] : 0;
        const bool swap = li < lj;
        const int m = swap ? lj : li, n = swap ? li : lj;
        const uint16_t *pat = sym + (active ? a.soff[swap ? pq.sj : pq.si] : 0);
        const uint16_t *tex = sym + (active ? a.soff[swap ? pq.si : pq.sj] : 0);
        const int Wp = (m + 31) >> 5;
        if (slot_ok && w == 0) ssum[g] = 0;
        uint32_t pr[16];   // pr[r] = row 15 - r | row 31 - r << 16 of this lane's word
        {
            const bool has = active && w < Wp;
            const uint4 *p16 = reinterpret_cast<const uint4 *>(pat + w * 32);
            const uint4 z = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
            const uint4 q0 = has ? p16[0] : z, q1 = has ? p16[1] : z, q2 = has ? p16[2] : z, q3 = has ? p16[3] : z;
            const uint32_t v[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
            const int valid = has ? min(32, m - w * 32) : 0;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lo = 15 - r, hi = 31 - r;
                const uint32_t slo = lo < valid ? (v[lo >> 1] >> ((lo & 1) * 16)) & 0xffffu : 0xffffu;
                const uint32_t shi = hi < valid ? (v[hi >> 1] >> ((hi & 1) * 16)) & 0xffffu : 0xffffu;
                pr[r] = slo | (shi << 16);
            }
        }
        if (active) {
            const int chunks = (n + 7) >> 3;   // 8 symbols per 16 bytes
            for (int ch = w; ch < chunks; ch += GL) reinterpret_cast<uint4 *>(txt_g + a.pad)[ch] = reinterpret_cast<const uint4 *>(tex)[ch];
        }
        wave_lds_fence();

        const bool walk = active && m > 0;
        const uint32_t un = walk ? (uint32_t)n : 0u;
        const IndelBounds b = indel_bounds(walk, n, Wp, GL);
        uint32_t V[1] = {0xffffffffu};
        const uint16_t *tp = txt_g + a.pad - w;
        uint32_t c0 = tp[0];
        cs.reset();
        auto column = [&](int k, auto checked) {
            constexpr bool CHECKED = decltype(checked)::value;
            const uint32_t c1 = tp[k + 1];
            const uint32_t cc = c0 | (c0 << 16);
            uint32_t eq[1] = {0u};
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const us2 x = __builtin_bit_cast(us2, pr[r] ^ cc);
                eq[0] = (eq[0] << 1) | __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(us2, one), x));
            }
            indel_column<1, CHECKED>(cs, V, eq, !CHECKED || (uint32_t)(k - w) < un);
            c0 = c1;
        };
        int k = 0;
        for (; k < b.k_lo; ++k) column(k, std::true_type());
        for (; k < b.k_hi; ++k) column(k, std::false_type());
        for (; k < b.max_steps; ++k) column(k, std::true_type());
        indel_finish(a, ssum, g, w, active, __popc(~V[0] & lev_rows_mask(w, Wp, m)), m, n, t_pair, pq.opos);
    }
}

int ann_indel_launch(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    if (src.n == 0) return ANNCHOR_OK;
    ANN_REQUIRE(c, c->maxlen >= 0 && c->maxlen <= INDEL_MAXLEN, ANNCHOR_ELIMIT, "string length %d outside 0..%d", c->maxlen, INDEL_MAXLEN);
    const IndelLayout L = indel_layout(c->alphabet, c->maxlen, c->sym_wide);
    IndelArgs a;
    a.sym = c->sym.p; a.soff = c->soff.as<int32_t>(); a.slen = c->slen.as<int32_t>();
    a.ij = src.ij; a.idx = src.idx; a.anchor = src.anchor; a.n = src.n;
    a.out = d_out; a.RA = d_RA; a.ncm = d_ncm;
    a.GL = L.GL; a.P = L.P; a.alphabet = c->alphabet; a.pad = L.pad; a.text_stride = L.text_stride; a.pm_bytes = L.pm_bytes;
    const void *kernel = c->sym_wide ? (const void *)k_indel_w : L.R == 1 ? (const void *)k_indel_f<1> : (const void *)k_indel_f<2>;
    // every kernel here may ask for up to 160 KiB of dynamic LDS; beyond 64 KiB the function must be told
    ANN_REQUIRE(c, L.bytes <= 160 * 1024, ANNCHOR_ELIMIT, "alphabet %d x length %d needs %zu B of LDS (> 160 KiB)", c->alphabet,
                c->maxlen, L.bytes);
    if (L.bytes > 64 * 1024) ANN_CHECK_HIP(c, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.bytes));
    const int64_t blocks = std::min<int64_t>((src.n + L.P - 1) / L.P, (int64_t)c->prop.multiProcessorCount * 32);
    ProfScope ps(c, "indel_pairs", (double)src.n * (2.0 * c->maxlen * (c->sym_wide ? 2 : 1) + 8));
    if (c->sym_wide) k_indel_w<<<(int)blocks, ANN_WAVE, L.bytes, c->stream>>>(a);
    else if (L.R == 1) k_indel_f<1><<<(int)blocks, ANN_WAVE, L.bytes, c->stream>>>(a);
    else k_indel_f<2><<<(int)blocks, ANN_WAVE, L.bytes, c->stream>>>(a);
    ANN_CHECK_HIP(c, hipGetLastError());
    return ANNCHOR_OK;
}
