// knntile.h -- what the streamed k-NN build's tile kernels have in common: k_st_knn (streamed.hip, exact f32), k_st_knnbf
// (knnbf.hip, split fp16), k_st_knnbk (knnbk.hip, the same, k-blocked) and k_st_knnh (knnh.hip, two-stage filter).
//
// A tile kernel's workgroup owns a 128-row tile, ranks all column tiles, and in rounds selects the next best-ranked tiles and
// streams them.  The streams are each kernel's own (their files say how); what surrounds them is here, once, as
// __forceinline__ function templates on the thread count, the kernel's shared-memory struct, KMAX and JOIN:
//   st_now, P8 / PS / PS0, f16x8, ST_BF_MARGIN, SelBuf, unit_swz, slab_end                         whoever needs them
//   st_row_tile       the XCD-banded row-tile assignment                                           all four kernels
//   st_rank_fill      rank key and valid bound of every column tile into the scratch rows          all four
//   st_select_round   a selection round: short list, 3-level radix selection, collect, sort        k_st_knn, knnh
//   st_hand_over      the round's tiles out of the sort buffers (which alias the operand ring)     knnh
//   st_thrmax         the row tile's worst k-th distance as last published                         knnbf, knnbk, knnh
//   st_publish, st_test_only   the end of a tile / of a run of the stream                          knnbf, knnbk
//   st_merge_lists    the cooperative merge of a slab's survivors into the sorted lists            knnbf, knnbk
//   st_launch_tile    (host) LDS attribute + launch of a tile kernel or its join-pass form         knnbf, knnbk
// Inlined, each is the code the kernels used to carry themselves: the arithmetic and its order are unchanged.
// What is NOT here although two kernels have it: k_st_knnbf and k_st_knnbk keep their own selection rounds, next_tile and
// exact re-ranking epilogue (knnbf's 128-dimension kernels sit at 256 vector registers and gain spills through any shared form
// of the three; knnbk's tile phase measured 0.4 % slower through st_select_round) -- their files give the figures.
#pragma once
#include "streamed.h"

#define ST_BF_MARGIN 2   // list entries beyond K kept by the split-fp16 distance (re-ranked exactly at the end)

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// ST_PROFILE builds: per-wave cycle sums by segment into the kernel's own `pf` array (each kernel lists its segments), added to
// a.prof at the end and printed by knn_tile_phase.
#ifdef ST_PROFILE
// (ordered: nothing may be scheduled across the time stamp, and it waits for the wave's outstanding LDS / scalar traffic)
__device__ __forceinline__ long long st_now()
{
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return (long long)t;
}
#define P8(i) { const long long pf_n = st_now(); pf[i] += pf_n - pf_t; pf_t = pf_n; }
// sub-segment stamp: time since the last P8 / PS goes to slot i (8..15) without resetting the P8 clock
#define PS(i) { const long long pf_n = st_now(); pf[i] += pf_n - pf_s; pf_s = pf_n; }
#define PS0 { pf_s = st_now(); }
#else
#define P8(i)
#define PS(i)
#define PS0
#endif

struct SelBuf {   // candidate tiles of a selection round (aliases the operand ring, idle between runs)
    float surv_lb[ST_SURV];
    float surv_vb[ST_SURV];
    int32_t surv_j[ST_SURV];
};

// swizzle of a column's 16-byte units in an operand slab (knnbf.hip's header comment); UPC = units per column
template <int UPC> __device__ __forceinline__ int unit_swz(int col) { return UPC >= 16 ? (col & 15) : ((col >> 1) & (UPC - 1)); }

// End of a slab: the wave's LDS-DMA pieces of the next slab have landed and its LDS traffic is done; the barrier hands the
// next slab to every wave and this slab's ring slot back to the requests.  (The requests are invisible to the compiler's
// wait bookkeeping -- inline asm; sched_barrier: the memory clobber alone does not keep register-only instructions on
// their side.)
__device__ __forceinline__ void slab_end()
{
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// XCD-banded row-tile assignment (workgroup b of nb runs on XCD b % 8): the workgroups resident on one XCD own consecutive row
// tiles of the k-d order, whose column-tile lists overlap, so the streamed column tiles are shared through that XCD's L2
__device__ __forceinline__ int st_row_tile(int b, int nb)
{
    const int q = nb >> 3, r = nb & 7, x = b & 7, y = b >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + y;
}

// Rank key and valid bound of every column tile against row tile I into the scratch rows -- unless k_st_rank_pairs
// (streamed.hip) has filled them ahead of the kernel
template <int THREADS, class Sh> __device__ __forceinline__ void st_rank_fill(const KnnArgs &a, const Sh &sh, int I, float *skey, float *slb)
{
    if (!a.pre_ranked)
    for (int J = threadIdx.x; J < a.nt_all; J += THREADS) {
        float lb = 0.f, lbc = 0.f;
        for (int an = 0; an < a.na; ++an) {
            const float lj = a.lo[(size_t)an * a.nt_all + J], hj = a.hi[(size_t)an * a.nt_all + J];
            const float gap = fmaxf(sh.loI[an] - hj, lj - sh.hiI[an]);
            // slack for the float32 rounding of D (bounds must stay valid lower bounds)
            lb = fmaxf(lb, gap - 4e-6f * (fabsf(hj) + fabsf(sh.hiI[an])));
            const float dm = a.mid[(size_t)an * a.nt_all + J] - sh.midI[an];
            lbc += dm * dm;   // rank key: squared L2 distance between the tiles' mean anchor vectors
        }
        skey[J] = ((J == I && !a.query) || !(lbc < INFINITY)) ? INFINITY : lbc;   // +inf: never a candidate
        slb[J] = lb;
    }
}

// (as of the last tile whose publication a barrier separates from the reader: tile `tdone`)
template <class Sh> __device__ __forceinline__ float st_thrmax(const Sh &sh, int tdone)
{
    const float *w = sh.wave_thr[tdone & 1];
    return fmaxf(fmaxf(w[0], w[1]), fmaxf(w[2], w[3]));
}

// the round's tiles leave the sort buffers before the stream takes the ring back
template <int THREADS, class Sh> __device__ __forceinline__ void st_hand_over(Sh &sh, const SelBuf &sb, int ns)
{
    for (int q = threadIdx.x; q < ns; q += THREADS) { sh.run_j[q] = sb.surv_j[q]; sh.run_vb[q] = sb.surv_vb[q]; }
}

// One selection round of a row tile.  A tile is ELIGIBLE while its valid bound is below the row tile's worst k-th distance
// `thrmax`; eligible tiles are taken in (rank key, tile) order.  A round finds the bits of the keep-th smallest remaining key
// with a 3-level radix selection (12 + 12 + 8 bits; non-negative floats order like their bit patterns; 4096-bin histogram
// `hist`), collects the tiles up to it into `sb` and sorts them once: entries [0, ns) of sb are the round's tiles in rank
// order, ns is returned (0: nothing is eligible any more).  The caller takes them out of sb (st_hand_over, where sb aliases
// what the stream needs), runs them, calls st_round_done and goes on while sel.more, the budget and the early stop allow.
// `processed`: tiles evaluated so far -- a round selects what the budget can still use, twice over for the entries the
// bounds will drop, at least 64 and at most ST_KEEP (the tiles and their order do not depend on it).
//
// SHORT LIST.  A selection round sweeps the scratch row four times (three histogram levels + the collection): at 62 500 column
// tiles that is 2 MB per round and row tile, a fifth of the kernel's wave cycles once the ranking had left it.  Instead: ONE
// histogram sweep of the key's top 12 bits finds the key bound below which ~4 ST_KEEP eligible tiles lie, ONE more sweep copies
// those (key, bound, tile) to a short list `clk` ([3][ST_CL_CAP]: key bits, bound bits, tile), and the rounds select from the list
// -- the same tiles in the same order: every eligible tile below the key bound is in the list, and the list is rebuilt behind the
// cursor when a round finds fewer than ST_KEEP eligible tiles in it while tiles beyond its bound remain.  clk == nullptr (short
// rows: knn_tile_phase reserves none): every sweep goes over the scratch row.
struct TileSelect {
    uint32_t done_bits = 0;   // (done_bits, done_j): key bits / index of the last tile already considered
    int done_j = -1;          // (nothing considered yet: every key is > (0, -1))
    int cl_n = 0;             // entries of the short list (uniform)
    bool cl_valid = false, cl_complete = false;
    bool more = false;        // the last round was cut at `keep`: later tiles remain
    uint32_t last_bits = 0;   // (last_bits, last_j): the last round's last tile -- the cursor once the round has run (st_round_done)
    int last_j = -1;
};
template <int THREADS, class Sh>
__device__ __forceinline__ int st_select_round(const KnnArgs &a, Sh &sh, SelBuf &sb, uint32_t *hist, const float *skey, const float *slb, uint32_t *clk,
                                               int lane, int wave, float thrmax, int processed, TileSelect &sel)
{
    uint32_t &done_bits = sel.done_bits;
    int &done_j = sel.done_j, &cl_n = sel.cl_n;
    bool &cl_valid = sel.cl_valid, &cl_complete = sel.cl_complete;
    // entries (key bits, valid bound, tile) of the short list or of the whole scratch row, thread-strided
    auto sweep = [&](bool from_list, auto f) {
        // (eight entries' loads in flight per thread: one entry at a time, a sweep of the 62 500 tiles of N = 8 x 10^6 was 244 dependent
        // global round trips per thread -- the selection rounds were 15 % of the two-stage kernel there, 7 % at N = 10^6)
        constexpr int SW = 8;
        if (from_list) {
            int q = threadIdx.x;
            for (; q + (SW - 1) * THREADS < cl_n; q += SW * THREADS) {
                uint32_t kb[SW], lbb[SW], jj[SW];
#pragma unroll
                for (int u = 0; u < SW; ++u) { kb[u] = clk[q + u * THREADS]; lbb[u] = clk[ST_CL_CAP + q + u * THREADS]; jj[u] = clk[2 * ST_CL_CAP + q + u * THREADS]; }
#pragma unroll
                for (int u = 0; u < SW; ++u) f(kb[u], __uint_as_float(lbb[u]), (int)jj[u]);
            }
            for (; q < cl_n; q += THREADS) f(clk[q], __uint_as_float(clk[ST_CL_CAP + q]), (int)clk[2 * ST_CL_CAP + q]);
        } else {
            int J = threadIdx.x;
            for (; J + (SW - 1) * THREADS < a.nt_all; J += SW * THREADS) {
                uint32_t kb[SW];
                float lbv[SW];
#pragma unroll
                for (int u = 0; u < SW; ++u) { kb[u] = __float_as_uint(skey[J + u * THREADS]); lbv[u] = slb[J + u * THREADS]; }
#pragma unroll
                for (int u = 0; u < SW; ++u) f(kb[u], lbv[u], J + u * THREADS);
            }
            for (; J < a.nt_all; J += THREADS) f(__float_as_uint(skey[J]), slb[J], J);
        }
    };
    // first bin whose cumulative count reaches `want` among nbins bins of `hist`: thread t owns bins [per t, per (t+1)); the
    // bin in sh.sel_bin (-1: the total stays below `want`), the count before it in sh.sel_before
    auto find_bin = [&](int nbins, uint32_t want) {
        const int per = nbins >= THREADS ? nbins / THREADS : 1;
        const bool owner = (int)threadIdx.x * per < nbins;
        uint32_t mine = 0;
        if (owner)
            for (int q = 0; q < per; ++q) mine += hist[threadIdx.x * per + q];
        uint32_t incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        uint32_t *wtot = reinterpret_cast<uint32_t *>(&sb.surv_lb[0]);   // 4 wave totals (surv_lb is idle here)
        if (threadIdx.x == 0) sh.sel_bin = -1;
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        uint32_t before = incl - mine;
        for (int w2 = 0; w2 < wave; ++w2) before += wtot[w2];
        if (owner && before < want && before + mine >= want) {
            uint32_t ac = before;
            int q = threadIdx.x * per;
            for (;; ++q) { if (ac + hist[q] >= want) break; ac += hist[q]; }
            sh.sel_bin = q;
            sh.sel_before = ac;
        }
        __syncthreads();
    };
    {
        // (a round selects what the budget can still use, twice over for the entries the bounds will drop: the warm-up of the two-stage
        // kernel -- 33 tiles -- selected, collected and sorted 512 like everyone else; the tiles and their order are the same)
        const uint32_t keep = (uint32_t)min(ST_KEEP, max(64, 2 * (a.max_tiles - processed)));
        uint32_t prefix = 0;
        uint32_t want = keep;
        bool all = false, use_list = false;
        for (int attempt = 0; attempt < 2; ++attempt) {
            if (clk && !cl_valid) {
                // ---- (re)build the short list behind the cursor
                for (int q = threadIdx.x; q < 4096; q += THREADS) hist[q] = 0;
                __syncthreads();
                sweep(false, [&](uint32_t kb, float lb, int J) {
                    const bool after_done = kb > done_bits || (kb == done_bits && J > done_j);
                    if (kb < 0x7f800000u && after_done && lb * lb < thrmax) atomicAdd(&hist[kb >> 20], 1u);
                });
                __syncthreads();
                find_bin(4096, ST_CL_TARGET);
                const int bb = sh.sel_bin;
                cl_complete = bb < 0;                                  // fewer than the target in all: the list holds every eligible tile
                const uint32_t through = cl_complete ? 0u : sh.sel_before + hist[bb];
                __syncthreads();
                if (cl_complete || through <= ST_CL_CAP) {   // (else: a bin of equal leading key bits larger than the list -- the row is swept this round)
                    const uint32_t bound_bits = cl_complete ? 0x7f800000u : (uint32_t)(bb + 1) << 20;
                    if (threadIdx.x == 0) sh.nsurv = 0;
                    __syncthreads();
                    sweep(false, [&](uint32_t kb, float lb, int J) {
                        const bool after_done = kb > done_bits || (kb == done_bits && J > done_j);
                        if (kb < bound_bits && after_done && lb * lb < thrmax) {
                            const int slot = atomicAdd(&sh.nsurv, 1);
                            if (slot < ST_CL_CAP) { clk[slot] = kb; clk[ST_CL_CAP + slot] = __float_as_uint(lb); clk[2 * ST_CL_CAP + slot] = (uint32_t)J; }
                        }
                    });
                    __syncthreads();
                    cl_n = min(sh.nsurv, ST_CL_CAP);
                    cl_valid = true;
                    __syncthreads();
                }
            }
            use_list = clk && cl_valid;
            prefix = 0; want = keep; all = false;
            for (int level = 0; level < 3 && !all; ++level) {
                const int shift = level == 0 ? 20 : level == 1 ? 8 : 0;
                const int nbins = level == 2 ? 256 : 4096;
                const uint32_t pmask = level == 0 ? 0u : level == 1 ? 0xfff00000u : 0xffffff00u;
                for (int q = threadIdx.x; q < nbins; q += THREADS) hist[q] = 0;
                __syncthreads();
                sweep(use_list, [&](uint32_t kb, float lb, int J) {
                    const bool after_done = kb > done_bits || (kb == done_bits && J > done_j);
                    if (kb < 0x7f800000u && after_done && lb * lb < thrmax && (kb & pmask) == prefix)
                        atomicAdd(&hist[(kb >> shift) & (nbins - 1)], 1u);
                });
                __syncthreads();
                find_bin(nbins, want);
                if (sh.sel_bin < 0) all = true;
                else { prefix |= (uint32_t)sh.sel_bin << shift; want -= sh.sel_before; }
                __syncthreads();
            }
            if (!use_list || !all || cl_complete) break;
            cl_valid = false;   // fewer than ST_KEEP eligible tiles left in the list, and tiles beyond its bound remain: rebuild, select again
        }
        const uint32_t cut_bits = all ? 0x7f7fffffu : prefix;   // take keys <= cut (ties resolved by the sort below)
        // ---- collect (at most ST_SURV; more than ST_SURV - ST_KEEP ties on one key value would be dropped)
        if (threadIdx.x == 0) sh.nsurv = 0;
        __syncthreads();
        sweep(use_list, [&](uint32_t kb, float lb, int J) {
            const bool after_done = kb > done_bits || (kb == done_bits && J > done_j);
            if (kb < 0x7f800000u && after_done && lb * lb < thrmax && kb <= cut_bits) {
                const int slot = atomicAdd(&sh.nsurv, 1);
                if (slot < ST_SURV) { sb.surv_lb[slot] = __uint_as_float(kb); sb.surv_vb[slot] = lb; sb.surv_j[slot] = J; }
            }
        });
        __syncthreads();
        int ns = min(sh.nsurv, ST_SURV);
        if (ns == 0) return 0;
        {   // sort by (rank key, J): bitonic over the next power of two >= ns slots
            int sortn = 2;
            while (sortn < ns) sortn <<= 1;
            for (int q = threadIdx.x; q < sortn; q += THREADS)
                if (q >= ns) { sb.surv_lb[q] = INFINITY; sb.surv_j[q] = 0x7fffffff; }
            __syncthreads();
            for (int k2 = 2; k2 <= sortn; k2 <<= 1)
                for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
                    for (int q = threadIdx.x; q < sortn; q += THREADS) {
                        const int p2 = q ^ j2;
                        if (p2 > q) {
                            const bool up = (q & k2) == 0;
                            const float lq = sb.surv_lb[q], lp = sb.surv_lb[p2];
                            const int jq = sb.surv_j[q], jp = sb.surv_j[p2];
                            const bool gt = lq > lp || (lq == lp && jq > jp);
                            if (gt == up) {
                                sb.surv_lb[q] = lp; sb.surv_lb[p2] = lq; sb.surv_j[q] = jp; sb.surv_j[p2] = jq;
                                const float t = sb.surv_vb[q]; sb.surv_vb[q] = sb.surv_vb[p2]; sb.surv_vb[p2] = t;
                            }
                        }
                    }
                    __syncthreads();
                }
        }
        sel.more = !all;          // the selection was cut at `keep`: later tiles remain
        if (ns > (int)keep && sel.more) ns = (int)keep;
        sel.last_bits = __float_as_uint(sb.surv_lb[ns - 1]);
        sel.last_j = sb.surv_j[ns - 1];
        return ns;
    }
}
// (the round's tiles have run: the cursor moves behind them)
__device__ __forceinline__ void st_round_done(TileSelect &sel) { sel.done_bits = sel.last_bits; sel.done_j = sel.last_j; }

// ---------------------------------------------------------------- control of a run of the stream (knnbf.hip, knnbk.hip)
// Decisions that steer the stream (skip a ranked tile whose bound has fallen behind the thresholds, early stop, budget) are
// taken by every wave from barrier-separated LDS state, for the tile AFTER the one in the stream and from the thresholds as
// merged through the tile BEFORE it -- a fixed lag, so runs are reproducible.

// the wave's insertion count and its rows' worst k-th distance, at the end of a tile
template <class Sh> __device__ __forceinline__ void st_publish(Sh &sh, int lane, int wave, int rowbase, float inv_scale2, int ins, int tdone)
{
    int wins = ins;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) wins += __shfl_xor(wins, off);
    float t = lane < 32 ? sh.thr[rowbase + lane] : -1.f;   // padding rows: -1
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) t = fmaxf(t, __shfl_xor(t, off));
    if (lane == 0) { sh.wave_ins[(tdone + 1) & 1][wave] = wins; sh.wave_thr[(tdone + 1) & 1][wave] = t * inv_scale2; }   // (the lists are in scaled units, the tile bounds are not)
}

// a slab's threshold test without a stream to hide it in: bit r = accumulator r of the lane's column passes its row's test
// (row r of the lane's column passes iff x_r . x_c > hb[r] + |x_c|^2 / 2; rj: the column's squared norm)
template <class Sh> __device__ __forceinline__ uint32_t st_test_only(const Sh &sh, const f32x16 &accP, float rj, int rowq)
{
    uint32_t pass = 0;
    const float hrj = 0.5f * rj;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 h4 = *reinterpret_cast<const float4 *>(&sh.hb[rowq + 8 * q]);
        const float hv[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) pass |= (accP[4 * q + e] > hv[e] + hrj ? 1u : 0u) << (4 * q + e);
    }
    return pass;
}

// ---- merge, cooperatively, of the survivors a slab left in the rows' candidate slots (sh.cand_d / cand_c / cnt) into the
// wave's sorted lists: a group of GL lanes (GL = KMAX: 16 or 32) holds one row's sorted list in registers, one entry per lane; a
// candidate's position is a popcount over the group's comparison ballot and the entries behind it move up by one lane (a DPP
// row shift for 16-lane groups).  64 / GL rows at a time -- the lane-per-row form walked every list through dependent LDS
// round trips (a fifth of the kernel).  col0: the slab's first column; join passes: sh.slab_id[idsel] holds the slab's gathered column indices.
template <int KMAX, bool JOIN, class Sh>
__device__ __forceinline__ void st_merge_lists(Sh &sh, int lane, int rowbase, int64_t grow0, int K, int KL, int32_t col0, int idsel, int &ins)
{
    constexpr int GL = KMAX;                  // lanes per row
    constexpr int NG = 64 / GL;               // rows per batch
    const int grpi = lane / GL, e = lane % GL;
    const int mycnt = lane < 32 ? sh.cnt[rowbase + lane] : 0;
    unsigned long long todo = __ballot(mycnt > 0);
    while (todo) {
        int rsel = -1;   // this group's row (relative to rowbase)
#pragma unroll
        for (int k = 0; k < NG; ++k) {
            const int r = todo ? (int)__builtin_ctzll(todo) : -1;
            if (todo) todo &= todo - 1;
            rsel = grpi == k ? r : rsel;
        }
        const int row = rowbase + max(rsel, 0);
        const bool live = rsel >= 0;
        const int nc = live ? sh.cnt[row] : 0;
        float ld = (live && e < KL) ? sh.list_d[row][e] : INFINITY;
        int32_t lc = (live && e < KL) ? sh.list_c[row][e] : 0x7fffffff;
        int q = 0;
        while (__ballot(q < nc)) {
            const bool on = q < nc;
            const float d = on ? sh.cand_d[row][q] : INFINITY;
            int32_t cc;
            if constexpr (JOIN) cc = on ? (int32_t)sh.slab_id[idsel][sh.cand_c[row][q]] : 0x7fffffff;
            else cc = on ? col0 + sh.cand_c[row][q] : 0x7fffffff;
            const bool before = e < KL && (ld < d || (ld == d && lc < cc));   // entries that stay ahead of the candidate
            const unsigned long long bb = __ballot(before);
            const unsigned long long gmask = (GL == 64) ? ~0ull : ((1ull << GL) - 1);
            const int pos = __popcll((bb >> (grpi * GL)) & gmask);
            bool skip = false;
            if constexpr (JOIN) {
                // gathered columns: the row itself and columns the row already lists may come by
                const unsigned long long dup = __ballot(e < KL && lc == cc);
                skip = ((dup >> (grpi * GL)) & gmask) != 0 || (int64_t)cc == grow0 + row;
            }
            float pd;
            int32_t pc;
            if constexpr (GL == 16) {
                pd = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, ld), 0x111, 0xf, 0xf, false));   // row_shr:1
                pc = __builtin_amdgcn_update_dpp(0, lc, 0x111, 0xf, 0xf, false);
            } else {
                pd = __shfl_up(ld, 1, GL);
                pc = __shfl_up(lc, 1, GL);
            }
            if (on && !skip && pos < KL) {
                ld = e > pos ? pd : (e == pos ? d : ld);
                lc = e > pos ? pc : (e == pos ? cc : lc);
                ins += (e == 0 && pos < K) ? 1 : 0;   // the yield that stops the tile phase counts what reaches the K entries handed on
            }
            ++q;
        }
        if (live) {
            if (e < KL) { sh.list_d[row][e] = ld; sh.list_c[row][e] = lc; }
            if (e == KL - 1) { sh.thr[row] = ld; sh.hb[row] = 0.5f * (sh.rrow[row] - ld); }
            if (e == 0) sh.cnt[row] = 0;
        }
    }
}

// (host) a tile kernel `tile`, or its join-pass form `join_pass`, over a.tile_count row tiles with `lds` bytes of dynamic LDS
inline int st_launch_tile(annchor_ctx *c, const KnnArgs &a, void (*tile)(KnnArgs), void (*join_pass)(KnnArgs), bool join, int threads, size_t lds,
                          const char *form)
{
    ANN_REQUIRE(c, lds <= 160 * 1024, ANNCHOR_ELIMIT, "streamed k-NN (%s form) needs %zu B of LDS", form, lds);
    void (*kernel)(KnnArgs) = join ? join_pass : tile;
    ANN_CHECK_HIP(c, hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kernel<<<a.tile_count, threads, lds, c->stream>>>(a);
    ANN_CHECK_HIP(c, hipGetLastError());
    return ANNCHOR_OK;
}
