// emd.hip -- exact optimal transport (Wasserstein / Kantorovich) between histograms.
//
// Replaces, for f = wasserstein (reference annchor/utils.py:75-86 ->
// pynndescent.distances.kantorovich(x, y, cost=M): restrict x, y to their supports,
// normalise each to unit mass, return the optimum of the transportation LP), the
// evaluator get_exact(f, X, IJ) of annchor/utils.py:110-177.
//
// Sinkhorn is NOT used for the returned value: SURVEY.md section 7 (hard part 2)
// measured entropic OT 30-100x outside the tolerance that parity needs (and inexact
// anchor distances void the triangle bounds).  The kernel is an exact primal-dual
// solver shaped for a wavefront:
//   * one wavefront per pair; lane j owns sink j (its demand, potential v_j, tentative
//     distance, predecessor) and lane i owns source i (supply, u_i);
//   * Dijkstra on reduced costs over the dense bipartite graph: "pop the nearest
//     unscanned sink" is a DPP min-reduction, "relax a source row" is one LDS row read
//     of the cost matrix executed by all lanes;
//   * the flow matrix F (n x m float64, <= 33 KB) lives in LDS, one slab per wave; the
//     ground-cost matrix (<= 32 KB) is staged in LDS once per workgroup;
//   * control flow is wave-uniform (scalar branches); no atomics, no global scratch.
// Three kernels: k_emd (successive shortest paths, any cost matrix, up to 64 bins; described above), k_emd_ns (transportation
// simplex for metric costs, one lane per node: solves of up to 64 nodes) and k_emd_wide (the same simplex with four node slots
// per lane, the basis tree in LDS and block pricing from global memory: solves of up to 256 nodes, reached through
// annchor_set_histograms_wide only).  A fourth, k_emd_points, runs k_emd_wide's solve on point clouds: uniform masses, the distance
// between points as ground cost (annchor_set_clouds_f32 / _f64).
// Latency/branch bound by nature: reported as pairs/s and
// microseconds per pair, not as an HBM or MFMA fraction.
//
// Layout of this file: what the four kernels share on the device (the work counters, the decode of a solve's pair, the end of a
// solve, the fused max-min pick, the DPP reductions); k_emd; k_emd_ns; emdw_solve with k_emd_wide and k_emd_points on top of it;
// then the host side -- one set of helpers (pick take-over, waves per workgroup, counters, the simplex kernels' launch, the
// -DEMD_PROFILE read-back) and the three ann_emd_*_launch entry points.
#include "pairkern.h"

#define EMD_MAXB 64
#define EMDW_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); } while (0)

// c->supp: the sticky failure flag at word 0, two work counters at words 4 and 5.  The launches use the counters in turn -- each
// claims its solves from `work` and zeroes `work_next` for the launch after it, so there is no memset between launches.
struct EmdCounters {
    int32_t *fail;  // set when a solve hits an iteration cap or meets a broken tree (sticky)
    int32_t *work;  // the next unclaimed solve, counted from the first one not handed out by position
    int32_t *work_next;
};

// max-min picking fused into a one-to-all launch (PairSource::pick_*): the launch derives its own anchor from the previous round's row
struct PickArgs {
    const double *row;
    double *runmin;
    int32_t *out;
    int reset, nx;
};

struct EmdArgs {
    const double *hist;
    const double *cost;
    int nb;
    int S;          // padded row stride of the flow slab (odd); 0: per solve, (number of sinks) | 1
    int waves;      // waves per block
    int slab_bytes; // LDS bytes per wave (flow slab + support index lists)
    PairArgs p;
    EmdCounters k;
    int reduce;     // metric ground cost: solve on the differences of the two (scaled) histograms
    long long *dbg; // -DEMD_PROFILE
    int dantzig_cap; // k_emd_ns: pivots under Dantzig's rule before Bland's takes over (-1: 16 (n + m) + 64; tests force 0)
    PickArgs pick;
    const int32_t *hs_bin;   // k_emd_ns<.., true>: [nx][32] bins of the non-zero entries (ascending), their masses, their number
    const double *hs_val;
    const int32_t *hs_cnt;
    double eps;     // k_emd_ns: an arc enters the basis when its reduced cost is below -eps (2^-43 x the largest ground cost)
};

// Solve t of a launch: its pair, wave-uniform, and where the result goes.  picked >= 0: the anchor a fused pick derived
// (emd_pick), which stands in for *a.anchor -- only a one-to-all launch is given a row to pick from (emd_pick_fill).
//
// k_emd_ns sits at its 128-VGPR cap and spills: these helpers stay __forceinline__, take the lane from their caller, and the two
// that run outside the decode take their argument structs by value, so that nothing of them stays live across the pivot loop.
__device__ __forceinline__ PairSlot emd_pair(const PairArgs &a, int64_t t, int picked)
{
    PairSlot s = pair_decode(a, t);
    if (picked >= 0) s.i = picked;
    s.i = __builtin_amdgcn_readfirstlane(s.i);
    s.j = __builtin_amdgcn_readfirstlane(s.j);
    return s;
}

// The end of solve t: NaN and the flag for a failed one, the store by lane 0, then the wave's next solve from the counter (the
// first wave_total ones were handed out by position).  LDS_SYNC: what the kernel puts between store and claim -- EMDW_SYNC for
// the kernels whose next solve rewrites LDS other lanes may still read, a wave barrier otherwise.
template <bool LDS_SYNC>
__device__ __forceinline__ int64_t emd_finish(const PairArgs a, const EmdCounters k, int64_t t, int64_t opos, double tot, bool failed,
                                              int64_t wave_total, int lane)
{
    if (failed) { tot = NAN; if (lane == 0) *k.fail = 1; }
    if (lane == 0) pair_store(a, t, opos, tot);
    if (LDS_SYNC) EMDW_SYNC();
    else __builtin_amdgcn_wave_barrier();
    int nxt = 0;
    if (lane == 0) nxt = atomicAdd(k.work, 1);
    return wave_total + (int64_t)__builtin_amdgcn_readfirstlane(nxt);
}

// The anchor of a max-min round (pickers.py:47-50), or -1 without a pick request: every wave derives it for itself from the
// previous round's row -- running minimum (idempotent: the first wave of workgroup 0 also stores it), first arg-max -- so the
// picker needs no launch of its own.
__device__ __forceinline__ int emd_pick(const PickArgs k, int lane, int wave)
{
    if (!k.row) return -1;
    double bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int j = lane; j < k.nx; j += 64) {
        const double d = k.row[j];
        const double v = k.reset ? d : fmin(k.runmin[j], d);
        if (blockIdx.x == 0 && wave == 0) k.runmin[j] = v;
        argmax_combine(bv, bi, v, j);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        argmax_combine(bv, bi, ov, oi);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *k.out = bi;
    return bi;
}

// ---- wave-level min over lanes (double), result broadcast; DPP, no LDS traffic
template <int CTRL, int ROW_MASK> __device__ __forceinline__ double dpp_f64(double v, double identity)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    int ilo = __double2loint(identity), ihi = __double2hiint(identity);
    lo = __builtin_amdgcn_update_dpp(ilo, lo, CTRL, ROW_MASK, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(ihi, hi, CTRL, ROW_MASK, 0xf, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double wave_min_f64(double v)
{
    const double inf = INFINITY;
    v = fmin(v, dpp_f64<0xb1, 0xf>(v, inf));   // quad_perm [1,0,3,2]
    v = fmin(v, dpp_f64<0x4e, 0xf>(v, inf));   // quad_perm [2,3,0,1]
    v = fmin(v, dpp_f64<0x141, 0xf>(v, inf));  // row_half_mirror
    v = fmin(v, dpp_f64<0x140, 0xf>(v, inf));  // row_mirror
    v = fmin(v, dpp_f64<0x142, 0xa>(v, inf));  // row_bcast:15 -> rows 1,3
    v = fmin(v, dpp_f64<0x143, 0xc>(v, inf));  // row_bcast:31 -> rows 2,3
    // lane 63 now holds the minimum of all 64 lanes
    int lo = __builtin_amdgcn_readlane(__double2loint(v), 63);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), 63);
    return __hiloint2double(hi, lo);
}

// Minimum of NON-NEGATIVE doubles (+inf allowed): they order like their bit patterns, so the high words are
// reduced first and the low words among the lanes that hold the minimal high word -- twelve 32-bit DPP minimum
// steps instead of six 64-bit ones made of two moves and a v_min_f64 each (the kernel is issue bound and this
// reduction runs once per Dijkstra pop).
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v)
{
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)0xffffffffu, (int)v, 0xb1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)0xffffffffu, (int)v, 0x4e, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)0xffffffffu, (int)v, 0x141, 0xf, 0xf, false));  // row_half_mirror
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)0xffffffffu, (int)v, 0x140, 0xf, 0xf, false));  // row_mirror
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)0xffffffffu, (int)v, 0x142, 0xa, 0xf, false));  // row_bcast:15 -> rows 1,3
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)0xffffffffu, (int)v, 0x143, 0xc, 0xf, false));  // row_bcast:31 -> rows 2,3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ double wave_min_nonneg_f64(double v)
{
    const uint32_t hi = (uint32_t)__double2hiint(v), lo = (uint32_t)__double2loint(v);
    const uint32_t mh = wave_min_u32(hi);
    const uint32_t ml = wave_min_u32(hi == mh ? lo : 0xffffffffu);
    return __hiloint2double((int)mh, (int)ml);
}

__device__ __forceinline__ double readlane_f64(double v, int lane)
{
    int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// Flow / mass type: double in general; int32 when both histograms are integer valued (then
// supplies x_i * sum(y) and demands y_j * sum(x) are exact integers and the flow slab is half
// the size, which doubles the waves a CU can hold).
__device__ __forceinline__ double rl(double v, int lane) { return readlane_f64(v, lane); }
__device__ __forceinline__ int rl(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ double tmin(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ int tmin(int a, int b) { return a < b ? a : b; }

// -DEMD_PROFILE: per-solve cycle counts by phase (small launches only), printed for the slowest solve of a launch
#ifdef EMD_PROFILE
#define EP_DECL long long ep_t = (long long)__builtin_readcyclecounter(), ep_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}; int ep_cnt[4] = {0, 0, 0, 0}
#define EP(i) do { const long long ep_n = (long long)__builtin_readcyclecounter(); ep_acc[i] += ep_n - ep_t; ep_t = ep_n; } while (0)
#define EP_CNT(i) (++ep_cnt[i])
#define EP_FLUSH(dbg, t, n, m) do { if ((dbg) && (t) < 4096 && lane == 0) { \
        for (int q = 0; q < 8; ++q) (dbg)[(t) * 16 + q] = ep_acc[q]; \
        for (int q = 0; q < 4; ++q) (dbg)[(t) * 16 + 8 + q] = ep_cnt[q]; \
        (dbg)[(t) * 16 + 12] = (n); (dbg)[(t) * 16 + 13] = (m); } } while (0)
#else
#define EP_DECL do { } while (0)
#define EP(i) do { } while (0)
#define EP_CNT(i) do { } while (0)
#define EP_FLUSH(dbg, t, n, m) do { } while (0)
#endif

// T: masses and flows in registers; FT: the flow slab's storage type (int16 when every flow fits: half the LDS per wave again)
template <typename T, typename FT> __global__ __launch_bounds__(1024) void k_emd(EmdArgs a)
{
    constexpr bool INTEGRAL = sizeof(T) == 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nb = a.nb;
    double *costL = reinterpret_cast<double *>(smem);                       // [nb][nb]
    unsigned char *slab = reinterpret_cast<unsigned char *>(costL + nb * nb) + (size_t)wave * a.slab_bytes;
    FT *F = reinterpret_cast<FT *>(slab);                                   // [<=64][S] flow slab
    int *rowsL = reinterpret_cast<int *>(slab + a.slab_bytes - 2 * EMD_MAXB * sizeof(int));  // [64] support of x
    int *colsL = rowsL + EMD_MAXB;                                          // [64] support of y
    for (int t = threadIdx.x; t < nb * nb; t += blockDim.x) costL[t] = a.cost[t];
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.k.work_next = 0;
    __syncthreads();

    // Solves are claimed one at a time from a counter: their durations differ by an order of magnitude (near pairs need a few
    // searches, far pairs scan the whole graph every time), and a fixed share per wave left most of the chip waiting for the
    // unluckiest wave of a launch.
    const int64_t wave_global = (int64_t)blockIdx.x * a.waves + wave;
    const int64_t wave_total = (int64_t)gridDim.x * a.waves;
    for (int64_t t = wave_global;;) {
        if (t >= a.p.n) break;
        EP_DECL;
        const PairSlot ps = emd_pair(a.p, t, -1);
        const double *hx = a.hist + (size_t)ps.i * nb, *hy = a.hist + (size_t)ps.j * nb;
        // masses and their sums in index order (sequential index order: exact parity
        // of the normalisation for non-integer inputs)
        const double xk = lane < nb ? hx[lane] : 0.0, yk = lane < nb ? hy[lane] : 0.0;
        double sa = 0, sb = 0;
        for (int k = 0; k < nb; ++k) { sa += readlane_f64(xk, k); sb += readlane_f64(yk, k); }
        // masses of bin `lane` in the solver's units: 1 / (sa * sb) (exact integers) or unit total mass
        T xm, ym;
        if (INTEGRAL) { xm = (T)(xk * sb); ym = (T)(yk * sa); }
        else { xm = (T)(xk / sa); ym = (T)(yk / sb); }
        if (a.reduce) {
            // metric ground cost (c_kk = 0, triangle inequality): an optimal plan leaves min(x_k, y_k) on bin k, so only the
            // differences travel -- sources and sinks become disjoint and fewer (two digits share most of their pixels), and
            // the saturated (k, k) arcs whose backward edges the shortest-path searches would otherwise walk are gone
            const T d = xm - ym;
            xm = d > (T)0 ? d : (T)0;
            ym = d < (T)0 ? -d : (T)0;
        }
        const unsigned long long mx = __ballot(xm != (T)0), my = __ballot(ym != (T)0);
        const int n = __popcll(mx), m = __popcll(my);
        const int S = a.S ? a.S : (m | 1);
        const unsigned long long below = (1ull << lane) - 1ull;
        if (xm != (T)0) rowsL[__popcll(mx & below)] = lane;
        if (ym != (T)0) colsL[__popcll(my & below)] = lane;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const int myrow = lane < n ? rowsL[lane] : 0;   // source `lane` is histogram bin myrow
        const int mycol = lane < m ? colsL[lane] : 0;   // sink `lane` is histogram bin mycol
        // supply of source `lane`, demand of sink `lane`: the masses of their bins
        T a_rem = __shfl(xm, myrow), b_rem = __shfl(ym, mycol);
        if (lane >= n) a_rem = (T)0;
        if (lane >= m) b_rem = (T)0;
        double u = 0.0;                                  // potential of source `lane`
        // v_j = min_i C[i][j] (first minimal source on ties): dual feasible with u = 0, and
        // arc (amin_j, j) is tight for every sink
        double v = INFINITY;
        int amin = 0;
        for (int i = 0; i < n; ++i) {
            const int r = __builtin_amdgcn_readlane(myrow, i);
            if (lane < m) {
                const double cc = costL[r * nb + mycol];
                if (cc < v) { v = cc; amin = i; }
            }
        }
        // zero the flow slab
        for (int i = 0; i < n; ++i)
            if (lane < m) F[i * S + lane] = (FT)0;
        __builtin_amdgcn_wave_barrier();
        // greedy start on the tight arcs (complementary slackness holds: flow only where the
        // reduced cost is zero).  For near-by histograms most mass sits on identical bins
        // (cost 0) and is routed here, before any shortest-path search.
        for (int j = 0; j < m; ++j) {
            const int i = __builtin_amdgcn_readlane(amin, j);
            const T f = tmin(rl(a_rem, i), rl(b_rem, j));
            if (f > (T)0) {
                if (lane == 0) F[i * S + j] = (FT)f;
                if (lane == i) a_rem -= f;
                if (lane == j) b_rem -= f;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

        EP(0);
        int guard = 64 * (n + m) + 1024;
        bool failed = false, dust = false;
        for (int s = 0; s < n && !dust && !failed; ++s) {
            const int rs = __builtin_amdgcn_readlane(myrow, s);
            for (;;) {
                const T as = rl(a_rem, s);
                if (!(as > (T)0)) break;
                if (--guard < 0) { failed = true; break; }
                // ---- Dijkstra from source s on reduced costs
                const double us = readlane_f64(u, s);
                // (reduced costs are >= 0 up to rounding: clamped, so that the tentative distances are non-negative
                // doubles -- the invariant the wave minimum below relies on)
                double dist = lane < m ? fmax(costL[rs * nb + mycol] - us - v, 0.0) : INFINITY;
                int pred = s;
                unsigned long long sinkdone = 0, srcdone = 1ull << s;
                double srcdist = 0.0;   // valid on lanes whose srcdone bit is set
                int srcfrom = -1;
                double mu = 0.0;
                // The search does not stop at the first sink with demand left: it goes on until the demand it has met covers
                // what source s still has to place (or every sink is scanned).  One shortest-path tree then carries several
                // augmentations -- a source whose mass splits over two or three sinks used to start its search over for each of
                // them and re-scan the same near sinks.
                int prank = -1;         // order in which THIS lane's sink was reached, among the sinks with demand left
                int nhit = 0;
                T need = as;
                EP(1); EP_CNT(0);
                for (;;) {
                    const bool open = lane < m && !((sinkdone >> lane) & 1ull);
                    // nearest open sink: non-negative doubles order like their bit patterns -- minimum of the high words first;
                    // only when several open sinks share it (equal distances: tight arcs at 0, symmetric costs) do the low words
                    // need their own reduction
                    const uint32_t dhi = open ? (uint32_t)__double2hiint(dist) : 0x7ff00000u, dlo = (uint32_t)__double2loint(dist);
                    const uint32_t mh = wave_min_u32(dhi);
                    unsigned long long hit = __ballot(open && dhi == mh);
                    double best;
                    if (hit & (hit - 1)) {
                        const uint32_t ml = wave_min_u32(open && dhi == mh ? dlo : 0xffffffffu);
                        hit = __ballot(open && dhi == mh && dlo == ml);
                        best = __hiloint2double((int)mh, (int)ml);
                    } else {
                        best = hit ? readlane_f64(dist, __ffsll((unsigned long long)hit) - 1) : INFINITY;
                    }
                    EP(2); EP_CNT(1);
                    if (!hit) break;                       // every sink scanned
                    const int js = __ffsll((unsigned long long)hit) - 1;  // first index on ties
                    sinkdone |= 1ull << js;
                    mu = best;
                    const T bj = rl(b_rem, js);
                    if (bj > (T)0) {
                        if (lane == js) prank = nhit;
                        ++nhit;
                        need -= tmin(need, bj);
                        if (!(need > (T)0)) break;
                    }
                    // sources with flow into js that are not scanned yet
                    const T fcol = lane < n ? (T)F[lane * S + js] : (T)0;
                    unsigned long long todo = __ballot(lane < n && fcol > (T)0 && !((srcdone >> lane) & 1ull));
                    EP(3);
                    while (todo) {
                        EP_CNT(2);
                        const int i = __ffsll((unsigned long long)todo) - 1;
                        todo &= todo - 1;
                        srcdone |= 1ull << i;
                        if (lane == i) { srcdist = mu; srcfrom = js; }
                        const int ri = __builtin_amdgcn_readlane(myrow, i);
                        const double ui = readlane_f64(u, i);
                        if (lane < m && !((sinkdone >> lane) & 1ull)) {
                            const double nd = fmax(mu + (costL[ri * nb + mycol] - ui - v), 0.0);
                            if (nd < dist) { dist = nd; pred = i; }
                        }
                    }
                    EP(4);
                }
                if (nhit == 0) { dust = true; break; }     // only rounding dust left
                // ---- potentials: every scanned node against the last distance popped -- the tree's arcs are tight afterwards
                if ((srcdone >> lane) & 1ull) u += mu - srcdist;
                if ((sinkdone >> lane) & 1ull) v -= mu - dist;
                EP(5);
                // ---- augment along the tree to every sink reached with demand left, nearest first; a path's bottleneck is taken
                // from the flows as the earlier augmentations of this search left them
                for (int k = 0; k < nhit; ++k) {
                    const int jend = __ffsll((unsigned long long)__ballot(prank == k)) - 1;
                    T delta = tmin(rl(a_rem, s), rl(b_rem, jend));
                    for (int j = jend; delta > (T)0;) {
                        const int i = __builtin_amdgcn_readlane(pred, j);
                        if (i == s) break;
                        const int jj = __builtin_amdgcn_readlane(srcfrom, i);
                        delta = tmin(delta, (T)F[i * S + jj]);   // uniform address: LDS broadcast
                        j = jj;
                    }
                    if (!(delta > (T)0)) continue;
                    for (int j = jend;;) {
                        const int i = __builtin_amdgcn_readlane(pred, j);
                        if (lane == 0) F[i * S + j] = (FT)((T)F[i * S + j] + delta);
                        if (i == s) break;
                        const int jj = __builtin_amdgcn_readlane(srcfrom, i);
                        if (lane == 0) F[i * S + jj] = (FT)((T)F[i * S + jj] - delta);
                        j = jj;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    if (lane == s) a_rem -= delta;
                    if (lane == jend) b_rem -= delta;
                    EP_CNT(3);
                }
                EP(6);
            }
        }
        // ---- objective
        double tot = 0.0;
        for (int i = 0; i < n; ++i) {
            const int r = __builtin_amdgcn_readlane(myrow, i);
            if (lane < m) tot += (double)F[i * S + lane] * costL[r * nb + mycol];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off);
        if (INTEGRAL) tot /= sa * sb;
        EP(7);
        EP_FLUSH(a.dbg, t, n, m);
        t = emd_finish<false>(a.p, a.k, t, ps.opos, tot, failed, wave_total, lane);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_emd_ns: the same LP by the transportation simplex on a spanning-tree basis, for metric ground costs (the common mass of
// the two histograms cancels: sources and sinks are disjoint bins, n + m <= 64 -- ONE LANE PER NODE).
//
// Why: the shortest-path solver above does ~200-350 Dijkstra pops per solve on the digits (up to 1700 on far pairs: ~100
// searches of ~17 pops), each a dependent chain of a DPP minimum, an LDS column read and LDS row reads; an anchor round lasts as
// long as its slowest solve.  The simplex needs 20-30 pivots (at most ~75; tools/sim/emd_simplex_sim.cpp counts them on the same
// pairs) and keeps the whole basis in registers:
//   * lane k < n is source k, lane n + j sink j; per lane: histogram bin, parent in the basis tree, flow on the arc to the
//     parent (always source -> sink), potential, and the SET OF NODES BELOW IT as a 64-bit mask (`sub`);
//   * pricing (Dantzig): every sink lane scans the sources (one LDS cost read each, independent), one wave minimum;
//   * the cycle of the entering arc (x, y) needs no tree walk: the ancestors of x are the lanes whose `sub` holds bit x (one
//     ballot), likewise y; the cycle's arcs are the lanes in exactly one of the two sets; which of them lose flow follows from
//     the node type and the side; theta and the leaving arc are one wave minimum, the flow update one masked add;
//   * the part of the tree cut off by the leaving arc is `sub` of its lower node (one readlane): potentials shift by the
//     entering arc's reduced cost there, the `sub` masks of the old / new ancestors lose / gain it, and the parent pointers
//     along the short path from the entering arc's end to the leaving arc are reversed;
//   * start: row-minimum rule (each step closes exactly one line: a spanning tree with n + m - 1 arcs, degenerate ones
//     included), potentials in reverse closing order.
// No flow slab: LDS holds the ground costs and 512 B per wave.  Degenerate pivots are rare (< 1 %); should Dantzig's rule not
// finish within its cap the loop continues under Bland's rule (lowest index in, lowest index out), which cannot cycle.
#define EMD_NS_WAVE_BYTES (2 * EMD_MAXB * (int)sizeof(int) + 64 * (int)sizeof(double))

template <typename T> __device__ __forceinline__ T wave_min_nonneg(T v);
template <> __device__ __forceinline__ int wave_min_nonneg<int>(int v) { return (int)wave_min_u32((uint32_t)v); }
template <> __device__ __forceinline__ double wave_min_nonneg<double>(double v) { return wave_min_nonneg_f64(v); }
__device__ __forceinline__ unsigned long long rl64(unsigned long long v, int lane)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}

// SPARSE: histograms of more than 64 bins with at most 32 non-zero entries each (annchor_set_histograms keeps them as (bin, mass)
// lists): lanes 0..31 take x's entries, lanes 32..63 y's; the ground costs stay in global memory (read at the start of a solve, in
// the start rule and for the objective -- never per pivot)
template <typename T, bool SPARSE> __global__ __launch_bounds__(1024) void k_emd_ns(EmdArgs a)
{
    constexpr bool INTEGRAL = sizeof(T) == 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nb = a.nb;
    double *costL = reinterpret_cast<double *>(smem);                       // [nb][nb] (not SPARSE)
    // per wave: [64] support of x, [64] support of y (ints), [64] potentials by node (doubles)
    unsigned char *wv = reinterpret_cast<unsigned char *>(costL + (SPARSE ? 0 : nb * nb)) + (size_t)wave * EMD_NS_WAVE_BYTES;
    auto COST = [&](int ra, int cb) -> double { return SPARSE ? a.cost[(size_t)ra * nb + cb] : costL[ra * nb + cb]; };
    int *rowsL = reinterpret_cast<int *>(wv);
    int *colsL = rowsL + EMD_MAXB;
    double *potL = reinterpret_cast<double *>(wv + 2 * EMD_MAXB * sizeof(int));
    if (!SPARSE)
        for (int t = threadIdx.x; t < nb * nb; t += blockDim.x) costL[t] = a.cost[t];
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.k.work_next = 0;
    __syncthreads();
    const double eps = a.eps;
    const unsigned long long lanebit = 1ull << lane;
    const int picked = emd_pick(a.pick, lane, wave);

    const int64_t wave_global = (int64_t)blockIdx.x * a.waves + wave;
    const int64_t wave_total = (int64_t)gridDim.x * a.waves;
    for (int64_t t = wave_global;;) {
        if (t >= a.p.n) break;
        EP_DECL;
        const PairSlot ps = emd_pair(a.p, t, picked);
        const int pi = ps.i, pj = ps.j;
        double sa = 0, sb = 0;
        T xm, ym;
        int ebin = lane;   // histogram bin of the entry this lane holds (dense: bin = lane)
        if constexpr (SPARSE) {
            const int side = lane >> 5, e = lane & 31;
            const int cx = a.hs_cnt[pi], cy = a.hs_cnt[pj];
            const int pidx = side ? pj : pi, cnt = side ? cy : cx;
            ebin = e < cnt ? a.hs_bin[(size_t)pidx * 32 + e] : -1 - lane;   // (empty slots: distinct negative numbers, matching nothing)
            const double ev = e < cnt ? a.hs_val[(size_t)pidx * 32 + e] : 0.0;
            for (int k = 0; k < cx; ++k) sa += readlane_f64(ev, k);          // entries are in bin order: the dense loop's sums
            for (int k = 0; k < cy; ++k) sb += readlane_f64(ev, 32 + k);
            T mine;
            if (INTEGRAL) mine = (T)(ev * (side ? sa : sb));
            else mine = (T)(ev / (side ? sb : sa));
            // the other histogram's mass on the same bin
            T other = (T)0;
            for (int k = 0; k < cy; ++k) {
                const int b = __builtin_amdgcn_readlane(ebin, 32 + k);
                const T v = rl(mine, 32 + k);
                if (side == 0 && ebin == b) other = v;
            }
            for (int k = 0; k < cx; ++k) {
                const int b = __builtin_amdgcn_readlane(ebin, k);
                const T v = rl(mine, k);
                if (side == 1 && ebin == b) other = v;
            }
            const T d = mine - other;     // the common mass stays where it is (metric cost)
            const T pos = d > (T)0 ? d : (T)0;
            xm = side == 0 ? pos : (T)0;
            ym = side == 1 ? pos : (T)0;
        } else {
            const double *hx = a.hist + (size_t)pi * nb, *hy = a.hist + (size_t)pj * nb;
            const double xk = lane < nb ? hx[lane] : 0.0, yk = lane < nb ? hy[lane] : 0.0;
            for (int k = 0; k < nb; ++k) { sa += readlane_f64(xk, k); sb += readlane_f64(yk, k); }
            if (INTEGRAL) { xm = (T)(xk * sb); ym = (T)(yk * sa); }
            else { xm = (T)(xk / sa); ym = (T)(yk / sb); }
            // the common mass stays where it is (metric cost): only the differences travel
            const T d = xm - ym;
            xm = d > (T)0 ? d : (T)0;
            ym = d < (T)0 ? -d : (T)0;
        }
        const unsigned long long mx = __ballot(xm != (T)0), my = __ballot(ym != (T)0);
        const int n = __popcll(mx), m = __popcll(my), N = n + m;
        double tot = 0.0;
        bool failed = false;
        if (n > 0 && m > 0) {
            const unsigned long long below = lanebit - 1ull;
            if (xm != (T)0) rowsL[__popcll(mx & below)] = lane;
            if (ym != (T)0) colsL[__popcll(my & below)] = lane;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            // ---- nodes: lane k < n = source k, lane n + j = sink j
            const bool is_src = lane < n, is_snk = lane >= n && lane < N;
            const int holder = is_src ? rowsL[lane] : (is_snk ? colsL[lane - n] : 0);   // the lane that holds this node's entry
            const int ebin_of = __shfl(ebin, holder);   // (every lane takes part: a holder lane may lie beyond the N node lanes)
            const int bin = lane < N ? ebin_of : 0;
            if constexpr (SPARSE) {   // the lists now carry the nodes' bins (dense: they already do)
                __builtin_amdgcn_wave_barrier();
                if (is_src) rowsL[lane] = bin;
                if (is_snk) colsL[lane - n] = bin;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            }
            // ---- the arcs, dealt over the lanes: arc a = slot * 64 + lane is (source a / m, sink a % m); its ground cost and the
            // LDS offsets of its ends' potentials stay in registers for the whole solve (<= 16 slots: n m <= 1024)
            const int nm = n * m;
            double ac[16];
            int aij[16];
            {
                const float inv_m = 1.0f / (float)m;
#pragma unroll
                for (int sl = 0; sl < 16; ++sl) {
                    ac[sl] = 0.0; aij[sl] = -1;
                    if (sl * 64 < nm) {
                        const int aidx = sl * 64 + lane;
                        const int ac_ = min(aidx, nm - 1);
                        const int ai = (int)(((float)ac_ + 0.5f) * inv_m);
                        const int aj = ac_ - ai * m;
                        ac[sl] = COST(rowsL[ai], colsL[aj]);
                        if (aidx < nm) aij[sl] = (ai << 16) | (n + aj);
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
            const T mass_x = __shfl(xm, holder), mass_y = __shfl(ym, holder);
            T rem = is_src ? mass_x : (is_snk ? mass_y : (T)0);       // supply / demand still to place (start rule)
            const unsigned long long allmask = N == 64 ? ~0ull : ((1ull << N) - 1ull);
            const unsigned long long srcmask = (1ull << n) - 1ull, snkmask = allmask & ~srcmask;
            int parent = -1;
            T pflow = (T)0;
            double pot = 0.0, pcost = 0.0;
            unsigned long long sub = lane < N ? lanebit : 0ull;
            int ord = -1;
            // ---- start: row-minimum rule.  The first open source takes its cheapest open sink; the assignment exhausts one of
            // the two, which closes and hangs below the other (never the last source while several sinks are open: with the totals
            // balanced their demands are zero then, and they close one by one on degenerate arcs).
            unsigned long long open = allmask;
            int step = 0;
            EP(0);
            while (open & (open - 1)) {
                const unsigned long long osrc = open & srcmask;
                const int i = __ffsll(osrc) - 1;                       // (an open source always exists while two lines are open)
                const int bi = __builtin_amdgcn_readlane(bin, i);
                const bool cand = is_snk && ((open >> lane) & 1ull);
                const double c = cand ? COST(bi, bin) : INFINITY;
                // (minimum of the high words first; the low words only when several candidates share it)
                const uint32_t chi = (uint32_t)__double2hiint(c);
                const uint32_t mh = wave_min_u32(chi);
                unsigned long long hitc = __ballot(cand && chi == mh);
                if (hitc & (hitc - 1)) {
                    const uint32_t ml = wave_min_u32(cand && chi == mh ? (uint32_t)__double2loint(c) : 0xffffffffu);
                    hitc = __ballot(cand && chi == mh && (uint32_t)__double2loint(c) == ml);
                }
                const int j = __ffsll(hitc) - 1;
                const double cmin = readlane_f64(c, j);
                const T ai = rl(rem, i), bj = rl(rem, j);
                const T f = tmin(ai, bj);
                const unsigned long long osnk = open & snkmask;
                const bool last_src = (osrc & (osrc - 1)) == 0, last_snk = (osnk & (osnk - 1)) == 0;
                // (the exhausted line closes; never the last line of its kind while several of the other kind are open -- with
                // balanced totals what those still hold is zero, or rounding dust for non-integer masses)
                const bool close_src = (ai - f > (T)0) ? (last_snk && !last_src) : !(last_src && !last_snk);
                const int cn = close_src ? i : j, on = close_src ? j : i;
                if (lane == i || lane == j) rem -= f;
                const unsigned long long csub = rl64(sub, cn);
                if (lane == cn) { parent = on; pflow = f; pcost = cmin; ord = step; }
                if (lane == on) sub |= csub;
                open &= ~(1ull << cn);
                ++step;
            }
            EP(1);
            // potentials: the root (the line left open) at 0, the others in reverse closing order -- u_i + v_j = c_ij on tree arcs
            for (int s = step - 1; s >= 0; --s) {
                const int cn = __ffsll((unsigned long long)__ballot(ord == s)) - 1;
                const int pn = __builtin_amdgcn_readlane(parent, cn);
                const double pp = readlane_f64(pot, pn);
                if (lane == cn) pot = pcost - pp;
            }
            EP(2);
            // ---- pivots
            const int dantzig_cap = a.dantzig_cap >= 0 ? a.dantzig_cap : 16 * N + 64, total_cap = dantzig_cap + 4096;
            int piv = 0;
            for (;; ++piv) {
                if (piv >= total_cap) { failed = true; break; }
                const bool bland = piv >= dantzig_cap;
                // pricing: every lane its <= 16 arcs; the ends' potentials through LDS (independent reads, one wait)
                potL[lane] = pot;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                double best = 0.0;
                int bestij = -1;
                // (four slots per uniform branch: their eight LDS reads are in flight together)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if (g * 256 < nm) {
                        double pu[4], pv[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int e = aij[4 * g + q] < 0 ? 0 : aij[4 * g + q];
                            pu[q] = potL[e >> 16];
                            pv[q] = potL[e & 0xffff];
                        }
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const double rc = (ac[4 * g + q] - pu[q]) - pv[q];
                            const bool take = aij[4 * g + q] >= 0 && (bland ? (bestij < 0 && rc < -eps) : (rc < best));
                            if (take) { best = rc; bestij = aij[4 * g + q]; }
                        }
                    }
                }
                __builtin_amdgcn_wave_barrier();
                EP(3); EP_CNT(0);
                int x, y;
                double rcin;
                {
                    int from;
                    if (!bland) {
                        rcin = wave_min_f64(best);
                        if (!(rcin < -eps)) break;                     // optimal
                        from = __ffsll((unsigned long long)__ballot(bestij >= 0 && best == rcin)) - 1;
                    } else {
                        // lowest arc index: a lane's first hit is its lowest slot; arcs are numbered slot * 64 + lane
                        const unsigned long long cands = __ballot(bestij >= 0);
                        if (!cands) break;
                        const uint32_t key = bestij >= 0 ? (uint32_t)((bestij >> 16) * 64 + (bestij & 0xffff)) : 0xffffffffu;
                        const uint32_t kmin = wave_min_u32(key);
                        from = __ffsll((unsigned long long)__ballot(key == kmin)) - 1;
                        rcin = readlane_f64(best, from);
                    }
                    const int e = __builtin_amdgcn_readlane(bestij, from);
                    x = e >> 16; y = e & 0xffff;
                }
                // ---- the cycle: tree path x ~> y plus the entering arc.  Ancestors (incl. the node itself) by `sub`.
                const unsigned long long AX = __ballot((sub >> x) & 1ull), AY = __ballot((sub >> y) & 1ull);
                const unsigned long long xs = AX & ~AY, ys = AY & ~AX;
                // theta enters on x -> y and travels y ~> top ~> x: upwards on y's side (a sink below a source loses), downwards on
                // x's side (a source below a sink loses)
                const unsigned long long dec = (xs & srcmask) | (ys & snkmask);
                const bool in_dec = (dec >> lane) & 1ull;
                T theta;
                int leave;
                if (INTEGRAL) {
                    theta = wave_min_nonneg<T>(in_dec ? pflow : (T)0x7fffffff);
                } else {
                    theta = wave_min_nonneg<T>(in_dec ? pflow : (T)INFINITY);
                }
                {
                    const unsigned long long ties = __ballot(in_dec && pflow == theta);
                    leave = __ffsll(ties) - 1;
                    if (bland && (ties & (ties - 1))) {
                        // lowest arc index (sink-major) among the ties
                        const int asrc = is_src ? lane : parent, asnk = is_src ? parent : lane;
                        const uint32_t aidx = ((ties >> lane) & 1ull) ? (uint32_t)(asnk * 64 + asrc) : 0xffffffffu;
                        const uint32_t amin = wave_min_u32(aidx);
                        leave = __ffsll((unsigned long long)__ballot(aidx == amin)) - 1;
                    }
                }
                if (((xs | ys) >> lane) & 1ull) pflow += in_dec ? -theta : theta;
                EP(4);
                // ---- the tree: T2 = what hangs below the leaving arc; it re-attaches through the entering arc
                const unsigned long long T2 = rl64(sub, leave);
                const bool on_x = (xs >> leave) & 1ull;
                const int q = on_x ? x : y, p = on_x ? y : x;
                if ((T2 >> lane) & 1ull) pot += (is_src == (q < n)) ? rcin : -rcin;
                else if ((sub >> leave) & 1ull) sub &= ~T2;              // old ancestors of the cut part
                if (!((T2 >> lane) & 1ull) && ((sub >> p) & 1ull)) sub |= T2;   // its new ancestors: p and everything above p
                int w = q, cpar = p;
                T cflow = theta;
                unsigned long long prevsub = 0ull;
                for (;;) {
                    const int opar = __builtin_amdgcn_readlane(parent, w);
                    const T oflow = rl(pflow, w);
                    const unsigned long long osub = rl64(sub, w);
                    if (lane == w) { parent = cpar; pflow = cflow; sub = T2 & ~prevsub; }
                    if (w == leave) break;
                    cpar = w; cflow = oflow; prevsub = osub; w = opar;
                    EP_CNT(1);
                }
                EP(5);
            }
            // ---- objective: flow x cost over the tree arcs
            {
                const int pb = __shfl(bin, parent < 0 ? lane : parent);
                const double cst = (lane < N && parent >= 0) ? COST(is_src ? bin : pb, is_src ? pb : bin) : 0.0;
                tot = (lane < N && parent >= 0) ? (double)pflow * cst : 0.0;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off);
            if (INTEGRAL) tot /= sa * sb;
        }
        EP(6);
        EP_FLUSH(a.dbg, t, n, m);
        t = emd_finish<false>(a.p, a.k, t, ps.opos, tot, failed, wave_total, lane);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_emd_wide: the transportation simplex of k_emd_ns for solves of up to 256 nodes -- NODE SLOTS: lane l looks after nodes l,
// l + 64, l + 128 and l + 192, and every lane-parallel step runs once per occupied slot (a wave-uniform count: a 65-node solve
// does two slots, not four).  Reached only by contexts bound through annchor_set_histograms_wide whose data k_emd_ns cannot take
// (dense rows of 65 .. 256 bins, or (bin, mass) lists of up to 128 entries): same LP, same terms (metric ground cost, common mass
// cancelled, int32 flows for integral histograms, float64 costs / potentials / objective).
//   * the basis tree lives in LDS, 8 KB per wave: per node its histogram bin, its parent, the flow on the arc to the parent
//     (always source -> sink), its potential, a visit stamp.  There are no `sub` masks: the cycle of the entering arc is found by a
//     pointer walk (stamp the ancestors of x, climb from y to the first stamped node), and the part of the tree the leaving arc
//     cuts off by every node climbing towards the root until it meets the arc's lower end -- all slots climb together, one
//     wave-uniform loop;
//   * the n m <= 16 384 arcs do not fit in registers: pricing reads the ground costs from global memory (512 KB at 256 bins: they
//     stay in L2), BY BLOCKS of whole sources holding at most 1024 arcs, taken round robin; Dantzig's rule within the block; the
//     basis is optimal after one clean sweep of all blocks.  Beyond the Dantzig cap Bland's rule takes over: blocks from the first
//     one upwards, lowest arc index in, lowest arc index among the ties out (one order, source-major, for both);
//   * every loop is bounded: pivots by a cap scaled to the node count (NaN and the `fail` flag at the cap), block scans between
//     two pivots by the number of blocks, every tree walk by the node count (a longer walk means a broken tree: `fail` as well);
//   * start (row-minimum rule), work claiming from a counter, resident workgroups only and the fused max-min pick: as k_emd_ns.
#define EMDW_MAXN 256
#define EMDW_BLOCK_ARCS 1024
#define EMDW_WAVE_BYTES (4 * EMDW_MAXN * (int)sizeof(int) + 2 * EMDW_MAXN * (int)sizeof(double))

struct EmdWideArgs {
    const double *hist;      // dense rows [nx][nb] (stride == 0)
    const double *cost;
    int nb;
    int stride;              // > 0: (bin, mass) lists [nx][stride] in hs_bin / hs_val, their lengths in hs_cnt
    int waves;
    PairArgs p;
    EmdCounters k;
    int dantzig_cap;         // -1: 16 N + 64
    PickArgs pick;
    const int32_t *hs_bin;
    const double *hs_val;
    const int32_t *hs_cnt;
    double eps;
};

template <typename T> __device__ __forceinline__ T emdw_big();
template <> __device__ __forceinline__ int emdw_big<int>() { return 0x7fffffff; }
template <> __device__ __forceinline__ double emdw_big<double>() { return INFINITY; }

// The ground cost of the wide simplex, by NODE (source i, sink v).  It is read in three places -- the start rule, the pricing and the
// objective -- and always through one of these.  EmdwHistCost: the histogram kernels' bound cost matrix, by the nodes' bins.
// EmdwPointCost: the distance between two points of a pair of clouds whose coordinates the wave holds in LDS, computed when read:
//   dim 1: |x - y|;  dim > 1: sqrt(sum over k in order of t_k * t_k), t_k = x[k] - y[k], every operation rounded on its own, the
//   sum started from the k = 0 product, correctly rounded sqrt (ERP's `dist`, seqdp.hip) -- the same bits whichever end comes first.
struct EmdwHistCost {
    const double *cost;
    const int *binL;
    int nb;
    __device__ __forceinline__ double operator()(int i, int v) const { return cost[(size_t)binL[i] * nb + binL[v]]; }
};

template <int DIM> struct EmdwPointCost {
    const double *xyL;   // [N][DIM]
    __device__ __forceinline__ double operator()(int i, int v) const
    {
        const double *p = xyL + i * DIM, *q = xyL + v * DIM;
        double t = p[0] - q[0];
        if (DIM == 1) return fabs(t);
        double s = t * t;
#pragma unroll
        for (int k = 1; k < DIM; ++k) {
            t = p[k] - q[k];
            s = s + t * t;
        }
        return __dsqrt_rn(s);
    }
};

// One solve: nodes 0 .. n - 1 are the sources, n .. n + m - 1 the sinks; pflL holds what each supplies / demands (balanced totals)
// and `cost` can be read for every (source, sink).  Returns sum of flow x cost over the optimal basis (the caller scales it);
// `failed` is set at a cap or on a broken tree.
template <typename T, typename Cost>
__device__ __forceinline__ double emdw_solve(const Cost &cost, const int n, const int m, int *parL, int *markL, int *ordL, T *pflL,
                                             double *potL, const double eps, const int cap_in, bool &failed)
{
    const int lane = threadIdx.x & 63;
    const int N = n + m;
    double tot = 0.0;
    const int slots = (N + 63) >> 6;
    for (int s = 0; s < slots; ++s) {
        const int v = s * 64 + lane;
        if (v < N) { parL[v] = -2; markL[v] = 0; potL[v] = 0.0; }   // (-2: an open line of the start rule)
    }
    EMDW_SYNC();
    // ---- start: row-minimum rule, as k_emd_ns.  The open sources are always cur .. n - 1 (only the first open source
    // ever closes); N - 1 steps, each closes one line and hangs it below the other end of its arc.
    int cur = 0, nso = n, nko = m;
    for (int step = 0; step < N - 1; ++step) {
        const int i = cur;
        double c = INFINITY;
        int cj = 0x7fffffff;
        for (int s = n >> 6; s < slots; ++s) {
            const int v = s * 64 + lane;
            if (v >= n && v < N && parL[v] == -2) {
                const double cc = cost(i, v);
                if (cc < c) { c = cc; cj = v; }
            }
        }
        const double cmin = wave_min_f64(c);
        const int j = (int)wave_min_u32(c == cmin ? (uint32_t)cj : 0xffffffffu);   // (first minimal sink)
        if (j < n || j >= N) { failed = true; break; }                            // (no open sink: cannot happen while two lines are open)
        const T ai = pflL[i], bj = pflL[j];
        const T f = tmin(ai, bj);
        const bool last_src = nso == 1, last_snk = nko == 1;
        const bool close_src = (ai - f > (T)0) ? (last_snk && !last_src) : !(last_src && !last_snk);
        const int cn = close_src ? i : j, on = close_src ? j : i;
        EMDW_SYNC();
        if (lane == 0) {
            pflL[on] = (close_src ? bj : ai) - f;
            pflL[cn] = f;
            parL[cn] = on;
            potL[cn] = cmin;     // (the arc's cost: turned into the potential below)
            ordL[step] = cn;
        }
        if (close_src) { ++cur; --nso; } else --nko;
        EMDW_SYNC();
    }
    if (!failed) {
        // the root (the line left open) at 0, the others in reverse closing order: u_i + v_j = c_ij on tree arcs
        uint32_t rk = 0xffffffffu;
        for (int s = 0; s < slots; ++s) {
            const int v = s * 64 + lane;
            if (v < N && parL[v] == -2) rk = min(rk, (uint32_t)v);
        }
        const int root = (int)wave_min_u32(rk);
        EMDW_SYNC();
        if (lane == 0) { parL[root] = -1; potL[root] = 0.0; }
        EMDW_SYNC();
        for (int s = N - 2; s >= 0; --s) {
            const int cn = ordL[s];
            const double pp = potL[parL[cn]];
            const double pc = potL[cn];
            EMDW_SYNC();
            if (lane == 0) potL[cn] = pc - pp;
            EMDW_SYNC();
        }
    }
    // ---- pivots
    const int dantzig_cap = cap_in >= 0 ? cap_in : 16 * N + 64, total_cap = dantzig_cap + 64 * N + 4096;   // (Bland's rule alone: up to ~24 N pivots on 256-node solves)
    const int bs = max(1, EMDW_BLOCK_ARCS / m), nblk = (n + bs - 1) / bs;   // whole sources per block
    const float inv_m = 1.0f / (float)m;
    int piv = 0, blk = 0, clean = 0;
    while (!failed) {
        if (piv >= total_cap) { failed = true; break; }
        const bool bland = piv >= dantzig_cap;
        // ---- pricing: the block's arcs dealt over the lanes, arc e = (source i0 + e / m, sink e % m)
        const int i0 = blk * bs, na = min(bs, n - i0) * m;
        double best = 0.0;
        int bestij = -1;
        for (int k = 0; k * 64 < na; ++k) {
            const int e = k * 64 + lane;
            const int ec = min(e, na - 1);
            const int il = (int)(((float)ec + 0.5f) * inv_m);
            const int i = i0 + il, v = n + (ec - il * m);
            const double rc = (cost(i, v) - potL[i]) - potL[v];
            const bool take = e < na && (bland ? (bestij < 0 && rc < -eps) : (rc < best));
            if (take) { best = rc; bestij = (i << 16) | v; }
        }
        int x, y;
        double rcin;
        {
            int from;
            if (!bland) {
                rcin = wave_min_f64(best);
                from = rcin < -eps ? __ffsll((unsigned long long)__ballot(bestij >= 0 && best == rcin)) - 1 : -1;
            } else {
                // lowest arc index: a lane's first hit is its lowest; (i << 16) | v orders the arcs source-major
                const uint32_t key = bestij >= 0 ? (uint32_t)bestij : 0xffffffffu;
                const uint32_t kmin = wave_min_u32(key);
                from = kmin != 0xffffffffu ? __ffsll((unsigned long long)__ballot(key == kmin)) - 1 : -1;
                rcin = from >= 0 ? readlane_f64(best, from) : 0.0;
            }
            if (from < 0) {                                  // a clean block
                if (++clean >= nblk) break;                  // ... and a clean sweep: optimal
                blk = blk + 1 < nblk ? blk + 1 : 0;
                continue;
            }
            const int e = __builtin_amdgcn_readlane(bestij, from);
            x = e >> 16; y = e & 0xffff;
        }
        // ---- the cycle: tree path x ~> apex <~ y plus the entering arc
        const int stamp = piv + 1;
        {
            int w = x, g = 0;
            for (; w >= 0 && g <= N; ++g) { if (lane == 0) markL[w] = stamp; w = parL[w]; }
            if (w >= 0) { failed = true; break; }
        }
        EMDW_SYNC();
        int apex = y;
        {
            int g = 0;
            for (; apex >= 0 && g <= N && markL[apex] != stamp; ++g) apex = parL[apex];
            if (apex < 0 || g > N) { failed = true; break; }
        }
        // theta enters on x -> y and travels y ~> apex ~> x: upwards on y's side (a sink below a source loses), downwards on
        // x's side (a source below a sink loses); the leaving arc is the lowest-numbered one (source-major) among the ties
        T theta = emdw_big<T>();
        int leave = -1;
        uint32_t lkey = 0xffffffffu;
        bool on_x = false;
        for (int w = y, g = 0; w != apex && g <= N; ++g) {   // (both paths were just walked: at most N arcs each)
            const int p = parL[w];
            if (w >= n) {
                const T f = pflL[w];
                const uint32_t key = ((uint32_t)p << 16) | (uint32_t)w;
                if (f < theta || (f == theta && key < lkey)) { theta = f; leave = w; lkey = key; on_x = false; }
            }
            w = p;
        }
        for (int w = x, g = 0; w != apex && g <= N; ++g) {
            const int p = parL[w];
            if (w < n) {
                const T f = pflL[w];
                const uint32_t key = ((uint32_t)w << 16) | (uint32_t)p;
                if (f < theta || (f == theta && key < lkey)) { theta = f; leave = w; lkey = key; on_x = true; }
            }
            w = p;
        }
        if (leave < 0) { failed = true; break; }
        // ---- what hangs below the leaving arc (old parents): every node climbs until it meets `leave` or the root
        bool in2[4];
        {
            int w[4];
            bool act[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) { w[s] = s * 64 + lane; act[s] = s < slots && w[s] < N; in2[s] = false; }
            bool climbing = true;
            for (int g = 0; g <= N && climbing; ++g) {
                bool any = false;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    if (act[s]) {
                        if (w[s] == leave) { in2[s] = true; act[s] = false; }
                        else { w[s] = parL[w[s]]; if (w[s] < 0) act[s] = false; }
                    }
                    any = any || act[s];
                }
                climbing = __any(any);
            }
            if (climbing) { failed = true; break; }   // (a climb longer than N: a broken tree)
        }
        EMDW_SYNC();
        // flows round the cycle
        if (lane == 0) {
            for (int w = y, g = 0; w != apex && g <= N; w = parL[w], ++g) pflL[w] += w >= n ? -theta : theta;
            for (int w = x, g = 0; w != apex && g <= N; w = parL[w], ++g) pflL[w] += w < n ? -theta : theta;
        }
        // the cut part re-attaches through the entering arc: q is its end inside, p the one outside; potentials shift by the
        // entering arc's reduced cost there
        const int q = on_x ? x : y, p = on_x ? y : x;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int v = s * 64 + lane;
            if (in2[s]) potL[v] += ((v < n) == (q < n)) ? rcin : -rcin;
        }
        EMDW_SYNC();
        // parent pointers along q ~> leave are reversed (one lane: `leave` lies on the path from q to the apex walked above,
        // so the walk ends within N steps)
        if (lane == 0) {
            int w = q, cpar = p;
            T cflow = theta;
            for (int g = 0; g <= N; ++g) {
                const int opar = parL[w];
                const T oflow = pflL[w];
                parL[w] = cpar; pflL[w] = cflow;
                if (w == leave || opar < 0) break;
                cpar = w; cflow = oflow; w = opar;
            }
        }
        EMDW_SYNC();
        ++piv;
        clean = 0;
        blk = piv >= dantzig_cap ? 0 : (blk + 1 < nblk ? blk + 1 : 0);   // (Bland's rule scans from the first block)
    }
    // ---- objective: flow x cost over the tree arcs
    if (!failed) {
        for (int s = 0; s < slots; ++s) {
            const int v = s * 64 + lane;
            const int p = v < N ? parL[v] : -1;
            if (p >= 0) {
                tot += (double)pflL[v] * (v < n ? cost(v, p) : cost(p, v));
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off);
    return tot;
}

template <typename T, bool LISTS> __global__ __launch_bounds__(512) void k_emd_wide(EmdWideArgs a)
{
    constexpr bool INTEGRAL = sizeof(T) == 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nb = a.nb;
    // per wave, by node: bin, parent (-1: the root), visit stamp, closing order of the start rule; flow to the parent; potential
    unsigned char *wv = smem + (size_t)wave * EMDW_WAVE_BYTES;
    int *binL = reinterpret_cast<int *>(wv);
    int *parL = binL + EMDW_MAXN;
    int *markL = parL + EMDW_MAXN;
    int *ordL = markL + EMDW_MAXN;
    T *pflL = reinterpret_cast<T *>(wv + 4 * EMDW_MAXN * sizeof(int));           // (start rule: what an open line still has to place)
    double *potL = reinterpret_cast<double *>(wv + 4 * EMDW_MAXN * sizeof(int) + EMDW_MAXN * sizeof(double));
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.k.work_next = 0;
    const double eps = a.eps;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int picked = emd_pick(a.pick, lane, wave);

    const int64_t wave_global = (int64_t)blockIdx.x * a.waves + wave;
    const int64_t wave_total = (int64_t)gridDim.x * a.waves;
    for (int64_t t = wave_global;;) {
        if (t >= a.p.n) break;
        const PairSlot ps = emd_pair(a.p, t, picked);
        const int pi = ps.i, pj = ps.j;
        // ---- the entries: four per lane, each with its bin and what it supplies / demands once the common mass is cancelled.
        // Dense rows: entry e is bin e.  Lists: entries 0..127 are x's, 128..255 y's.
        double sa = 0, sb = 0;
        int ebin[4];
        T smass[4], kmass[4];
        if constexpr (LISTS) {
            const int st = a.stride;
            const int cx = min(a.hs_cnt[pi], 128), cy = min(a.hs_cnt[pj], 128);
            const int32_t *bx = a.hs_bin + (size_t)pi * st, *by = a.hs_bin + (size_t)pj * st;
            const double *vx = a.hs_val + (size_t)pi * st, *vy = a.hs_val + (size_t)pj * st;
            for (int k = 0; k < cx; ++k) sa += vx[k];          // (in bin order: the dense sums)
            for (int k = 0; k < cy; ++k) sb += vy[k];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int side = s >> 1, e = (s & 1) * 64 + lane;
                const int cnt = side ? cy : cx, ocnt = side ? cx : cy;
                const int32_t *mb = side ? by : bx, *ob = side ? bx : by;
                const double *mv = side ? vy : vx, *ov = side ? vx : vy;
                ebin[s] = 0; smass[s] = (T)0; kmass[s] = (T)0;
                if (e < cnt) {
                    const int b = mb[e];
                    const double ev = mv[e];
                    T mine, other = (T)0;
                    if (INTEGRAL) mine = (T)(ev * (side ? sa : sb));
                    else mine = (T)(ev / (side ? sb : sa));
                    // the other histogram's mass on the same bin: its list is in bin order
                    int lo = 0, hi = ocnt;
                    for (int g = 0; g < 8 && lo < hi; ++g) {
                        const int mid = (lo + hi) >> 1;
                        if (ob[mid] < b) lo = mid + 1; else hi = mid;
                    }
                    if (lo < ocnt && ob[lo] == b) {
                        const double w = ov[lo];
                        if (INTEGRAL) other = (T)(w * (side ? sb : sa));
                        else other = (T)(w / (side ? sa : sb));
                    }
                    const T d = mine - other;
                    const T pos = d > (T)0 ? d : (T)0;
                    ebin[s] = b;
                    if (side == 0) smass[s] = pos; else kmass[s] = pos;
                }
            }
        } else {
            const double *hx = a.hist + (size_t)pi * nb, *hy = a.hist + (size_t)pj * nb;
            for (int k = 0; k < nb; ++k) { sa += hx[k]; sb += hy[k]; }   // (in index order, as k_emd_ns)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int b = s * 64 + lane;
                const double xk = b < nb ? hx[b] : 0.0, yk = b < nb ? hy[b] : 0.0;
                T xm, ym;
                if (INTEGRAL) { xm = (T)(xk * sb); ym = (T)(yk * sa); }
                else { xm = (T)(xk / sa); ym = (T)(yk / sb); }
                const T d = xm - ym;
                ebin[s] = b;
                smass[s] = d > (T)0 ? d : (T)0;
                kmass[s] = d < (T)0 ? -d : (T)0;
            }
        }
        int n = 0, m = 0;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            n += __popcll(__ballot(smass[s] != (T)0));
            m += __popcll(__ballot(kmass[s] != (T)0));
        }
        const int N = n + m;
        double tot = 0.0;
        bool failed = N > EMDW_MAXN;   // (the binding admits no such data set)
        if (n > 0 && m > 0 && !failed) {
            // ---- nodes: k < n = source k, n + j = sink j, both in entry order
            {
                int sbase = 0, kbase = n;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const unsigned long long ms = __ballot(smass[s] != (T)0), mk = __ballot(kmass[s] != (T)0);
                    if (smass[s] != (T)0) { const int v = sbase + __popcll(ms & below); binL[v] = ebin[s]; pflL[v] = smass[s]; }
                    if (kmass[s] != (T)0) { const int v = kbase + __popcll(mk & below); binL[v] = ebin[s]; pflL[v] = kmass[s]; }
                    sbase += __popcll(ms); kbase += __popcll(mk);
                }
            }
            const EmdwHistCost cost{a.cost, binL, nb};
            tot = emdw_solve<T>(cost, n, m, parL, markL, ordL, pflL, potL, eps, a.dantzig_cap, failed);
            if (INTEGRAL) tot /= sa * sb;
        }
        t = emd_finish<true>(a.p, a.k, t, ps.opos, tot, failed, wave_total, lane);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_emd_points: the earth mover's distance between two point clouds of the ragged pool (ctx.hip set_pool: 1 .. 128 points of DIM
// coordinates each, DIM in 1 .. 4), uniform masses, ground cost the distance between points -- k_emd_wide's simplex (emdw_solve)
// on EmdwPointCost.  One wavefront per solve; what differs from the histogram form is how a solve is set up:
//   * a pure function of the pair.  Nothing of the bound data set enters: the pricing tolerance is 2^-43 x the diagonal of the
//     two clouds' common bounding box (an upper bound of every ground cost of the pair), computed per solve;
//   * a canonical orientation, so that emd(x, y) and emd(y, x) run the same solve: the cloud with fewer points is the source
//     side; at equal sizes the one whose first differing stored coordinate is smaller (identical sequences need no rule);
//   * packed nodes: the source cloud's points are nodes 0 .. n - 1, the sink cloud's n .. n + m - 1 (20 + 30 points: one slot);
//     their coordinates, widened to float64, sit in LDS per wave, [n + m][DIM] -- the layout is sized by DIM at launch;
//   * integer masses: every source supplies m / g and every sink demands n / g, g = gcd(n, m); the total n m / g <= 16 384, so the
//     flows are int32 and exact, and the only rounding outside the costs is in sum(flow x cost) / total.
// Two clouds that are equal as multisets of points give exactly 0.0: the row-minimum start puts every unit on a zero-cost arc
// (each source finds an open copy of itself: the sources before it took copies of their own points only), the pivots that may
// follow are degenerate, and the objective is a sum of products with a zero factor.
#define EMDP_MAXPTS 128
#define EMDP_TREE_BYTES (3 * EMDW_MAXN * (int)sizeof(int) + 2 * EMDW_MAXN * (int)sizeof(double))
#define EMDP_WAVE_BYTES(dim) (EMDP_TREE_BYTES + EMDW_MAXN * (dim) * (int)sizeof(double))

template <typename V> struct EmdPointsArgs {
    const V *val;
    const int32_t *off, *len;   // counted in points
    int waves;
    PairArgs p;
    EmdCounters k;
    int dantzig_cap;            // -1: 16 N + 64
};

template <typename V, int DIM> __global__ __launch_bounds__(256) void k_emd_points(EmdPointsArgs<V> a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    // per wave, by node: parent (-1: the root), visit stamp, closing order of the start rule; flow to the parent; potential; point
    unsigned char *wv = smem + (size_t)wave * EMDP_WAVE_BYTES(DIM);
    int *parL = reinterpret_cast<int *>(wv);
    int *markL = parL + EMDW_MAXN;
    int *ordL = markL + EMDW_MAXN;
    int *pflL = reinterpret_cast<int *>(wv + 3 * EMDW_MAXN * sizeof(int));   // (int32 flows in slots of 8 bytes)
    double *potL = reinterpret_cast<double *>(wv + 3 * EMDW_MAXN * sizeof(int) + EMDW_MAXN * sizeof(double));
    double *xyL = reinterpret_cast<double *>(wv + EMDP_TREE_BYTES);
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.k.work_next = 0;
    const int64_t wave_global = (int64_t)blockIdx.x * a.waves + wave;
    const int64_t wave_total = (int64_t)gridDim.x * a.waves;
    for (int64_t t = wave_global;;) {
        if (t >= a.p.n) break;
        const PairSlot ps = emd_pair(a.p, t, -1);
        int pi = ps.i, pj = ps.j;
        // ---- orientation
        {
            const int li = a.len[pi], lj = a.len[pj];
            bool swap = lj < li;
            if (li == lj && pi != pj) {
                const V *x = a.val + (int64_t)a.off[pi] * DIM, *y = a.val + (int64_t)a.off[pj] * DIM;
                const int cnt = li * DIM;
                for (int base = 0; base < cnt; base += 64) {
                    const int e = base + lane;
                    const V xv = e < cnt ? x[e] : (V)0, yv = e < cnt ? y[e] : (V)0;
                    const unsigned long long diff = __ballot(xv != yv);
                    if (diff) {
                        swap = (__ballot(yv < xv) >> (__ffsll(diff) - 1)) & 1ull;
                        break;
                    }
                }
            }
            if (swap) { const int k = pi; pi = pj; pj = k; }
        }
        const int n = __builtin_amdgcn_readfirstlane(a.len[pi]), m = __builtin_amdgcn_readfirstlane(a.len[pj]);
        const int N = n + m;
        double tot = 0.0;
        bool failed = n < 1 || m < 1 || n > EMDP_MAXPTS || m > EMDP_MAXPTS;   // (the binding admits no such data set)
        if (!failed) {
            // ---- nodes: the points, and what each supplies / demands
            const V *sx = a.val + (int64_t)a.off[pi] * DIM, *sy = a.val + (int64_t)a.off[pj] * DIM;
            for (int e = lane; e < n * DIM; e += 64) xyL[e] = (double)sx[e];
            for (int e = lane; e < m * DIM; e += 64) xyL[n * DIM + e] = (double)sy[e];
            int g = n;
            for (int r = m, it = 0; r != 0 && it < 16; ++it) { const int q = g % r; g = r; r = q; }   // (gcd: <= 11 steps below 128)
            const int supply = m / g, demand = n / g;
            const int slots = (N + 63) >> 6;
            for (int s = 0; s < slots; ++s) {
                const int v = s * 64 + lane;
                if (v < N) pflL[v] = v < n ? supply : demand;
            }
            EMDW_SYNC();
            // ---- the pricing tolerance, from the pair alone: the diagonal of the common bounding box
            double lo[DIM], hi[DIM];
#pragma unroll
            for (int k = 0; k < DIM; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; }
            for (int s = 0; s < slots; ++s) {
                const int v = s * 64 + lane;
                if (v < N) {
#pragma unroll
                    for (int k = 0; k < DIM; ++k) { const double z = xyL[v * DIM + k]; lo[k] = fmin(lo[k], z); hi[k] = fmax(hi[k], z); }
                }
            }
            double diag;
            {
                double s2 = 0.0;
#pragma unroll
                for (int k = 0; k < DIM; ++k) {
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) { lo[k] = fmin(lo[k], __shfl_xor(lo[k], off)); hi[k] = fmax(hi[k], __shfl_xor(hi[k], off)); }
                    const double w = hi[k] - lo[k];
                    s2 = k == 0 ? w * w : s2 + w * w;
                }
                diag = DIM == 1 ? hi[0] - lo[0] : __dsqrt_rn(s2);
            }
            const double eps = diag * 1.1368683772161603e-13;   // 2^-43
            const EmdwPointCost<DIM> cost{xyL};
            tot = emdw_solve<int>(cost, n, m, parL, markL, ordL, pflL, potL, eps, a.dantzig_cap, failed);
            tot /= (double)(supply * n);
        }
        t = emd_finish<true>(a.p, a.k, t, ps.opos, tot, failed, wave_total, lane);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side: what the launchers share, then the launchers.

// The fused pick of a one-to-all launch (k_emd_ns, k_emd_wide): reported through *src.pick_fused whenever the caller asks whether
// this metric fuses, filled in when the launch is to pick its anchor from a row.
static void emd_pick_fill(PickArgs &k, const annchor_ctx *c, const PairSource &src)
{
    k = PickArgs{nullptr, nullptr, nullptr, 0, 0};
    if (src.anchor && src.pick_fused && c->nx <= 65536) {
        *src.pick_fused = true;
        if (src.pick_row) k = PickArgs{src.pick_row, src.pick_runmin, src.pick_out, src.pick_reset, (int)c->nx};
    }
}

// Waves per workgroup, from the kernel's own figure.  A small launch (an anchor round: one solve per point) is as slow as its
// slowest solve: it is spread over every SIMD of the chip instead of filling a few CUs.  ANNCHOR_EMD_WAVES lowers the figure
// further (tuning / occupancy experiments).
static int emd_waves(const annchor_ctx *c, int64_t n, int waves)
{
    const int64_t spread = (n + 2 * (int64_t)c->prop.multiProcessorCount - 1) / (2 * (int64_t)c->prop.multiProcessorCount);
    if (spread < waves) waves = (int)std::max<int64_t>(spread, 1);
    if (const char *w = getenv("ANNCHOR_EMD_WAVES")) { const int ww = atoi(w); if (ww >= 1 && ww < waves) waves = ww; }
    return waves;
}

// pivots under Dantzig's rule before Bland's takes over: -1 (the kernels' 16 N + 64) unless ANNCHOR_EMD_DANTZIG_CAP says otherwise
static int emd_dantzig_cap()
{
    const char *dc = getenv("ANNCHOR_EMD_DANTZIG_CAP");
    return dc ? atoi(dc) : -1;
}

// The launch's turn at the counters.  Taken as the last thing before the launch, when nothing can refuse it any more: it is the
// kernel that zeroes work_next, and a turn taken without a kernel would hand the next launch a counter that is not zero.
static int emd_counters(annchor_ctx *c, EmdCounters &k)
{
    if (!c->supp.p) {
        ANN_TRY(ann_reserve(c, c->supp, 64));
        ANN_CHECK_HIP(c, hipMemsetAsync(c->supp.p, 0, 64, c->stream));
        c->emd_epoch = 0;
    }
    k.fail = c->supp.as<int32_t>();
    k.work = k.fail + 4 + (c->emd_epoch & 1);
    k.work_next = k.fail + 4 + ((c->emd_epoch + 1) & 1);
    ++c->emd_epoch;
    return ANNCHOR_OK;
}

// Launch of a simplex kernel (k_emd_ns, k_emd_wide, k_emd_points) at a.waves waves per workgroup and `lds` bytes of dynamic LDS.
// Resident workgroups only: the waves claim their solves from a counter.
template <typename Args>
static int emd_simplex_launch(annchor_ctx *c, void (*kern)(Args), Args &a, size_t lds, const char *prof_name, double prof_bytes)
{
    const void *fn = (const void *)kern;
    const int waves = a.waves;
    ANN_CHECK_HIP(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int64_t blocks = (a.p.n + waves - 1) / waves;
    int per_cu = 1;
    ANN_CHECK_HIP(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, waves * 64, lds));
    const int64_t resident = (int64_t)c->prop.multiProcessorCount * std::max(per_cu, 1);
    if (blocks > resident) blocks = resident;
    ANN_TRY(emd_counters(c, a.k));
    ProfScope ps(c, prof_name, prof_bytes);
    kern<<<(int)blocks, waves * 64, lds, c->stream>>>(a);
    ANN_CHECK_HIP(c, hipGetLastError());
    return ANNCHOR_OK;
}

#ifdef EMD_PROFILE
// The cycle counts the EP macros collect, for launches of up to 4096 solves.  emd_prof_buf: the zeroed buffer for such a launch
// (nullptr for a larger one).  emd_prof_print, on every 20th launch that had one: the slowest solve and the means, by phase.
static long long *emd_prof_buf(annchor_ctx *c, int64_t n)
{
    static long long *dbg = nullptr;
    if (!dbg) (void)hipMalloc(&dbg, sizeof(long long) * 4096 * 16);
    if (n > 4096) return nullptr;
    (void)hipMemsetAsync(dbg, 0, sizeof(long long) * 4096 * 16, c->stream);
    return dbg;
}

static void emd_prof_print(annchor_ctx *c, const long long *dbg, int64_t n, int waves, const char *kernel,
                           std::initializer_list<const char *> phases, std::initializer_list<const char *> counts)
{
    static int calls = 0;
    if (!dbg || ++calls % 20 != 7) return;
    std::vector<long long> h((size_t)4096 * 16);
    (void)hipStreamSynchronize(c->stream);
    (void)hipMemcpy(h.data(), dbg, h.size() * sizeof(long long), hipMemcpyDeviceToHost);
    int64_t worst = 0; long long wt = 0; double tot[8] = {0};
    for (int64_t t = 0; t < n; ++t) { long long sum = 0; for (int q = 0; q < 8; ++q) { sum += h[t * 16 + q]; tot[q] += h[t * 16 + q]; } if (sum > wt) { wt = sum; worst = t; } }
    fprintf(stderr, "%s launch of %lld solves, %d waves per block: slowest solve %lld: %lld cycles, n %lld m %lld,", kernel,
            (long long)n, waves, (long long)worst, wt, h[worst * 16 + 12], h[worst * 16 + 13]);
    int q = 8;
    for (const char *name : counts) fprintf(stderr, " %s %lld", name, h[worst * 16 + q++]);
    fprintf(stderr, "\n");
    q = 0;
    for (const char *name : phases) { fprintf(stderr, "   %-14s slowest %8lld   mean %8.0f\n", name, h[worst * 16 + q], tot[q] / (double)n); ++q; }
}
#endif

int ann_emd_wide_launch(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    if (src.n == 0) return ANNCHOR_OK;
    ANN_REQUIRE(c, c->cost_is_metric, ANNCHOR_ESTATE, "the wide exact-OT kernel needs a metric ground cost");
    EmdWideArgs a;
    a.hist = c->hist.as<double>();
    a.cost = c->cost.as<double>();
    a.nb = c->nbins;
    a.stride = c->hs_stride;
    pair_fill(a.p, src, d_out, d_RA, d_ncm);
    emd_pick_fill(a.pick, c, src);
    a.eps = c->cost_max * 1.1368683772161603e-13;   // 2^-43
    a.dantzig_cap = emd_dantzig_cap();
    // 8 KB of LDS per wave and a latency-bound solve: eight waves per workgroup, two or more workgroups per CU
    a.waves = emd_waves(c, src.n, 8);
    a.hs_bin = c->hs_bin.as<int32_t>(); a.hs_val = c->hs_val.as<double>(); a.hs_cnt = c->hs_cnt.as<int32_t>();
    const bool integral = c->hist_integral, lists = a.stride > 0;
    void (*kern)(EmdWideArgs) = lists ? (integral ? k_emd_wide<int, true> : k_emd_wide<double, true>)
                                      : (integral ? k_emd_wide<int, false> : k_emd_wide<double, false>);
    return emd_simplex_launch(c, kern, a, (size_t)a.waves * EMDW_WAVE_BYTES, "wasserstein_pairs",
                              (double)src.n * (2.0 * std::min(a.nb, 256) * 8 + 8));
}

template <typename V> static int emd_points_launch(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    ANN_REQUIRE(c, c->maxlen >= 1 && c->maxlen <= EMDP_MAXPTS, ANNCHOR_ELIMIT, "cloud size %d outside 1..%d", c->maxlen, EMDP_MAXPTS);
    EmdPointsArgs<V> a;
    a.val = c->sym.as<V>();
    a.off = c->soff.as<int32_t>(); a.len = c->slen.as<int32_t>();
    pair_fill(a.p, src, d_out, d_RA, d_ncm);
    a.dantzig_cap = emd_dantzig_cap();
    // 7 KB + DIM x 2 KB of LDS per wave and a latency-bound solve: four waves per workgroup, so that two to four workgroups share
    // a CU at every DIM
    a.waves = emd_waves(c, src.n, 4);
    void (*kern)(EmdPointsArgs<V>);
    switch (c->curve_dim) {
    case 1: kern = k_emd_points<V, 1>; break;
    case 2: kern = k_emd_points<V, 2>; break;
    case 3: kern = k_emd_points<V, 3>; break;
    case 4: kern = k_emd_points<V, 4>; break;
    default: ann_set_err(c, "cloud dim %d outside 1..4", c->curve_dim); return ANNCHOR_EINVAL;
    }
    return emd_simplex_launch(c, kern, a, (size_t)a.waves * EMDP_WAVE_BYTES(c->curve_dim), "emd_points_pairs",
                              (double)src.n * (2.0 * c->maxlen * c->curve_dim * sizeof(V) + 16));
}

int ann_emd_points_launch(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    if (src.n == 0) return ANNCHOR_OK;
    return c->metric == ANNCHOR_METRIC_EMD_POINTS_F32 ? emd_points_launch<float>(c, src, d_out, d_RA, d_ncm)
                                                      : emd_points_launch<double>(c, src, d_out, d_RA, d_ncm);
}

int ann_emd_launch(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    if (src.n == 0) return ANNCHOR_OK;
    EmdArgs a = {};
    a.hist = c->hist.as<double>();
    a.cost = c->cost.as<double>();
    a.nb = c->nbins;
    pair_fill(a.p, src, d_out, d_RA, d_ncm);
    a.reduce = c->cost_is_metric && !getenv("ANNCHOR_EMD_NO_REDUCE");
    const size_t cost_bytes = sizeof(double) * (size_t)a.nb * a.nb;
    const bool integral = c->hist_integral;
    // metric ground cost: the transportation simplex with one lane per node (ANNCHOR_EMD_SOLVER=ssp keeps the shortest-path solver)
    const char *e = getenv("ANNCHOR_EMD_SOLVER");
    if (a.reduce && !(e && !strcmp(e, "ssp"))) {
        a.eps = c->cost_max * 1.1368683772161603e-13;   // 2^-43
        emd_pick_fill(a.pick, c, src);
        a.dantzig_cap = emd_dantzig_cap();
        a.waves = emd_waves(c, src.n, 16);
        const bool sparse = a.nb > EMD_MAXB;
        a.hs_bin = c->hs_bin.as<int32_t>(); a.hs_val = c->hs_val.as<double>(); a.hs_cnt = c->hs_cnt.as<int32_t>();
        void (*kern)(EmdArgs) = sparse ? (integral ? k_emd_ns<int, true> : k_emd_ns<double, true>)
                                       : (integral ? k_emd_ns<int, false> : k_emd_ns<double, false>);
#ifdef EMD_PROFILE
        a.dbg = emd_prof_buf(c, src.n);
#endif
        ANN_TRY(emd_simplex_launch(c, kern, a, (sparse ? 0 : cost_bytes) + (size_t)a.waves * EMD_NS_WAVE_BYTES, "wasserstein_pairs",
                                   (double)src.n * (2.0 * std::min(a.nb, 64) * 8 + 8)));
#ifdef EMD_PROFILE
        emd_prof_print(c, a.dbg, src.n, a.waves, "k_emd_ns",
                       {"setup", "start basis", "potentials", "pricing", "cycle+theta", "tree update", "objective"}, {"pivots", "path steps"});
#endif
        return ANNCHOR_OK;
    }
    ANN_REQUIRE(c, a.nb <= EMD_MAXB, ANNCHOR_ELIMIT, "histograms of %d bins need a metric ground cost (the shortest-path solver takes up to %d bins)", a.nb, EMD_MAXB);
    const bool narrow = integral && c->hist_fits_i16 && !getenv("ANNCHOR_EMD_WIDE_FLOWS");
    // Flow slab: n sources x (m | 1) sinks.  The supports of the raw histograms bound n and m by max_support; with the common
    // mass cancelled the two supports are disjoint (n + m <= bins), which halves the worst case again.
    size_t entries = 0;
    if (a.reduce) {
        a.S = 0;   // stride per solve
        for (int n = 1; n <= c->max_support; ++n) {
            const int m = std::min(c->max_support, a.nb - n);
            if (m >= 1) entries = std::max(entries, (size_t)n * (size_t)(m | 1));
        }
        if (!entries) entries = 1;
    } else {
        a.S = c->max_support | 1;  // odd stride: conflict-free column reads
        entries = (size_t)c->max_support * a.S;
    }
    const size_t esz = narrow ? 2 : integral ? 4 : 8;
    const size_t slab = ((esz * entries + 2 * EMD_MAXB * sizeof(int)) + 15) & ~(size_t)15;
    a.slab_bytes = (int)slab;
    // The solver is latency bound (one DPP minimum per Dijkstra pop on the critical path): as many waves per SIMD as the LDS
    // takes.  A workgroup holds at most 16 waves, so two workgroups per CU, each with its own copy of the ground costs.
    int per_cu = 2;
    int waves = (int)(((160 * 1024) / per_cu - cost_bytes) / slab);
    if (waves < 8) { per_cu = 1; waves = (int)((160 * 1024 - cost_bytes) / slab); }
    if (waves > 16) waves = 16;
    waves = emd_waves(c, src.n, waves);
    ANN_REQUIRE(c, waves >= 1, ANNCHOR_ELIMIT, "histogram support %d needs more LDS than a CU has", c->max_support);
    a.waves = waves;
    const size_t lds = cost_bytes + slab * waves;
    void (*kern)(EmdArgs) = narrow ? k_emd<int, int16_t> : integral ? k_emd<int, int> : k_emd<double, double>;
    ANN_CHECK_HIP(c, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int64_t blocks = (src.n + waves - 1) / waves;
    if (blocks > (int64_t)per_cu * c->prop.multiProcessorCount) blocks = (int64_t)per_cu * c->prop.multiProcessorCount;  // resident blocks only (LDS bound)
    ANN_TRY(emd_counters(c, a.k));
#ifdef EMD_PROFILE
    a.dbg = emd_prof_buf(c, src.n);
#endif
    ProfScope ps(c, "wasserstein_pairs", (double)src.n * (2.0 * a.nb * 8 + 8));
    kern<<<(int)blocks, waves * 64, lds, c->stream>>>(a);
#ifdef EMD_PROFILE
    emd_prof_print(c, a.dbg, src.n, waves, "k_emd",
                   {"setup", "search init", "pop min", "column+ballot", "relax", "potentials", "augment", "objective"},
                   {"searches", "pops", "relaxed", "augmentations"});
#endif
    ANN_CHECK_HIP(c, hipGetLastError());
    return ANNCHOR_OK;
}

