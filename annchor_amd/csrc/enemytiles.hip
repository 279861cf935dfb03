// enemytiles.hip -- the nearest-enemy graph of the streamed form: for every row its nn nearest rows of a DIFFERENT label
// (Annchor.get_nearest_enemies, reference annchor/annchor.py:685-773, for data sets beyond the pair-list form).
//
// The tile kernels know nothing about labels and stay that way.  The rows are ordered so that every 128-row tile holds ONE
// label (class-pure tiles); whether a row may list a column is then a property of the TILE PAIR, and the tile kernels already
// have a way to never meet a tile pair: a rank key of +inf (the self tile of a graph build).  So the label mask is two stores
// per same-label pair into the scratch rows the ranking pass leaves (scr_key: what the selection rounds read; scr_lb: what the
// exact repair of flagged rows reads -- without it the repair would bring same-label columns back), and everything after it
// -- k_st_knnbf / knnbk / k_st_knn in query form, the guards, k_st_repair, the finalize -- runs as for annchor_stream_query.
//
//   annchor_stream_order_classes   the data set's k-d order (annchor_stream_order_begin), stably sorted by label code: the
//       rows of a class keep their relative k-d order, so a class tile is a run of k-d neighbours of that class.  Every class
//       is padded to a multiple of 128 slots; padding slots are what tail padding is in the plain order (zero rows, +inf
//       norms, perm -1), validity is a flag per slot (slot_src = ~0), and the per-tile tables (intervals, means, the fp16 split's
//       scale) count real rows only.  tlab[tile] = the tile's label code.
//   annchor_stream_enemies         rows = columns = the context's own arrays, query form, K = nn, budget
//       ceil(p_work x #tiles) per row tile, no join passes (a neighbour's enemies are mostly one's own friends).
#include "streamed.h"

#define EN_NONE 0xffffffffu

__global__ void k_en_label_keys(const int32_t *__restrict__ lab, const uint32_t *__restrict__ order, int64_t n, unsigned long long *__restrict__ keys)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) keys[p] = (unsigned long long)(uint32_t)lab[order[p]];
}

// position p of the label-sorted order -> its slot of the class-padded order: off / poff = first position / first slot of each class
__global__ void k_en_slots(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ order, int64_t n, const int64_t *__restrict__ off,
                           const int64_t *__restrict__ poff, uint32_t *__restrict__ slot_src)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int cl = (int)keys[p];
    slot_src[poff[cl] + (p - off[cl])] = order[p];
}

// k_st_gather with a validity flag per slot: 16 lanes per slot
__global__ void k_en_gather(const float *__restrict__ X, const uint32_t *__restrict__ slot_src, int64_t n_pad, int dim, int dimp, int64_t base,
                            float *__restrict__ Xs, float *__restrict__ rs, int64_t *__restrict__ perm)
{
    const int sub = threadIdx.x & 15;
    const int64_t s = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    if (s >= n_pad) return;
    const uint32_t src = slot_src[s];
    const bool real = src != EN_NONE;
    float acc = 0.f;
    for (int k = sub; k < dimp; k += 16) {
        const float v = (real && k < dim) ? X[(size_t)src * dim + k] : 0.f;
        Xs[(size_t)s * dimp + k] = v;
        acc += v * v;
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 16);
    if (sub == 0) {
        rs[s] = real ? acc : INFINITY;
        perm[s] = real ? base + (int64_t)src : -1;
    }
}

// k_st_intervals over the real rows of a tile (block = tile, thread = slot), and the tile's label.  Every tile begins with a
// real row (a class has at least one row and its padding follows its rows).
__global__ __launch_bounds__(ST_T) void k_en_intervals(const float *__restrict__ Dt, int nap, const uint32_t *__restrict__ slot_src,
                                                      const int32_t *__restrict__ lab, int na, int nt, float *__restrict__ lo,
                                                      float *__restrict__ hi, float *__restrict__ mid, int32_t *__restrict__ tlab)
{
    __shared__ float sv[ST_T][65];   // [slot][anchor]
    __shared__ int nreal;
    const int t = blockIdx.x;
    const uint32_t src = slot_src[(size_t)t * ST_T + threadIdx.x];
    const bool real = src != EN_NONE;
    if (threadIdx.x == 0) { nreal = 0; tlab[t] = real ? lab[src] : -1; }
    __syncthreads();
    if (real) {
        atomicAdd(&nreal, 1);
        const float4 *row = reinterpret_cast<const float4 *>(Dt + (size_t)src * nap);
        for (int q = 0; q < nap / 4; ++q) {
            const float4 v = row[q];
            sv[threadIdx.x][4 * q] = v.x; sv[threadIdx.x][4 * q + 1] = v.y; sv[threadIdx.x][4 * q + 2] = v.z; sv[threadIdx.x][4 * q + 3] = v.w;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < na) {
        // (the real rows are the tile's first `rows` slots; the mean is summed row by row, not in k_st_intervals' tree order: the
        // rank keys of this order differ in the last bits from those of a plain order of the same rows)
        const int a = threadIdx.x, rows = nreal;
        float mn = INFINITY, mx = -INFINITY, sum = 0.f;
        for (int r = 0; r < rows; ++r) { const float v = sv[r][a]; mn = fminf(mn, v); mx = fmaxf(mx, v); sum += v; }
        lo[(size_t)a * nt + t] = mn;
        hi[(size_t)a * nt + t] = mx;
        mid[(size_t)a * nt + t] = rows ? sum / (float)rows : INFINITY;
    }
}

// the label mask: RK rows of the scratch per workgroup row, one column tile per thread
#define EN_MASK_ROWS 32
__global__ __launch_bounds__(256) void k_en_mask_pairs(const int32_t *__restrict__ tlab, int tile_begin, int tile_count, int nt_all,
                                                       float *__restrict__ scr_key, float *__restrict__ scr_lb)
{
    const int J = blockIdx.x * 256 + threadIdx.x;
    if (J >= nt_all) return;
    const int lj = tlab[J];
    const int i0 = blockIdx.y * EN_MASK_ROWS, i1 = min(i0 + EN_MASK_ROWS, tile_count);
    for (int i = i0; i < i1; ++i)
        if (tlab[tile_begin + i] == lj) {
            scr_key[(size_t)i * nt_all + J] = INFINITY;   // never a candidate of the selection rounds
            scr_lb[(size_t)i * nt_all + J] = INFINITY;    // never below a row's K-th distance (k_st_repair)
        }
}

int ann_stream_mask_same_label(annchor_ctx *c, const KnnArgs &a, const int32_t *tlab)
{
    const dim3 grid((unsigned)ann_blocks(a.nt_all, 256), (unsigned)ann_blocks(a.tile_count, EN_MASK_ROWS));
    k_en_mask_pairs<<<grid, 256, 0, c->stream>>>(tlab, a.tile_begin, a.tile_count, a.nt_all, a.scr_key, a.scr_lb);
    ANN_CHECK_HIP(c, hipGetLastError());
    return ANNCHOR_OK;
}

// rows back in the bound rows' own order: row perm[r] - base gets its K ordered enemies (no self column); padding slots are dropped
__global__ void k_en_emit(const int64_t *__restrict__ perm, int64_t rows, int K, int64_t base, int64_t n_local, const int64_t *__restrict__ idx,
                          const float *__restrict__ dist, int64_t *__restrict__ oidx, double *__restrict__ odist)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows * K) return;
    const int64_t r = t / K;
    const int e = (int)(t - r * K);
    const int64_t g = perm[r];
    if (g < 0) return;
    const int64_t loc = g - base;
    if (loc < 0 || loc >= n_local) return;
    oidx[loc * K + e] = idx[t];
    odist[loc * K + e] = (double)dist[t];
}

extern "C" int annchor_stream_order_classes(annchor_ctx *c, const int32_t *labels, int32_t n_classes, const float *anchor_vecs,
                                            int64_t *n_pad, int32_t *n_tiles, int32_t *dim_padded)
{
    if (!c || !labels || !n_pad || !n_tiles || !dim_padded) return ANNCHOR_EINVAL;
    StreamState *s = ann_stream_state(c, false);
    ANN_REQUIRE(c, s && s->na > 0, ANNCHOR_ESTATE, "anchor rounds not run");
    const int64_t n = s->n_local;
    ANN_REQUIRE(c, n_classes >= 1 && (int64_t)n_classes <= n, ANNCHOR_EINVAL, "n_classes=%d for %lld rows", n_classes, (long long)n);
    // class extents: rows [off[c], off[c + 1]) of the label-sorted order -> slots [poff[c], poff[c] + count), padded to whole tiles
    std::vector<int64_t> tab(2 * ((size_t)n_classes + 1), 0);
    int64_t *off = tab.data(), *poff = tab.data() + n_classes + 1;
    for (int64_t i = 0; i < n; ++i) {
        ANN_REQUIRE(c, labels[i] >= 0 && labels[i] < n_classes, ANNCHOR_EINVAL, "label code %d of row %lld outside [0, %d)", labels[i], (long long)i, n_classes);
        ++off[labels[i] + 1];
    }
    for (int cl = 0; cl < n_classes; ++cl) {
        ANN_REQUIRE(c, off[cl + 1] > 0, ANNCHOR_EINVAL, "label code %d has no rows", cl);
        poff[cl + 1] = poff[cl] + (off[cl + 1] + ST_T - 1) / ST_T * ST_T;
        off[cl + 1] += off[cl];
    }
    const int64_t n_pad_c = poff[n_classes];
    ANN_REQUIRE(c, n_pad_c < (1ll << 31), ANNCHOR_ELIMIT, "class-padded order: %lld slots", (long long)n_pad_c);
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    // the data set's k-d order (all of it: this context orders everything itself), then the stable sort by label
    void *ol = nullptr, *oa = nullptr;
    int64_t ob = 0;
    ANN_TRY(annchor_stream_order_begin(c, 0, 0, 0, &ol, &oa, &ob));
    ProfScope ps(c, "stream_order_classes", (double)n_pad_c * (s->dimp * 8.0 + s->na * 4.0 + 40.0));
    uint32_t *cur = s->order_cur, *other = cur == s->vals.as<uint32_t>() ? s->vals2.as<uint32_t>() : s->vals.as<uint32_t>();
    s->order_cur = nullptr;
    ANN_TRY(ann_stream_reserve(c, s->cls_lab, sizeof(int32_t) * (size_t)n));
    ANN_TRY(ann_stream_reserve(c, s->cls_off, sizeof(int64_t) * tab.size()));
    ANN_TRY(ann_h2d(c, s->cls_lab.p, labels, sizeof(int32_t) * (size_t)n));
    ANN_TRY(ann_h2d(c, s->cls_off.p, tab.data(), sizeof(int64_t) * tab.size()));
    unsigned long long *keys = s->keys.as<unsigned long long>(), *keys2 = s->keys2.as<unsigned long long>();
    k_en_label_keys<<<ann_blocks(n, 256), 256, 0, c->stream>>>(s->cls_lab.as<int32_t>(), cur, n, keys);
    int bits = 8;
    while (bits < 32 && (1ll << bits) < (int64_t)n_classes) bits += 8;
    int where = 0;
    ANN_TRY(ann_stream_sort_pairs(c, s->cubtmp.as<uint32_t>(), keys, keys2, cur, other, n, bits, &where));
    s->nt = (int)(n_pad_c / ST_T);
    s->n_pad = n_pad_c;
    ANN_TRY(ann_stream_reserve(c, s->order_all, sizeof(uint32_t) * (size_t)n_pad_c));   // slot_src: the bound row of every slot, ~0 = padding
    uint32_t *slot_src = s->order_all.as<uint32_t>();
    ANN_CHECK_HIP(c, hipMemsetAsync(slot_src, 0xff, sizeof(uint32_t) * (size_t)n_pad_c, c->stream));
    k_en_slots<<<ann_blocks(n, 256), 256, 0, c->stream>>>(where ? keys2 : keys, where ? other : cur, n, s->cls_off.as<int64_t>(),
                                                         s->cls_off.as<int64_t>() + n_classes + 1, slot_src);
    ANN_TRY(ann_stream_reserve(c, s->Xs, sizeof(float) * (size_t)n_pad_c * s->dimp));
    ANN_TRY(ann_stream_reserve(c, s->rs, sizeof(float) * (size_t)n_pad_c));
    ANN_TRY(ann_stream_reserve(c, s->perm, sizeof(int64_t) * (size_t)n_pad_c));
    ANN_TRY(ann_stream_reserve(c, s->lo, sizeof(float) * (size_t)s->na * s->nt));
    ANN_TRY(ann_stream_reserve(c, s->hi, sizeof(float) * (size_t)s->na * s->nt));
    ANN_TRY(ann_stream_reserve(c, s->mid, sizeof(float) * (size_t)s->na * s->nt));
    ANN_TRY(ann_stream_reserve(c, s->tlab, sizeof(int32_t) * (size_t)s->nt));
    k_en_gather<<<ann_blocks(n_pad_c * 16, 256), 256, 0, c->stream>>>(s->X.as<float>(), slot_src, n_pad_c, s->dim, s->dimp, s->base, s->Xs.as<float>(),
                                                                     s->rs.as<float>(), s->perm.as<int64_t>());
    k_en_intervals<<<s->nt, ST_T, 0, c->stream>>>(s->Dt.as<float>(), (s->na + 3) & ~3, slot_src, s->cls_lab.as<int32_t>(), s->na, s->nt,
                                                 s->lo.as<float>(), s->hi.as<float>(), s->mid.as<float>(), s->tlab.as<int32_t>());
    ANN_CHECK_HIP(c, hipGetLastError());
    if (anchor_vecs) {   // the centre of the fp16 split copy: the mean of the anchors' coordinates, as in a fit
        ANN_TRY(ann_stream_reserve(c, s->avecs, sizeof(float) * (size_t)s->na * s->dim));
        ANN_TRY(ann_h2d(c, s->avecs.p, anchor_vecs, sizeof(float) * (size_t)s->na * s->dim));
    }
    ANN_TRY(ann_stream_split_rows(c, s));
    ANN_CHECK_HIP(c, ann_stream_wait(c, __func__));
    s->class_pure = true;
    *n_pad = s->n_pad; *n_tiles = s->nt; *dim_padded = s->dimp;
    return ANNCHOR_OK;
}

extern "C" int annchor_stream_enemies(annchor_ctx *c, int32_t nn, double p_work, int64_t *out_idx, double *out_dist, int64_t *tile_evals)
{
    if (!c || !out_idx || !out_dist) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, nn >= 1 && nn < ST_KMAX_HUGE, ANNCHOR_ELIMIT, "streamed nearest enemies support 1 <= nn <= %d (beyond 256 dimensions: <= %d)",
                ST_KMAX_HUGE - 1, ST_KMAX_BIG - 2);
    StreamState *s = ann_stream_state(c, false);
    ANN_REQUIRE(c, s && s->class_pure && s->nt > 0 && s->Xs.p && s->tlab.p && s->n_pad == (int64_t)s->nt * ST_T,
                ANNCHOR_ESTATE, "rows are not in class-pure tiles (bind, anchor rounds, annchor_stream_order_classes)");
    ANN_REQUIRE(c, s->dimp <= 256 || nn <= ST_KMAX_BIG - 2, ANNCHOR_ELIMIT, "streamed nearest enemies: beyond 256 dimensions nn <= %d (got %d at padded dim %d)",
                ST_KMAX_BIG - 2, nn, s->dimp);
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    KnnArgs a;
    a.Xs = s->Xs.as<float>(); (void)ann_stream_split_of(s->Xs.p, &a.Xb, &a.rsb, &a.cvec); a.rs = s->rs.as<float>();
    a.lo = s->lo.as<float>(); a.hi = s->hi.as<float>(); a.mid = s->mid.as<float>();
    a.Rs = a.Xs; a.rr = a.rs; a.rlo = a.lo; a.rhi = a.hi; a.rmid = a.mid;
    a.nt_r = s->nt; a.query = 1;   // query form: no self tile, no self exclusion -- a row's own tile carries its own label
    a.nt_all = s->nt; a.na = s->na; a.tile_begin = 0; a.tile_count = s->nt; a.K = nn;
    int T = 0, tp = 0, pp = 0;
    ANN_TRY(annchor_stream_budget(s->nt, p_work, 0, &T, &tp, &pp));
    s->rank_tlab = s->tlab.as<int32_t>();
    const int rc = ann_stream_tile_phase_query(c, s, a, s->dimp, tp);
    s->rank_tlab = nullptr;
    ANN_TRY(rc);
    int64_t *d_idx = nullptr;
    float *d_dist = nullptr;
    ANN_TRY(ann_stream_knn_finish(c, s, a, s->perm.p, s->dimp, &d_idx, &d_dist, tile_evals));
    const int64_t rows = s->n_pad, n = s->n_local;
    ANN_TRY(ann_stream_reserve(c, s->emit_idx, sizeof(int64_t) * (size_t)n * nn));
    ANN_TRY(ann_stream_reserve(c, s->emit_dist, sizeof(double) * (size_t)n * nn));
    {
        ProfScope ps(c, "stream_enemies_emit", (double)n * nn * 28.0);
        k_en_emit<<<ann_blocks(rows * nn, 256), 256, 0, c->stream>>>(s->perm.as<int64_t>(), rows, nn, s->base, n, d_idx, d_dist,
                                                                    s->emit_idx.as<int64_t>(), s->emit_dist.as<double>());
        ANN_CHECK_HIP(c, hipGetLastError());
    }
    ANN_TRY(ann_d2h(c, out_idx, s->emit_idx.p, sizeof(int64_t) * (size_t)n * nn));
    return ann_d2h(c, out_dist, s->emit_dist.p, sizeof(double) * (size_t)n * nn);
}
