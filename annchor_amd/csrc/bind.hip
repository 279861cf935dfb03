// bind.hip -- binding a data set to a context: the loaders of every metric, the metric switch, annchor_metric_pairs.
#include <climits>
#include <cmath>

#include "common.h"
#include "poollayout.h"
#include <algorithm>

// ------------------------------------------------------------------- data set
static void reset_pipeline(annchor_ctx *c)
{
    c->na = c->nA = 0;
    c->n = 0; c->have_bitmap = false;
    c->have_features = c->have_RA = false; c->sel_prepared = false;
    ann_mask_changed(c);
    c->nsamp = c->ncand = c->nnext = 0;
}

// Every loader calls this where it commits, after its last check, and THEN sets the fields of its own: the scalars of the binding
// before (BoundState, common.h) route nothing of the new one.  The buffers are grow-only and stay.
static void reset_bound(annchor_ctx *c) { static_cast<BoundState &>(*c) = BoundState(); }

extern "C" int annchor_set_opaque(annchor_ctx *c, int64_t nx)
{
    if (!c) return ANNCHOR_EINVAL;
    // (one point: no pair-list stage can run on it, but the fixed-radius graph of a single point is the empty graph)
    ANN_REQUIRE(c, nx >= 1 && nx < (1ll << 31), ANNCHOR_ELIMIT, "nx=%lld out of range", (long long)nx);
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    ANN_TRY(ann_arena_init(c, nx));
    ANN_TRY(ann_prewarm_state(c));
    reset_bound(c);
    c->metric = ANNCHOR_METRIC_NONE;
    c->nx = nx;
    reset_pipeline(c);
    return ANNCHOR_OK;
}

static int set_points(annchor_ctx *c, const void *X, int64_t nx, int32_t dim, size_t esz, int metric)
{
    if (!c || !X) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, nx > 1 && nx < (1ll << 31), ANNCHOR_ELIMIT, "nx=%lld out of range", (long long)nx);
    ANN_REQUIRE(c, dim >= 1 && dim <= 65536, ANNCHOR_ELIMIT, "dim=%d out of range", dim);
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    size_t bytes = esz * (size_t)nx * (size_t)dim;
    ANN_TRY(ann_arena_init(c, nx));
    ANN_TRY(ann_prewarm_state(c));
    ANN_TRY(ann_reserve(c, c->pts, bytes));
    ANN_TRY(ann_h2d(c, c->pts.p, X, bytes));
    reset_bound(c);
    c->metric = metric;
    c->nx = nx;
    c->dim = dim;
    reset_pipeline(c);
    return ANNCHOR_OK;
}

extern "C" int annchor_set_points_f32(annchor_ctx *c, const float *X, int64_t nx, int32_t dim)
{
    return set_points(c, X, nx, dim, sizeof(float), ANNCHOR_METRIC_EUCLIDEAN_F32);
}

extern "C" int annchor_set_points_f64(annchor_ctx *c, const double *X, int64_t nx, int32_t dim)
{
    return set_points(c, X, nx, dim, sizeof(double), ANNCHOR_METRIC_EUCLIDEAN_F64);
}

extern "C" int annchor_set_points_cosine_f32(annchor_ctx *c, const float *X, int64_t nx, int32_t dim)
{
    return set_points(c, X, nx, dim, sizeof(float), ANNCHOR_METRIC_COSINE_F32);
}

extern "C" int annchor_set_points_cosine_f64(annchor_ctx *c, const double *X, int64_t nx, int32_t dim)
{
    return set_points(c, X, nx, dim, sizeof(double), ANNCHOR_METRIC_COSINE_F64);
}

// the tail every loader of the pool shares: the arena, the upload of a checked and repacked pool, the bound state
static int pool_commit(annchor_ctx *c, const void *pool, size_t bytes, const int32_t *o, const int32_t *lens, int64_t nx, int maxlen,
                       int metric)
{
    ANN_TRY(ann_arena_init(c, nx));
    ANN_TRY(ann_prewarm_state(c));
    ANN_TRY(ann_reserve(c, c->sym, bytes));
    ANN_TRY(ann_reserve(c, c->soff, sizeof(int32_t) * (size_t)nx));
    ANN_TRY(ann_reserve(c, c->slen, sizeof(int32_t) * (size_t)nx));
    ANN_TRY(ann_h2d(c, c->sym.p, pool, bytes));
    ANN_TRY(ann_h2d(c, c->soff.p, o, sizeof(int32_t) * (size_t)nx));
    ANN_TRY(ann_h2d(c, c->slen.p, lens, sizeof(int32_t) * (size_t)nx));
    reset_bound(c);
    c->metric = metric;
    c->nx = nx;
    c->maxlen = maxlen;
    reset_pipeline(c);
    return ANNCHOR_OK;
}

// The two layouts of a pool of symbols that the bit-parallel kernels read with wide loads (lev.hip, indel.hip): members start at
// multiples of `align` symbols, and the gaps between them and `slack` symbols behind the last one hold `pad`.
struct SymLayout {
    size_t align, slack;
    uint16_t pad;
};
static constexpr SymLayout SYM_BYTES = {16, 16, 0};        // uint8 codes, alphabets up to 256: 16-byte aligned starts
static constexpr SymLayout SYM_WIDE = {8, 64, 0xffffu};    // uint16 codes: 16-byte aligned starts, 0xffff is the kernels' "no symbol"

// Strings for the Levenshtein distance (lev.hip) in one of the two layouts: dense codes 0 .. alphabet - 1 of T
template <typename T> static int set_lev_strings(annchor_ctx *c, const T *symbols, const int64_t *offs, const int32_t *lens, int64_t nx,
                                                 int32_t alphabet, const SymLayout &lay, size_t cap, int limit)
{
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    const PoolLayout L = pool_layout(lens, nx, 0, INT_MAX, lay.align, cap);
    ANN_REQUIRE(c, L.refusal != PoolRefusal::TooShort, ANNCHOR_EINVAL, "negative length at %lld", (long long)L.at);
    ANN_REQUIRE(c, L.refusal != PoolRefusal::TooLarge, ANNCHOR_ELIMIT, "string pool exceeds 2 GiB");
    ANN_REQUIRE(c, L.maxlen <= limit, ANNCHOR_ELIMIT, "string length %d exceeds the supported %d%s", L.maxlen, limit,
                sizeof(T) == 2 ? " (16-bit symbols)" : "");
    std::vector<T> pool(L.total + lay.slack, (T)lay.pad);
    for (int64_t s = 0; s < nx; ++s) {
        ANN_REQUIRE(c, offs[s] >= 0, ANNCHOR_EINVAL, "negative offset at %lld", (long long)s);
        for (int32_t k = 0; k < lens[s]; ++k)
            ANN_REQUIRE(c, symbols[offs[s] + k] < alphabet, ANNCHOR_EINVAL, "symbol code out of range in string %lld", (long long)s);
        memcpy(pool.data() + L.offs[(size_t)s], symbols + offs[s], sizeof(T) * (size_t)lens[s]);
    }
    ANN_TRY(pool_commit(c, pool.data(), pool.size() * sizeof(T), L.offs.data(), lens, nx, L.maxlen, ANNCHOR_METRIC_LEVENSHTEIN));
    c->alphabet = alphabet;
    c->sym_wide = sizeof(T) == 2;
    return ANNCHOR_OK;
}

// Strings over more than 256 distinct symbols: 16-bit dense codes 0 .. alphabet - 1, alphabet <= 65 535 (code 0xffff is the
// kernel's "no symbol").  Evaluated by k_lev_w (lev.hip): match words computed per column instead of looked up.
extern "C" int annchor_set_strings_u16(annchor_ctx *c, const uint16_t *symbols, const int64_t *offs, const int32_t *lens, int64_t nx,
                                       int32_t alphabet)
{
    if (!c || !symbols || !offs || !lens) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, nx > 1 && nx < (1ll << 31), ANNCHOR_ELIMIT, "nx=%lld out of range", (long long)nx);
    ANN_REQUIRE(c, alphabet >= 1 && alphabet <= 65535, ANNCHOR_ELIMIT, "alphabet=%d not in 1..65535", alphabet);
    return set_lev_strings(c, symbols, offs, lens, nx, alphabet, SYM_WIDE, (size_t)1 << 30, 2048);
}

extern "C" int annchor_set_strings(annchor_ctx *c, const uint8_t *symbols, const int64_t *offs,
                                   const int32_t *lens, int64_t nx, int32_t alphabet)
{
    if (!c || !symbols || !offs || !lens) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, nx > 1 && nx < (1ll << 31), ANNCHOR_ELIMIT, "nx=%lld out of range", (long long)nx);
    ANN_REQUIRE(c, alphabet >= 1 && alphabet <= 256, ANNCHOR_ELIMIT, "alphabet=%d not in 1..256", alphabet);
    ANN_TRY(set_lev_strings(c, symbols, offs, lens, nx, alphabet, SYM_BYTES, (size_t)1 << 31, 32 * 64 * 8));
    {   // anchor rounds (lev.hip, k_lev_a2): strings of <= 16 words first
        std::vector<int32_t> ord((size_t)nx);
        int64_t ns = 0;
        for (int64_t s = 0; s < nx; ++s) ns += lens[s] <= 512;
        int64_t a = 0, b = ns;
        for (int64_t s = 0; s < nx; ++s) ord[(size_t)(lens[s] <= 512 ? a++ : b++)] = (int32_t)s;
        ANN_TRY(ann_reserve(c, c->lev_order, sizeof(int32_t) * (size_t)nx));
        ANN_TRY(ann_h2d(c, c->lev_order.p, ord.data(), sizeof(int32_t) * (size_t)nx));
        c->lev_nshort = (int)ns;
    }
    {   // slot classes of the Levenshtein kernel (lev.hip, k_lev_f): P pairs per wave for the longest string,
        // P + 1 for pairs whose shorter string has <= 64 / (P + 1) words
        const int W = (c->maxlen + 31) / 32 > 0 ? (c->maxlen + 31) / 32 : 1;
        if (W <= 32) {
            const int gl0 = 64 / (64 / W + 1);
            if (gl0 >= 1) {
                int64_t cnt = 0;
                for (int64_t s = 0; s < nx; ++s) cnt += (lens[s] + 31) / 32 <= gl0;
                c->lev_gl0 = gl0;
                c->lev_frac0 = (double)cnt / (double)nx;
            }
        }
    }
    return ANNCHOR_OK;
}

// The ragged pool of the sequence and set measures (seqdp.hip, hausdorff.hip): the members' points end to end in `sym` as
// strings are (f32 or f64, `dim` coordinates each); int32 offsets in `soff`, lengths in `slen` and the longest in `maxlen`, all
// counted in POINTS.  A metric's wording of the refusals: "series" of "values" for "dtw", and so on; at_dim: the length limit
// depends on dim and the message says so.  min_dim .. max_dim: the dims taken, 1 .. 4 but for the wide loaders (seqwide.hip, editwide.hip, threshwide.hip, hauswide.hip).
struct PoolWords {
    const char *noun, *unit, *metric_name;
    bool at_dim;
};

template <typename T> static int set_pool(annchor_ctx *c, const T *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                          int32_t dim, int limit, const PoolWords &w, int metric, int min_dim = 1, int max_dim = 4)
{
    if (!c || !values || !offs || !lens) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, nx > 1 && nx < (1ll << 31), ANNCHOR_ELIMIT, "nx=%lld out of range", (long long)nx);
    ANN_REQUIRE(c, dim >= min_dim && dim <= max_dim, ANNCHOR_ELIMIT, "%s dim %d: %s supports %d..%d", w.noun, dim, w.metric_name, min_dim, max_dim);
    char at[16] = "";
    if (w.at_dim) snprintf(at, sizeof at, " at dim %d", dim);
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    // (counted in points: total x dim < 2^31 values)
    const PoolLayout L = pool_layout(lens, nx, 1, limit, 1, (((size_t)1 << 31) - 1) / (size_t)dim + 1);
    const long long at_s = (long long)L.at;
    ANN_REQUIRE(c, L.refusal != PoolRefusal::TooShort, ANNCHOR_EINVAL, "%s %lld is empty", w.noun, at_s);
    ANN_REQUIRE(c, L.refusal != PoolRefusal::TooLong, ANNCHOR_ELIMIT, "%s %lld has %d %s: %s supports 1..%d%s", w.noun, at_s, lens[L.at],
                w.unit, w.metric_name, limit, at);
    ANN_REQUIRE(c, L.refusal != PoolRefusal::TooLarge, ANNCHOR_ELIMIT, "%s pool exceeds 2^31 values", w.noun);
    std::vector<T> pool(L.total * (size_t)dim);
    for (int64_t s = 0; s < nx; ++s) {
        ANN_REQUIRE(c, offs[s] >= 0, ANNCHOR_EINVAL, "negative offset at %lld", (long long)s);
        const T *src = values + offs[s] * dim;
        const size_t cnt = (size_t)lens[s] * (size_t)dim;
        for (size_t k = 0; k < cnt; ++k)
            ANN_REQUIRE(c, std::isfinite((double)src[k]), ANNCHOR_EINVAL, "%s %lld holds a non-finite value", w.noun, (long long)s);
        memcpy(pool.data() + (size_t)L.offs[(size_t)s] * (size_t)dim, src, sizeof(T) * cnt);
    }
    return pool_commit(c, pool.data(), pool.size() * sizeof(T), L.offs.data(), lens, nx, L.maxlen, metric);
}

// Time series for dynamic time warping: dim 1, the Sakoe-Chiba half width in `dtw_window`
template <typename T> static int set_series(annchor_ctx *c, const T *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                            int32_t window, int metric)
{
    ANN_TRY(set_pool(c, values, offs, lens, nx, 1, 2048, {"series", "values", "dtw", false}, metric));
    c->curve_dim = 1;
    c->dtw_window = window < 0 ? -1 : window;
    return ANNCHOR_OK;
}

// The same with `dim` coordinates per point in `curve_dim`: Frechet's length limits
template <typename T> static int set_series_nd(annchor_ctx *c, const T *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                               int32_t dim, int32_t window, int metric)
{
    ANN_TRY(set_pool(c, values, offs, lens, nx, dim, dim <= 2 ? 2048 : 1024, {"series", "points", "dtw", true}, metric));
    c->curve_dim = dim;
    c->dtw_window = window < 0 ? -1 : window;
    return ANNCHOR_OK;
}

// Series for the edit distance on real sequences and the longest-common-subsequence distance: `dim` coordinates per point in
// `curve_dim`, the matching threshold in `match_eps`; EDR's `normalize`; LCSS's delta in `dtw_window` (the kernel's band slot)
// (wide_name, "wide edr" / "wide lcss": the loader of threshwide.hip, 5 .. 64 coordinates per point)
template <typename T> static int set_thresh_series(annchor_ctx *c, const T *values, const int64_t *offs, const int32_t *lens,
                                                   int64_t nx, int32_t dim, double eps, const char *name, int metric,
                                                   const char *wide_name = nullptr)
{
    if (!c) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, std::isfinite(eps) && eps >= 0.0, ANNCHOR_EINVAL, "%s: the threshold eps is not a finite number >= 0", name);
    if (wide_name)
        ANN_TRY(set_pool(c, values, offs, lens, nx, dim, 1024, {"series", "points", wide_name, true}, metric, 5, 64));
    else
        ANN_TRY(set_pool(c, values, offs, lens, nx, dim, dim <= 2 ? 2048 : 1024, {"series", "points", name, true}, metric));
    c->curve_dim = dim;
    c->match_eps = eps;
    return ANNCHOR_OK;
}

extern "C" int annchor_set_series_nd_f32(annchor_ctx *c, const float *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                         int32_t dim, int32_t window)
{
    return set_series_nd(c, values, offs, lens, nx, dim, window, ANNCHOR_METRIC_DTW_F32);
}

extern "C" int annchor_set_series_nd_f64(annchor_ctx *c, const double *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                         int32_t dim, int32_t window)
{
    return set_series_nd(c, values, offs, lens, nx, dim, window, ANNCHOR_METRIC_DTW_F64);
}

extern "C" int annchor_set_edr_series_f32(annchor_ctx *c, const float *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                          int32_t dim, double eps, int32_t normalize)
{
    ANN_TRY(set_thresh_series(c, values, offs, lens, nx, dim, eps, "edr", ANNCHOR_METRIC_EDR_F32));
    c->edr_normalize = normalize != 0;
    return ANNCHOR_OK;
}

extern "C" int annchor_set_edr_series_f64(annchor_ctx *c, const double *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                          int32_t dim, double eps, int32_t normalize)
{
    ANN_TRY(set_thresh_series(c, values, offs, lens, nx, dim, eps, "edr", ANNCHOR_METRIC_EDR_F64));
    c->edr_normalize = normalize != 0;
    return ANNCHOR_OK;
}

extern "C" int annchor_set_lcss_series_f32(annchor_ctx *c, const float *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                           int32_t dim, double eps, int32_t delta)
{
    ANN_TRY(set_thresh_series(c, values, offs, lens, nx, dim, eps, "lcss", ANNCHOR_METRIC_LCSS_F32));
    c->dtw_window = delta < 0 ? -1 : delta;
    return ANNCHOR_OK;
}

extern "C" int annchor_set_lcss_series_f64(annchor_ctx *c, const double *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                           int32_t dim, double eps, int32_t delta)
{
    ANN_TRY(set_thresh_series(c, values, offs, lens, nx, dim, eps, "lcss", ANNCHOR_METRIC_LCSS_F64));
    c->dtw_window = delta < 0 ? -1 : delta;
    return ANNCHOR_OK;
}

// EDR and LCSS on series of 5 .. 64 coordinates per point (threshwide.hip): the same pool, metric ids and fields; curve_dim > 4
// is what sends a launch to k_threshwide
extern "C" int annchor_set_edr_series_wide_f32(annchor_ctx *c, const float *values, const int64_t *offs, const int32_t *lens,
                                               int64_t nx, int32_t dim, double eps, int32_t normalize)
{
    ANN_TRY(set_thresh_series(c, values, offs, lens, nx, dim, eps, "edr", ANNCHOR_METRIC_EDR_F32, "wide edr"));
    c->edr_normalize = normalize != 0;
    return ANNCHOR_OK;
}

extern "C" int annchor_set_edr_series_wide_f64(annchor_ctx *c, const double *values, const int64_t *offs, const int32_t *lens,
                                               int64_t nx, int32_t dim, double eps, int32_t normalize)
{
    ANN_TRY(set_thresh_series(c, values, offs, lens, nx, dim, eps, "edr", ANNCHOR_METRIC_EDR_F64, "wide edr"));
    c->edr_normalize = normalize != 0;
    return ANNCHOR_OK;
}

extern "C" int annchor_set_lcss_series_wide_f32(annchor_ctx *c, const float *values, const int64_t *offs, const int32_t *lens,
                                                int64_t nx, int32_t dim, double eps, int32_t delta)
{
    ANN_TRY(set_thresh_series(c, values, offs, lens, nx, dim, eps, "lcss", ANNCHOR_METRIC_LCSS_F32, "wide lcss"));
    c->dtw_window = delta < 0 ? -1 : delta;
    return ANNCHOR_OK;
}

extern "C" int annchor_set_lcss_series_wide_f64(annchor_ctx *c, const double *values, const int64_t *offs, const int32_t *lens,
                                                int64_t nx, int32_t dim, double eps, int32_t delta)
{
    ANN_TRY(set_thresh_series(c, values, offs, lens, nx, dim, eps, "lcss", ANNCHOR_METRIC_LCSS_F64, "wide lcss"));
    c->dtw_window = delta < 0 ? -1 : delta;
    return ANNCHOR_OK;
}

extern "C" int annchor_set_series_f32(annchor_ctx *c, const float *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                      int32_t window)
{
    return set_series(c, values, offs, lens, nx, window, ANNCHOR_METRIC_DTW_F32);
}

extern "C" int annchor_set_series_f64(annchor_ctx *c, const double *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                      int32_t window)
{
    return set_series(c, values, offs, lens, nx, window, ANNCHOR_METRIC_DTW_F64);
}

// Curves for the discrete Frechet distance and point sets for the Hausdorff distance: `dim` coordinates per point in `curve_dim`
template <typename T> static int set_curves(annchor_ctx *c, const T *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                            int32_t dim, int metric)
{
    ANN_TRY(set_pool(c, values, offs, lens, nx, dim, dim <= 2 ? 2048 : 1024, {"curve", "points", "frechet", true}, metric));
    c->curve_dim = dim;
    return ANNCHOR_OK;
}

// Series for the edit distance with real penalty: `dim` coordinates per point in `curve_dim`, the gap value in `erp_gap`, and in
// `gapsum` the boundaries of every member's matrix against any other: E(i, -1) = E(i-1, -1) + dist(x[i], gap point), summed
// left to right here, one addition per point, so that the kernel (seqdp.hip) loads what the sequential definition holds
template <typename T> static double erp_gap_cost(const T *p, int dim, double g)
{
    double t = (double)p[0] - g;
    if (dim == 1) return fabs(t);
    double s = t * t;
    for (int k = 1; k < dim; ++k) {
        t = (double)p[k] - g;
        s = s + t * t;
    }
    return sqrt(s);
}

// (wide: the loader of editwide.hip, which also takes the gap costs themselves, one per point, in `ptcost`)
template <typename T> static int set_erp_series(annchor_ctx *c, const T *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                                int32_t dim, double gap, int metric, bool wide = false)
{
    if (!c) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, std::isfinite(gap), ANNCHOR_EINVAL, "erp: the gap value is not finite");
    if (wide)
        ANN_TRY(set_pool(c, values, offs, lens, nx, dim, 1024, {"series", "points", "wide erp", true}, metric, 5, 64));
    else
        ANN_TRY(set_pool(c, values, offs, lens, nx, dim, dim == 1 ? 2048 : 1024, {"series", "points", "erp", true}, metric));
    size_t total = 0;
    for (int64_t s = 0; s < nx; ++s) total += (size_t)lens[s];
    std::vector<double> gs(total), gc(wide ? total : 0);
    size_t at = 0;   // (the pool's order: the members end to end)
    for (int64_t s = 0; s < nx; ++s) {
        const T *src = values + offs[s] * dim;
        double e = 0.0;
        for (int32_t i = 0; i < lens[s]; ++i) {
            const double g = erp_gap_cost(src + (size_t)i * dim, dim, gap);
            e = e + g;
            if (wide) gc[at] = g;
            gs[at++] = e;
        }
    }
    ANN_TRY(ann_reserve(c, c->gapsum, sizeof(double) * total));
    ANN_TRY(ann_h2d(c, c->gapsum.p, gs.data(), sizeof(double) * total));
    if (wide) {
        ANN_TRY(ann_reserve(c, c->ptcost, sizeof(double) * total));
        ANN_TRY(ann_h2d(c, c->ptcost.p, gc.data(), sizeof(double) * total));
        c->have_ptcost = true;
    }
    c->curve_dim = dim;
    c->erp_gap = gap;
    return ANNCHOR_OK;
}

// Series for Move-Split-Merge: dim 1, the cost of a split or merge in `msm_c`
template <typename T> static int set_msm_series(annchor_ctx *c, const T *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                                double cost, int metric)
{
    if (!c) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, std::isfinite(cost) && cost > 0.0, ANNCHOR_EINVAL, "msm: the cost c is not a finite number above 0");
    ANN_TRY(set_pool(c, values, offs, lens, nx, 1, 2048, {"series", "values", "msm", false}, metric));
    c->curve_dim = 1;
    c->msm_c = cost;
    return ANNCHOR_OK;
}

// Series for the time warp edit distance: `dim` coordinates per point in `curve_dim`; the kernel takes nu + lam and 2 nu, each
// rounded once, here
// dist(p, q) of two points of dim > 1 (q == nullptr: the origin), ERP's arithmetic
template <typename T> static double twe_point_dist(const T *p, const T *q, int dim)
{
    double t = (double)p[0] - (q ? (double)q[0] : 0.0);
    double s = t * t;
    for (int k = 1; k < dim; ++k) {
        t = (double)p[k] - (q ? (double)q[k] : 0.0);
        s = s + t * t;
    }
    return sqrt(s);
}

// (wide: the loader of editwide.hip, which takes dx(i) = dist(x[i], x[i-1]) + nl of every point, x[-1] the origin, in `ptcost`)
template <typename T> static int set_twe_series(annchor_ctx *c, const T *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                                int32_t dim, double nu, double lam, int metric, bool wide = false)
{
    if (!c) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, std::isfinite(nu) && nu >= 0.0, ANNCHOR_EINVAL, "twe: the stiffness nu is not a finite number >= 0");
    ANN_REQUIRE(c, std::isfinite(lam) && lam >= 0.0, ANNCHOR_EINVAL, "twe: the penalty lam is not a finite number >= 0");
    const double nl = nu + lam;
    if (wide) {
        ANN_TRY(set_pool(c, values, offs, lens, nx, dim, 1024, {"series", "points", "wide twe", true}, metric, 5, 64));
        size_t total = 0;
        for (int64_t s = 0; s < nx; ++s) total += (size_t)lens[s];
        std::vector<double> dx(total);
        size_t at = 0;   // (the pool's order: the members end to end)
        for (int64_t s = 0; s < nx; ++s) {
            const T *src = values + offs[s] * dim;
            for (int32_t i = 0; i < lens[s]; ++i)
                dx[at++] = twe_point_dist(src + (size_t)i * dim, i ? src + (size_t)(i - 1) * dim : (const T *)nullptr, dim) + nl;
        }
        ANN_TRY(ann_reserve(c, c->ptcost, sizeof(double) * total));
        ANN_TRY(ann_h2d(c, c->ptcost.p, dx.data(), sizeof(double) * total));
        c->have_ptcost = true;
    } else
        ANN_TRY(set_pool(c, values, offs, lens, nx, dim, dim == 1 ? 2048 : 1024, {"series", "points", "twe", true}, metric));
    c->curve_dim = dim;
    c->twe_nl = nl;
    c->twe_nu2 = 2.0 * nu;
    return ANNCHOR_OK;
}

template <typename T> static int set_point_sets(annchor_ctx *c, const T *values, const int64_t *offs, const int32_t *lens,
                                                int64_t nx, int32_t dim, int metric)
{
    ANN_TRY(set_pool(c, values, offs, lens, nx, dim, 4096, {"point set", "points", "hausdorff", false}, metric));
    c->curve_dim = dim;
    return ANNCHOR_OK;
}

// Point sets of 5 .. 512 coordinates per point (hauswide.hip): the same pool, metric ids and fields; curve_dim > 4 is what sends
// a launch to k_hauswide
template <typename T> static int set_point_sets_wide(annchor_ctx *c, const T *values, const int64_t *offs, const int32_t *lens,
                                                     int64_t nx, int32_t dim, int metric)
{
    ANN_TRY(set_pool(c, values, offs, lens, nx, dim, 4096, {"point set", "points", "wide hausdorff", false}, metric, 5, 512));
    c->curve_dim = dim;
    return ANNCHOR_OK;
}

// Point clouds for the earth mover's distance (emd.hip, k_emd_points): a solve takes up to 128 + 128 nodes
template <typename T> static int set_clouds(annchor_ctx *c, const T *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                            int32_t dim, int metric)
{
    ANN_TRY(set_pool(c, values, offs, lens, nx, dim, 128, {"cloud", "points", "emd", true}, metric));
    c->curve_dim = dim;
    return ANNCHOR_OK;
}

extern "C" int annchor_set_curves_f32(annchor_ctx *c, const float *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                      int32_t dim)
{
    return set_curves(c, values, offs, lens, nx, dim, ANNCHOR_METRIC_FRECHET_F32);
}

extern "C" int annchor_set_curves_f64(annchor_ctx *c, const double *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                      int32_t dim)
{
    return set_curves(c, values, offs, lens, nx, dim, ANNCHOR_METRIC_FRECHET_F64);
}

// DTW and Frechet on members of 5 .. 64 coordinates per point (seqwide.hip): the same pool, metric ids and fields; curve_dim > 4
// is what sends a launch to k_seqwide
template <typename T> static int set_series_wide(annchor_ctx *c, const T *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                                 int32_t dim, int32_t window, int metric)
{
    ANN_TRY(set_pool(c, values, offs, lens, nx, dim, 1024, {"series", "points", "wide dtw", true}, metric, 5, 64));
    c->curve_dim = dim;
    c->dtw_window = window < 0 ? -1 : window;
    return ANNCHOR_OK;
}

template <typename T> static int set_curves_wide(annchor_ctx *c, const T *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                                 int32_t dim, int metric)
{
    ANN_TRY(set_pool(c, values, offs, lens, nx, dim, 1024, {"curve", "points", "wide frechet", true}, metric, 5, 64));
    c->curve_dim = dim;
    return ANNCHOR_OK;
}

extern "C" int annchor_set_series_wide_f32(annchor_ctx *c, const float *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                           int32_t dim, int32_t window)
{
    return set_series_wide(c, values, offs, lens, nx, dim, window, ANNCHOR_METRIC_DTW_F32);
}

extern "C" int annchor_set_series_wide_f64(annchor_ctx *c, const double *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                           int32_t dim, int32_t window)
{
    return set_series_wide(c, values, offs, lens, nx, dim, window, ANNCHOR_METRIC_DTW_F64);
}

extern "C" int annchor_set_curves_wide_f32(annchor_ctx *c, const float *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                           int32_t dim)
{
    return set_curves_wide(c, values, offs, lens, nx, dim, ANNCHOR_METRIC_FRECHET_F32);
}

extern "C" int annchor_set_curves_wide_f64(annchor_ctx *c, const double *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                           int32_t dim)
{
    return set_curves_wide(c, values, offs, lens, nx, dim, ANNCHOR_METRIC_FRECHET_F64);
}

extern "C" int annchor_set_erp_series_f32(annchor_ctx *c, const float *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                          int32_t dim, double gap)
{
    return set_erp_series(c, values, offs, lens, nx, dim, gap, ANNCHOR_METRIC_ERP_F32);
}

extern "C" int annchor_set_erp_series_f64(annchor_ctx *c, const double *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                          int32_t dim, double gap)
{
    return set_erp_series(c, values, offs, lens, nx, dim, gap, ANNCHOR_METRIC_ERP_F64);
}

// ERP and TWE on members of 5 .. 64 coordinates per point (editwide.hip): the same pool, metric ids and fields, and `ptcost`;
// curve_dim > 4 is what sends a launch to k_editwide
extern "C" int annchor_set_erp_series_wide_f32(annchor_ctx *c, const float *values, const int64_t *offs, const int32_t *lens,
                                               int64_t nx, int32_t dim, double gap)
{
    return set_erp_series(c, values, offs, lens, nx, dim, gap, ANNCHOR_METRIC_ERP_F32, true);
}

extern "C" int annchor_set_erp_series_wide_f64(annchor_ctx *c, const double *values, const int64_t *offs, const int32_t *lens,
                                               int64_t nx, int32_t dim, double gap)
{
    return set_erp_series(c, values, offs, lens, nx, dim, gap, ANNCHOR_METRIC_ERP_F64, true);
}

extern "C" int annchor_set_twe_series_wide_f32(annchor_ctx *c, const float *values, const int64_t *offs, const int32_t *lens,
                                               int64_t nx, int32_t dim, double nu, double lam)
{
    return set_twe_series(c, values, offs, lens, nx, dim, nu, lam, ANNCHOR_METRIC_TWE_F32, true);
}

extern "C" int annchor_set_twe_series_wide_f64(annchor_ctx *c, const double *values, const int64_t *offs, const int32_t *lens,
                                               int64_t nx, int32_t dim, double nu, double lam)
{
    return set_twe_series(c, values, offs, lens, nx, dim, nu, lam, ANNCHOR_METRIC_TWE_F64, true);
}

extern "C" int annchor_set_msm_series_f32(annchor_ctx *c, const float *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                          double cost)
{
    return set_msm_series(c, values, offs, lens, nx, cost, ANNCHOR_METRIC_MSM_F32);
}

extern "C" int annchor_set_msm_series_f64(annchor_ctx *c, const double *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                          double cost)
{
    return set_msm_series(c, values, offs, lens, nx, cost, ANNCHOR_METRIC_MSM_F64);
}

extern "C" int annchor_set_twe_series_f32(annchor_ctx *c, const float *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                          int32_t dim, double nu, double lam)
{
    return set_twe_series(c, values, offs, lens, nx, dim, nu, lam, ANNCHOR_METRIC_TWE_F32);
}

extern "C" int annchor_set_twe_series_f64(annchor_ctx *c, const double *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                          int32_t dim, double nu, double lam)
{
    return set_twe_series(c, values, offs, lens, nx, dim, nu, lam, ANNCHOR_METRIC_TWE_F64);
}

extern "C" int annchor_set_point_sets_f32(annchor_ctx *c, const float *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                          int32_t dim)
{
    return set_point_sets(c, values, offs, lens, nx, dim, ANNCHOR_METRIC_HAUSDORFF_F32);
}

extern "C" int annchor_set_point_sets_f64(annchor_ctx *c, const double *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                          int32_t dim)
{
    return set_point_sets(c, values, offs, lens, nx, dim, ANNCHOR_METRIC_HAUSDORFF_F64);
}

extern "C" int annchor_set_point_sets_wide_f32(annchor_ctx *c, const float *values, const int64_t *offs, const int32_t *lens,
                                               int64_t nx, int32_t dim)
{
    return set_point_sets_wide(c, values, offs, lens, nx, dim, ANNCHOR_METRIC_HAUSDORFF_F32);
}

extern "C" int annchor_set_point_sets_wide_f64(annchor_ctx *c, const double *values, const int64_t *offs, const int32_t *lens,
                                               int64_t nx, int32_t dim)
{
    return set_point_sets_wide(c, values, offs, lens, nx, dim, ANNCHOR_METRIC_HAUSDORFF_F64);
}

extern "C" int annchor_set_clouds_f32(annchor_ctx *c, const float *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                      int32_t dim)
{
    return set_clouds(c, values, offs, lens, nx, dim, ANNCHOR_METRIC_EMD_POINTS_F32);
}

extern "C" int annchor_set_clouds_f64(annchor_ctx *c, const double *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                      int32_t dim)
{
    return set_clouds(c, values, offs, lens, nx, dim, ANNCHOR_METRIC_EMD_POINTS_F64);
}

// Sets of integers for the Jaccard distance (jaccard.hip), tokens form: member s is lens[s] dense codes, strictly ascending, in the
// same pool fields as above -- `sym` holds int32, a member may be empty.  The host (distances.pack_token_sets) recodes, sorts and
// removes duplicates; what is checked here is what the kernel's search relies on.
#define JACCARD_MAX_TOKENS 65536
#define JACCARD_MAX_BITS 8192
extern "C" int annchor_set_token_sets(annchor_ctx *c, const int32_t *codes, const int64_t *offs, const int32_t *lens, int64_t nx)
{
    if (!c || !codes || !offs || !lens) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, nx > 1 && nx < (1ll << 31), ANNCHOR_ELIMIT, "nx=%lld out of range", (long long)nx);
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    const PoolLayout L = pool_layout(lens, nx, 0, JACCARD_MAX_TOKENS, 1, (size_t)1 << 31);
    ANN_REQUIRE(c, L.refusal != PoolRefusal::TooShort, ANNCHOR_EINVAL, "token set %lld has a negative size", (long long)L.at);
    ANN_REQUIRE(c, L.refusal != PoolRefusal::TooLong, ANNCHOR_ELIMIT, "token set %lld has %d tokens: jaccard supports 0..%d", (long long)L.at,
                lens[L.at], JACCARD_MAX_TOKENS);
    ANN_REQUIRE(c, L.refusal != PoolRefusal::TooLarge, ANNCHOR_ELIMIT, "token set pool exceeds 2^31 codes");
    std::vector<int32_t> pool(L.total);
    for (int64_t s = 0; s < nx; ++s) {
        ANN_REQUIRE(c, offs[s] >= 0, ANNCHOR_EINVAL, "negative offset at %lld", (long long)s);
        const int32_t *src = codes + offs[s];
        int64_t prev = -1;
        for (int32_t k = 0; k < lens[s]; ++k) {
            ANN_REQUIRE(c, src[k] >= 0, ANNCHOR_EINVAL, "token set %lld holds a negative code", (long long)s);
            ANN_REQUIRE(c, src[k] > prev, ANNCHOR_EINVAL, "token set %lld: its codes are not strictly ascending", (long long)s);
            prev = src[k];
        }
        if (lens[s]) memcpy(pool.data() + L.offs[(size_t)s], src, sizeof(int32_t) * (size_t)lens[s]);
    }
    return pool_commit(c, pool.data(), pool.size() * sizeof(int32_t), L.offs.data(), lens, nx, L.maxlen, ANNCHOR_METRIC_JACCARD_TOKENS);
}

// Strings for the weighted Levenshtein distance (wed.hip): member s is lens[s] dense codes below `alphabet`, 0 .. 2048 of them, in
// the same pool fields -- `sym` holds uint8, a member may be empty.  The host (distances.pack_coded_strings) maps symbols to
// codes; what is checked here is what the kernel's table lookups and its symmetry argument rely on.  `gapsum` holds the boundaries
// of every member's matrix against any other, E(i, -1) = E(i-1, -1) + indel[x_i], summed left to right here as for ERP.  The pool
// and `gapsum` end with one slack entry: an empty member's clamped index 0 is then an address of the buffer wherever it lies.
// Nothing is uploaded before every check has passed: a refusal leaves what was bound as it was.
#define WED_MAXLEN 2048
#define WED_MAX_ALPHABET 128
#define AFFINE_MAXLEN 1024
#define OSA_MAXLEN 1024
// A metric's wording of the refusals and what tells the two apart: `gap` names the per-symbol costs ("indel", "extend"), every
// member's sum in `gapsum` starts from `open` (0.0 for weighted Levenshtein, whose sums then are what they were).
struct CodedWords {
    const char *metric_name, *gap;
    int limit, metric;
    double open;
};

// The pool plan of the loaders of coded strings (this one, Damerau-Levenshtein, indel) in the words they share: 0 .. limit symbols
// per string, a pool that stays below `cap`, which the refusal calls 2^`cap_log2` symbols
static int coded_layout(annchor_ctx *c, const int32_t *lens, int64_t nx, int limit, const char *metric_name, size_t align, size_t cap,
                        int cap_log2, PoolLayout &L)
{
    L = pool_layout(lens, nx, 0, limit, align, cap);
    ANN_REQUIRE(c, L.refusal != PoolRefusal::TooShort, ANNCHOR_EINVAL, "string %lld has a negative length", (long long)L.at);
    ANN_REQUIRE(c, L.refusal != PoolRefusal::TooLong, ANNCHOR_ELIMIT, "string %lld has %d symbols: %s supports 0..%d", (long long)L.at,
                lens[L.at], metric_name, limit);
    ANN_REQUIRE(c, L.refusal != PoolRefusal::TooLarge, ANNCHOR_ELIMIT, "string pool exceeds 2^%d symbols", cap_log2);
    return ANNCHOR_OK;
}

static int set_coded_strings(annchor_ctx *c, const uint8_t *codes, const int64_t *offs, const int32_t *lens, int64_t nx,
                             int32_t alphabet, const double *substitution, const double *indel, const CodedWords &w)
{
    if (!c || !codes || !offs || !lens || !substitution || !indel) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, nx > 1 && nx < (1ll << 31), ANNCHOR_ELIMIT, "nx=%lld out of range", (long long)nx);
    ANN_REQUIRE(c, alphabet >= 1 && alphabet <= WED_MAX_ALPHABET, ANNCHOR_ELIMIT, "alphabet=%d: %s supports 1..%d symbols",
                alphabet, w.metric_name, WED_MAX_ALPHABET);
    ANN_REQUIRE(c, std::isfinite(w.open) && w.open >= 0.0, ANNCHOR_EINVAL, "%s: open is not a finite cost >= 0", w.metric_name);
    const int A = alphabet;
    for (int a = 0; a < A; ++a) {
        ANN_REQUIRE(c, std::isfinite(indel[a]) && indel[a] >= 0.0, ANNCHOR_EINVAL, "%s: %s[%d] is not a finite cost >= 0", w.metric_name, w.gap, a);
        ANN_REQUIRE(c, substitution[a * A + a] == 0.0, ANNCHOR_EINVAL, "%s: substitution[%d][%d] is not 0", w.metric_name, a, a);
        for (int b = 0; b < A; ++b) {
            const double s = substitution[a * A + b];
            ANN_REQUIRE(c, std::isfinite(s) && s >= 0.0, ANNCHOR_EINVAL, "%s: substitution[%d][%d] is not a finite cost >= 0", w.metric_name, a, b);
            ANN_REQUIRE(c, memcmp(&s, &substitution[b * A + a], sizeof s) == 0, ANNCHOR_EINVAL,
                        "%s: substitution[%d][%d] != substitution[%d][%d]", w.metric_name, a, b, b, a);
        }
    }
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    PoolLayout L;
    ANN_TRY(coded_layout(c, lens, nx, w.limit, w.metric_name, 1, ((size_t)1 << 31) - 1, 31, L));
    std::vector<uint8_t> pool(L.total + 1, (uint8_t)0);
    std::vector<double> gs(L.total + 1, 0.0);
    for (int64_t s = 0; s < nx; ++s) {
        ANN_REQUIRE(c, offs[s] >= 0, ANNCHOR_EINVAL, "negative offset at %lld", (long long)s);
        const uint8_t *src = codes + offs[s];
        size_t at = (size_t)L.offs[(size_t)s];
        double e = w.open;
        for (int32_t i = 0; i < lens[s]; ++i, ++at) {
            ANN_REQUIRE(c, src[i] < A, ANNCHOR_EINVAL, "string %lld holds code %d: the alphabet has %d symbols", (long long)s, (int)src[i], A);
            pool[at] = src[i];
            e = e + indel[src[i]];
            gs[at] = e;
        }
    }
    std::vector<double> tab((size_t)A * A + A);
    memcpy(tab.data(), indel, sizeof(double) * (size_t)A);   // (the kernel's LDS image: g, then S)
    memcpy(tab.data() + A, substitution, sizeof(double) * (size_t)A * A);
    ANN_TRY(pool_commit(c, pool.data(), pool.size(), L.offs.data(), lens, nx, L.maxlen, w.metric));
    ANN_TRY(ann_reserve(c, c->gapsum, sizeof(double) * gs.size()));
    ANN_TRY(ann_h2d(c, c->gapsum.p, gs.data(), sizeof(double) * gs.size()));
    ANN_TRY(ann_reserve(c, c->wedtab, sizeof(double) * tab.size()));   // (grow-only: a rebind overwrites the costs bound before)
    ANN_TRY(ann_h2d(c, c->wedtab.p, tab.data(), sizeof(double) * tab.size()));
    c->alphabet = A;
    c->affine_open = w.open;
    return ANNCHOR_OK;
}

extern "C" int annchor_set_coded_strings(annchor_ctx *c, const uint8_t *codes, const int64_t *offs, const int32_t *lens, int64_t nx,
                                         int32_t alphabet, const double *substitution, const double *indel)
{
    return set_coded_strings(c, codes, offs, lens, nx, alphabet, substitution, indel,
                             {"weighted_levenshtein", "indel", WED_MAXLEN, ANNCHOR_METRIC_WEIGHTED_LEVENSHTEIN, 0.0});
}

// Strings under affine gap costs (wed.hip, k_affine): the same pool and table with `extend` in the place of `indel`, 0 .. 1024
// codes per string, and H(i, -1) = P(i, -1) = ((open + extend[x_0]) + extend[x_1]) + ... in `gapsum`.  (-0.0 + 0.0: a gap_open of
// -0.0 is bound as 0.0.)
extern "C" int annchor_set_coded_strings_affine(annchor_ctx *c, const uint8_t *codes, const int64_t *offs, const int32_t *lens,
                                                int64_t nx, int32_t alphabet, const double *substitution, const double *extend,
                                                double gap_open)
{
    return set_coded_strings(c, codes, offs, lens, nx, alphabet, substitution, extend,
                             {"affine_gap", "extend", AFFINE_MAXLEN, ANNCHOR_METRIC_AFFINE_GAP, gap_open + 0.0});
}

// Strings under optimal string alignment (wed.hip, k_osa): weighted Levenshtein's pool, table and sums (from 0.0), 0 .. 1024 codes
// per string, and the cost of swapping two adjacent symbols, kept in the context: >= 0, +inf for "no transpositions".  It is
// checked first, so a refused value uploads nothing.  (-0.0 + 0.0: a transpose of -0.0 is bound as 0.0.)
extern "C" int annchor_set_coded_strings_osa(annchor_ctx *c, const uint8_t *codes, const int64_t *offs, const int32_t *lens,
                                             int64_t nx, int32_t alphabet, const double *substitution, const double *indel,
                                             double transpose)
{
    if (!c) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, transpose >= 0.0, ANNCHOR_EINVAL, "osa: transpose is not a cost >= 0 (+inf: no transpositions)");   // (NaN fails too)
    ANN_TRY(set_coded_strings(c, codes, offs, lens, nx, alphabet, substitution, indel,
                              {"osa", "indel", OSA_MAXLEN, ANNCHOR_METRIC_OSA, 0.0}));
    c->osa_transpose = transpose + 0.0;
    return ANNCHOR_OK;
}

// Strings under the unrestricted Damerau-Levenshtein distance at unit costs (dlev.hip): member s is lens[s] 16-bit dense codes
// below `alphabet`, 0 .. DLEV_MAXLEN of them, in the same pool fields -- `sym` holds uint16, a member may be empty, and the pool
// ends with one slack entry as the coded strings' does.  Only the equality of codes matters: no table, no `gapsum`.  Nothing is
// uploaded before every check has passed.
extern "C" int annchor_set_strings_dlev(annchor_ctx *c, const uint16_t *codes, const int64_t *offs, const int32_t *lens, int64_t nx,
                                        int32_t alphabet)
{
    if (!c || !codes || !offs || !lens) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, nx > 1 && nx < (1ll << 31), ANNCHOR_ELIMIT, "nx=%lld out of range", (long long)nx);
    ANN_REQUIRE(c, alphabet >= 1 && alphabet <= 65535, ANNCHOR_ELIMIT, "alphabet=%d: damerau_levenshtein supports 1..65535 symbols",
                alphabet);
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    PoolLayout L;
    ANN_TRY(coded_layout(c, lens, nx, DLEV_MAXLEN, "damerau_levenshtein", 1, ((size_t)1 << 31) - 1, 31, L));
    std::vector<uint16_t> pool(L.total + 1, (uint16_t)0);
    for (int64_t s = 0; s < nx; ++s) {
        ANN_REQUIRE(c, offs[s] >= 0, ANNCHOR_EINVAL, "negative offset at %lld", (long long)s);
        const uint16_t *src = codes + offs[s];
        for (int32_t i = 0; i < lens[s]; ++i) {
            ANN_REQUIRE(c, src[i] < alphabet, ANNCHOR_EINVAL, "string %lld holds code %d: the alphabet has %d symbols", (long long)s,
                        (int)src[i], alphabet);
            pool[(size_t)L.offs[(size_t)s] + (size_t)i] = src[i];
        }
    }
    ANN_TRY(pool_commit(c, pool.data(), pool.size() * sizeof(uint16_t), L.offs.data(), lens, nx, L.maxlen, ANNCHOR_METRIC_DAMERAU_LEVENSHTEIN));
    c->alphabet = alphabet;
    return ANNCHOR_OK;
}

// Strings under the indel (LCS) distance (indel.hip): member s is lens[s] 16-bit dense codes below `alphabet`, 0 .. INDEL_MAXLEN of
// them.  Up to 256 symbols the pool holds them as bytes (SYM_BYTES, D = uint8_t) for k_indel_f's match-mask tables; beyond, as
// 16-bit codes (SYM_WIDE, D = uint16_t) for k_indel_w.  One slot class, so no length census.  Nothing is uploaded before every
// check has passed.
template <typename D> static int set_indel_strings(annchor_ctx *c, const uint16_t *codes, const int64_t *offs, const int32_t *lens,
                                                   int64_t nx, int32_t alphabet, const SymLayout &lay)
{
    PoolLayout L;
    ANN_TRY(coded_layout(c, lens, nx, INDEL_MAXLEN, "indel", lay.align, (size_t)1 << 30, 30, L));
    const size_t lds = ann_indel_lds_bytes(alphabet, L.maxlen);
    ANN_REQUIRE(c, lds <= 160 * 1024, ANNCHOR_ELIMIT, "alphabet %d x length %d needs %zu B of LDS (> 160 KiB)", alphabet, L.maxlen, lds);
    std::vector<D> pool(L.total + lay.slack, (D)lay.pad);
    for (int64_t s = 0; s < nx; ++s) {
        ANN_REQUIRE(c, offs[s] >= 0, ANNCHOR_EINVAL, "negative offset at %lld", (long long)s);
        const uint16_t *src = codes + offs[s];
        for (int32_t i = 0; i < lens[s]; ++i) {
            ANN_REQUIRE(c, src[i] < alphabet, ANNCHOR_EINVAL, "string %lld holds code %d: the alphabet has %d symbols", (long long)s,
                        (int)src[i], alphabet);
            pool[(size_t)L.offs[(size_t)s] + (size_t)i] = (D)src[i];
        }
    }
    ANN_TRY(pool_commit(c, pool.data(), pool.size() * sizeof(D), L.offs.data(), lens, nx, L.maxlen, ANNCHOR_METRIC_INDEL));
    c->alphabet = alphabet;
    c->sym_wide = sizeof(D) == 2;
    return ANNCHOR_OK;
}

extern "C" int annchor_set_strings_indel(annchor_ctx *c, const uint16_t *codes, const int64_t *offs, const int32_t *lens, int64_t nx,
                                         int32_t alphabet)
{
    if (!c || !codes || !offs || !lens) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, nx > 1 && nx < (1ll << 31), ANNCHOR_ELIMIT, "nx=%lld out of range", (long long)nx);
    ANN_REQUIRE(c, alphabet >= 1 && alphabet <= 65535, ANNCHOR_ELIMIT, "alphabet=%d: indel supports 1..65535 symbols", alphabet);
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    return alphabet > 256 ? set_indel_strings<uint16_t>(c, codes, offs, lens, nx, alphabet, SYM_WIDE)
                          : set_indel_strings<uint8_t>(c, codes, offs, lens, nx, alphabet, SYM_BYTES);
}

// The same sets, bits form: member s is row s of `words`, W = ceil(nbits / 32) rounded up to a multiple of 4 words each (`set_words`),
// bit p of a member in bit p % 32 of word p / 32.  `slen` holds the rows' popcounts -- the kernel counts only the intersection --
// and `soff` the rows' starts in words.
extern "C" int annchor_set_bitsets(annchor_ctx *c, const uint32_t *words, int64_t nx, int32_t nbits)
{
    if (!c || !words) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, nx > 1 && nx < (1ll << 31), ANNCHOR_ELIMIT, "nx=%lld out of range", (long long)nx);
    ANN_REQUIRE(c, nbits >= 1 && nbits <= JACCARD_MAX_BITS, ANNCHOR_ELIMIT, "nbits=%d: jaccard's bitsets support 1..%d bits", nbits,
                JACCARD_MAX_BITS);
    const int W = ((nbits + 31) / 32 + 3) & ~3;
    ANN_REQUIRE(c, (size_t)nx * (size_t)W < (1ull << 31), ANNCHOR_ELIMIT, "bitset pool exceeds 2^31 words");
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    std::vector<int32_t> o((size_t)nx), cnt((size_t)nx);
    int maxlen = 0;
    for (int64_t s = 0; s < nx; ++s) {
        const uint32_t *row = words + (size_t)s * (size_t)W;
        int pc = 0;
        for (int w = 0; w < W; ++w) {
            const int first = w * 32;   // the bits of this word at or past nbits are padding
            const uint32_t pad = first >= nbits ? 0xffffffffu : nbits - first >= 32 ? 0u : ~0u << (nbits - first);
            ANN_REQUIRE(c, (row[w] & pad) == 0, ANNCHOR_EINVAL, "bitset %lld has a padding bit set (nbits=%d)", (long long)s, nbits);
            pc += __builtin_popcount(row[w]);
        }
        o[(size_t)s] = (int32_t)(s * W);
        cnt[(size_t)s] = pc;
        if (pc > maxlen) maxlen = pc;
    }
    ANN_TRY(pool_commit(c, words, sizeof(uint32_t) * (size_t)nx * (size_t)W, o.data(), cnt.data(), nx, maxlen, ANNCHOR_METRIC_JACCARD_BITS));
    c->set_words = W;
    return ANNCHOR_OK;
}

// wide: annchor_set_histograms_wide -- whatever the narrow binding takes is stored and routed as it stores and routes it; beyond
// that, under a metric ground cost, every data set whose solves have at most 256 nodes goes to the wide simplex kernel (emd.hip)
static int set_histograms(annchor_ctx *c, const double *hist, int64_t nx, int32_t nbins, const double *cost, bool wide)
{
    if (!c || !hist || !cost) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, nx > 1 && nx < (1ll << 31), ANNCHOR_ELIMIT, "nx=%lld out of range", (long long)nx);
    ANN_REQUIRE(c, nbins >= 1 && nbins <= 1024, ANNCHOR_ELIMIT, "nbins=%d: this build supports 1..1024 bins", nbins);
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    int maxs = 0;
    bool integral = true;
    double maxsum = 0, maxval = 0;
    for (int64_t s = 0; s < nx; ++s) {
        int k = 0;
        double sum = 0;
        for (int b = 0; b < nbins; ++b) {
            const double v = hist[s * nbins + b];
            if (v > maxval) maxval = v;
            k += v != 0;
            sum += v;
            if (v < 0 || v != (double)(int64_t)v) integral = false;
        }
        if (sum > maxsum) maxsum = sum;
        ANN_REQUIRE(c, k > 0, ANNCHOR_EINVAL, "histogram %lld is empty", (long long)s);
        if (k > maxs) maxs = k;
    }
    // more than 64 bins: sparse histograms only (at most 32 non-zero entries each, kept as (bin, mass) lists: the two supports of a
    // solve are then at most 64 nodes, one lane each); the metric test below must hold as well
    const bool narrow = nbins <= 64 || maxs <= 32;   // what annchor_set_histograms takes
    ANN_REQUIRE(c, wide || narrow, ANNCHOR_ELIMIT,
                "histograms of %d bins: at most 32 non-zero entries each are supported beyond 64 bins (largest support here: %d)", nbins, maxs);
    // the wide route: dense rows up to 256 bins (a solve's two supports are disjoint: at most 256 nodes), (bin, mass) lists of at
    // most 128 entries beyond (128 + 128 nodes)
    ANN_REQUIRE(c, narrow || nbins <= 256 || maxs <= 128, ANNCHOR_ELIMIT,
                "histograms of %d bins: at most 128 non-zero entries each are supported beyond 256 bins -- a solve takes up to 256 nodes (largest support here: %d)", nbins, maxs);
    const bool wide_dense = !narrow && nbins <= 256, wide_lists = !narrow && !wide_dense;
    const int stride = wide_lists ? maxs : 32;
    ANN_TRY(ann_arena_init(c, nx));
    ANN_TRY(ann_prewarm_state(c));
    ANN_TRY(ann_reserve(c, c->cost, sizeof(double) * (size_t)nbins * nbins));
    if (nbins <= 64 || wide_dense) {
        ANN_TRY(ann_reserve(c, c->hist, sizeof(double) * (size_t)nx * nbins));
        ANN_TRY(ann_h2d(c, c->hist.p, hist, sizeof(double) * (size_t)nx * nbins));
    } else {
        std::vector<int32_t> hb((size_t)nx * stride, 0), hc((size_t)nx, 0);
        std::vector<double> hv((size_t)nx * stride, 0.0);
        for (int64_t s = 0; s < nx; ++s) {
            int k = 0;
            for (int b = 0; b < nbins; ++b) {
                const double v = hist[s * nbins + b];
                if (v != 0) { hb[(size_t)s * stride + k] = b; hv[(size_t)s * stride + k] = v; ++k; }
            }
            hc[(size_t)s] = k;
        }
        ANN_TRY(ann_reserve(c, c->hs_bin, sizeof(int32_t) * hb.size()));
        ANN_TRY(ann_reserve(c, c->hs_val, sizeof(double) * hv.size()));
        ANN_TRY(ann_reserve(c, c->hs_cnt, sizeof(int32_t) * hc.size()));
        ANN_TRY(ann_h2d(c, c->hs_bin.p, hb.data(), sizeof(int32_t) * hb.size()));
        ANN_TRY(ann_h2d(c, c->hs_val.p, hv.data(), sizeof(double) * hv.size()));
        ANN_TRY(ann_h2d(c, c->hs_cnt.p, hc.data(), sizeof(int32_t) * hc.size()));
    }
    ANN_TRY(ann_h2d(c, c->cost.p, cost, sizeof(double) * (size_t)nbins * nbins));
    reset_bound(c);   // (the exception among the loaders: this one commits and uploads BEFORE its last check, the metric test below)
    c->metric = ANNCHOR_METRIC_WASSERSTEIN;
    c->nx = nx;
    c->nbins = nbins;
    c->max_support = maxs;
    c->hist_integral = integral && maxsum * maxsum < 2147483647.0;
    c->hist_fits_i16 = c->hist_integral && maxval * maxsum < 32767.0;   // a flow is at most (a mass) x (the other histogram's sum)
    // Is the ground cost a metric on the bins (zero diagonal, triangle inequality)?  Then mass two histograms hold on the same
    // bin stays where it is in some optimal plan, and the solver works on the two differences only (csrc/emd.hip).  The
    // inequality is tested with a relative slack of 2^-40: Euclidean costs computed in floating point miss it by an ulp on
    // collinear bins, and a violation of eps changes the optimum by at most eps x the moved mass.
    bool metric_cost = true;
    for (int i = 0; i < nbins && metric_cost; ++i) {
        if (cost[i * nbins + i] != 0.0) metric_cost = false;
        for (int j = 0; j < nbins && metric_cost; ++j) {
            const double cij = cost[i * nbins + j];
            if (!(cij >= 0.0)) { metric_cost = false; break; }
            for (int k = 0; k < nbins; ++k) {
                const double via = cost[i * nbins + k] + cost[k * nbins + j];
                if (cij > via + 9.094947017729282e-13 * via) { metric_cost = false; break; }
            }
        }
    }
    ANN_REQUIRE(c, nbins <= 64 || metric_cost, ANNCHOR_ELIMIT,
                "histograms of %d bins need a metric ground cost (zero diagonal, triangle inequality): the solver for other costs takes up to 64 bins", nbins);
    c->cost_is_metric = metric_cost;
    c->emd_wide = !narrow;
    c->hs_stride = wide_lists ? stride : 0;
    c->cost_max = 0.0;
    for (int i = 0; i < nbins * nbins; ++i) c->cost_max = std::max(c->cost_max, fabs(cost[i]));
    reset_pipeline(c);
    return ANNCHOR_OK;
}

extern "C" int annchor_set_histograms(annchor_ctx *c, const double *hist, int64_t nx, int32_t nbins,
                                      const double *cost)
{
    return set_histograms(c, hist, nx, nbins, cost, false);
}

extern "C" int annchor_set_histograms_wide(annchor_ctx *c, const double *hist, int64_t nx, int32_t nbins,
                                           const double *cost)
{
    return set_histograms(c, hist, nx, nbins, cost, true);
}

// ----------------------------------------------------------- metric boundary
int ann_metric_launch(annchor_ctx *c, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    switch (c->metric) {
    case ANNCHOR_METRIC_LEVENSHTEIN: return ann_lev_launch(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_EUCLIDEAN_F32:
    case ANNCHOR_METRIC_EUCLIDEAN_F64:
    case ANNCHOR_METRIC_COSINE_F32:
    case ANNCHOR_METRIC_COSINE_F64: return ann_euclid_launch(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_WASSERSTEIN:
        return c->emd_wide ? ann_emd_wide_launch(c, src, d_out, d_RA, d_ncm) : ann_emd_launch(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_DTW_F32:
    case ANNCHOR_METRIC_DTW_F64:
    case ANNCHOR_METRIC_FRECHET_F32:
    case ANNCHOR_METRIC_FRECHET_F64:
        return c->curve_dim > 4 ? ann_seqwide_launch(c, src, d_out, d_RA, d_ncm) : ann_seqdp_launch(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_ERP_F32:
    case ANNCHOR_METRIC_ERP_F64:
    case ANNCHOR_METRIC_TWE_F32:
    case ANNCHOR_METRIC_TWE_F64:
        return c->curve_dim > 4 ? ann_editwide_launch(c, src, d_out, d_RA, d_ncm) : ann_seqdp_launch(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_MSM_F32:
    case ANNCHOR_METRIC_MSM_F64: return ann_seqdp_launch(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_EDR_F32:
    case ANNCHOR_METRIC_EDR_F64:
    case ANNCHOR_METRIC_LCSS_F32:
    case ANNCHOR_METRIC_LCSS_F64:
        return c->curve_dim > 4 ? ann_threshwide_launch(c, src, d_out, d_RA, d_ncm) : ann_seqdp_launch(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_HAUSDORFF_F32:
    case ANNCHOR_METRIC_HAUSDORFF_F64:
        return c->curve_dim > 4 ? ann_hauswide_launch(c, src, d_out, d_RA, d_ncm) : ann_hausdorff_launch(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_WEIGHTED_LEVENSHTEIN:
    case ANNCHOR_METRIC_AFFINE_GAP:
    case ANNCHOR_METRIC_OSA: return ann_wed_launch(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_DAMERAU_LEVENSHTEIN: return ann_dlev_launch(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_INDEL: return ann_indel_launch(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_EMD_POINTS_F32:
    case ANNCHOR_METRIC_EMD_POINTS_F64: return ann_emd_points_launch(c, src, d_out, d_RA, d_ncm);
    case ANNCHOR_METRIC_JACCARD_TOKENS:
    case ANNCHOR_METRIC_JACCARD_BITS: return ann_jaccard_launch(c, src, d_out, d_RA, d_ncm);
    default: ann_set_err(c, "no device metric bound to this context"); return ANNCHOR_EINVAL;
    }
}

__global__ void k_ij64_to_int2(const int64_t *__restrict__ ij, int2 *__restrict__ out, int64_t n)
{
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) out[t] = make_int2((int)ij[2 * t], (int)ij[2 * t + 1]);
}

extern "C" int annchor_metric_pairs(annchor_ctx *c, const int64_t *ij, int64_t n, double *out)
{
    if (!c || (n > 0 && (!ij || !out))) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, c->metric != ANNCHOR_METRIC_NONE, ANNCHOR_EINVAL, "no device metric bound to this context");
    ANN_REQUIRE(c, n >= 0 && n < (1ll << 31), ANNCHOR_ELIMIT, "n=%lld out of range", (long long)n);
    if (n == 0) return ANNCHOR_OK;
    for (int64_t t = 0; t < 2 * n; ++t)
        ANN_REQUIRE(c, ij[t] >= 0 && ij[t] < c->nx, ANNCHOR_EINVAL, "pair index %lld out of range", (long long)ij[t]);
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    ANN_TRY(ann_reserve(c, c->stage_in, sizeof(int64_t) * 2 * (size_t)n));
    ANN_TRY(ann_reserve(c, c->tmp0, sizeof(int2) * (size_t)n));
    ANN_TRY(ann_reserve(c, c->stage_out, sizeof(double) * (size_t)n));
    ANN_TRY(ann_h2d(c, c->stage_in.p, ij, sizeof(int64_t) * 2 * (size_t)n));
    k_ij64_to_int2<<<ann_blocks(n, 256), 256, 0, c->stream>>>(c->stage_in.as<int64_t>(), c->tmp0.as<int2>(), n);
    PairSource src;
    src.ij = c->tmp0.as<int2>();
    src.n = n;
    ANN_CHECK_HIP(c, hipEventRecord(c->call_a, c->stream));
    ANN_TRY(ann_metric_launch(c, src, c->stage_out.as<double>(), nullptr, nullptr));
    ANN_CHECK_HIP(c, hipEventRecord(c->call_b, c->stream));
    c->call_timed = true;
    ANN_CHECK_HIP(c, hipGetLastError());
    return ann_d2h(c, out, c->stage_out.p, sizeof(double) * (size_t)n);
}
