/*
 * annchor_hip.h -- C-ABI of libannchor_hip.so, the MI355X (gfx950) implementation of
 * the ANNchor `Annchor.fit()` -> `neighbor_graph` hot path.
 *
 * The reference (gchq/annchor) is pure Python + numba and has no FFI of its own; the
 * entry points below are exactly what a binding of its hot-path functions would
 * call.  Each one cites the reference function it replaces (paths relative to the
 * reference repository root).  INTEGRATION.md shows the ctypes stubs.
 *
 * Conventions
 *   - every function returns 0 on success or a negative ANNCHOR_E* code;
 *     annchor_last_error(ctx) gives a message for the last failure on that ctx;
 *   - all pointer arguments are HOST pointers owned by the caller; the library
 *     copies in/out and keeps no host pointer after returning;
 *   - all pipeline state lives in HBM inside the opaque context between calls;
 *   - one in-flight call per context (no internal locking); contexts are independent;
 *   - "pair position" = row index into the candidate pair list IJs built by
 *     annchor_build_locality (sorted by (i, j), i < j).
 */
#ifndef ANNCHOR_HIP_H
#define ANNCHOR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct annchor_ctx annchor_ctx;

enum {
    ANNCHOR_OK = 0,
    ANNCHOR_EINVAL = -1,   /* bad argument / call out of order            */
    ANNCHOR_EHIP = -2,     /* HIP runtime error (message has the details) */
    ANNCHOR_ENODEV = -3,   /* no usable GPU                               */
    ANNCHOR_ELIMIT = -4,   /* size outside what this build supports       */
    ANNCHOR_ESTATE = -5    /* algorithmic failure the reference raises on */
};

enum { ANNCHOR_METRIC_NONE = 0, ANNCHOR_METRIC_LEVENSHTEIN = 1, ANNCHOR_METRIC_EUCLIDEAN_F32 = 2,
       ANNCHOR_METRIC_EUCLIDEAN_F64 = 3, ANNCHOR_METRIC_WASSERSTEIN = 4, ANNCHOR_METRIC_COSINE_F32 = 5,
       ANNCHOR_METRIC_COSINE_F64 = 6, ANNCHOR_METRIC_DTW_F32 = 7, ANNCHOR_METRIC_DTW_F64 = 8,
       ANNCHOR_METRIC_FRECHET_F32 = 9, ANNCHOR_METRIC_FRECHET_F64 = 10, ANNCHOR_METRIC_HAUSDORFF_F32 = 11,
       ANNCHOR_METRIC_HAUSDORFF_F64 = 12, ANNCHOR_METRIC_ERP_F32 = 13, ANNCHOR_METRIC_ERP_F64 = 14,
       ANNCHOR_METRIC_EMD_POINTS_F32 = 15, ANNCHOR_METRIC_EMD_POINTS_F64 = 16, ANNCHOR_METRIC_JACCARD_TOKENS = 17,
       ANNCHOR_METRIC_JACCARD_BITS = 18, ANNCHOR_METRIC_WEIGHTED_LEVENSHTEIN = 19, ANNCHOR_METRIC_MSM_F32 = 20,
       ANNCHOR_METRIC_MSM_F64 = 21, ANNCHOR_METRIC_TWE_F32 = 22, ANNCHOR_METRIC_TWE_F64 = 23,
       ANNCHOR_METRIC_AFFINE_GAP = 24, ANNCHOR_METRIC_EDR_F32 = 25, ANNCHOR_METRIC_EDR_F64 = 26,
       ANNCHOR_METRIC_LCSS_F32 = 27, ANNCHOR_METRIC_LCSS_F64 = 28, ANNCHOR_METRIC_OSA = 29 };

/* fields for annchor_download / annchor_upload */
enum {
    ANNCHOR_F_D = 1,        /* float64 [nx, na]  anchor distances (row-major as the reference's D) */
    ANNCHOR_F_A = 2,        /* int64   [nA]      anchor indices                                    */
    ANNCHOR_F_SID = 3,      /* uint64  [nx][w]   nearest-anchor bitmask (bit a = anchor a in sid); w = 1 / 2 / 4 words for <= 64 / 128 / 256 anchors, ceil(na / 64) above (up to 1024) */
    ANNCHOR_F_IJS = 4,      /* int64   [n, 2]    candidate pairs                                   */
    ANNCHOR_F_I_PTR = 5,    /* int64   [nx+1]    CSR offsets of I                                  */
    ANNCHOR_F_I_IDX = 6,    /* int64   [2n]      CSR pair positions of I ([n] after annchor_build_query_locality: each pair sits in its query's row only) */
    ANNCHOR_F_FEATURES = 7, /* float64 [n, 4]    lb, ub, dad, is_anchor                            */
    ANNCHOR_F_NCM = 8,      /* uint8   [n]       not_computed_mask                                 */
    ANNCHOR_F_RA = 9,       /* float64 [n]       RefineApprox                                      */
    ANNCHOR_F_LABELS = 10,  /* int64   [n]       error-bin label per pair                          */
    ANNCHOR_F_THRESH = 11,  /* float64 [nx]      per-row threshold                                 */
    ANNCHOR_F_PROB = 12,    /* float64 [n]       ECDF probability (-1 on computed pairs)           */
    ANNCHOR_F_CAND = 13,    /* int64   [ncand]   pair positions selected for refinement (ascending) */
    ANNCHOR_F_NEXT = 14,    /* int64   [nnext]   lookahead pair positions (ascending)              */
    ANNCHOR_F_DAD = 15      /* float64 [n]       double anchor distance only                       */
};

/* ---------------------------------------------------------------- lifecycle */
int annchor_create(int device, annchor_ctx **out);
void annchor_destroy(annchor_ctx *ctx);
/* A destroyed context parks its stream, pinned staging, events and device slab (up to 2 GB) for the
 * next context on the same device (at most four such shells per process).  This frees them; returns
 * how many there were. */
int annchor_release_parked(void);
/* Device memory this process holds for reuse on `device` (parked slabs + cached blocks of closed contexts): memory the next context
 * gets without asking the driver, so it counts as free when a data set is sized (annchor_amd/_native.py: pairlist_point_limit). */
int annchor_parked_bytes(int device, int64_t *bytes);
const char *annchor_last_error(annchor_ctx *ctx);
/* Non-ctx error text for failures of annchor_create itself. */
const char *annchor_create_error(void);
int annchor_device_name(annchor_ctx *ctx, char *buf, int buflen);
/* PCI bus id of a device ("0000:c1:00.0", buflen >= 16): for binding the process to the GPU's NUMA node. */
int annchor_device_pci_bus_id(int device, char *buf, int buflen);
/* Free / total memory of a device in bytes (the host derives the largest pair list it will materialise from it). */
int annchor_device_mem_info(int device, int64_t *free_bytes, int64_t *total_bytes);
int annchor_synchronize(annchor_ctx *ctx);
/* Device-side elapsed time (ms) of the work enqueued by the most recent call,
 * measured with HIP events on the context's stream. */
int annchor_last_kernel_ms(annchor_ctx *ctx, float *ms);

/* ------------------------------------------------------------------ data set
 * Replaces the `X` operand of get_exact(f, X, IJ) (annchor/utils.py:110-177).
 * Strings: symbols[offs[s] .. offs[s]+lens[s]) are dense symbol codes
 * 0..alphabet-1 (the host maps characters to codes). */
int annchor_set_strings(annchor_ctx *ctx, const uint8_t *symbols, const int64_t *offs,
                        const int32_t *lens, int64_t nx, int32_t alphabet);
/* The same for alphabets of 257 .. 65 535 distinct symbols: 16-bit dense codes (a Unicode corpus).  Levenshtein then runs the
 * kernel that computes its match words per column (about six times slower than the table-driven ones, exact for any alphabet). */
int annchor_set_strings_u16(annchor_ctx *ctx, const uint16_t *symbols, const int64_t *offs, const int32_t *lens, int64_t nx,
                            int32_t alphabet);
int annchor_set_points_f32(annchor_ctx *ctx, const float *X, int64_t nx, int32_t dim);
int annchor_set_points_f64(annchor_ctx *ctx, const double *X, int64_t nx, int32_t dim);
/* Same data, metric = cosine distance 1 - u.v / (|u| |v|), clipped to [0, 2]
 * (annchor/utils.py:14,67 -> scipy.spatial.distance.cosine). */
int annchor_set_points_cosine_f32(annchor_ctx *ctx, const float *X, int64_t nx, int32_t dim);
int annchor_set_points_cosine_f64(annchor_ctx *ctx, const double *X, int64_t nx, int32_t dim);
/* Univariate time series under dynamic time warping (no reference counterpart: the reference bundles no DTW).  Series s is
 * values[offs[s] .. offs[s]+lens[s]), 1 .. 2048 finite values each (longer: ANNCHOR_ELIMIT; a non-finite value: ANNCHOR_EINVAL).
 * d(x, y) = sqrt(D(n-1, m-1)) with D(i, j) = (x_i - y_j)^2 + min(D(i-1, j), D(i, j-1), D(i-1, j-1)), D(-1, -1) = 0 and +inf
 * outside the matrix, all in float64 (float32 values widen exactly; the square is a rounded difference times itself, never
 * fused).  window < 0: unconstrained; window >= 0: cells with |i - j| > max(window, |n - m|) are +inf (a Sakoe-Chiba band that
 * always reaches the corner).  Every cell has fixed operands and min is exact, so the value is the sequential recurrence's bit
 * for bit (csrc/seqdp.hip).  DTW can violate the triangle inequality: fit with is_metric = 0. */
int annchor_set_series_f32(annchor_ctx *ctx, const float *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                           int32_t window);
int annchor_set_series_f64(annchor_ctx *ctx, const double *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                           int32_t window);
/* Series of `dim` coordinates per point under the same dynamic time warping, dim in 1 .. 4.  `values` holds the points end to end;
 * offs and lens are counted in POINTS: series s is the points offs[s] .. offs[s]+lens[s).  A series has 1 .. 2048 points at
 * dim <= 2 and 1 .. 1024 points at dim 3 and 4 (longer, or a dim outside 1 .. 4: ANNCHOR_ELIMIT); every value is finite (else
 * ANNCHOR_EINVAL).  The cell's cost is Frechet's c(i, j) below:
 *   c(i, j) = sum over k = 0 .. dim-1, in that order, of t_k * t_k,  t_k = x[i][k] - y[j][k]   (each operation rounded on its own)
 *   D(i, j) = c(i, j) + min(D(i-1, j), D(i, j-1), D(i-1, j-1)),   D(-1, -1) = 0, +inf outside the matrix
 *   dtw(x, y) = sqrt(D(n-1, m-1)), correctly rounded
 * `window` as above.  At dim 1 this is annchor_set_series_*, bit for bit.  Not a metric: fit with is_metric = 0. */
int annchor_set_series_nd_f32(annchor_ctx *ctx, const float *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                              int32_t dim, int32_t window);
int annchor_set_series_nd_f64(annchor_ctx *ctx, const double *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                              int32_t dim, int32_t window);
/* Series under the edit distance on real sequences, EDR (Chen, Ozsu & Oria 2005; no reference counterpart).  `values`, `dim`,
 * offs and lens as for annchor_set_series_nd_*: 1 .. 2048 points at dim <= 2 and 1 .. 1024 points at dim 3 and 4 (longer, or a
 * dim outside 1 .. 4: ANNCHOR_ELIMIT); every value is finite (else ANNCHOR_EINVAL).  `eps` is the matching threshold: finite and
 * >= 0 (else ANNCHOR_EINVAL, before anything is uploaded).  All arithmetic is float64; float32 input widens exactly.
 *   match(p, q) iff fabs(p[k] - q[k]) <= eps for every k = 0 .. dim-1   (each subtraction rounded on its own; a difference of
 *               exactly eps matches; a threshold per coordinate, not a Euclidean ball)
 *   E(-1, -1) = 0     E(i, -1) = i + 1     E(-1, j) = j + 1
 *   E(i, j) = min( E(i-1, j-1) + (match(x[i], y[j]) ? 0.0 : 1.0),   E(i-1, j) + 1.0,   E(i, j-1) + 1.0 )
 *   edr(x, y) = E(n-1, m-1)                      normalize == 0 (an edit count)
 *             = E(n-1, m-1) / (double)max(n, m)  normalize != 0 (one float64 division)
 * Every cell is an integer of at most 4096, which float64 holds exactly: the value is the sequential recurrence's bit for bit,
 * and edr(x, y) == edr(y, x) bit for bit (csrc/seqdp.hip).  There is no window.  EDR violates the triangle inequality and
 * edr(x, y) = 0 does not imply x = y: fit with is_metric = 0. */
int annchor_set_edr_series_f32(annchor_ctx *ctx, const float *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                               int32_t dim, double eps, int32_t normalize);
int annchor_set_edr_series_f64(annchor_ctx *ctx, const double *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                               int32_t dim, double eps, int32_t normalize);
/* Series under the longest-common-subsequence distance, LCSS (Vlachos, Kollios & Gunopulos 2002; no reference counterpart).
 * `values`, `dim`, offs, lens, `eps`, match and the limits as for EDR.  `delta` limits how far apart in time two matched points
 * may be; delta < 0: no limit.  It is plain: never widened to |n - m| as DTW's band is.
 *   L(-1, -1) = L(i, -1) = L(-1, j) = 0
 *   L(i, j) = L(i-1, j-1) + 1.0          if match(x[i], y[j]) and (delta < 0 or |i - j| <= delta)
 *           = max(L(i-1, j), L(i, j-1))  otherwise
 *   lcss(x, y) = 1.0 - L(n-1, m-1) / (double)min(n, m)     (one division, one subtraction; in [0, 1])
 * Every cell is an integer of at most 2048: the value is the sequential recurrence's bit for bit, and lcss(x, y) == lcss(y, x)
 * bit for bit (csrc/seqdp.hip).  Not a metric: fit with is_metric = 0. */
int annchor_set_lcss_series_f32(annchor_ctx *ctx, const float *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                int32_t dim, double eps, int32_t delta);
int annchor_set_lcss_series_f64(annchor_ctx *ctx, const double *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                                int32_t dim, double eps, int32_t delta);
/* Curves under the discrete Frechet distance (no reference counterpart).  `values` holds the points end to end, `dim`
 * coordinates each, dim in 1 .. 4; offs and lens are counted in POINTS: curve s is the points offs[s] .. offs[s]+lens[s).  A curve
 * has 1 .. 2048 points at dim <= 2 and 1 .. 1024 points at dim 3 and 4 (longer, or a dim outside 1 .. 4: ANNCHOR_ELIMIT); every
 * value is finite (else ANNCHOR_EINVAL).  All arithmetic is float64; float32 input widens exactly.
 *   c(i, j) = sum over k = 0 .. dim-1, in that order, of t_k * t_k,  t_k = x[i][k] - y[j][k]
 *             (every subtraction, product and addition rounded on its own, never an fma;
 *              the sum starts from the k = 0 product, not from 0.0 + ...)
 *   F(i, j) = max(c(i, j), min(F(i-1, j), F(i, j-1), F(i-1, j-1))),   F(-1, -1) = 0, +inf outside the matrix
 *   frechet(x, y) = sqrt(F(n-1, m-1)), correctly rounded
 * max and min are exact and every c(i, j) has fixed operands, so the value is the sequential recurrence's bit for bit
 * (csrc/seqdp.hip).  There is no window.  A (pseudo-)metric: fit with is_metric = 1. */
int annchor_set_curves_f32(annchor_ctx *ctx, const float *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                           int32_t dim);
int annchor_set_curves_f64(annchor_ctx *ctx, const double *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                           int32_t dim);
/* Series under the edit distance with real penalty, ERP (Chen & Ng 2004; no reference counterpart).  `values` holds the points
 * end to end, `dim` coordinates each, dim in 1 .. 4; offs and lens are counted in POINTS: series s is the points
 * offs[s] .. offs[s]+lens[s).  A series has 1 .. 2048 points at dim 1 and 1 .. 1024 points at dim 2, 3 and 4 (longer, or a dim
 * outside 1 .. 4: ANNCHOR_ELIMIT); every value is finite, and so is `gap` (else ANNCHOR_EINVAL).  All arithmetic is float64;
 * float32 input widens exactly.  `gap` is the gap value g; the gap point is (g, ..., g).
 *   dist(a, b)  dim 1:   |a[0] - b[0]|
 *               dim > 1: sqrt( sum over k = 0 .. dim-1, in that order, of t_k * t_k ),  t_k = a[k] - b[k],  correctly rounded sqrt
 *               (every subtraction, product and addition rounded on its own, never an fma; the sum starts from the k = 0 product)
 *   gx(i) = dist(x[i], gap point)        gy(j) = dist(y[j], gap point)
 *   E(-1, -1) = 0     E(i, -1) = E(i-1, -1) + gx(i)     E(-1, j) = E(-1, j-1) + gy(j)        (left to right, one addition per step)
 *   E(i, j) = min( E(i-1, j-1) + dist(x[i], y[j]),   E(i-1, j) + gx(i),   E(i, j-1) + gy(j) )
 *   erp(x, y) = E(n-1, m-1)                                                                    (no square root at the end)
 * Every cell is the min of three sums of fixed operands, min is exact and the additions are commutative, so the value is the
 * sequential recurrence's bit for bit, and erp(x, y) == erp(y, x) bit for bit (csrc/seqdp.hip).  There is no window: a banded
 * ERP loses the triangle inequality.  A metric: fit with is_metric = 1. */
int annchor_set_erp_series_f32(annchor_ctx *ctx, const float *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                               int32_t dim, double gap);
int annchor_set_erp_series_f64(annchor_ctx *ctx, const double *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                               int32_t dim, double gap);
/* Univariate series under Move-Split-Merge, MSM (Stefan, Athitsos & Das 2013; no reference counterpart).  Series s is
 * values[offs[s] .. offs[s]+lens[s]), 1 .. 2048 finite values each (longer: ANNCHOR_ELIMIT; a non-finite value: ANNCHOR_EINVAL).
 * `c` is the cost of a split or merge: finite and > 0 (else ANNCHOR_EINVAL, before anything is uploaded).  All arithmetic is
 * float64, every operation rounded on its own; float32 input widens exactly.  Indices are 0-based; x has n >= 1 values, y has m >= 1.
 *   M(-1, -1) = 0     M(i, -1) = M(-1, j) = +inf     the virtual previous values x[-1] and y[-1] are 0.0
 *   C(v, a, b) = c                              if a <= v <= b or a >= v >= b
 *              = c + min(|v - a|, |v - b|)      otherwise
 *   M(i, j) = min( M(i-1, j-1) + |x[i] - y[j]|,   M(i-1, j) + C(x[i], x[i-1], y[j]),   M(i, j-1) + C(y[j], x[i], y[j-1]) )
 *   msm(x, y) = M(n-1, m-1)
 * (the virtual values only ever meet +inf; this is the textbook form, M(0, 0) = |x[0] - y[0]| and a first row and column of
 * running sums of C, bit for bit).  Every cell is the min of three sums of fixed operands, so the value is the sequential
 * recurrence's bit for bit; C is symmetric in (a, b), so msm(x, y) == msm(y, x) bit for bit (csrc/seqdp.hip).  There is no
 * window.  A metric: fit with is_metric = 1. */
int annchor_set_msm_series_f32(annchor_ctx *ctx, const float *values, const int64_t *offs, const int32_t *lens, int64_t nx, double c);
int annchor_set_msm_series_f64(annchor_ctx *ctx, const double *values, const int64_t *offs, const int32_t *lens, int64_t nx, double c);
/* Series under the time warp edit distance, TWE (Marteau 2009; no reference counterpart), with uniform timestamps: point i has
 * time i + 1.  `values`, `dim`, offs and lens as for ERP: 1 .. 2048 points at dim 1 and 1 .. 1024 points at dim 2, 3 and 4 (longer,
 * or a dim outside 1 .. 4: ANNCHOR_ELIMIT); every value is finite (else ANNCHOR_EINVAL).  `nu` is the stiffness and `lam` the
 * penalty of a delete: both finite and >= 0 (else ANNCHOR_EINVAL, before anything is uploaded).  All arithmetic is float64, every
 * operation rounded on its own; float32 input widens exactly.  dist is ERP's dist.  nl = nu + lam and nu2 = 2.0 * nu are formed
 * once.
 *   T(-1, -1) = 0     T(i, -1) = T(-1, j) = +inf     the virtual previous points x[-1] and y[-1] are the origin
 *   dx(i) = dist(x[i], x[i-1]) + nl        dy(j) = dist(y[j], y[j-1]) + nl
 *   T(i, j) = min( T(i-1, j-1) + ((dist(x[i], y[j]) + dist(x[i-1], y[j-1])) + nu2 * (double)|i - j|),
 *                  T(i-1, j) + dx(i),   T(i, j-1) + dy(j) )
 *   twe(x, y) = T(n-1, m-1)
 * (Marteau's recurrence in its common implementation: zero-padded series, DP[0, 0] = 0, +inf on the rest of row 0 and column 0).
 * Every cell is the min of three sums of fixed operands, so the value is the sequential recurrence's bit for bit, and
 * twe(x, y) == twe(y, x) bit for bit (csrc/seqdp.hip).  There is no window.  A metric: fit with is_metric = 1. */
int annchor_set_twe_series_f32(annchor_ctx *ctx, const float *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                               int32_t dim, double nu, double lam);
int annchor_set_twe_series_f64(annchor_ctx *ctx, const double *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                               int32_t dim, double nu, double lam);
/* Strings under the weighted Levenshtein distance (no reference counterpart: the reference answers every cost model but unit
 * costs with a user-supplied host function).  An alphabet of `alphabet` distinct symbols, 1 .. 128 (else ANNCHOR_ELIMIT); string s
 * is the dense codes codes[offs[s] .. offs[s]+lens[s]), each below `alphabet` (else ANNCHOR_EINVAL, with the string's index in the
 * message), 0 .. 2048 of them -- a string may be empty (longer, a pool of 2^31 symbols or more: ANNCHOR_ELIMIT).  `substitution` is
 * S, float64 [alphabet][alphabet] row-major: finite, >= 0, zero diagonal, S[a][b] == S[b][a] bit for bit; `indel` is g, float64
 * [alphabet], the cost of inserting or deleting each symbol: finite, >= 0 (else ANNCHOR_EINVAL, naming the entry).  Both are copied
 * into buffers of the context, replaced by the next call and released with the context.  All arithmetic is float64.
 *   E(-1, -1) = 0     E(i, -1) = E(i-1, -1) + g[x_i]     E(-1, j) = E(-1, j-1) + g[y_j]        (left to right, one addition per step)
 *   E(i, j) = min( E(i-1, j-1) + S[x_i][y_j],   E(i-1, j) + g[x_i],   E(i, j-1) + g[y_j] )
 *   wed(x, y) = E(n-1, m-1)            wed(x, "") = E(n-1, -1)            wed("", "") = 0.0
 * Every cell is the min of three sums of fixed operands, min is exact and the additions are commutative, so the value is the
 * sequential recurrence's bit for bit, and wed(x, y) == wed(y, x) bit for bit because S is (csrc/wed.hip).  Mapping symbols to
 * codes is the caller's part.  A metric exactly when the costs are one on the symbols and the gap (off-diagonal S > 0, g > 0,
 * the triangle inequalities among S and g): fit with is_metric = 1 then, with 0 otherwise.  A refused call leaves what was bound
 * before as it was. */
int annchor_set_coded_strings(annchor_ctx *ctx, const uint8_t *codes, const int64_t *offs, const int32_t *lens, int64_t nx,
                              int32_t alphabet, const double *substitution, const double *indel);
/* The same strings under affine gap costs (no reference counterpart): a run of k symbols against a gap costs open + the sum of
 * their extension costs, not k independent indels (Gotoh's three-state recurrence).  codes, offs, lens, alphabet and
 * `substitution` are as above, with 0 .. 1024 codes per string; `extend` is g, float64 [alphabet], the cost of each symbol inside
 * a gap: finite, >= 0; `gap_open` is o, the cost of opening a gap: finite, >= 0 (else ANNCHOR_EINVAL).  All arithmetic is float64.
 *   H(-1,-1) = 0     P(-1, j) = +inf     Q(i, -1) = +inf     P(-1,-1) = Q(-1,-1) = +inf
 *   P(i, j) = min( P(i-1, j), H(i-1, j) + o ) + g[x_i]                          (x_i against a gap)
 *   Q(i, j) = min( Q(i, j-1), H(i, j-1) + o ) + g[y_j]                          (y_j against a gap)
 *   H(i, j) = min( H(i-1, j-1) + S[x_i][y_j],   P(i, j),   Q(i, j) )
 *   affine(x, y) = H(n-1, m-1)     affine(x, "") = P(n-1, -1) = ((o + g[x_0]) + g[x_1]) + ...     affine("", "") = 0.0
 * Every cell is a min of sums of fixed operands, so the value is the sequential recurrence's bit for bit; the transposed matrix
 * swaps P and Q and holds the same H, so affine(x, y) == affine(y, x) bit for bit; with gap_open = 0.0 the value is
 * annchor_set_coded_strings' bit for bit (csrc/wed.hip, k_affine).  A metric under the conditions given above for S and g
 * (gap_open >= 0 keeps the gap function subadditive).  A refused call leaves what was bound before as it was. */
int annchor_set_coded_strings_affine(annchor_ctx *ctx, const uint8_t *codes, const int64_t *offs, const int32_t *lens, int64_t nx,
                                     int32_t alphabet, const double *substitution, const double *extend, double gap_open);
/* The same strings under optimal string alignment, OSA (no reference counterpart): the weighted edit distance above with one more
 * edit, the swap of two adjacent symbols at the cost `transpose`.  No substring is edited twice: this is the RESTRICTED form, not
 * the unrestricted Damerau-Levenshtein distance.  codes, offs, lens, alphabet, `substitution` and `indel` are as for
 * annchor_set_coded_strings, with 0 .. 1024 codes per string; `transpose` is T, a double >= 0, +inf meaning "no transpositions"
 * (NaN or negative: ANNCHOR_EINVAL, checked before anything else).  All arithmetic is float64.
 *   E(-1,-1), E(i,-1), E(-1,j) as above
 *   E(i, j) = min( E(i-1, j-1) + S[x_i][y_j],   E(i-1, j) + g[x_i],   E(i, j-1) + g[y_j],
 *                  E(i-2, j-2) + T   if i >= 1 and j >= 1 and x_i == y_{j-1} and x_{i-1} == y_j )
 *   osa(x, y) = E(n-1, m-1)            osa(x, "") = E(n-1, -1)            osa("", "") = 0.0
 * Row -1 and column -1 are legal sources of the fourth term.  Every cell is a min of sums of fixed operands, so the value is the
 * sequential recurrence's bit for bit; the condition is symmetric in the two strings, so osa(x, y) == osa(y, x) bit for bit; with
 * transpose = +inf the value is annchor_set_coded_strings' bit for bit (csrc/wed.hip, k_osa).  NOT a metric whatever the costs:
 * at unit costs osa("ca", "abc") = 3 > osa("ca", "ac") + osa("ac", "abc") = 2; fit with is_metric = 0.  A refused call leaves
 * what was bound before as it was. */
int annchor_set_coded_strings_osa(annchor_ctx *ctx, const uint8_t *codes, const int64_t *offs, const int32_t *lens, int64_t nx,
                                  int32_t alphabet, const double *substitution, const double *indel, double transpose);
/* Point sets under the Hausdorff distance (no reference counterpart).  `values` holds the points end to end, `dim` coordinates
 * each; offs and lens are counted in POINTS: set s is the points offs[s] .. offs[s]+lens[s).  A point set is 1 .. 4096 points of
 * `dim` coordinates, with `dim` in 1 .. 4 (a larger set, a dim outside 1 .. 4, a pool of 2^31 values or more: ANNCHOR_ELIMIT; an
 * empty set or a non-finite value: ANNCHOR_EINVAL).  All arithmetic is float64.  float32 input widens exactly.
 *   c(i, j)  = sum over k = 0 .. dim-1, in that order, of t_k * t_k,   t_k = x[i][k] - y[j][k]
 *              (every subtraction, product and addition rounded on its own: -ffp-contract=off, never an fma;
 *               the sum starts from the k = 0 product, not from 0.0 + ...)
 *   h(x, y)  = max over i of ( min over j of c(i, j) )          -- directed, x to y
 *   hausdorff(x, y) = sqrt( max( h(x, y), h(y, x) ) ), correctly rounded
 * min and max are exact and every c(i, j) has fixed operands, so the value is the definition's bit for bit under any evaluation
 * order, and hausdorff(x, y) == hausdorff(y, x) bit for bit (csrc/hausdorff.hip).  A metric on sets (on the stored arrays a
 * pseudo-metric: a permuted or duplicated copy is at distance 0): fit with is_metric = 1. */
int annchor_set_point_sets_f32(annchor_ctx *ctx, const float *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                               int32_t dim);
int annchor_set_point_sets_f64(annchor_ctx *ctx, const double *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                               int32_t dim);
/* Point clouds under the earth mover's distance with uniform masses (no reference counterpart).  `values` holds the points end to
 * end, `dim` coordinates each; offs and lens are counted in POINTS: cloud s is the points offs[s] .. offs[s]+lens[s).  A cloud is
 * 1 .. 128 points of `dim` coordinates, with `dim` in 1 .. 4 (a larger cloud, a dim outside 1 .. 4, a pool of 2^31 values or more:
 * ANNCHOR_ELIMIT; an empty cloud or a non-finite value: ANNCHOR_EINVAL).  All arithmetic is float64.  float32 input widens exactly.
 *   c(i, j)   dim 1:   |x[i][0] - y[j][0]|
 *             dim > 1: sqrt( sum over k = 0 .. dim-1, in that order, of t_k * t_k ),  t_k = x[i][k] - y[j][k]
 *             (every operation rounded on its own, never an fma, correctly rounded sqrt: ERP's `dist`, the same bits)
 *   emd(x, y) = min over F >= 0 of  sum_ij F_ij c(i, j)   with  sum_j F_ij = 1/n,  sum_i F_ij = 1/m
 * The optimum is exact (the transportation simplex of csrc/emd.hip on integer flows, no Sinkhorn).  The value is a pure function of
 * the two clouds (nothing of the rest of the data set enters a solve), emd(x, y) == emd(y, x) bit for bit (every pair is solved in
 * one canonical orientation), and it is exactly 0.0 when the clouds are equal as multisets of points.  A solve that fails (pivot
 * cap) gives NaN.  A metric on uniform point measures (on the stored arrays a pseudo-metric: a permuted copy is at distance 0):
 * fit with is_metric = 1. */
int annchor_set_clouds_f32(annchor_ctx *ctx, const float *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                           int32_t dim);
int annchor_set_clouds_f64(annchor_ctx *ctx, const double *values, const int64_t *offs, const int32_t *lens, int64_t nx,
                           int32_t dim);
/* Finite sets of integers under the Jaccard (Tanimoto) distance (no reference counterpart), in one of two layouts.
 *   i = |A n B|      u = |A| + |B| - i
 *   jaccard(A, B) = 0.0 if u == 0 (both empty),  (double)(u - i) / (double)u otherwise: one float64 division of two exact integers
 * The counts are integers, so the value is the definition's bit for bit in either layout and under any evaluation order, and
 * jaccard(A, B) == jaccard(B, A) exactly (csrc/jaccard.hip).  A metric: fit with is_metric = 1.
 * Tokens: member s is the codes offs[s] .. offs[s]+lens[s) of `codes`, non-negative and strictly ascending (else ANNCHOR_EINVAL,
 * with the member's index in the message); 0 .. 65536 codes per member, a member may be empty (more codes, a pool of 2^31 codes
 * or more: ANNCHOR_ELIMIT).  Recoding arbitrary int64 tokens to dense codes, sorting and removing duplicates is the caller's part. */
int annchor_set_token_sets(annchor_ctx *ctx, const int32_t *codes, const int64_t *offs, const int32_t *lens, int64_t nx);
/* Bits: member s is row s of `words`, W words per row, W = ceil(nbits / 32) rounded up to a multiple of 4; bit p of a member is
 * bit p % 32 of word p / 32.  nbits in 1 .. 8192 (else ANNCHOR_ELIMIT); the bits at and past nbits are zero (else ANNCHOR_EINVAL,
 * with the member's index in the message). */
int annchor_set_bitsets(annchor_ctx *ctx, const uint32_t *words, int64_t nx, int32_t nbits);
/* Wasserstein: hist float64 [nx, nbins], cost float64 [nbins, nbins]
 * (annchor/utils.py:75-86, func_kwargs['cost_matrix']).  Up to 64 bins: any histograms, any cost matrix.  65 .. 1024 bins:
 * histograms with at most 32 non-zero entries each under a metric ground cost (zero diagonal, triangle inequality) -- kept as
 * (bin, mass) lists; anything else returns ANNCHOR_ELIMIT. */
int annchor_set_histograms(annchor_ctx *ctx, const double *hist, int64_t nx, int32_t nbins,
                           const double *cost);
/* The same call with the wide exact-OT route open: whatever annchor_set_histograms accepts is stored and evaluated exactly as
 * it does.  Beyond that, under a metric ground cost, every data set whose solves have at most 256 nodes is accepted: up to 256
 * bins any histograms (dense rows), up to 1024 bins histograms with at most 128 non-zero entries each ((bin, mass) lists).
 * These run the transportation simplex with four node slots per lane (csrc/emd.hip, k_emd_wide).  Anything else -- more bins,
 * larger supports beyond 256 bins, a non-metric cost beyond 64 bins -- returns ANNCHOR_ELIMIT. */
int annchor_set_histograms_wide(annchor_ctx *ctx, const double *hist, int64_t nx, int32_t nbins,
                                const double *cost);
/* Data set without a device metric (user metric evaluated on the host). */
int annchor_set_opaque(annchor_ctx *ctx, int64_t nx);

/* --------------------------------------------------------- metric boundary a2
 * get_exact(f, X, IJ): out[t] = f(X[IJ[t,0]], X[IJ[t,1]]) as float64
 * (annchor/utils.py:110-177).  ij: int64 [n, 2]; may contain i == j and repeats. */
int annchor_metric_pairs(annchor_ctx *ctx, const int64_t *ij, int64_t n, double *out);
/* BruteForce.fit (annchor/annchor.py:1004-1023): all-pairs metric + per-row stable
 * sort; writes the first k columns of (argsort(D), sort(D)). */
int annchor_brute_force(annchor_ctx *ctx, int32_t k, int64_t *ng_idx, double *ng_dist);

/* ------------------------------------------------------------------ anchors a6
 * MaxMinAnchorPicker.get_anchors (annchor/pickers.py:18-52).  `first` is the
 * host-drawn np.random.randint(nx).  Fills A and D inside the context. */
int annchor_pick_anchors_maxmin(annchor_ctx *ctx, int32_t n_anchors, int64_t first);
/* SelectedAnchorPicker / RandomAnchorPicker (pickers.py:86-128): given indices. */
int annchor_pick_anchors_selected(annchor_ctx *ctx, const int64_t *A, int32_t n_anchors);
/* Any other picker (ExternalAnchorPicker, user classes): the host hands over
 * (A, D, evals) as AnchorPicker.get_anchors returns them.  D float64 [nx, na]. */
int annchor_set_anchor_distances(annchor_ctx *ctx, const double *D, int32_t n_anchors,
                                 const int64_t *A, int32_t nA);

/* ----------------------------------------------------------------- locality a7
 * Annchor.get_locality + get_check/adjust_check/get_IJs_from_check
 * (annchor/annchor.py:208-256, annchor/utils.py:437-540).  Returns the number of
 * candidate pairs and the smallest |I[i]| (annchor.py:252-256 raises when it is
 * below n_neighbors -- the host does that). */
int annchor_build_locality(annchor_ctx *ctx, int32_t locality, int32_t loc_thresh, int32_t loc_min,
                           int64_t *n_pairs, int64_t *min_row_len);

/* Query form (Annchor.query, annchor/query_functions.py:18-62): the bound data set is X
 * (rows [0, nx_base)) followed by the queries; candidate pairs are (i, nx_base + j) with
 * |sid[i] & sid[nx_base + j]| >= loc_thresh, sorted by (j, i); rows of X are empty. */
int annchor_build_query_locality(annchor_ctx *ctx, int64_t nx_base, int32_t locality, int32_t loc_thresh,
                                 int64_t *n_pairs, int64_t *min_row_len);

/* ------------------------------------------------------------- features a8-a10
 * get_bounds_njit_ijs, get_dad_ijs, get_features_IJ (utils.py:274-301,355-380;
 * annchor.py:258-303): lb, ub, dad, is_anchor, not_computed_mask for every pair. */
int annchor_compute_features(annchor_ctx *ctx);

/* ------------------------------------------------------------------ sample a11
 * Helpers for Sampler.sample (annchor/samplers.py:75-140) on the device-resident
 * state.  kth_uncomputed_dad: np.partition(dad[ncm], k)[k] for each requested k. */
int annchor_count_uncomputed(annchor_ctx *ctx, int64_t *n_unc);
int annchor_kth_uncomputed_dad(annchor_ctx *ctx, const int64_t *ks, int32_t nk, double *out);
/* counts[b] = #{uncomputed pairs with bins[b] <= dad < bins[b+1]} (utils.py:547-549). */
int annchor_bin_counts(annchor_ctx *ctx, const double *bins, int32_t nbins, int64_t *counts);
/* Sampler.get_partition + the partition populations in ONE host round trip (samplers.py:75-105): q[0..1] = the ks[0]-th / ks[1]-th
 * smallest dad among the uncomputed pairs; *fused = 1: edges[0..n_partitions] = {-inf, np.linspace(q[0], q[1], n_partitions - 1),
 * +inf} computed on the device (the caller compares them with its own np.linspace) and counts[b] as annchor_bin_counts would
 * give for them; *fused = 0 (very long lists, degenerate keys): only q is set, the caller continues with annchor_bin_counts. */
int annchor_sampler_stats(annchor_ctx *ctx, const int64_t *ks, int32_t n_partitions, double *q, double *edges, int64_t *counts,
                          int32_t *fused);
/* For each request t: the pair position of the ranks[t]-th (0-based, position
 * order) uncomputed pair inside bin bin_of[t]. */
int annchor_select_by_rank(annchor_ctx *ctx, const double *bins, int32_t nbins, const int32_t *bin_of,
                           const int64_t *ranks, int64_t nreq, int64_t *positions);
/* Host-only helper (no device work, no context): the draws of
 * `np.random.seed(seed)` followed, per bin, by
 * `np.random.choice(ixmask, want[b], replace=False)` (annchor/utils.py:543-578),
 * returned as ranks into the bin (= positions of the legacy permutation prefix);
 * a bin with counts[b] < want[b] yields 0..counts[b]-1 without consuming the stream.
 * ranks_out must hold sum(min(counts, want)); n_out[b] = entries written for bin b. */
/* Start generating the raw MT19937 stream of `seed` on a background host thread (it
 * depends on the seed only); a later annchor_legacy_choice_ranks(seed, ...) consumes it.
 * Purely an overlap device: results are identical with or without it. */
int annchor_legacy_prefetch(uint32_t seed, int64_t ndraws);
/* The same stream generated on the CALLING thread before the call returns (a warm core: ~0.4 ms for the 1.9 M words of
 * a C2 sampling step, against ~2 ms on a freshly woken producer thread); fit() calls it while the GPU runs a stage the
 * host would otherwise only wait for. */
int annchor_legacy_generate(uint32_t seed, int64_t ndraws);
/* ... on the calling thread at the context's NEXT host waits, `chunk` words per wait (<= 0: all at the first): after the caller's
 * next enqueues, while the GPU works on them */
int annchor_legacy_generate_at_next_wait(annchor_ctx *ctx, uint32_t seed, int64_t ndraws, int64_t chunk);
int annchor_legacy_choice_ranks(uint32_t seed, const int64_t *counts, const int64_t *want, int32_t nbins,
                                int64_t *ranks_out, int64_t *n_out);
/* The same draw on the library's persistent worker thread (warm core, warm caches), so that it
 * overlaps device work the caller enqueues meanwhile: begin() copies the inputs and returns at
 * once; end() waits, writes ranks_out / n_out as annchor_legacy_choice_ranks would, returns its
 * status and releases the ticket. */
int annchor_legacy_choice_begin(uint32_t seed, const int64_t *counts, const int64_t *want, int32_t nbins, void **ticket);
int annchor_legacy_choice_end(void *ticket, int64_t *ranks_out, int64_t *n_out);

/* Host-only helper (no device work, no context): the per-partition ordinary least squares of
 * SimpleStratifiedLinearRegression.fit (annchor/regressors.py:60-84; sklearn LinearRegression =
 * centre, LAPACK dgelsd, intercept) for all partitions in one call.  dgelsd_ptr: the Fortran
 * dgelsd of the caller's LAPACK (Python: scipy.linalg.cython_lapack.__pyx_capi__["dgelsd"]).
 * X: nf columns of ld doubles (column k at X + k * ld), y: ld doubles, samples grouped by
 * partition: partition b = rows cuts[b] .. cuts[b+1].  Out: coef [nbins, nf], xmean [nbins, nf],
 * ymean [nbins] (the intercept is ymean - xmean . coef), status [nbins] (0 = solved, 1 = fewer
 * rows than features, > 1 = LAPACK failure: solve that partition on the caller's general path). */
int annchor_ols_bins(void *dgelsd_ptr, const double *X, const double *y, int64_t ld, int32_t nf, const int64_t *cuts,
                     int32_t nbins, double *coef, double *xmean, double *ymean, int32_t *status);
/* Gather features [m, 4] at the given pair positions (self.features[sample_ixs]). */
int annchor_gather_features(annchor_ctx *ctx, const int64_t *pos, int64_t m, double *feats);
/* get_sample (annchor.py:336-343): evaluate the metric on the sample pairs, clear
 * their not_computed_mask bit, remember (positions, y) for the merge. */
int annchor_evaluate_samples(annchor_ctx *ctx, const int64_t *pos, int64_t m, double *sample_y);
/* The built-in sampling step in one call (get_sample, annchor.py:313-343): (bin, rank) -> pair
 * positions [nreq], their feature rows [nreq, 4], their exact distances [nreq]; clears
 * not_computed_mask for them.  counts = annchor_bin_counts for the same edges.  Equivalent to
 * annchor_select_by_rank + annchor_gather_features + annchor_evaluate_samples with one host
 * wait and no host round trip of the positions. */
int annchor_sample_pairs(annchor_ctx *ctx, const double *bins, int32_t nbins, const int64_t *counts, const int32_t *bin_of,
                         const int64_t *ranks, int64_t nreq, int64_t *positions, double *feats, double *sample_y);
/* Same, when the metric was evaluated by the host. */
int annchor_set_samples(annchor_ctx *ctx, const int64_t *pos, int64_t m, const double *sample_y);

/* ----------------------------------------------------- regression/errors a12-13
 * SimpleStratifiedLinearRegression.predict + clip + RefineApprox merge
 * (regressors.py:71-103, annchor.py:356-380) and
 * SimpleStratifiedErrorRegression.predict (error_predictors.py:56-67), fused.
 * bins float64 [nb+1], W float64 [nb,3], c float64 [nb].  sample_predict receives
 * the UNCLIPPED prediction at the current sample positions (annchor.py:357). */
int annchor_predict_merge(annchor_ctx *ctx, const double *bins, int32_t nb, const double *W,
                          const double *c, int32_t first_iteration, int32_t is_metric,
                          double *sample_predict);
/* Custom Regression / ErrorPredictor plugins: host-computed arrays are merged. */
int annchor_merge_host_prediction(annchor_ctx *ctx, const double *pred, int32_t first_iteration,
                                  int32_t is_metric);
int annchor_set_labels(annchor_ctx *ctx, const int64_t *labels);

/* ------------------------------------------- a11-a13 with the iteration's models fitted on the device
 * The same three stages -- get_sample (annchor.py:313-343), fit_predict_regression (annchor.py:345-380,
 * regressors.py:39-103), fit_predict_errors (annchor.py:382-393, error_predictors.py:26-53) -- without a host round
 * trip between them, for the reference's default plugins and a device metric:
 *   annchor_sample_pairs_device   = annchor_sample_pairs, results left in device memory;
 *   annchor_fit_regression_device = per-partition OLS with intercept on (lb, ub, dad) -> y (Householder QR on the centred
 *     samples, float64; coefficients agree with the reference's LAPACK dgelsd solution to ~1e-13 relative, not bit for
 *     bit -- annchor_predict_merge with host-fitted coefficients remains for that), then the fused predict / clip /
 *     merge / label pass from the coefficients in place;
 *   annchor_fit_errors_device     = per-partition sorted residuals into the context (annchor_select_candidates with
 *     errs == NULL reads them there).
 * Nothing waits for the host.  A rank-deficient partition gets dgelsd's minimum-norm solution on the device (status 0).
 * Problems a kernel finds (a sampled (bin, rank) that does not exist, a partition of fewer than three rows, an empty
 * residual list or one longer than the sorter takes) raise sticky flags that annchor_model_download returns (and clears)
 * together with the fitted coefficients; the caller redoes the step on the host path then.
 * annchor_fit_regression_device needs the feature rows of the CURRENT sample in device memory: after annchor_set_samples,
 * annchor_evaluate_samples, annchor_sample_pairs or annchor_hash_sample_pairs (which hand the rows to the host) it returns
 * ANNCHOR_ESTATE until one of the *_device sampling calls has run again.  annchor_download_samples /
 * annchor_errors_download materialise the sample arrays and the residual lists for the host (plugin-visible attributes;
 * not on the fit path). */
int annchor_sample_pairs_device(annchor_ctx *ctx, const double *bins, int32_t nbins, const int64_t *counts, const int32_t *bin_of,
                                const int64_t *ranks, int64_t nreq);
/* The same for DeviceStratifiedSampler's order-free choice (annchor_hash_sample_pairs with the results left in device memory
 * and no host wait: a partition whose key list came out short or overflowed raises the sticky sample-step flag, read with
 * annchor_model_download).  *n_out = sum over the partitions of min(want, counts). */
int annchor_hash_sample_pairs_device(annchor_ctx *ctx, const double *bins, int32_t nbins, const int64_t *counts, const int64_t *want,
                                     uint64_t seed_key, int64_t *n_out);
/* The built-in sampling step with the LEGACY draw (SimpleStratifiedSampler: NumPy's stream, utils.py:543-578) in one call, the
 * draw's backward trace on the device: the host walks the stream (the rejection scan), every bin's swap partners are uploaded on a
 * side stream as they complete, three kernels undo the swaps for the kept entries and write the chosen ranks into the slot map
 * the rank -> position kernels read.  Same samples, same order as annchor_legacy_choice_ranks + annchor_sample_pairs_device.
 * *taken = 0: not applicable here (a partition keeps more than 8192 entries): draw on the host.  The second form returns
 * the ranks alone (tests). */
int annchor_sample_pairs_device_draw(annchor_ctx *ctx, const double *bins, int32_t nbins, const int64_t *counts, const int64_t *want,
                                     uint32_t seed, int64_t *n_out, int32_t *taken);
int annchor_legacy_choice_ranks_device(annchor_ctx *ctx, uint32_t seed, const int64_t *counts, const int64_t *want, int32_t nbins,
                                       int64_t *ranks_out, int32_t *taken);
int annchor_download_samples(annchor_ctx *ctx, int64_t *positions, double *feats, double *sample_y, double *sample_predict);
int annchor_fit_regression_device(annchor_ctx *ctx, const double *bins, int32_t nbins, int32_t first_iteration, int32_t is_metric);
int annchor_fit_errors_device(annchor_ctx *ctx);
int annchor_model_download(annchor_ctx *ctx, double *W, double *c, int32_t *status, int64_t *err_ptr, int32_t *flags /*[3]*/);
int annchor_errors_download(annchor_ctx *ctx, double *errs, int64_t n_errs);
/* Both behind one host wait (what fit() calls after its last iteration): errs has room for errs_cap doubles (2 x n_samples
 * always suffices); *n_errs = err_ptr[nbins], or -1 when the flags report a failed step. */
int annchor_model_download_with_errors(annchor_ctx *ctx, double *W, double *c, int32_t *status, int64_t *err_ptr, int32_t *flags /*[3]*/,
                                       double *errs, int64_t errs_cap, int64_t *n_errs);

/* --------------------------------------------------------------- selection a14
 * select_refine_candidate_pairs (annchor.py:395-473) up to, not including, the
 * metric call: thresh, guarantee_nmin (when nmin > 0), p, ECDF prob (errs:
 * concatenated sorted residuals, err_ptr int64 [nlabels+1]; errs == NULL: the lists
 * annchor_fit_errors_device left on the device), top-n_refine and
 * lookahead selection.  Ties at a cut (np.argpartition is arbitrary there): probability descending, then
 * the fixed pseudo-random order (position * 0x9E3779B97F4A7C15 mod 2^64) >> 11 ascending, then position
 * ascending. */
int annchor_select_candidates(annchor_ctx *ctx, int32_t n_neighbors, int32_t nmin, const double *errs,
                              const int64_t *err_ptr, int32_t nlabels, int64_t n_refine,
                              int32_t lookahead, int64_t *n_cand, int64_t *n_next);
/* The part of annchor_select_candidates that depends on RefineApprox and the mask only -- row thresholds
 * (annchor.py:399-404) and guarantee_nmin (utils.py:600-621) -- launched ahead, without a host wait: the caller
 * fits its error model (error_predictors.py:26-53, host) while it runs, then calls annchor_select_candidates
 * with the same n_neighbors / nmin, which picks up from there.  Any call that changes RefineApprox or the mask
 * in between voids the preparation (the selection then starts from the beginning). */
int annchor_select_prepare(annchor_ctx *ctx, int32_t n_neighbors, int32_t nmin);
/* Clear not_computed_mask for the selected candidates ahead of their refinement
 * (annchor.py:473 does it after the metric calls).  Lets the next iteration's sampling
 * statistics (which depend on the mask and dad only, samplers.py:119-140) be taken, and the
 * host-side draw be made, while the refinement kernel runs.  Idempotent with
 * annchor_refine_candidates / annchor_set_refined. */
int annchor_mark_candidates(annchor_ctx *ctx);
/* Evaluate the metric on the selected candidates and write back
 * (annchor.py:467-473). */
int annchor_refine_candidates(annchor_ctx *ctx);
/* The max-min picker's Levenshtein rounds run as ONE persistent launch when every wave of it can be resident (reference: the
 * loop of annchor/pickers.py:44-50).  A launch that gives up (GPU shared with another process) falls back to a one-workgroup form
 * after its time limit; after two such launches the library switches the persistent form off for the process.
 * set = 0: switch it off, 1: re-arm it, other: query.  Returns 1 when it is armed. */
int annchor_lev_persist_state(int set);

/* fit() pipelining: action 1 parks the refinement launch so that the next annchor_sampler_stats (the NEXT iteration's sampling
 * statistics, which depend on the candidate marks only) queues it behind its download and waits for the statistics alone;
 * action 2 launches it now if it is still parked. */
int annchor_park_refine(annchor_ctx *ctx, int32_t action);
/* Same, host-evaluated metric: exact float64 [n_cand] in ANNCHOR_F_CAND order. */
int annchor_set_refined(annchor_ctx *ctx, const double *exact, int64_t n_cand);

/* ----------------------------------------------------------- bound update a15
 * update_anchor_points + update_bounds/get_bounds_alt (annchor.py:475-512,
 * utils.py:304-352) over the lookahead pairs, all chunks (no wall-clock cut). */
int annchor_update_bounds(annchor_ctx *ctx);
/* fit() overlap (an engine created with ANNCHOR_FIT_OVERLAP=0 in the environment runs everything on its one stream, in the order
 * of the calls; the call is then a no-op).
 * annchor_update_bounds_prepare: the half of annchor_update_bounds that reads the not-computed mask alone (row counts, scan, keys
 * of the computed-neighbour lists) on the engine's side stream.  Call it where the mask the update will see is final -- fit():
 * right after annchor_mark_candidates, before the refinement launch -- and it runs beside whatever is queued next.  A later
 * call that changes the mask (annchor_set_refined, a sampling step, a new locality, ...) voids it: annchor_update_bounds then
 * builds the lists itself, as it does without any prepare. */
int annchor_update_bounds_prepare(annchor_ctx *ctx);
/* For tests: out[0] = 1 when the engine uses a side stream, out[1] = calls of annchor_update_bounds that found their lists prepared. */
int annchor_overlap_stats(annchor_ctx *ctx, int64_t *out);

/* ------------------------------------------------------------------ graph a16
 * get_ann + get_nn (annchor.py:514-530, utils.py:383-429).  ng_idx int64 [nx, k],
 * ng_dist float64 [nx, k], column 0 = self. */
int annchor_neighbor_graph(annchor_ctx *ctx, int32_t n_neighbors, int64_t *ng_idx, double *ng_dist);

/* ------------------------------------------------ streamed form (large-N Euclidean)
 * Tile-granular form of the same path for float32 points when the pair list cannot
 * exist (N >> 10^4).  One context = one GPU = one
 * contiguous shard of rows [global_base, global_base + n_local).  See
 * annchor_amd/csrc/streamed.hip for how each stage of Annchor.fit()
 * (annchor/annchor.py:532-623) maps onto tiles.
 *
 * annchor_stream_bind: copy the shard (host or device pointer) into the context.
 * annchor_stream_anchor_round: one max-min round (annchor/pickers.py:44-50) on the shard:
 *   distances of every local row to `anchor_vec` (host float32 [dim]), running-min update,
 *   local arg-max (local index, first index on ties).  The host combines ranks.
 * annchor_stream_get_row: fetch one local row (the next anchor's coordinates).
 * annchor_stream_order: order the bound rows into 128-row tiles (balanced k-d splits in
 *   anchor-distance space) with their anchor-distance intervals; returns DEVICE pointers (owned by
 *   the context): Xs float32 [n_pad, dim_padded], rs float32 [n_pad], perm int64 [n_pad] (global
 *   ids, -1 on padding), lo/hi/mid float32 [n_anchors, n_tiles] (per-tile min / max / mean distance
 *   to each anchor).  min_tiles pads the tile count (e.g. to a multiple of the rank count).
 *   Row-sharded runs (annchor_amd/streamed.py): after the sharded anchor rounds every rank binds ALL
 *   rows (all-gathered raw shards, device pointer), replays the anchors through
 *   annchor_stream_anchor_round and orders them itself -- one tile structure whatever the rank
 *   count -- and owns a contiguous range of the global tile order.
 * annchor_stream_knn: k-NN rows of tiles [tile_begin, tile_begin+tile_count) against all
 *   column tiles (DEVICE pointers, concatenated over ranks); get_ann-shaped HOST outputs
 *   (annchor/annchor.py:514-530): column 0 = self.  Two phases: the budgeted tile phase
 *   (ceil(p_work * n_tiles) column tiles per row tile, the work budget of annchor.py:438-442),
 *   then `join_passes` passes of the streamed update_anchor_points (annchor.py:475-512,
 *   utils.py:304-352): pairs that share a computed neighbour -- j in list(c), c in list(i) --
 *   are evaluated exactly, per row tile, as gathered tile GEMMs; up to `join_extra` further
 *   passes run while a pass still replaces more than 1 % of the list entries (small data sets,
 *   whose tile budget is coarse).  Join passes need the launch to cover every row tile (one rank).
 * annchor_stream_knn_begin / _join / _end: the same build in steps for row-sharded runs: the
 *   ranks all-gather their list buffers (*lists_local: int32 [tile_count*128][k-1] ordered column
 *   indices, device memory; lists_bytes its size) after _begin and after every _join into
 *   lists_all [n_all][k-1], the input of the next _join (*updates: list entries the pass replaced
 *   on this rank); _end = annchor_stream_knn's outputs. */
int annchor_stream_bind(annchor_ctx *ctx, const float *X, int64_t n_local, int32_t dim, int64_t global_base,
                        int32_t x_on_device);
int annchor_stream_anchor_round(annchor_ctx *ctx, const float *anchor_vec, int32_t round, int32_t n_anchors,
                                double *local_max, int64_t *local_arg);
int annchor_stream_get_row(annchor_ctx *ctx, int64_t local_idx, float *out);
int annchor_stream_order(annchor_ctx *ctx, int32_t min_tiles, void **Xs, void **rs, void **perm, void **lo, void **hi,
                         void **mid, int64_t *n_pad, int32_t *n_tiles, int32_t *dim_padded);
/* The ordering in two steps, for row-sharded runs (no reference counterpart: annchor/utils.py:494-540 materialises every
 * pair; this is the streamed form's locality stage).  _order_begin runs the k-d level sorts restricted at
 * every level to the segments that hold the caller's tile range [tile_begin, tile_begin + tile_count) (tile_count <= 0:
 * all tiles) -- a rank that owns 1 / G of the tiles sorts ~(levels / G + 2) n keys instead of levels x n -- and returns
 * its slice of the order (*order_local: uint32 [tile_count x 128], device), the all-gather target (*order_all: uint32
 * [n_tiles x 128]; rank r's slice at r x *order_bytes) and the slice's size.  _order_end (after the all-gather; at once
 * when the range was everything) gathers the rows into tile order and returns annchor_stream_order's outputs. */
int annchor_stream_order_begin(annchor_ctx *ctx, int32_t min_tiles, int32_t tile_begin, int32_t tile_count, void **order_local,
                               void **order_all, int64_t *order_bytes);
int annchor_stream_order_end(annchor_ctx *ctx, void **Xs, void **rs, void **perm, void **lo, void **hi, void **mid, int64_t *n_pad,
                             int32_t *n_tiles, int32_t *dim_padded);
int annchor_stream_knn(annchor_ctx *ctx, const void *Xs_all, const void *rs_all, const void *perm_all, const void *lo_all,
                       const void *hi_all, const void *mid_all, int64_t n_all, int32_t nt_all, int32_t n_anchors, int32_t dim_padded,
                       int32_t tile_begin, int32_t tile_count, int32_t k, double p_work, int32_t join_passes, int32_t join_extra,
                       int64_t *row_ids, int64_t *ng_idx, double *ng_dist, int64_t *tile_evals);
/* annchor_stream_knn in two halves: _run leaves the finished graph on the device, _fetch downloads it (same outputs as
 * annchor_stream_knn) -- for hosts that prepare the result arrays on another thread while the GPU works. */
int annchor_stream_knn_run(annchor_ctx *ctx, const void *Xs_all, const void *rs_all, const void *perm_all, const void *lo_all,
                           const void *hi_all, const void *mid_all, int64_t n_all, int32_t nt_all, int32_t n_anchors,
                           int32_t dim_padded, int32_t tile_begin, int32_t tile_count, int32_t k, double p_work, int32_t join_passes,
                           int32_t join_extra, int64_t *tile_evals);
int annchor_stream_knn_fetch(annchor_ctx *ctx, int64_t *row_ids, int64_t *ng_idx, double *ng_dist);
int annchor_stream_knn_begin(annchor_ctx *ctx, const void *Xs_all, const void *rs_all, const void *perm_all, const void *lo_all,
                             const void *hi_all, const void *mid_all, int64_t n_all, int32_t nt_all, int32_t n_anchors,
                             int32_t dim_padded, int32_t tile_begin, int32_t tile_count, int32_t k, int32_t tile_budget,
                             void **lists_local, int64_t *lists_bytes);
int annchor_stream_knn_join(annchor_ctx *ctx, const void *lists_all, int32_t per_pass, void **lists_local, int64_t *updates);
/* Row-sharded join pass, first half (the streamed analogue of update_anchor_points' computed-neighbour lists,
 * annchor/annchor.py:475-512, restricted to the columns a rank owns): the reverse neighbour lists of this rank's tile range
 * from the all-gathered lists.  *rev_local: int32 [tile_count x 128][15] (device: the rank's slice), *rev_all: int32 [n_all][15], *rev_bytes: bytes per rank.  The host all-gathers the
 * slices and calls annchor_stream_knn_join with the same lists_all; a host that skips this call gets every column's
 * reverse list built by the join pass itself (one rank). */
int annchor_stream_join_rev_begin(annchor_ctx *ctx, const void *lists_all, void **rev_local, void **rev_all, int64_t *rev_bytes);
/* The work budget of the streamed form.  p_work is the share of THIS form's brute force -- n_tiles
 * tile evaluations per row tile -- that one row tile may spend, all phases included:
 * total = ceil(p_work * n_tiles) = tile_phase + join_passes * per_pass (per_pass = runs of 128
 * gathered columns one join pass may evaluate; when a tile has more candidates, the ones reached
 * over the most two-hop paths are kept). */
int annchor_stream_budget(int32_t n_tiles, double p_work, int32_t join_passes, int32_t *total, int32_t *tile_phase,
                          int32_t *per_pass);
int annchor_stream_knn_end(annchor_ctx *ctx, int64_t *row_ids, int64_t *ng_idx, double *ng_dist, int64_t *tile_evals);
/* Split of the last build's tile_evals: tile evaluations of the tile phase, 128-column runs of the join passes. */
int annchor_stream_last_counts(annchor_ctx *ctx, int64_t *tile_phase_evals, int64_t *join_chunks);
/* Which kernel evaluated the last build's tile phase: 0 = exact float32 tile GEMMs (v_mfma_f32_32x32x2_f32; shapes the
 * split kernels do not take: more than 30 neighbours at padded dim <= 128, more than 62 at 256, no split copy), 1 = split-fp16 tile GEMMs (three
 * v_mfma_f32_32x32x16_f16 per 16 dimensions on centred, power-of-two scaled rows: products to ~2^-22 |x||y|, the accuracy of
 * the f32 MFMA stream; K + 2 columns kept per row and re-ranked by their exact float32 distances; csrc/knnbf.hip,
 * csrc/knnh.hip, csrc/knnbk.hip).  *guard_rows = rows the split kernel flagged: its K-th exact distance came within twice the
 * measured error of the products of the list's last approximate entry, i.e. a neighbour may have stayed outside the list.
 * Flagged rows are repaired exactly (annchor_stream_last_tile_kernels) and kind stays 1.  The reported neighbour distances
 * are exact float32 in every case (the metric of the reference on float32 rows: distances.py:8-13). */
int annchor_stream_last_kernel(annchor_ctx *ctx, int32_t *kind, int64_t *guard_rows);
/* Round 6.  *two_stage = 1: the tile phase of the last build ran k_st_knnh (csrc/knnh.hip) behind a short k_st_knnbf warm-up -- fp16
 * hi-only products with a rigorous error bound decide which columns MAY enter a row's list, float32 differences of the original rows
 * (the reference's arithmetic, distances.py:8-13) decide which do: graph builds at padded dimension 128, <= 14 neighbours kept.
 * *repaired = 1: rows flagged by the split kernels' guard (see above) were evaluated again with float32 differences over the column
 * tiles their row tile evaluated (csrc/repair.hip: any dimension). */
int annchor_stream_last_tile_kernels(annchor_ctx *ctx, int32_t *two_stage, int32_t *repaired);
/* Queries against a fitted data set in the streamed form (Annchor.query, annchor.py:643-683 ->
 * query_functions.py:183-212, for data sets beyond the pair-list form).  The context holds
 * the QUERY rows: bound with annchor_stream_bind (global_base 0), given the data set's anchor
 * vectors through annchor_stream_anchor_round, ordered with annchor_stream_order.  The six
 * column arrays are the data set's.  out_idx int64 [nq, nn] (global ids), out_dist float64
 * [nq, nn], in the queries' own order. */
int annchor_stream_query(annchor_ctx *ctx, const void *Xs_all, const void *rs_all, const void *perm_all, const void *lo_all,
                         const void *hi_all, const void *mid_all, int64_t n_all, int32_t nt_all, int32_t n_anchors, int32_t dim_padded,
                         int32_t nn, double p_work, int64_t *out_idx, double *out_dist, int64_t *tile_evals);
/* float64 rows in the streamed form (annchor_amd/csrc/rerank64.hip).  The reference computes `euclidean` and `cosine` in the dtype
 * of X (annchor/distances.py:8-13: np.linalg.norm(x - y)); for float64 rows that is float64 differences, which these calls restate:
 * the float32 pipeline above becomes the filter, float64 differences of the resident float64 rows decide.
 * annchor_stream_bind_f64 (restates distances.py:8-13 for float64 X): X HOST float64 [n_local, dim]; the rows stay resident in
 *   float64; a float64 centre -- centre_in (HOST [dim]) or, NULL, the column means computed on the device -- is subtracted and the
 *   centred rows, narrowed to float32, become the context's bound rows exactly as annchor_stream_bind would have left them,
 *   with a per-row bound e_i >= |x~_i - float32(x~_i)|.  centre_out (HOST [dim], may be NULL) receives the centre; *rows64 (may
 *   be NULL) the device pointer of the float64 rows (a query context re-ranks against the DATA set's).
 * annchor_stream_rerank64 (distances.py:8-13, float64): in place of annchor_stream_knn_fetch after an annchor_stream_knn_run over
 *   every row tile with lists LONGER than asked for: every row's listed columns are measured again by float64 differences and
 *   ordered by (d^2, index); ng_idx int64 / ng_dist float64 [n_local, k], column 0 = self, k - 1 <= the run's list length.  When the
 *   run's tile budget did not bind, a guard certifies the rows whose k-th float64 distance is provably below every unlisted column's
 *   ("float64 rows") and the others are evaluated again against every column: the result is the float64 k-NN graph.
 * annchor_stream_query64 (distances.py:8-13, float64): annchor_stream_query for queries bound with annchor_stream_bind_f64 (centre_in =
 *   the data set's centre): the search keeps nn_search >= nn entries, the re-rank against rows64_data (the data set's float64 rows:
 *   n_data of them, global ids from data_base) keeps nn; guard and repair as above.
 * annchor_stream_last_rerank64: rows the last re-rank's guard flagged, and whether they were repaired. */
int annchor_stream_bind_f64(annchor_ctx *ctx, const double *X, int64_t n_local, int32_t dim, int64_t global_base, const double *centre_in,
                            double *centre_out, void **rows64);
int annchor_stream_rerank64(annchor_ctx *ctx, int32_t k, int64_t *ng_idx, double *ng_dist);
int annchor_stream_query64(annchor_ctx *ctx, const void *Xs_all, const void *rs_all, const void *perm_all, const void *lo_all,
                           const void *hi_all, const void *mid_all, int64_t n_all, int32_t nt_all, int32_t n_anchors, int32_t dim_padded,
                           int32_t nn, int32_t nn_search, double p_work, const void *rows64_data, int64_t n_data, int64_t data_base,
                           int64_t *out_idx, double *out_dist, int64_t *tile_evals);
int annchor_stream_last_rerank64(annchor_ctx *ctx, int64_t *flagged_rows, int32_t *repaired);
/* The nearest-enemy graph in the streamed form (Annchor.get_nearest_enemies, annchor/annchor.py:685-773, for data sets beyond
 * the pair-list form; annchor_amd/csrc/enemytiles.hip): for every bound row its nn nearest rows of a DIFFERENT label.  The context
 * holds the labelled rows: bound with annchor_stream_bind, given the fitted anchors through annchor_stream_anchor_round.
 * _order_classes replaces annchor_stream_order for it: the rows in k-d order, stably sorted by label code, every class padded
 * to a multiple of 128 slots -- every tile holds ONE label (class-pure tiles; padding slots are what tail padding is: zero rows,
 * +inf norms, perm -1).  labels: HOST int32 [n_local], codes 0 .. n_classes - 1, every code used; anchor_vecs: HOST float
 * [n_anchors][dim], the anchors' coordinates (the centre of the fp16 split copy is their mean; NULL: no centring).  *n_pad,
 * *n_tiles: the class-padded extent (< n_local + 128 n_classes), *dim_padded as annchor_stream_order returns it.
 * _enemies runs the tile phase in query form (rows = columns = these arrays, nn entries kept, ceil(p_work * *n_tiles) column
 * tiles per row tile, no join passes) with every same-label tile pair masked out of the ranking (rank key AND bound +inf: neither
 * the selection rounds nor the exact repair of flagged rows meet it), then guard, repair and finalize as annchor_stream_query.
 * out_idx int64 [n_local, nn] (global ids), out_dist float64 [n_local, nn]: no self column, ascending, in the bound rows' own
 * order (-1 / +inf where a budgeted run met fewer than nn rows of another label).  A later annchor_stream_order /
 * annchor_stream_order_begin on the context replaces the class-pure order: _enemies then refuses until _order_classes ran again.  annchor_stream_last_kernel,
 * annchor_stream_last_tile_kernels and annchor_stream_last_counts report on it as on a build. */
int annchor_stream_order_classes(annchor_ctx *ctx, const int32_t *labels, int32_t n_classes, const float *anchor_vecs, int64_t *n_pad,
                                 int32_t *n_tiles, int32_t *dim_padded);
int annchor_stream_enemies(annchor_ctx *ctx, int32_t nn, double p_work, int64_t *out_idx, double *out_dist, int64_t *tile_evals);
/* Interval tables after a rank-major all-gather ([world][n_anchors][n_tiles], device) joined along
 * the tile axis ([n_anchors][world * n_tiles], device): the layout the column arguments above use.
 * (For hosts that order every shard on its own rank and all-gather the ordered shards; the bundled
 * host no longer does -- see annchor_stream_order.) */
int annchor_stream_join_tables(annchor_ctx *ctx, const void *gathered, int32_t world, int32_t n_anchors, int32_t n_tiles,
                               void *joined);
/* ---- Row-sharded builds with device-resident exchange buffers (annchor_amd/csrc/sharded.hip; SURVEY.md section 8(e);
 * no reference counterpart: the reference has no collectives).  One process per GPU; the host hands the DEVICE buffers
 * below to its collective library (RCCL over xGMI) on the context's stream (annchor_stream_hip_stream) -- no host
 * round trip per max-min round, no host staging of rows, lists or results.
 *
 * Anchors (annchor/pickers.py:44-50 across ranks): _anchor_begin leaves this rank's candidate for the first anchor
 *   ((0, first_global or -1, that row's coordinates): 2 + dim doubles) in *cand; per round the host all-gathers the
 *   candidates (rank order) into *gathered (room for world of them; a single rank may pass *cand itself) and calls _anchor_step(gathered, world, round): the winner (largest value, then smallest global
 *   row) becomes anchor `round`, the local rows are swept with its coordinates (running minimum reset for rounds 0 and 1,
 *   the reference's D[1:] quirk) and this rank's next candidate replaces *cand.  Nothing waits for the host;
 *   _anchor_end downloads the anchors' global rows and coordinates.
 * Rows: _rows_begin gives the all-gather's send buffer (the shard padded with zero rows to the largest shard) and
 *   receive buffer ([world][most][dim]); _rows_end compacts what arrived, rebinds the context to ALL rows (global_base 0:
 *   rows are numbered by position in the rank-ordered concatenation).  Anchor distances: _anchor_dists_begin (between the
 *   anchor rounds and _rows_end) gives the send / receive buffers of the all-gather of the ranks' own anchor distances
 *   (float [n_anchors][most] per rank -- the "all-gather of anchor feature vectors"); _rows_end assembles D [n_anchors][total]
 *   from them (a host that skips the exchange gets them recomputed from the anchors, every row on every rank).
 *   annchor_stream_order_begin / _end then build the one global tile order, each rank ordering its own tile range.
 * Lists: annchor_stream_lists_all = the all-gather target for annchor_stream_knn_join.
 * Result: _route_begin replaces annchor_stream_knn_end: finished rows become records [global id, k-1 neighbour ids,
 *   k-1 float64 distances] (int64 words) grouped by owner rank (starts / bases: first position / first global row of
 *   every rank's shard); the host exchanges them with one all-to-all (send_counts -> receive counts) into the buffer of
 *   _route_recv; _route_end scatters them into this rank's own row order, keeps the graph rows on the device
 *   (annchor_stream_graph_device: int64 / float64 [rows_padded][k], padding rows (-1, inf) -- the source of a final
 *   graph all-gather) and downloads them (get_ann-shaped, annchor.py:514-530). */
int annchor_stream_hip_stream(annchor_ctx *ctx, void **stream);
int annchor_stream_anchor_begin(annchor_ctx *ctx, int32_t n_anchors, int64_t first_global, int32_t world, void **cand, void **gathered,
                                int64_t *cand_bytes);
int annchor_stream_anchor_step(annchor_ctx *ctx, const void *gathered, int32_t world, int32_t round);

/* ------------------------------------------------------------ in-library collectives (csrc/comm.hip)
 * RCCL called from inside the library, on the context's stream, so that the row-sharded build's rounds never return to
 * the host language: rank 0 makes a 128-byte id (annchor_comm_unique_id), the host hands it to every rank by whatever it
 * has (torch.distributed / MPI broadcast, a file), every rank calls annchor_comm_init on its context.  RCCL is loaded
 * with dlopen at first use (ANNCHOR_RCCL_LIB overrides the name); nothing here is touched by single-GPU use.
 *   annchor_comm_allgather          every rank's nbytes at send -> rank order at recv (device pointers)
 *   annchor_comm_alltoall_records   records of `words` 8-byte words grouped by destination -> source-rank order
 *   annchor_stream_anchor_rounds    ALL max-min rounds after annchor_stream_anchor_begin: per round the all-gather of the
 *                                   candidates, the winner's pick, the sweep (no communicator: one rank, no collective) */
int annchor_comm_unique_id(uint8_t *id128);
int annchor_comm_init(annchor_ctx *ctx, const uint8_t *id128, int32_t world, int32_t rank);
int annchor_comm_destroy(annchor_ctx *ctx);
/* Robustness of a multi-rank job (no reference counterpart: the reference has no collectives):
 *   annchor_comm_set_timeout   host waits of a context with a communicator run under a watchdog: one that lasts longer than
 *                              `seconds` (default 300; ANNCHOR_COMM_TIMEOUT_S; <= 0: off) aborts the communicators
 *                              (ncclCommAbort) and the call fails with "collective timed out" -- a dead peer no longer blocks
 *                              the other ranks for good
 *   annchor_comm_preflight     1 KB all-gather of (rank, position) bytes on every communicator of the context, checked, under
 *                              a timeout of its own: a mis-wired job fails here, loudly
 *   annchor_comm_init_side     a second communicator (its own 128-byte id) on a stream of its own
 *   annchor_comm_allgather_begin   ONE large all-gather beside the engine stream's work (the raw rows of the row-sharded
 *                              build beside the anchor rounds and the k-d order); the library waits for it where it first needs
 *                              the rows (annchor_stream_rows_end / _order_end); annchor_comm_side_join for other users */
int annchor_comm_set_timeout(annchor_ctx *ctx, double seconds);
int annchor_comm_preflight(annchor_ctx *ctx, double seconds);
int annchor_comm_init_side(annchor_ctx *ctx, const uint8_t *id128);
int annchor_comm_allgather_begin(annchor_ctx *ctx, const void *send, void *recv, int64_t nbytes);
int annchor_comm_side_join(annchor_ctx *ctx);
int annchor_comm_allgather(annchor_ctx *ctx, const void *send, void *recv, int64_t nbytes);
int annchor_comm_alltoall_records(annchor_ctx *ctx, const void *send, const int64_t *send_counts, void *recv,
                                  const int64_t *recv_counts, int32_t words);
int annchor_stream_anchor_rounds(annchor_ctx *ctx, int32_t n_anchors);
int annchor_stream_anchor_end(annchor_ctx *ctx, int64_t *A, float *anchor_vectors);
int annchor_stream_rows_begin(annchor_ctx *ctx, int32_t world, const int64_t *counts, void **send, void **recv, int64_t *bytes_per_rank);
int annchor_stream_anchor_dists_begin(annchor_ctx *ctx, int32_t world, const int64_t *counts, void **send, void **recv,
                                      int64_t *bytes_per_rank);
int annchor_stream_rows_end(annchor_ctx *ctx, int32_t world, const int64_t *counts);
int annchor_stream_lists_all(annchor_ctx *ctx, int32_t world, int64_t bytes_per_rank, void **all);
int annchor_stream_route_begin(annchor_ctx *ctx, int32_t world, const int64_t *starts, const int64_t *bases, void **send,
                               int64_t *send_counts, int64_t *record_words, int64_t *tile_evals);
int annchor_stream_route_recv(annchor_ctx *ctx, int64_t n_recv, void **recv);
int annchor_stream_route_end(annchor_ctx *ctx, int64_t n_recv, int64_t rows_padded, int64_t *ng_idx, double *ng_dist);
int annchor_stream_graph_device(annchor_ctx *ctx, void **idx, void **dist, int64_t *rows_padded, int32_t *k);
/* Raw device copies for hosts that stage the exchanges through host memory (process groups without device
 * collectives, e.g. gloo). */
int annchor_device_alloc(annchor_ctx *ctx, int64_t bytes, void **dptr);
int annchor_device_free(annchor_ctx *ctx, void *dptr);
int annchor_device_copy(annchor_ctx *ctx, void *dst, const void *src, int64_t bytes, int32_t kind /*1 H2D, 2 D2H, 3 D2D*/);

/* ------------------------------------------------------------- nearest enemies (f4)
 * Annchor.get_nearest_enemies (annchor/annchor.py:685-782; get_check with the label filter utils.py:454-491,
 * adjust_check utils.py:437-451, get_IJs_from_check utils.py:502-540) on a fitted pair list, in stages:
 *   annchor_enemies_candidates  y = dense label codes (HOST int32 [nx]): the enemy pairs sharing nearest anchors
 *     (per-point threshold among enemies, symmetrised when one was lowered) that fit() does not hold, as a sorted pair
 *     list + per-point index, with their bounds / dad / anchor flag; *n_new = their number;
 *   annchor_enemies_predict     their predicted distances, clipped to [lb, ub] (annchor.py:724-728): the fitted
 *     stratified regression (HOST bins / W / c), or -- pred != NULL -- a custom regression's host predictions;
 *   annchor_enemies_first       per point the `first` closest-looking enemies among its fitted + new entries; the
 *     not-computed ones are evaluated exactly (device metric: here; otherwise the pairs are returned in todo_ij and
 *     annchor_enemies_set_exact takes the values); RefineApprox / not_computed_mask are updated in place (:744-761);
 *   annchor_enemies_graph       the nn nearest computed enemies per point (:763-781): idx int64 [nx, nn] (the other
 *     endpoint), dist float64 [nx, nn].  Refused with ANNCHOR_ESTATE, before any launch, unless the last
 *     annchor_enemies_first on these candidates succeeded with an nn no smaller than this one: only that call checks
 *     that every point has more than nn entries to choose from.  annchor_enemies_candidates and a refused
 *     annchor_enemies_first forget what was checked;
 *   annchor_enemies_download   the new pairs for the host's views (the reference appends them to IJs, features,
 *     RefineApprox, not_computed_mask and I, :729-740).
 * Ties by list order (fitted entries by other endpoint, then new entries by other endpoint). */
int annchor_enemies_candidates(annchor_ctx *ctx, const int32_t *y, int32_t loc_thresh, int32_t loc_min, int64_t *n_new);
int annchor_enemies_predict(annchor_ctx *ctx, const double *bins, int32_t nbins, const double *W, const double *c, const double *pred);
int annchor_enemies_first(annchor_ctx *ctx, int32_t first, int32_t nn, int32_t evaluate, int64_t *todo_ij, int64_t cap, int64_t *n_todo);
int annchor_enemies_set_exact(annchor_ctx *ctx, const double *exact, int64_t n_todo);
int annchor_enemies_graph(annchor_ctx *ctx, int32_t nn, int64_t *idx, double *dist);
int annchor_enemies_download(annchor_ctx *ctx, int64_t *ij, double *feats, double *RA, uint8_t *ncm, int64_t *I_ptr, int64_t *I_idx);

/* Annchor.to_sparse_matrix (annchor/annchor.py:625-641): the symmetric sparse distance matrix of a
 * k-NN graph (HOST arrays ng_idx int64 [nx, k], ng_dist float64 [nx, k]) in COO form: every cell once,
 * value = distance + nextafter(0, 1), later assignments of the reference's loop order win.  rows /
 * cols / vals are HOST arrays with room for 2 * nx * k entries; *nnz entries are written. */
int annchor_graph_to_coo(annchor_ctx *ctx, const int64_t *ng_idx, const double *ng_dist, int64_t nx, int32_t k,
                         int64_t *rows, int64_t *cols, double *vals, int64_t *nnz);

/* DeviceStratifiedSampler (annchor_amd/samplers.py; protocol of annchor/samplers.py:75-110): the
 * stratified draw with an order-free random choice.  Partition b (bins[b] <= dad < bins[b+1], not
 * computed; counts[b] members, from annchor_bin_counts) keeps the min(want[b], counts[b]) members with
 * the smallest key = splitmix64(seed_key ^ position), ties to the smaller position.  positions (HOST,
 * room for sum of want): the samples, partition by partition, ascending position inside a partition. */
int annchor_hash_sample(annchor_ctx *ctx, const double *bins, int32_t nbins, const int64_t *counts, const int64_t *want,
                        uint64_t seed_key, int64_t *positions, int64_t *n_out);
/* The same choice followed by the samples' feature rows (annchor.py:325-338) and exact distances
 * (get_exact on the sampled pairs, annchor.py:340) in one call: feats float64 [m, 4], sample_y
 * float64 [m]; the sampled pairs become computed.  Device metric only. */
int annchor_hash_sample_pairs(annchor_ctx *ctx, const double *bins, int32_t nbins, const int64_t *counts, const int64_t *want,
                              uint64_t seed_key, int64_t *positions, double *feats, double *sample_y, int64_t *n_out);

/* ------------------------------------------------- fixed-radius graph (csrc/radius.hip; DESIGN.md, "Fixed-radius graphs")
 * Every pair i < j with d(i, j) <= r, exactly, from the anchor table (no reference counterpart: every result of the reference is
 * a k-NN list).  For a true metric lb = max_a |D[i,a] - D[j,a]| never exceeds d(i, j), so a pair with lb > r is outside the graph
 * without a metric call (LAESA-style pruning); every pair that is left is evaluated, and membership is decided on the computed
 * distance alone.  The classification rule, in float64 and written exactly so (the library is built with -ffp-contract=off;
 * a NumPy restatement gives the same classes bit for bit):
 *   s = D[i,a]   t = D[j,a]   m = (s + t) + r
 *   out(a): (fabs(s - t) - r) > rtol * m          in(a): (r - (s + t)) > rtol * m
 *   OUT  if any out(a);   else SURE if mode == 1 (connectivity) and any in(a);   else EVAL
 * A NaN (inf - inf) makes neither comparison true: the pair is evaluated.  rtol >= 0 is the relative margin that covers the
 * rounding of COMPUTED distances, for which the triangle inequality holds only approximately (0 for integer-valued metrics).
 * SURE (d <= s + t < r) is only taken in connectivity mode, where the distance itself is not wanted.
 *
 * annchor_radius_count: classifies all nx (nx - 1) / 2 pairs from the anchor table alone -- the pair list is never built -- and
 *   returns the per-row numbers of EVAL and SURE pairs (HOST int64 [nx] each; row i counts its pairs (i, j), j > i).  Remembers
 *   (r, rtol, mode, use_bounds) for the calls below.  use_bounds = 0: no anchor table is read and every pair is EVAL (the
 *   brute-force route through the same code).  Needs no metric: annchor_set_opaque + annchor_set_anchor_distances suffice.
 * annchor_radius_rows: the pairs (i, j) with row_begin <= i < row_end and max(i + 1, col_begin) <= j < col_end: their EVAL list
 *   and (mode 1) SURE list are written to buffers of the context as int32 pairs in row-major order, ascending j inside a row.
 *   Every output position comes from an exclusive scan of per-(row, 64-column chunk) counts: the order is a pure function of the
 *   input, no atomic decides a position.  *n_eval / *n_sure = their lengths.  max_pairs > 0 and *n_eval + *n_sure > max_pairs:
 *   nothing is emitted and *n_kept = -1 (the caller takes a smaller range; one row may be split by column range).  evaluate != 0
 *   (needs a device metric): the metric runs on the EVAL list and the pairs with d <= r (<=, not <; a NaN distance is dropped)
 *   are compacted in the same order with their distances; *n_kept = their number.  evaluate == 0: *n_kept = 0 and the EVAL list
 *   waits to be fetched (host-evaluated metrics).  (rows x ceil(columns / 64)) is at most 2^23 per call (ANNCHOR_ELIMIT).
 * annchor_radius_fetch: downloads a list of the last annchor_radius_rows: which = 0 the EVAL pairs (d, when not NULL and the
 *   range was evaluated: their distances), 1 the SURE pairs (d is not written), 2 the kept pairs and their distances.
 *   ij: HOST int64 [n][2]; d: HOST float64 [n].
 * None of these calls touches the pair list, RefineApprox, the masks or the graph of a fit on the same context. */
int annchor_radius_count(annchor_ctx *ctx, double r, double rtol, int32_t mode, int32_t use_bounds, int64_t *row_eval,
                         int64_t *row_sure);
int annchor_radius_rows(annchor_ctx *ctx, int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end, int64_t max_pairs,
                        int32_t evaluate, int64_t *n_eval, int64_t *n_sure, int64_t *n_kept);
int annchor_radius_fetch(annchor_ctx *ctx, int32_t which, int64_t *ij, double *d);

/* Fixed-radius queries for NEW points: every (q, j) with d(Q[q], X[j]) <= r, exactly.  The context holds nx_data data points
 * followed by nq = nx - nx_data queries (the layout of a query context: bind X followed by Q, annchor_set_anchor_distances with
 * the rows of both), so Dt is [na][nx_data + nq].  The rule, in float64 and written exactly so, for every query q, data point j
 * and anchor a:
 *   s = D[nx_data + q, a]   t = D[j, a]   m = (s + t) + r
 *   out(a): (fabs(s - t) - r) > rtol * m          in(a): (r - (s + t)) > rtol * m
 *   OUT  if any out(a);   else SURE if mode == 1 (connectivity) and any in(a);   else EVAL
 * -- the expressions of the rule above; a NaN makes neither comparison true.  Every (q, j) of the rectangle is a valid pair:
 * there is no i < j cut and no self-exclusion (a query equal to X[j] gets j at distance 0).
 *
 * annchor_radius_query_count: one pass over the nq x nx_data rectangle; returns the per-query numbers of EVAL and SURE pairs (HOST
 *   int64 [nq] each).  Validates as annchor_radius_count, and 1 <= nx_data < nx.  Remembers (r, rtol, mode, use_bounds, nx_data)
 *   for annchor_radius_query_rows; use_bounds = 0: no anchor table is read and every (q, j) is EVAL.
 * annchor_radius_query_rows: the queries q_begin <= q < q_end against the data columns col_begin <= j < col_end (inside
 *   0..nx_data): the same stages, limits (2^23 (query, 64-column chunk) entries, 2^31 - 1 candidates) and *n_kept = -1 over-cap
 *   answer as annchor_radius_rows.  The lists are query-major with ascending j inside a query, a pure function of the input (every
 *   position comes from the exclusive scan; the count form's atomics give integer sums, never positions), and hold the pairs
 *   as (j, nx_data + q): the data index first, both indices into the context's points, so the metric evaluates them as they are.
 * annchor_radius_fetch serves these lists as it serves those of annchor_radius_rows.  A count of either form invalidates the
 * other form's *_rows until its own count has run again. */
int annchor_radius_query_count(annchor_ctx *ctx, int64_t nx_data, double r, double rtol, int32_t mode, int32_t use_bounds,
                               int64_t *row_eval, int64_t *row_sure);
int annchor_radius_query_rows(annchor_ctx *ctx, int64_t nx_data, int64_t q_begin, int64_t q_end, int64_t col_begin, int64_t col_end,
                              int64_t max_pairs, int32_t evaluate, int64_t *n_eval, int64_t *n_sure, int64_t *n_kept);

/* ------------------------------------------------- DBSCAN on the fixed-radius graph (csrc/dbscan.hip)
 * One label per point from the edges {(i, j) : d(i, j) <= eps} alone, on the device (no reference counterpart).  The rule --
 * scikit-learn's DBSCAN made order-free:
 *   core(i)    iff degree(i) + 1 >= min_samples (the neighbourhood of i includes i)
 *   clusters   the connected components of the core-core edges, numbered 0, 1, ... by ascending smallest core index
 *   border     a non-core point with a core neighbour takes the smallest cluster number among its core neighbours
 *   noise      every other point: -1
 * The answer is a pure function of the edge SET: neither the order of the edges nor the scheduling of the threads changes a
 * label (degrees are integer sums, the union-find hangs the larger root under the smaller one, border labels are minima).
 *
 * annchor_dbscan_begin: zeroes the degrees and empties the edge list for the nx points of the context; min_samples >= 1.
 * annchor_dbscan_absorb: appends the kept and the SURE pairs of the last annchor_radius_rows call on this context to the edge
 *   list, device to device, and counts their end points' degrees; *n_edges = how many it took.  ANNCHOR_EINVAL when that range
 *   was not evaluated and holds candidates (their membership is unknown), when it was of the query form, or when it has been
 *   absorbed already.  A range answered with *n_kept = -1 emitted nothing: 0 edges.
 * annchor_dbscan_edges: the same for n edges from the HOST (int64 [n][2]): the route of host-evaluated metrics.  Every edge
 *   is validated before anything is uploaded: 0 <= i, j < nx and i != j.  Each unordered pair is passed once, in either
 *   orientation (a pair passed twice counts twice in both degrees).
 * annchor_dbscan_finish: core flags, union-find, numbering and border labels from the edge list as it stands; labels (HOST int32
 *   [nx]), core (HOST uint8 [nx]) and *n_clusters are downloaded.  May be called again after more edges were added: everything
 *   is computed anew from the list.
 * The edge list grows geometrically; ANNCHOR_ELIMIT when it cannot (more than 2^31 - 1 edges, or no device memory).  None of
 * these calls touches the pair list, RefineApprox, the masks or the graph of a fit on the same context. */
int annchor_dbscan_begin(annchor_ctx *ctx, int32_t min_samples);
int annchor_dbscan_absorb(annchor_ctx *ctx, int64_t *n_edges);
int annchor_dbscan_edges(annchor_ctx *ctx, const int64_t *ij, int64_t n);
int annchor_dbscan_finish(annchor_ctx *ctx, int32_t *labels, uint8_t *core, int64_t *n_clusters);

/* ------------------------------------------------- exact k-NN graph from the anchor bounds (csrc/knnexact.hip)
 * annchor_brute_force's answer -- identical indices, bit-equal distances -- without evaluating every pair (no reference
 * counterpart).  The fixed-radius rule above with one radius per row instead of one for all.  k counts the point itself, as in
 * annchor_brute_force: the exact row of i is the k smallest of {(d(i, j), j)} over all j, with d(i, i) = 0, ordered by distance,
 * then index (a duplicate of i with a lower index precedes i).
 *   radii     u[i] >= 0 is ANY upper bound of row i's true k-th distance; +inf: unknown.  A guess of k neighbours per row supplies
 *             it: the largest exact distance among the row's distinct entries != i, when there are at least k - 1 of them -- with
 *             i itself these are k distinct points within u[i].
 *   classify  a pair i < j, R = max(u[i], u[j]); for every anchor a, s = D[i,a], t = D[j,a], in float64 and written exactly so
 *             (-ffp-contract=off):  out(a): (fabs(s - t) - R) > rtol * ((s + t) + R)
 *             OUT if any out(a), else EVAL; there is no SURE class.  R = +inf never fires (-inf > +inf is false, and so is
 *             -inf > NaN at rtol = 0); neither does a NaN in the anchor table.
 *   absorb    an evaluated pair with distance d becomes the directed entry (i -> j, d) if d <= u[i], and (j -> i, d) if d <= u[j]
 *             (<=, not <; a NaN distance passes neither test).
 *   finish    row i = the k smallest of its entries plus (0.0, i), by (ann_key_asc(d), index), written in that order.
 * Why it is exact: the pairs an anchor excludes have d(i, j) > max(u[i], u[j]), beyond both rows' k-th distance, and an entry
 * dropped by a directed test lies beyond that row's; what is left of row i holds every point within u[i], so at least k.  A
 * poor u costs evaluations, never correctness.  The result is a pure function of the entry set: a walk classifies every
 * unordered pair in exactly one range, so no entry repeats, and (key, index) is a total order on a row's entries.
 *
 * annchor_knn_exact_begin: uploads u (HOST float64 [nx]; every u[i] >= 0, +inf allowed, NaN refused), empties the entry list and
 *   returns the per-row numbers of EVAL pairs over all pairs (HOST int64 [nx]; row i counts its pairs (i, j), j > i).  1 <= k <=
 *   nx and k <= 8533 (annchor_brute_force's bound).  use_bounds = 0: no anchor table is read and every pair is EVAL.  The walk
 *   reuses the fixed-radius stages' table and list buffers: what annchor_radius_count fixed is forgotten (annchor_radius_rows,
 *   annchor_radius_fetch and annchor_dbscan_absorb are refused until a count has run again).
 * annchor_knn_exact_rows: the pairs (i, j) with row_begin <= i < row_end and max(i + 1, col_begin) <= j < col_end: classify, scan,
 *   emit -- annchor_radius_rows' stages, order and limits; *n_eval = the length of the EVAL list.  max_pairs > 0 and *n_eval >
 *   max_pairs: nothing is emitted and *n_entries = -1 (the caller takes a smaller range; one row may be split by column range).
 *   evaluate != 0 (needs a device metric): the metric runs on the list and the pairs are absorbed; *n_entries = the entries
 *   added.  evaluate == 0: *n_entries = 0 and the list waits to be fetched.  Every unordered pair must be covered by exactly
 *   one absorbed range.
 * annchor_knn_exact_fetch: the EVAL list of the last annchor_knn_exact_rows (HOST int64 [n_eval][2]).
 * annchor_knn_exact_edges: absorbs n host-evaluated candidates (HOST int64 [n][2], float64 [n]) under the same directed tests:
 *   the route of host metrics.  Every pair is validated before anything is uploaded (0 <= i, j < nx, i != j); either
 *   orientation; each unordered pair once.
 * annchor_knn_exact_finish: idx (HOST int64 [nx][k]) and dist (HOST float64 [nx][k]); row_entries (HOST int64 [nx], or NULL): the
 *   entries every row held, the diagonal not counted.  ANNCHOR_ESTATE when a row holds fewer than k - 1 (a u[i] was no upper
 *   bound, or a range was never absorbed), ANNCHOR_EINVAL while an emitted range waits for annchor_knn_exact_edges.  row_cap: 0,
 *   or the number of row slots the selection may keep in LDS (longer rows are re-read from memory on every pass; a test knob:
 *   the result does not depend on it).  May be called again: everything is computed anew from the entry list.
 * The entry list grows geometrically and has room for two entries per candidate of a range; ANNCHOR_ELIMIT when it cannot grow
 * (more than 2^31 - 1 entries, or no device memory).  None of these calls touches the pair list, RefineApprox, the masks or
 * the graph of a fit on the same context. */
int annchor_knn_exact_begin(annchor_ctx *ctx, int32_t k, const double *u, double rtol, int32_t use_bounds, int64_t *row_eval);
int annchor_knn_exact_rows(annchor_ctx *ctx, int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end, int64_t max_pairs,
                           int32_t evaluate, int64_t *n_eval, int64_t *n_entries);
int annchor_knn_exact_fetch(annchor_ctx *ctx, int64_t *ij);
int annchor_knn_exact_edges(annchor_ctx *ctx, const int64_t *ij, const double *d, int64_t n);
int annchor_knn_exact_finish(annchor_ctx *ctx, int64_t *idx, double *dist, int64_t *row_entries, int32_t row_cap);

/* -------------------------------------------------------------- state access */
int annchor_field_size(annchor_ctx *ctx, int32_t field, int64_t *n_elems);
int annchor_download(annchor_ctx *ctx, int32_t field, void *dst, int64_t n_elems);
int annchor_upload(annchor_ctx *ctx, int32_t field, const void *src, int64_t n_elems);

/* ------------------------------------------------------------------ profiling
 * Per-kernel-family accumulated device time since the last reset (HIP events on
 * the stream): names[i] is a static string; returns the number of entries.
 * on: 0 = off, 1 = every kernel family, 2 = the metric kernels only ("*_pairs"; cheap enough
 * to leave on inside a timed region). */
int annchor_prof_enable(annchor_ctx *ctx, int32_t on);
int annchor_prof_reset(annchor_ctx *ctx);
int annchor_prof_get(annchor_ctx *ctx, int32_t max_entries, const char **names, double *ms,
                     int64_t *launches, double *alg_bytes);

#ifdef __cplusplus
}
#endif
#endif /* ANNCHOR_HIP_H */
