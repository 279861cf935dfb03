// model.hip -- the per-iteration models of Annchor.fit() fitted ON THE DEVICE, so that an iteration runs from the
// sampling step to the candidate selection without a host round trip:
//   annchor_fit_regression_device  SimpleStratifiedLinearRegression.fit (annchor/regressors.py:39-69) -- per partition
//                                  (lo < dad <= hi) ordinary least squares with intercept on [lb, ub, dad] -> y -- followed
//                                  by the fused predict / clip / merge / label pass (regressors.py:71-103,
//                                  annchor.py:356-380) from the coefficients where they are;
//   annchor_fit_errors_device      SimpleStratifiedErrorRegression.fit (annchor/error_predictors.py:26-53): per partition
//                                  (lo <= dad <= hi, both sides closed) the sorted residuals y - prediction.
// The reference solves each partition with LAPACK's SVD-based dgelsd on the centred samples (sklearn LinearRegression ->
// scipy.linalg.lstsq); here a partition is one workgroup running Householder QR on the same centred matrix in float64
// (backward stable: coefficients agree with dgelsd to ~cond * eps, 1e-13 relative on the bundled data -- tested at 1e-11;
// NOT bit-equal, which no two LAPACK builds are either).  Deterministic: rows are compacted in sample order and every
// reduction runs over a fixed tree, so two runs give the same bits.  A partition that is (numerically) rank deficient is
// solved ON THE DEVICE too: the minimum-norm solution dgelsd returns there, from a one-sided Jacobi SVD of the 3 x 3 factor R
// (singular values below OLS_RCOND of the largest dropped; every feature constant: w = 0, the intercept alone) -- status 0, no
// flag.  Only a partition with fewer than three rows (status 2), or an SVD that does not converge (status 1), raises
// dev_flags[1], and the host then redoes the step with dgelsd.  Tested kernel by kernel on constructed partitions against an
// exact solve in tests/test_model_kernels_gpu.py, and bit for bit against a recorded build in tests/test_model_kernels_bits_gpu.py
// (both kernels are latency chains over ~200 KB: their layout serves barrier and round-trip counts).
#include "common.h"
#include <atomic>

#define OLS_T 256
#define OLS_PER 8                     // samples a thread brings per compaction trip
#define OLS_TRIP (OLS_T * OLS_PER)    // samples per compaction trip: one barrier each
#define OLS_LDS_ROWS 4096             // a partition of up to this many rows is factored in LDS (32 bytes a row: 128 KiB)
#define ERR_CAP 8192   // residuals per partition the LDS sorter takes
#define ERR_T 1024
#define ERR_PER 8                     // samples a thread brings per trip of k_err_sort
#define ERR_TRIP (ERR_T * ERR_PER)

int ann_dev_flags(annchor_ctx *c)
{
    ANN_TRY(ann_reserve(c, c->dev_flags, sizeof(int32_t) * 16));
    if (!c->dev_flags_clean) {
        ANN_CHECK_HIP(c, hipMemsetAsync(c->dev_flags.p, 0, sizeof(int32_t) * 16, c->stream));
        c->dev_flags_clean = true;
    }
    return ANNCHOR_OK;
}

// The dynamic LDS a kernel may ask for (hipFuncAttributeMaxDynamicSharedMemorySize), set once per process and device instead of
// on every launch.  which: 0 k_ols_bins, 1 k_err_sort.
static int ann_lds_once(annchor_ctx *c, const void *fn, int which, size_t bytes)
{
    static std::atomic<bool> done[2][64];
    const int d = c->device;
    const bool memo = d >= 0 && d < 64;
    if (memo && done[which][d].load(std::memory_order_acquire)) return ANNCHOR_OK;
    ANN_CHECK_HIP(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    if (memo) done[which][d].store(true, std::memory_order_release);
    return ANNCHOR_OK;
}

// Fixed-tree block sums (the same association for the same block size, whatever the data) of NV values behind ONE barrier:
// per value the xor-shuffle tree 32 .. 1, then the four waves' sums left to right.  sh alternates between two buffers (par),
// so that a wave which runs ahead into the next call writes the other one; the barrier of that call frees this one.
template <int NV> __device__ __forceinline__ void block_sums(double (&v)[NV], double (*sh)[4][OLS_T / 64], int &par)
{
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) sh[par][k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        double s = sh[par][k][0];
#pragma unroll
        for (int w = 1; w < OLS_T / 64; ++w) s += sh[par][k][w];
        v[k] = s;
    }
    par ^= 1;
}

#define OLS_RCOND 1e-13   // relative singular value below which a direction of a rank-deficient partition is dropped
struct ModelEdges { double e[MAXBINS + 1]; };
struct OlsFactor { double mean[4], Rd[3], R01, R02, R12, qy[3], cmax; };

// Centring and Householder QR of the n x 4 matrix [X | y] at A (column k at A + k * cap; LDS or global: inlined per caller, so
// that the compiler knows which).  Thread tid owns rows j + tid + OLS_T i of step j and sums them in increasing i; every
// reduced value goes through block_sums' tree.  What is independent is reduced and applied together -- the four means; sigma_0
// with the centring (same owner, same order); the dots of a step's later columns, and their updates -- which changes no
// operand and no order of any sum.  v_0 = a_jj - alpha of a step is read by the owner of row j (thread 0) alone: it stays in
// a register instead of going through the matrix behind two barriers.
__device__ __forceinline__ void ols_factor(double *A, const size_t cap, const int n, double (*sh)[4][OLS_T / 64], int &par, OlsFactor &f)
{
    const int tid = threadIdx.x;
    double *col[4] = {A, A + cap, A + 2 * cap, A + 3 * cap};
    // ---- centre (sklearn LinearRegression(fit_intercept=True))
    double s4[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = tid; r < n; r += OLS_T) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s4[k] += col[k][r];
    }
    block_sums<4>(s4, sh, par);
#pragma unroll
    for (int k = 0; k < 4; ++k) f.mean[k] = s4[k] / (double)n;
    double sg[1] = {0.0};
    for (int r = tid; r < n; r += OLS_T) {
        const double x0 = col[0][r] - f.mean[0];
        col[0][r] = x0;
        sg[0] += x0 * x0;
#pragma unroll
        for (int k = 1; k < 4; ++k) col[k][r] -= f.mean[k];
    }
    // ---- Householder QR of [Xc | yc]: after step j column j is (.., R_jj, 0, ..) and rows j.. of the later columns hold Q^T
    f.R01 = f.R02 = f.R12 = 0.0;
    f.cmax = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (j > 0) {
            sg[0] = 0.0;
            for (int r = j + tid; r < n; r += OLS_T) sg[0] += col[j][r] * col[j][r];
        }
        block_sums<1>(sg, sh, par);   // (its barrier also publishes the centred rows to the readers of a_00)
        const double sigma = sg[0];
        const double ajj = col[j][j];
        const double alpha = ajj > 0.0 ? -sqrt(sigma) : sqrt(sigma);
        f.Rd[j] = alpha;
        f.cmax = fmax(f.cmax, fabs(alpha));
        // v = x; v[0] -= alpha; v^T v = sigma - 2 alpha a_jj + alpha^2 = 2 (sigma - alpha a_jj)
        const double vtv = 2.0 * (sigma - alpha * ajj);
        const double v0 = ajj - alpha;
        double dot[3] = {0.0, 0.0, 0.0};
        for (int r = j + tid; r < n; r += OLS_T) {
            const double vj = r == j ? v0 : col[j][r];
#pragma unroll
            for (int k = j + 1; k < 4; ++k) dot[k - 1] += vj * col[k][r];
        }
        block_sums<3>(dot, sh, par);
        double tau[3];
#pragma unroll
        for (int k = j + 1; k < 4; ++k) tau[k - 1] = vtv > 0.0 ? 2.0 * dot[k - 1] / vtv : 0.0;
        for (int r = j + tid; r < n; r += OLS_T) {
            const double vj = r == j ? v0 : col[j][r];
#pragma unroll
            for (int k = j + 1; k < 4; ++k) col[k][r] -= tau[k - 1] * vj;
        }
        __syncthreads();   // (the next step's owners are other threads)
        if (j == 0) { f.R01 = col[1][0]; f.R02 = col[2][0]; }
        if (j == 1) f.R12 = col[2][1];
        f.qy[j] = col[3][j];
    }
}

// One workgroup per partition.  The partition's rows (columns lb, ub, dad, y) are compacted in sample order into dynamic LDS,
// double [4][lrows] with lrows = min(m, OLS_LDS_ROWS), and factored there; the rows past lrows of a longer partition go to its
// global scratch, double [4][cap], the LDS part follows them, and the same code factors it in global memory.
// (the model's header -- edges, partition count, statuses -- is written here too: workgroup 0 for the shared part, every
// workgroup for its own partition; k_model_init used to be a launch of its own in front)
__global__ __launch_bounds__(OLS_T) void k_ols_bins(const double *__restrict__ sfeat, const double *__restrict__ sy, int64_t m,
                                                   DeviceModel *__restrict__ dm, double *__restrict__ scratch, int64_t cap,
                                                   int32_t *__restrict__ flags, ModelEdges ed, int nb, int lrows)
{
    extern __shared__ double ols_lds[];   // [4][lrows]
    __shared__ double sh[2][4][OLS_T / 64];
    __shared__ int wcnt[2][OLS_PER][OLS_T / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double lo = ed.e[b], hi = ed.e[b + 1];
    if (tid == 0) dm->status[b] = 0;
    if (b == 0) {
        if (tid >= nb && tid < MAXBINS) { dm->status[tid] = 0; dm->rows[tid] = 0; }
        if (tid <= nb) dm->reg.e[tid] = ed.e[tid];
        if (tid == 0) { dm->reg.nb = nb; dm->err_status = 0; }
    }
    double *G = scratch + (size_t)b * 4 * cap;
    // ---- rows of the partition, compacted in sample order (deterministic): OLS_TRIP samples per trip, every load of a trip in
    // flight at once, the trip's OLS_PER x 4 ballot counts through LDS behind one barrier (two buffers in turn), the running
    // base in a register of every thread
    const double2 *__restrict__ sf2 = reinterpret_cast<const double2 *>(sfeat);
    const unsigned long long below = (1ull << lane) - 1ull;
    int base = 0, wp = 0;
    for (int64_t t0 = 0; t0 < m; t0 += OLS_TRIP) {
        double2 fa[OLS_PER], fb[OLS_PER];
        double yv[OLS_PER];
        unsigned long long bal[OLS_PER];
#pragma unroll
        for (int i = 0; i < OLS_PER; ++i) {
            const int64_t t = t0 + i * OLS_T + tid, tc = t < m ? t : m - 1;
            fa[i] = sf2[2 * tc]; fb[i] = sf2[2 * tc + 1]; yv[i] = sy[tc];
        }
#pragma unroll
        for (int i = 0; i < OLS_PER; ++i) {
            const int64_t t = t0 + i * OLS_T + tid;
            bal[i] = __ballot(t < m && fb[i].x > lo && fb[i].x <= hi);
            if (lane == 0) wcnt[wp][i][wave] = __popcll(bal[i]);
        }
        __syncthreads();
        int run = base;
#pragma unroll
        for (int i = 0; i < OLS_PER; ++i) {
            int off = 0;
#pragma unroll
            for (int w = 0; w < OLS_T / 64; ++w) {
                if (w == wave) off = run;
                run += wcnt[wp][i][w];
            }
            if ((bal[i] >> lane) & 1ull) {
                const int r = off + __popcll(bal[i] & below);
                if (r < lrows) {
                    ols_lds[r] = fa[i].x; ols_lds[lrows + r] = fa[i].y; ols_lds[2 * lrows + r] = fb[i].x; ols_lds[3 * lrows + r] = yv[i];
                } else {
                    G[r] = fa[i].x; G[cap + r] = fa[i].y; G[2 * cap + r] = fb[i].x; G[3 * cap + r] = yv[i];
                }
            }
        }
        base = run;
        wp ^= 1;
    }
    const int n = base;
    if (tid == 0) dm->rows[b] = n;
    if (n < 3) {   // fewer rows than columns: the host decides (dgelsd's minimum-norm solution / the reference's error)
        if (tid == 0) {
            dm->status[b] = 2; dm->reg.w[b][0] = dm->reg.w[b][1] = dm->reg.w[b][2] = 0.0; dm->reg.c[b] = 0.0;
            atomicMax(&flags[1], 2);   // (sticky: a partition the device solver does not take)
        }
        return;
    }
    __syncthreads();
    OlsFactor f;
    int par = 0;
    if (n <= lrows) ols_factor(ols_lds, (size_t)lrows, n, sh, par, f);
    else {
        for (int r = tid; r < lrows; r += OLS_T) {
#pragma unroll
            for (int k = 0; k < 4; ++k) G[(size_t)k * cap + r] = ols_lds[k * lrows + r];
        }
        __syncthreads();
        ols_factor(G, (size_t)cap, n, sh, par, f);
    }
    const double *mean = f.mean, *Rd = f.Rd, *qy = f.qy;
    const double R01 = f.R01, R02 = f.R02, R12 = f.R12, cmax = f.cmax;
    if (tid == 0) {
        // numerically rank deficient (a constant or collinear feature inside the partition): leave it to dgelsd
        const double tol = 1e-10 * cmax;
        int st = 0;
        for (int j = 0; j < 3; ++j)
            if (!(fabs(Rd[j]) > tol)) st = 1;
        double w2 = 0, w1 = 0, w0 = 0;
        if (!st) {
            w2 = qy[2] / Rd[2];
            w1 = (qy[1] - R12 * w2) / Rd[1];
            w0 = ((qy[0] - R01 * w1) - R02 * w2) / Rd[0];
        } else {
            // Rank deficient inside the partition -- typically EXACT: among the closest pairs of Euclidean data both points
            // share their nearest anchor a*, which also gives the tightest upper bound, so ub = D[a*][i] + D[a*][j] = 2 dad
            // bit for bit.  What scipy's lstsq (dgelsd) returns there is the minimum-norm solution: the singular value
            // decomposition of the 3 x 3 factor R by one-sided Jacobi rotations, singular values below OLS_RCOND of the largest
            // dropped.  (dgelsd drops below machine epsilon; an exactly dependent column arrives at ~1e-16 of the largest in
            // either code, on one side or the other of that line by rounding luck, and when it lands above, the reference's
            // coefficients are ~1e15 and its predictions whatever the clip to [lb, ub] leaves.  The wider margin takes the
            // dependency for what it is.)  Restarting the whole fit with the host solver, as round 3 first did, doubled the
            // fit time of every Euclidean data set of this kind.
            double M[3][3] = {{Rd[0], R01, R02}, {0.0, Rd[1], R12}, {0.0, 0.0, Rd[2]}};
            double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
            bool conv = false;
            for (int sweep = 0; sweep < 40 && !conv; ++sweep) {
                conv = true;
                for (int p = 0; p < 2; ++p)
                    for (int q = p + 1; q < 3; ++q) {
                        double al = 0, be = 0, ga = 0;
                        for (int r = 0; r < 3; ++r) { al += M[r][p] * M[r][p]; be += M[r][q] * M[r][q]; ga += M[r][p] * M[r][q]; }
                        // (a column 1e-20 of the other is dropped by OLS_RCOND whatever it is orthogonal to; rotating against
                        // it would chase denormals)
                        if (ga == 0.0 || al <= 1e-40 * be || be <= 1e-40 * al || fabs(ga) <= 4.5e-16 * sqrt(al * be)) continue;
                        conv = false;
                        const double zeta = (be - al) / (2.0 * ga);
                        const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                        const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
                        for (int r = 0; r < 3; ++r) {
                            const double mp = M[r][p], mq = M[r][q];
                            M[r][p] = cs * mp - sn * mq; M[r][q] = sn * mp + cs * mq;
                            const double vp = V[r][p], vq = V[r][q];
                            V[r][p] = cs * vp - sn * vq; V[r][q] = sn * vp + cs * vq;
                        }
                    }
            }
            double sg2[3], smax2 = 0.0;
            for (int i = 0; i < 3; ++i) {
                sg2[i] = (M[0][i] * M[0][i] + M[1][i] * M[1][i]) + M[2][i] * M[2][i];
                smax2 = fmax(smax2, sg2[i]);
            }
            if (conv && smax2 > 0.0) {
                double w[3] = {0, 0, 0};
                for (int i = 0; i < 3; ++i)
                    if (sg2[i] > (OLS_RCOND * OLS_RCOND) * smax2) {
                        const double coef = ((M[0][i] * qy[0] + M[1][i] * qy[1]) + M[2][i] * qy[2]) / sg2[i];
                        for (int r = 0; r < 3; ++r) w[r] += coef * V[r][i];
                    }
                w0 = w[0]; w1 = w[1]; w2 = w[2];
                st = 0;
            } else if (smax2 == 0.0) st = 0;   // every feature constant inside the partition: the intercept alone (w = 0)
        }
        dm->status[b] = st;
        if (st) atomicMax(&flags[1], st);
        dm->reg.w[b][0] = w0; dm->reg.w[b][1] = w1; dm->reg.w[b][2] = w2;
        dm->reg.c[b] = mean[3] - ((mean[0] * w0 + mean[1] * w1) + mean[2] * w2);
    }
}

// bins: the partition edges (HOST, float64 [nb + 1]); the samples are the ones annchor_sample_pairs_device left on the
// device.  Enqueues the fit and the fused predict / clip / merge / label pass; no host wait.  A partition the device
// solver does not take (status != 0) raises dev_flags[1]; the caller reads it with annchor_model_status.
extern "C" int annchor_fit_regression_device(annchor_ctx *c, const double *bins, int32_t nb, int32_t first_iteration, int32_t is_metric)
{
    if (!c || !bins) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, c->have_features, ANNCHOR_EINVAL, "features not computed");
    ANN_REQUIRE(c, nb >= 1 && nb <= MAXBINS, ANNCHOR_ELIMIT, "1..%d partitions supported", MAXBINS);
    ANN_REQUIRE(c, first_iteration || c->have_RA, ANNCHOR_EINVAL, "RefineApprox not initialised");
    ANN_REQUIRE(c, c->nsamp > 0 && c->sfeat.p && c->sy.p, ANNCHOR_ESTATE, "no device-resident sample (annchor_sample_pairs_device)");
    // (annchor_set_samples, annchor_sample_pairs, annchor_hash_sample_pairs and annchor_evaluate_samples replace the sample but hand
    // its feature rows to the host: sfeat would be an earlier sample's, and shorter than nsamp rows if that one was smaller)
    ANN_REQUIRE(c, c->sfeat_rows == c->nsamp, ANNCHOR_ESTATE,
                "the current sample of %lld pairs has no device-resident feature rows (%lld rows from an earlier annchor_sample_pairs_device)",
                (long long)c->nsamp, (long long)c->sfeat_rows);
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    const int64_t m = c->nsamp;
    ANN_TRY(ann_reserve(c, c->model, sizeof(DeviceModel)));
    ANN_TRY(ann_reserve(c, c->ols_scratch, sizeof(double) * 4 * (size_t)m * (size_t)nb));
    ANN_TRY(ann_dev_flags(c));
    DeviceModel *dm = c->model.as<DeviceModel>();
    ModelEdges ed;
    for (int k = 0; k <= MAXBINS; ++k) ed.e[k] = k <= nb ? bins[k] : 0.0;
    static_assert(MAXBINS + 1 <= OLS_T, "one thread per edge");
    const int lrows = (int)std::min<int64_t>(m, OLS_LDS_ROWS);
    ANN_TRY(ann_lds_once(c, (const void *)k_ols_bins, 0, sizeof(double) * 4 * OLS_LDS_ROWS));
    {
        ProfScope ps(c, "ols_partitions", (double)m * 40.0 * nb);
        k_ols_bins<<<nb, OLS_T, sizeof(double) * 4 * (size_t)lrows, c->stream>>>(c->sfeat.as<double>(), c->sy.as<double>(), m, dm,
                                                                              c->ols_scratch.as<double>(), m, c->dev_flags.as<int32_t>(),
                                                                              ed, nb, lrows);
    }
    ANN_CHECK_HIP(c, hipGetLastError());
    c->model_fitted = true; c->model_nb = nb; c->errs_on_device = false; c->model_cache_valid = false;
    return ann_predict_merge_device(c, &dm->reg, first_iteration, is_metric);
}

// ---- residual lists: one workgroup per partition counts, compacts and sorts
// ascending order-preserving key of a double (NaNs last)
__device__ __forceinline__ unsigned long long err_key(double v) { return ann_key_asc(v); }

// Bitonic sort of the n keys at buf[0 .. n) (padded with ~0 to P2, a power of two) and the sorted residuals to out.  The keys
// live in registers: key e = s * ERR_T + tid is slot s of thread tid, so a stride below 64 is a shuffle inside the wave, a
// stride of ERR_T and above pairs two slots of one thread, and only the strides 64 .. 512 go through LDS -- buf's two halves
// [2][ERR_CAP] in turn, one barrier per stride (10 at P2 = 1024 where a barrier per stage made 55; 22 for 91 at 8192).
template <int E> __device__ __forceinline__ void err_sort_store(unsigned long long *buf, const int n, const int P2, double *__restrict__ out)
{
    const int tid = threadIdx.x;
    unsigned long long r[E];
#pragma unroll
    for (int s = 0; s < E; ++s) r[s] = s * ERR_T + tid < n ? buf[s * ERR_T + tid] : ~0ull;
    int p = 1;   // (the first exchange writes the half the compacted keys are NOT in: a slow wave may still be reading them)
    for (int k = 2; k <= P2; k <<= 1) {
#pragma unroll
        for (int js = E / 2; js >= 1; js >>= 1) {
            if (js * ERR_T < k) {
#pragma unroll
                for (int s = 0; s < E; ++s)
                    if ((s & js) == 0) {
                        const bool up = ((s * ERR_T + tid) & k) == 0;
                        const unsigned long long a = r[s], bb = r[s | js];
                        if ((a > bb) == up) { r[s] = bb; r[s | js] = a; }
                    }
            }
        }
        for (int j = min(k >> 1, ERR_T / 2); j >= 64; j >>= 1) {
            unsigned long long *w = buf + p * ERR_CAP;
#pragma unroll
            for (int s = 0; s < E; ++s) w[s * ERR_T + tid] = r[s];
            __syncthreads();
#pragma unroll
            for (int s = 0; s < E; ++s) {
                const int e = s * ERR_T + tid;
                const unsigned long long o = w[e ^ j];
                const bool take_min = ((e & j) == 0) == ((e & k) == 0);
                r[s] = take_min ? (o < r[s] ? o : r[s]) : (o > r[s] ? o : r[s]);
            }
            p ^= 1;
        }
        for (int j = min(k >> 1, 32); j >= 1; j >>= 1) {
#pragma unroll
            for (int s = 0; s < E; ++s) {
                const int e = s * ERR_T + tid;
                const unsigned long long o = __shfl_xor(r[s], j);
                const bool take_min = ((e & j) == 0) == ((e & k) == 0);
                r[s] = take_min ? (o < r[s] ? o : r[s]) : (o > r[s] ? o : r[s]);
            }
        }
    }
#pragma unroll
    for (int s = 0; s < E; ++s)
        if (s * ERR_T + tid < n) out[s * ERR_T + tid] = ann_key_asc_inv(r[s]);
}

__global__ __launch_bounds__(ERR_T) void k_err_sort(const double *__restrict__ sfeat, const double *__restrict__ sy,
                                                    const double *__restrict__ spred, int64_t m, DeviceModel *__restrict__ dm,
                                                    double *__restrict__ errs, int nb, int32_t *__restrict__ flags,
                                                    int64_t *__restrict__ errptr_out)
{
    extern __shared__ unsigned long long keys[];   // [2][ERR_CAP]
    __shared__ int wtot[2][ERR_T / 64];
    __shared__ int pcw[ERR_T / 64][MAXBINS];
    __shared__ int pcnt[MAXBINS];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the edges, read once: lane q holds partition q's, this workgroup's own are uniform
    const double elo = dm->reg.e[lane < nb ? lane : 0], ehi = dm->reg.e[lane < nb ? lane + 1 : 0];
    const double lo = dm->reg.e[b], hi = dm->reg.e[b + 1];
    const unsigned long long below = (1ull << lane) - 1ull;
    // One pass over the samples, ERR_TRIP per trip with every load of the trip in flight at once.  Every partition's population
    // (closed intervals: a sample on an inner edge counts for both neighbours) is counted by every workgroup for itself, by
    // ballots: lane q of a wave keeps the wave's count of partition q, the 16 waves' counts are added once at the end.  This
    // partition's members go to keys[0 ..) in the same trip, wave after wave (the order in the unsorted buffer is free), the
    // waves' totals of a trip through LDS behind one barrier (two buffers in turn).
    int mycnt = 0, base = 0, wp = 0;
    for (int64_t t0 = 0; t0 < m; t0 += ERR_TRIP) {
        double d[ERR_PER], res[ERR_PER];
        unsigned long long bal[ERR_PER];
#pragma unroll
        for (int i = 0; i < ERR_PER; ++i) {
            const int64_t t = t0 + i * ERR_T + tid, tc = t < m ? t : m - 1;
            d[i] = sfeat[4 * tc + 2];
            res[i] = sy[tc] - spred[tc];
            if (t >= m) d[i] = __longlong_as_double(-1ll);   // (a NaN: inside no interval)
        }
        int wsum = 0;
#pragma unroll
        for (int i = 0; i < ERR_PER; ++i) {
            bal[i] = __ballot(d[i] >= lo && d[i] <= hi);
            wsum += __popcll(bal[i]);
        }
        if (lane == 0) wtot[wp][wave] = wsum;
        for (int q = 0; q < nb; ++q) {
            const double ql = __shfl(elo, q), qh = __shfl(ehi, q);
            int cq = 0;
#pragma unroll
            for (int i = 0; i < ERR_PER; ++i) cq += __popcll(__ballot(d[i] >= ql && d[i] <= qh));
            if (lane == q) mycnt += cq;
        }
        __syncthreads();
        int off = base, tot = 0;
#pragma unroll
        for (int w = 0; w < ERR_T / 64; ++w) {
            const int x = wtot[wp][w];
            if (w < wave) off += x;
            tot += x;
        }
#pragma unroll
        for (int i = 0; i < ERR_PER; ++i) {
            if ((bal[i] >> lane) & 1ull) {
                const int at = off + __popcll(bal[i] & below);
                if (at < ERR_CAP) keys[at] = err_key(res[i]);
            }
            off += __popcll(bal[i]);
        }
        base += tot;
        wp ^= 1;
    }
    pcw[wave][lane] = mycnt;
    __syncthreads();
    if (tid < MAXBINS) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < ERR_T / 64; ++w) s += pcw[w][tid];
        pcnt[tid] = s;
    }
    __syncthreads();
    const int n = pcnt[b];
    if (tid == 0) dm->rows[b] = n;   // (rows is reused: the regression is done with it)
    // where this partition's list starts: the counts of the partitions before it; partition 0's workgroup also publishes the
    // offsets and the status (what a launch of its own, k_err_ptr, used to do)
    int64_t my_at = 0;
    for (int q = 0; q < b; ++q) my_at += pcnt[q];
    if (b == 0 && tid == 0) {
        int64_t at = 0;
        int st = 0;
        for (int q = 0; q < nb; ++q) {
            dm->errptr[q] = at;
            errptr_out[q] = at;
            const int64_t r = pcnt[q];
            if (r == 0) st = max(st, 1);
            if (r > ERR_CAP) st = max(st, 2);
            at += r;
        }
        dm->errptr[nb] = at;
        errptr_out[nb] = at;
        dm->err_status = st;
        if (st) flags[2] = st;
    }
    if (n == 0 || n > ERR_CAP) return;
    int P2 = 1;
    while (P2 < n) P2 <<= 1;
    double *out = errs + my_at;
    if (P2 <= ERR_T) err_sort_store<1>(keys, n, P2, out);
    else if (P2 == 2 * ERR_T) err_sort_store<2>(keys, n, P2, out);
    else if (P2 == 4 * ERR_T) err_sort_store<4>(keys, n, P2, out);
    else err_sort_store<8>(keys, n, P2, out);
}

// After annchor_fit_regression_device: the residual lists of the same samples / partition edges, sorted, into the
// context's `errs` / `errptr` (what annchor_select_candidates reads when it is handed errs == NULL).  No host wait; an
// empty partition or one longer than the sorter takes raises dev_flags[2].
extern "C" int annchor_fit_errors_device(annchor_ctx *c)
{
    if (!c) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, c->model_fitted && c->nsamp > 0 && c->spred.p, ANNCHOR_ESTATE, "annchor_fit_regression_device first");
    ANN_REQUIRE(c, c->sfeat_rows == c->nsamp, ANNCHOR_ESTATE, "the sample changed since annchor_fit_regression_device");
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    const int nb = c->model_nb;
    const int64_t m = c->nsamp;
    DeviceModel *dm = c->model.as<DeviceModel>();
    // a sample on an inner edge counts for both neighbours: at most 2 m entries
    ANN_TRY(ann_reserve(c, c->errs, sizeof(double) * 2 * (size_t)m));
    ANN_TRY(ann_reserve(c, c->errptr, sizeof(int64_t) * (size_t)(MAXBINS + 1)));
    const size_t lds = sizeof(unsigned long long) * 2 * ERR_CAP;
    ANN_TRY(ann_lds_once(c, (const void *)k_err_sort, 1, lds));
    {
        ProfScope ps(c, "error_residual_lists", (double)m * 32.0 * nb);
        k_err_sort<<<nb, ERR_T, lds, c->stream>>>(c->sfeat.as<double>(), c->sy.as<double>(), c->spred.as<double>(), m, dm, c->errs.as<double>(),
                                                  nb, c->dev_flags.as<int32_t>(), c->errptr.as<int64_t>());
    }
    ANN_CHECK_HIP(c, hipGetLastError());
    c->errs_on_device = true; c->model_cache_valid = false;
    return ANNCHOR_OK;
}

// The fitted model for the host (waits): coefficients W float64 [nb][3], intercepts float64 [nb], per-partition solver
// status int32 [nb] (0 = solved on the device), err_ptr int64 [nb + 1] (NULL: skip; valid after annchor_fit_errors_device),
// flags int32 [3] = the sticky flags (sample step, regression, residual lists), cleared by this call.
extern "C" int annchor_model_download(annchor_ctx *c, double *W, double *cc, int32_t *status, int64_t *err_ptr, int32_t *flags)
{
    if (!c || !W || !cc || !status || !flags) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, c->model.p && c->model_nb > 0, ANNCHOR_ESTATE, "no model on this context");
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    DeviceModel h;
    int32_t f[16];
    ANN_TRY(ann_dev_flags(c));
    ANN_TRY(ann_d2h2(c, &h, c->model.p, sizeof h, f, c->dev_flags.p, sizeof f));
    for (int b = 0; b < c->model_nb; ++b) {
        W[3 * b] = h.reg.w[b][0]; W[3 * b + 1] = h.reg.w[b][1]; W[3 * b + 2] = h.reg.w[b][2];
        cc[b] = h.reg.c[b];
        status[b] = h.status[b];
    }
    if (err_ptr)
        for (int b = 0; b <= c->model_nb; ++b) err_ptr[b] = h.errptr[b];
    flags[0] = f[0]; flags[1] = f[1]; flags[2] = f[2];
    if (f[0] | f[1] | f[2]) {
        ANN_CHECK_HIP(c, hipMemsetAsync(c->dev_flags.p, 0, sizeof(int32_t) * 16, c->stream));
    }
    return ANNCHOR_OK;
}

// The same three copies queued early -- annchor_neighbor_graph issues them before its kernel, into the tail of the pinned region
// its graph arrives in -- so that the end of a fit has ONE host wait (graph + model) instead of two.
int ann_model_prefetch_begin(annchor_ctx *c, unsigned char *at, size_t room, size_t *used)
{
    *used = 0;
    c->model_cache_valid = false;
    if (!(c->model_fitted && c->errs_on_device && c->model.p && c->errs.p && c->model_nb > 0)) return ANNCHOR_OK;
    const size_t eb = sizeof(double) * 2 * (size_t)c->nsamp;
    const size_t off_f = (sizeof(DeviceModel) + 63) & ~(size_t)63, off_e = off_f + 64;
    if (off_e + eb > room) return ANNCHOR_OK;
    ANN_TRY(ann_dev_flags(c));
    ANN_CHECK_HIP(c, hipMemcpyAsync(at, c->model.p, sizeof(DeviceModel), hipMemcpyDeviceToHost, c->stream));
    ANN_CHECK_HIP(c, hipMemcpyAsync(at + off_f, c->dev_flags.p, sizeof(int32_t) * 16, hipMemcpyDeviceToHost, c->stream));
    if (eb) ANN_CHECK_HIP(c, hipMemcpyAsync(at + off_e, c->errs.p, eb, hipMemcpyDeviceToHost, c->stream));
    c->model_cache_errs = eb;
    *used = off_e + eb;
    return ANNCHOR_OK;
}
void ann_model_prefetch_end(annchor_ctx *c, const unsigned char *at, size_t used)
{
    if (!used) return;
    c->model_cache.assign(at, at + used);
    c->model_cache_valid = true;
}

// annchor_model_download and annchor_errors_download behind ONE wait: the residual lists (at most 2 x n_samples doubles:
// a sample on a bin edge belongs to two partitions) are copied whole, *n_errs = err_ptr[nb] of them are meaningful.
extern "C" int annchor_model_download_with_errors(annchor_ctx *c, double *W, double *cc, int32_t *status, int64_t *err_ptr, int32_t *flags,
                                                  double *errs, int64_t errs_cap, int64_t *n_errs)
{
    if (!c || !W || !cc || !status || !flags || !err_ptr || !errs || !n_errs) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, c->model.p && c->model_nb > 0, ANNCHOR_ESTATE, "no model on this context");
    ANN_REQUIRE(c, c->errs_on_device && c->errs.p, ANNCHOR_ESTATE, "no device-resident residual lists");
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    size_t eb = sizeof(double) * (size_t)std::min<int64_t>(errs_cap, 2 * c->nsamp);
    const size_t off_f = (sizeof(DeviceModel) + 63) & ~(size_t)63, off_e = off_f + 64;
    const bool cached = c->model_cache_valid && c->model_cache.size() >= off_e + c->model_cache_errs;
    c->model_cache_valid = false;
    if (!cached && (!c->pin || off_e + eb > annchor_ctx::PIN_DL_BYTES)) {   // (large sample sets: the two-wait way)
        ANN_TRY(annchor_model_download(c, W, cc, status, err_ptr, flags));
        *n_errs = err_ptr[c->model_nb];
        ANN_REQUIRE(c, *n_errs <= errs_cap, ANNCHOR_EINVAL, "residual lists hold %lld entries, room for %lld", (long long)*n_errs, (long long)errs_cap);
        return annchor_errors_download(c, errs, *n_errs);
    }
    ANN_TRY(ann_dev_flags(c));
    const unsigned char *slot = c->pin + (size_t)annchor_ctx::PIN_SLOTS * annchor_ctx::PIN_SLOT_BYTES;
    if (cached) {   // fetched with the graph (ann_model_prefetch_*): no wait here
        slot = c->model_cache.data();
        eb = c->model_cache_errs;
    } else {
        unsigned char *dst = c->pin + (size_t)annchor_ctx::PIN_SLOTS * annchor_ctx::PIN_SLOT_BYTES;
        ANN_CHECK_HIP(c, hipMemcpyAsync(dst, c->model.p, sizeof(DeviceModel), hipMemcpyDeviceToHost, c->stream));
        ANN_CHECK_HIP(c, hipMemcpyAsync(dst + off_f, c->dev_flags.p, sizeof(int32_t) * 16, hipMemcpyDeviceToHost, c->stream));
        if (eb) ANN_CHECK_HIP(c, hipMemcpyAsync(dst + off_e, c->errs.p, eb, hipMemcpyDeviceToHost, c->stream));
        ANN_CHECK_HIP(c, ann_sync(c, __func__));
    }
    const DeviceModel &h = *reinterpret_cast<const DeviceModel *>(slot);
    const int32_t *f = reinterpret_cast<const int32_t *>(slot + off_f);
    for (int b = 0; b < c->model_nb; ++b) {
        W[3 * b] = h.reg.w[b][0]; W[3 * b + 1] = h.reg.w[b][1]; W[3 * b + 2] = h.reg.w[b][2];
        cc[b] = h.reg.c[b];
        status[b] = h.status[b];
    }
    for (int b = 0; b <= c->model_nb; ++b) err_ptr[b] = h.errptr[b];
    flags[0] = f[0]; flags[1] = f[1]; flags[2] = f[2];
    *n_errs = err_ptr[c->model_nb];
    if (*n_errs < 0 || (size_t)*n_errs * sizeof(double) > eb || *n_errs > errs_cap) *n_errs = -1;   // (a failed step: the flags say so; no list to hand out)
    else memcpy(errs, slot + off_e, sizeof(double) * (size_t)*n_errs);
    if (f[0] | f[1] | f[2]) ANN_CHECK_HIP(c, hipMemsetAsync(c->dev_flags.p, 0, sizeof(int32_t) * 16, c->stream));
    return ANNCHOR_OK;
}

// the sorted residuals of annchor_fit_errors_device (float64 [n_errs], n_errs = err_ptr[nb])
extern "C" int annchor_errors_download(annchor_ctx *c, double *errs, int64_t n_errs)
{
    if (!c || (n_errs > 0 && !errs)) return ANNCHOR_EINVAL;
    ANN_REQUIRE(c, c->errs_on_device && c->errs.p, ANNCHOR_ESTATE, "no device-resident residual lists");
    if (n_errs == 0) return ANNCHOR_OK;
    ANN_CHECK_HIP(c, hipSetDevice(c->device));
    return ann_d2h(c, errs, c->errs.p, sizeof(double) * (size_t)n_errs);
}
