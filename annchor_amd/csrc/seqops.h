// seqops.h -- what the two kernels of DTW and Frechet share (seqdp.hip: 1 .. 4 coordinates per point, seqwide.hip: 5 .. 64): the
// pair arguments of a sequence measure and the two cells.  The definitions are in the head of seqdp.hip.
#pragma once
#include "pairkern.h"

#define DTW_MAXLEN 2048

template <typename T> struct SeqArgs : PairArgs {
    const T *val;
    const int32_t *off, *len;   // counted in points
    int window;                 // DTW's band; LCSS's delta (-1: none); others: unused
    const double *gapsum;       // ERP: [points of the pool] running sums of gap costs, E(i, -1) of each member; others: unused
    double gap;                 // ERP: the gap value
    double msm_c;               // MSM: the cost of a split or merge
    double twe_nl, twe_nu2;     // TWE: nu + lam and 2 nu
    double eps;                 // EDR, LCSS: the matching threshold, per coordinate
    int normalize;              // EDR: whether the store divides by the longer member's length
};

// An Op is the cell and, as compile-time traits, what its launch needs: `profile`, the profile scope's name; `max_dim`, the
// largest dim (1: univariate members, whatever curve_dim holds); max_len(dim), the longest member its widest shape takes;
// point_bytes(dim, elem), what a point costs to read (the profile's traffic figure); `member`, the noun of its refusals.  Op::erp
// also says that `gapsum` must be bound.  (max_dim and max_len are k_seqdp's; k_seqwide has its own limits.)
template <bool BAND> struct DtwOp {
    static constexpr bool band = BAND, erp = false, prev = false, msm = false, thresh = false, lcss = false;
    static constexpr const char *profile = "dtw_pairs", *member = "series";
    static constexpr int max_dim = 4;
    static constexpr int max_len(int dim) { return (dim <= 2 ? 32 : 16) * 64; }
    static constexpr size_t point_bytes(int dim, size_t elem) { return dim * elem; }
    static __device__ __forceinline__ double cell(double cost, double left, double up, double dg) { return cost + fmin(fmin(left, up), dg); }
};
struct FrechetOp {
    static constexpr bool band = false, erp = false, prev = false, msm = false, thresh = false, lcss = false;
    static constexpr const char *profile = "frechet_pairs", *member = "curve";
    static constexpr int max_dim = 4;
    static constexpr int max_len(int dim) { return (dim <= 2 ? 32 : 16) * 64; }
    static constexpr size_t point_bytes(int dim, size_t elem) { return dim * elem; }
    static __device__ __forceinline__ double cell(double cost, double left, double up, double dg) { return fmax(cost, fmin(fmin(left, dg), up)); }
};
