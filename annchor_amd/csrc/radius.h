// radius.h -- what the pair classifiers of radius.hip and knnexact.hip share: the shape of the (row, 64-column chunk) table
// and the kernel that turns its masks into a pair list.
#pragma once
#include "common.h"

#define RAD_ROWS 128     // rows per workgroup: one row per lane, two waves
#define RAD_COLS 64      // columns per chunk: one mask bit each
#define RAD_TA 32        // anchors per tile: a lane's s values in registers, the chunk's t values in LDS
#define RAD_TABLE_MAX (1ll << 23)   // (row, chunk) entries per annchor_radius_rows call: 24 B each

// one thread per (row, chunk): the pairs of its mask, ascending column, at the scan's offset.  SWAP (the query form: a row is
// a query at pool index row_begin + ridx): the pair is written column first, (j, row)
template <bool SWAP>
__global__ __launch_bounds__(256) void k_rad_emit(const uint64_t *__restrict__ mask, const int64_t *__restrict__ off, int64_t entries,
                                                  int64_t nchunks, int64_t row_begin, int64_t col_begin, int2 *__restrict__ out,
                                                  int64_t n_out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= entries) return;
    uint64_t m = mask[t];
    if (!m) return;
    const int64_t ridx = t / nchunks, chunk = t - ridx * nchunks;
    const int i = (int)(row_begin + ridx);
    const int64_t j0 = col_begin + chunk * RAD_COLS;
    int64_t o = off[t];
    while (m) {
        const int b = __ffsll((long long)m) - 1;
        m &= m - 1ull;
        if (o < n_out) out[o] = SWAP ? make_int2((int)(j0 + b), i) : make_int2(i, (int)(j0 + b));   // (o < n_out always: the offsets are the scan of these popcounts)
        ++o;
    }
}
