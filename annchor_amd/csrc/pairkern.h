// pairkern.h -- what the pair-list kernels share (seqdp.hip, wed.hip, hausdorff.hip, jaccard.hip, euclid.hip, emd.hip): the pair
// arguments, the decode of a PairSource slot into a pair and its output position, and the result store; for the kernels on the
// ragged pool also the two DPP lane shifts and the launch grid.
#pragma once
#include "common.h"

#define PAIR_THREADS 256

// the three forms of a PairSource (common.h) and where a launch's results go
struct PairArgs {
    const int2 *ij;
    const int32_t *idx;
    const int32_t *anchor;
    int64_t n;
    double *out;
    double *RA;
    uint8_t *ncm;
};

static inline void pair_fill(PairArgs &a, const PairSource &src, double *d_out, double *d_RA, uint8_t *d_ncm)
{
    a.ij = src.ij; a.idx = src.idx; a.anchor = src.anchor; a.n = src.n;
    a.out = d_out; a.RA = d_RA; a.ncm = d_ncm;
}

// slot t of the list -> the pair (i, j) and its position in RA / ncm.  A slot past the end of the list works on the pair (0, 0)
// and stores nothing.
struct PairSlot {
    bool active;
    int i, j;
    int64_t opos;
};

__device__ __forceinline__ PairSlot pair_decode(const PairArgs &a, int64_t t)
{
    const bool active = t < a.n;
    int i = 0, j = 0;
    int64_t opos = t;
    if (active) {
        if (a.anchor) { i = *a.anchor; j = (int)t; }
        else {
            int64_t q = a.idx ? a.idx[t] : t;
            int2 p = a.ij[q];
            i = p.x; j = p.y;
            if (a.idx) opos = q;
        }
    }
    return {active, i, j, opos};
}

__device__ __forceinline__ void pair_store(const PairArgs &a, int64_t t, int64_t opos, double dist)
{
    if (a.out) a.out[t] = dist;
    if (a.RA) { a.RA[opos] = dist; a.ncm[opos] = 0; }
}

// lane l receives lane l - 1's value; lane 0 of the wavefront keeps its own
__device__ __forceinline__ double lane_down(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// lane l receives lane l + 1's value; lane 63 keeps its own
__device__ __forceinline__ double lane_up(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, 0x130, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// blocks of PAIR_THREADS for n pairs at one pair per G lanes; beyond the cap the waves take further pairs grid-stride
static inline int pair_grid(const annchor_ctx *c, int64_t n, int G)
{
    const int64_t waves = (n + ANN_WAVE / G - 1) / (ANN_WAVE / G);
    const int64_t cap = (int64_t)c->prop.multiProcessorCount * 64;
    const int64_t blocks = (waves + PAIR_THREADS / ANN_WAVE - 1) / (PAIR_THREADS / ANN_WAVE);
    return (int)(blocks < cap ? blocks : cap);
}
