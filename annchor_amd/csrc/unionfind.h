// unionfind.h -- the lock-free union-find of dbscan.hip and mst.hip.  parent[v] <= v always: the larger root is hung under the
// smaller one, so no cycle can form and a component's root is its smallest member whatever the interleaving.  Every access to
// `parent` is an agent-scope atomic (relaxed): the workgroups of one launch sit on different XCDs, whose L2s do not see each
// other's plain stores.
#pragma once
#include "common.h"

__device__ __forceinline__ int32_t uf_ld(int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Root of v's tree, with path halving: every other node on the way is re-hung under its grandparent.  The re-hanging is an
// atomicMin: a parent word only ever decreases, and only to an ancestor, so concurrent finds and hooks never undo each other's work.
__device__ __forceinline__ int32_t uf_find(int32_t *parent, int32_t v)
{
    for (;;) {
        const int32_t p = uf_ld(parent + v);
        if (p == v) return v;
        const int32_t g = uf_ld(parent + p);
        if (g == p) return p;
        (void)__hip_atomic_fetch_min(parent + v, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v = g;
    }
}

// Joins the trees of x and y.
__device__ __forceinline__ void uf_union(int32_t *parent, int32_t x, int32_t y)
{
    int32_t a = uf_find(parent, x), b = uf_find(parent, y);
    while (a != b) {
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        // hi was a root when it was found; if it still is, it now hangs under lo < hi.  Otherwise somebody else hung it
        // elsewhere in between: find both roots again and retry (every failure is another thread's success: no livelock)
        int32_t expect = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &expect, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        a = uf_find(parent, hi);
        b = uf_find(parent, lo);
    }
}

// parent[v] = the root of v (the smallest value the word can take: after this minimum it holds the root, whoever else halves)
__device__ __forceinline__ int32_t uf_flatten(int32_t *parent, int32_t v)
{
    const int32_t r = uf_find(parent, v);
    if (r != v) (void)__hip_atomic_fetch_min(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return r;
}
