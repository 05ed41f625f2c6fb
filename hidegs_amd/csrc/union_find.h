// union_find.h -- the lock-free forest of include/hidegs_components.h on the device: find and unite, shared by
// components.hip (edges from neighbour lists) and nearest_components.h (edges from the index's own walk).
//
// parent holds N int32.  Row i is a node iff parent[i] >= 0.  The invariant is parent[i] <= i for every node; a
// root is a node whose parent is not below it.  Every write lowers a word: a link is a compare-and-swap on a root,
// from the value find read there to a row below the root; a compression is an atomic minimum with an ancestor.
// The root of a tree is therefore its lowest row, and the forest after any set of unites depends on the set alone.
//
// Termination, on any content of parent.  find stands on one index at a time, and each step moves to a parent that
// is >= 0 and strictly below it, so it ends within N steps and reads only [0, N).  unite retries only after a failed
// compare-and-swap, that is after another thread lowered that word; words only go down and never below -1, so the
// number of writes of a launch is finite and so is the number of retries.  No thread waits for another.
//
// Every access is an agent-scope relaxed atomic: the XCDs' L2s are not coherent and a plain load may be served from
// a stale L1 line.  A stale value is an earlier parent, which is still an ancestor; only the compare-and-swap
// decides.  Launch boundaries order linking against finishing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hidegs {

__device__ __forceinline__ int32_t uf_load(const int32_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root above x (0 <= x < N), whose parent was read as p: the first index on the way down whose parent is negative
// or not below it.  `seen` is the parent read there: negative iff the walk ended at a row that is no node.  With
// HALVE every row passed is handed its grandparent (path halving), which is an ancestor below its parent.
template <bool HALVE>
__device__ __forceinline__ int32_t uf_find_from(int32_t* __restrict__ parent, int32_t x, int32_t p, int32_t& seen)
{
    while (p >= 0 && p < x) {  // x strictly descends
        const int32_t g = uf_load(parent + p);
        if (g < 0 || g >= p) {  // p is where the walk ends
            x = p, p = g;
            break;
        }
        if (HALVE) __hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p, p = g;
    }
    seen = p;
    return x;
}

template <bool HALVE>
__device__ __forceinline__ int32_t uf_find(int32_t* __restrict__ parent, int32_t x, int32_t& seen)
{
    return uf_find_from<HALVE>(parent, x, uf_load(parent + x), seen);
}

// Joins the trees of ra and rb, where find ended with sa and sb seen: the higher root's word is swapped from what
// find read there to the lower root.  A root that has gone stale since (another thread lowered its word) fails the
// swap, which returns where to go on.
__device__ __forceinline__ void uf_link(int32_t* __restrict__ parent, int32_t ra, int32_t sa, int32_t rb, int32_t sb)
{
    while (sa >= 0 && sb >= 0 && ra != rb) {
        if (ra < rb) {  // the higher root goes below the lower one
            int32_t t = ra;
            ra = rb, rb = t;
            t = sa, sa = sb, sb = t;
        }
        // expects what find read at the root; rb < ra <= sa, so a success lowers the word
        if (__hip_atomic_compare_exchange_strong(parent + ra, &sa, rb, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
        // another thread lowered parent[ra] to sa: go on from there
        if (sa >= 0 && sa < ra) ra = uf_find<true>(parent, sa, sa);
    }
}

// Adds the edge {a, b}, 0 <= a, b < N: afterwards both are in one tree, unless either is no node.
__device__ __forceinline__ void uf_unite(int32_t* __restrict__ parent, int32_t a, int32_t b)
{
    if (a == b) return;
    int32_t sa, sb;
    const int32_t ra = uf_find<true>(parent, a, sa), rb = uf_find<true>(parent, b, sb);
    uf_link(parent, ra, sa, rb, sb);
}

}  // namespace hidegs
