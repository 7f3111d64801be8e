// What the two union-find users share (internal; the C ABI is include/ogs_knn.h): the primitives of the lock-free "hook the
// larger root under the smaller" union-find, and the host entry of the tail that turns a parent[] forest into numbered
// components.  knn_components.hip unites along the slots of an index table, knn_radius.hip inside a radius walk; the argument
// for why a stale load cannot make a wrong hook is at the top of knn_components.hip and rests on the CAS of unite() alone.
#pragma once

#include "ogs_common.h"
#include "../../include/ogs_knn.h"

namespace ogs {

__device__ __forceinline__ int load_parent(const int32_t* parent, int64_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void store_parent(int32_t* parent, int64_t x, int v) {
    __hip_atomic_store(parent + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void report_bound(uint32_t* status_word) {
    if (status_word) __hip_atomic_fetch_or(status_word, kAsyncComponentsWalk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// One step towards the root of x with path halving: returns parent[x] as loaded (x itself: x looked like a root).
__device__ __forceinline__ int step_up(int32_t* parent, int x) {
    const int p = load_parent(parent, x);
    if (p == x) return x;
    const int g = load_parent(parent, p);
    if (g != p) store_parent(parent, x, g);             // x was seen as a non-root, g is an ancestor of it: a hint, never a hook
    return p;
}

// Join the sets of rows a and b, both in [0, n).  Every pass lowers a + b by at least one or ends the loop; a + b < 2 n at the
// start, so `bound` = 2 n + 2 passes suffice.  Returns a member of the joined set, its root as far as this thread has seen: a
// caller that unites one row with many may pass it in place of that row the next time (every value is a member of the row's set).
__device__ __forceinline__ int unite(int32_t* parent, int a, int b, int64_t bound, uint32_t* status_word) {
    for (int64_t it = 0; ; ++it) {
        if (a == b) return a;
        if (it >= bound) { report_bound(status_word); return b; }
        if (a < b) { const int t = a; a = b; b = t; }   // a: the larger end
        const int pa = step_up(parent, a);
        if (pa != a) { a = pa; continue; }
        const int pb = step_up(parent, b);
        if (pb != b) { b = pb; continue; }
        // both ends looked like roots: hook the larger under the smaller, if it still is one
        int expected = a;
        if (__hip_atomic_compare_exchange_strong(parent + a, &expected, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return b;
        if (expected >= a) { report_bound(status_word); return b; }       // cannot happen (invariant 1); never walk upwards
        a = expected;                                   // what parent[a] holds now: a member of a's set below a
    }
}

struct ComponentsTmp {
    int32_t* parent;                                    // [n]
    uint32_t* flag;                                     // [n] 1 on the root rows
    uint32_t* dense;                                    // [n] exclusive scan of flag
    int32_t* begin;                                     // [n + 1] member list of component c: members[begin[c] : begin[c + 1]]
    int32_t* members;                                   // [n]
    void* scan_tmp;
    void* lists_tmp;                                    // scratch of ogs_knn_transpose(n, 1, n)
    size_t lists_bytes;
    size_t bytes;
    static ComponentsTmp carve(Carver& c, int64_t n) {
        ComponentsTmp t{};
        t.parent = c.take<int32_t>((size_t)n);
        t.flag = c.take<uint32_t>((size_t)n);
        t.dense = c.take<uint32_t>((size_t)n);
        t.begin = c.take<int32_t>((size_t)n + 1);
        t.members = c.take<int32_t>((size_t)n);
        t.scan_tmp = c.take<char>(scan_tmp_bytes(n));
        t.lists_bytes = ogs_knn_transpose_tmp_bytes(n, 1, n);
        t.lists_tmp = c.take<char>(t.lists_bytes);
        t.bytes = c.off;
        return t;
    }
};

// The tail of ogs_knn_components (knn_components.hip), from a finished t.parent[] on: flatten -> root flags ->
// exclusive_scan_u32 -> number -> member lists through ogs_knn_transpose -> sizes.  n in [1, 2^31).
//   anchor == nullptr   every row with labels == nullptr or labels[i] >= 0 is a node of the forest: comp[i] = the number of its
//                       root, first[c] = the smallest member of c.
//   anchor != nullptr   (ogs_knn_dbscan; labels is not read) the nodes are the rows with anchor[i] == i; a row with another
//                       anchor >= 0 takes the root of that node without being one, a row with anchor[i] < 0 gets -1.  The
//                       components are numbered by their root, the smallest NODE, which is what first[c] holds then; anchor[]
//                       is overwritten (with every row's root, -1 for none).
// sizes[c] counts every row numbered c; count, sizes, first as include/ogs_knn.h states them (first may be nullptr).
int knn_components_tail(int64_t n, const int32_t* labels, int32_t* anchor, int32_t* comp, int32_t* sizes, int32_t* first,
                        int32_t* count, const ComponentsTmp& t, void* stream);

}  // namespace ogs
