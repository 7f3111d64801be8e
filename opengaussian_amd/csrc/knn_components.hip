// Connected components of the kNN graph (include/ogs_knn.h: ogs_knn_components): a lock-free union-find over the index table,
// "hook the larger root under the smaller", then a numbering by ascending smallest member.  One call, every launch sized from
// host-known bounds, nothing read back, no atomic but the CAS of the hook (and the relaxed loads and stores around it), no
// workgroup waits on another.
//
//   init     parent[i] = the smallest edge neighbour below i that row i itself lists (i when there is none, or when the row is
//            inactive).  A link i -> j < i along an edge is a union already made, so most of a dense graph is joined before a
//            single atomic is issued.
//   hook     one thread per slot: find both roots with path halving, CAS the larger root under the smaller.
//   flatten  comp[i] = the root of i (-1: inactive), flag[i] = (comp[i] == i).
//   scan     dense = exclusive scan of flag, count = its total (exclusive_scan_u32, radix_sort.hip).
//   number   comp[i] = dense[root].
//   sizes    the member lists of the components are the reverse lists of comp seen as an [n, 1] table (ogs_knn_transpose: a
//            stable radix sort, the rows of a component ascending); sizes[c] = the length of list c, first[c] = its first
//            entry.  No counter is shared: a component of 200 000 rows costs what 200 000 singletons cost.
//
// Why the hooks are right whatever a load returns.  The per-XCD L2s and the per-CU L1s are not coherent inside a kernel, so a
// load of parent[] may return a value that is no longer there.  Three invariants make that harmless:
//   (1) parent[x] <= x always: init links downwards, a hook puts the larger root under the smaller, halving stores an ancestor.
//   (2) a row that is not a root (parent[x] != x) never becomes one again: the only write that makes a root a non-root is the
//       CAS, the CAS expects parent[x] == x, and halving only ever stores to rows it has SEEN as non-roots.
//   (3) every value parent[x] has ever held is a member of x's set (sets only grow), and is at most x.
// A walk therefore moves through members of the row's own set with strictly decreasing numbers, wherever stale values lead
// it; what it ends on may be a former root.  The CAS on the larger end `a` succeeds only when a IS a root at that instant
// (atomics are performed at agent scope, on the one copy of the word).  The smaller end `b` need not be a root: b < a, b is not
// in a's tree (everything below a root in its tree is larger than it), so parent[a] = b joins the two sets, keeps (1) and
// makes no cycle.  A failed CAS returns the current parent[a] < a and the walk continues from there.  A stale load can cost
// steps, never a wrong hook; the halving stores are hints only.
//
// Every loop is bounded by n, not by a clock: each step of unite() strictly lowers a + b, so 2 n + 2 steps suffice; the walks
// of flatten are n + 1 steps at most.  A thread that reaches the bound ORs kAsyncComponentsWalk into the library's sticky
// status word (ogs_common.h) and leaves the loop: a bug here ends as OGS_ERR_DEVICE from ogs_check_async_status(), not as a
// hung card.
//
// The primitives (load_parent, store_parent, step_up, report_bound, unite) live in knn_union.h, shared with knn_radius.hip, which
// unites inside a radius walk and ends in the same tail (knn_components_tail below: flatten .. sizes).
//
// Addresses: a slot value outside [0, n) is skipped before it indexes anything; every value read from parent[] is one the
// kernels of this call wrote, in [0, n); dense[] values are clamped to [0, n - 1] before they become component numbers, and
// the list bounds to [0, n] before they index the member array.
#include "knn_union.h"

#include <limits.h>

namespace ogs {
namespace {

struct EdgeRule {
    int64_t n;
    int K;
    const int32_t* idx;
    const float* d2;                                    // may be NULL
    const float* max_d2;                                // device scalar, may be NULL
    const int32_t* labels;                              // may be NULL
    __device__ __forceinline__ bool active(int64_t i) const { return !labels || labels[i] >= 0; }
    // slot e of ACTIVE row i with label li: the neighbour it joins i to, or -1
    __device__ __forceinline__ int edge(int64_t e, int64_t i, int li, bool use_d2, float limit) const {
        const int j = idx[e];
        if (j < 0 || (int64_t)j >= n || (int64_t)j == i) return -1;
        if (labels && labels[j] != li) return -1;       // li >= 0: an inactive j never equals it
        if (use_d2 && !(d2[e] <= limit)) return -1;     // the fp32 compare as written: NaN on either side gives no edge
        return j;
    }
};

// A row is owned by a group of L consecutive lanes, L the smallest power of two >= min(K, 64): lane l looks at the slots l,
// l + L, ... (consecutive lanes read consecutive slots), the group folds its minima by xor-shuffles and lane 0 writes.
__host__ __device__ inline int lanes_for_row(int K) {
    int L = 1;
    while (L < kWave && L < K) L *= 2;
    return L;
}
__global__ __launch_bounds__(kBlock) void components_init_kernel(EdgeRule r, int L, int32_t* __restrict__ parent) {
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;     // no early return: the fold wants whole groups
    const int64_t i = tid / L;                          // a group never straddles a wave: L divides kWave
    const int l = (int)(tid - i * L);
    int p = INT_MAX;
    if (i < r.n) {
        p = (int)i;
        if (r.active(i)) {
            const int li = r.labels ? r.labels[i] : 0;
            const bool use_d2 = r.d2 && r.max_d2;
            const float limit = use_d2 ? r.max_d2[0] : 0.f;
            for (int k = l; k < r.K; k += L) {
                const int j = r.edge(i * r.K + k, i, li, use_d2, limit);
                if (j >= 0 && j < p) p = j;
            }
        }
    }
    for (int m = L >> 1; m >= 1; m >>= 1) p = min(p, __shfl_xor(p, m, kWave));
    if (i < r.n && l == 0) parent[i] = p;
}

__global__ __launch_bounds__(kBlock) void components_hook_kernel(EdgeRule r, int64_t E, int32_t* parent, uint32_t* status_word) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= E) return;
    const int64_t i = e / r.K;
    if (!r.active(i)) return;
    const bool use_d2 = r.d2 && r.max_d2;
    const int j = r.edge(e, i, r.labels ? r.labels[i] : 0, use_d2, use_d2 ? r.max_d2[0] : 0.f);
    if (j < 0) return;
    unite(parent, (int)i, j, 2 * r.n + 2, status_word);
}

// anchor (may be nullptr; knn_union.h): row i starts its walk at anchor[i] instead of at itself, is a node of the forest only when
// that IS itself, and leaves its root in anchor[i] (-1 stays -1); labels is not read then
__global__ __launch_bounds__(kBlock) void components_flatten_kernel(int64_t n, const int32_t* __restrict__ labels, int32_t* parent,
                                                                    int32_t* __restrict__ anchor, int32_t* __restrict__ comp,
                                                                    uint32_t* __restrict__ flag, uint32_t* status_word) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    int x = (int)i;
    if (anchor) {
        x = anchor[i];
        if (x < 0 || (int64_t)x >= n) { comp[i] = -1; flag[i] = 0u; anchor[i] = -1; return; }
    } else if (labels && labels[i] < 0) { comp[i] = -1; flag[i] = 0u; return; }
    const bool node = x == (int)i;
    // no hook runs in this launch: the roots are fixed, the walk strictly descends, halving is a hint for the other walkers
    for (int64_t it = 0; ; ++it) {
        if (it > n) { report_bound(status_word); break; }
        const int p = step_up(parent, x);
        if (p == x) break;
        x = p;
    }
    comp[i] = x;
    flag[i] = node && x == (int)i ? 1u : 0u;
    if (anchor) anchor[i] = x;
}

__global__ __launch_bounds__(kBlock) void components_number_kernel(int64_t n, const uint32_t* __restrict__ dense, int32_t* __restrict__ comp) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int root = comp[i];
    if (root >= 0 && (int64_t)root < n) comp[i] = (int)min((int64_t)dense[root], n - 1);
}

// sizes and first from the member lists of the components (the reverse lists of comp seen as an [n, 1] table: the rows of
// component c, ascending): the list's length, and its first entry -- or, with root_of (may be nullptr), the root of that entry
__global__ __launch_bounds__(kBlock) void components_sizes_kernel(int64_t n, const int32_t* __restrict__ begin, const int32_t* __restrict__ members,
                                                                  const int32_t* __restrict__ root_of, int32_t* __restrict__ sizes,
                                                                  int32_t* __restrict__ first) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= n) return;
    const int64_t b = min(max((int64_t)begin[c], (int64_t)0), n), e = min(max((int64_t)begin[c + 1], b), n);
    sizes[c] = (int32_t)(e - b);
    if (!first) return;
    int f = e > b ? members[b] : -1;
    if (root_of && f >= 0) f = (int64_t)f < n ? root_of[f] : -1;
    first[c] = f;
}

bool components_sizes_ok(int64_t n, int32_t K) { return n >= 0 && K >= 1 && n * (int64_t)K < ((int64_t)1 << 31); }
int64_t blocks_for(int64_t threads) { return (threads + kBlock - 1) / kBlock; }

}  // namespace

int knn_components_tail(int64_t n, const int32_t* labels, int32_t* anchor, int32_t* comp, int32_t* sizes, int32_t* first,
                        int32_t* count, const ComponentsTmp& t, void* stream_) {
    hipStream_t s = static_cast<hipStream_t>(stream_);
    uint32_t* status_word = async_status_word();
    if (!status_word) return OGS_ERR_HIP;
    const dim3 rows((unsigned)blocks_for(n)), block(kBlock);
    OGS_LAUNCH(components_flatten_kernel, rows, block, 0, s, n, labels, t.parent, anchor, comp, t.flag, status_word);
    OGS_LAUNCH_CHECK(0, s);
    int rc = exclusive_scan_u32(t.flag, nullptr, t.dense, n, reinterpret_cast<uint32_t*>(count), t.scan_tmp, s, 0);
    if (rc != OGS_OK) return rc;
    OGS_LAUNCH(components_number_kernel, rows, block, 0, s, n, (const uint32_t*)t.dense, comp);
    OGS_LAUNCH_CHECK(0, s);
    // the member lists: comp as an [n, 1] index table over n rows (-1 is an invalid slot there), a stable sort
    rc = ogs_knn_transpose(n, 1, n, comp, t.begin, t.members, t.lists_tmp, t.lists_bytes, stream_);
    if (rc != OGS_OK) return rc;
    OGS_LAUNCH(components_sizes_kernel, rows, block, 0, s, n, (const int32_t*)t.begin, (const int32_t*)t.members,
               (const int32_t*)anchor, sizes, first);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

}  // namespace ogs

using namespace ogs;

extern "C" {

size_t ogs_knn_components_tmp_bytes(int64_t n) {
    if (n <= 0 || n >= ((int64_t)1 << 31)) return 0;
    Carver c(nullptr);
    return ComponentsTmp::carve(c, n).bytes;
}

int ogs_knn_components(int64_t n, int32_t K, const int32_t* idx, const float* d2, const float* max_d2, const int32_t* labels,
                       int32_t* comp, int32_t* sizes, int32_t* first, int32_t* count, void* tmp, size_t tmp_bytes, void* stream_) {
    if (!components_sizes_ok(n, K)) {
        set_error("knn_components: bad sizes (n=%lld K=%d; 1 <= K, n * K < 2^31)", (long long)n, K);
        return OGS_ERR_INVALID_ARG;
    }
    if (!count) { set_error("knn_components: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    if (n == 0) {
        OGS_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(int32_t), s));
        return OGS_OK;
    }
    if (!idx || !comp || !sizes || !tmp) { set_error("knn_components: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    Carver c(tmp);
    const ComponentsTmp t = ComponentsTmp::carve(c, n);
    if (tmp_bytes < t.bytes) {
        set_error("knn_components: tmp has %zu bytes, %zu needed (ogs_knn_components_tmp_bytes)", tmp_bytes, t.bytes);
        return OGS_ERR_INVALID_ARG;
    }
    uint32_t* status_word = async_status_word();
    if (!status_word) return OGS_ERR_HIP;
    const EdgeRule r{n, K, idx, d2, max_d2, labels};
    const int64_t E = n * (int64_t)K;
    const dim3 block(kBlock);
    const int L = lanes_for_row(K);
    OGS_LAUNCH(components_init_kernel, dim3((unsigned)blocks_for(n * L)), block, 0, s, r, L, t.parent);
    OGS_LAUNCH_CHECK(0, s);
    OGS_LAUNCH(components_hook_kernel, dim3((unsigned)blocks_for(E)), block, 0, s, r, E, t.parent, status_word);
    OGS_LAUNCH_CHECK(0, s);
    return knn_components_tail(n, labels, nullptr, comp, sizes, first, count, t, stream_);
}

}  // extern "C"
