// Every point within a radius, without a neighbour list: radius counts over a persistent index and exact DBSCAN
// (include/ogs_knn.h: ogs_knn_radius_count, ogs_knn_dbscan).
//
// The walk of knn_boxes.h with a FIXED threshold r2 instead of the falling K-th distance of knn_search.hip: a box is visited
// unless its bound is above r2.  The threshold never moves, so the order of the visits does not matter: the boxes are walked in
// index order and there is no start box.  The pair test is d2 <= r2 as an fp32 compare: equality counts, a NaN on either side
// counts nothing, and the NaN coordinates of a padding point make its d2 a NaN.  r2 is a DEVICE scalar; when it is a NaN or
// negative no pair can pass and the walk is skipped (every box would be visited otherwise, to count nothing).
//
// Labels ride along as one more LDS word per candidate, the TAG, gathered through sid while the box is staged: the candidate's
// label when it is >= 0, -1 otherwise; the query's tag is its label when that is >= 0 and INT_MIN otherwise, so that "same label,
// both active" is one integer compare and an inactive row on either side matches nothing.
//
//   count   radius_walk_kernel<kCount>, with and without tags: per lane the number of candidates that pass.  For DBSCAN the same
//           launch writes core = degree >= min_pts twice: in the caller's row order (the output) and in SORTED position.
//   link    radius_walk_kernel<kLink>, the second pass over the same boxes.  The core flags are staged beside the ids, folded
//           into the tag: a NON-core candidate is staged with tag -1 and matches nothing -- neither kind of query has any use for
//           it.  A CORE query i calls unite(i, j) (knn_union.h) for every passing candidate j < i, which visits every undirected
//           core pair once (from the second call on with the root the last call ended on in place of i: a member of i's set); a
//           NON-core query keeps the smallest pair (d2, j) over its passing (core) candidates in the order of knn_before and
//           writes anchor[i] = j, or -1.  A core row writes anchor[i] = i.
//   tail    knn_components_tail (knn_components.hip) with the anchors: flatten over the core rows, a non-core row takes the root
//           of its anchor or -1; numbering by root = by smallest CORE row; member lists; sizes.
//
// Why the hooks are right whatever a load returns: the argument at the top of knn_components.hip carries over unchanged, because
// it rests on the CAS of unite() alone.  parent[i] = i is written by a launch BEFORE the link kernel (invariant 1 holds from the
// start), the core flags are written by the count launch and only READ by the link launch, and anchor[i] has one writer.  The
// row numbers that reach unite() are sid values, which the sort clamps to [0, n).
//
// All workgroup barriers sit at the staging of a box, in wave-uniform control flow, outside the divergent unite code.  No float
// atomics, no read-back, no workgroup waits on another.  Memory is O(n) whatever the radius is.
// This file is compiled with -ffp-contract=off: d2 = (dx*dx + dy*dy) + dz*dz, exactly so, and a lower bound that is monotone.
#include "knn_boxes.h"
#include "knn_union.h"

namespace ogs {
namespace {

constexpr int kCount = 0, kLink = 1;
constexpr int kNoTag = INT_MIN;                         // tag of a query that matches nothing

struct RadiusArgs {
    int nbox;                                           // candidate boxes
    int min_pts;                                        // count: core = passes >= min_pts (only with core_sorted / core)
    int64_t n;                                          // link: rows, for the bound of unite()
    const float* r2;                                    // device scalar
    const int32_t* ref_labels;                          // [rows of the candidates] or nullptr
    const int32_t* query_labels;                        // [rows of the queries] or nullptr (with ref_labels or not at all)
    int32_t* count;                                     // count: [rows of the queries] passes per query, may be nullptr
    uint8_t* core;                                      // count: [rows of the queries] may be nullptr
    uint8_t* core_sorted;                               // count: writes, link: reads; [nbox * kKnnBox] by sorted position
    int32_t* parent;                                    // link
    int32_t* anchor;                                    // link
    uint32_t* status_word;                              // link
};

template <int MODE, bool TAGS>
__global__ __launch_bounds__(kKnnBox) void radius_walk_kernel(RadiusArgs g, const float* __restrict__ qsx, const float* __restrict__ qsy,
                                                              const float* __restrict__ qsz, const int32_t* __restrict__ qsid,
                                                              const float* __restrict__ qbox, const float* __restrict__ sx,
                                                              const float* __restrict__ sy, const float* __restrict__ sz,
                                                              const int32_t* __restrict__ sid, const float* __restrict__ box) {
    static_assert(MODE == kCount || TAGS, "the link pass folds the core flags into the tags");
    __shared__ __attribute__((aligned(16))) float cx[kKnnBox], cy[kKnnBox], cz[kKnnBox];
    __shared__ __attribute__((aligned(16))) int cid[kKnnBox], ctag[kKnnBox];
    const int lane = threadIdx.x, run = blockIdx.x, nruns = gridDim.x, nbox = g.nbox;
    const size_t p = (size_t)run * kKnnBox + lane;
    // The lane and the bound below are KnnLane::load and KnnLane::bound (knn_boxes.h) written out, the set-up in this kernel's own
    // order (label and core flag before the run's bounds): with either of the two called instead the compiler schedules these
    // kernels differently, and the link pass measured 0.8 % slower, the tagged count 0.5 %.
    const float qx = qsx[p], qy = qsy[p], qz = qsz[p];
    const int qid = qsid[p];
    const bool valid = qid != kNoId;
    const float r2 = g.r2[0];
    int qtag = 0;
    if (g.query_labels) {
        const int l = valid ? g.query_labels[qid] : -1;
        qtag = l >= 0 ? l : kNoTag;
    }
    const bool qcore = MODE == kLink && g.core_sorted[p] != 0;     // false in a padding lane: the count pass wrote 0 there
    float qlo[3], qhi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { qlo[a] = qbox[(size_t)a * nruns + run]; qhi[a] = qbox[(size_t)(3 + a) * nruns + run]; }

    int passes = 0;                                                // count
    float bd = INFINITY;                                           // link, non-core query: the smallest (d2, j) so far
    int bi = kNoId;
    int qroot = qid;                                               // link, core query: a member of its set, the root as last seen
    const int64_t bound = 2 * g.n + 2;
    const int rounds = r2 >= 0.f ? (nbox + kKnnBox - 1) / kKnnBox : 0;         // a NaN or negative threshold: nothing can pass
    for (int r = 0; r < rounds; ++r) {
        // ---- 64 candidate boxes, one per lane: the lower bound of d2 between the two boxes --------------------------------
        const int c = r * kKnnBox + lane;
        const bool inside = c < nbox;
        float lb = 0.f;
        if (inside) {                                              // KnnLane::bound, and it must stay that expression     
            float gap[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float clo = box[(size_t)a * nbox + c], chi = box[(size_t)(3 + a) * nbox + c];
                gap[a] = fmaxf(fmaxf(clo - qhi[a], qlo[a] - chi), 0.f);
            }
            lb = (gap[0] * gap[0] + gap[1] * gap[1]) + gap[2] * gap[2];
        }
        unsigned long long todo = __ballot(inside && !(lb > r2));   // (a NaN bound is visited)
        while (todo) {                                             // wave-uniform
            const int cb = r * kKnnBox + __builtin_ctzll(todo);    // in [0, nbox): that lane was `inside`
            todo &= todo - 1;
            // ---- stage the box, then every query against its 64 points -----------------------------------------------------
            const size_t cp = (size_t)cb * kKnnBox + lane;
            const float lx = sx[cp], ly = sy[cp], lz = sz[cp];
            const int lid = sid[cp];
            int ltag = 0;
            if (TAGS) {
                const int l = g.ref_labels && lid != kNoId ? g.ref_labels[lid] : 0;
                ltag = l >= 0 ? l : -1;
                if (MODE == kLink && g.core_sorted[cp] == 0) ltag = -1;
            }
            __syncthreads();                                       // the previous box has been consumed
            cx[lane] = lx; cy[lane] = ly; cz[lane] = lz;
            if (MODE == kLink) cid[lane] = lid;
            if (TAGS) ctag[lane] = ltag;
            __syncthreads();
#pragma unroll 2
            for (int v = 0; v < kKnnBox; v += 4) {
                const float4 x4 = *reinterpret_cast<const float4*>(cx + v);
                const float4 y4 = *reinterpret_cast<const float4*>(cy + v);
                const float4 z4 = *reinterpret_cast<const float4*>(cz + v);
                const float xs[4] = {x4.x, x4.y, x4.z, x4.w}, ys[4] = {y4.x, y4.y, y4.z, y4.w}, zs[4] = {z4.x, z4.y, z4.z, z4.w};
                int ts[4] = {0, 0, 0, 0}, js[4] = {0, 0, 0, 0};
                if (TAGS) {
                    const int4 t4 = *reinterpret_cast<const int4*>(ctag + v);
                    ts[0] = t4.x; ts[1] = t4.y; ts[2] = t4.z; ts[3] = t4.w;
                }
                if (MODE == kLink) {
                    const int4 i4 = *reinterpret_cast<const int4*>(cid + v);
                    js[0] = i4.x; js[1] = i4.y; js[2] = i4.z; js[3] = i4.w;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float dx = qx - xs[u], dy = qy - ys[u], dz = qz - zs[u];
                    const float d = (dx * dx + dy * dy) + dz * dz;  // NaN for a padding point on either side: passes nothing
                    const bool pass = d <= r2 && (!TAGS || ts[u] == qtag);
                    if (MODE == kCount) {
                        passes += pass ? 1 : 0;
                    } else if (pass) {                             // divergent from here on: no barrier below
                        const int j = js[u];
                        if (qcore) {
                            if (j < qid) qroot = unite(g.parent, qroot, j, bound, g.status_word);
                        } else if (knn_before(d, j, bd, bi)) {
                            bd = d; bi = j;
                        }
                    }
                }
            }
        }
    }
    if (MODE == kCount) {
        if (g.core_sorted) g.core_sorted[p] = valid && passes >= g.min_pts ? 1 : 0;      // padding lanes too: the link reads them
        if (!valid) return;
        if (g.count) g.count[qid] = passes;
        if (g.core) g.core[qid] = passes >= g.min_pts ? 1 : 0;
    } else {
        if (!valid) return;
        g.anchor[qid] = qcore ? qid : (bi != kNoId ? bi : -1);
    }
}

__global__ __launch_bounds__(kBlock) void radius_identity_kernel(int64_t n, int32_t* __restrict__ parent) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) parent[i] = (int)i;
}

template <int MODE, bool TAGS>
int launch_walk(int nruns, const RadiusArgs& g, const KnnBoxes& q, const KnnBoxes& r, hipStream_t s) {
    OGS_LAUNCH_NAMED(MODE == kLink ? "radius_link_kernel" : TAGS ? "radius_count_labels_kernel" : "radius_count_kernel",
                     (radius_walk_kernel<MODE, TAGS>), dim3((unsigned)nruns), dim3(kKnnBox), 0, s, g, q.sx, q.sy, q.sz, q.sid, q.box,
                     r.sx, r.sy, r.sz, r.sid, r.box);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

struct DbscanTmp {
    SortedTmp s;                                        // the sort's scratch and the set, unkeyed
    uint8_t* core_sorted;                               // [nbox * kKnnBox]
    int32_t* anchor;                                    // [n]
    ComponentsTmp comps;
    size_t bytes;
    static DbscanTmp carve(void* p, int64_t n) {
        Carver c(p);
        DbscanTmp t{};
        t.s = SortedTmp::carve(c, n);
        t.core_sorted = c.take<uint8_t>((size_t)knn_nbox(n) * kKnnBox);
        t.anchor = c.take<int32_t>((size_t)n);
        t.comps = ComponentsTmp::carve(c, n);
        t.bytes = c.off;
        return t;
    }
};

}  // namespace
}  // namespace ogs

using namespace ogs;

extern "C" {

size_t ogs_knn_radius_count_tmp_bytes(int64_t n, int64_t m) {
    if (n <= 0 || m <= 0 || !knn_size_ok(n) || !knn_size_ok(m)) return 0;
    Carver c(nullptr);
    return SortedTmp::carve(c, m).bytes;
}

int ogs_knn_radius_count(int64_t n, const void* index, int64_t m, const float* queries, const float* radius2,
                         const int32_t* ref_labels, const int32_t* query_labels, int32_t* count, void* tmp, size_t tmp_bytes,
                         void* stream_) {
    if (!knn_size_ok(n) || !knn_size_ok(m)) {
        set_error("knn_radius_count: bad sizes (n=%lld m=%lld; 0 <= n, m <= INT32_MAX - %d)", (long long)n, (long long)m, kKnnBox);
        return OGS_ERR_INVALID_ARG;
    }
    if ((ref_labels == nullptr) != (query_labels == nullptr)) {
        set_error("knn_radius_count: labels are given for both sets or for neither");
        return OGS_ERR_INVALID_ARG;
    }
    if (m == 0) return OGS_OK;
    if (!count) { set_error("knn_radius_count: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    if (n == 0) {                                                  // no candidate: every count is 0
        OGS_HIP_CHECK(hipMemsetAsync(count, 0, (size_t)m * sizeof(int32_t), s));
        return OGS_OK;
    }
    if (!index || !queries || !radius2 || !tmp) { set_error("knn_radius_count: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    KnnTwoSets w;
    const int rc = knn_sort_queries(n, index, m, queries, tmp, tmp_bytes, "knn_radius_count", false, s, w);
    if (rc != OGS_OK) return rc;
    RadiusArgs g{};
    g.nbox = w.nbox; g.n = n; g.r2 = radius2; g.ref_labels = ref_labels; g.query_labels = query_labels; g.count = count;
    return ref_labels ? launch_walk<kCount, true>(w.nruns, g, w.q, w.r, s) : launch_walk<kCount, false>(w.nruns, g, w.q, w.r, s);
}

size_t ogs_knn_dbscan_tmp_bytes(int64_t n) {
    if (n <= 0 || !knn_size_ok(n)) return 0;
    return DbscanTmp::carve(nullptr, n).bytes;
}

int ogs_knn_dbscan(int64_t n, const float* points, const float* eps2, int32_t min_pts, const int32_t* labels, int32_t* cluster,
                   uint8_t* core, int32_t* degree, int32_t* sizes, int32_t* first, int32_t* count, void* tmp, size_t tmp_bytes,
                   void* stream_) {
    if (!knn_size_ok(n) || min_pts < 1) {
        set_error("knn_dbscan: bad sizes (n=%lld min_pts=%d; 0 <= n <= INT32_MAX - %d, 1 <= min_pts)", (long long)n, min_pts, kKnnBox);
        return OGS_ERR_INVALID_ARG;
    }
    if (!count) { set_error("knn_dbscan: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    if (n == 0) {
        OGS_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(int32_t), s));
        return OGS_OK;
    }
    if (!points || !eps2 || !cluster || !core || !sizes || !tmp) { set_error("knn_dbscan: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    const DbscanTmp t = DbscanTmp::carve(tmp, n);
    if (tmp_bytes < t.bytes) {
        set_error("knn_dbscan: tmp has %zu bytes, %zu needed (ogs_knn_dbscan_tmp_bytes)", tmp_bytes, t.bytes);
        return OGS_ERR_INVALID_ARG;
    }
    uint32_t* status_word = async_status_word();
    if (!status_word) return OGS_ERR_HIP;
    const int nbox = (int)knn_nbox(n);
    const KnnBoxes& b = t.s.boxes;
    int rc = knn_sort_into_boxes((int)n, points, t.s.sort, b, s);
    if (rc != OGS_OK) return rc;
    RadiusArgs g{};
    g.nbox = nbox; g.min_pts = min_pts; g.n = n; g.r2 = eps2; g.ref_labels = labels; g.query_labels = labels;
    g.count = degree; g.core = core; g.core_sorted = t.core_sorted;
    rc = labels ? launch_walk<kCount, true>(nbox, g, b, b, s) : launch_walk<kCount, false>(nbox, g, b, b, s);
    if (rc != OGS_OK) return rc;
    OGS_LAUNCH(radius_identity_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, n, t.comps.parent);
    OGS_LAUNCH_CHECK(0, s);
    g.parent = t.comps.parent; g.anchor = t.anchor; g.status_word = status_word;
    rc = launch_walk<kLink, true>(nbox, g, b, b, s);
    if (rc != OGS_OK) return rc;
    return knn_components_tail(n, nullptr, t.anchor, cluster, sizes, first, count, t.comps, stream_);
}

}  // extern "C"
