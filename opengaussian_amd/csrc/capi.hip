// extern "C" entry points of libogs_hip.so (declared in include/ogs_raster.h).  Host-side
// orchestration only: argument validation, scratch carving, kernel sequencing on the caller's stream.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "ogs_common.h"

namespace ogs {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- per-kernel timing ----------------------------------------------------------------------------------
namespace {
struct ProfRec { const char* name; hipEvent_t start, stop; };
int g_prof_mode = 0;     // 0 off, 1 every launch, 2 only kernels whose name starts with g_prof_prefix (cheap enough for a
                         // timed region: "blend_" = both blend kernels, or the one dominant kernel's name)
char g_prof_prefix[64] = "blend_";
std::vector<ProfRec> g_prof;
std::vector<hipEvent_t> g_event_pool;
std::mutex g_prof_mu;
hipEvent_t take_event() {
    if (!g_event_pool.empty()) { hipEvent_t e = g_event_pool.back(); g_event_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}
}  // namespace

ProfScope::ProfScope(const char* n, hipStream_t s) : name(n), stream(s), slot(-1) {
    if (g_prof_mode == 0) return;
    if (g_prof_mode == 2 && strncmp(n, g_prof_prefix, strlen(g_prof_prefix)) != 0) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    ProfRec r{n, take_event(), take_event()};
    (void)hipEventRecord(r.start, s);
    g_prof.push_back(r);
    slot = (int)g_prof.size() - 1;
}
ProfScope::~ProfScope() {
    if (slot < 0) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    (void)hipEventRecord(g_prof[slot].stop, stream);
}

// ---- sticky asynchronous device status (ogs_common.h) -----------------------------------------------------------------
namespace {
uint32_t* g_async_status = nullptr;      // pinned, device-mapped; never freed (process lifetime)
std::mutex g_async_mu;
}  // namespace
uint32_t* async_status_word() {
    std::lock_guard<std::mutex> lk(g_async_mu);
    if (!g_async_status) {
        void* p = nullptr;
        const hipError_t e = hipHostMalloc(&p, 64, hipHostMallocMapped | hipHostMallocPortable);
        if (e != hipSuccess || !p) {
            set_error("hipHostMalloc of the async status word failed: %s", hipGetErrorString(e));
            return nullptr;
        }
        memset(p, 0, 64);
        g_async_status = static_cast<uint32_t*>(p);
    }
    return g_async_status;
}
int take_async_status() {
    std::lock_guard<std::mutex> lk(g_async_mu);
    if (!g_async_status) return 0;
    return (int)__atomic_exchange_n(g_async_status, 0u, __ATOMIC_ACQ_REL);
}
int check_async_status(const char* where) {
    const int st = take_async_status();
    if (st == 0) return OGS_OK;
    set_error("%s: a kernel of an earlier launch reported status 0x%x%s%s%s -- the results of the passes since the last check "
              "are not valid", where, st,
              (st & (int)kAsyncRadixSpin) ? " (one-launch radix pass: a look-back wait exceeded its bound)" : "",
              (st & (int)kAsyncSplitOverflow) ? " (query split: the scatter met more rows than its capacity)" : "",
              (st & (int)kAsyncComponentsWalk) ? " (knn components: a union-find walk exceeded the bound n sets for it)" : "");
    return OGS_ERR_DEVICE;
}

}  // namespace ogs (reopened below)
int ogs::blend_prefetch_lines() {
    static const int v = [] {
        const char* e = getenv("OGS_BLEND_PREFETCH");
        const int n = e ? atoi(e) : kPrefetchMax;
        const int lines = (n & 0xFF) > kPrefetchMax ? kPrefetchMax : (n & 0xFF);
#ifdef OGS_EXPERIMENTS
        return n < 0 ? 0 : (lines | (n & 0x300));        // bits 8 / 9: timing ablations (skip the feature / geometry atomics):
                                                         // WRONG gradients by construction, compiled in only with -DOGS_EXPERIMENTS
#else
        return n < 0 ? 0 : lines;                        // the shipped library has no switch that changes a result
#endif
    }();
    return v;
}
namespace ogs {

static int bit_length(uint32_t v) {
    int n = 0;
    while (v) { ++n; v >>= 1; }
    return n;
}

static int validate_fwd(const OgsRasterFwdArgs* a, bool images = true) {
    if (!a) { set_error("args == NULL"); return OGS_ERR_INVALID_ARG; }
    if (a->P < 0 || a->W <= 0 || a->H <= 0) { set_error("bad sizes P=%d W=%d H=%d", a->P, a->W, a->H); return OGS_ERR_INVALID_ARG; }
    if (a->C != 3 && a->C != 6 && a->C != 9 && a->C != 12) { set_error("C=%d unsupported (3, 6, 9, 12)", a->C); return OGS_ERR_UNSUPPORTED; }
    if (a->shs == nullptr && a->colors_precomp == nullptr) {
        set_error("provide shs or colors_precomp"); return OGS_ERR_INVALID_ARG;
    }
    if (a->shs != nullptr && (a->colors_precomp != nullptr) != (a->C > 3)) {
        set_error("with shs: C == 3 and no colors_precomp, or C > 3 with colors_precomp holding the C-3 extra channels");
        return OGS_ERR_INVALID_ARG;
    }
    const bool sr = a->scales != nullptr && a->rotations != nullptr;
    if (sr == (a->cov3D_precomp != nullptr) || (a->scales != nullptr) != (a->rotations != nullptr)) {
        set_error("provide exactly one of (scales, rotations) / cov3D_precomp"); return OGS_ERR_INVALID_ARG;
    }
    if (a->shs) {
        if (a->sh_degree < 0 || a->sh_degree > 3 || a->sh_coeffs < (a->sh_degree + 1) * (a->sh_degree + 1)) {
            set_error("sh_degree=%d needs >= %d coefficients, got %d", a->sh_degree, (a->sh_degree + 1) * (a->sh_degree + 1), a->sh_coeffs);
            return OGS_ERR_INVALID_ARG;
        }
    }
    if (!a->bg || !a->viewmatrix || !a->projmatrix || !a->campos || (images && (!a->out_color || !a->out_depth || !a->out_alpha))) {
        set_error("NULL required pointer"); return OGS_ERR_INVALID_ARG;
    }
    if (a->P > 0 && (!a->means3D || !a->opacities || !a->radii || !a->geom_buffer || !a->geom_tmp)) {
        set_error("NULL required per-Gaussian pointer"); return OGS_ERR_INVALID_ARG;
    }
    if (a->num_groups < 0 || (a->num_groups > 1 && a->P > 0 && !a->group_ids)) {
        set_error("num_groups=%d needs group_ids", a->num_groups); return OGS_ERR_INVALID_ARG;
    }
    return OGS_OK;
}

// ---- raw-model entries (include/ogs_model.h) ------------------------------------------------------------------------------
// The per-Gaussian kernels take the raw model through the pointer slots the args structs already have -- shs = features_dc
// (non-NULL, so every `shs != NULL` test in the library keeps meaning "channels 0..2 come from SH"), cov3D_precomp = features_rest
// (a raw pass has no precomputed covariance), opacities / scales / rotations = the raw arrays -- and a template switch that makes
// them read those slots through ogs_model_act.h.  The copies below are what the launchers get; the callers' structs are
// checked to have all five slots NULL.
static int validate_raw(const OgsRawModel* raw, int P, int M) {
    if (!raw) { set_error("raw == NULL"); return OGS_ERR_INVALID_ARG; }
    if (M < 1) { set_error("raw model: sh_coeffs=%d < 1", M); return OGS_ERR_INVALID_ARG; }
    if (P > 0 && (!raw->features_dc || !raw->scaling || !raw->rotation || !raw->opacity)) {
        set_error("raw model: NULL features_dc / scaling / rotation / opacity"); return OGS_ERR_INVALID_ARG;
    }
    if (P > 0 && M > 1 && !raw->features_rest) { set_error("raw model: features_rest == NULL with %d SH coefficients", M); return OGS_ERR_INVALID_ARG; }
    return OGS_OK;
}

static int raw_fwd_args(const OgsRasterFwdArgs* a, const OgsRawModel* raw, OgsRasterFwdArgs* out) {
    if (!a) { set_error("args == NULL"); return OGS_ERR_INVALID_ARG; }
    if (a->shs || a->opacities || a->scales || a->rotations || a->cov3D_precomp) {
        set_error("raw pass: args.shs / opacities / scales / rotations / cov3D_precomp must be NULL (the raw model takes their place)");
        return OGS_ERR_INVALID_ARG;
    }
    int rc = validate_raw(raw, a->P, a->sh_coeffs);
    if (rc != OGS_OK) return rc;
    *out = *a;
    out->shs = raw->features_dc;
    out->opacities = raw->opacity;
    out->scales = raw->scaling;
    out->rotations = raw->rotation;
    if (a->P == 0) {                     // nothing is read per Gaussian; the argument check wants a colour source and a covariance form
        out->shs = out->scales = out->rotations = a->bg;
    }
    return OGS_OK;
}

}  // namespace ogs

using namespace ogs;

extern "C" {

int ogs_version(void) { return 420; }

int ogs_check_async_status(void) { return check_async_status("ogs_check_async_status"); }

/* Per-kernel timing with HIP events recorded on the launch stream (bench.py's `roofline` leg).
 * ogs_prof_enable(1) starts a fresh recording; ogs_prof_collect() waits for the recorded events and
 * writes a JSON object {"kernel": {"calls": n, "total_ms": t}, ...} into buf. */
int ogs_prof_enable(int on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& r : g_prof) { g_event_pool.push_back(r.start); g_event_pool.push_back(r.stop); }
    g_prof.clear();
    g_prof_mode = on;
    return OGS_OK;
}

int ogs_prof_filter(const char* prefix) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (!prefix || strlen(prefix) >= sizeof(g_prof_prefix)) { set_error("prof_filter: prefix NULL or longer than %zu", sizeof(g_prof_prefix) - 1); return OGS_ERR_INVALID_ARG; }
    strcpy(g_prof_prefix, prefix);
    return OGS_OK;
}

int ogs_prof_collect(char* buf, size_t n) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    std::map<std::string, std::pair<long, double>> agg;
    for (auto& r : g_prof) {
        OGS_HIP_CHECK(hipEventSynchronize(r.stop));
        float ms = 0.f;
        OGS_HIP_CHECK(hipEventElapsedTime(&ms, r.start, r.stop));
        auto& a = agg[r.name];
        a.first += 1;
        a.second += ms;
    }
    std::string out = "{";
    bool first = true;
    for (auto& kv : agg) {
        char line[384];
        std::string nm = kv.first;
        for (auto& ch : nm) if (ch == '"') ch = '\'';
        snprintf(line, sizeof(line), "%s\"%s\": {\"calls\": %ld, \"total_ms\": %.6f}", first ? "" : ", ", nm.c_str(),
                 kv.second.first, kv.second.second);
        out += line;
        first = false;
    }
    out += "}";
    if (!buf || out.size() + 1 > n) { set_error("prof_collect: buffer too small (%zu needed)", out.size() + 1); return OGS_ERR_SCRATCH_TOO_SMALL; }
    memcpy(buf, out.c_str(), out.size() + 1);
    return OGS_OK;
}
const char* ogs_last_error(void) { return g_err; }

size_t ogs_raster_geom_bytes(int32_t P, int32_t C) { return GeomState::bytes(P > 0 ? P : 1, C); }
size_t ogs_raster_geom_tmp_bytes(int32_t P) { return GeomTmp::bytes(P > 0 ? P : 1); }
size_t ogs_raster_image_bytes(int32_t W, int32_t H) { return ImageState::bytes(W, H); }
size_t ogs_raster_image_bytes_grouped(int32_t W, int32_t H, int32_t G) { return ImageState::bytes(W, H, num_groups_of(G)); }
size_t ogs_raster_binning_tmp_bytes(int64_t D, int32_t, int32_t) { return BinTmp::bytes(D > 0 ? D : 1); }
size_t ogs_raster_sorted_bytes(int64_t D, int32_t C) {
    return align_up((size_t)(D > 0 ? D : 1) * stream_vec4(C) * sizeof(float4));
}
size_t ogs_raster_quad_list_bytes(int64_t D) {
    // per tile four quadrant regions + the full-list positions, each of capacity n_tile (only the kept ~1.1 x D
    // indices and ~0.5 x D positions are written) + slack for the blend loops' two-ahead index prefetch on either side
    return align_up((size_t)(5 * (D > 0 ? D : 1) + 2 * kQuadPad) * sizeof(uint32_t));
}
size_t ogs_raster_backward_tmp_bytes(int32_t P) { return align_up((size_t)(P > 0 ? P : 1) * 16 * sizeof(double)); }
size_t ogs_raster_backward_pose_tmp_bytes(int32_t P) { return pose_tmp_bytes(P); }
int ogs_pose_partial_chunk(void) { return pose_partial_chunk(); }

// raw_rest: NULL for the existing entry; otherwise `a` is raw_fwd_args' copy and this is the raw model's features_rest (which may
// itself be NULL when M == 1: `raw` says which form runs)
static int forward_geometry_impl(const OgsRasterFwdArgs* a_in, void* stream_, int64_t* num_rendered_host, bool raw,
                                 const float* raw_rest) {
    int rc = validate_fwd(a_in, /*images=*/false);        // the images are written by the render phase only
    if (rc != OGS_OK) return rc;
    OgsRasterFwdArgs a_raw;
    const OgsRasterFwdArgs* a = a_in;
    if (raw) { a_raw = *a_in; a_raw.cov3D_precomp = raw_rest; a = &a_raw; }      // after the check: the slot is not a covariance
    hipStream_t s = static_cast<hipStream_t>(stream_);
    if (num_rendered_host) *num_rendered_host = 0;
    if (a->P == 0) return OGS_OK;
    rc = check_async_status("forward (entry)");          // sticky: something an EARLIER pass reported after its last check
    if (rc != OGS_OK) return rc;
    const GeomState gs = GeomState::carve(a->geom_buffer, a->P, a->C);
    const GeomTmp gt = GeomTmp::carve(a->geom_tmp, a->P);
    if (a->P <= kSmallMaxP) {
        // small pass: preprocess + depth order + scan in ONE single-workgroup launch instead of 15 (preprocess_fwd.hip)
        rc = launch_small_geometry(*a, gs, gt, s, raw);
        if (rc != OGS_OK) return rc;
    } else if (per_tile_depth_order(*a)) {
        // no depth sort: duplicate walks the Gaussians in index order and every tile's list is sorted by depth in the render
        // phase (tile_depth_sort_kernel, which gathers keys[0] as preprocess leaves it).  A culled Gaussian has tiles_touched 0,
        // so the scan and duplicate pass over it.  offsets[i] = exclusive scan of tiles_touched; total = num_rendered
        // (full-list passes; a default pass leaves offsets[] unwritten, see below)
        rc = launch_preprocess(*a, gs, gt, s, raw);
        if (rc != OGS_OK) return rc;
        // default mode: preprocess left two sums per workgroup (emitted and reference tiles), one small launch makes the emitted
        // ones offsets and forms both totals, and duplicate scans its own 256 counts (block_sum_offsets); the full-list export
        // keeps the scan
        rc = block_sum_offsets(*a) ? launch_block_offsets(*a, gt, s)
                                   : exclusive_scan_u32(gt.tiles_touched, nullptr, gt.offsets, a->P, gt.num_rendered, gt.sort_tmp, s, a->debug);
        if (rc != OGS_OK) return rc;
    } else {
        rc = launch_preprocess(*a, gs, gt, s, raw);
        if (rc != OGS_OK) return rc;
        // grouped pass (up to 2^31 virtual tiles of a few entries each: the lists are not sorted one by one, the Gaussians are
        // sorted once): depth sort of the Gaussians that are drawn, 4 x 8-bit stable passes, ends in keys[0]/order[0].  A Gaussian that is
        // not (behind the near plane, outside every group, degenerate, empty tile rect: preprocess gave it the key kDropKey)
        // leaves the list in the FIRST pass -- the mechanism the tile sort uses for its unreachable pairs -- and the other
        // three passes, the scan and duplicate run on the visible count (device word; the launches stay sized for P).  On the
        // bench scene that is 14 % of the Gaussians; a camera inside a room-scale scene sees a fraction of the model
        // (the reference only ever sorts the pairs of visible Gaussians: SURVEY.md Appendix A.2).
        const RadixSort depth_sort = {{gt.keys[0], gt.keys[1]}, {gt.order[0], gt.order[1]}, a->P, nullptr, 4, {0, 8, 16, 24}, {8, 8, 8, 8},
                                      true, gt.visible(), gt.sort_tmp};
        rc = radix_sort(depth_sort, s, a->debug);
        if (rc != OGS_OK) return rc;
        // offsets[r] = exclusive scan of tiles_touched in depth order; total = num_rendered
        rc = exclusive_scan_u32(gt.tiles_touched, gt.order[0], gt.offsets, a->P, gt.num_rendered, gt.sort_tmp, s, a->debug, gt.visible());
        if (rc != OGS_OK) return rc;
    }
    if (num_rendered_host) {       // blocking read-back (what the reference does once per forward)
        uint32_t d = 0;
        OGS_HIP_CHECK(hipMemcpyAsync(&d, gt.num_rendered, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        OGS_HIP_CHECK(hipStreamSynchronize(s));
        *num_rendered_host = (int64_t)d;
        rc = check_async_status("forward geometry phase");      // the depth sort of THIS pass has finished
        if (rc != OGS_OK) return rc;
    }
    return OGS_OK;
}

int ogs_raster_forward_geometry(const OgsRasterFwdArgs* a, void* stream_, int64_t* num_rendered_host) {
    return forward_geometry_impl(a, stream_, num_rendered_host, false, nullptr);
}

int ogs_raster_forward_geometry_raw(const OgsRasterFwdArgs* a, const OgsRawModel* raw, void* stream_, int64_t* num_rendered_host) {
    OgsRasterFwdArgs b;
    const int rc = raw_fwd_args(a, raw, &b);
    if (rc != OGS_OK) return rc;
    return forward_geometry_impl(&b, stream_, num_rendered_host, true, raw->features_rest);
}

int ogs_model_activate(int32_t P, int32_t M, const OgsRawModel* raw, float* scales, float* rotations, float* opacities, float* shs,
                       void* stream_) {
    if (P < 0) { set_error("model_activate: P=%d", P); return OGS_ERR_INVALID_ARG; }
    if (P == 0) return OGS_OK;
    if (!raw) { set_error("model_activate: raw == NULL"); return OGS_ERR_INVALID_ARG; }
    if ((scales && !raw->scaling) || (rotations && !raw->rotation) || (opacities && !raw->opacity) ||
        (shs && (M < 1 || !raw->features_dc || (M > 1 && !raw->features_rest)))) {
        set_error("model_activate: an output is requested whose raw input is NULL (M=%d)", M); return OGS_ERR_INVALID_ARG;
    }
    return launch_model_activate(P, M, *raw, scales, rotations, opacities, shs, static_cast<hipStream_t>(stream_));
}

// A one-thread kernel storing the word into the mapped pinned buffer instead of this 4-byte copy was tried (round 3: the copy costs
// 6 us idle + 4 us blit + 6 us idle between the scan and duplicate_kernel in the kernel trace): no gain at S1M and 0.28 -> 0.38 ms
// at C2 -- a kernel that writes host memory ends with a system-scope release, i.e. an L2 write-back the next kernels pay for.
int ogs_raster_read_num_rendered_async(const OgsRasterFwdArgs* a, void* stream_, uint32_t* host_pinned) {
    if (!a || !host_pinned) { set_error("read_num_rendered_async: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    if (a->P == 0) { *host_pinned = 0; return OGS_OK; }
    const GeomTmp gt = GeomTmp::carve(a->geom_tmp, a->P);
    OGS_HIP_CHECK(hipMemcpyAsync(host_pinned, gt.num_rendered, sizeof(uint32_t), hipMemcpyDeviceToHost,
                                 static_cast<hipStream_t>(stream_)));
    return OGS_OK;
}

// The count of (Gaussian, tile) pairs the pass's duplicate_kernel writes, by a blocking 4-byte copy (tests, scripts: no pass
// needs it on the host).  Call between the geometry phase and the release of geom_tmp.
int ogs_raster_read_num_emitted(const OgsRasterFwdArgs* a, void* stream_, uint32_t* host) {
    if (!a || !host) { set_error("read_num_emitted: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    *host = 0;
    if (a->P == 0) return OGS_OK;
    if (!a->geom_tmp) { set_error("read_num_emitted: geom_tmp == NULL"); return OGS_ERR_INVALID_ARG; }
    const GeomTmp gt = GeomTmp::carve(a->geom_tmp, a->P);
    hipStream_t s = static_cast<hipStream_t>(stream_);
    OGS_HIP_CHECK(hipMemcpyAsync(host, block_sum_offsets(*a) ? gt.emitted() : gt.num_rendered, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    OGS_HIP_CHECK(hipStreamSynchronize(s));
    return OGS_OK;
}

// D = exact num_rendered (deferred == false) or the CAPACITY of point_list / binning_tmp / sorted_rec while the
// binning kernels read the true count from device memory (deferred == true).
// stats != NULL: the statistics pass of ogs_raster_forward_group_stats (no images; its own, smaller image state).
static int render_impl(const OgsRasterFwdArgs* a, int64_t D, bool deferred, hipStream_t s,
                       const OgsGroupStatsArgs* stats = nullptr) {
    int rc = validate_fwd(a, stats == nullptr);
    if (rc != OGS_OK) return rc;
    if (!a->image_buffer) { set_error("image_buffer == NULL"); return OGS_ERR_INVALID_ARG; }
    if (a->bwd_clear && !stats && (((uintptr_t)a->bwd_clear | a->bwd_clear_bytes) & 15u) != 0) {
        set_error("bwd_clear / bwd_clear_bytes must be multiples of 16"); return OGS_ERR_INVALID_ARG;
    }
    const int G = num_groups_of(a->num_groups);
    const ImageState is = stats ? ImageState::carve_stats(a->image_buffer, a->W, a->H, G)
                                : ImageState::carve(a->image_buffer, a->W, a->H, G);
    const int gx = (a->W + kTile - 1) / kTile, gy = (a->H + kTile - 1) / kTile;
    const int64_t tiles = (int64_t)gx * gy * G;             // virtual tiles: image (group) * tiles_per_image + tile
    if (tiles >= (1ll << 31)) { set_error("%d groups x %d tiles exceed 2^31 virtual tiles", G, gx * gy); return OGS_ERR_UNSUPPORTED; }
    const GeomState gs = GeomState::carve(a->geom_buffer, a->P > 0 ? a->P : 1, a->C);
    const bool per_tile = per_tile_depth_order(*a);        // as the geometry phase of this pass decided
    bool order_ready = false;
    if (D > 0) {
        if (!a->point_list || !a->binning_tmp) { set_error("point_list / binning_tmp == NULL with num_rendered=%lld", (long long)D); return OGS_ERR_INVALID_ARG; }
        if (D >= (1ll << 31)) { set_error("num_rendered=%lld exceeds 2^31", (long long)D); return OGS_ERR_UNSUPPORTED; }
        const GeomTmp gt = GeomTmp::carve(a->geom_tmp, a->P);
        const BinTmp bt = BinTmp::carve(a->binning_tmp, D);
        const int bits = bit_length((uint32_t)(tiles - 1));
        const int passes = bits == 0 ? 1 : (bits + 7) / 8;
        const int per = bits == 0 ? 1 : (bits + passes - 1) / passes;
        // value ping-pong is arranged so that the LAST pass writes args->point_list
        uint32_t* vbuf[2];
        vbuf[passes & 1] = a->point_list;        // buffer index after `passes` flips from 0
        vbuf[(passes & 1) ^ 1] = bt.vals;
        // How many keys there are.  A block-sum pass emits the pairs of the reach ellipse's rects (preprocess_one, "8b"): fewer
        // than the D the host sized the buffers for, whether D is exact or a capacity, so its kernels always read the emitted
        // count from device memory.  Every other pass emits the reference rects: D itself, or gt.num_rendered when deferred.
        const uint32_t* n_dev = block_sum_offsets(*a) ? gt.emitted() : deferred ? gt.num_rendered : nullptr;
        // The (Gaussian, tile) pairs that cannot reach a pixel of their tile (52 % on the bench scene) leave the list in the FIRST
        // pass of the tile sort: duplicate gives them the key kDropKey, the pass leaves those out of its histograms and of its
        // output and reports how many keys it wrote; every later pass, the tile ranges and pack see the reachable pairs only,
        // in the order the full list has them.  args.full_binning != 0 keeps the reference's full list (the dropped pairs stay,
        // flagged in bit 31 of the value, and pack skips them): what ogs_raster_export_binning hands to the parity tests.
        const bool cull = a->full_binning == 0;
        // The default streaming pass groups the pairs by ONE counting pass on the tile id (binning.hip, "tile count" path): the
        // per-tile depth sort orders ties by id itself, so nothing before it has to be stable.  duplicate writes its values to
        // bt.vals, the count table borrows bt.tile_keys[1], the values land in point_list, every range is written (no clear).
        // Decided from the arguments alone (and the test hook's forced chunk count): 0 chunks = the radix sort below, which
        // full_binning, grouped passes, the small path, grids past the LDS histogram and lists shorter than two grids keep.
        const int count_blocks = block_sum_offsets(*a) ? tile_count_blocks(D, tiles) : 0;
        if (count_blocks > 0) {
            rc = launch_duplicate(*a, gs, gt, bt.tile_keys[0], bt.vals, (uint32_t)D, true, false, s);
            if (rc != OGS_OK) return rc;
            rc = launch_tile_count_binning(bt.tile_keys[0], bt.vals, D, n_dev, count_blocks, tiles, bt.tile_keys[1], is.ranges, bt.kept,
                                           a->point_list, s, a->debug);
            if (rc != OGS_OK) return rc;
        } else {
            const bool zero_in_dup = tiles <= (int64_t)a->P;          // one thread per range to clear
            rc = launch_duplicate(*a, gs, gt, bt.tile_keys[0], vbuf[0], (uint32_t)D, cull, !per_tile, s,
                                  zero_in_dup ? is.ranges : nullptr, zero_in_dup ? (int)tiles : 0);
            if (rc != OGS_OK) return rc;
            RadixSort tile_sort = {{bt.tile_keys[0], bt.tile_keys[1]}, {vbuf[0], vbuf[1]}, D, n_dev, passes, {}, {}, cull, bt.kept, bt.sort_tmp};
            for (int p = 0; p < passes; ++p) {
                tile_sort.shift[p] = p * per;
                tile_sort.bits[p] = (p == passes - 1) ? (bits == 0 ? 1 : bits - tile_sort.shift[p]) : per;
            }
            if (passes == 2 && (bits & 1)) {
                // odd digit total: the SMALLER digit goes first -- the first pass ranks every pair, the second only those that survive
                // the drop (13 bits: 6 + 7 instead of 7 + 6, a few us on the scatters)
                tile_sort.bits[0] = bits / 2; tile_sort.shift[1] = tile_sort.bits[0]; tile_sort.bits[1] = bits - tile_sort.bits[0];
            }
            rc = radix_sort(tile_sort, s, a->debug);
            if (rc != OGS_OK) return rc;
            rc = launch_tile_ranges(bt.tile_keys[passes & 1], D, is.ranges, tiles, s, a->debug, cull ? bt.kept : n_dev, zero_in_dup);
            if (rc != OGS_OK) return rc;
        }
        if (per_tile) {
            // each tile's list (id order after the stable radix sort, any order after the counting sort) into (depth, id) order;
            // heaviest tiles first, the same workgroup order pack then uses.  Long lists pass through bt.vals, which the tile
            // sort's last pass / tile_place_kernel left free
            const uint32_t* order = launch_tile_order(is, tiles, a->P, s, a->debug);
            order_ready = true;
            rc = launch_tile_depth_sort(is.ranges, tiles, order, a->point_list, gt.keys[0], bt.vals, s, a->debug);
            if (rc != OGS_OK) return rc;
        }
    } else {
        OGS_HIP_CHECK(hipMemsetAsync(is.ranges, 0, (size_t)tiles * sizeof(uint2), s));
    }
    if (stats) return launch_group_stats(*a, *stats, gs, is, s, order_ready);
    if (!a->sorted_rec || !a->quad_list) { set_error("sorted_rec / quad_list == NULL"); return OGS_ERR_INVALID_ARG; }
    return launch_blend_forward(*a, gs, is, D, s, order_ready);
}

int ogs_raster_forward_render(const OgsRasterFwdArgs* a, int64_t D, void* stream_) {
    return render_impl(a, D, false, static_cast<hipStream_t>(stream_));
}

size_t ogs_raster_stats_image_bytes(int32_t W, int32_t H, int32_t G) {
    return ImageState::stats_bytes(W > 0 ? W : 1, H > 0 ? H : 1, num_groups_of(G));
}
size_t ogs_raster_stats_tmp_bytes(int32_t G, int32_t L, int32_t C) {
    return align_up((size_t)num_groups_of(G) * (size_t)((L > 0 ? L : 0) + 1) * (size_t)(C > 0 ? C : 1) * sizeof(int64_t));
}

// Grouped label statistics (include/ogs_raster.h): the render phase of a grouped pass with the statistics epilogue.
// The tile sort's keys are the virtual tile ids g * tiles + t (render_impl rejects 2^31 and more): 640 groups of a 1080p frame
// are 640 * 8160 = 5.2 M virtual tiles, 23 key bits, three 8-bit passes.
int ogs_raster_forward_group_stats(const OgsRasterFwdArgs* a, const OgsGroupStatsArgs* st, int64_t D, void* stream_) {
    if (!a || !st) { set_error("forward_group_stats: NULL argument"); return OGS_ERR_INVALID_ARG; }
    if (st->num_labels < 0) { set_error("forward_group_stats: num_labels=%d < 0", st->num_labels); return OGS_ERR_INVALID_ARG; }
    if (!st->labels || !st->max_alpha || !st->count || !st->feat_sum || !st->stats_tmp) {
        set_error("forward_group_stats: NULL labels / output / stats_tmp pointer"); return OGS_ERR_INVALID_ARG;
    }
    if (D < 0) { set_error("forward_group_stats: num_rendered=%lld < 0", (long long)D); return OGS_ERR_INVALID_ARG; }
    if (a->P == 0) D = 0;
    return render_impl(a, D, false, static_cast<hipStream_t>(stream_), st);
}

int ogs_raster_forward_render_deferred(const OgsRasterFwdArgs* a, int64_t capacity, void* stream_) {
    if (capacity <= 0) { set_error("forward_render_deferred: capacity must be > 0"); return OGS_ERR_INVALID_ARG; }
    return render_impl(a, capacity, true, static_cast<hipStream_t>(stream_));
}

// Re-blend of a kept pass (include/ogs_raster.h): same geometry, same lists, new feature channels.
int ogs_raster_forward_reblend(const OgsRasterFwdArgs* a, void* stream_) {
    if (!a) { set_error("args == NULL"); return OGS_ERR_INVALID_ARG; }
    if (a->P <= 0 || a->W <= 0 || a->H <= 0) { set_error("forward_reblend: bad sizes P=%d W=%d H=%d", a->P, a->W, a->H); return OGS_ERR_INVALID_ARG; }
    if (a->C != 3 && a->C != 6 && a->C != 9 && a->C != 12) { set_error("C=%d unsupported (3, 6, 9, 12)", a->C); return OGS_ERR_UNSUPPORTED; }
    if (a->num_groups > 1) { set_error("forward_reblend: grouped passes are not kept"); return OGS_ERR_UNSUPPORTED; }
    if (!a->colors_precomp || !a->bg || !a->out_color || !a->out_depth || !a->out_alpha || !a->image_buffer || !a->sorted_rec ||
        !a->quad_list) {
        set_error("forward_reblend: NULL required pointer (colors_precomp, bg, out_*, image_buffer, sorted_rec, quad_list)");
        return OGS_ERR_INVALID_ARG;
    }
    const int rc = check_async_status("forward_reblend (entry)");
    if (rc != OGS_OK) return rc;
    const ImageState is = ImageState::carve(a->image_buffer, a->W, a->H, 1);
    return launch_reblend(*a, is, static_cast<hipStream_t>(stream_));
}

int ogs_raster_compact_kept(int32_t W, int32_t H, int32_t C, const void* image_buffer, const void* sorted_rec, const void* quad_list,
                            void* new_image_buffer, void* new_sorted_rec, void* new_quad_list, void* stream_) {
    if (W <= 0 || H <= 0) { set_error("compact_kept: bad sizes W=%d H=%d", W, H); return OGS_ERR_INVALID_ARG; }
    if (!image_buffer || !sorted_rec || !quad_list || !new_image_buffer || !new_sorted_rec || !new_quad_list) {
        set_error("compact_kept: NULL pointer"); return OGS_ERR_INVALID_ARG;
    }
    const ImageState is_old = ImageState::carve(const_cast<void*>(image_buffer), W, H, 1);
    const ImageState is_new = ImageState::carve(new_image_buffer, W, H, 1);
    return launch_compact_kept(W, H, C, is_old, is_new, sorted_rec, quad_list, new_sorted_rec, new_quad_list,
                               static_cast<hipStream_t>(stream_));
}

size_t ogs_raster_tiny_max_points(void) { return (size_t)kTinyMaxP; }

size_t ogs_raster_tile_sort_capacity(int32_t level) {
    return level == 0 ? (size_t)kWaveSortCap : level == 1 ? (size_t)kTileSortCap : level == 2 ? (size_t)tile_sort_bucket_cap() : 0;
}

// Tests: the bucket cap of the one-wave depth sort.  bucket_cap > 0 forces it (1: every list of two entries or more takes the LSD
// passes; above the list length: every list is ranked inside its buckets), 0 gives the choice back to the library, a negative
// value leaves it as it is.  Process-wide: a test restores 0 when it is done.
int ogs_raster_tile_sort_debug(int32_t bucket_cap) {
    tile_sort_debug(bucket_cap);
    return OGS_OK;
}

// Tests: the chunk count B the counting sort by tile takes for a list capacity D and a grid of `tiles` (0: such a pass takes the
// radix sort), after setting the hooks -- force_blocks > 0 forces B (still cut to what the table has room for), 0 gives the
// choice back to the library, reverse != 0 makes tile_place_kernel walk its chunks back to front; a negative value leaves a
// hook as it is.  Process-wide: a test restores (0, 0) when it is done.
int ogs_raster_tile_count_debug(int64_t D, int64_t tiles, int32_t force_blocks, int32_t reverse) {
    tile_count_debug(force_blocks, reverse);
    return tile_count_blocks(D, tiles);
}
size_t ogs_raster_tile_count_trip(void) { return (size_t)tile_count_trip(); }

// Tests: the grid of tile_place_kernel.  group / slices / stage_words > 0 force G (count chunks per place chunk), S (tile slices)
// and the staging words per workgroup, 0 gives that choice back to the library, a negative value leaves it as it is; chosen[0..2]
// receives (place chunks, slices, staging words) of a pass with list capacity D and `tiles` tiles under the hooks as they stand
// (all 0 when such a pass takes the radix sort).  Process-wide: a test restores (0, 0, 0) when it is done.
int ogs_raster_tile_place_debug(int64_t D, int64_t tiles, int32_t group, int32_t slices, int32_t stage_words, int32_t* chosen) {
    tile_place_debug(group, slices, stage_words);
    if (chosen) {
        const TilePlacePlan pl = tile_place_plan(D, tiles, tile_count_blocks(D, tiles));
        chosen[0] = pl.chunks; chosen[1] = pl.slices; chosen[2] = (int32_t)pl.stage_words;
    }
    return OGS_OK;
}

static int forward_tiny_impl(const OgsRasterFwdArgs* a_in, void* stream_, bool raw, const float* raw_rest) {
    int rc = validate_fwd(a_in);
    if (rc != OGS_OK) return rc;
    OgsRasterFwdArgs a_raw;
    const OgsRasterFwdArgs* a = a_in;
    if (raw) { a_raw = *a_in; a_raw.cov3D_precomp = raw_rest; a = &a_raw; }
    if (a->P <= 0 || a->P > kTinyMaxP) { set_error("forward_tiny: P=%d outside [1, %d]", a->P, kTinyMaxP); return OGS_ERR_INVALID_ARG; }
    if (a->num_groups > 1) { set_error("forward_tiny: grouped passes use the streaming path"); return OGS_ERR_UNSUPPORTED; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const GeomState gs = GeomState::carve(a->geom_buffer, a->P, a->C);
    uint32_t* order = static_cast<uint32_t*>(a->geom_tmp);        // [P] depth order; geom_tmp >= ogs_raster_geom_tmp_bytes(P)
    rc = launch_tiny_geometry(*a, gs, order, s, raw);
    if (rc != OGS_OK) return rc;
    return launch_tiny_blend(*a, gs, order, s);
}

int ogs_raster_forward_tiny(const OgsRasterFwdArgs* a, void* stream_) { return forward_tiny_impl(a, stream_, false, nullptr); }

int ogs_raster_forward_tiny_raw(const OgsRasterFwdArgs* a, const OgsRawModel* raw, void* stream_) {
    OgsRasterFwdArgs b;
    const int rc = raw_fwd_args(a, raw, &b);
    if (rc != OGS_OK) return rc;
    return forward_tiny_impl(&b, stream_, true, raw->features_rest);
}

static int backward_impl(const OgsRasterBwdArgs* a, void* stream_, const OgsRawModelGrads* raw_grads) {
    if (!a) { set_error("args == NULL"); return OGS_ERR_INVALID_ARG; }
    if (a->C != 3 && a->C != 6 && a->C != 9) { set_error("backward: C=%d unsupported (3, 6, 9)", a->C); return OGS_ERR_UNSUPPORTED; }
    // camera gradients (pose_bwd.hip): all of the three outputs and their scratch, or none
    const bool pose = backward_wants_pose(*a);
    if (pose) {
        if (!a->dL_dviewmatrix || !a->dL_dprojmatrix || !a->dL_dcampos || !a->pose_tmp) {
            set_error("backward: dL_dviewmatrix, dL_dprojmatrix, dL_dcampos and pose_tmp must be given together");
            return OGS_ERR_INVALID_ARG;
        }
        if (a->P < 0) { set_error("backward: P=%d", a->P); return OGS_ERR_INVALID_ARG; }
        if (a->num_groups > 1) {
            set_error("backward: camera gradients of a grouped pass (num_groups=%d) are not supported", a->num_groups);
            return OGS_ERR_UNSUPPORTED;
        }
        // nothing was blended: the 35 floats are still written, as zeros (the fold of no rows)
        if (a->P == 0) return launch_pose_backward(*a, GeomState{}, nullptr, static_cast<hipStream_t>(stream_), false);
    }
    if (a->P == 0) return OGS_OK;
    // the features-only pass reads the blend state and the radii alone: a caller that kept only those (the re-blend of a kept
    // pass, ogs_raster_forward_reblend) may leave the per-Gaussian inputs, geom_buffer and point_list NULL
    const bool feat_only = backward_is_features_only(*a);
    if (!a->dL_dcolor || !a->image_buffer || !a->bwd_tmp || !a->radii) {
        set_error("backward: NULL required pointer"); return OGS_ERR_INVALID_ARG;
    }
    if (!feat_only && (!a->geom_buffer || !a->bg || !a->means3D || !a->viewmatrix || !a->projmatrix || !a->campos)) {
        set_error("backward: NULL required pointer"); return OGS_ERR_INVALID_ARG;
    }
    if (!feat_only && a->num_rendered > 0 && !a->point_list) { set_error("backward: point_list == NULL"); return OGS_ERR_INVALID_ARG; }
    // the blend kernels address the gradient record with 32-bit element offsets (g * 16 + slot, SGPR-base atomics)
    if ((int64_t)a->P * grad_stride(a->C) >= (1ll << 32)) {
        set_error("backward: P=%d exceeds the %lld Gaussians the 32-bit gradient-record offsets address", a->P,
                  (long long)((1ll << 32) / grad_stride(a->C)) - 1);
        return OGS_ERR_UNSUPPORTED;
    }
    {
        const int st = check_async_status("backward (entry)");
        if (st != OGS_OK) return st;
    }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const GeomState gs = GeomState::carve(const_cast<void*>(a->geom_buffer), a->P, a->C);
    if (a->num_groups < 0) { set_error("backward: num_groups=%d", a->num_groups); return OGS_ERR_INVALID_ARG; }
    const ImageState is = ImageState::carve(const_cast<void*>(a->image_buffer), a->W, a->H, num_groups_of(a->num_groups));
    void* grad_rec = a->bwd_tmp;
    if (pose) {
        // what pose_partials_kernel re-derives the covariance from; every check of such a call comes before its first launch
        if (!a->cov3D_precomp && (!a->scales || !a->rotations)) {
            set_error("backward: camera gradients need scales + rotations or cov3D_precomp"); return OGS_ERR_INVALID_ARG;
        }
        if (a->num_rendered > 0 && (!a->sorted_rec || !a->quad_list)) { set_error("backward: sorted_rec / quad_list == NULL"); return OGS_ERR_INVALID_ARG; }
    }
    // features-only pass: a record is the feature sums alone, 64 bytes when they fit (feat_grad_stride) -- half the fill.  (A strided
    // hipMemset2DAsync over the front halves of full-size records cost 0.1 ms against 0.016 ms for a contiguous fill: measured.)
    const int rec_doubles = feat_only ? feat_grad_stride(a->C, a->shs ? 3 : 0) : grad_stride(a->C);
    // bwd_tmp_is_clear: the forward blend of this pass zeroed the record on its way (OgsRasterFwdArgs.bwd_clear)
    if (!a->bwd_tmp_is_clear) OGS_HIP_CHECK(hipMemsetAsync(grad_rec, 0, (size_t)a->P * rec_doubles * sizeof(double), s));
    if (a->num_rendered > 0 && (!a->sorted_rec || !a->quad_list)) { set_error("backward: sorted_rec / quad_list == NULL"); return OGS_ERR_INVALID_ARG; }
    int rc = launch_blend_backward(*a, is, grad_rec, s);
    if (rc != OGS_OK) return rc;
    if (!pose) return launch_preprocess_backward(*a, gs, grad_rec, s, raw_grads);
    // a pose-only call (frozen model) has no per-Gaussian output: preprocess_backward would read every record to write nothing
    const bool per_gaussian = a->dL_dmeans2D || a->dL_dcolors || a->dL_dopacity || a->dL_dmeans3D || a->dL_dcov3D || a->dL_dsh ||
                              a->dL_dscales || a->dL_drotations || a->dL_dsh_rgb || (raw_grads && raw_grads->features_rest);
    if (per_gaussian) {
        rc = launch_preprocess_backward(*a, gs, grad_rec, s, raw_grads);
        if (rc != OGS_OK) return rc;
    }
    return launch_pose_backward(*a, gs, grad_rec, s, raw_grads != nullptr);
}

int ogs_raster_backward(const OgsRasterBwdArgs* a, void* stream_) { return backward_impl(a, stream_, nullptr); }

int ogs_raster_backward_raw(const OgsRasterBwdArgs* a, const OgsRawModel* raw, const OgsRawModelGrads* grads, void* stream_) {
    if (!a) { set_error("args == NULL"); return OGS_ERR_INVALID_ARG; }
    if (a->shs || a->opacities || a->scales || a->rotations || a->cov3D_precomp || a->dL_dsh || a->dL_dopacity || a->dL_dscales ||
        a->dL_drotations || a->dL_dcov3D) {
        set_error("raw backward: args.shs / opacities / scales / rotations / cov3D_precomp and their dL_d* outputs must be NULL "
                  "(the raw model and its gradient struct take their place)");
        return OGS_ERR_INVALID_ARG;
    }
    const int rc = validate_raw(raw, a->P, a->sh_coeffs);
    if (rc != OGS_OK) return rc;
    static const OgsRawModelGrads kNoGrads = {nullptr, nullptr, nullptr, nullptr, nullptr};
    const OgsRawModelGrads* g = grads ? grads : &kNoGrads;
    if (g->features_rest && !raw->features_rest) { set_error("raw backward: a features_rest gradient without features_rest"); return OGS_ERR_INVALID_ARG; }
    // the copy the kernels get (see raw_fwd_args).  dL_dsh stands for "the dense SH gradient is wanted" in the host-side choices
    // (backward_is_features_only); launch_preprocess_backward puts the two halves into the kernel's slots
    OgsRasterBwdArgs b = *a;
    b.shs = raw->features_dc;
    b.opacities = raw->opacity;
    b.scales = raw->scaling;
    b.rotations = raw->rotation;
    b.cov3D_precomp = raw->features_rest;
    b.dL_dsh = g->features_dc ? g->features_dc : g->features_rest;
    b.dL_dopacity = g->opacity;
    b.dL_dscales = g->scaling;
    b.dL_drotations = g->rotation;
    return backward_impl(&b, stream_, g);
}

int ogs_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float*, uint8_t* present,
                     void* stream_) {
    if (P == 0) return OGS_OK;
    if (!means3D || !viewmatrix || !present) { set_error("mark_visible: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    return launch_mark_visible(P, means3D, viewmatrix, present, static_cast<hipStream_t>(stream_));
}

int ogs_sh_grad_from_views(int32_t P, int32_t V, int32_t sh_degree, int32_t sh_coeffs, const float* means3D,
                           const float* campos, const float* dL_drgb, float* dL_dsh, void* stream_) {
    if (P == 0) return OGS_OK;
    if (P < 0 || V < 1 || sh_degree < 0 || sh_degree > 3 || sh_coeffs < (sh_degree + 1) * (sh_degree + 1)) {
        set_error("sh_grad_from_views: bad sizes P=%d V=%d degree=%d coeffs=%d", P, V, sh_degree, sh_coeffs);
        return OGS_ERR_INVALID_ARG;
    }
    if (!means3D || !campos || !dL_drgb || !dL_dsh) { set_error("sh_grad_from_views: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    return launch_sh_grad_from_views(P, V, sh_degree, sh_coeffs, means3D, campos, dL_drgb, dL_dsh,
                                     static_cast<hipStream_t>(stream_));
}

/* test hook (not part of the reference boundary): the wave64 16-slot transposed reduction used by the
 * backward blend.  in: [64][16] floats, out: [64]; out[lane] must equal sum_l in[l][lane>>2]. */
int ogs_selftest_wave_fold16(const float* in, float* out, void* stream_) {
    if (!in || !out) { set_error("selftest: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    return launch_wave_fold16_test(in, out, static_cast<hipStream_t>(stream_));
}

/* test hook: the forward walk's per-step accumulation as a matrix instruction (4 rank-one 16x16 updates per MFMA, K = 1) chained
 * `steps` times, and the same chain as one fmaf per element; the two outputs must agree bit for bit. */
int ogs_selftest_mfma_rank1(const float* w, const float* f, const float* acc0, int32_t steps, float* out_mfma, float* out_fma,
                            void* stream_) {
    if (!w || !f || !acc0 || !out_mfma || !out_fma || steps < 0) { set_error("selftest: NULL pointer / steps < 0"); return OGS_ERR_INVALID_ARG; }
    return launch_mfma_rank1_test(w, f, acc0, steps, out_mfma, out_fma, static_cast<hipStream_t>(stream_));
}

int ogs_selftest_tile_order(const uint32_t* ranges, int64_t vtiles, uint32_t* order, void* stream_) {
    if (!ranges || !order || vtiles <= 0) { set_error("selftest: NULL pointer / no tiles"); return OGS_ERR_INVALID_ARG; }
    return launch_tile_order_test(ranges, vtiles, order, static_cast<hipStream_t>(stream_));
}

size_t ogs_selftest_radix_tmp_bytes(int64_t n) { return sort_tmp_bytes(n > 0 ? n : 1); }

int ogs_selftest_radix_sort(uint32_t* keys0, uint32_t* vals0, uint32_t* keys1, uint32_t* vals1, int64_t n, int32_t key_bits,
                            int32_t variant, int32_t items, const uint32_t* n_dev, void* tmp, int32_t* result_buffer,
                            void* stream_) {
    if (!result_buffer) { set_error("selftest_radix_sort: NULL result_buffer"); return OGS_ERR_INVALID_ARG; }
    *result_buffer = 0;
    if (n <= 0) return OGS_OK;
    if (items != 0 && items != 4 && items != 16) { set_error("selftest_radix_sort: items=%d (0, 4 or 16)", items); return OGS_ERR_INVALID_ARG; }
    if (!keys0 || !vals0 || !keys1 || !vals1 || !tmp || key_bits < 1 || key_bits > 32) {
        set_error("selftest_radix_sort: bad arguments"); return OGS_ERR_INVALID_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const int passes = (key_bits + 7) / 8, per = (key_bits + passes - 1) / passes;
    // variant bit 0: one launch per pass; bit 1: drop mode -- keys equal to 0xFFFFFFFF leave in the first pass (the tile sort of the
    // default binning mode); the number of keys left is returned in bits 1.. of *result_buffer
    // variant bit 2: the look-back waits of the one-launch passes get a bound of ZERO polls -- fault injection for the
    // sticky status word: the call must come back with OGS_ERR_DEVICE (and a wrong permutation)
    const bool drop = (variant & 2) != 0;
    RadixSort sort = {{keys0, keys1}, {vals0, vals1}, n, n_dev, passes, {}, {}, drop, nullptr, tmp,
                      (variant & 1) ? RadixImpl::OneLaunch : RadixImpl::ThreeLaunch, items, (variant & 4) ? 0 : -1};
    for (int p = 0; p < passes; ++p) { sort.shift[p] = p * per; sort.bits[p] = p == passes - 1 ? key_bits - sort.shift[p] : per; }
    (void)take_async_status();       // the hook reports what THIS sort does
    if (drop) {
        OGS_HIP_CHECK(hipMalloc(&sort.kept, sizeof(uint32_t)));
        // poisoned, as the render phase's scratch is (torch.empty): every path of the first pass must write it
        OGS_HIP_CHECK(hipMemsetAsync(sort.kept, 0xA5, sizeof(uint32_t), s));
    }
    int rc = radix_sort(sort, s, 0);
    uint32_t kept_host = 0;
    if (drop) {
        if (rc == OGS_OK && hipMemcpyAsync(&kept_host, sort.kept, sizeof(uint32_t), hipMemcpyDeviceToHost, s) != hipSuccess) rc = OGS_ERR_HIP;
        (void)hipStreamSynchronize(s);
        (void)hipFree(sort.kept);
    } else {
        (void)hipStreamSynchronize(s);
    }
    if (rc != OGS_OK) return rc;
    *result_buffer = (passes & 1) | (drop ? (int32_t)(kept_host << 1) : 0);
    return check_async_status("selftest_radix_sort");
}

size_t ogs_selftest_scan_tmp_bytes(int64_t n) { return scan_tmp_bytes(n > 0 ? n : 1); }

/* test hook: exclusive_scan_u32 as the library's callers reach it -- no read-back, no synchronisation */
int ogs_selftest_scan_u32(const uint32_t* in, const uint32_t* gather, uint32_t* out, int64_t n, uint32_t* total,
                          const uint32_t* n_dev, void* tmp, void* stream_) {
    if (n > 0 && (!in || !out || !tmp)) { set_error("selftest_scan_u32: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    return exclusive_scan_u32(in, gather, out, n, total, tmp, static_cast<hipStream_t>(stream_), 0, n_dev);
}

int ogs_raster_export_binning(const OgsRasterFwdArgs* a, int64_t D, uint64_t* keys_out, uint32_t* ranges_out,
                              uint32_t* n_contrib_out, void* stream_) {
    if (!a) { set_error("args == NULL"); return OGS_ERR_INVALID_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const int G = num_groups_of(a->num_groups);     // grouped pass: everything below is per VIRTUAL tile / image
    const ImageState is = ImageState::carve(a->image_buffer, a->W, a->H, G);
    const int gx = (a->W + kTile - 1) / kTile, gy = (a->H + kTile - 1) / kTile;
    if (keys_out && D > 0) {
        const GeomState gs = GeomState::carve(a->geom_buffer, a->P, a->C);
        int rc = launch_export_keys(is.ranges, gx * gy * G, a->point_list, gs.rec, rec_vec4(a->C), keys_out, s);
        if (rc != OGS_OK) return rc;
    }
    if (ranges_out)
        OGS_HIP_CHECK(hipMemcpyAsync(ranges_out, is.ranges, (size_t)gx * gy * G * sizeof(uint2), hipMemcpyDeviceToDevice, s));
    if (n_contrib_out) {
        if (D > 0) {
            int rc = launch_export_n_contrib(*a, is, n_contrib_out, s);
            if (rc != OGS_OK) return rc;
        } else {
            OGS_HIP_CHECK(hipMemsetAsync(n_contrib_out, 0, (size_t)G * a->W * a->H * sizeof(uint32_t), s));
        }
    }
    return OGS_OK;
}

}  // extern "C"
