// Shared declarations for the gfx950 rasterizer / k-means kernels (internal; the public C ABI is
// include/ogs_raster.h and include/ogs_kmeans.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <type_traits>

#include "../../include/ogs_raster.h"
#include "../../include/ogs_model.h"

namespace ogs {

constexpr int kTile = OGS_TILE;      // 16x16 pixel tiles
constexpr int kBlock = 256;          // 4 wave64 per workgroup everywhere
constexpr int kWave = 64;
constexpr int kTinyMaxP = 256;       // largest P of the tiny pass (one workgroup does the whole geometry phase)
constexpr int kSmallMaxP = 1024;     // largest P whose geometry phase (preprocess + depth sort + scan) is ONE workgroup

// ---- error plumbing -------------------------------------------------------------------------
void set_error(const char* fmt, ...);

#define OGS_HIP_CHECK(expr)                                                              \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess) {                                                          \
            ogs::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return OGS_ERR_HIP;                                                          \
        }                                                                                \
    } while (0)

// After a kernel launch: always catch launch errors; with debug also synchronise (the reference's
// debug=True behaviour, SURVEY.md section 8(b) "Errors").
#define OGS_LAUNCH_CHECK(debug, stream)                                                  \
    do {                                                                                 \
        OGS_HIP_CHECK(hipGetLastError());                                                \
        if (debug) OGS_HIP_CHECK(hipStreamSynchronize(stream));                          \
    } while (0)

// ---- sticky asynchronous device status ------------------------------------------------------------------------------
// One 32-bit word in pinned, device-mapped host memory (allocated on first use, one per process = one per GPU).  A kernel
// that detects a condition it cannot recover from ORs a bit into it with a system-scope atomic -- code that never executes
// in a healthy run, so it costs nothing there -- and carries on without hanging or writing out of bounds.  The host reads
// (and clears) the word wherever it already synchronises with the stream: after the num_rendered read-back of a forward,
// at the entry of the next forward / backward, in the self-test hooks; ogs_check_async_status() turns it into
// OGS_ERR_DEVICE.  Producers: the bounded look-back spin of radix_onesweep_kernel (radix_sort.hip), and the scatter of the query
// split (query.hip) when a row's position lies at or beyond the capacity it was given, and the walks and retry loops of the
// union-find (knn_components.hip) when one passes the bound that n sets for it.
constexpr uint32_t kAsyncRadixSpin = 1u;
constexpr uint32_t kAsyncSplitOverflow = 2u;
constexpr uint32_t kAsyncComponentsWalk = 4u;
uint32_t* async_status_word();                   // device-usable pointer (nullptr + set_error when the allocation fails)
int take_async_status();                         // read and clear; 0 = nothing happened (also when never allocated)
int check_async_status(const char* where);       // OGS_OK, or OGS_ERR_DEVICE with the message set

// ---- optional per-kernel timing (HIP events on the launch stream; used by bench.py) -----------------
struct ProfScope {
    const char* name;
    hipStream_t stream;
    int slot;
    ProfScope(const char* name, hipStream_t s);
    ~ProfScope();
};
#define OGS_LAUNCH(kernel, grid, block, lds, stream, ...)                      \
    do {                                                                       \
        ogs::ProfScope _ps(#kernel, stream);                                   \
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);     \
    } while (0)

// same, with an explicit timing name (template kernels: one name per channel count)
#define OGS_LAUNCH_NAMED(name, kernel, grid, block, lds, stream, ...)          \
    do {                                                                       \
        ogs::ProfScope _ps(name, stream);                                      \
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);     \
    } while (0)
template <int C>
constexpr const char* chan_name(const char* const (&names)[4]) {
    return C == 3 ? names[0] : C == 6 ? names[1] : C == 9 ? names[2] : names[3];
}

// Runtime channel count -> compile-time constant: f(std::integral_constant<int, C>) for C in {3, 6, 9, 12} up to MaxC (the
// backward kernels stop at 9); anything else sets `unsupported_fmt` (one %d: the count) and returns OGS_ERR_UNSUPPORTED.
template <int MaxC, class F>
int dispatch_channels(int C, const char* unsupported_fmt, F&& f) {
    static_assert(MaxC == 9 || MaxC == 12, "supported sets: {3, 6, 9} and {3, 6, 9, 12}");
    switch (C) {
        case 3: return f(std::integral_constant<int, 3>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 9: return f(std::integral_constant<int, 9>{});
        case 12:
            if constexpr (MaxC >= 12) return f(std::integral_constant<int, 12>{});
            [[fallthrough]];
        default: set_error(unsupported_fmt, C); return OGS_ERR_UNSUPPORTED;
    }
}

// ---- scratch carving ------------------------------------------------------------------------
constexpr size_t kAlign = 256;
inline size_t align_up(size_t v, size_t a = kAlign) { return (v + a - 1) / a * a; }

struct Carver {
    char* base;
    size_t off = 0;
    explicit Carver(void* p) : base(static_cast<char*>(p)) {}
    template <typename T>
    T* take(size_t n) {
        T* r = reinterpret_cast<T*>(base ? base + off : nullptr);
        off = align_up(off + n * sizeof(T));
        return r;
    }
};

// ---- per-Gaussian forward record ("rec") ------------------------------------------------------
// One contiguous, 16-byte aligned record per Gaussian, written by preprocess and gathered by the
// blend kernels with float4 loads:
//   f4[0] = { px, py, depth, bits(radius) }     pixel centre, view depth, int radius
//   f4[1] = { conic A, B, C, opacity }
//   f4[2..] = C blended feature channels, zero padded to a multiple of 4
__host__ __device__ constexpr int rec_vec4(int C) { return 2 + (C + 3) / 4; }   // float4 per record

// Packed per-list-entry record ("stream record") written by the forward pack and read by every blend kernel:
// 8 geometry floats (the last is the Gaussian id) + C features + depth, padded to float4 (layout: blend_fwd.hip).
__host__ __device__ constexpr int stream_vec4(int C) { return (8 + C + 1 + 3) / 4; }

// Blend-side layout (blend_fwd.hip): `sorted_rec` holds ONE packed record per entry of the sorted (Gaussian, tile)
// list that some quadrant of the tile can reach, COMPACTED: the k kept entries of a tile with list
// [start, start + n) sit at records start .. start + k - 1, depth order preserved (the other n - k slots of the
// tile's range stay unused).  `quad_list` holds, per tile, five regions of n u32 at 5*start: for each 8x8
// quadrant q the compact indices (0 .. k-1) of the entries that quadrant keeps, depth order preserved
// (5*start + q*n ...), and the position of every kept entry in the tile's FULL list (5*start + 4*n + compact index;
// read only by the n_contrib export).  The blend loops prefetch two indices past either end of a region
// (kQuadPad u32 of slack in front and behind) and clamp whatever they read to [0, k-1] before touching a record.
constexpr int kQuadPad = 16;
template <int C>
inline float4* stream_base(void* buf) { return static_cast<float4*>(buf); }
inline uint32_t* quad_base(void* buf) { return static_cast<uint32_t*>(buf) + kQuadPad; }
// A pixel that is finished (or outside the image) is parked at this x coordinate: its quadratic form
// becomes hugely negative, so the single candidate compare of the blend loops rejects it.
constexpr float kFar = 3.0e18f;
constexpr float kFarTest = 1.0e18f;

typedef float f8 __attribute__((ext_vector_type(8)));
// One stream record as the backward blend loops (blend_bwd.hip) hold it: loaded from a WAVE-UNIFORM address, so hipcc emits
// s_load_dwordx8 / s_load_dwordx4 and the fields live in SGPRs (operands of the per-pixel VALU math).  The forward walk
// (blend_fwd.hip) keeps its records in VGPRs instead.
template <int C>
struct StreamRec {
    static constexpr int NF4 = stream_vec4(C) - 2;
    f8 g;               // x, y, -A/2, -C/2, -B, h = -thr/2, opacity, Gaussian id (bit pattern)
    float4 f[NF4];      // features, then the view depth at slot C
    __device__ __forceinline__ void load(const float* __restrict__ p) {
        g = *reinterpret_cast<const f8*>(p);
#pragma unroll
        for (int k = 0; k < NF4; ++k) f[k] = *reinterpret_cast<const float4*>(p + 8 + 4 * k);
    }
    __device__ __forceinline__ float feat(int c) const {     // c must be a compile-time constant after unrolling
        const float4 v = f[c >> 2];
        return (c & 3) == 0 ? v.x : (c & 3) == 1 ? v.y : (c & 3) == 2 ? v.z : v.w;
    }
};

// Per-Gaussian gradient record accumulated by the backward blend: 16 slots (fp64: 128 B = two 64-byte halves, the
// granularity of the memory-side atomics; one lane group of 16 adds a whole record with one instruction):
//   [0..8]   dL/dfeature 0..8      [9] dL/ddepth
//   [10..15] pixel moments of q = opacity * G * dL/dalpha about the IMAGE ORIGIN: M0, MX, MY, MXX, MXY, MYY = sum over the
//            Gaussian's pixels (X, Y) of q * {1, X, Y, X^2, XY, Y^2} (round 4; round 2 / 3 shifted them to the Gaussian's
//            centre inside the blend kernel).  preprocess_bwd.hip re-centres them in fp64 (d = centre - pixel: S0, Sx, Sy,
//            Sxx, Sxy, Syy) and maps those to dL/dmean2D, dL/dconic, dL/dopacity
// (blend_bwd.hip: every slot is reduced on the matrix cores).
// Features-only backward (blend_backward_feat_lds_kernel): channels F0..C-1 sit at slots 0..C-F0-1 (first half only).
constexpr int kSlotDepth = 9, kSlotMoments = 10;
__host__ __device__ constexpr int grad_stride(int C) { return (C + 7 <= 16) ? 16 : 32; }
// features-only backward: the record of a Gaussian is its NS = C - F0 feature sums alone -- one 64-byte segment when they fit
// (half the bytes to clear before the pass and to read after it), the full stride otherwise
__host__ __device__ constexpr int feat_grad_stride(int C, int F0) { return (C - F0 <= 8) ? 8 : grad_stride(C); }

// ---- geometry scratch layout (shared by forward phases) ------------------------------------------
struct GeomState {      // kept until backward
    float4* rec;        // [P * rec_vec4(C)]
    uint32_t* clamped;  // [P] bit ch set when SH colour channel ch was clamped at 0
    static GeomState carve(void* p, int P, int C) {
        Carver c(p);
        GeomState g;
        g.rec = c.take<float4>((size_t)P * rec_vec4(C));
        g.clamped = c.take<uint32_t>(P);
        return g;
    }
    static size_t bytes(int P, int C) {
        Carver c(nullptr);
        c.take<float4>((size_t)P * rec_vec4(C));
        c.take<uint32_t>(P);
        return c.off;
    }
};

struct ImageState {     // kept until backward
    uint2* ranges;          // [tiles] range of the tile in the sorted list (reference-exact)
    uint32_t* n_contrib;    // [W*H] last contributor, as 1-based index into the pixel's QUADRANT stream
    uint32_t* qcount;       // [tiles*5] entries kept in each 8x8 quadrant stream (4) + records kept by the tile (1)
    float* final_T;         // [W*H] transmittance left after the last contributor, exactly as the forward loop held it.
                            // The upstream backward re-derives it as 1 - out_alpha (Appendix A.4), which in fp32 loses
                            // up to eps / T_final = 6e-4 relative on saturated pixels (T_final -> 1e-4) and scales every
                            // gradient of the pixel by that error; keeping the forward's own value costs 4 B/pixel.
    uint32_t* tile_order;   // [tiles] virtual tiles, heaviest list first: workgroup b of the pack / blend kernels takes tile
                            // tile_order[b] (launch_tile_order; the hardware hands workgroups out in index order, so the
                            // long lists start first and the short ones fill the tail of the launch)
    // G images of a grouped pass are G * tiles "virtual tiles": virtual tile vt = g * tiles + t
    static ImageState carve(void* p, int W, int H, int G = 1) {
        Carver c(p);
        ImageState s;
        const size_t tiles = (size_t)G * ((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile);
        s.ranges = c.take<uint2>(tiles);
        s.n_contrib = c.take<uint32_t>((size_t)G * W * H);
        s.qcount = c.take<uint32_t>(tiles * 5);
        s.final_T = c.take<float>((size_t)G * W * H);
        s.tile_order = c.take<uint32_t>(tiles);
        return s;
    }
    static size_t bytes(int W, int H, int G = 1) {
        Carver c(nullptr);
        const size_t tiles = (size_t)G * ((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile);
        c.take<uint2>(tiles);
        c.take<uint32_t>((size_t)G * W * H);
        c.take<uint32_t>(tiles * 5);
        c.take<float>((size_t)G * W * H);
        c.take<uint32_t>(tiles);
        return c.off;
    }    // the image state of a statistics pass (ogs_raster_forward_group_stats): tile ranges and workgroup order only -- nothing
    // per pixel, nothing kept for a backward
    static ImageState carve_stats(void* p, int W, int H, int G) {
        Carver c(p);
        ImageState s{};
        const size_t tiles = (size_t)G * ((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile);
        s.ranges = c.take<uint2>(tiles);
        s.tile_order = c.take<uint32_t>(tiles);
        return s;
    }
    static size_t stats_bytes(int W, int H, int G) {
        Carver c(nullptr);
        const size_t tiles = (size_t)G * ((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile);
        c.take<uint2>(tiles);
        c.take<uint32_t>(tiles);
        return c.off;
    }
};
// heaviest-first workgroup order of the per-tile kernels; returns the array the kernels index with blockIdx.x, or
// nullptr (identity) when the ordering is off (OGS_TILE_ORDER=0) or not worth a launch
// (P: a pass with fewer than four Gaussians per tile is all launch latency -- no ordering, one launch less)
const uint32_t* launch_tile_order(const ImageState& is, int64_t vtiles, int P, hipStream_t s, int debug);
const uint32_t* tile_order_of(const ImageState& is, int64_t vtiles, int P);      // what the forward of this pass used
int launch_export_n_contrib(const OgsRasterFwdArgs& a, const ImageState& is, uint32_t* out, hipStream_t s);

// radix sort / scan (radix_sort.hip) ------------------------------------------------------------
size_t scan_tmp_bytes(int64_t n);
size_t sort_tmp_bytes(int64_t n);                      // scratch of a whole sort of n keys, either implementation

// exclusive prefix sum of n uint32; if total != nullptr the grand total is written there (device).  `gather` (optional) makes
// element i = in[gather[i]].  in may equal out, with two limits, both refused with OGS_ERR_INVALID_ARG before anything is
// launched: not together with `gather` (element i would read a word another thread has already overwritten), and not together
// with `total` above 16384 x 2048 elements (the multi-level route takes the total from the last input, which is gone by then).
// tmp: scan_tmp_bytes(n) bytes; sort_tmp_bytes(n) >= scan_tmp_bytes(n), so a caller may lend it a sort's scratch.
// n_dev (optional): the element count lives in device memory, n is the capacity the launches are sized for; elements past the
// count read as zeros and their outputs are not written.
int exclusive_scan_u32(const uint32_t* in, const uint32_t* gather, uint32_t* out, int64_t n,
                       uint32_t* total, void* tmp, hipStream_t stream, int debug, const uint32_t* n_dev = nullptr);
// Stable LSD radix sort of n (key, value) pairs in npass digit passes, pass p on bits [shift[p], shift[p] + bits[p]) (1..4
// passes of 1..8 bits).  n is the element count, or -- when n_dev != nullptr -- the CAPACITY the launches are sized for while
// the kernels read the true count (<= capacity after clamping) from device memory.
// drop: keys equal to kDropKey are not part of the sort -- they are left out of the histograms and of the output of pass 0,
// which comes out COMPACTED and stores the number of keys it wrote to *kept (device, required), the element count of every
// later pass.  (The tile sort drops the (Gaussian, tile) pairs that cannot reach a pixel of their tile: duplicate_kernel.)
// impl: ThreeLaunch = histogram table, row scan and scatter per pass, nothing waits on another workgroup; OneLaunch = one
// launch per pass with decoupled look-back, fewer than 2^30 keys; BySize = OneLaunch up to 256 Ki keys (OGS_RADIX=legacy /
// sweep: never / wherever it can run).
constexpr uint32_t kDropKey = 0xFFFFFFFFu;
enum class RadixImpl { BySize, ThreeLaunch, OneLaunch };
struct RadixSort {
    uint32_t* keys[2]; uint32_t* vals[2];   // pass p reads [p & 1], writes [(p + 1) & 1]; result in [npass & 1]
    int64_t n; const uint32_t* n_dev;
    int npass; int shift[4]; int bits[4];
    bool drop; uint32_t* kept;
    void* tmp;                               // sort_tmp_bytes(n)
    RadixImpl impl = RadixImpl::BySize;
    int items = 0, spin_limit = -1;          // self-test hook only: a forced tile size of the one-launch passes (4 / 16), and the
                                             // bound of a look-back wait (0 trips it)
};
int radix_sort(const RadixSort&, hipStream_t, int debug);

// words of one run of GeomTmp::block_sum holding nb sums: padded, so that block_offsets_kernel loads both runs 16 bytes at a time
constexpr int kBlockSumPad = 8;
__host__ __device__ constexpr int block_sum_run(int nb) { return (nb + kBlockSumPad - 1) / kBlockSumPad * kBlockSumPad; }

struct GeomTmp {        // transient, but must survive from forward_geometry to forward_render
    uint32_t* tiles_touched;   // [P]
    uint32_t* keys[2];         // [P] depth bits ping-pong; keys[0] by Gaussian index as preprocess wrote it on the per-tile path
                               // (per_tile_depth_order: nothing sorts it, tile_depth_sort_kernel gathers from it)
    uint32_t* order[2];        // [P] Gaussian ids ping-pong; order[0] holds the depth order at the end (depth-sorted paths only)
    uint32_t* offsets;         // [P] exclusive scan of tiles_touched in the order duplicate walks (index or depth order); not
                               // written by a pass that takes its offsets from block_sum (block_sum_offsets)
    uint32_t* num_rendered;    // [64] word 0: num_rendered (sum of the reference rects); word 2: emitted(), below; word 1 (`visible()`, depth-sorted paths only): Gaussians in the depth
                               // order -- the culled ones (key kDropKey: behind the near plane, outside every group, empty tile
                               // rect) leave the depth sort in its first pass, so the later passes, the scan and duplicate only
                               // see what is drawn
    void* sort_tmp;
    uint32_t* block_sum;       // [2 block_sum_run(ceil(P / kBlock))] block-sum scheme (block_sum_offsets): preprocess leaves two sums per workgroup,
                               // first run: the tiles of its EMITTED rects (emit_rect), which block_offsets_kernel turns into their
                               // exclusive prefix in place and where the workgroup of duplicate_kernel with the same index starts
                               // its range; second run: the tiles of its reference rects, summed into num_rendered[0]
    uint2* emit_rect;          // [P] block-sum scheme: the tile rect duplicate_kernel expands for the Gaussian, x = min | max << 16 of
                               // the columns, y of the rows (max exclusive; all zero: nothing).  The reference rect cut down to the
                               // bounding box of the reach ellipse (preprocess_one, "8b"): never larger, so the count of emitted
                               // pairs, word kEmittedWord of num_rendered, is at most the reported num_rendered
    static constexpr int kEmittedWord = 2;
    uint32_t* visible() const { return num_rendered + 1; }
    // how many (Gaussian, tile) pairs duplicate_kernel writes: what the render phase's kernels read as their key count on a
    // block-sum pass; on every other pass the pairs are the reference rects' and num_rendered[0] is that count
    uint32_t* emitted() const { return num_rendered + kEmittedWord; }
    static GeomTmp carve(void* p, int P) {
        Carver c(p);
        GeomTmp g;
        g.tiles_touched = c.take<uint32_t>(P);
        g.keys[0] = c.take<uint32_t>(P);
        g.keys[1] = c.take<uint32_t>(P);
        g.order[0] = c.take<uint32_t>(P);
        g.order[1] = c.take<uint32_t>(P);
        g.offsets = c.take<uint32_t>(P);
        g.num_rendered = c.take<uint32_t>(64);
        g.sort_tmp = c.take<char>(sort_tmp_bytes(P));
        g.block_sum = c.take<uint32_t>(2 * (size_t)block_sum_run((P + kBlock - 1) / kBlock));
        g.emit_rect = c.take<uint2>(P);
        return g;
    }
    static size_t bytes(int P) {
        Carver c(nullptr);
        for (int i = 0; i < 6; ++i) c.take<uint32_t>(P);
        c.take<uint32_t>(64);
        c.take<char>(sort_tmp_bytes(P));
        c.take<uint32_t>(2 * (size_t)block_sum_run((P + kBlock - 1) / kBlock));
        c.take<uint2>(P);
        return c.off;
    }
};

struct BinTmp {         // transient, render phase
    uint32_t* tile_keys[2];    // [D]
    uint32_t* vals;            // [D] ping buffer (the pong is args->point_list)
    uint32_t* kept;            // [1] pairs left after the first pass of the tile sort dropped the unreachable ones
    void* sort_tmp;
    static BinTmp carve(void* p, int64_t D) {
        Carver c(p);
        BinTmp b;
        b.tile_keys[0] = c.take<uint32_t>(D);
        b.tile_keys[1] = c.take<uint32_t>(D);
        b.vals = c.take<uint32_t>(D);
        b.kept = c.take<uint32_t>(1);
        b.sort_tmp = c.take<char>(sort_tmp_bytes(D));
        return b;
    }
    static size_t bytes(int64_t D) {
        Carver c(nullptr);
        for (int i = 0; i < 3; ++i) c.take<uint32_t>(D);
        c.take<uint32_t>(1);
        c.take<char>(sort_tmp_bytes(D));
        return c.off;
    }
};

// kernels launched by capi.hip ------------------------------------------------------------------
// raw (here and in the two single-workgroup launchers below): the raw-model form of the kernel (include/ogs_model.h); the
// pointer slots of `a` then hold the raw arrays (capi.hip::raw_fwd_args)
int launch_preprocess(const OgsRasterFwdArgs& a, const GeomState& gs, const GeomTmp& gt, hipStream_t s, bool raw = false);
// block-sum scheme: gt.block_sum (per preprocess workgroup, emitted tiles | reference tiles) -> exclusive prefix of the emitted sums
// in place, their total -> gt.emitted(), the reference total -> gt.num_rendered[0]; one workgroup
int launch_block_offsets(const OgsRasterFwdArgs& a, const GeomTmp& gt, hipStream_t s);
int launch_tiny_geometry(const OgsRasterFwdArgs& a, const GeomState& gs, uint32_t* order, hipStream_t s, bool raw = false);
int launch_small_geometry(const OgsRasterFwdArgs& a, const GeomState& gs, const GeomTmp& gt, hipStream_t s, bool raw = false);
int launch_model_activate(int P, int M, const OgsRawModel& raw, float* scales, float* rotations, float* opacities, float* shs,
                          hipStream_t s);
int launch_tiny_blend(const OgsRasterFwdArgs& a, const GeomState& gs, const uint32_t* order, hipStream_t s);
// re-blend of a kept pass with new feature channels: ONE launch of the stand-alone forward blend, which takes the replaced
// channels from the caller's per-Gaussian features while it gathers the kept records (blend_forward_rows_kernel<C, RF>)
int launch_reblend(const OgsRasterFwdArgs& a, const ImageState& is, hipStream_t s);
// a finished pass' records and quadrant streams re-laid out by the ranges of what each tile packed (blend_fwd.hip)
int launch_compact_kept(int W, int H, int C, const ImageState& is_old, const ImageState& is_new, const void* old_rec,
                        const void* old_quad, void* new_rec, void* new_quad, hipStream_t s);
// zero_ranges / n_zero (optional, n_zero <= P): the kernel also clears that many tile ranges (then launch_tile_ranges is told so)
// depth_order: walk the Gaussians in the depth order of the geometry phase (order[0], visible() of them); otherwise in index
// order, all P (per_tile_depth_order)
int launch_duplicate(const OgsRasterFwdArgs& a, const GeomState& gs, const GeomTmp& gt, uint32_t* tile_keys,
                     uint32_t* vals, uint32_t capacity, bool drop_unreachable, bool depth_order, hipStream_t s,
                     uint2* zero_ranges = nullptr, int n_zero = 0);
int launch_tile_ranges(const uint32_t* tile_keys_sorted, int64_t D, uint2* ranges, int64_t tiles, hipStream_t s,
                       int debug, const uint32_t* n_dev = nullptr, bool already_zeroed = false);
// Counting sort by tile (binning.hip, "tile count" path): what replaces the radix tile sort and launch_tile_ranges on a default
// streaming pass (block_sum_offsets) whose grid fits the LDS histogram.  keys / vals: what duplicate_kernel wrote, n_dev of them
// (at most D); table: (B + 1) * tiles <= D words of scratch; out: ranges (every tile written, (0, 0) when empty), kept, and point_list
// with every tile's values in its range, in no particular order -- launch_tile_depth_sort orders ties by id itself.
constexpr int kTileCountMaxTiles = 12288;      // 48 KB of LDS counters / cursors per workgroup
constexpr int kTileCountBlocks = 128;          // chunks (workgroups of 1024 threads; DESIGN 3h has the sweep), unless the list or the table is too short for as many
int tile_count_blocks(int64_t D, int64_t tiles);           // B for this pass; 0: the radix path
int tile_count_trip();
void tile_count_debug(int force_blocks, int reverse);      // test hooks; a negative argument leaves its setting as it is
// tile_place_kernel's grid for a pass of B count chunks: `chunks` = ceil(B / group) place chunks of `group` count chunks each, times
// `slices` slices of the tiles; stage_words of LDS per workgroup for the runs it writes out in slot order (0: none, every pair is
// stored from the walk).  All zero when B < 1.
struct TilePlacePlan { int group, chunks, slices; uint32_t stage_words; };
TilePlacePlan tile_place_plan(int64_t D, int64_t tiles, int B);
void tile_place_debug(int group, int slices, int stage_words);   // test hooks; > 0 forces, 0 hands back, < 0 leaves as it is
int launch_tile_count_binning(const uint32_t* keys, const uint32_t* vals, int64_t D, const uint32_t* n_dev, int B, int64_t tiles,
                              uint32_t* table, uint2* ranges, uint32_t* kept, uint32_t* point_list, hipStream_t s, int debug);
// Ungrouped streaming passes with P > kSmallMaxP bin without a global depth sort: the geometry phase scans tiles_touched in
// Gaussian-index order, duplicate walks the Gaussians in that order, and after the pairs are grouped by tile every tile's list
// is sorted by (depth, id) on its own (launch_tile_depth_sort: whatever order the list arrives in).  Grouped passes and the small path keep the depth order of the P
// Gaussians.  Decided from the arguments alone, so that the geometry and the render phase of a pass agree.
inline bool per_tile_depth_order(const OgsRasterFwdArgs& a) { return a.num_groups <= 1 && a.P > kSmallMaxP; }
// The default-mode passes among those need no scan over the P Gaussians either: preprocess_kernel and duplicate_kernel cut the
// Gaussians into the same 256-wide workgroups, so preprocess leaves one sum of emitted tiles per workgroup, one small launch
// turns the sums into offsets, and every workgroup of duplicate scans its own 256 counts in LDS.  These are also the passes
// whose pairs come from the reach ellipse's rect (GeomTmp::emit_rect) instead of the reference's: the count of pairs is then
// gt.emitted(), below the reported num_rendered.  A full_binning pass (the parity export) keeps the reference rects, the scan
// and offsets[].  Also decided from the arguments alone.
inline bool block_sum_offsets(const OgsRasterFwdArgs& a) { return per_tile_depth_order(a) && a.full_binning == 0; }
// Every tile's segment of point_list into (depth key, id) order in place, keys gathered by id from depth_keys (the 32-bit keys
// preprocess wrote); workgroup b takes tiles tile_order[4b .. 4b+3] (b.. when NULL).  Lists up to kWaveSortCap entries are sorted by
// one wave, up to kTileSortCap by the workgroup in LDS; longer ones run their passes through the same positions of `scratch`
// (D entries, free after the tile sort).  Equal keys come out in id order whether or not they arrived so.
constexpr int kTileSortItems = 16;
constexpr int kTileSortCap = kBlock * kTileSortItems;       // 4096 entries: 32 KB of keys + values, 4 workgroups per CU
constexpr int kWaveSortCap = kTileSortCap / (kBlock / kWave);   // 1024: lists one wave sorts alone (a quarter of that space)
// One-wave lists: a bucket pass on the top 8 bits of the list's key range and a ranking inside each bucket, unless the list's
// largest bucket holds more than the cap (clustered depths, many equal keys): such a list takes the stable LSD passes.  The
// crossover of the two lies between 32 and 64 entries for lists of 512 and of 1024 (DESIGN 3j has the sweep).
constexpr int kWaveBucketCap = 32;
void tile_sort_debug(int bucket_cap);                      // test hook; > 0 forces the cap, 0 hands back, < 0 leaves as it is
int tile_sort_bucket_cap();                                // the cap in force
int launch_tile_depth_sort(const uint2* ranges, int64_t tiles, const uint32_t* tile_order, uint32_t* point_list,
                           const uint32_t* depth_keys, uint32_t* scratch, hipStream_t s, int debug);
inline int num_groups_of(int g) { return g > 1 ? g : 1; }
// order_ready: the render phase already ran launch_tile_order for this pass (per-tile depth sort), the kernels reuse it
int launch_group_stats(const OgsRasterFwdArgs& a, const OgsGroupStatsArgs& st, const GeomState& gs, const ImageState& is,
                       hipStream_t s, bool order_ready = false);
int launch_blend_forward(const OgsRasterFwdArgs& a, const GeomState& gs, const ImageState& is, int64_t D,
                         hipStream_t s, bool order_ready = false);
// The per-Gaussian gradient record is accumulated in fp64 (128 B = one L2 line): with thousands of float atomics per
// large Gaussian, arriving in a different order every run and cancelling against each other, an fp32 running sum made
// the gradients differ run to run by ~1e-4 of their maximum (GPUTEST_r01: rotations at S1M); the fp64 sum is
// order-insensitive to ~1e-16 and is rounded to fp32 ONCE, in preprocess_backward_kernel.  (Round 4: the fp32 record of
// OGS_GRAD_ACCUM=f32 is gone -- the moment slots are sums about the image origin now and NEED the fp64 headroom.)
int launch_blend_backward(const OgsRasterBwdArgs& a, const ImageState& is, void* grad_rec, hipStream_t s);
// raw_grads != NULL: the raw-model form (include/ogs_model.h) -- `a` holds the raw arrays in its pointer slots and the dense SH
// gradient goes to raw_grads->features_dc / features_rest (capi.hip::ogs_raster_backward_raw)
int launch_preprocess_backward(const OgsRasterBwdArgs& a, const GeomState& gs, const void* grad_rec, hipStream_t s,
                               const OgsRawModelGrads* raw_grads = nullptr);
// Only dL/dcolors_precomp is requested (every other output pointer NULL): the stage >= 1 training graph
// (train.py:431-436) -> features-only kernels.
// Camera gradients (pose_bwd.hip) are asked for: they need the geometry slots of the record, so such a pass is never features-only.
inline bool backward_wants_pose(const OgsRasterBwdArgs& a) { return a.dL_dviewmatrix || a.dL_dprojmatrix || a.dL_dcampos; }
inline bool backward_is_features_only(const OgsRasterBwdArgs& a) {
    return a.dL_dcolors != nullptr && a.colors_precomp != nullptr && !a.dL_dmeans2D && !a.dL_dopacity &&
           !a.dL_dmeans3D && !a.dL_dcov3D && !a.dL_dsh && !a.dL_dscales && !a.dL_drotations && !a.dL_dsh_rgb &&
           !backward_wants_pose(a);
}
// the two camera-gradient launches (partials per workgroup into a.pose_tmp, then one workgroup folds them into the 35 floats);
// P == 0: the fold alone, which writes zeros.  raw: `a` holds the raw model in its pointer slots, as launch_preprocess_backward
int launch_pose_backward(const OgsRasterBwdArgs& a, const GeomState& gs, const void* grad_rec, hipStream_t s, bool raw);
size_t pose_tmp_bytes(int P);
int pose_partial_chunk();
int launch_sh_grad_from_views(int P, int V, int sh_degree, int sh_coeffs, const float* means3D, const float* campos,
                              const float* dL_drgb, float* dL_dsh, hipStream_t s);
int launch_wave_fold16_test(const float* in, float* out, hipStream_t s);
int launch_mfma_rank1_test(const float* w, const float* f, const float* acc0, int steps, float* out_mfma, float* out_fma,
                           hipStream_t s);
int launch_tile_order_test(const uint32_t* ranges, int64_t vtiles, uint32_t* order, hipStream_t s);
int launch_mark_visible(int P, const float* means3D, const float* viewmatrix, uint8_t* present, hipStream_t s);
int launch_export_keys(const uint2* ranges, int tiles, const uint32_t* point_list, const float4* rec, int recv4,
                       uint64_t* keys_out, hipStream_t s);

// ---- blend arithmetic shared by every kernel that evaluates a Gaussian at a pixel ----------------------------------
// power = a2*dx^2 + b2*dx*dy + c2*dy^2 (a2 = -A/2, b2 = -B, c2 = -C/2) in ONE fixed operation order with explicit
// FMAs.  The forward, both backward variants and the tiny pass must reproduce the same bits: a pixel's skip
// decisions (alpha >= 1/255, T < 1e-4) are re-taken by the backward pass from the recomputed alpha, and left to the
// compiler the contraction of this expression differed from kernel to kernel (SGPR vs LDS operands).
__device__ __forceinline__ float blend_power(float a2, float b2, float c2, float dx, float dy) {
    const float u = fmaf(b2, dy, a2 * dx);         // a2*dx + b2*dy
    return fmaf(c2 * dy, dy, u * dx);              // (a2*dx + b2*dy)*dx + c2*dy^2
}

// ---- record prefetch of the blend kernels --------------------------------------------------------------------------
// The backward blend loops (blend_bwd.hip) read the tile's record stream through the SCALAR path, two batches in flight per
// wave: with the stream coming from HBM (far larger than L2) the loops are bound by the latency of those scalar loads, not
// by VALU issue.  At kernel entry the four waves of a tile therefore touch every 128-byte line of the tile's record range
// with plain vector loads -- all issued at once, never waited for until the kernel's last instruction -- which pulls the
// range towards the XCD's L2 ahead of the loads that need it.  The stand-alone forward blend (blend_forward_rows_kernel)
// does the same ahead of its per-lane vector gathers.
// `lines` = 128-byte lines per thread (0: off; tuning knob OGS_BLEND_PREFETCH), `sink` is opaque to the compiler.
constexpr int kPrefetchMax = 4;
struct RecordPrefetch {
    uint32_t v[kPrefetchMax];
    __device__ __forceinline__ void issue(const float* __restrict__ tile_records, int n_tile, int rec_floats, int tid,
                                          int lines) {
        const uint32_t total = (uint32_t)n_tile * (uint32_t)rec_floats;          // floats in the tile's range
#pragma unroll
        for (int k = 0; k < kPrefetchMax; ++k) {
            v[k] = 0u;
            const uint32_t off = ((uint32_t)(k * kBlock + tid)) * 32u;            // one 128-byte line per thread and round
            if (k < lines && off < total) v[k] = __float_as_uint(tile_records[off]);
        }
    }
    // keeps the loads alive without ever waiting for them inside the loop: folded into a store that cannot happen
    __device__ __forceinline__ void retire(uint32_t* __restrict__ sink, int never) const {
        const uint32_t x = v[0] ^ v[1] ^ v[2] ^ v[3];
        if (never < 0 && x == 0x7FC12345u) sink[0] = x;
    }
};
int blend_prefetch_lines();     // capi.hip: OGS_BLEND_PREFETCH (default kPrefetchMax)

// ---- can a Gaussian reach a pixel box? ------------------------------------------------------------------------------
// Candidate window of the blend loops: thr <= power <= 0 with thr = ln(1 / (255 * opacity)) - kThrMargin, i.e. alpha can
// reach 1/255 (the margin absorbs the rounding differences between this test and the blend kernels' own evaluation of
// the power).  duplicate_kernel (preprocess_fwd.hip) tests the whole 16x16 tile once per (Gaussian, tile) pair and
// flags the pair in the top bit of the sorted value; pack_blend_chunked_kernel (blend_fwd.hip) tests the four 8x8 quadrants
// of the flagged pairs.
constexpr float kThrMargin = 0.01f;
constexpr int kReachBit = 31;                           // Gaussian ids are < 2^31
constexpr uint32_t kGidMask = (1u << kReachBit) - 1u;
// max over the box d in [xlo,xhi] x [ylo,yhi] of  -0.5*(A dx^2 + C dy^2) - B dx dy   (A, C > 0, AC - B^2 > 0)
// nbA = -B / A, nbC = -B / C: the slopes of the 1-D maximisers (per Gaussian, so a caller with many boxes divides once)
// The result is an UPPER bound that also covers fp32 rounding: for a needle-shaped Gaussian far from its centre the terms
// A dx^2, C dy^2, 2 B dx dy reach 1e5 .. 1e6 while their sum is O(1) -- the cancellation error of this evaluation AND of the
// blend kernels' own evaluation of the power at a pixel (each a few ulp of the largest term) can exceed the fixed
// kThrMargin.  Slack: 8e-7 x the largest possible term magnitude over the box.
__device__ __forceinline__ float max_power_in_box(float A, float B, float Cc, float nbA, float nbC, float xlo, float xhi,
                                                  float ylo, float yhi) {
    if (xlo <= 0.f && xhi >= 0.f && ylo <= 0.f && yhi >= 0.f) return 0.f;
    auto q = [&](float dx, float dy) { return -0.5f * (A * dx * dx + Cc * dy * dy) - B * dx * dy; };
    // concave form, origin outside the box: the maximum sits on an edge, at the clamped 1-D maximiser
    float m = q(xlo, fminf(fmaxf(nbC * xlo, ylo), yhi));
    m = fmaxf(m, q(xhi, fminf(fmaxf(nbC * xhi, ylo), yhi)));
    m = fmaxf(m, q(fminf(fmaxf(nbA * ylo, xlo), xhi), ylo));
    m = fmaxf(m, q(fminf(fmaxf(nbA * yhi, xlo), xhi), yhi));
    const float X = fmaxf(fabsf(xlo), fabsf(xhi)), Y = fmaxf(fabsf(ylo), fabsf(yhi));
    return m + 8e-7f * (0.5f * (A * X * X + Cc * Y * Y) + fabsf(B) * X * Y);
}
__device__ __forceinline__ float max_power_in_box(float A, float B, float Cc, float xlo, float xhi, float ylo,
                                                  float yhi) {
    return max_power_in_box(A, B, Cc, -B / A, -B / Cc, xlo, xhi, ylo, yhi);
}

// ---- tiny device helpers ------------------------------------------------------------------------
// s_waitcnt lgkmcnt(0) (vmcnt / expcnt untouched), pinned in place: nothing is scheduled across it
__device__ __forceinline__ void wait_scalar_loads() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ int lane_id() { return threadIdx.x & (kWave - 1); }
// Workgroup barrier that orders LDS traffic ONLY.  __syncthreads() is a workgroup-scope fence as well: the compiler puts
// s_waitcnt vmcnt(0) in front of it, i.e. every wave first waits for ITS outstanding global stores and atomics to complete --
// 1-3 us under load, per barrier.  The chunked forward (record write-out for the backward) and the merged backward (the
// windows' fp64 atomics) issue global writes that nothing in the kernel reads back; the waves only hand LDS contents to each
// other.  (Round 4: with __syncthreads() the merged backward was SLOWER than the unmerged one, 0.658 vs 0.616 ms.)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

}  // namespace ogs
