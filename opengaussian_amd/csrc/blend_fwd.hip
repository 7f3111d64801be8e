// Forward front-to-back alpha blend for gfx950 over per-quadrant compacted index streams.
//
// Measured on the bench scene, only 48 % of the reference's (Gaussian, tile) list entries can reach alpha >= 1/255 on ANY
// pixel of their tile and only 28 % of the (entry, 8x8 quadrant) pairs: the reference's tile rect is the square around
// ceil(3 sigma_max).  So a pass PACKS each tile's sorted list before it blends it:
//   * pack: an EXACT conservative test per 8x8 quadrant (maximum of the Gaussian's quadratic form over the quadrant's pixel
//     box vs ln(1/(255*opacity)) - margin); a surviving entry gathers its record and writes ONE packed copy at its
//     compact position, and its compact index is appended to the index stream of every quadrant it can reach.  Depth
//     order inside a stream is preserved with a block-wide prefix sum over per-quadrant counters packed in one u64.  The
//     reference-visible binning state (sorted keys, point list, tile ranges) is untouched and stays bit-exact; dropped
//     entries are exactly those every lane of the quadrant would have skipped.
//   * blend: each wave64 owns one quadrant and walks its index stream in sub-chunks of 64 entries, per 4x4 pixel block, with
//     every operand of the per-pixel arithmetic in VGPRs.
// The walk exists ONCE, as QuadWalk<C>: the per-pixel state, the arithmetic of one (pixel, entry) pair, the sub-chunk step and
// the image epilogue.  Two kernels feed it 64 records at a time in LDS:
//   * pack_blend_chunked_kernel packs a tile chunk by chunk in one workgroup, blends each chunk straight from its staging
//     buffer, and stops when every pixel is done (the default forward, and the statistics pass);
//   * blend_forward_rows_kernel gathers records that are already packed: a pass with an empty list, and the re-blend of a
//     kept pass.
// Both therefore give the same bits on the same streams.  DESIGN.md section 3 has the history of this design and of the
// kernels it replaced.
// No MFMA: the recurrence (T, the stop) is per pixel, and the one part of a step that IS a product -- the rank-one update
// sums[pixel][channel] += w[pixel] * f[channel] per 4x4 block -- was built on v_mfma_f32_16x16x1_4b_f32 and measured slower than
// the packed FMAs it replaced (rank1_update below).
#include "ogs_common.h"

namespace ogs {

namespace {

constexpr float kAlphaMin = 1.0f / 255.0f;
typedef float v2f __attribute__((ext_vector_type(2)));   // register pair -> v_pk_fma_f32

__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int d) {
    const uint32_t lo = __shfl_up((uint32_t)v, d, kWave), hi = __shfl_up((uint32_t)(v >> 32), d, kWave);
    return ((uint64_t)hi << 32) | lo;
}

// blend record (one per tile-list entry that reaches some quadrant, at the entry's list position):
//   [0] x  [1] y  [2] -0.5*A  [3] -0.5*C  [4] -B  [5] h=-thr/2  [6] opacity  [7] Gaussian id (bit pattern)
//   (round 4: -0.5*C moved next to -0.5*A -- (x, y) and (-A/2, -C/2) are even-aligned pairs, so the quadrant walks form the
//   pixel offset and the two products a2*dx, c2*dy with ONE packed instruction each)
//   [8..8+C) features  [8+C] view depth, rest zero padding to a multiple of 4 floats.
// The depth sits right behind the features so that the (feature, feature) / (feature, depth) operand pairs of
// the blend loops' packed FMAs are even-aligned pairs (no shuffles).
template <int C>
struct RowRec {          // one record in VGPRs
    static constexpr int NV4 = stream_vec4(C);
    float4 v[NV4];
    __device__ __forceinline__ void load_lds(const float4* __restrict__ p) {
#pragma unroll
        for (int k = 0; k < NV4; ++k) v[k] = p[k];
    }
    __device__ __forceinline__ float at(int i) const {      // i compile-time after unrolling
        const float4 q = v[i >> 2];
        return (i & 3) == 0 ? q.x : (i & 3) == 1 ? q.y : (i & 3) == 2 ? q.z : q.w;
    }
    __device__ __forceinline__ float feat(int c) const { return at(8 + c); }
};

// the record a finished row keeps reading: h < 0 makes |power + h| <= h false for every pixel
template <int C>
__device__ __forceinline__ void write_dummy_record(float4* __restrict__ slot) {
#pragma unroll
    for (int k = 0; k < stream_vec4(C); ++k) slot[k] = float4{0.f, 0.f, 0.f, 0.f};
    slot[1] = float4{0.f, -1.f, 0.f, 0.f};                    // fields 4..7: b2, h = -1, opacity, id
}

constexpr int kRowListLen = 72;              // 64 sub-chunk entries + slack for the two-ahead index reads

// ---- the quadrant walk ------------------------------------------------------------------------------------------------
// A wave owns an 8x8 quadrant and takes its index stream in SUB-CHUNKS of 64 entries whose records sit in LDS.  (Walking it one
// entry at a time with the record in SGPRs keeps ~51 % of the lanes busy and pays 4 issue cycles for nearly every vector
// instruction: profiles/r03_valu_issue_price_list.json, any SGPR operand halves the issue rate.)  One step():
//   1. lane e tests record e of the sub-chunk against the four 4x4 blocks of the quadrant (the exact box-vs-ellipse test of
//      pack, on a 4x4 box);
//   2. four ballots + prefix popcounts turn the test bits into four compacted lists (LDS), one per DPP row;
//   3. the four rows of the wave -- row r = the 16 pixels of block r -- walk THEIR lists side by side: per trip a row reads its
//      next two records from LDS into VGPRs (four different records per ds_read_b128, one LDS cycle per row) and every operand
//      of the per-pixel arithmetic is a VGPR;
//   4. the pixel's last contributor in the sub-chunk becomes its stream index (settle).
// A skipped (entry, block) pair is one every pixel of the block would have skipped.  n_contrib is the 1-based position of
// the pixel's last contributor in the QUADRANT stream (the backward walks the same streams).  A finished or outside pixel is
// parked far away (fxe = kFar): its power becomes hugely negative and the candidate compare fails, so no `done` flag enters
// the per-pixel arithmetic.
template <int C>
struct QuadWalk {
    static constexpr int NPF = (C + 2) / 2;
    static constexpr uint32_t kNoEntry = 0xFFFFFFFFu;
    float fxe, fy, T, wacc;
    v2f accp[NPF];           // channels 0..C-1, then the depth
    uint32_t last;           // 1-based stream index of the pixel's last contributor (n_contrib)
    uint32_t last_e;         // list entry of the pixel's last contributor in the current sub-chunk
    // pixels still blending, as a wave-uniform 64-bit mask (an SGPR pair: a `bool all_done` went through a VGPR and back on every
    // walk step); a quadrant outside the image starts with none and its feeder skips the stream
    uint64_t alive;

    __device__ __forceinline__ void init(int px, int py, bool inside) {
        fxe = inside ? (float)px : kFar;
        fy = (float)py;
        T = 1.0f;
        wacc = 0.f;
#pragma unroll
        for (int k = 0; k < NPF; ++k) accp[k] = (v2f){0.f, 0.f};
        last = 0;
        last_e = kNoEntry;
        alive = __ballot(inside);
    }

    __device__ __forceinline__ void consume(const RowRec<C>& r, uint32_t entry) {
        // blend_power(a2, b2, c2, dx, dy) with its subtractions and its first two products as PACKED operations on the record's
        // register pairs (x, y) and (a2, c2) -- v_pk_add_f32 / v_pk_mul_f32: one issue slot for two results, and this walk is
        // bound by vector issue.  Same operations, same roundings, same bits as blend_power() (ogs_common.h)
        const v2f d = (v2f){r.at(0), r.at(1)} - (v2f){fxe, fy};
        const v2f m = (v2f){r.at(2), r.at(3)} * d;                  // a2 * dx, c2 * dy
        const float u = fmaf(r.at(4), d.y, m.x);                    // a2*dx + b2*dy
        const float power = fmaf(m.y, d.y, u * d.x);
        const float h = r.at(5);
        const bool cand = fabsf(power + h) <= h;
        if (__ballot(cand) != 0ull) {
            // straight-line for all 64 lanes (no exec-mask region: a lane that is no candidate gets alpha = 0, which leaves
            // every one of its accumulators, its T and its `last` untouched -- w = 0, test_T = T >= 1e-4)
            const float araw = fminf(0.99f, r.at(6) * __expf(power));
            const bool act = cand && araw >= kAlphaMin;
            const float alpha = act ? araw : 0.f;
            const float test_T = T * (1.0f - alpha);
            const bool stop = test_T < 0.0001f;
            float w = alpha * T;
            // the pixel's last contributor: this entry iff it contributes, w > 0 <=> act && !stop (alpha >= 1/255, T >= 1e-4).
            // The condition is a lane mask the step already has (SGPR pair), and what is recorded is the step's LIST ENTRY as it
            // sits in a VGPR (slot << 16 | LDS offset) -- one select per step; it becomes the stream index once per sub-chunk
            // (settle), instead of an index add, a compare and a select per step
            bool contributes = act;
            // a pixel saturates once: the three selects of the stop (weight, T, parking) only run in a step in which some lane
            // stops; every other step takes the values straight (same bits: the selects would have picked them)
            if (__ballot(stop) != 0ull) {
                w = stop ? 0.f : w;
                T = stop ? T : test_T;
                fxe = stop ? kFar : fxe;
                alive = __ballot(fxe < kFarTest);
                contributes = act && !stop;
            } else {
                T = test_T;
            }
            const v2f w2 = {w, w};
#pragma unroll
            for (int k = 0; k < NPF; ++k)
                accp[k] = __builtin_elementwise_fma((v2f){r.feat(2 * k), r.feat(2 * k + 1)}, w2, accp[k]);
            wacc += w;
            last_e = contributes ? entry : last_e;
        }
    }

    // One sub-chunk: lane e < 64 holds entry e of it.  g0, g1: the two geometry float4 of the lane's record; have: the lane has an
    // entry; rec_off: byte offset of the lane's record from `recs` (the LDS staging; every record of the sub-chunk is there, or
    // is parked there before the fence below by the lane that holds it); dummy: the list entry of the dummy record; s_list: the
    // wave's four lists, mylist = s_list[this lane's row]; (bx0, by0): the quadrant's origin; jbase: 1-based stream index of the
    // sub-chunk's entry 0.  A list entry = sub-chunk slot << 16 | rec_off of the slot's record (no multiply in the walk).
    __device__ __forceinline__ void step(const float4 g0, const float4 g1, bool have, uint32_t rec_off, uint32_t dummy,
                                         uint32_t (&s_list)[4][kRowListLen], const uint32_t* mylist, const float4* recs,
                                         float bx0, float by0, uint32_t jbase, int lane) {
        bool reach[4];
        {
            const float gxp = g0.x, gyp = g0.y;
            const float A = -2.f * g0.z, B = -g1.x, Cc = -2.f * g0.w, thr = -2.f * g1.y;
            const float nbA = -B / A, nbC = -B / Cc;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const float ox = bx0 + 4.f * (float)(b & 1), oy = by0 + 4.f * (float)(b >> 1);
                const float m = max_power_in_box(A, B, Cc, nbA, nbC, gxp - ox - 3.f, gxp - ox, gyp - oy - 3.f, gyp - oy);
                reach[b] = have && m >= thr;
            }
        }
        // four compacted lists (row b's list: sub-chunk slots that can reach block b), padded with the dummy
#pragma unroll
        for (int b = 0; b < 4; ++b) s_list[b][lane] = dummy;
        if (lane < kRowListLen - kWave) {
#pragma unroll
            for (int b = 0; b < 4; ++b) s_list[b][kWave + lane] = dummy;
        }
        int maxlen = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint64_t mask = __ballot(reach[b]);
            const int pos = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            if (reach[b]) s_list[b][pos] = ((uint32_t)lane << 16) | rec_off;
            maxlen = max(maxlen, (int)__popcll(mask));
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // the four rows walk their lists; records in two register sets, indices two steps ahead
        RowRec<C> ra, rb;
        auto rec_of = [&](uint32_t e) {
            return reinterpret_cast<const float4*>(reinterpret_cast<const char*>(recs) + (e & 0xFFFFu));
        };
        uint32_t e0 = mylist[0], e1 = mylist[1];
        ra.load_lds(rec_of(e0));
        for (int t = 0; t < maxlen && alive != 0ull; t += 2) {
            const uint32_t e2 = mylist[t + 2], e3 = mylist[t + 3];
            rb.load_lds(rec_of(e1));
            consume(ra, e0);
            ra.load_lds(rec_of(e2));
            if (t + 1 < maxlen) consume(rb, e1);
            e0 = e2; e1 = e3;
        }
        // settle: list entry -> 1-based index into the quadrant stream (entry's slot in the sub-chunk + what came before)
        if (last_e != kNoEntry) last = jbase + (last_e >> 16);
        last_e = kNoEntry;
        __builtin_amdgcn_wave_barrier();       // the lists and the staging may be rewritten
    }

    __device__ __forceinline__ float sum(int c) const { return (c & 1) ? accp[c / 2].y : accp[c / 2].x; }      // c <= C: depth
    __device__ __forceinline__ float colour(int c, const float* __restrict__ bg) const { return sum(c) + T * bg[c]; }

    // image epilogue of a pixel inside the image
    __device__ __forceinline__ void write_pixel(int img, int W, int H, int px, int py, const float* __restrict__ bg,
                                                float* __restrict__ out_color, float* __restrict__ out_depth,
                                                float* __restrict__ out_alpha, uint32_t* __restrict__ n_contrib,
                                                float* __restrict__ final_T) const {
        const size_t plane = (size_t)W * H;
        const size_t pix = (size_t)img * plane + (size_t)py * W + px;
        float* oc = out_color + (size_t)img * (C - 1) * plane;
#pragma unroll
        for (int c = 0; c < C; ++c) oc[c * plane + pix] = colour(c, bg);
        out_depth[pix] = sum(C);
        out_alpha[pix] = wacc;
        n_contrib[pix] = last;
        final_T[pix] = T;
    }
};

// ---- stand-alone blend of streams that are already packed ---------------------------------------------------------------
// Per sub-chunk, lane e gathers record e through the quadrant's index stream with vector loads (L2 hits: the prefetch at kernel
// entry pulled the tile's records in) and parks it in the wave's LDS region for QuadWalk::step.
// RF >= 0 (re-blend of a kept pass, ogs_raster_forward_reblend): channels [RF, C) of every record come from the caller's CURRENT
// per-Gaussian features `feats` [P, C - RF] instead of the record -- the lane that gathers a record fetches its Gaussian's row
// (slot 7 of the record is the id) on the way into LDS; the kept records are never written.
template <int C>
struct RowsLds {
    float4 s_rec[kBlock / kWave][(kWave + 1) * stream_vec4(C)];      // per wave: 64 sub-chunk records + the dummy
    uint32_t s_list[kBlock / kWave][4][kRowListLen];
};

template <int C, int RF = -1>
__global__ __launch_bounds__(kBlock) void blend_forward_rows_kernel(
    const uint2* __restrict__ ranges, const uint32_t* __restrict__ qcount, const float* __restrict__ stream,
    const uint32_t* __restrict__ quad_list, int W, int H, int gx, int tiles, const float* __restrict__ bg, float* __restrict__ out_color,
    float* __restrict__ out_depth, float* __restrict__ out_alpha, uint32_t* __restrict__ n_contrib,
    float* __restrict__ final_T, int pf_lines, const uint32_t* __restrict__ tile_order, const float* __restrict__ feats) {
    constexpr int NV4 = stream_vec4(C);
    constexpr int RS = NV4 * 4;                  // floats per stream record
    __shared__ RowsLds<C> lds;
    const int tile = tile_order ? (int)tile_order[blockIdx.x] : (int)blockIdx.x;
    const int img = tile / tiles, timg = tile - img * tiles;
    const int tx = timg % gx, ty = timg / gx;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = lane >> 4, l16 = lane & 15;
    const int qx0 = tx * kTile + (wave & 1) * 8, qy0 = ty * kTile + (wave >> 1) * 8;       // quadrant origin
    const int px = qx0 + 4 * (row & 1) + (l16 & 3);
    const int py = qy0 + 4 * (row >> 1) + (l16 >> 2);
    const bool inside = px < W && py < H;

    // n = this wave's quadrant count, n_kept = records kept by the tile
    const uint2 range = ranges[tile];
    const int n = (int)qcount[tile * 5 + wave], n_kept = (int)qcount[tile * 5 + 4];
    const int n_tile = (int)(range.y - range.x);
    const float* __restrict__ tb = stream + (size_t)range.x * RS;
    const uint32_t* __restrict__ qi = quad_list + ((size_t)range.x * 5 + (size_t)wave * n_tile);
    const uint32_t lim = n_kept > 0 ? (uint32_t)n_kept - 1u : 0u;
    RecordPrefetch pf;
    pf.issue(tb, n_kept, RS, tid, pf_lines);

    float4* __restrict__ recs = lds.s_rec[wave];
    uint32_t* __restrict__ mylist = lds.s_list[wave][row];
    if (lane == 0) write_dummy_record<C>(recs + kWave * NV4);
    QuadWalk<C> walk;
    walk.init(px, py, inside);

    constexpr uint32_t kDummy = ((uint32_t)kWave << 16) | ((uint32_t)kWave * NV4 * 16u);
    const float bx0 = (float)qx0, by0 = (float)qy0;
    for (int c0 = 0; c0 < n && walk.alive != 0ull; c0 += kWave) {
        const bool have = lane < min(kWave, n - c0);
        const uint32_t ridx = have ? min(qi[c0 + lane], lim) : 0u;
        const float4* __restrict__ rp = reinterpret_cast<const float4*>(tb + (size_t)ridx * RS);
        float4 r[NV4];
#pragma unroll
        for (int k = 0; k < NV4; ++k) r[k] = rp[k];
        if constexpr (RF >= 0) {
            constexpr int E = C - RF;
            const float* __restrict__ fp = feats + (size_t)__float_as_uint(r[1].w) * E;
            float fv[E];
#pragma unroll
            for (int k = 0; k < E; ++k) fv[k] = fp[k];
            float* rf = reinterpret_cast<float*>(r);
#pragma unroll
            for (int k = 0; k < E; ++k) rf[8 + RF + k] = fv[k];
        }
#pragma unroll
        for (int k = 0; k < NV4; ++k) recs[lane * NV4 + k] = r[k];
        walk.step(r[0], r[1], have, (uint32_t)lane * NV4 * 16u, kDummy, lds.s_list[wave], mylist, recs, bx0, by0,
                  (uint32_t)c0 + 1u, lane);
    }

    if (inside) walk.write_pixel(img, W, H, px, py, bg, out_color, out_depth, out_alpha, n_contrib, final_T);
    pf.retire(n_contrib, W);
}

// ---- the step's accumulation as a matrix instruction (NOT used by the kernels: DESIGN.md section 3e) ---------------------------
// sums[pixel][channel] += w[pixel] * f[channel] for the four 4x4 blocks of a quadrant at once: v_mfma_f32_16x16x1_4b_f32 is four
// independent 16x16 outer products, block b taking its A column and its B row from lanes 16b..16b+15 -- the walk's own layout
// (DPP row = block, lane in row = pixel for A, = channel for B).  K = 1: every element gets one fused multiply-add per call, no
// summation order exists, and a chain of calls is bit for bit the chain of fmaf() the kernels run (ogs_selftest_mfma_rank1 holds
// it to that: denormals, signed zeros, cancellation).  Register 4b + m of lane 16q + j holds block b, pixel 4q + m, channel j.
// A pack_blend_chunked_kernel built on it issued fewer vector and LDS instructions and ran slower: the instruction has the rate
// of the packed FMAs, works on a 16-channel tile of which C + 2 are needed, and holds the SIMD's vector issue while it starts
// (numbers: DESIGN.md section 3e).  Kept as the tested statement of what the instruction computes.
typedef float v16f __attribute__((ext_vector_type(16)));
__device__ __forceinline__ v16f rank1_update(float w, float f, v16f acc) {
    return __builtin_amdgcn_mfma_f32_16x16x1f32(w, f, acc, 0, 0, 0);
}
// test hook (ogs_selftest_mfma_rank1): `steps` chained updates of the 4 x 16 x 16 sums, w / f [steps][64] as the lanes of a
// wave hold them, acc0 / out [4][16][16] = [block][pixel][channel]; once on the matrix pipe, once as fmaf per element
__global__ __launch_bounds__(kWave) void mfma_rank1_test_kernel(const float* __restrict__ w, const float* __restrict__ f,
                                                                const float* __restrict__ acc0, int steps, float* __restrict__ out) {
    const int lane = threadIdx.x, q = lane >> 4, j = lane & 15;
    v16f acc;
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = acc0[((k >> 2) * 16 + 4 * q + (k & 3)) * 16 + j];
    for (int t = 0; t < steps; ++t) acc = rank1_update(w[t * kWave + lane], f[t * kWave + lane], acc);
#pragma unroll
    for (int k = 0; k < 16; ++k) out[((k >> 2) * 16 + 4 * q + (k & 3)) * 16 + j] = acc[k];
}
__global__ __launch_bounds__(256) void fma_rank1_test_kernel(const float* __restrict__ w, const float* __restrict__ f,
                                                             const float* __restrict__ acc0, int steps, float* __restrict__ out) {
    const int b = blockIdx.x, i = threadIdx.x >> 4, j = threadIdx.x & 15;
    float a = acc0[b * 256 + threadIdx.x];
    for (int t = 0; t < steps; ++t) a = fmaf(w[t * kWave + 16 * b + i], f[t * kWave + 16 * b + j], a);
    out[b * 256 + threadIdx.x] = a;
}

// ---- pack + forward blend of a tile, CHUNK BY CHUNK with a workgroup-wide exit (the default forward) -------------------
// The reference's forward fetches a tile's list 256 entries at a time and the whole block stops once every pixel is done
// (SURVEY.md section 2.1 `renderCUDA`, Appendix A.3).  On a ScanNet-class view (2 M Gaussians behind a 648 x 484 image, culled
// tile lists of ~3 000 entries) the last contributor of any pixel sits at 15 % of its tile's list
// (scripts/list_depth_stats.py -> profiles/r04_list_depth.json; 77 % at the headline workload), so packing the whole list
// before the first pixel is blended does mostly wasted work.  Here the tile's list is taken in chunks of 256 entries:
//     pack the chunk (quadrant box tests, block scan, kept records staged in LDS, index streams and records written out for
//     the backward) -> barrier -> every wave blends the entries the chunk ADDED to its quadrant's stream (QuadWalk::step,
//     64 at a time) -> the four waves vote; the workgroup leaves the list when every pixel of the tile is done.
// The walk takes the records from the chunk's staging buffer, which all four waves share read-only between two barriers,
// instead of re-reading the records it has just written.  qcount holds the counts AT THE EXIT: the backward (which starts
// from n_contrib) and the n_contrib export never look past them; entries behind the exit are neither packed nor written.
template <int C>
struct ChunkLds {
    static constexpr int SV = stream_vec4(C);
    uint64_t wave_tot[kBlock / kWave];
    uint32_t done[kBlock / kWave];
    float4 s_rec[(kBlock + 1) * SV];                       // kept records of the chunk, compact order (+ the dummy at slot kBlock)
    uint32_t s_list[kBlock / kWave][4][kRowListLen];       // per wave and 4x4 block: entries of the current 64-entry sub-chunk
    uint8_t s_qnew[4][kBlock];                             // per quadrant: staging slot of every entry the chunk adds to its stream
};

// ---- grouped label statistics (ogs_raster_forward_group_stats) ----------------------------------------------------------
// Per (group g, label bucket l): the pixels of image g with alpha > thr whose label is l (bucket L: no mask), the sum of their
// blended colour, and per group the maximum alpha -- what the 2D-3D association reads off the images of a grouped pass, taken
// in the blend's epilogue instead.  Sums are int64 fixed point (quantum 2^-32): integer adds commute, so the result does not
// depend on the order in which workgroups arrive -- bit-reproducible run to run (fp32 atomics are not).  One tile reduces in
// LDS first: wave 0 walks the tile's 256 pixels (four per lane) label by label (the first pending label of the first pending
// lane, broadcast), sums the matching pixels per lane, then across the wave, and issues ONE global atomic per (label, channel)
// the tile touched.
struct GroupStatsOut {
    const int32_t* labels;       // [H*W]
    int32_t L;                   // labels in [0, L); anything else -> bucket L
    float thr;
    uint32_t* max_alpha;         // [G] fp32 bit patterns (alpha >= 0: integer order == float order)
    unsigned long long* count;   // [G, L+1]
    unsigned long long* fsum;    // [G, L+1, C] int64, quantum 2^-32
};

constexpr float kFixedScale = 4294967296.0f;          // 2^32

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
    const uint32_t lo = __shfl_xor((uint32_t)v, m, kWave), hi = __shfl_xor((uint32_t)(v >> 32), m, kWave);
    return ((unsigned long long)hi << 32) | lo;
}

// s_buf: >= (C + 2) * kBlock floats of LDS no other wave reads any more.  pix = py * W + px, or -1 outside the image.
template <int C>
__device__ __forceinline__ void group_stats_epilogue(const GroupStatsOut& st, float* __restrict__ s_buf, int img, int W, int pix,
                                                     float alpha, const float (&colour)[C]) {
    float* s_val = s_buf;                                               // [C][kBlock]
    float* s_alpha = s_buf + C * kBlock;                                // [kBlock]
    int* s_key = reinterpret_cast<int*>(s_buf + (C + 1) * kBlock);      // [kBlock]: bucket, -1 = not counted
    const int tid = threadIdx.x, lane = tid & 63;
    int key = -1;
    if (pix >= 0 && alpha > st.thr) {
        const int l = st.labels[pix];
        key = (l >= 0 && l < st.L) ? l : st.L;
    }
    s_key[tid] = key;
    s_alpha[tid] = pix >= 0 ? alpha : 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) s_val[c * kBlock + tid] = colour[c];
    lds_barrier();
    if (tid >= kWave) return;
    int k[kBlock / kWave];
    float m = 0.f;
#pragma unroll
    for (int j = 0; j < kBlock / kWave; ++j) {
        k[j] = s_key[lane + kWave * j];
        m = fmaxf(m, s_alpha[lane + kWave * j]);
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, kWave));
    if (lane == 0 && m > 0.f) atomicMax(st.max_alpha + img, __float_as_uint(m));
    const size_t row0 = (size_t)img * (size_t)(st.L + 1);
    for (;;) {
        int cand = -1;
#pragma unroll
        for (int j = kBlock / kWave - 1; j >= 0; --j) cand = k[j] >= 0 ? k[j] : cand;
        const uint64_t pending = __ballot(cand >= 0);
        if (pending == 0ull) break;
        const int K = __shfl(cand, __ffsll((unsigned long long)pending) - 1, kWave);
        unsigned long long cnt = 0, sum[C];
#pragma unroll
        for (int c = 0; c < C; ++c) sum[c] = 0ull;
#pragma unroll
        for (int j = 0; j < kBlock / kWave; ++j) {
            if (k[j] == K) {
                ++cnt;
#pragma unroll
                for (int c = 0; c < C; ++c) sum[c] += (unsigned long long)__float2ll_rn(s_val[c * kBlock + lane + kWave * j] * kFixedScale);
                k[j] = -1;
            }
        }
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) {
            cnt += (unsigned long long)__shfl_xor((uint32_t)cnt, off, kWave);
#pragma unroll
            for (int c = 0; c < C; ++c) sum[c] += shfl_xor_u64(sum[c], off);
        }
        if (lane == 0) {
            const size_t r = row0 + (size_t)K;
            atomicAdd(st.count + r, cnt);
#pragma unroll
            for (int c = 0; c < C; ++c) atomicAdd(st.fsum + r * C + c, sum[c]);
        }
    }
}

// fixed point -> fp32, once per (group, bucket, channel)
__global__ __launch_bounds__(256) void group_stats_finish_kernel(const long long* __restrict__ fsum, float* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (float)((double)fsum[i] * (1.0 / 4294967296.0));
}

// Six waves per SIMD: the kernel is sensitive to occupancy (probe: 24 KB more LDS per workgroup, three workgroups per CU instead of
// six: 0.402 -> 0.514 ms) and its 26 KB of LDS allow six workgroups per CU, but at C = 9 the register allocator settles at 92 VGPRs
// = five waves.  Asking for six gives 0.402 -> 0.390 ms (A-B-A-B on one box); C = 12 cannot fit (its 30 KB of LDS allow five
// workgroups) and stays where it was.  This file is compiled without the SLP vectoriser (build.py): left to it, the compiler
// pairs the scalar multiplies of the box tests into ~80 v_pk_mul / v_pk_fma per kernel, whose even-aligned register pairs cost
// the C = 9 kernel three spilled dwords at 80 VGPRs; without it, 78 VGPRs and no scratch (AMD clang 22.0.0git, roc-7.2.0: the
// figures depend on the compiler's register allocation; table and timings in DESIGN.md section 3e).  The packed operations
// written out below (v2f) are not affected.
// STATS (ogs_raster_forward_group_stats): the same walk -- same packing, same per-pixel arithmetic, same exit -- with the
// image epilogue replaced by group_stats_epilogue (per-(group, label) statistics, nothing of size G*W*H) and the write-outs
// kept for the backward (records, quadrant streams, qcount) compiled out.  `st` is unused when STATS is false.
template <int C, bool STATS = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(6, 8)))
void pack_blend_chunked_kernel(
    const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list, const float4* __restrict__ rec,
    float4* __restrict__ stream, uint32_t* __restrict__ quad_list, uint32_t* __restrict__ qcount, int W, int H, int gx, int tiles,
    const float* __restrict__ bg, float* __restrict__ out_color, float* __restrict__ out_depth, float* __restrict__ out_alpha,
    uint32_t* __restrict__ n_contrib, float* __restrict__ final_T, const uint32_t* __restrict__ tile_order,
    uint4* __restrict__ clear, unsigned long long clear_units, GroupStatsOut st = GroupStatsOut{}) {
    // clear / clear_units (optional, not STATS): a range of 16-byte units this launch zeroes for a later kernel
    // (OgsRasterFwdArgs.bwd_clear: the gradient record of the backward).  Workgroup b takes slice b of gridDim.x equal slices,
    // whatever its tile's list looks like, at its exit: stores nothing waits for, in a kernel that is not bandwidth-bound.  (At
    // workgroup entry, in front of the first gather, the same stores cost the S1M step 0.005 ms more: DESIGN.md section 3d)
    constexpr int NV = rec_vec4(C);
    constexpr int SV = stream_vec4(C);
    __shared__ ChunkLds<C> lds;
    const int tile = tile_order ? (int)tile_order[blockIdx.x] : (int)blockIdx.x;
    const int img = tile / tiles, timg = tile - img * tiles;
    const uint2 range = ranges[tile];
    const int n = (int)(range.y - range.x);
    const int tx = timg % gx, ty = timg / gx;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float X0 = (float)(tx * kTile), Y0 = (float)(ty * kTile);
    // blend side: wave = quadrant, DPP row = 4x4 block
    const int row = lane >> 4, l16 = lane & 15;
    const int qx0 = tx * kTile + (wave & 1) * 8, qy0 = ty * kTile + (wave >> 1) * 8;
    const int px = qx0 + 4 * (row & 1) + (l16 & 3);
    const int py = qy0 + 4 * (row >> 1) + (l16 >> 2);
    const bool inside = px < W && py < H;
    QuadWalk<C> walk;
    walk.init(px, py, inside);

    const float4* __restrict__ recs = lds.s_rec;
    uint32_t* __restrict__ mylist = lds.s_list[wave][row];
    if (tid == 0) write_dummy_record<C>(lds.s_rec + kBlock * SV);

    uint32_t running[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) running[q] = 0u;
    const float bx0 = (float)qx0, by0 = (float)qy0;

    for (int base = 0; base < n; base += kBlock) {
        // ================= pack the chunk =================
        const int i = base + tid;
        uint32_t mask = 0;
        float4 a = make_float4(0, 0, 0, 0), b = a;
        float h = 0.f;
        uint32_t gid_of_thread = 0;
        // sorted value = Gaussian id | "reaches this tile" << 31: duplicate_kernel ran ONE box test per (Gaussian, tile) pair,
        // so nothing is gathered here for the pairs that reach no pixel of the tile
        const uint32_t sv = i < n ? point_list[range.x + i] : 0u;
        if (sv >> kReachBit) {
            const uint32_t gid = sv & kGidMask;
            gid_of_thread = gid;
            const float4* src = rec + (size_t)gid * NV;
            a = src[0]; b = src[1];              // geometry only: the features are fetched if the entry survives
            // candidate window thr <= power <= 0, thr = ln(1/(255*opacity)) - margin; stored as h = -thr/2 so the blend loops
            // test it with ONE compare |power + h| <= h (opacity <= 0: NaN/-inf, never a candidate)
            h = 0.5f * (__logf(255.0f * b.w) + kThrMargin);
            const float thr = -2.0f * h;
            const float nbA = -b.y / b.x, nbC = -b.y / b.z;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float qx = X0 + (float)((q & 1) * 8), qy = Y0 + (float)((q >> 1) * 8);
                const float m = max_power_in_box(b.x, b.y, b.z, nbA, nbC, a.x - qx - 7.f, a.x - qx, a.y - qy - 7.f, a.y - qy);
                if (m >= thr) mask |= 1u << q;
            }
        }
        // block-wide exclusive prefix of the four per-quadrant keep flags and of "kept at all" (12-bit fields of one u64)
        const uint64_t mine = (uint64_t)(mask & 1u) | ((uint64_t)((mask >> 1) & 1u) << 12) |
                              ((uint64_t)((mask >> 2) & 1u) << 24) | ((uint64_t)((mask >> 3) & 1u) << 36) |
                              ((uint64_t)(mask != 0u ? 1u : 0u) << 48);
        uint64_t inc = mine;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const uint64_t t = shfl_up_u64(inc, d);
            if (lane >= d) inc += t;
        }
        if (lane == kWave - 1) lds.wave_tot[wave] = inc;
        lds_barrier();                    // (1) wave totals; also: every wave has left the previous chunk's blend
        uint64_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kBlock / kWave; ++w) {
            const uint64_t t = lds.wave_tot[w];
            if (w < wave) before += t;
            total += t;
        }
        const uint64_t pos = before + inc - mine;
        if (mask) {
            // ONE copy of the record, COMPACTED (kept entry c of the tile -> record range.x + c, depth order preserved), staged
            // in LDS; its compact index goes to the index stream of every quadrant it can reach, and its position in the
            // tile's full list is kept for the n_contrib export
            const uint32_t c_loc = (uint32_t)(pos >> 48) & 0xFFFu;
            const uint32_t c_idx = running[4] + c_loc;
            float4* dst = lds.s_rec + c_loc * SV;
            dst[0] = make_float4(a.x, a.y, -0.5f * b.x, -0.5f * b.z);
            dst[1] = make_float4(-b.y, h, b.w, __uint_as_float(gid_of_thread));
            const float4* src = rec + (size_t)gid_of_thread * NV;
            float f[(SV - 2) * 4];
#pragma unroll
            for (int k = 0; k < (SV - 2) * 4; ++k) f[k] = 0.f;
#pragma unroll
            for (int v = 0; v < NV - 2; ++v) {
                const float4 t = src[2 + v];
                f[4 * v] = t.x; f[4 * v + 1] = t.y; f[4 * v + 2] = t.z; f[4 * v + 3] = t.w;
            }
            f[C] = a.z;
#pragma unroll
            for (int v = 0; v < SV - 2; ++v) dst[2 + v] = make_float4(f[4 * v], f[4 * v + 1], f[4 * v + 2], f[4 * v + 3]);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (mask & (1u << q)) {
                    const uint32_t pq = (uint32_t)(pos >> (12 * q)) & 0xFFFu;
                    if constexpr (!STATS) quad_list[(size_t)range.x * 5 + (size_t)q * n + running[q] + pq] = c_idx;   // for the backward
                    lds.s_qnew[q][pq] = (uint8_t)c_loc;                                            // for this chunk's blend
                }
            }
            if constexpr (!STATS) quad_list[(size_t)range.x * 5 + (size_t)4 * n + c_idx] = (uint32_t)i;
        }
        lds_barrier();                    // (2) the chunk's records and stream entries are staged
        if constexpr (!STATS) {
            // record write-out for the backward: one contiguous range, the whole workgroup (stores only: nothing waits for them)
            const int kept4 = (int)((uint32_t)(total >> 48) & 0xFFFu) * SV;
            float4* __restrict__ out = stream + ((size_t)range.x + (size_t)running[4]) * SV;
            for (int e = tid; e < kept4; e += kBlock) out[e] = lds.s_rec[e];
        }
        // ================= blend what the chunk added to this wave's quadrant stream =================
        const int cnt_q = (int)((uint32_t)(total >> (12 * wave)) & 0xFFFu);
        const uint32_t j0 = wave == 0 ? running[0] : wave == 1 ? running[1] : wave == 2 ? running[2] : running[3];
        // list entry = sub-chunk slot << 16 | byte offset of the record in the staging buffer
        constexpr uint32_t kDummy = ((uint32_t)kWave << 16) | ((uint32_t)kBlock * SV * 16u);
        for (int c0 = 0; c0 < cnt_q && walk.alive != 0ull; c0 += kWave) {
            const bool have = lane < min(kWave, cnt_q - c0);
            const uint32_t cl = have ? (uint32_t)lds.s_qnew[wave][c0 + lane] : (uint32_t)kBlock;
            walk.step(recs[cl * SV], recs[cl * SV + 1], have, cl * SV * 16u, kDummy, lds.s_list[wave], mylist, recs, bx0, by0,
                      j0 + (uint32_t)c0 + 1u, lane);
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) running[q] += (uint32_t)(total >> (12 * q)) & 0xFFFu;
        if (lane == 0) lds.done[wave] = walk.alive == 0ull ? 1u : 0u;
        lds_barrier();                    // (3) the staging buffer is free again; the four votes are in
        if ((lds.done[0] & lds.done[1] & lds.done[2] & lds.done[3]) != 0u) break;       // block-uniform
    }
    if constexpr (STATS) {
        // every wave is past barrier (3) of the last chunk (or never entered the loop): the staging buffer is free
        float colour[C];
#pragma unroll
        for (int c = 0; c < C; ++c) colour[c] = walk.colour(c, bg);
        group_stats_epilogue<C>(st, reinterpret_cast<float*>(lds.s_rec), img, W, inside ? py * W + px : -1, walk.wacc, colour);
    } else {
        if (tid == 0) {
#pragma unroll
            for (int q = 0; q < 5; ++q) qcount[tile * 5 + q] = running[q];
        }
        if (inside) walk.write_pixel(img, W, H, px, py, bg, out_color, out_depth, out_alpha, n_contrib, final_T);
        if (clear != nullptr) {           // kernel-uniform
            const unsigned long long per = (clear_units + gridDim.x - 1) / gridDim.x;
            const unsigned long long u0 = min(clear_units, (unsigned long long)blockIdx.x * per), u1 = min(clear_units, u0 + per);
            for (unsigned long long u = u0 + (unsigned)tid; u < u1; u += kBlock) clear[u] = uint4{0u, 0u, 0u, 0u};
        }
    }
}

// test/diagnostic export: translate the per-quadrant stream index kept in n_contrib back to the reference's
// convention, the 1-based position in the tile's full sorted list
template <int C>
__global__ __launch_bounds__(kBlock) void export_n_contrib_kernel(const uint2* __restrict__ ranges,
                                                                  const uint32_t* __restrict__ point_list,
                                                                  const uint32_t* __restrict__ quad_list, int W, int H,
                                                                  int gx, int tiles, const uint32_t* __restrict__ n_contrib,
                                                                  uint32_t* __restrict__ out) {
    const int tile = blockIdx.x;
    const int img = tile / tiles, timg = tile - img * tiles;
    const int tx = timg % gx, ty = timg / gx;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int px = tx * kTile + (wave & 1) * 8 + (lane & 7);
    const int py = ty * kTile + (wave >> 1) * 8 + (lane >> 3);
    if (px >= W || py >= H) return;
    const uint2 range = ranges[tile];
    const int n_tile = (int)(range.y - range.x);
    n_contrib += (size_t)img * W * H;
    out += (size_t)img * W * H;
    const uint32_t last = n_contrib[(size_t)py * W + px];
    // n_contrib counts inside the quadrant's index stream; the stream entry IS the position in the tile list
    uint32_t res = 0;
    if (last > 0) {
        const uint32_t c_idx = quad_list[(size_t)range.x * 5 + (size_t)wave * n_tile + (last - 1)];
        res = quad_list[(size_t)range.x * 5 + (size_t)4 * n_tile + c_idx] + 1u;       // compact index -> full-list position
    }
    out[(size_t)py * W + px] = res;
}

// Tiny pass (P <= kTinyMaxP, see preprocess_fwd.hip::tiny_geometry_kernel): no duplicate / sort / ranges / pack.  One
// workgroup per tile walks the P depth-sorted Gaussians, keeps those whose tile rect (A.1 step 8) covers the tile --
// exactly the reference's tile list, in its order -- stages their blend records in LDS and blends them with the
// per-pixel arithmetic of the streaming forward (blend_power, the same candidate window, the same FMAs), so the images
// equal the streaming path's bit for bit.  2 launches per pass instead of ~25; nothing is kept for a backward pass (the facade
// re-renders through the streaming path if backward() is ever called on a tiny pass).
template <int C>
__global__ __launch_bounds__(kBlock) void tiny_blend_kernel(int P, const uint32_t* __restrict__ order,
                                                            const float4* __restrict__ rec, int W, int H, int gx,
                                                            const float* __restrict__ bg, float* __restrict__ out_color,
                                                            float* __restrict__ out_depth, float* __restrict__ out_alpha) {
    constexpr int NV = rec_vec4(C);
    constexpr int RS = 8 + (C + 1 + 3) / 4 * 4;                 // floats per staged record (geometry 8, features + depth)
    static_assert(kTinyMaxP == kBlock, "one staging round");
    __shared__ float s_rec[kTinyMaxP * RS];
    __shared__ uint32_t s_wave_cnt[kBlock / kWave];
    const int tile = blockIdx.x;
    const int tx = tile % gx, ty = tile / gx;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int gy = (H + kTile - 1) / kTile;

    // ---- tile list: sorted position tid -> does its rect cover this tile? ----------------------------------------
    bool keep = false;
    float4 a = make_float4(0, 0, 0, 0), b = a;
    uint32_t gid = 0;
    if (tid < P) {
        gid = order[tid];
        const float4* src = rec + (size_t)gid * NV;
        a = src[0]; b = src[1];
        const int radius = __float_as_int(a.w);
        if (radius > 0) {
            const float rf = (float)radius;
            auto tr = [](float v) -> int {
                if (!(fabsf(v) < 3.0e38f)) v = 0.f;
                v = fminf(fmaxf(v, -2.0e9f), 2.0e9f);
                return (int)v;
            };
            // same expressions as preprocess / duplicate (division by 16 and the +15 are exact in fp32)
            const int rminx = min(gx, max(0, tr((a.x - rf) / (float)kTile)));
            const int rminy = min(gy, max(0, tr((a.y - rf) / (float)kTile)));
            const int rmaxx = min(gx, max(0, tr((a.x + rf + (float)kTile - 1.0f) / (float)kTile)));
            const int rmaxy = min(gy, max(0, tr((a.y + rf + (float)kTile - 1.0f) / (float)kTile)));
            keep = tx >= rminx && tx < rmaxx && ty >= rminy && ty < rmaxy;
        }
    }
    const uint64_t bal = __ballot(keep);
    if (lane == 0) s_wave_cnt[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t before = 0, n = 0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) {
        const uint32_t c = s_wave_cnt[w];
        if (w < wave) before += c;
        n += c;
    }
    if (keep) {
        const uint32_t pos = before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        float* dst = s_rec + pos * RS;
        dst[0] = a.x; dst[1] = a.y; dst[2] = -0.5f * b.x; dst[3] = -b.y; dst[4] = -0.5f * b.z;
        dst[5] = 0.5f * (__logf(255.0f * b.w) + kThrMargin);
        dst[6] = b.w; dst[7] = __uint_as_float(gid);
        const float4* src = rec + (size_t)gid * NV;
        float f[(NV - 2) * 4 + 4];
#pragma unroll
        for (int v = 0; v < NV - 2; ++v) {
            const float4 t = src[2 + v];
            f[4 * v] = t.x; f[4 * v + 1] = t.y; f[4 * v + 2] = t.z; f[4 * v + 3] = t.w;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) dst[8 + c] = f[c];
        dst[8 + C] = a.z;
    }
    __syncthreads();

    // ---- blend (A.3), one pixel per thread, same arithmetic as QuadWalk::consume ----------------------------
    const int px = tx * kTile + (wave & 1) * 8 + (lane & 7);
    const int py = ty * kTile + (wave >> 1) * 8 + (lane >> 3);
    const bool inside = px < W && py < H;
    const float fx = (float)px, fy = (float)py;
    float T = 1.0f, wacc = 0.f;
    float acc[C + 1];
#pragma unroll
    for (int c = 0; c <= C; ++c) acc[c] = 0.f;
    bool done = !inside;
    for (uint32_t j = 0; j < n; ++j) {
        if (__ballot(!done) == 0ull) break;
        const float* r = s_rec + j * RS;                          // wave-uniform LDS address: broadcast reads
        const float dx = r[0] - fx, dy = r[1] - fy;
        const float power = blend_power(r[2], r[3], r[4], dx, dy);
        const bool cand = !done && fabsf(power + r[5]) <= r[5];
        if (cand) {
            float alpha = fminf(0.99f, r[6] * __expf(power));
            alpha = alpha >= kAlphaMin ? alpha : 0.f;
            const float test_T = T * (1.0f - alpha);
            const bool stop = test_T < 0.0001f;
            const float w = stop ? 0.f : alpha * T;
#pragma unroll
            for (int c = 0; c <= C; ++c) acc[c] = fmaf(r[8 + c], w, acc[c]);
            wacc += w;
            T = stop ? T : test_T;
            done = stop;
        }
    }
    if (inside) {
        const size_t plane = (size_t)W * H;
        const size_t pix = (size_t)py * W + px;
#pragma unroll
        for (int c = 0; c < C; ++c) out_color[c * plane + pix] = acc[c] + T * bg[c];
        out_depth[pix] = acc[C];
        out_alpha[pix] = wacc;
    }
}

template <int C>
int tiny_c(const OgsRasterFwdArgs& a, const GeomState& gs, const uint32_t* order, hipStream_t s) {
    const int gx = (a.W + kTile - 1) / kTile, gy = (a.H + kTile - 1) / kTile;
    OGS_LAUNCH(tiny_blend_kernel<C>, dim3((unsigned)(gx * gy)), dim3(kBlock), 0, s, a.P, order, (const float4*)gs.rec, a.W, a.H,
               gx, a.bg, a.out_color, a.out_depth, a.out_alpha);
    OGS_LAUNCH_CHECK(a.debug, s);
    return OGS_OK;
}


// ---- heaviest-first workgroup order ---------------------------------------------------------------------------------
// A tile's kernels run as long as its list is long, and the lists of one view span two orders of magnitude.  The
// hardware hands workgroups to the CUs in index order, so with workgroup = tile in raster order the launch ends with
// whatever long lists happen to sit at the bottom of the image running alone (SQ counters of the forward blend: 4.4
// waves per SIMD on average where 8 fit).  One workgroup sorts the tiles by list length into 256 classes of a
// pseudo-logarithmic scale (3 mantissa bits: classes are <= 12.5 % wide), heaviest class first; order inside a class is
// whatever the LDS atomics give -- any permutation is a valid schedule.
constexpr int kOrderThreads = 1024;
constexpr int64_t kOrderMaxTiles = 1 << 16;      // one workgroup walks all tiles: beyond this the launch costs more than it buys
__device__ __forceinline__ uint32_t work_class(uint32_t n) {      // 255 = empty ... 0 = longest
    if (n < 8u) return 255u - n;
    const uint32_t e = 31u - (uint32_t)__builtin_clz(n);
    const uint32_t v = e * 8u + ((n >> (e - 3u)) & 7u);          // monotonic in n, 24 .. 255
    return 255u - min(v, 255u);
}
// bins[cls] += 1 for every valid lane; returns the lane's slot (old count + its rank among the wave's lanes of the same
// class).  One LDS atomic per (wave, distinct class): a view with few Gaussians leaves most tiles EMPTY, and thousands
// of single-lane atomics on that one counter serialise (P = 10 k at 1080p: 60 us for this kernel before, 6 us after).
__device__ __forceinline__ uint32_t class_counter_add(uint32_t* bins, uint32_t cls, bool valid, int lane) {
    uint32_t pos = 0u;
    uint64_t todo = __ballot(valid);
    while (todo != 0ull) {                                // wave-uniform: at most one trip per distinct class
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t c0 = (uint32_t)__shfl((int)cls, leader, kWave);
        const uint64_t same = __ballot(valid && cls == c0) & todo;
        uint32_t base = 0u;
        if (lane == leader) base = atomicAdd(&bins[c0], (uint32_t)__popcll(same));
        base = (uint32_t)__shfl((int)base, leader, kWave);
        if ((same >> lane) & 1ull) pos = base + (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        todo &= ~same;
    }
    return pos;
}
__global__ __launch_bounds__(kOrderThreads) void tile_order_kernel(const uint2* __restrict__ ranges, uint32_t vtiles,
                                                                   uint32_t* __restrict__ order) {
    __shared__ uint32_t bins[256];
    __shared__ uint32_t wave_max[kOrderThreads / kWave], wave_sum[kOrderThreads / kWave];
    const uint32_t tid = threadIdx.x;
    // longest list and total length: every thread's loads in flight at once, one LDS slot per wave
    uint32_t my_max = 0u, my_sum = 0u;
    for (uint32_t t0 = 0; t0 < vtiles; t0 += 8u * kOrderThreads) {
        uint2 r[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t t = t0 + (uint32_t)k * kOrderThreads + tid;
            r[k] = t < vtiles ? ranges[t] : make_uint2(0u, 0u);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) { my_max = max(my_max, r[k].y - r[k].x); my_sum += r[k].y - r[k].x; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        my_max = max(my_max, (uint32_t)__shfl_xor((int)my_max, d, kWave));
        my_sum += (uint32_t)__shfl_xor((int)my_sum, d, kWave);
    }
    if ((tid & 63u) == 0u) { wave_max[tid >> 6] = my_max; wave_sum[tid >> 6] = my_sum; }
    if (tid < 256u) bins[tid] = 0u;
    __syncthreads();
    uint32_t longest = 0u;
    unsigned long long total = 0ull;
#pragma unroll
    for (int w = 0; w < kOrderThreads / kWave; ++w) { longest = max(longest, wave_max[w]); total += wave_sum[w]; }
    // lists of similar length everywhere (longest <= 2 x mean): raster order, which keeps neighbouring tiles -- and the
    // Gaussians they share -- on the chip at the same time (the uniform bench scene: 1.5 % faster forward than a
    // shuffled order)
    if ((unsigned long long)longest * vtiles <= 2ull * total) {
        for (uint32_t t = tid; t < vtiles; t += kOrderThreads) order[t] = t;
        return;
    }
    for (uint32_t t0 = 0; t0 < vtiles; t0 += kOrderThreads) {
        const uint32_t t = t0 + tid;
        const bool valid = t < vtiles;
        const uint2 r = valid ? ranges[t] : make_uint2(0u, 0u);
        (void)class_counter_add(bins, work_class(r.y - r.x), valid, (int)(tid & 63u));
    }
    __syncthreads();
    if (tid < 64u) {                                      // exclusive scan of the 256 class counts: 4 per lane of one wave
        uint32_t c[4], sum = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) { c[k] = bins[tid * 4u + k]; sum += c[k]; }
        uint32_t incl = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d, kWave);
            if ((int)tid >= d) incl += o;
        }
        uint32_t base = incl - sum;
#pragma unroll
        for (int k = 0; k < 4; ++k) { bins[tid * 4u + k] = base; base += c[k]; }
    }
    __syncthreads();
    for (uint32_t t0 = 0; t0 < vtiles; t0 += kOrderThreads) {
        const uint32_t t = t0 + tid;
        const bool valid = t < vtiles;
        const uint2 r = valid ? ranges[t] : make_uint2(0u, 0u);
        const uint32_t pos = class_counter_add(bins, work_class(r.y - r.x), valid, (int)(tid & 63u));
        if (valid) order[pos] = t;
    }
}

// D > 0: pack and blend in one launch; an empty list: no counts to pack, the stand-alone blend writes the background
template <int C>
int launch_c(const OgsRasterFwdArgs& a, const GeomState& gs, const ImageState& is, int64_t D, hipStream_t s, bool order_ready) {
    const int gx = (a.W + kTile - 1) / kTile, gy = (a.H + kTile - 1) / kTile;
    const int tiles = gx * gy;
    const unsigned vtiles = (unsigned)tiles * (unsigned)num_groups_of(a.num_groups);
    // the range the caller wants zeroed (OgsRasterFwdArgs.bwd_clear): stores hosted by the chunked kernel on the ungrouped
    // streaming path, a fill launch everywhere else
    const bool host_clear = a.bwd_clear != nullptr && D > 0 && per_tile_depth_order(a);
    if (a.bwd_clear != nullptr && !host_clear) OGS_HIP_CHECK(hipMemsetAsync(a.bwd_clear, 0, a.bwd_clear_bytes, s));
    if (D > 0) {
        const uint32_t* order = order_ready ? tile_order_of(is, vtiles, a.P) : launch_tile_order(is, vtiles, a.P, s, a.debug);
        static constexpr const char* const kChunked[4] = {"pack_blend_chunked_kernel<3>", "pack_blend_chunked_kernel<6>",
                                                          "pack_blend_chunked_kernel<9>", "pack_blend_chunked_kernel<12>"};
        OGS_LAUNCH_NAMED(chan_name<C>(kChunked), pack_blend_chunked_kernel<C>, dim3(vtiles), dim3(kBlock), 0, s,
                         (const uint2*)is.ranges, (const uint32_t*)a.point_list, (const float4*)gs.rec, stream_base<C>(a.sorted_rec),
                         quad_base(a.quad_list), is.qcount, a.W, a.H, gx, tiles, a.bg, a.out_color, a.out_depth, a.out_alpha,
                         is.n_contrib, is.final_T, order, host_clear ? static_cast<uint4*>(a.bwd_clear) : (uint4*)nullptr,
                         (unsigned long long)(a.bwd_clear_bytes / 16));
        OGS_LAUNCH_CHECK(a.debug, s);
        return OGS_OK;
    }
    OGS_HIP_CHECK(hipMemsetAsync(is.qcount, 0, (size_t)vtiles * 5 * sizeof(uint32_t), s));
    static constexpr const char* const kRows[4] = {"blend_forward_rows_kernel<3>", "blend_forward_rows_kernel<6>",
                                                   "blend_forward_rows_kernel<9>", "blend_forward_rows_kernel<12>"};
    OGS_LAUNCH_NAMED(chan_name<C>(kRows), blend_forward_rows_kernel<C>, dim3(vtiles), dim3(kBlock), 0, s,
                     (const uint2*)is.ranges, (const uint32_t*)is.qcount, (const float*)stream_base<C>(a.sorted_rec),
                     (const uint32_t*)quad_base(a.quad_list), a.W, a.H, gx, tiles, a.bg, a.out_color, a.out_depth,
                     a.out_alpha, is.n_contrib, is.final_T, blend_prefetch_lines(), (const uint32_t*)nullptr, (const float*)nullptr);
    OGS_LAUNCH_CHECK(a.debug, s);
    return OGS_OK;
}

// statistics variant of launch_c: the chunked walk on every virtual tile (an empty list included: n = 0, the pixels keep the
// background), then the fixed-point sums to fp32.  The outputs and the fixed-point scratch are cleared here.
template <int C>
int stats_c(const OgsRasterFwdArgs& a, const OgsGroupStatsArgs& sa, const GeomState& gs, const ImageState& is, hipStream_t s,
            bool order_ready) {
    const int gx = (a.W + kTile - 1) / kTile, gy = (a.H + kTile - 1) / kTile;
    const int tiles = gx * gy;
    const int G = num_groups_of(a.num_groups);
    const unsigned vtiles = (unsigned)tiles * (unsigned)G;
    const size_t rows = (size_t)G * (size_t)(sa.num_labels + 1);
    long long* fixed = static_cast<long long*>(sa.stats_tmp);
    OGS_HIP_CHECK(hipMemsetAsync(sa.max_alpha, 0, (size_t)G * sizeof(float), s));
    OGS_HIP_CHECK(hipMemsetAsync(sa.count, 0, rows * sizeof(int64_t), s));
    OGS_HIP_CHECK(hipMemsetAsync(fixed, 0, rows * C * sizeof(long long), s));
    const uint32_t* order = order_ready ? tile_order_of(is, vtiles, a.P) : launch_tile_order(is, vtiles, a.P, s, a.debug);
    GroupStatsOut st;
    st.labels = sa.labels;
    st.L = sa.num_labels;
    st.thr = sa.alpha_threshold;
    st.max_alpha = reinterpret_cast<uint32_t*>(sa.max_alpha);
    st.count = reinterpret_cast<unsigned long long*>(sa.count);
    st.fsum = reinterpret_cast<unsigned long long*>(fixed);
    static constexpr const char* const kStats[4] = {"pack_blend_chunked_kernel<3, stats>", "pack_blend_chunked_kernel<6, stats>",
                                                    "pack_blend_chunked_kernel<9, stats>", "pack_blend_chunked_kernel<12, stats>"};
    OGS_LAUNCH_NAMED(chan_name<C>(kStats), (pack_blend_chunked_kernel<C, true>), dim3(vtiles), dim3(kBlock), 0, s,
                     (const uint2*)is.ranges, (const uint32_t*)a.point_list, (const float4*)gs.rec, (float4*)nullptr,
                     (uint32_t*)nullptr, (uint32_t*)nullptr, a.W, a.H, gx, tiles, a.bg, (float*)nullptr, (float*)nullptr,
                     (float*)nullptr, (uint32_t*)nullptr, (float*)nullptr, order, (uint4*)nullptr, 0ull, st);
    OGS_LAUNCH_CHECK(a.debug, s);
    const size_t n = rows * C;
    OGS_LAUNCH(group_stats_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const long long*)fixed,
               sa.feat_sum, n);
    OGS_LAUNCH_CHECK(a.debug, s);
    return OGS_OK;
}

// ---- re-blend of a kept pass (frozen geometry, round 4) ----------------------------------------------------------------
// From stage 1 on the reference trains `_ins_feat` alone (train.py:431-436): for a given camera every later pass bins, sorts and
// packs exactly what the first one did, only the feature channels of the records differ.  A caller that kept image_buffer,
// sorted_rec and quad_list of such a pass (rasterizer.py: KeptPasses) re-renders with ONE launch: the stand-alone forward blend
// walks the kept quadrant streams and takes channels [F0, C) of every record from the current per-Gaussian features
// (blend_forward_rows_kernel<C, RF>).  (First version: a kernel that rewrote the channels inside the kept records, then the plain blend --
// 0.13 ms at the bench scene for the read-modify-write of 24 bytes in every 80-byte record, against 0.32 ms for the blend.)
template <int C>
int reblend_c(const OgsRasterFwdArgs& a, const ImageState& is, hipStream_t s) {
    const int gx = (a.W + kTile - 1) / kTile, gy = (a.H + kTile - 1) / kTile;
    const int tiles = gx * gy;
    const unsigned vtiles = (unsigned)tiles;
    const uint32_t* order = tile_order_of(is, vtiles, a.P);        // written by the kept pass
    static constexpr const char* const kRows[4] = {"blend_forward_rows_kernel<3, refresh>", "blend_forward_rows_kernel<6, refresh>",
                                                   "blend_forward_rows_kernel<9, refresh>", "blend_forward_rows_kernel<12, refresh>"};
    const float* stream = reinterpret_cast<const float*>(stream_base<C>(a.sorted_rec));
#define OGS_REBLEND(RFV)                                                                                                    \
    OGS_LAUNCH_NAMED(chan_name<C>(kRows), (blend_forward_rows_kernel<C, RFV>), dim3(vtiles), dim3(kBlock), 0, s,           \
                     (const uint2*)is.ranges, (const uint32_t*)is.qcount, stream, (const uint32_t*)quad_base(a.quad_list), a.W,  \
                     a.H, gx, tiles, a.bg, a.out_color, a.out_depth, a.out_alpha, is.n_contrib, is.final_T,                  \
                     blend_prefetch_lines(), order, a.colors_precomp)
    if (a.sh_coeffs != 0) {
        if constexpr (C > 3) {
            OGS_REBLEND(3);
        } else {
            set_error("forward_reblend: a 3-channel SH pass has no channel to replace");
            return OGS_ERR_INVALID_ARG;
        }
    } else {
        OGS_REBLEND(0);
    }
#undef OGS_REBLEND
    OGS_LAUNCH_CHECK(a.debug, s);
    return OGS_OK;
}

// Compaction of a pass that is going to be kept (rasterizer.KeptPasses): the pass' record array and quadrant streams are laid out
// by the tile ranges of the SORTED list (tile t at range.x, capacity n_t = its list length), but a tile only ever packed the
// k_t <= n_t records its pixels needed (qcount[t][4]: 15 % of the list on a ScanNet-class view, where the workgroups leave early).
// One workgroup per tile copies the k_t records and the four quadrant streams to the offsets of the NEW ranges (exclusive scan of
// k_t, built by the caller): 6 x less to keep for such a view.  The fifth region of the stream block (positions in the full
// list, read by the n_contrib export only) is not carried over.
template <int C>
__global__ __launch_bounds__(kBlock) void compact_kept_kernel(const uint2* __restrict__ old_ranges, const uint2* __restrict__ new_ranges,
                                                              const uint32_t* __restrict__ qcount, const float4* __restrict__ old_rec,
                                                              const uint32_t* __restrict__ old_quad, float4* __restrict__ new_rec,
                                                              uint32_t* __restrict__ new_quad) {
    constexpr int SV = stream_vec4(C);
    const int tile = blockIdx.x;
    const uint2 ro = old_ranges[tile], rn = new_ranges[tile];
    const uint32_t n_old = ro.y - ro.x, k = qcount[tile * 5 + 4];
    const float4* __restrict__ src = old_rec + (size_t)ro.x * SV;
    float4* __restrict__ dst = new_rec + (size_t)rn.x * SV;
    for (uint32_t e = threadIdx.x; e < k * SV; e += kBlock) dst[e] = src[e];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t nq = qcount[tile * 5 + q];
        const uint32_t* __restrict__ qs = old_quad + ((size_t)ro.x * 5 + (size_t)q * n_old);
        uint32_t* __restrict__ qd = new_quad + ((size_t)rn.x * 5 + (size_t)q * k);
        for (uint32_t e = threadIdx.x; e < nq; e += kBlock) qd[e] = qs[e];
    }
}

template <int C>
int compact_c(int W, int H, const ImageState& is_old, const ImageState& is_new, const void* old_rec, const void* old_quad,
              void* new_rec, void* new_quad, hipStream_t s) {
    const int gx = (W + kTile - 1) / kTile, gy = (H + kTile - 1) / kTile;
    OGS_LAUNCH(compact_kept_kernel<C>, dim3((unsigned)(gx * gy)), dim3(kBlock), 0, s, (const uint2*)is_old.ranges,
               (const uint2*)is_new.ranges, (const uint32_t*)is_old.qcount, (const float4*)stream_base<C>(const_cast<void*>(old_rec)),
               (const uint32_t*)quad_base(const_cast<void*>(old_quad)), stream_base<C>(new_rec), quad_base(new_quad));
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

template <int C>
int export_c(const OgsRasterFwdArgs& a, const ImageState& is, uint32_t* out, hipStream_t s) {
    const int gx = (a.W + kTile - 1) / kTile, gy = (a.H + kTile - 1) / kTile;
    OGS_LAUNCH(export_n_contrib_kernel<C>, dim3((unsigned)(gx * gy) * (unsigned)num_groups_of(a.num_groups)), dim3(kBlock), 0,
               s, (const uint2*)is.ranges, (const uint32_t*)a.point_list, (const uint32_t*)quad_base(a.quad_list), a.W,
               a.H, gx, gx * gy, (const uint32_t*)is.n_contrib, out);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

constexpr const char* kBadC = "unsupported channel count C=%d";

}  // namespace

static bool tile_order_enabled() {
    static const bool v = [] { const char* e = getenv("OGS_TILE_ORDER"); return !(e && atoi(e) == 0); }();
    return v;
}
const uint32_t* tile_order_of(const ImageState& is, int64_t vtiles, int P) {
    return (tile_order_enabled() && vtiles > 1 && vtiles <= kOrderMaxTiles && (int64_t)P >= 4 * vtiles) ? is.tile_order : nullptr;
}
const uint32_t* launch_tile_order(const ImageState& is, int64_t vtiles, int P, hipStream_t s, int debug) {
    const uint32_t* order = tile_order_of(is, vtiles, P);
    if (!order) return nullptr;
    OGS_LAUNCH(tile_order_kernel, dim3(1), dim3(kOrderThreads), 0, s, (const uint2*)is.ranges, (uint32_t)vtiles, is.tile_order);
    if (debug) (void)hipStreamSynchronize(s);
    return order;
}

int launch_tile_order_test(const uint32_t* ranges, int64_t vtiles, uint32_t* order, hipStream_t s) {
    if (vtiles > kOrderMaxTiles) { set_error("selftest: more than %lld tiles", (long long)kOrderMaxTiles); return OGS_ERR_UNSUPPORTED; }
    OGS_LAUNCH(tile_order_kernel, dim3(1), dim3(kOrderThreads), 0, s, (const uint2*)ranges, (uint32_t)vtiles, order);
    OGS_LAUNCH_CHECK(1, s);
    return OGS_OK;
}

int launch_mfma_rank1_test(const float* w, const float* f, const float* acc0, int steps, float* out_mfma, float* out_fma,
                           hipStream_t s) {
    OGS_LAUNCH(mfma_rank1_test_kernel, dim3(1), dim3(kWave), 0, s, w, f, acc0, steps, out_mfma);
    OGS_LAUNCH(fma_rank1_test_kernel, dim3(4), dim3(256), 0, s, w, f, acc0, steps, out_fma);
    OGS_LAUNCH_CHECK(1, s);
    return OGS_OK;
}

int launch_blend_forward(const OgsRasterFwdArgs& a, const GeomState& gs, const ImageState& is, int64_t D,
                         hipStream_t s, bool order_ready) {
    return dispatch_channels<12>(a.C, kBadC, [&](auto c) { return launch_c<c()>(a, gs, is, D, s, order_ready); });
}

int launch_group_stats(const OgsRasterFwdArgs& a, const OgsGroupStatsArgs& st, const GeomState& gs, const ImageState& is,
                       hipStream_t s, bool order_ready) {
    return dispatch_channels<12>(a.C, kBadC, [&](auto c) { return stats_c<c()>(a, st, gs, is, s, order_ready); });
}

int launch_compact_kept(int W, int H, int C, const ImageState& is_old, const ImageState& is_new, const void* old_rec,
                        const void* old_quad, void* new_rec, void* new_quad, hipStream_t s) {
    return dispatch_channels<12>(C, kBadC, [&](auto c) {
        return compact_c<c()>(W, H, is_old, is_new, old_rec, old_quad, new_rec, new_quad, s);
    });
}

int launch_reblend(const OgsRasterFwdArgs& a, const ImageState& is, hipStream_t s) {
    return dispatch_channels<12>(a.C, kBadC, [&](auto c) { return reblend_c<c()>(a, is, s); });
}

int launch_tiny_blend(const OgsRasterFwdArgs& a, const GeomState& gs, const uint32_t* order, hipStream_t s) {
    return dispatch_channels<12>(a.C, kBadC, [&](auto c) { return tiny_c<c()>(a, gs, order, s); });
}

int launch_export_n_contrib(const OgsRasterFwdArgs& a, const ImageState& is, uint32_t* out, hipStream_t s) {
    return dispatch_channels<12>(a.C, kBadC, [&](auto c) { return export_c<c()>(a, is, out, s); });
}

}  // namespace ogs
