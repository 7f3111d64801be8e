// The walk of a finished ("kept") ungrouped streaming pass, shared by the kernels that visit it again: label_map.hip,
// label_votes.hip, feature_votes.hip and feature_map.hip (internal; the public C ABI is include/ogs_query.h).
//
// One workgroup per tile, wave = 8x8 quadrant, lane = pixel.  A wave takes its quadrant's stream 64 entries at a time: lane e
// parks the geometry of record e in LDS, with the row the kernel counts the entry under in place of the Gaussian id, and the wave
// walks the 64 entries with the record broadcast from LDS, T / done / the stop rule per lane.  The per-pixel arithmetic restates
// QuadWalk::consume (blend_fwd.hip) as refine.hip does: blend_power, the candidate window |power + h| <= h,
// min(0.99, opacity * __expf(power)), the 1/255 skip and the stop at T * (1 - alpha) < 1e-4, in the same operation order; every
// file that includes this header is compiled with -ffp-contract=off, so w = alpha * T is the weight the blend adds to out_alpha,
// bit for bit.  The 4x4-block sublists of QuadWalk::step are a speed device of the blend and are not restated.
//
// There is ONE definition of each step here, so that what the four kernels promise about each other (alpha equal to the pass's,
// the feature map equal to the re-blend route, one-hot feature votes equal to the label votes, the adjoint identity between the
// map and the votes) does not rest on copies staying equal.  Everything is forced inline and parameterised by callables: no
// function pointers, no state in memory beyond the wave's 2 KiB of parked records.
#pragma once

#include "ogs_common.h"

namespace ogs {

constexpr float kAlphaMin = 1.0f / 255.0f;
constexpr int kWaves = kBlock / kWave;
constexpr int kFoldRows = 16;                        // entries per batch of a fold on the matrix pipe
constexpr int kFoldCols = 16;                        // columns per MFMA block
typedef float floatx4 __attribute__((ext_vector_type(4)));

// ---- the rows of a table [R, ...] ------------------------------------------------------------------------------------------------
// row_of of the kernels that count per Gaussian or per mapped row: rows_of[id] (id itself when rows_of is NULL) inside [0, R),
// else -1 -- the entry occludes and is not counted
struct TableRow {
    const int32_t* __restrict__ rows_of;
    int P, R;
    __device__ __forceinline__ int32_t operator()(float id_bits) const {
        const uint32_t id = __float_as_uint(id_bits);
        int32_t row = -1;
        if (id < (uint32_t)P) {
            const int32_t r = rows_of ? rows_of[id] : (int32_t)id;
            if (r >= 0 && r < R) row = r;
        }
        return row;
    }
};

// ---- a wave's quadrant of a kept pass ----------------------------------------------------------------------------------------------
struct KeptQuad {
    int tile, wave, lane;
    int qx0, qy0, px, py;                            // the quadrant's corner, the lane's pixel
    bool inside;
    float fx, fy;
    int n, n_kept;                                   // entries of the quadrant's stream, records the tile packed
    int RS;                                          // floats per record
    const float* __restrict__ tb;                    // the tile's records
    const uint32_t* __restrict__ qi;                 // the quadrant's indices into them
    uint32_t lim;                                    // largest index a record is read at

    // Two steps, so that the kernel's exit stands between them:
    //     KeptQuad q;
    //     if (!q.find_tile(tiles, tile_order)) return;          // block-uniform
    //     q.setup(ranges, qcount, stream, RS, quad_list, W, H, gx);
    // A set-up in one call that returns false leaves a merge of its two paths in front of the kernel's return, and that merge
    // costs the compiler what it knows about lane, wave and n (their known bits and their uniformity: adds for ors in the LDS
    // addressing, a vector loop counter) -- measured while this header was written.
    //
    // false: the tile index lies outside [0, tiles) -- an order the pass never wrote addresses nothing
    __device__ __forceinline__ bool find_tile(int tiles, const uint32_t* __restrict__ tile_order) {
        tile = tile_order ? (int)tile_order[blockIdx.x] : (int)blockIdx.x;
        return (unsigned)tile < (unsigned)tiles;
    }
    // n <= 0 is wave-uniform and left to the kernel: one that owes every pixel an output must not return on it.
    __device__ __forceinline__ void setup(const uint2* __restrict__ ranges, const uint32_t* __restrict__ qcount,
                                          const float* __restrict__ stream, int RS_, const uint32_t* __restrict__ quad_list, int W,
                                          int H, int gx) {
        const int tx = tile % gx, ty = tile / gx;
        const int tid = threadIdx.x;
        lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        qx0 = tx * kTile + (wave & 1) * 8;
        qy0 = ty * kTile + (wave >> 1) * 8;
        px = qx0 + (lane & 7);
        py = qy0 + (lane >> 3);
        inside = px < W && py < H;
        fx = (float)px;
        fy = (float)py;
        // both layouts with one formula (blend_forward_rows_kernel): the tile owns n_tile slots at range.x, of which it packed n_kept
        const uint2 range = ranges[tile];
        const int n_tile = (int)(range.y - range.x);
        n = min((int)qcount[tile * 5 + wave], n_tile);
        n_kept = min((int)qcount[tile * 5 + 4], n_tile);
        RS = RS_;
        tb = stream + (size_t)range.x * RS;
        qi = quad_list + ((size_t)range.x * 5 + (size_t)wave * n_tile);
        lim = n_kept > 0 ? (uint32_t)n_kept - 1u : 0u;
    }

    // One walk of the quadrant's stream from T = 1.  rec: the wave's 2 * kWave float4 of LDS.  row_of(id_bits) -> int32_t gives
    // the row of a record (lane e asks for record e of the chunk); on_entry(row, w) is called once per entry that had a candidate
    // lane, in depth order: row is wave-uniform, w the lane's weight alpha * T, 0 where stopped, skipped or outside.
    template <class RowOf, class OnEntry>
    __device__ __forceinline__ void walk(float4* __restrict__ rec, RowOf&& row_of, OnEntry&& on_entry) const {
        float T = 1.0f;
        bool done = !inside;
        for (int c0 = 0; c0 < n && __ballot(!done) != 0ull; c0 += kWave) {
            const int chunk = min(kWave, n - c0);
            if (lane < chunk) {
                const uint32_t ridx = min(qi[c0 + lane], lim);
                const float4* __restrict__ rp = reinterpret_cast<const float4*>(tb + (size_t)ridx * RS);
                const float4 g0 = rp[0], g1 = rp[1];
                const int32_t row = row_of(g1.w);
                rec[lane * 2] = g0;
                rec[lane * 2 + 1] = make_float4(g1.x, g1.y, g1.z, __int_as_float(row));     // the id has served: its slot carries the row
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int e = 0; e < chunk && __ballot(!done) != 0ull; ++e) {
                const float4 g0 = rec[e * 2], g1 = rec[e * 2 + 1];               // x y a2 c2 | b2 h opacity row
                const float dx = g0.x - fx, dy = g0.y - fy;
                const float power = blend_power(g0.z, g1.x, g0.w, dx, dy);
                const bool cand = !done && fabsf(power + g1.y) <= g1.y;
                if (__ballot(cand) == 0ull) continue;
                const float araw = fminf(0.99f, g1.z * __expf(power));
                const bool act = cand && araw >= kAlphaMin;
                const float alpha = act ? araw : 0.f;
                const float test_T = T * (1.0f - alpha);
                const bool stop = test_T < 0.0001f;
                const float w = stop ? 0.f : alpha * T;
                T = stop ? T : test_T;
                done = done || stop;
                on_entry(__builtin_amdgcn_readfirstlane(__float_as_int(g1.w)), w);   // the same word in every lane
            }
            __builtin_amdgcn_wave_barrier();                                     // the staging may be rewritten
        }
    }
};

// ---- the vote fold: weights of a batch of entries x a B tile of the wave's 64 pixels, added to an int64 table --------------------
// Entries that put weight on the quadrant and map to a counted row are staged kFoldRows at a time (one ds_write of the 64 weights
// each); the batch is then folded on the matrix pipe per block of kFoldCols columns as
//     D[16 entries, 16 columns] = Wt[16, 64 pixels] x B[64 pixels, 16 columns]          v_mfma_f32_16x16x4_f32, exact fp32
// sixteen MFMAs in two accumulator chains (even and odd k-steps), pixel 4 j + kq at step j.  A partial -- one entry, one quadrant,
// one column -- is therefore the fp32 value
//     (chain over even j of fma(w[4 j + k], B[4 j + k, c], acc), k = 0..3, from +0) + (the same chain over odd j)
// a function of that column's 64 B values and of the weights only.  It is rounded ONCE, __float2ll_rn(partial * 2^32) (the rule of
// the group statistics, kFixedScale in blend_fwd.hip), and added to its cell with a 64-bit integer atomic from the vector lanes,
// in two's complement; integer addition commutes, so two runs give the same bytes and V views sum into one table.
constexpr float kVoteScale = 4294967296.0f;          // 2^32
constexpr int kFoldStride = 66;                      // row stride in words: the transposed read is bank-conflict free
constexpr int kFoldWords = kFoldRows * kFoldStride;  // LDS words of a wave's staged weights, [entry][pixel]

struct VoteFold {
    float* __restrict__ wbuf;                        // the wave's kFoldWords
    int lane, m, kq;                                 // operand row / column m, k group kq
    int cnt;                                         // wave-uniform: entries staged
    int32_t rowv;                                    // lane e: table row of staged entry e

    __device__ __forceinline__ void init(float* __restrict__ wbuf_, int lane_) {
        wbuf = wbuf_;
        lane = lane_;
        m = lane_ & 15;
        kq = lane_ >> 4;
        cnt = 0;
        rowv = -1;
    }
    // true: the batch is full and must be folded before the next entry
    __device__ __forceinline__ bool stage(float w, int32_t row) {
        wbuf[cnt * kFoldStride + lane] = w;
        if (lane == cnt) rowv = row;
        return ++cnt == kFoldRows;
    }
    // the A operand of the batch (entry m, pixels 4 j + kq) and the rows of the four entries 4 kq + r whose partials the lane gets
    __device__ __forceinline__ void operands(float (&a)[16], int32_t (&rowr)[4]) const {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < 16; ++j) a[j] = m < cnt ? wbuf[m * kFoldStride + 4 * j + kq] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) rowr[r] = __shfl(rowv, 4 * kq + r, kWave);
    }
    // the partials of one column block: b(j) is the lane's B value of pixel 4 j + kq (j a constant after unrolling)
    template <class B>
    static __device__ __forceinline__ floatx4 partials(const float (&a)[16], B&& b) {
        floatx4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = d0;
#pragma unroll
        for (int j = 0; j < 16; j += 2) {
            d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b(j), d0, 0, 0, 0);
            d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j + 1], b(j + 1), d1, 0, 0, 0);
        }
        return d0 + d1;
    }
    // the lane's four partials to votes[row, col] of a table of last_col + 1 columns; zero partials are skipped.  Every index is
    // checked where it is used: a staged row lies in [0, R), a column in [0, last_col]
    __device__ __forceinline__ void add(const floatx4& d, const int32_t (&rowr)[4], int col, int last_col, int R,
                                        unsigned long long* __restrict__ votes) const {
        const int64_t pitch = (int64_t)last_col + 1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int e = 4 * kq + r;
            const int32_t row = rowr[r];
            if (e < cnt && d[r] != 0.f && (uint32_t)row < (uint32_t)R && col >= 0 && col <= last_col)
                atomicAdd(votes + ((size_t)row * (size_t)pitch + (size_t)col),
                          (unsigned long long)__float2ll_rn(d[r] * kVoteScale));      // two's complement: the sign carries
        }
    }
    __device__ __forceinline__ void reset() {
        cnt = 0;
        __builtin_amdgcn_wave_barrier();             // the staging may be rewritten
    }
};

// ---- host side: the arguments every entry point over a kept pass shares ------------------------------------------------------------
struct KeptPass {
    const uint2* ranges;
    const uint32_t* qcount;
    const float* stream;
    int RS;
    const uint32_t* quad_list;
    int W, H, gx, tiles;
    const uint32_t* order;                           // heaviest first, as the kept pass ran
    int P;
    bool pointers;                                   // image_buffer, sorted_rec and quad_list are all there
    hipStream_t s;
};
// the leading kernel arguments, in the order every kernel over a kept pass declares them
#define OGS_KEPT_PASS_ARGS(kp) \
    (kp).ranges, (kp).qcount, (kp).stream, (kp).RS, (kp).quad_list, (kp).W, (kp).H, (kp).gx, (kp).tiles, (kp).order, (kp).P

// Validates what the entry points share, in their order (args, sizes, channel set, groups), with `who` in front of the messages,
// and fills kp.  The entry point goes on with its own counts and then its pointers (kept_pass_null together with kp.pointers).
inline int kept_pass_of(const char* who, const OgsRasterFwdArgs* a, const void* own, void* stream_, KeptPass* kp) {
    if (!a || !own) { set_error("%s: args == NULL", who); return OGS_ERR_INVALID_ARG; }
    if (a->P <= 0 || a->W <= 0 || a->H <= 0) { set_error("%s: bad sizes P=%d W=%d H=%d", who, a->P, a->W, a->H); return OGS_ERR_INVALID_ARG; }
    if (a->C != 3 && a->C != 6 && a->C != 9 && a->C != 12) { set_error("C=%d unsupported (3, 6, 9, 12)", a->C); return OGS_ERR_UNSUPPORTED; }
    if (a->num_groups > 1) { set_error("%s: grouped passes are not supported", who); return OGS_ERR_UNSUPPORTED; }
    const ImageState is = ImageState::carve(a->image_buffer, a->W, a->H, 1);
    kp->ranges = is.ranges;
    kp->qcount = is.qcount;
    kp->stream = static_cast<const float*>(a->sorted_rec);
    kp->RS = stream_vec4(a->C) * 4;
    kp->quad_list = a->quad_list ? quad_base(a->quad_list) : nullptr;
    kp->W = a->W;
    kp->H = a->H;
    kp->gx = (a->W + kTile - 1) / kTile;
    kp->tiles = kp->gx * ((a->H + kTile - 1) / kTile);
    kp->order = tile_order_of(is, kp->tiles, a->P);
    kp->P = a->P;
    kp->pointers = a->image_buffer && a->sorted_rec && a->quad_list;
    kp->s = static_cast<hipStream_t>(stream_);
    return OGS_OK;
}
inline int kept_pass_null(const char* who, const char* own_names) {
    set_error("%s: NULL required pointer (image_buffer, sorted_rec, quad_list, %s)", who, own_names);
    return OGS_ERR_INVALID_ARG;
}

}  // namespace ogs
