// Image-space mask reductions for gfx950 (include/ogs_mask.h).
//
// The reference expands the feature map to [num_mask, C, H, W] (several GB at 1080p) to take per-mask means and
// distances (utils/opengs_utlis.py:240-283, train.py:102-122).  Here every kernel is one streaming pass:
// a lane owns 4 consecutive pixels (float4 / u32 loads when H*W is a multiple of 4), a wave a 256-pixel strip,
// and the mask stack is walked with one u32 per lane and mask.  A mask with no pixel in the strip costs one
// ballot; a mask that is present contributes its partial sums through the 16-slot transposed wave fold
// (wave_fold.h) and ONE float-atomic instruction on a contiguous table row.  HBM-bound: feat + weight once,
// N bytes per pixel of masks.  The label form is the same passes over ONE int32 label image (disjoint masks):
// 4 bytes per pixel of masks whatever N is, and a loop over the distinct labels of the strip in place of the stack walk.
// The reducing forward kernels are written once, over a membership policy (Stack / Label below) that owns what the two
// forms do differently: the pixel loader, the walk over the rows present in a wave's strip, and "pixel j is in row n".
#include <initializer_list>
#include <type_traits>

#include "ogs_common.h"
#include "wave_fold.h"
#include "../../include/ogs_mask.h"

namespace ogs {

namespace {

constexpr int kPix = 4;                       // pixels per lane
constexpr int kStrip = kBlock * kPix;         // pixels per workgroup
constexpr int kMaskUnroll = 8;                // mask words in flight per lane
constexpr int kRow = OGS_MASK_TABLE_STRIDE;   // floats between table rows: one 64-byte atomic segment per mask

template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ p, int64_t i0, int64_t n, float out[kPix]) {
    if (VEC) {
        const float4 v = (i0 < n) ? *reinterpret_cast<const float4*>(p + i0) : make_float4(0.f, 0.f, 0.f, 0.f);
        out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < kPix; ++j) out[j] = (i0 + j < n) ? p[i0 + j] : 0.f;
    }
}

// load4 with the bounds test moved from the load to the address: past the end a lane re-reads element 0 (n > 0 in every
// launch) and zeroes the result, so nothing branches around a load and the C + 2 loads of a lane are all in flight at
// once.  (The label kernels move so few bytes that a whole 1080p launch is ONE round of resident waves: a chain of
// load -> wait -> load would be its run time.)
template <bool VEC, typename T>
__device__ __forceinline__ void load4_clamped(const T* __restrict__ p, int64_t i0, int64_t n, T out[kPix]) {
    if (VEC) {
        typedef T vec4 __attribute__((ext_vector_type(4)));
        const bool ok = i0 < n;
        const vec4 v = *reinterpret_cast<const vec4*>(p + (ok ? i0 : 0));
        out[0] = ok ? v.x : T(0); out[1] = ok ? v.y : T(0); out[2] = ok ? v.z : T(0); out[3] = ok ? v.w : T(0);
    } else {
#pragma unroll
        for (int j = 0; j < kPix; ++j) {
            const bool ok = i0 + j < n;
            const T v = p[ok ? i0 + j : 0];
            out[j] = ok ? v : T(0);
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ p, int64_t i0, int64_t n, const float v[kPix]) {
    if (VEC) {
        if (i0 < n) *reinterpret_cast<float4*>(p + i0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < kPix; ++j)
            if (i0 + j < n) p[i0 + j] = v[j];
    }
}

// ---- membership policies ------------------------------------------------------------------------------------------------
// What a kernel needs to know about how the masks are stored.  `elem` / `kAlign`: the element type and the alignment the
// vector path asks of the pointer; `load`: the form's 4-pixel loader for the fp32 maps; `for_each_present(N, HW, i0,
// body)`: calls `body(n, hit)` (wave-uniformly) once for every row n that has a pixel somewhere in the wave's strip,
// `hit.in(j)` saying whether this lane's pixel j lies in row n; `names`: the timing name of each kernel in this form.
// The kernels take the pointer as a plain argument and build the policy around it.
struct Names { const char *sums, *sums_backward, *cohesion, *sqdev, *cohesion_backward; };

// the [N, H, W] byte stack: masks may overlap
template <bool VEC>
struct Stack {
    using elem = uint8_t;
    static constexpr size_t kAlign = 4;       // one u32 of 4 mask bytes
    static constexpr Names names{"mask_feature_sums_kernel", "mask_feature_sums_backward_kernel", "mask_cohesion_kernel",
                                 "mask_feature_sqdev_kernel", "mask_cohesion_backward_kernel"};
    const uint8_t* __restrict__ masks;

    static __device__ __forceinline__ void load(const float* __restrict__ p, int64_t i0, int64_t n, float out[kPix]) {
        load4<VEC>(p, i0, n, out);
    }

    // byte j of the word != 0  <=>  pixel i0 + j lies inside the mask
    struct Hit {
        uint32_t word;
        __device__ __forceinline__ bool in(int j) const { return ((word >> (8 * j)) & 0xFFu) != 0u; }
    };

    static __device__ __forceinline__ uint32_t mask_word(const uint8_t* __restrict__ m, int64_t i0, int64_t n) {
        if (VEC) return (i0 < n) ? *reinterpret_cast<const uint32_t*>(m + i0) : 0u;
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < kPix; ++j)
            if (i0 + j < n) w |= (uint32_t)m[i0 + j] << (8 * j);
        return w;
    }

    // Walk the mask stack for this lane's 4 pixels; `body` runs only for masks that have a pixel in the wave's strip.
    template <typename F>
    __device__ __forceinline__ void for_each_present(int N, int64_t HW, int64_t i0, F&& body) const {
        for (int n0 = 0; n0 < N; n0 += kMaskUnroll) {
            uint32_t mw[kMaskUnroll];
#pragma unroll
            for (int j = 0; j < kMaskUnroll; ++j)
                mw[j] = (n0 + j < N) ? mask_word(masks + (size_t)(n0 + j) * HW, i0, HW) : 0u;
#pragma unroll
            for (int j = 0; j < kMaskUnroll; ++j) {
                if (__ballot(mw[j] != 0u) == 0ull) continue;
                body(n0 + j, Hit{mw[j]});
            }
        }
    }
};

// ONE int32 label image instead of the [N,H,W] byte stack (the masks of one SAM level are disjoint).  Pixel p lies in
// row labels[p] - 1 when 1 <= labels[p] <= N and in no row otherwise (0 = invalid, negative, > N): 4 bytes per pixel of
// masks whatever N is.  row[j] = that row, or -1; only a row that passed the range test is ever used as an address.
template <bool VEC>
struct Label {
    using elem = int32_t;
    static constexpr size_t kAlign = 16;      // one vector of 4 labels
    static constexpr Names names{"label_feature_sums_kernel", "label_feature_sums_backward_kernel", "label_cohesion_kernel",
                                 "label_feature_sqdev_kernel", "label_cohesion_backward_kernel"};
    const int32_t* __restrict__ labels;

    static __device__ __forceinline__ void load(const float* __restrict__ p, int64_t i0, int64_t n, float out[kPix]) {
        load4_clamped<VEC>(p, i0, n, out);
    }

    // bit j set  <=>  pixel i0 + j lies in the row
    struct Hit {
        uint32_t bits;
        __device__ __forceinline__ bool in(int j) const { return (bits >> j) & 1u; }
    };

    static __device__ __forceinline__ int label_row(int l, int N) {
        const uint32_t r = (uint32_t)l - 1u;                  // unsigned: no label value can overflow
        return (r < (uint32_t)N) ? (int)r : -1;
    }

    __device__ __forceinline__ void load_rows(int N, int64_t HW, int64_t i0, int row[kPix]) const {
        int l[kPix];
        load4_clamped<VEC>(labels, i0, HW, l);
#pragma unroll
        for (int j = 0; j < kPix; ++j) row[j] = label_row(l[j], N);
    }

    // `body(n, hit)` once for every distinct row n among the wave's `row` values.  Each lane keeps a 4-bit set of its
    // pixels still pending; a trip takes the first pending row of the first pending lane and every lane retires all of
    // its pixels in that row, so a trip retires at least one pixel and the loop ends after at most 256 trips whatever
    // the labels hold.
    template <typename F>
    static __device__ __forceinline__ void for_each_present_row(const int row[kPix], F&& body) {
        uint32_t pending = 0u;
#pragma unroll
        for (int j = 0; j < kPix; ++j) pending |= (row[j] >= 0 ? 1u : 0u) << j;
        for (;;) {
            const unsigned long long live = __ballot(pending != 0u);
            if (live == 0ull) break;
            const int src = __ffsll(live) - 1;
            const int first = (pending & 1u) ? row[0] : (pending & 2u) ? row[1] : (pending & 4u) ? row[2] : row[3];
            const int n = __builtin_amdgcn_readlane(first, src);          // wave-uniform: row reads go the scalar way
            uint32_t hit = 0u;
#pragma unroll
            for (int j = 0; j < kPix; ++j) hit |= (row[j] == n ? 1u : 0u) << j;
            pending &= ~hit;
            body(n, Hit{hit});
        }
    }

    template <typename F>
    __device__ __forceinline__ void for_each_present(int N, int64_t HW, int64_t i0, F&& body) const {
        int row[kPix];
        load_rows(N, HW, i0, row);
        for_each_present_row(row, body);
    }
};

// ---- the reducing forward kernels, once for both forms (M = Stack<VEC> or Label<VEC>) --------------------------------------
template <typename M, int C, bool SQ>
__global__ __launch_bounds__(kBlock) void feature_sums_kernel(const float* __restrict__ feat,
                                                              const typename M::elem* __restrict__ member,
                                                              const float* __restrict__ weight, int N, int64_t HW,
                                                              float* __restrict__ table) {
    constexpr int WIDTH = SQ ? 2 * C + 1 : C + 1;
    static_assert(WIDTH <= 16, "table row must fit the 16-slot fold");
    const M m{member};
    const int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kPix;
    float f[C][kPix], w[kPix];
#pragma unroll
    for (int c = 0; c < C; ++c) M::load(feat + (size_t)c * HW, i0, HW, f[c]);
    if (weight) M::load(weight, i0, HW, w);
    else {
#pragma unroll
        for (int j = 0; j < kPix; ++j) w[j] = 1.f;
    }
    const int lane = lane_id();
    m.for_each_present(N, HW, i0, [&](int n, typename M::Hit hit) {
        float v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = 0.f;
#pragma unroll
        for (int j = 0; j < kPix; ++j) {
            const float wj = hit.in(j) ? w[j] : 0.f;
            v[C] += wj;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float t = wj * f[c][j];
                v[c] += t;
                if (SQ) v[C + 1 + c] += t * f[c][j];
            }
        }
        const float y = wave_fold16(v);
        const int slot = lane >> 2;
        if ((lane & 3) == 0 && slot < WIDTH) atomicAdd(table + (size_t)n * kRow + slot, y);
    });
}

template <typename M, int C>
__global__ __launch_bounds__(kBlock) void cohesion_kernel(const float* __restrict__ feat,
                                                          const typename M::elem* __restrict__ member,
                                                          const float* __restrict__ mean, int N, int64_t HW,
                                                          float* __restrict__ table) {
    const M m{member};
    const int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kPix;
    float f[C][kPix];
#pragma unroll
    for (int c = 0; c < C; ++c) M::load(feat + (size_t)c * HW, i0, HW, f[c]);
    const int lane = lane_id();
    m.for_each_present(N, HW, i0, [&](int n, typename M::Hit hit) {
        float mu[C];                                   // wave-uniform row -> scalar loads
#pragma unroll
        for (int c = 0; c < C; ++c) mu[c] = mean[(size_t)n * C + c];
        float v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = 0.f;
#pragma unroll
        for (int j = 0; j < kPix; ++j) {
            float d2 = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float d = f[c][j] - mu[c];
                d2 += d * d;
            }
            const bool in = hit.in(j);
            v[0] += in ? sqrtf(d2) : 0.f;
            v[1] += in ? 1.f : 0.f;
        }
        const float y = wave_fold16(v);
        const int slot = lane >> 2;
        if ((lane & 3) == 0 && slot < 2) atomicAdd(table + (size_t)n * kRow + slot, y);
    });
}

// Second pass of the variance of mask_feature_mean(return_var=True): table[n, c] = sum_pix mask * w * (feat[c] - mean[n, c])^2,
// the deviations formed per pixel from means that are already known.  (The one-pass form sum f^2 - 2 mean sum f + n mean^2
// cancels: on a mask whose features sit at 0.9 +- 0.05 it keeps three of the seven digits of its fp32 sums.)
template <typename M, int C>
__global__ __launch_bounds__(kBlock) void feature_sqdev_kernel(const float* __restrict__ feat,
                                                               const typename M::elem* __restrict__ member,
                                                               const float* __restrict__ weight,
                                                               const float* __restrict__ mean, int N, int64_t HW,
                                                               float* __restrict__ table) {
    const M m{member};
    const int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kPix;
    float f[C][kPix], w[kPix];
#pragma unroll
    for (int c = 0; c < C; ++c) M::load(feat + (size_t)c * HW, i0, HW, f[c]);
    if (weight) M::load(weight, i0, HW, w);
    else {
#pragma unroll
        for (int j = 0; j < kPix; ++j) w[j] = 1.f;
    }
    const int lane = lane_id();
    m.for_each_present(N, HW, i0, [&](int n, typename M::Hit hit) {
        float mu[C];                                   // wave-uniform row -> scalar loads
#pragma unroll
        for (int c = 0; c < C; ++c) mu[c] = mean[(size_t)n * C + c];
        float v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = 0.f;
#pragma unroll
        for (int j = 0; j < kPix; ++j) {
            const float wj = hit.in(j) ? w[j] : 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float d = f[c][j] - mu[c];
                v[c] += wj * d * d;
            }
        }
        const float y = wave_fold16(v);
        const int slot = lane >> 2;
        if ((lane & 3) == 0 && slot < C) atomicAdd(table + (size_t)n * kRow + slot, y);
    });
}

// ---- the backward kernels: a different algorithm per form -------------------------------------------------------------------
// Stack: walk the stack and accumulate per pixel over the masks that hold it.
// DW: also the gradient w.r.t. the weight map, dweight[pix] = sum_n mask * (sum_c coef[n,c] * feat[c,pix] + coef_cnt[n])
// (the silhouette the reference passes as image_mask is an output of the rasterizer and so part of the graph).
template <int C, bool VEC, bool DW>
__global__ __launch_bounds__(kBlock) void mask_feature_sums_backward_kernel(const uint8_t* __restrict__ masks,
                                                                            const float* __restrict__ weight,
                                                                            const float* __restrict__ coef,
                                                                            const float* __restrict__ feat,
                                                                            const float* __restrict__ coef_cnt, int N,
                                                                            int64_t HW, float* __restrict__ dfeat,
                                                                            float* __restrict__ dweight) {
    using M = Stack<VEC>;
    const M m{masks};
    const int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kPix;
    float acc[C][kPix], w[kPix], accn[kPix];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int j = 0; j < kPix; ++j) acc[c][j] = 0.f;
#pragma unroll
    for (int j = 0; j < kPix; ++j) accn[j] = 0.f;
    if (weight) M::load(weight, i0, HW, w);
    else {
#pragma unroll
        for (int j = 0; j < kPix; ++j) w[j] = 1.f;
    }
    m.for_each_present(N, HW, i0, [&](int n, typename M::Hit hit) {
        float cf[C];                                   // wave-uniform row -> scalar loads
#pragma unroll
        for (int c = 0; c < C; ++c) cf[c] = coef[(size_t)n * C + c];
        const float cn = DW ? coef_cnt[n] : 0.f;
#pragma unroll
        for (int j = 0; j < kPix; ++j) {
            const bool in = hit.in(j);
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c][j] += in ? cf[c] : 0.f;
            if (DW) accn[j] += in ? cn : 0.f;
        }
    });
    if (DW) {
        // sum_n mask * sum_c coef[n,c] * f[c]  ==  sum_c f[c] * (sum_n mask * coef[n,c])  ==  sum_c f[c] * acc[c]
        float dw[kPix];
#pragma unroll
        for (int j = 0; j < kPix; ++j) dw[j] = accn[j];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float f[kPix];
            M::load(feat + (size_t)c * HW, i0, HW, f);
#pragma unroll
            for (int j = 0; j < kPix; ++j) dw[j] += f[j] * acc[c][j];
        }
        store4<VEC>(dweight, i0, HW, dw);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int j = 0; j < kPix; ++j) acc[c][j] *= w[j];
        store4<VEC>(dfeat + (size_t)c * HW, i0, HW, acc[c]);
    }
}

template <int C, bool VEC>
__global__ __launch_bounds__(kBlock) void mask_cohesion_backward_kernel(const float* __restrict__ feat,
                                                                        const uint8_t* __restrict__ masks,
                                                                        const float* __restrict__ mean,
                                                                        const float* __restrict__ gl, int N, int64_t HW,
                                                                        float* __restrict__ dfeat,
                                                                        float* __restrict__ dmean) {
    using M = Stack<VEC>;
    const M m{masks};
    const int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kPix;
    float f[C][kPix], acc[C][kPix];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        M::load(feat + (size_t)c * HW, i0, HW, f[c]);
#pragma unroll
        for (int j = 0; j < kPix; ++j) acc[c][j] = 0.f;
    }
    const int lane = lane_id();
    m.for_each_present(N, HW, i0, [&](int n, typename M::Hit hit) {
        float mu[C];
#pragma unroll
        for (int c = 0; c < C; ++c) mu[c] = mean[(size_t)n * C + c];
        const float g = gl[n];
        float v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = 0.f;
#pragma unroll
        for (int j = 0; j < kPix; ++j) {
            float d[C], d2 = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                d[c] = f[c][j] - mu[c];
                d2 += d[c] * d[c];
            }
            const float dist = sqrtf(d2);
            // d||x|| / dx = x / ||x||, defined as 0 at x = 0 (torch.norm's subgradient)
            const float s = (hit.in(j) && dist > 0.f) ? g / dist : 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float t = d[c] * s;
                acc[c][j] += t;
                v[c] -= t;
            }
        }
        const float y = wave_fold16(v);
        const int slot = lane >> 2;
        if ((lane & 3) == 0 && slot < C) atomicAdd(dmean + (size_t)n * kRow + slot, y);
    });
#pragma unroll
    for (int c = 0; c < C; ++c) store4<VEC>(dfeat + (size_t)c * HW, i0, HW, acc[c]);
}

// Label: per pixel, no loop: dfeat[c,pix] = w[pix] * coef[row,c], dweight[pix] = sum_c coef[row,c] * feat[c,pix] + coef_cnt[row],
// a gather by the pixel's own row (neighbouring lanes mostly share it); zeros where the pixel lies in no row.
template <int C, bool VEC, bool DW>
__global__ __launch_bounds__(kBlock) void label_feature_sums_backward_kernel(const int32_t* __restrict__ labels,
                                                                             const float* __restrict__ weight,
                                                                             const float* __restrict__ coef,
                                                                             const float* __restrict__ feat,
                                                                             const float* __restrict__ coef_cnt, int N,
                                                                             int64_t HW, float* __restrict__ dfeat,
                                                                             float* __restrict__ dweight) {
    using M = Label<VEC>;
    const M m{labels};
    const int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kPix;
    float acc[C][kPix], w[kPix], dw[kPix];
    int row[kPix];
    m.load_rows(N, HW, i0, row);
    if (weight) M::load(weight, i0, HW, w);
    else {
#pragma unroll
        for (int j = 0; j < kPix; ++j) w[j] = 1.f;
    }
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
        const bool in = row[j] >= 0;
        const size_t r = in ? (size_t)row[j] : 0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float v = coef[r * C + c];            // row 0 where the pixel has none (N > 0): loaded, not used
            acc[c][j] = in ? v : 0.f;
        }
        if (DW) {
            const float v = coef_cnt[r];
            dw[j] = in ? v : 0.f;
        }
    }
    if (DW) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float f[kPix];
            M::load(feat + (size_t)c * HW, i0, HW, f);
#pragma unroll
            for (int j = 0; j < kPix; ++j) dw[j] += f[j] * acc[c][j];
        }
        store4<VEC>(dweight, i0, HW, dw);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int j = 0; j < kPix; ++j) acc[c][j] *= w[j];
        store4<VEC>(dfeat + (size_t)c * HW, i0, HW, acc[c]);
    }
}

// dfeat is per pixel (mean and gl gathered by the pixel's own row, written in place of the feature registers); dmean is
// minus the sum of those same terms over the pixels of a row, so the row loop only folds what the pixels already hold.
template <int C, bool VEC>
__global__ __launch_bounds__(kBlock) void label_cohesion_backward_kernel(const float* __restrict__ feat,
                                                                         const int32_t* __restrict__ labels,
                                                                         const float* __restrict__ mean,
                                                                         const float* __restrict__ gl, int N, int64_t HW,
                                                                         float* __restrict__ dfeat,
                                                                         float* __restrict__ dmean) {
    using M = Label<VEC>;
    const M m{labels};
    const int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kPix;
    float f[C][kPix];
    int row[kPix];
#pragma unroll
    for (int c = 0; c < C; ++c) M::load(feat + (size_t)c * HW, i0, HW, f[c]);
    m.load_rows(N, HW, i0, row);
    float mu[C][kPix], g[kPix];
#pragma unroll
    for (int j = 0; j < kPix; ++j) {                    // all gathers first: nothing below waits on a load of its own
        const bool in = row[j] >= 0;
        const size_t r = in ? (size_t)row[j] : 0;       // row 0 where the pixel has none (N > 0): g = 0 there
#pragma unroll
        for (int c = 0; c < C; ++c) mu[c][j] = mean[r * C + c];
        const float v = gl[r];
        g[j] = in ? v : 0.f;
    }
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
        float d[C], d2 = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            d[c] = f[c][j] - mu[c][j];
            d2 += d[c] * d[c];
        }
        const float dist = sqrtf(d2);
        // d||x|| / dx = x / ||x||, defined as 0 at x = 0 (torch.norm's subgradient)
        const float s = (row[j] >= 0 && dist > 0.f) ? g[j] / dist : 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) f[c][j] = d[c] * s;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) store4<VEC>(dfeat + (size_t)c * HW, i0, HW, f[c]);
    const int lane = lane_id();
    M::for_each_present_row(row, [&](int n, typename M::Hit hit) {
        float v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = 0.f;
#pragma unroll
        for (int j = 0; j < kPix; ++j)
#pragma unroll
            for (int c = 0; c < C; ++c) v[c] -= hit.in(j) ? f[c][j] : 0.f;
        const float y = wave_fold16(v);
        const int slot = lane >> 2;
        if ((lane & 3) == 0 && slot < C) atomicAdd(dmean + (size_t)n * kRow + slot, y);
    });
}

// the backward kernels of each form, for the host templates below
template <template <bool> class M> struct Backward;
template <> struct Backward<Stack> {
    template <int C, bool VEC, bool DW> static constexpr auto sums = mask_feature_sums_backward_kernel<C, VEC, DW>;
    template <int C, bool VEC> static constexpr auto cohesion = mask_cohesion_backward_kernel<C, VEC>;
};
template <> struct Backward<Label> {
    template <int C, bool VEC, bool DW> static constexpr auto sums = label_feature_sums_backward_kernel<C, VEC, DW>;
    template <int C, bool VEC> static constexpr auto cohesion = label_cohesion_backward_kernel<C, VEC>;
};

// ---- host side: one function per entry-point pair, over the policy template ------------------------------------------------
int check(int C, int N, int64_t HW, const void* a, const void* b, const void* c) {
    if (C != 3 && C != 6) { set_error("mask ops: C=%d unsupported (3 or 6)", C); return OGS_ERR_UNSUPPORTED; }
    if (N < 0 || HW < 0 || HW >= ((int64_t)1 << 40)) { set_error("mask ops: bad sizes N=%d HW=%lld", N, (long long)HW); return OGS_ERR_INVALID_ARG; }
    if ((N > 0 && HW > 0) && (!a || !b || !c)) { set_error("mask ops: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    return OGS_OK;
}

inline dim3 strips(int64_t HW) { return dim3((unsigned)((HW + kStrip - 1) / kStrip)); }

// The vector path (float4 maps, u32 of mask bytes / int4 of labels): H*W a multiple of 4, every fp32 map the kernel
// touches 16-byte aligned or NULL, the membership pointer aligned as its policy says.
template <template <bool> class M>
bool vec_path(int64_t HW, const typename M<true>::elem* member, std::initializer_list<const float*> maps) {
    auto al = [](const void* p, size_t a) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) % a) == 0; };
    bool ok = HW % 4 == 0 && al(member, M<true>::kAlign);
    for (const float* p : maps) ok = ok && al(p, 16);
    return ok;
}

// `launch(c, v)` with the channel count and the vector path as compile-time constants (decltype(c)::value, decltype(v)::value)
template <typename F>
void dispatch(int C, bool vec, F&& launch) {
    using c3 = std::integral_constant<int, 3>;
    using c6 = std::integral_constant<int, 6>;
    if (C == 6) { if (vec) launch(c6{}, std::true_type{}); else launch(c6{}, std::false_type{}); }
    else        { if (vec) launch(c3{}, std::true_type{}); else launch(c3{}, std::false_type{}); }
}

template <template <bool> class M>
int feature_sums(const float* feat, const typename M<true>::elem* member, const float* weight, int C, int N, int64_t HW,
                 int with_squares, float* table, hipStream_t s) {
    int rc = check(C, N, HW, feat, member, table);
    if (rc != OGS_OK) return rc;
    if (N == 0) return OGS_OK;
    OGS_HIP_CHECK(hipMemsetAsync(table, 0, (size_t)N * kRow * sizeof(float), s));
    if (HW == 0) return OGS_OK;
    dispatch(C, vec_path<M>(HW, member, {feat, weight}), [&](auto c, auto v) {
        constexpr int CC = decltype(c)::value;
        using P = M<decltype(v)::value>;
        if (with_squares) OGS_LAUNCH_NAMED(P::names.sums, (feature_sums_kernel<P, CC, true>), strips(HW), dim3(kBlock), 0, s,
                                           feat, member, weight, N, HW, table);
        else OGS_LAUNCH_NAMED(P::names.sums, (feature_sums_kernel<P, CC, false>), strips(HW), dim3(kBlock), 0, s, feat,
                              member, weight, N, HW, table);
    });
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

template <template <bool> class M>
int feature_sums_backward(const typename M<true>::elem* member, const float* weight, const float* coef, const float* feat,
                          const float* coef_cnt, int C, int N, int64_t HW, float* dfeat, float* dweight, hipStream_t s) {
    int rc = check(C, N, HW, member, coef, dfeat);
    if (rc != OGS_OK) return rc;
    if (HW == 0) return OGS_OK;
    if (!dfeat) { set_error("mask ops: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    if (dweight && N > 0 && (!feat || !coef_cnt)) { set_error("mask ops: dweight needs feat and coef_cnt"); return OGS_ERR_INVALID_ARG; }
    if (N == 0) {
        OGS_HIP_CHECK(hipMemsetAsync(dfeat, 0, (size_t)C * HW * sizeof(float), s));
        if (dweight) OGS_HIP_CHECK(hipMemsetAsync(dweight, 0, (size_t)HW * sizeof(float), s));
        return OGS_OK;
    }
    dispatch(C, vec_path<M>(HW, member, {dfeat, weight, feat, dweight}), [&](auto c, auto v) {
        constexpr int CC = decltype(c)::value;
        constexpr bool VV = decltype(v)::value;
        if (dweight) OGS_LAUNCH_NAMED(M<VV>::names.sums_backward, (Backward<M>::template sums<CC, VV, true>), strips(HW),
                                      dim3(kBlock), 0, s, member, weight, coef, feat, coef_cnt, N, HW, dfeat, dweight);
        else OGS_LAUNCH_NAMED(M<VV>::names.sums_backward, (Backward<M>::template sums<CC, VV, false>), strips(HW),
                              dim3(kBlock), 0, s, member, weight, coef, feat, coef_cnt, N, HW, dfeat, dweight);
    });
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

template <template <bool> class M>
int cohesion(const float* feat, const typename M<true>::elem* member, const float* mean, int C, int N, int64_t HW,
             float* table, hipStream_t s) {
    int rc = check(C, N, HW, feat, member, table);
    if (rc != OGS_OK) return rc;
    if (N == 0) return OGS_OK;
    if (!mean) { set_error("mask ops: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    OGS_HIP_CHECK(hipMemsetAsync(table, 0, (size_t)N * kRow * sizeof(float), s));
    if (HW == 0) return OGS_OK;
    dispatch(C, vec_path<M>(HW, member, {feat}), [&](auto c, auto v) {
        using P = M<decltype(v)::value>;
        OGS_LAUNCH_NAMED(P::names.cohesion, (cohesion_kernel<P, decltype(c)::value>), strips(HW), dim3(kBlock), 0, s, feat,
                         member, mean, N, HW, table);
    });
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

template <template <bool> class M>
int feature_sqdev(const float* feat, const typename M<true>::elem* member, const float* weight, const float* mean, int C,
                  int N, int64_t HW, float* table, hipStream_t s) {
    int rc = check(C, N, HW, feat, member, table);
    if (rc != OGS_OK) return rc;
    if (N == 0) return OGS_OK;
    if (!mean) { set_error("mask ops: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    OGS_HIP_CHECK(hipMemsetAsync(table, 0, (size_t)N * kRow * sizeof(float), s));
    if (HW == 0) return OGS_OK;
    dispatch(C, vec_path<M>(HW, member, {feat, weight}), [&](auto c, auto v) {
        using P = M<decltype(v)::value>;
        OGS_LAUNCH_NAMED(P::names.sqdev, (feature_sqdev_kernel<P, decltype(c)::value>), strips(HW), dim3(kBlock), 0, s, feat,
                         member, weight, mean, N, HW, table);
    });
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

template <template <bool> class M>
int cohesion_backward(const float* feat, const typename M<true>::elem* member, const float* mean, const float* gl, int C,
                      int N, int64_t HW, float* dfeat, float* dmean, hipStream_t s) {
    int rc = check(C, N, HW, feat, member, dfeat);
    if (rc != OGS_OK) return rc;
    if (N > 0) {
        if (!mean || !gl || !dmean) { set_error("mask ops: NULL pointer"); return OGS_ERR_INVALID_ARG; }
        OGS_HIP_CHECK(hipMemsetAsync(dmean, 0, (size_t)N * kRow * sizeof(float), s));
    }
    if (HW == 0) return OGS_OK;
    if (!dfeat) { set_error("mask ops: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    if (N == 0) { OGS_HIP_CHECK(hipMemsetAsync(dfeat, 0, (size_t)C * HW * sizeof(float), s)); return OGS_OK; }
    dispatch(C, vec_path<M>(HW, member, {feat, dfeat}), [&](auto c, auto v) {
        constexpr bool VV = decltype(v)::value;
        OGS_LAUNCH_NAMED(M<VV>::names.cohesion_backward, (Backward<M>::template cohesion<decltype(c)::value, VV>), strips(HW),
                         dim3(kBlock), 0, s, feat, member, mean, gl, N, HW, dfeat, dmean);
    });
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

}  // namespace
}  // namespace ogs

using namespace ogs;

// ---- separation_loss (train.py:124-155): [N, N] work on the mask means ------------------------------------------------
// In torch this is ~30 launch-bound little kernels plus two segmented sorts (argsort().argsort() = the rank of every
// element inside its row): 0.3-0.45 ms forward + backward for N = 32..200 masks, as much as a quarter of a stage-1
// iteration.  Here: one workgroup per row i computes inv[i][j] = 1 / (|m_i - m_j|^2 + 1) (0 on the diagonal) into
// LDS, ranks every element inside the row by counting (ties by column index, i.e. a stable sort), applies the
// rank weight and leaves the row's partial loss and its weights; a second launch sums the rows in index order and
// forms the gradient  dL/dm_i = -2 / (N (N-1)) * sum_j (w_ij + w_ji) * inv_ij^2 * (m_i - m_j)  (the weights come from
// sort indices and carry no gradient, as in autograd).
constexpr int kSepMaxN = 1024, kSepMaxC = 16;
__global__ __launch_bounds__(kBlock) void separation_rows_kernel(const float* __restrict__ means, int N, int C, int late,
                                                                 float* __restrict__ weights, float* __restrict__ row_loss) {
    // The rank weights are compared bit for bit with the reference's float32 expression, and the late rule is an exact
    // decision on them.  The pragma keeps every product written in this body rounded on its own; __fmul_rn / __fadd_rn
    // would not (plain * and + in HIP's headers, compiled there under the default -ffp-contract=fast, they fuse once
    // inlined -- (rank / (N-1)) * 0.9 + 0.1 came out as one v_fmamk_f32, off by an ulp for 299 of the 1024 ranks of N = 1024).
#pragma clang fp contract(off)
    __shared__ float s_inv[kSepMaxN];
    __shared__ float s_mi[kSepMaxC];
    __shared__ float s_part[kBlock];
    const int i = blockIdx.x, tid = threadIdx.x;
    if (tid < C) s_mi[tid] = means[(size_t)i * C + tid];
    __syncthreads();
    for (int j = tid; j < N; j += kBlock) {
        float d2 = 0.f;
        for (int c = 0; c < C; ++c) {
            const float d = s_mi[c] - means[(size_t)j * C + c];
            d2 = d2 + d * d;                                // pow(2) then sum(2): no contraction
        }
        s_inv[j] = j == i ? 0.f : 1.0f / (d2 + 1.0f);
    }
    __syncthreads();
    float part = 0.f;
    for (int j = tid; j < N; j += kBlock) {
        const float v = s_inv[j];
        int rank = 0;
        for (int k = 0; k < N; ++k) {
            const float u = s_inv[k];                          // wave-uniform address: broadcast read
            rank += (u < v || (u == v && k < j)) ? 1 : 0;
        }
        float w = ((float)rank / (float)(N - 1)) * 0.9f + 0.1f;     // (rank / (N-1)) * (1.0 - 0.1) + 0.1
        if (late && w < 0.9f) w = 0.1f;                         // iteration > 35 000 (train.py:148-149)
        weights[(size_t)i * N + j] = w;
        part = part + v * w;
    }
    s_part[tid] = part;
    __syncthreads();
    for (int st = kBlock / 2; st >= 1; st >>= 1) {              // fixed-order tree: deterministic
        if (tid < st) s_part[tid] += s_part[tid + st];
        __syncthreads();
    }
    if (tid == 0) row_loss[i] = s_part[0];
}

__global__ __launch_bounds__(kBlock) void separation_finish_kernel(const float* __restrict__ means, int N, int C,
                                                                   const float* __restrict__ weights,
                                                                   const float* __restrict__ row_loss,
                                                                   float* __restrict__ loss_out, float* __restrict__ grad) {
    // one workgroup per row i: thread j owns the pairs (i, j), (i, j + 256), ...; per-channel sums leave the workgroup
    // through a wave butterfly and four LDS slots (fixed order: deterministic)
    __shared__ float s_g[kBlock / kWave][kSepMaxC];
    const float scale = 1.0f / ((float)N * (float)(N - 1));
    const int i = blockIdx.x, tid = threadIdx.x;
    if (i == 0 && tid == 0) {
        float t = 0.f;
        for (int r = 0; r < N; ++r) t += row_loss[r];           // rows in index order
        loss_out[0] = t * scale;
    }
    if (!grad) return;
    float mi[kSepMaxC], g[kSepMaxC];
#pragma unroll
    for (int c = 0; c < kSepMaxC; ++c) { mi[c] = c < C ? means[(size_t)i * C + c] : 0.f; g[c] = 0.f; }
    for (int j = tid; j < N; j += kBlock) {
        if (j == i) continue;
        float d[kSepMaxC], d2 = 0.f;
#pragma unroll
        for (int c = 0; c < kSepMaxC; ++c) {
            d[c] = c < C ? mi[c] - means[(size_t)j * C + c] : 0.f;
            d2 += d[c] * d[c];
        }
        const float inv = 1.0f / (d2 + 1.0f);
        const float k = (weights[(size_t)i * N + j] + weights[(size_t)j * N + i]) * inv * inv;
#pragma unroll
        for (int c = 0; c < kSepMaxC; ++c) g[c] += k * d[c];
    }
#pragma unroll
    for (int c = 0; c < kSepMaxC; ++c) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) g[c] += __shfl_xor(g[c], o, kWave);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int c = 0; c < kSepMaxC; ++c) s_g[tid >> 6][c] = g[c];
    }
    __syncthreads();
    if (tid < C) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < kBlock / kWave; ++w) t += s_g[w][tid];
        grad[(size_t)i * C + tid] = -2.0f * scale * t;
    }
}

extern "C" {

int ogs_mask_feature_sums(const float* feat, const uint8_t* masks, const float* weight, int32_t C, int32_t N, int64_t HW,
                          int32_t with_squares, float* table, void* stream_) {
    return feature_sums<Stack>(feat, masks, weight, C, N, HW, with_squares, table, static_cast<hipStream_t>(stream_));
}

int ogs_mask_feature_sums_backward(const uint8_t* masks, const float* weight, const float* coef, const float* feat,
                                   const float* coef_cnt, int32_t C, int32_t N, int64_t HW, float* dfeat,
                                   float* dweight, void* stream_) {
    return feature_sums_backward<Stack>(masks, weight, coef, feat, coef_cnt, C, N, HW, dfeat, dweight,
                                        static_cast<hipStream_t>(stream_));
}

int ogs_mask_cohesion(const float* feat, const uint8_t* masks, const float* mean, int32_t C, int32_t N, int64_t HW,
                      float* table, void* stream_) {
    return cohesion<Stack>(feat, masks, mean, C, N, HW, table, static_cast<hipStream_t>(stream_));
}

int ogs_mask_feature_sqdev(const float* feat, const uint8_t* masks, const float* weight, const float* mean, int32_t C,
                           int32_t N, int64_t HW, float* table, void* stream_) {
    return feature_sqdev<Stack>(feat, masks, weight, mean, C, N, HW, table, static_cast<hipStream_t>(stream_));
}

int ogs_mask_cohesion_backward(const float* feat, const uint8_t* masks, const float* mean, const float* gl, int32_t C,
                               int32_t N, int64_t HW, float* dfeat, float* dmean, void* stream_) {
    return cohesion_backward<Stack>(feat, masks, mean, gl, C, N, HW, dfeat, dmean, static_cast<hipStream_t>(stream_));
}

// ---- label twins of the five entry points above: same checks, same tables, labels [HW] int32 in place of the stack ----
int ogs_label_feature_sums(const float* feat, const int32_t* labels, const float* weight, int32_t C, int32_t N,
                           int64_t HW, int32_t with_squares, float* table, void* stream_) {
    return feature_sums<Label>(feat, labels, weight, C, N, HW, with_squares, table, static_cast<hipStream_t>(stream_));
}

int ogs_label_feature_sums_backward(const int32_t* labels, const float* weight, const float* coef, const float* feat,
                                    const float* coef_cnt, int32_t C, int32_t N, int64_t HW, float* dfeat,
                                    float* dweight, void* stream_) {
    return feature_sums_backward<Label>(labels, weight, coef, feat, coef_cnt, C, N, HW, dfeat, dweight,
                                        static_cast<hipStream_t>(stream_));
}

int ogs_label_cohesion(const float* feat, const int32_t* labels, const float* mean, int32_t C, int32_t N, int64_t HW,
                       float* table, void* stream_) {
    return cohesion<Label>(feat, labels, mean, C, N, HW, table, static_cast<hipStream_t>(stream_));
}

int ogs_label_feature_sqdev(const float* feat, const int32_t* labels, const float* weight, const float* mean, int32_t C,
                            int32_t N, int64_t HW, float* table, void* stream_) {
    return feature_sqdev<Label>(feat, labels, weight, mean, C, N, HW, table, static_cast<hipStream_t>(stream_));
}

int ogs_label_cohesion_backward(const float* feat, const int32_t* labels, const float* mean, const float* gl, int32_t C,
                                int32_t N, int64_t HW, float* dfeat, float* dmean, void* stream_) {
    return cohesion_backward<Label>(feat, labels, mean, gl, C, N, HW, dfeat, dmean, static_cast<hipStream_t>(stream_));
}

int ogs_separation_loss(const float* means, int32_t N, int32_t C, int32_t late, float* loss, float* grad, float* tmp,
                        void* stream_) {
    if (N < 2 || N > kSepMaxN || C < 1 || C > kSepMaxC) {
        set_error("separation_loss: N=%d (2..%d), C=%d (1..%d)", N, kSepMaxN, C, kSepMaxC); return OGS_ERR_UNSUPPORTED;
    }
    if (!means || !loss || !tmp) { set_error("separation_loss: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    float* weights = tmp;                        // [N, N]
    float* row_loss = tmp + (size_t)N * N;       // [N]
    OGS_LAUNCH(separation_rows_kernel, dim3(N), dim3(kBlock), 0, s, means, N, C, late, weights, row_loss);
    OGS_LAUNCH_CHECK(0, s);
    OGS_LAUNCH(separation_finish_kernel, dim3(grad ? N : 1), dim3(kBlock), 0, s, means, N, C,
               (const float*)weights, (const float*)row_loss, loss, grad);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

}  // extern "C"
