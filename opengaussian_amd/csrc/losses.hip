// Full-frame image losses of stage 0 (L1 + D-SSIM) and stage 2 (masked L1 / L2): include/ogs_loss.h.
//
// Photometric pair.  One workgroup = one 32x32 tile of ONE channel.  The 11x11 window is separable: an 11-tap row pass and
// an 11-tap column pass through LDS on the tile plus its halo, zeros staged for pixels outside the image (the reference's
// zero padding; the weights are never renormalised).  img and gt are staged once and all five moments come from that staging.
//   forward : stage (32+10)^2 of img, gt -> row pass (5 moments) -> column pass -> ssim, |img - gt| -> one fp64 pair per tile
//   backward: stage (32+20)^2 of img, gt -> row + column pass give the moments, hence A, B, Cm, on the (32+10)^2 pixels the
//             tile's gradient reaches (0 at pixels outside the image) -> row + column pass of A, B, Cm -> dimg.
// Backward RECOMPUTES A, B, Cm rather than loading maps saved by forward.  Algorithmic HBM bytes, N = C*H*W floats:
//   recompute: forward 8 N read;            backward 8 N read + 4 N written           = 20 N
//   saved    : forward 8 N read + 12 N written; backward 20 N read + 4 N written      = 44 N
// (halo re-reads are L2 hits: a tile's halo is its neighbours' interior).  The extra row / column passes of the recompute
// are LDS work that a 256-thread workgroup has to spare next to 12 bytes of HBM traffic per pixel.
// Each thread produces four adjacent outputs of a pass from 14 loads (a sliding window) instead of 4 x 11; lanes step along
// the axis whose LDS pitch is odd, so neither the loads nor the stores of a pass conflict.
//
// Masked pair: one grid-stride pass over x, t (float4 where the layout allows), mask bytes and weights read beside them.
//
// No atomics anywhere: every workgroup stores one fp64 pair, a one-workgroup launch adds the pairs in index order.
#include "ogs_common.h"
#include "../../include/ogs_loss.h"

namespace ogs {
namespace {

constexpr int kR = 5;                      // window radius: 11 taps
constexpr int kTX = 32, kTY = 32;          // output tile
static_assert(kTX == kTY && kTX * kTY == 4 * kBlock, "square tile; the last column pass gives every thread four rows of one column");
constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;
constexpr int kMaskedMaxBlocks = 1024;

// exp(-(i-5)^2 / (2 * 1.5^2)) / sum, rounded to fp32 (loss_utils.py:33-35): the values torch holds
__device__ __forceinline__ constexpr float win(int k) {
    return (k == 0 || k == 10) ? 0x1.0d956cp-10f
         : (k == 1 || k == 9)  ? 0x1.f1fe02p-8f
         : (k == 2 || k == 8)  ? 0x1.26eb18p-5f
         : (k == 3 || k == 7)  ? 0x1.bff0fep-4f
         : (k == 4 || k == 6)  ? 0x1.b43c3ep-3f
                               : 0x1.10656p-2f;
}

constexpr int odd_pitch(int n) { return n | 1; }

// Row pass: out[o][r][c] = sum_k win(k) * v_o(r, c + k) for r < rows, c < cols_out, where load(r, c, v) yields the NOUT
// values to filter at source position (r, c), c < cols_in = cols_out + 10.
template <int NOUT, class Load>
__device__ __forceinline__ void row_pass(Load load, float* __restrict__ out, int rows, int cols_out, int pitch_out,
                                         int plane_out) {
    const int cols_in = cols_out + 2 * kR;
    const int groups = (cols_out + 3) >> 2;
    for (int item = threadIdx.x; item < rows * groups; item += kBlock) {
        const int r = item % rows, c0 = (item / rows) << 2;
        float acc[4][NOUT];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int o = 0; o < NOUT; ++o) acc[j][o] = 0.f;
#pragma unroll
        for (int k = 0; k < 14; ++k) {
            float v[NOUT];
            load(r, min(c0 + k, cols_in - 1), v);      // the clamp only feeds outputs past cols_out, which are dropped
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (k - j >= 0 && k - j <= 2 * kR) {
#pragma unroll
                    for (int o = 0; o < NOUT; ++o) acc[j][o] = fmaf(win(k - j), v[o], acc[j][o]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c0 + j < cols_out) {
#pragma unroll
                for (int o = 0; o < NOUT; ++o) out[o * plane_out + r * pitch_out + c0 + j] = acc[j][o];
            }
    }
}

// Column pass over in[o][r][x] (rows_out + 10 rows): store(r, x, acc) receives the NOUT filtered values at (r, x).
template <int NOUT, class Store>
__device__ __forceinline__ void col_pass(const float* __restrict__ in, int pitch_in, int plane_in, int rows_out, int cols,
                                         Store store) {
    const int rows_in = rows_out + 2 * kR;
    const int groups = (rows_out + 3) >> 2;
    for (int item = threadIdx.x; item < cols * groups; item += kBlock) {
        const int x = item % cols, r0 = (item / cols) << 2;
        float acc[4][NOUT];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int o = 0; o < NOUT; ++o) acc[j][o] = 0.f;
#pragma unroll
        for (int k = 0; k < 14; ++k) {
            const int r = min(r0 + k, rows_in - 1);
            float v[NOUT];
#pragma unroll
            for (int o = 0; o < NOUT; ++o) v[o] = in[o * plane_in + r * pitch_in + x];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (k - j >= 0 && k - j <= 2 * kR) {
#pragma unroll
                    for (int o = 0; o < NOUT; ++o) acc[j][o] = fmaf(win(k - j), v[o], acc[j][o]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (r0 + j < rows_out) store(r0 + j, x, j, acc[j]);
    }
}

// img, gt of one channel, rows [y0, y0 + n) x cols [x0, x0 + n), into s[0], s[1] (pitch `pitch`); zeros outside the image
__device__ __forceinline__ void stage(const float* __restrict__ img, const float* __restrict__ gt, int H, int W, int y0,
                                      int x0, int rows, int cols, float* __restrict__ s, int pitch, int plane) {
    for (int i = threadIdx.x; i < rows * cols; i += kBlock) {
        const int r = i / cols, c = i - r * cols;
        const int y = y0 + r, x = x0 + c;
        float a = 0.f, b = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const size_t p = (size_t)y * W + x;
            a = img[p];
            b = gt[p];
        }
        s[r * pitch + c] = a;
        s[plane + r * pitch + c] = b;
    }
}

struct Ssim {
    float s, A, B, Cm;
};
// m = { G*x, G*y, G*x^2, G*y^2, G*xy } at one pixel (loss_utils.py:54-68)
template <bool GRAD>
__device__ __forceinline__ Ssim ssim_of(const float (&m)[5]) {
    const float mu1 = m[0], mu2 = m[1];
    const float s11 = m[2] - mu1 * mu1, s22 = m[3] - mu2 * mu2, s12 = m[4] - mu1 * mu2;
    const float a1 = 2.f * mu1 * mu2 + kC1, a2 = 2.f * s12 + kC2;
    const float b1 = mu1 * mu1 + mu2 * mu2 + kC1, b2 = s11 + s22 + kC2;
    Ssim r;
    r.s = (a1 * a2) / (b1 * b2);
    r.A = r.B = r.Cm = 0.f;
    if (GRAD) {
        const float inv = 1.f / (b1 * b2);
        r.B = -r.s / b2;                        // d s / d sigma_x^2
        r.Cm = 2.f * a1 * inv;                  // d s / d sigma_xy
        // d s / d mu_x, with sigma_x^2 = G*x^2 - mu_x^2 and sigma_xy = G*xy - mu_x mu_y folded in
        r.A = 2.f * mu2 * a2 * inv - 2.f * mu1 * r.s / b1 - 2.f * mu1 * r.B - mu2 * r.Cm;
    }
    return r;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}
// sum of (a, b) over the workgroup in a fixed order; valid in thread 0
__device__ __forceinline__ void block_sum2(double& a, double& b, double* red /* [2 * kBlock / kWave] */) {
    a = wave_sum(a);
    b = wave_sum(b);
    const int w = threadIdx.x / kWave;
    if (lane_id() == 0) { red[2 * w] = a; red[2 * w + 1] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = red[0]; b = red[1];
        for (int k = 1; k < kBlock / kWave; ++k) { a += red[2 * k]; b += red[2 * k + 1]; }
    }
}

// ---- photometric forward ---------------------------------------------------------------------------------------------
constexpr int kFwdIn = kTX + 2 * kR;                       // 42: staged rows / cols
constexpr int kFwdInPitch = odd_pitch(kFwdIn);             // 43
constexpr int kFwdHPitch = odd_pitch(kTX);                 // 33
constexpr int kFwdInPlane = kFwdIn * kFwdInPitch, kFwdHPlane = kFwdIn * kFwdHPitch;

__global__ void __launch_bounds__(kBlock) loss_photometric_forward_kernel(const float* __restrict__ img,
                                                                          const float* __restrict__ gt, int H, int W,
                                                                          double2* __restrict__ partials) {
    __shared__ float s_in[2 * kFwdInPlane];        // 14.1 KB
    __shared__ float s_h[5 * kFwdHPlane];          // 27.1 KB
    __shared__ double s_red[2 * kBlock / kWave];
    const int x0 = blockIdx.x * kTX, y0 = blockIdx.y * kTY;
    const size_t chan = (size_t)blockIdx.z * H * W;
    stage(img + chan, gt + chan, H, W, y0 - kR, x0 - kR, kFwdIn, kFwdIn, s_in, kFwdInPitch, kFwdInPlane);
    __syncthreads();
    row_pass<5>([&](int r, int c, float (&v)[5]) {
        const float a = s_in[r * kFwdInPitch + c], b = s_in[kFwdInPlane + r * kFwdInPitch + c];
        v[0] = a; v[1] = b; v[2] = a * a; v[3] = b * b; v[4] = a * b;
    }, s_h, kFwdIn, kTX, kFwdHPitch, kFwdHPlane);
    __syncthreads();
    double sum_l1 = 0.0, sum_ssim = 0.0;
    col_pass<5>(s_h, kFwdHPitch, kFwdHPlane, kTY, kTX, [&](int r, int x, int, const float (&m)[5]) {
        if (y0 + r < H && x0 + x < W) {
            const int q = (r + kR) * kFwdInPitch + x + kR;
            sum_l1 += (double)fabsf(s_in[q] - s_in[kFwdInPlane + q]);
            sum_ssim += (double)ssim_of<false>(m).s;
        }
    });
    block_sum2(sum_l1, sum_ssim, s_red);
    if (threadIdx.x == 0)
        partials[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = make_double2(sum_l1, sum_ssim);
}

// the pairs in index order, fp64; one workgroup
__device__ __forceinline__ void sum_pairs(const double2* __restrict__ partials, int n, double& a, double& b, double* red) {
    a = 0.0; b = 0.0;
    for (int i = threadIdx.x; i < n; i += kBlock) { const double2 p = partials[i]; a += p.x; b += p.y; }
    block_sum2(a, b, red);
}

__global__ void __launch_bounds__(kBlock) loss_photometric_reduce_kernel(const double2* __restrict__ partials, int n,
                                                                         double count, float lambda_dssim,
                                                                         float* __restrict__ out) {
    __shared__ double s_red[2 * kBlock / kWave];
    double a, b;
    sum_pairs(partials, n, a, b, s_red);
    if (threadIdx.x == 0) {
        const double l1 = a / count, ss = b / count;
        out[0] = (float)a; out[1] = (float)b; out[2] = (float)l1; out[3] = (float)ss;
        out[4] = (float)((1.0 - (double)lambda_dssim) * l1 + (double)lambda_dssim * (1.0 - ss));
    }
}

// ---- photometric backward --------------------------------------------------------------------------------------------
constexpr int kBwdIn = kTX + 4 * kR;                       // 52: staged rows / cols of img, gt
constexpr int kBwdMid = kTX + 2 * kR;                      // 42: rows / cols of A, B, Cm
constexpr int kBwdInPitch = odd_pitch(kBwdIn);             // 53
constexpr int kBwdMidPitch = odd_pitch(kBwdMid);           // 43
constexpr int kBwdOutPitch = odd_pitch(kTX);               // 33
constexpr int kBwdInPlane = kBwdIn * kBwdInPitch;          // img | gt
constexpr int kBwdHPlane = kBwdIn * kBwdMidPitch;          // row-filtered moments: 52 rows x 42 cols
constexpr int kBwdAbcPlane = kBwdMid * kBwdMidPitch;       // A | B | Cm, laid over the staged images
constexpr int kBwdH2Plane = kBwdMid * kBwdOutPitch;        // row-filtered A, B, Cm, laid over the moments
static_assert(3 * kBwdAbcPlane <= 2 * kBwdInPlane && 3 * kBwdH2Plane <= 5 * kBwdHPlane, "LDS overlays");

__global__ void __launch_bounds__(kBlock) loss_photometric_backward_kernel(
    const float* __restrict__ img, const float* __restrict__ gt, const float* __restrict__ g_l1,
    const float* __restrict__ g_ssim, const float* __restrict__ g_loss, float lambda_dssim, int H, int W, float inv_count,
    float* __restrict__ dimg) {
    __shared__ float s_a[2 * kBwdInPlane];         // 21.5 KB: img | gt, then A | B | Cm
    __shared__ float s_b[5 * kBwdHPlane];          // 43.7 KB: row-filtered moments, then row-filtered A | B | Cm
    const int x0 = blockIdx.x * kTX, y0 = blockIdx.y * kTY;
    const size_t chan = (size_t)blockIdx.z * H * W;
    const float gt_loss = g_loss ? g_loss[0] : 0.f;
    const float gl = ((g_l1 ? g_l1[0] : 0.f) + (1.f - lambda_dssim) * gt_loss) * inv_count;
    const float gs = ((g_ssim ? g_ssim[0] : 0.f) - lambda_dssim * gt_loss) * inv_count;

    stage(img + chan, gt + chan, H, W, y0 - 2 * kR, x0 - 2 * kR, kBwdIn, kBwdIn, s_a, kBwdInPitch, kBwdInPlane);
    __syncthreads();
    // this thread's four output pixels (column px, rows py .. py + 3): their img, gt leave LDS before A, B, Cm overwrite them
    const int px = threadIdx.x % kTX, py = (threadIdx.x / kTX) << 2;
    float own_img[4], own_gt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = (py + j + 2 * kR) * kBwdInPitch + px + 2 * kR;
        own_img[j] = s_a[q];
        own_gt[j] = s_a[kBwdInPlane + q];
    }
    row_pass<5>([&](int r, int c, float (&v)[5]) {
        const float a = s_a[r * kBwdInPitch + c], b = s_a[kBwdInPlane + r * kBwdInPitch + c];
        v[0] = a; v[1] = b; v[2] = a * a; v[3] = b * b; v[4] = a * b;
    }, s_b, kBwdIn, kBwdMid, kBwdMidPitch, kBwdHPlane);
    __syncthreads();
    // A, B, Cm on the 42 x 42 pixels around the tile; a pixel outside the image has no ssim term: 0
    col_pass<5>(s_b, kBwdMidPitch, kBwdHPlane, kBwdMid, kBwdMid, [&](int r, int x, int, const float (&m)[5]) {
        const int y = y0 - kR + r, xx = x0 - kR + x;
        Ssim d = ssim_of<true>(m);
        if (y < 0 || y >= H || xx < 0 || xx >= W) d.A = d.B = d.Cm = 0.f;
        const int q = r * kBwdMidPitch + x;
        s_a[q] = d.A;
        s_a[kBwdAbcPlane + q] = d.B;
        s_a[2 * kBwdAbcPlane + q] = d.Cm;
    });
    __syncthreads();
    row_pass<3>([&](int r, int c, float (&v)[3]) {
        const int q = r * kBwdMidPitch + c;
        v[0] = s_a[q]; v[1] = s_a[kBwdAbcPlane + q]; v[2] = s_a[2 * kBwdAbcPlane + q];
    }, s_b, kBwdMid, kTX, kBwdOutPitch, kBwdH2Plane);
    __syncthreads();
    // 32 x 8 items = one per thread: item t is column t % 32, rows 4 (t / 32) .. + 3, the pixels loaded above
    col_pass<3>(s_b, kBwdOutPitch, kBwdH2Plane, kTY, kTX, [&](int r, int x, int j, const float (&f)[3]) {
        const int y = y0 + r, xx = x0 + x;
        if (y < H && xx < W) {
            const float a = own_img[j], b = own_gt[j];
            const float d = a - b;
            const float sgn = d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f;
            dimg[chan + (size_t)y * W + xx] = gs * (f[0] + 2.f * a * f[1] + b * f[2]) + gl * sgn;
        }
    });
}

// ---- masked L1 / L2 --------------------------------------------------------------------------------------------------
struct MaskedArgs {
    const float* x;
    const float* t;
    const uint8_t* mask;        // may be NULL
    const float* weight;        // may be NULL
    int64_t n, HW;              // n = C * HW
    int per_channel;            // mask (and weight) hold n elements, not HW
    int p;
};

__device__ __forceinline__ float masked_term(float d, bool m, float w, int p) {
    return !m ? 0.f : p == 1 ? fabsf(d * w) : d * d * w;
}
__device__ __forceinline__ float masked_grad(float d, bool m, float w, int p, float scale) {
    if (!m) return 0.f;
    return p == 1 ? (d > 0.f ? fabsf(w) : d < 0.f ? -fabsf(w) : 0.f) * scale : 2.f * d * w * scale;
}

template <bool VEC>
__global__ void __launch_bounds__(kBlock) loss_masked_forward_kernel(MaskedArgs a, double2* __restrict__ partials) {
    __shared__ double s_red[2 * kBlock / kWave];
    double num = 0.0, den = 0.0;
    constexpr int V = VEC ? 4 : 1;
    const int64_t steps = (a.n + V - 1) / V;
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < steps; s += (int64_t)gridDim.x * kBlock) {
        const int64_t i = s * V;
        const int64_t mi = a.per_channel ? i : i % a.HW;      // VEC: HW % 4 == 0, the four elements share a channel
        const bool own = a.per_channel || i < a.HW;            // the mask's own elements are counted once
        float xv[V], tv[V], wv[V];
        bool mv[V];
        if constexpr (VEC) {
            const float4 x4 = *reinterpret_cast<const float4*>(a.x + i), t4 = *reinterpret_cast<const float4*>(a.t + i);
            xv[0] = x4.x; xv[1] = x4.y; xv[2] = x4.z; xv[3] = x4.w;
            tv[0] = t4.x; tv[1] = t4.y; tv[2] = t4.z; tv[3] = t4.w;
            uchar4 m4 = make_uchar4(1, 1, 1, 1);
            if (a.mask) m4 = *reinterpret_cast<const uchar4*>(a.mask + mi);
            mv[0] = m4.x != 0; mv[1] = m4.y != 0; mv[2] = m4.z != 0; mv[3] = m4.w != 0;
            float4 w4 = make_float4(1.f, 1.f, 1.f, 1.f);
            if (a.weight) w4 = *reinterpret_cast<const float4*>(a.weight + mi);
            wv[0] = w4.x; wv[1] = w4.y; wv[2] = w4.z; wv[3] = w4.w;
        } else {
            xv[0] = a.x[i]; tv[0] = a.t[i];
            mv[0] = a.mask ? a.mask[mi] != 0 : true;
            wv[0] = a.weight ? a.weight[mi] : 1.f;
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            num += (double)masked_term(xv[k] - tv[k], mv[k], wv[k], a.p);
            if (own && mv[k]) den += 1.0;
        }
    }
    block_sum2(num, den, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = make_double2(num, den);
}

__global__ void __launch_bounds__(kBlock) loss_masked_reduce_kernel(const double2* __restrict__ partials, int n,
                                                                    double plain_count, float* __restrict__ out) {
    __shared__ double s_red[2 * kBlock / kWave];
    double num, den;
    sum_pairs(partials, n, num, den, s_red);
    if (threadIdx.x == 0) {
        if (plain_count > 0.0) den = plain_count;          // mask == NULL: the mean over C * HW
        out[0] = (float)num; out[1] = (float)den;
        out[2] = (float)(num / (den < 1.0 ? 1.0 : den));
    }
}

template <bool VEC>
__global__ void __launch_bounds__(kBlock) loss_masked_backward_kernel(MaskedArgs a, const float* __restrict__ fwd_out,
                                                                      const float* __restrict__ g, float* __restrict__ dx) {
    const float scale = g[0] / fmaxf(fwd_out[1], 1.f);
    constexpr int V = VEC ? 4 : 1;
    const int64_t steps = (a.n + V - 1) / V;
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < steps; s += (int64_t)gridDim.x * kBlock) {
        const int64_t i = s * V;
        const int64_t mi = a.per_channel ? i : i % a.HW;
        if constexpr (VEC) {
            const float4 x4 = *reinterpret_cast<const float4*>(a.x + i), t4 = *reinterpret_cast<const float4*>(a.t + i);
            uchar4 m4 = make_uchar4(1, 1, 1, 1);
            if (a.mask) m4 = *reinterpret_cast<const uchar4*>(a.mask + mi);
            float4 w4 = make_float4(1.f, 1.f, 1.f, 1.f);
            if (a.weight) w4 = *reinterpret_cast<const float4*>(a.weight + mi);
            float4 o;
            o.x = masked_grad(x4.x - t4.x, m4.x != 0, w4.x, a.p, scale);
            o.y = masked_grad(x4.y - t4.y, m4.y != 0, w4.y, a.p, scale);
            o.z = masked_grad(x4.z - t4.z, m4.z != 0, w4.z, a.p, scale);
            o.w = masked_grad(x4.w - t4.w, m4.w != 0, w4.w, a.p, scale);
            *reinterpret_cast<float4*>(dx + i) = o;
        } else {
            const bool m = a.mask ? a.mask[mi] != 0 : true;
            const float w = a.weight ? a.weight[mi] : 1.f;
            dx[i] = masked_grad(a.x[i] - a.t[i], m, w, a.p, scale);
        }
    }
}

inline bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int masked_check(const float* x, const float* t, const uint8_t* mask, const float* weight, int32_t mask_channels, int32_t p,
                 int32_t C, int64_t HW) {
    if (p != 1 && p != 2) { set_error("masked loss: p=%d unsupported (1 or 2)", p); return OGS_ERR_UNSUPPORTED; }
    if (C < 1 || (mask && C != 3 && C != 6)) { set_error("masked loss: C=%d unsupported (3 or 6 with a mask)", C); return OGS_ERR_UNSUPPORTED; }
    if (HW < 0 || HW >= ((int64_t)1 << 40)) { set_error("masked loss: bad size HW=%lld", (long long)HW); return OGS_ERR_INVALID_ARG; }
    if (mask && mask_channels != 1 && mask_channels != C) { set_error("masked loss: mask_channels=%d must be 1 or C=%d", mask_channels, C); return OGS_ERR_INVALID_ARG; }
    if (weight && !mask) { set_error("masked loss: a weight needs a mask"); return OGS_ERR_INVALID_ARG; }
    if (HW > 0 && (!x || !t)) { set_error("masked loss: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    return OGS_OK;
}

MaskedArgs masked_args(const float* x, const float* t, const uint8_t* mask, const float* weight, int32_t mask_channels,
                       int32_t p, int32_t C, int64_t HW) {
    MaskedArgs a;
    a.x = x; a.t = t; a.mask = mask; a.weight = weight;
    a.n = (int64_t)C * HW; a.HW = HW;
    a.per_channel = (!mask || mask_channels == C) ? 1 : 0;     // without a mask the index is never used
    a.p = p;
    return a;
}
bool masked_vec_ok(const MaskedArgs& a, const void* dx) {
    return a.HW % 4 == 0 && aligned(a.x, 16) && aligned(a.t, 16) && aligned(a.mask, 4) && aligned(a.weight, 16) &&
           aligned(dx, 16);
}
int masked_blocks(const MaskedArgs& a, bool vec) {
    const int64_t steps = (a.n + (vec ? 4 : 1) - 1) / (vec ? 4 : 1);
    const int64_t b = (steps + kBlock - 1) / kBlock;
    return (int)(b < 1 ? 1 : b > kMaskedMaxBlocks ? kMaskedMaxBlocks : b);
}

int photometric_check(const void* a, const void* b, const void* c, int32_t C, int32_t H, int32_t W) {
    if (C != 3) { set_error("photometric loss: C=%d unsupported (3)", C); return OGS_ERR_UNSUPPORTED; }
    if (H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31)) { set_error("photometric loss: bad size H=%d W=%d", H, W); return OGS_ERR_INVALID_ARG; }
    if ((H + kTY - 1) / kTY > 65535) { set_error("photometric loss: H=%d too tall", H); return OGS_ERR_UNSUPPORTED; }
    if (!a || !b || !c) { set_error("photometric loss: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    return OGS_OK;
}
dim3 photometric_grid(int32_t C, int32_t H, int32_t W) { return dim3((W + kTX - 1) / kTX, (H + kTY - 1) / kTY, C); }

}  // namespace
}  // namespace ogs

using namespace ogs;

extern "C" {

size_t ogs_loss_photometric_tmp_bytes(int32_t C, int32_t H, int32_t W) {
    if (C < 1 || H < 1 || W < 1) return sizeof(double2);
    const dim3 g = photometric_grid(C, H, W);
    return (size_t)g.x * g.y * g.z * sizeof(double2);
}

int ogs_loss_photometric_forward(const float* img, const float* gt, int32_t C, int32_t H, int32_t W, float lambda_dssim,
                                 float* out, void* partials, void* stream_) {
    int rc = photometric_check(img, gt, out, C, H, W);
    if (rc != OGS_OK) return rc;
    if (!partials) { set_error("photometric loss: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const dim3 g = photometric_grid(C, H, W);
    OGS_LAUNCH(loss_photometric_forward_kernel, g, dim3(kBlock), 0, s, img, gt, H, W, static_cast<double2*>(partials));
    OGS_LAUNCH_CHECK(0, s);
    OGS_LAUNCH(loss_photometric_reduce_kernel, dim3(1), dim3(kBlock), 0, s, static_cast<const double2*>(partials),
               (int)(g.x * g.y * g.z), (double)C * H * W, lambda_dssim, out);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

int ogs_loss_photometric_backward(const float* img, const float* gt, const float* g_l1, const float* g_ssim,
                                  const float* g_loss, float lambda_dssim, int32_t C, int32_t H, int32_t W, float* dimg,
                                  void* stream_) {
    int rc = photometric_check(img, gt, dimg, C, H, W);
    if (rc != OGS_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream_);
    OGS_LAUNCH(loss_photometric_backward_kernel, photometric_grid(C, H, W), dim3(kBlock), 0, s, img, gt, g_l1, g_ssim, g_loss,
               lambda_dssim, H, W, (float)(1.0 / ((double)C * H * W)), dimg);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

size_t ogs_loss_masked_tmp_bytes(void) { return (size_t)kMaskedMaxBlocks * sizeof(double2); }

int ogs_loss_masked_forward(const float* x, const float* t, const uint8_t* mask, const float* weight, int32_t mask_channels,
                            int32_t p, int32_t C, int64_t HW, float* out, void* partials, void* stream_) {
    int rc = masked_check(x, t, mask, weight, mask_channels, p, C, HW);
    if (rc != OGS_OK) return rc;
    if (!out || !partials) { set_error("masked loss: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const MaskedArgs a = masked_args(x, t, mask, weight, mask_channels, p, C, HW);
    const bool vec = masked_vec_ok(a, nullptr);
    const int blocks = masked_blocks(a, vec);
    if (vec) OGS_LAUNCH(loss_masked_forward_kernel<true>, dim3(blocks), dim3(kBlock), 0, s, a, static_cast<double2*>(partials));
    else OGS_LAUNCH(loss_masked_forward_kernel<false>, dim3(blocks), dim3(kBlock), 0, s, a, static_cast<double2*>(partials));
    OGS_LAUNCH_CHECK(0, s);
    OGS_LAUNCH(loss_masked_reduce_kernel, dim3(1), dim3(kBlock), 0, s, static_cast<const double2*>(partials), blocks,
               mask ? 0.0 : (double)a.n, out);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

int ogs_loss_masked_backward(const float* x, const float* t, const uint8_t* mask, const float* weight,
                             int32_t mask_channels, int32_t p, int32_t C, int64_t HW, const float* fwd_out, const float* g,
                             float* dx, void* stream_) {
    int rc = masked_check(x, t, mask, weight, mask_channels, p, C, HW);
    if (rc != OGS_OK) return rc;
    if (HW == 0) return OGS_OK;
    if (!fwd_out || !g || !dx) { set_error("masked loss: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const MaskedArgs a = masked_args(x, t, mask, weight, mask_channels, p, C, HW);
    const bool vec = masked_vec_ok(a, dx);
    const int blocks = masked_blocks(a, vec);
    if (vec) OGS_LAUNCH(loss_masked_backward_kernel<true>, dim3(blocks), dim3(kBlock), 0, s, a, fwd_out, g, dx);
    else OGS_LAUNCH(loss_masked_backward_kernel<false>, dim3(blocks), dim3(kBlock), 0, s, a, fwd_out, g, dx);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

}  // extern "C"
