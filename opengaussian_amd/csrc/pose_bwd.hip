// Camera gradients of one pass (include/ogs_raster.h: OgsRasterBwdArgs.dL_dviewmatrix / dL_dprojmatrix / dL_dcampos) for gfx950.
//
// What is returned: the partial derivatives of the pass' loss with respect to the three camera arrays AS THE KERNELS READ THEM,
// each array independent of the other two -- 12 entries of the view matrix (p_view = V[0] x + V[4] y + V[8] z + V[12], ...; the
// rotation block again through T = J W), 12 of the projection matrix (hx, hy, hw rows; p_w = 1 / (hw + 1e-7f) as written) and the
// camera centre (view direction of the SH colours, clamp mask respected).  Entries 3, 7, 11, 15 of the view matrix and 2, 6, 10,
// 14 of the projection matrix are never read by a pass and come back as exact 0.0f, as does dL_dcampos of a colors_precomp pass.
// Cull, skip and saturation decisions are constants; where the +-1.3 tanfov clamp of tx/tz, ty/tz is active the clamped branch is
// detached, exactly as preprocess_backward_kernel treats it for dL/dmeans3D.
//
// Two launches behind preprocess_backward on the same stream, nothing read back, no atomics:
//   pose_partials_kernel  one thread per Gaussian.  Reads what preprocess_backward_kernel reads -- the fp64 gradient record, the
//                         forward record, the inputs, radii, the clamp mask -- re-derives the forward intermediates with the same
//                         fp32 expressions (this file is compiled with that file's flags) and forms the thread's 27 terms.  An
//                         untouched Gaussian (all-zero record) is dropped before its inputs are read.  The terms are widened to
//                         fp64 and summed lanes -> waves (LDS) -> one row of 32 doubles per workgroup in pose_tmp, in a fixed
//                         order; every workgroup writes its row, zeros included, so pose_tmp needs no clear.
//   pose_fold_kernel      one workgroup (1024 threads) adds the rows in fixed chunks of kPoseChunk, rounds each sum to fp32 once
//                         and writes all 35 floats on every call (P == 0: 35 zeros).
// fp32 terms summed in fp64: the result is within rounding of the fp32 terms' own error, |error| <~ 1e-6 x sum |term|, and two
// runs give the same bits.
#include "ogs_common.h"
#include "ogs_model_act.h"

namespace ogs {

namespace {

constexpr float kC1 = 0.4886025119029199f;
__device__ constexpr float kC2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                     -1.0925484305920792f, 0.5462742152960396f};
__device__ constexpr float kC3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                                     0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                                     -0.5900435899266435f};

// Row layout (doubles): [0..11] view matrix, slot 3 i + r = entry 4 i + r (r < 3: the x, y, z rows of p_view; i = 3: the
// translation); [12..23] projection matrix, slot 12 + 3 i + r = entry 4 i + (r < 2 ? r : 3) (hx, hy, hw); [24..26] campos;
// [27..31] padding, written as zeros.
constexpr int kPoseSlots = 27;
constexpr int kPoseRow = 32;
constexpr int kPoseChunk = 512;                       // rows pose_fold_kernel adds per step
constexpr int kFoldBlock = 1024;                      // threads of the one workgroup of pose_fold_kernel
constexpr int kFoldLanes = kFoldBlock / kPoseRow;     // 32 row lanes per slot
constexpr int kFoldRun = kPoseChunk / kFoldLanes;     // 16 consecutive rows per lane and step: 16 loads in flight per thread
static_assert(kPoseChunk % kFoldLanes == 0, "a chunk is cut evenly over the row lanes");

template <bool RAW>
__global__ __launch_bounds__(kBlock) void pose_partials_kernel(
    int P, int W, int H, int sh_degree, int sh_coeffs, float tanfovx, float tanfovy, float focal_x, float focal_y,
    float scale_modifier, const float* __restrict__ means3D, const float* __restrict__ shs,
    const float* __restrict__ scales, const float* __restrict__ rotations, const float* __restrict__ cov3D_precomp,
    const float* __restrict__ viewmatrix, const float* __restrict__ projmatrix, const float* __restrict__ campos,
    const int32_t* __restrict__ radii, const uint32_t* __restrict__ clamped_in, const float4* __restrict__ rec, int rec_v4,
    const double* __restrict__ grad_rec, int gstride, double* __restrict__ pose_tmp) {
    __shared__ double s_part[kBlock / kWave][kPoseRow];
    const int tid = threadIdx.x;
    const int idx = blockIdx.x * kBlock + tid;
    float c[kPoseSlots];
#pragma unroll
    for (int k = 0; k < kPoseSlots; ++k) c[k] = 0.f;

    if (idx < P && radii[idx] > 0) {
        double g64[16];
        const double2* g2 = reinterpret_cast<const double2*>(grad_rec + (size_t)idx * gstride);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const double2 t = g2[k];
            g64[2 * k] = t.x; g64[2 * k + 1] = t.y;
        }
        // a visible Gaussian behind saturated pixels received nothing: it owes nothing, and none of its inputs is read
        bool touched = false;
#pragma unroll
        for (int k = 0; k < 16; ++k) touched = touched || g64[k] != 0.0;
        if (touched) {
            float gr[kSlotMoments];
#pragma unroll
            for (int k = 0; k < kSlotMoments; ++k) gr[k] = (float)g64[k];
            const float d_depth = gr[kSlotDepth];
            // moments about the image origin -> centred on the pixel centre the blend used (preprocess_bwd.hip has the algebra)
            const float4 ge = rec[(size_t)idx * rec_v4];
            const float4 co = rec[(size_t)idx * rec_v4 + 1];
            const double cx = (double)ge.x, cy = (double)ge.y;
            const double M0 = g64[kSlotMoments], MX = g64[kSlotMoments + 1], MY = g64[kSlotMoments + 2];
            const double MXX = g64[kSlotMoments + 3], MXY = g64[kSlotMoments + 4], MYY = g64[kSlotMoments + 5];
            const float Sx = (float)(cx * M0 - MX), Sy = (float)(cy * M0 - MY);
            const float Sxx = (float)(cx * (cx * M0 - 2.0 * MX) + MXX);
            const float Sxy = (float)(cx * (cy * M0 - MY) - cy * MX + MXY);
            const float Syy = (float)(cy * (cy * M0 - 2.0 * MY) + MYY);
            const float dm2x = (-0.5f * (float)W) * (co.x * Sx + co.y * Sy);
            const float dm2y = (-0.5f * (float)H) * (co.z * Sy + co.y * Sx);
            const float dconA = -0.5f * Sxx, dconB = -0.5f * Sxy, dconC = -0.5f * Syy;

            float V[16], M[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) { V[i] = viewmatrix[i]; M[i] = projmatrix[i]; }
            const float x = means3D[3 * idx], y = means3D[3 * idx + 1], z = means3D[3 * idx + 2];
            const float m[4] = {x, y, z, 1.f};

            // ---- forward intermediates ----------------------------------------------------------------------
            float cov[6];
            if (!RAW && cov3D_precomp) {
#pragma unroll
                for (int i = 0; i < 6; ++i) cov[i] = cov3D_precomp[6 * idx + i];
            } else {
                float sx, sy, sz, qr, qx, qy, qz;
                if constexpr (RAW) {
                    sx = scale_modifier * opaque(act_scale(scales[3 * idx]));
                    sy = scale_modifier * opaque(act_scale(scales[3 * idx + 1]));
                    sz = scale_modifier * opaque(act_scale(scales[3 * idx + 2]));
                    const float4 q_raw = reinterpret_cast<const float4*>(rotations)[idx];
                    const float4 q = act_rotation(q_raw, quat_norm(q_raw));
                    qr = opaque(q.x); qx = opaque(q.y); qy = opaque(q.z); qz = opaque(q.w);
                } else {
                    sx = scale_modifier * scales[3 * idx]; sy = scale_modifier * scales[3 * idx + 1];
                    sz = scale_modifier * scales[3 * idx + 2];
                    const float4 q = reinterpret_cast<const float4*>(rotations)[idx];
                    qr = q.x; qx = q.y; qy = q.z; qz = q.w;
                }
                const float Rm[9] = {1.f - 2.f * (qy * qy + qz * qz), 2.f * (qx * qy - qr * qz), 2.f * (qx * qz + qr * qy),
                                     2.f * (qx * qy + qr * qz), 1.f - 2.f * (qx * qx + qz * qz), 2.f * (qy * qz - qr * qx),
                                     2.f * (qx * qz - qr * qy), 2.f * (qy * qz + qr * qx), 1.f - 2.f * (qx * qx + qy * qy)};
                const float Mm[9] = {Rm[0] * sx, Rm[1] * sy, Rm[2] * sz, Rm[3] * sx, Rm[4] * sy, Rm[5] * sz,
                                     Rm[6] * sx, Rm[7] * sy, Rm[8] * sz};
                cov[0] = Mm[0] * Mm[0] + Mm[1] * Mm[1] + Mm[2] * Mm[2];
                cov[1] = Mm[0] * Mm[3] + Mm[1] * Mm[4] + Mm[2] * Mm[5];
                cov[2] = Mm[0] * Mm[6] + Mm[1] * Mm[7] + Mm[2] * Mm[8];
                cov[3] = Mm[3] * Mm[3] + Mm[4] * Mm[4] + Mm[5] * Mm[5];
                cov[4] = Mm[3] * Mm[6] + Mm[4] * Mm[7] + Mm[5] * Mm[8];
                cov[5] = Mm[6] * Mm[6] + Mm[7] * Mm[7] + Mm[8] * Mm[8];
            }
            const float pvx = V[0] * x + V[4] * y + V[8] * z + V[12];
            const float pvy = V[1] * x + V[5] * y + V[9] * z + V[13];
            const float pvz = V[2] * x + V[6] * y + V[10] * z + V[14];
            const float limx = 1.3f * tanfovx, limy = 1.3f * tanfovy;
            const float txtz = pvx / pvz, tytz = pvy / pvz;
            const float tx = fminf(limx, fmaxf(-limx, txtz)) * pvz;
            const float ty = fminf(limy, fmaxf(-limy, tytz)) * pvz;
            const float x_grad_mul = (txtz < -limx || txtz > limx) ? 0.f : 1.f;
            const float y_grad_mul = (tytz < -limy || tytz > limy) ? 0.f : 1.f;
            const float tz = pvz;
            const float itz = 1.f / tz, itz2 = itz * itz, itz3 = itz2 * itz;
            const float J00 = focal_x * itz, J02 = -(focal_x * tx) * itz2;
            const float J11 = focal_y * itz, J12 = -(focal_y * ty) * itz2;
            const float T0[3] = {J00 * V[0] + J02 * V[2], J00 * V[4] + J02 * V[6], J00 * V[8] + J02 * V[10]};
            const float T1[3] = {J11 * V[1] + J12 * V[2], J11 * V[5] + J12 * V[6], J11 * V[9] + J12 * V[10]};
            const float S0[3] = {cov[0] * T0[0] + cov[1] * T0[1] + cov[2] * T0[2],
                                 cov[1] * T0[0] + cov[3] * T0[1] + cov[4] * T0[2],
                                 cov[2] * T0[0] + cov[4] * T0[1] + cov[5] * T0[2]};
            const float S1[3] = {cov[0] * T1[0] + cov[1] * T1[1] + cov[2] * T1[2],
                                 cov[1] * T1[0] + cov[3] * T1[1] + cov[4] * T1[2],
                                 cov[2] * T1[0] + cov[4] * T1[1] + cov[5] * T1[2]};
            const float a = T0[0] * S0[0] + T0[1] * S0[1] + T0[2] * S0[2] + 0.3f;
            const float b = T0[0] * S1[0] + T0[1] * S1[1] + T0[2] * S1[2];
            const float cc = T1[0] * S1[0] + T1[1] * S1[1] + T1[2] * S1[2] + 0.3f;

            // ---- conic -> cov2D (a, b, c) -> T -----------------------------------------------------------------
            const float denom = a * cc - b * b;
            const float denom2inv = 1.0f / (denom * denom + 0.0000001f);
            float da = 0.f, db = 0.f, dc = 0.f;
            if (denom2inv != 0.f) {
                da = denom2inv * (-cc * cc * dconA + 2.f * b * cc * dconB + (denom - a * cc) * dconC);
                dc = denom2inv * (-a * a * dconC + 2.f * a * b * dconB + (denom - a * cc) * dconA);
                db = denom2inv * 2.f * (b * cc * dconA - (denom + 2.f * b * b) * dconB + a * b * dconC);
            }
            float dT0[3], dT1[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                dT0[k] = 2.f * S0[k] * da + S1[k] * db;
                dT1[k] = 2.f * S1[k] * dc + S0[k] * db;
            }
            // ---- T -> J -> t = p_view (clamped branch detached) ---------------------------------------------------
            const float dJ00 = V[0] * dT0[0] + V[4] * dT0[1] + V[8] * dT0[2];
            const float dJ02 = V[2] * dT0[0] + V[6] * dT0[1] + V[10] * dT0[2];
            const float dJ11 = V[1] * dT1[0] + V[5] * dT1[1] + V[9] * dT1[2];
            const float dJ12 = V[2] * dT1[0] + V[6] * dT1[1] + V[10] * dT1[2];
            const float dtx = x_grad_mul * -focal_x * itz2 * dJ02;
            const float dty = y_grad_mul * -focal_y * itz2 * dJ12;
            const float dtz = -focal_x * itz2 * dJ00 - focal_y * itz2 * dJ11 + (2.f * focal_x * tx) * itz3 * dJ02 +
                              (2.f * focal_y * ty) * itz3 * dJ12;
            // depth reads the z row of the view matrix (ashawkey addition)
            const float dpvz = dtz + d_depth;
            // view matrix: through p_view (all four columns) and, for the rotation block, through T = J W directly
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                c[3 * i + 0] = m[i] * dtx;
                c[3 * i + 1] = m[i] * dty;
                c[3 * i + 2] = m[i] * dpvz;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                c[3 * k + 0] += J00 * dT0[k];
                c[3 * k + 1] += J11 * dT1[k];
                c[3 * k + 2] += J02 * dT0[k] + J12 * dT1[k];
            }

            // ---- mean2D (NDC) -> hx, hy, hw -> projection matrix ---------------------------------------------------
            const float hx = M[0] * x + M[4] * y + M[8] * z + M[12];
            const float hy = M[1] * x + M[5] * y + M[9] * z + M[13];
            const float hw = M[3] * x + M[7] * y + M[11] * z + M[15];
            const float m_w = 1.0f / (hw + 0.0000001f);
            const float mul1 = hx * m_w * m_w, mul2 = hy * m_w * m_w;
            const float dhx = m_w * dm2x, dhy = m_w * dm2y;
            const float dhw = -(mul1 * dm2x + mul2 * dm2y);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                c[12 + 3 * i + 0] = m[i] * dhx;
                c[12 + 3 * i + 1] = m[i] * dhy;
                c[12 + 3 * i + 2] = m[i] * dhw;
            }

            // ---- colour -> view direction -> campos ------------------------------------------------------------------
            if (shs != nullptr) {
                const uint32_t cl = clamped_in[idx];
                const float dRGB[3] = {(cl & 1u) ? 0.f : gr[0], (cl & 2u) ? 0.f : gr[1], (cl & 4u) ? 0.f : gr[2]};
                const auto sh = [&] {
                    if constexpr (RAW) return raw_sh_row(shs, cov3D_precomp, idx, sh_coeffs);
                    else return shs + (size_t)idx * sh_coeffs * 3;
                }();
                const float ox = x - campos[0], oy = y - campos[1], oz = z - campos[2];
                const float il = rsqrtf(ox * ox + oy * oy + oz * oz);
                const float dxn = ox * il, dyn = oy * il, dzn = oz * il;
                float ddir[3] = {0.f, 0.f, 0.f};   // dL/d(normalised dir)
                auto emit = [&](int k, float bx, float by, float bz) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const float s = sh[3 * k + ch] * dRGB[ch];
                        ddir[0] += bx * s; ddir[1] += by * s; ddir[2] += bz * s;
                    }
                };
                if (sh_degree > 0) {
                    emit(1, 0.f, -kC1, 0.f);
                    emit(2, 0.f, 0.f, kC1);
                    emit(3, -kC1, 0.f, 0.f);
                    if (sh_degree > 1) {
                        const float xx = dxn * dxn, yy = dyn * dyn, zz = dzn * dzn;
                        const float xy = dxn * dyn, yz = dyn * dzn, xz = dxn * dzn;
                        emit(4, kC2[0] * dyn, kC2[0] * dxn, 0.f);
                        emit(5, 0.f, kC2[1] * dzn, kC2[1] * dyn);
                        emit(6, kC2[2] * -2.f * dxn, kC2[2] * -2.f * dyn, kC2[2] * 4.f * dzn);
                        emit(7, kC2[3] * dzn, 0.f, kC2[3] * dxn);
                        emit(8, kC2[4] * 2.f * dxn, kC2[4] * -2.f * dyn, 0.f);
                        if (sh_degree > 2) {
                            emit(9, kC3[0] * 6.f * xy, kC3[0] * (3.f * xx - 3.f * yy), 0.f);
                            emit(10, kC3[1] * yz, kC3[1] * xz, kC3[1] * xy);
                            emit(11, kC3[2] * -2.f * xy, kC3[2] * (4.f * zz - xx - 3.f * yy), kC3[2] * 8.f * yz);
                            emit(12, kC3[3] * -6.f * xz, kC3[3] * -6.f * yz, kC3[3] * (6.f * zz - 3.f * xx - 3.f * yy));
                            emit(13, kC3[4] * (4.f * zz - 3.f * xx - yy), kC3[4] * -2.f * xy, kC3[4] * 8.f * xz);
                            emit(14, kC3[5] * 2.f * xz, kC3[5] * -2.f * yz, kC3[5] * (xx - yy));
                            emit(15, kC3[6] * (3.f * xx - 3.f * yy), kC3[6] * -6.f * xy, 0.f);
                        }
                    }
                }
                // dir = mean - campos: the mean's term with the sign turned.  d(dir/|dir|)/d(dir) = (I - n n^T) / |dir|
                const float nd = dxn * ddir[0] + dyn * ddir[1] + dzn * ddir[2];
                c[24] = -((ddir[0] - dxn * nd) * il);
                c[25] = -((ddir[1] - dyn * nd) * il);
                c[26] = -((ddir[2] - dzn * nd) * il);
            }
        }
    }

    // ---- fp64, fixed order: lanes (63 + ... folded onto lane 0), the four waves in index order, one row per workgroup ---------
    const int lane = tid & (kWave - 1), wave = tid / kWave;
#pragma unroll
    for (int k = 0; k < kPoseSlots; ++k) {
        double v = (double)c[k];
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
        if (lane == 0) s_part[wave][k] = v;
    }
    __syncthreads();
    if (tid < kPoseRow) {
        double t = 0.0;
        if (tid < kPoseSlots) t = ((s_part[0][tid] + s_part[1][tid]) + s_part[2][tid]) + s_part[3][tid];
        pose_tmp[(size_t)blockIdx.x * kPoseRow + tid] = t;
    }
}

// One workgroup of 1024.  Thread (lane r = tid / 32, slot e = tid % 32) owns rows base + 16 r .. base + 16 r + 15 of every chunk:
// per step it loads its 16 rows (all in flight at once: the kernel is one workgroup waiting on memory) and adds them to its
// running sum in index order, chunk after chunk; at the end the 32 lane sums of a slot are added in lane order.  A fixed order
// for a given row count.  The 35 outputs are written on every call, the never-read entries as 0.0f.
__global__ __launch_bounds__(kFoldBlock) void pose_fold_kernel(const double* __restrict__ rows, int nrows, float* __restrict__ dV,
                                                               float* __restrict__ dM, float* __restrict__ dcampos) {
    __shared__ double s_lane[kFoldLanes][kPoseRow];
    __shared__ double s_total[kPoseRow];
    const int tid = threadIdx.x;
    const int e = tid & (kPoseRow - 1), r = tid / kPoseRow;
    double acc = 0.0;
    for (int base = 0; base < nrows; base += kPoseChunk) {
        const int lo = base + r * kFoldRun;
        double v[kFoldRun];
#pragma unroll
        for (int k = 0; k < kFoldRun; ++k) v[k] = lo + k < nrows ? rows[(size_t)(lo + k) * kPoseRow + e] : 0.0;
#pragma unroll
        for (int k = 0; k < kFoldRun; ++k) acc += v[k];
    }
    s_lane[r][e] = acc;
    __syncthreads();
    if (r == 0) {
        double t = s_lane[0][e];
#pragma unroll
        for (int k = 1; k < kFoldLanes; ++k) t += s_lane[k][e];
        s_total[e] = t;
    }
    __syncthreads();
    if (tid < 16) {
        dV[tid] = (tid & 3) == 3 ? 0.f : (float)s_total[3 * (tid >> 2) + (tid & 3)];
    } else if (tid < 32) {
        const int j = tid - 16, col = j & 3;
        dM[j] = col == 2 ? 0.f : (float)s_total[12 + 3 * (j >> 2) + (col == 3 ? 2 : col)];
    } else if (tid < 35) {
        dcampos[tid - 32] = (float)s_total[24 + (tid - 32)];
    }
}

}  // namespace

size_t pose_tmp_bytes(int P) {
    const size_t rows = P > 0 ? ((size_t)P + kBlock - 1) / kBlock : 1;
    return align_up(rows * kPoseRow * sizeof(double));
}

int pose_partial_chunk() { return kPoseChunk; }

int launch_pose_backward(const OgsRasterBwdArgs& a, const GeomState& gs, const void* grad_rec, hipStream_t s, bool raw) {
    const int grid = a.P > 0 ? (a.P + kBlock - 1) / kBlock : 0;
    double* rows = static_cast<double*>(a.pose_tmp);
    if (grid > 0) {
        const float focal_x = (float)a.W / (2.0f * a.tanfovx);
        const float focal_y = (float)a.H / (2.0f * a.tanfovy);
        auto launch = [&](auto raw_tag) {
            constexpr bool kRaw = decltype(raw_tag)::value;
            OGS_LAUNCH_NAMED(kRaw ? "pose_partials_kernel<raw>" : "pose_partials_kernel", (pose_partials_kernel<kRaw>), dim3(grid),
                             dim3(kBlock), 0, s, a.P, a.W, a.H, a.sh_degree, a.sh_coeffs, a.tanfovx, a.tanfovy, focal_x, focal_y,
                             a.scale_modifier, a.means3D, a.shs, a.scales, a.rotations, a.cov3D_precomp, a.viewmatrix, a.projmatrix,
                             a.campos, a.radii, (const uint32_t*)gs.clamped, (const float4*)gs.rec, rec_vec4(a.C),
                             (const double*)grad_rec, grad_stride(a.C), rows);
        };
        if (raw) launch(std::true_type{});
        else launch(std::false_type{});
        OGS_LAUNCH_CHECK(a.debug, s);
    }
    OGS_LAUNCH(pose_fold_kernel, dim3(1), dim3(kFoldBlock), 0, s, (const double*)rows, grid, a.dL_dviewmatrix, a.dL_dprojmatrix,
               a.dL_dcampos);
    OGS_LAUNCH_CHECK(a.debug, s);
    return OGS_OK;
}

}  // namespace ogs
