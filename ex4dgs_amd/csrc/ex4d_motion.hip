// Per-Gaussian displacement between two timestamps, in the world or on the screen, forward and backward (ex4d_attributes.h, "Motion").
//
// One Gaussian per lane, 256 threads, like attributes_fwd_kernel; only the position tensors are read: 24 B per static row, at most
// eight keyframe rows (96 B) per dynamic row, 12 B written.  No atomics, no host read-back: the launches are graph-capturable.
//
// The arithmetic is shared with two other files BY RESTATEMENT (same expressions, same order, same -ffp-contract=off), so that the
// values carry the same bits:
//   position_at      = the position block of attributes_fwd_kernel (ex4d_attributes.hip): x(t) is the float32 value that kernel
//                      writes to means3D; position_adjoint = the position block of attributes_bwd_kernel, pchip_slope_adjoint included
//   project          = xform4x4 / xform4x3, inv_w = 1 / (h.w + 1e-7f) and the double-precision ndc2Pix of ex4d_preprocess.hip: (u, v)
//                      is the pixel position, z the view depth the rasterizer keeps in its geometry records
// Those kernels are not edited for this (their cube instantiations are documented as the parent's machine code).
#include "ex4d_internal.h"
#include <cmath>
#include <cstdio>

namespace {

// ex4d_attributes.hip: pchip_slope / pchip_slope_adjoint (utils/interpolations.py:72-73 of the reference and what autograd forms for it)
struct PchipSlope { float a, b, s, p; bool keep; };

__device__ __forceinline__ float pchip_slope(float ym, float y0, float yp, PchipSlope &m)
{
    m.a = yp - y0; m.b = y0 - ym; m.s = yp - ym;
    m.p = m.a * m.b;
    m.keep = m.p > 0.f;
    const float q = m.p / m.s * 2.0f;
    return m.keep ? q : 0.f;
}

__device__ __forceinline__ void pchip_slope_adjoint(const PchipSlope &m, float g_m, float &g_a, float &g_b, float &g_s)
{
    const float g_q = (m.keep ? g_m : 0.f) * 2.0f;
    const float g_p = g_q / m.s;
    g_s = -g_q * ((m.p / m.s) / m.s);
    g_a = g_p * m.b;
    g_b = g_p * m.a;
}

// means3D of row i at the timestamp of `a`: attributes_fwd_kernel's position block
template <int INTERP>
__device__ __forceinline__ void position_at(const Ex4dAttrParams &a, int i, const float *__restrict__ xyz, const float *__restrict__ xyz_disp,
                                            const float *__restrict__ xyz_motion, float *m)
{
    if (i < a.Ns) {
#pragma unroll
        for (int c = 0; c < 3; c++) m[c] = xyz[3 * (size_t)i + c] + (xyz_disp[3 * (size_t)i + c] * a.t) / a.duration;
    } else {
        const size_t j = (size_t)(i - a.Ns);
        if (INTERP == EX4D_INTERP_LINEAR) {
            const float *y = xyz_motion + (j * a.K + a.k) * 3;
#pragma unroll
            for (int c = 0; c < 3; c++) m[c] = y[c] * a.h00 + y[3 + c] * a.h01;
        } else {
            const float *y = xyz_motion + (j * a.K + (a.k - 1)) * 3;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float y0 = y[c], y1 = y[3 + c], y2 = y[6 + c], y3 = y[9 + c];
                float mk, mk1;
                if (INTERP == EX4D_INTERP_PCHIP) {
                    PchipSlope s0, s1;
                    mk = pchip_slope(y0, y1, y2, s0); mk1 = pchip_slope(y1, y2, y3, s1);
                } else {
                    mk = (y2 - y0) / 2.0f; mk1 = (y3 - y1) / 2.0f;
                }
                m[c] = a.h00 * y1 + a.h10 * mk + a.h01 * y2 + a.h11 * mk1;
            }
        }
    }
}

// the keyframe gradients of dynamic row j for the position gradient gm at the timestamp of `a`, as one window [4,3] (linear: [2,3]):
// attributes_bwd_kernel's position block in its sliced form
template <int INTERP>
__device__ __forceinline__ void position_adjoint(const Ex4dAttrParams &a, size_t j, const float *__restrict__ xyz_motion, const float *gm, float *gy)
{
    if (INTERP == EX4D_INTERP_LINEAR) {
#pragma unroll
        for (int c = 0; c < 3; c++) { gy[c] = gm[c] * a.h00; gy[3 + c] = gm[c] * a.h01; }
    } else if (INTERP == EX4D_INTERP_PCHIP) {
        const float *y = xyz_motion + (j * a.K + (a.k - 1)) * 3;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            PchipSlope s0, s1;
            (void)pchip_slope(y[c], y[3 + c], y[6 + c], s0);
            (void)pchip_slope(y[3 + c], y[6 + c], y[9 + c], s1);
            float ga0, gb0, gs0, ga1, gb1, gs1;
            pchip_slope_adjoint(s0, a.h10 * gm[c], ga0, gb0, gs0);
            pchip_slope_adjoint(s1, a.h11 * gm[c], ga1, gb1, gs1);
            gy[c] = -gb0 - gs0;
            gy[3 + c] = a.h00 * gm[c] + (gb0 - ga0) + (-gb1 - gs1);
            gy[6 + c] = a.h01 * gm[c] + (ga0 + gs0) + (gb1 - ga1);
            gy[9 + c] = ga1 + gs1;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            gy[c] = -(a.h10 * gm[c]) / 2.0f;
            gy[3 + c] = a.h00 * gm[c] - (a.h11 * gm[c]) / 2.0f;
            gy[6 + c] = (a.h10 * gm[c]) / 2.0f + a.h01 * gm[c];
            gy[9 + c] = (a.h11 * gm[c]) / 2.0f;
        }
    }
}

// ex4d_preprocess.hip: xform4x4 / xform4x3
__device__ __forceinline__ float3 xform4x3(float3 p, const float *m)
{
    return make_float3(m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12],
                       m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13],
                       m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14]);
}
__device__ __forceinline__ float4 xform4x4(float3 p, const float *m)
{
    return make_float4(m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12],
                       m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13],
                       m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14],
                       m[3] * p.x + m[7] * p.y + m[11] * p.z + m[15]);
}

struct Projected { float4 h; float inv_w, u, v, z; };

// frustum_test's projection and the ndc2Pix of preprocess_fwd_kernel (no culling here but the caller's depth rule)
__device__ __forceinline__ void project(const float *m, const float *__restrict__ vm, const float *__restrict__ pm, int W, int H, Projected &q)
{
    const float3 p = make_float3(m[0], m[1], m[2]);
    q.h = xform4x4(p, pm);
    q.inv_w = 1.0f / (q.h.w + 0.0000001f);
    const float ndc_x = q.h.x * q.inv_w;
    const float ndc_y = q.h.y * q.inv_w;
    const float3 p_view = xform4x3(p, vm);
    q.u = (float)((((double)ndc_x + 1.0) * (double)W - 1.0) * 0.5);
    q.v = (float)((((double)ndc_y + 1.0) * (double)H - 1.0) * 0.5);
    q.z = p_view.z;
}

// dL/dp from dL/d(u, v, z): the adjoint of project (float32; the pixel scale 0.5 W is what the double expression differentiates to)
__device__ __forceinline__ void project_adjoint(const Projected &q, const float *__restrict__ vm, const float *__restrict__ pm, int W, int H,
                                                float gu, float gv, float gz, float *gp)
{
    const float g_nx = gu * (0.5f * (float)W), g_ny = gv * (0.5f * (float)H);
    const float g_hx = g_nx * q.inv_w, g_hy = g_ny * q.inv_w;
    const float g_iw = g_nx * q.h.x + g_ny * q.h.y;
    const float g_hw = -g_iw * (q.inv_w * q.inv_w);
#pragma unroll
    for (int c = 0; c < 3; c++) gp[c] = pm[4 * c] * g_hx + pm[4 * c + 1] * g_hy + pm[4 * c + 3] * g_hw + vm[4 * c + 2] * gz;
}

template <int INTERP, bool SCREEN>
__global__ __launch_bounds__(256) void motion_fwd_kernel(Ex4dAttrParams a0, Ex4dAttrParams a1,
    const float *__restrict__ xyz, const float *__restrict__ xyz_disp, const float *__restrict__ xyz_motion,
    const float *__restrict__ vm, const float *__restrict__ pm, int W, int H, float min_depth, float *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a0.Ns + a0.Nd) return;
    float m0[3], m1[3], d[3];
    position_at<INTERP>(a0, i, xyz, xyz_disp, xyz_motion, m0);
    position_at<INTERP>(a1, i, xyz, xyz_disp, xyz_motion, m1);
    if (SCREEN) {
        Projected q0, q1;
        project(m0, vm, pm, W, H, q0);
        project(m1, vm, pm, W, H, q1);
        // a mean at or behind min_depth at either timestamp has no meaningful projection
        const bool behind = (q0.z <= min_depth) || (q1.z <= min_depth);
        d[0] = behind ? 0.f : q1.u - q0.u;
        d[1] = behind ? 0.f : q1.v - q0.v;
        d[2] = behind ? 0.f : q1.z - q0.z;
    } else {
#pragma unroll
        for (int c = 0; c < 3; c++) d[c] = m1[c] - m0[c];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) out[3 * (size_t)i + c] = d[c];
}

template <int INTERP, bool SCREEN>
__global__ __launch_bounds__(256) void motion_bwd_kernel(Ex4dAttrParams a0, Ex4dAttrParams a1,
    const float *__restrict__ xyz, const float *__restrict__ xyz_disp, const float *__restrict__ xyz_motion,
    const float *__restrict__ vm, const float *__restrict__ pm, int W, int H, float min_depth, const float *__restrict__ g_out,
    float *__restrict__ g_xyz, float *__restrict__ g_xyz_disp, float *__restrict__ g_win0, float *__restrict__ g_win1)
{
    constexpr int WIN = INTERP == EX4D_INTERP_LINEAR ? 6 : 12;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a0.Ns + a0.Nd) return;
    float g[3], gm0[3], gm1[3];
#pragma unroll
    for (int c = 0; c < 3; c++) g[c] = g_out[3 * (size_t)i + c];
    if (SCREEN) {
        float m0[3], m1[3];
        position_at<INTERP>(a0, i, xyz, xyz_disp, xyz_motion, m0);
        position_at<INTERP>(a1, i, xyz, xyz_disp, xyz_motion, m1);
        Projected q0, q1;
        project(m0, vm, pm, W, H, q0);
        project(m1, vm, pm, W, H, q1);
        if ((q0.z <= min_depth) || (q1.z <= min_depth)) {
            // the forward wrote constants: every gradient of the row is zero
            if (i < a0.Ns) {
#pragma unroll
                for (int c = 0; c < 3; c++) { g_xyz[3 * (size_t)i + c] = 0.f; g_xyz_disp[3 * (size_t)i + c] = 0.f; }
            } else {
                const size_t j = (size_t)(i - a0.Ns);
#pragma unroll
                for (int c = 0; c < WIN; c++) { g_win0[j * WIN + c] = 0.f; g_win1[j * WIN + c] = 0.f; }
            }
            return;
        }
        project_adjoint(q0, vm, pm, W, H, -g[0], -g[1], -g[2], gm0);
        project_adjoint(q1, vm, pm, W, H, g[0], g[1], g[2], gm1);
    } else {
#pragma unroll
        for (int c = 0; c < 3; c++) { gm0[c] = -g[c]; gm1[c] = g[c]; }
    }
    if (i < a0.Ns) {
        // x(t) = xyz + (disp * t) / duration, twice
#pragma unroll
        for (int c = 0; c < 3; c++) {
            g_xyz[3 * (size_t)i + c] = gm0[c] + gm1[c];
            g_xyz_disp[3 * (size_t)i + c] = (gm0[c] / a0.duration) * a0.t + (gm1[c] / a1.duration) * a1.t;
        }
    } else {
        const size_t j = (size_t)(i - a0.Ns);
        float w0[WIN], w1[WIN];
        position_adjoint<INTERP>(a0, j, xyz_motion, gm0, w0);
        position_adjoint<INTERP>(a1, j, xyz_motion, gm1, w1);
#pragma unroll
        for (int c = 0; c < WIN; c++) { g_win0[j * WIN + c] = w0[c]; g_win1[j * WIN + c] = w1[c]; }
    }
}

thread_local char g_motion_err[256] = "";

bool check_motion(const Ex4dAttrParams *a0, const Ex4dAttrParams *a1, int32_t interp, int32_t space, const float *vm, const float *pm, int32_t W, int32_t H)
{
    if (!a0 || !a1 || a0->Ns < 0 || a0->Nd < 0) { snprintf(g_motion_err, sizeof(g_motion_err), "bad parameters"); return false; }
    if (interp != EX4D_INTERP_CUBE && interp != EX4D_INTERP_LINEAR && interp != EX4D_INTERP_PCHIP) {
        snprintf(g_motion_err, sizeof(g_motion_err), "unknown interpolator %d (0 cube, 1 linear, 2 pchip)", (int)interp); return false;
    }
    if (space != EX4D_MOTION_WORLD && space != EX4D_MOTION_SCREEN) {
        snprintf(g_motion_err, sizeof(g_motion_err), "unknown space %d (0 world, 1 screen)", (int)space); return false;
    }
    if (a0->Ns != a1->Ns || a0->Nd != a1->Nd || a0->K != a1->K) {
        snprintf(g_motion_err, sizeof(g_motion_err), "the two timestamps disagree in shape: Ns %d / %d, Nd %d / %d, K %d / %d",
                 a0->Ns, a1->Ns, a0->Nd, a1->Nd, a0->K, a1->K);
        return false;
    }
    if ((int64_t)a0->Ns + a0->Nd > 0x7FFFFFFF) { snprintf(g_motion_err, sizeof(g_motion_err), "more than 2^31 - 1 rows"); return false; }
    if (a0->Nd > 0) {
        const int before = interp == EX4D_INTERP_LINEAR ? 0 : 1, after = interp == EX4D_INTERP_LINEAR ? 1 : 2;
        const Ex4dAttrParams *both[2] = { a0, a1 };
        for (int w = 0; w < 2; w++) {
            const Ex4dAttrParams *a = both[w];
            if (a->k < before || (int64_t)a->k + after >= (int64_t)a->K) {
                snprintf(g_motion_err, sizeof(g_motion_err), "keyframe index %d of t%d needs k-%d..k+%d inside [0,%d)", a->k, w, before, after, a->K);
                return false;
            }
        }
    }
    if (space == EX4D_MOTION_SCREEN && (!vm || !pm || W <= 0 || H <= 0)) {
        snprintf(g_motion_err, sizeof(g_motion_err), "screen space needs viewmatrix, projmatrix and a positive image size (W %d, H %d)", (int)W, (int)H);
        return false;
    }
    return true;
}

}  // namespace

extern "C" {

const char *ex4d_motion_last_error(void) { return g_motion_err; }

#define EX4D_MOTION_DISPATCH(LAUNCH)                                                                  \
    do {                                                                                              \
        if (space == EX4D_MOTION_SCREEN) {                                                            \
            if (interp == EX4D_INTERP_LINEAR) LAUNCH(EX4D_INTERP_LINEAR, true);                       \
            else if (interp == EX4D_INTERP_PCHIP) LAUNCH(EX4D_INTERP_PCHIP, true);                    \
            else LAUNCH(EX4D_INTERP_CUBE, true);                                                      \
        } else {                                                                                      \
            if (interp == EX4D_INTERP_LINEAR) LAUNCH(EX4D_INTERP_LINEAR, false);                      \
            else if (interp == EX4D_INTERP_PCHIP) LAUNCH(EX4D_INTERP_PCHIP, false);                   \
            else LAUNCH(EX4D_INTERP_CUBE, false);                                                     \
        }                                                                                             \
    } while (0)

int ex4d_motion_forward(const Ex4dAttrParams *a0, const Ex4dAttrParams *a1, int32_t interp, int32_t space,
    const float *xyz, const float *xyz_disp, const float *xyz_motion, const float *viewmatrix, const float *projmatrix,
    int32_t W, int32_t H, float min_depth, float *out, void *stream_)
{
    g_motion_err[0] = 0;
    hipStream_t stream = (hipStream_t)stream_;
    if (!check_motion(a0, a1, interp, space, viewmatrix, projmatrix, W, H)) return EX4D_ERR_ARG;
    const int N = a0->Ns + a0->Nd;
    if (N == 0) return EX4D_OK;
    if (!out || (a0->Ns > 0 && (!xyz || !xyz_disp)) || (a0->Nd > 0 && !xyz_motion)) {
        snprintf(g_motion_err, sizeof(g_motion_err), "a position tensor or the output is NULL"); return EX4D_ERR_ARG;
    }
#define EX4D_LAUNCH_MOTION_FWD(I, S) hipLaunchKernelGGL((motion_fwd_kernel<I, S>), dim3((N + 255) / 256), dim3(256), 0, stream, *a0, *a1, \
        xyz, xyz_disp, xyz_motion, viewmatrix, projmatrix, (int)W, (int)H, min_depth, out)
    EX4D_MOTION_DISPATCH(EX4D_LAUNCH_MOTION_FWD);
#undef EX4D_LAUNCH_MOTION_FWD
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_motion_err, sizeof(g_motion_err), "launch failed: %s", hipGetErrorString(e)); return EX4D_ERR_HIP; }
    return EX4D_OK;
}

int ex4d_motion_backward(const Ex4dAttrParams *a0, const Ex4dAttrParams *a1, int32_t interp, int32_t space,
    const float *xyz, const float *xyz_disp, const float *xyz_motion, const float *viewmatrix, const float *projmatrix,
    int32_t W, int32_t H, float min_depth, const float *g_out,
    float *g_xyz, float *g_xyz_disp, float *g_win0, float *g_win1, int32_t *windows, void *stream_)
{
    g_motion_err[0] = 0;
    hipStream_t stream = (hipStream_t)stream_;
    if (!check_motion(a0, a1, interp, space, viewmatrix, projmatrix, W, H)) return EX4D_ERR_ARG;
    if (windows) {
        const bool linear = interp == EX4D_INTERP_LINEAR;
        windows[0] = linear ? a0->k : a0->k - 1; windows[1] = linear ? 2 : 4;
        windows[2] = linear ? a1->k : a1->k - 1; windows[3] = linear ? 2 : 4;
    }
    const int N = a0->Ns + a0->Nd;
    if (N == 0) return EX4D_OK;
    if (!g_out || (a0->Ns > 0 && (!xyz || !xyz_disp || !g_xyz || !g_xyz_disp)) || (a0->Nd > 0 && (!xyz_motion || !g_win0 || !g_win1))) {
        snprintf(g_motion_err, sizeof(g_motion_err), "a position tensor, the output gradient or a gradient buffer is NULL"); return EX4D_ERR_ARG;
    }
#define EX4D_LAUNCH_MOTION_BWD(I, S) hipLaunchKernelGGL((motion_bwd_kernel<I, S>), dim3((N + 255) / 256), dim3(256), 0, stream, *a0, *a1, \
        xyz, xyz_disp, xyz_motion, viewmatrix, projmatrix, (int)W, (int)H, min_depth, g_out, g_xyz, g_xyz_disp, g_win0, g_win1)
    EX4D_MOTION_DISPATCH(EX4D_LAUNCH_MOTION_BWD);
#undef EX4D_LAUNCH_MOTION_BWD
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_motion_err, sizeof(g_motion_err), "launch failed: %s", hipGetErrorString(e)); return EX4D_ERR_HIP; }
    return EX4D_OK;
}

}  // extern "C"
