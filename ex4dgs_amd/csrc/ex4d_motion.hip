// Per-Gaussian displacement between two timestamps, in the world or on the screen, forward and backward (ex4d_attributes.h, "Motion").
//
// One Gaussian per lane, 256 threads, like attributes_fwd_kernel; only the position tensors are read: 24 B per static row, at most
// eight keyframe rows (96 B) per dynamic row, 12 B written.  No atomics, no host read-back: the launches are graph-capturable.
//
// The arithmetic is that of two other files, and its definitions are shared with them, so that the values carry the same bits:
//   ex4d_keyframes.h  static_position / keyframe_position: x(t) is the float32 value attributes_fwd_kernel writes to means3D;
//                     keyframe_position_adjoint: the keyframe gradients attributes_bwd_kernel writes in its sliced form
//   ex4d_camera.h     project_point / ndc_to_pix: (u, v) is the pixel position, z the view depth the rasterizer's per-Gaussian forward
//                     (ex4d_preprocess.hip) keeps in its geometry records
#include "ex4d_internal.h"
#include "ex4d_camera.h"
#include "ex4d_keyframes.h"
#include <cmath>
#include <cstdio>

namespace {

// means3D of row i at the timestamp of `a`
template <int INTERP>
__device__ __forceinline__ void position_at(const Ex4dAttrParams &a, int i, const float *__restrict__ xyz, const float *__restrict__ xyz_disp,
                                            const float *__restrict__ xyz_motion, float *m)
{
    if (i < a.Ns) static_position(a, i, xyz, xyz_disp, m);
    else keyframe_position<INTERP>(a, (size_t)(i - a.Ns), xyz_motion, m);
}

struct Projected { float4 h; float inv_w, u, v, z; };

// the pixel position and view depth of a mean (no culling here but the caller's depth rule)
__device__ __forceinline__ void project(const float *m, const float *__restrict__ vm, const float *__restrict__ pm, int W, int H, Projected &q)
{
    ProjectedPoint pp;
    project_point(make_float3(m[0], m[1], m[2]), vm, pm, pp);
    q.h = pp.h; q.inv_w = pp.inv_w;
    q.u = ndc_to_pix(pp.ndc_x, W);
    q.v = ndc_to_pix(pp.ndc_y, H);
    q.z = pp.p_view.z;
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
    constexpr int WIN = ex4d_key_window(INTERP, 0).count * 3;
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
        keyframe_position_adjoint<INTERP>(a0, j, xyz_motion, gm0, w0);
        keyframe_position_adjoint<INTERP>(a1, j, xyz_motion, gm1, w1);
#pragma unroll
        for (int c = 0; c < WIN; c++) { g_win0[j * WIN + c] = w0[c]; g_win1[j * WIN + c] = w1[c]; }
    }
}

thread_local char g_motion_err[256] = "";

bool check_motion(const Ex4dAttrParams *a0, const Ex4dAttrParams *a1, int32_t interp, int32_t space, const float *vm, const float *pm, int32_t W, int32_t H)
{
    if (!a0 || !a1 || a0->Ns < 0 || a0->Nd < 0) { snprintf(g_motion_err, sizeof(g_motion_err), "bad parameters"); return false; }
    if (!ex4d_known_interp(interp)) { snprintf(g_motion_err, sizeof(g_motion_err), EX4D_UNKNOWN_INTERP_FMT, (int)interp); return false; }
    if (space != EX4D_MOTION_WORLD && space != EX4D_MOTION_SCREEN) {
        snprintf(g_motion_err, sizeof(g_motion_err), "unknown space %d (0 world, 1 screen)", (int)space); return false;
    }
    if (a0->Ns != a1->Ns || a0->Nd != a1->Nd || a0->K != a1->K) {
        snprintf(g_motion_err, sizeof(g_motion_err), "the two timestamps disagree in shape: Ns %d / %d, Nd %d / %d, K %d / %d",
                 a0->Ns, a1->Ns, a0->Nd, a1->Nd, a0->K, a1->K);
        return false;
    }
    if ((int64_t)a0->Ns + a0->Nd > 0x7FFFFFFF) { snprintf(g_motion_err, sizeof(g_motion_err), "more than 2^31 - 1 rows"); return false; }
    if (!ex4d_check_key_window(a0, interp, 0, g_motion_err, sizeof(g_motion_err)) ||
        !ex4d_check_key_window(a1, interp, 1, g_motion_err, sizeof(g_motion_err))) return false;
    if (space == EX4D_MOTION_SCREEN && (!vm || !pm || W <= 0 || H <= 0)) {
        snprintf(g_motion_err, sizeof(g_motion_err), "screen space needs viewmatrix, projmatrix and a positive image size (W %d, H %d)", (int)W, (int)H);
        return false;
    }
    return true;
}

}  // namespace

extern "C" {

const char *ex4d_motion_last_error(void) { return g_motion_err; }

// LAUNCH(I) names its kernel's second template argument SCREEN
#define EX4D_MOTION_DISPATCH(LAUNCH)                                                                                  \
    do {                                                                                                              \
        if (space == EX4D_MOTION_SCREEN) { constexpr bool SCREEN = true; EX4D_DISPATCH_INTERP(interp, LAUNCH); }      \
        else { constexpr bool SCREEN = false; EX4D_DISPATCH_INTERP(interp, LAUNCH); }                                 \
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
#define EX4D_LAUNCH_MOTION_FWD(I) hipLaunchKernelGGL((motion_fwd_kernel<I, SCREEN>), dim3((N + 255) / 256), dim3(256), 0, stream, *a0, *a1, \
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
        const Ex4dKeyWindow w0 = ex4d_key_window(interp, a0->k), w1 = ex4d_key_window(interp, a1->k);
        windows[0] = w0.first; windows[1] = w0.count; windows[2] = w1.first; windows[3] = w1.count;
    }
    const int N = a0->Ns + a0->Nd;
    if (N == 0) return EX4D_OK;
    if (!g_out || (a0->Ns > 0 && (!xyz || !xyz_disp || !g_xyz || !g_xyz_disp)) || (a0->Nd > 0 && (!xyz_motion || !g_win0 || !g_win1))) {
        snprintf(g_motion_err, sizeof(g_motion_err), "a position tensor, the output gradient or a gradient buffer is NULL"); return EX4D_ERR_ARG;
    }
#define EX4D_LAUNCH_MOTION_BWD(I) hipLaunchKernelGGL((motion_bwd_kernel<I, SCREEN>), dim3((N + 255) / 256), dim3(256), 0, stream, *a0, *a1, \
        xyz, xyz_disp, xyz_motion, viewmatrix, projmatrix, (int)W, (int)H, min_depth, g_out, g_xyz, g_xyz_disp, g_win0, g_win1)
    EX4D_MOTION_DISPATCH(EX4D_LAUNCH_MOTION_BWD);
#undef EX4D_LAUNCH_MOTION_BWD
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_motion_err, sizeof(g_motion_err), "launch failed: %s", hipGetErrorString(e)); return EX4D_ERR_HIP; }
    return EX4D_OK;
}

}  // extern "C"
