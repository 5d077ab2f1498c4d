// Fused optical-flow loss on 16-bit encoded ground truth, forward and backward, for gfx950 (include/ex4d_loss.h, "FLOW").
//
// The reference carries a frame's flow as a 16-bit three-channel image (utils/general_utils.py:39-53, read_opticalflow / decode_flow;
// scene/cameras.py:85,102 opticalflow_path): u and v offset by 2^15 and scaled by 2^8, the third word above 2^15 where the pixel is
// valid.  The kernels decode on load -- 6 (or 8) bytes per pixel instead of a float [H,W,2] image and a mask -- and compare with the
// rasterizer's `opticalflow` output, float32 [3,H,W] whose third plane is never read:
//     g = (float)(code - 32768) / 256 * flow_scale          (one rounding: the first two operations are exact)
//     m = code2 > 32768
//     r = (flow_u - g_u, flow_v - g_v);   rho = |r_u| + |r_v|   or   sqrt(r_u^2 + r_v^2 + eps^2)
//     loss = sum m w rho / max(sum m, 1),   w = acc[p] (a constant) or 1
// This file is compiled with -ffp-contract=off: the decode gives the bits of the reference's float32 numpy arithmetic, and the same
// residual in the forward and the backward.
//
// A STREAMING PASS over flat pixels p = y W + x (the planes and the codes are contiguous, so rows do not matter): a lane owns
// EX4D_FLOW_PIXELS_PER_LANE = 4 consecutive pixels, a workgroup of 256 lanes 1024.  A float plane is read (written) as one 16-byte
// vector per lane where the lane's first element is 16-byte aligned -- the same answer for every lane of a plane, since a lane's first
// pixel is a multiple of 4: a plane at a 4-byte offset of an allocation, or the v plane of a frame whose H W is no multiple of 4,
// goes by single floats.  The codes of a lane's four pixels are 6 dwords (stride 3; u, v and the validity word of all four) or, at
// stride 4, a dword (u, v) and a 2-byte load (validity) per pixel: the fourth word is never read.  A base that is not 4-byte aligned
// and the last, partial lane of a frame go by 2-byte loads.  Invalid and out-of-range pixels are SELECTED out, never multiplied by
// zero: a NaN behind an invalid pixel stays out of every sum and every gradient.
// Forward: four float sums per workgroup (weighted rho, valid pixels, end-point error, valid pixels with a non-finite u or v: the last
// three at most 1024, exact), wave shuffle then LDS, written to scratch; one wave adds the workgroups' partials in double, in a fixed
// order, and writes loss and row.  Backward: one launch, the count read from the forward's row on the device; all three planes of
// grad_flow are written.  No atomics, no allocation, no synchronisation.
#include "ex4d_internal.h"
#include "../../include/ex4d_loss.h"
#include <cmath>
#include <cstdio>

char *ex4d_loss_error_buffer(size_t *capacity);         // ex4d_loss.hip: the text ex4d_loss_last_error returns

namespace {

#define FL_PPL EX4D_FLOW_PIXELS_PER_LANE
#define FL_THREADS EX4D_FLOW_THREADS
#define FL_WG_PIXELS (FL_PPL * FL_THREADS)
#define FL_FOLD EX4D_FLOW_FOLD
static_assert(FL_PPL == 4, "a lane's pixels are one float4 per plane and 6 dwords of three-word codes");
static_assert(FL_THREADS == 256 && FL_FOLD == 64, "four waves per workgroup; the finish kernel is one wave");

int fail(const char *text)
{
    size_t cap = 0;
    char *buf = ex4d_loss_error_buffer(&cap);
    snprintf(buf, cap, "%s", text);
    return EX4D_ERR_ARG;
}

int launch_status(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return EX4D_OK;
    size_t cap = 0;
    char *buf = ex4d_loss_error_buffer(&cap);
    snprintf(buf, cap, "%s: launch failed: %s", what, hipGetErrorString(e));
    return EX4D_ERR_HIP;
}

// ---- a lane's n <= 4 consecutive elements of a float plane, from element p0 (a multiple of 4)
__device__ __forceinline__ void load4(const float *__restrict__ plane, long long p0, int n, float (&o)[FL_PPL], float fill)
{
    const float *q = plane + p0;
    if (n == FL_PPL && ((uintptr_t)q & 15) == 0) {
        const float4 t = *reinterpret_cast<const float4 *>(q);
        o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < FL_PPL; j++) o[j] = j < n ? q[j] : fill;
    }
}

__device__ __forceinline__ void store4(float *__restrict__ plane, long long p0, int n, const float (&v)[FL_PPL])
{
    float *q = plane + p0;
    if (n == FL_PPL && ((uintptr_t)q & 15) == 0) {
        *reinterpret_cast<float4 *>(q) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < FL_PPL; j++)
            if (j < n) q[j] = v[j];
    }
}

// ---- the codes of the lane's pixels; pixels j >= n come back invalid (validity word 0)
struct Codes { int u[FL_PPL], v[FL_PPL], m[FL_PPL]; };

template <int S>
__device__ __forceinline__ Codes load_codes(const uint16_t *__restrict__ gt, long long p0, int n, bool dwords)
{
    Codes c;
    const uint16_t *q = gt + (size_t)p0 * S;
    if (dwords && n == FL_PPL) {                       // p0 is a multiple of 4: q is 4-byte aligned where gt is
        const uint32_t *d = reinterpret_cast<const uint32_t *>(q);
        if (S == 3) {
            uint32_t w[6];
#pragma unroll
            for (int k = 0; k < 6; k++) w[k] = d[k];
#pragma unroll
            for (int j = 0; j < FL_PPL; j++) {
                const int k = 3 * j;
                c.u[j] = (int)((w[k >> 1] >> (16 * (k & 1))) & 0xffffu);
                c.v[j] = (int)((w[(k + 1) >> 1] >> (16 * ((k + 1) & 1))) & 0xffffu);
                c.m[j] = (int)((w[(k + 2) >> 1] >> (16 * ((k + 2) & 1))) & 0xffffu);
            }
        } else {
#pragma unroll
            for (int j = 0; j < FL_PPL; j++) {
                const uint32_t a = d[2 * j];
                c.u[j] = (int)(a & 0xffffu);
                c.v[j] = (int)(a >> 16);
                c.m[j] = (int)q[4 * j + 2];
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < FL_PPL; j++) {
            const bool in = j < n;
            c.u[j] = in ? (int)q[S * j] : 32768;
            c.v[j] = in ? (int)q[S * j + 1] : 32768;
            c.m[j] = in ? (int)q[S * j + 2] : 0;
        }
    }
    return c;
}

// decode_flow followed by read_opticalflow's scale: the subtraction and the division by 2^8 are exact in float32
__device__ __forceinline__ float decode(int code, float flow_scale) { return (float)(code - 32768) / 256.0f * flow_scale; }

__device__ __forceinline__ bool finite(float x) { return fabsf(x) <= 3.402823466e+38f; }

// ---- N sums over the workgroup's 256 threads, as ex4d_frame_metrics adds them: wave shuffle, then LDS, the four waves in a fixed order
template <typename V, int N>
__device__ __forceinline__ void wave_sum(V (&v)[N])
{
#pragma unroll
    for (int q = 0; q < N; q++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_xor(v[q], o, 64);
    }
}

template <int S>
__global__ __launch_bounds__(FL_THREADS) void flow_loss_fwd_kernel(long long HW, const float *__restrict__ flow,
    const uint16_t *__restrict__ gt, int gt_dwords, float flow_scale, const float *__restrict__ acc, int kind, float eps,
    float *__restrict__ partials)
{
    __shared__ float s[4][FL_THREADS / 64];
    const long long p0 = ((long long)blockIdx.x * FL_THREADS + threadIdx.x) * FL_PPL;
    const int n = p0 >= HW ? 0 : (HW - p0 < FL_PPL ? (int)(HW - p0) : FL_PPL);
    float sums[4] = { 0.f, 0.f, 0.f, 0.f };              // weighted rho, valid pixels, end-point error, non-finite valid pixels
    if (n > 0) {
        float u[FL_PPL], v[FL_PPL], w[FL_PPL];
        load4(flow, p0, n, u, 0.f);
        load4(flow + HW, p0, n, v, 0.f);
        const Codes c = load_codes<S>(gt, p0, n, gt_dwords != 0);
        if (acc) load4(acc, p0, n, w, 0.f);
        const float eps2 = eps * eps;
#pragma unroll
        for (int j = 0; j < FL_PPL; j++) {
            const bool m = c.m[j] > 32768;
            const float ru = u[j] - decode(c.u[j], flow_scale), rv = v[j] - decode(c.v[j], flow_scale);
            const float sq = ru * ru + rv * rv;
            const float rho = kind == EX4D_FLOW_L1 ? fabsf(ru) + fabsf(rv) : sqrtf(sq + eps2);
            const float term = acc ? w[j] * rho : rho;
            sums[0] += m ? term : 0.f;
            sums[1] += m ? 1.f : 0.f;
            sums[2] += m ? sqrtf(sq) : 0.f;
            sums[3] += (m && !(finite(u[j]) && finite(v[j]))) ? 1.f : 0.f;
        }
    }
    wave_sum(sums);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 4; q++) s[q][wave] = sums[q];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int q = threadIdx.x;
        partials[4 * (size_t)blockIdx.x + q] = s[q][0] + s[q][1] + s[q][2] + s[q][3];
    }
}

// one wave: the workgroups' partials added in double, lane i taking workgroups i, i + 64, ... in order, then the shuffle tree
__global__ __launch_bounds__(FL_FOLD) void flow_loss_finish_kernel(int nblocks, const float *__restrict__ partials,
    float *__restrict__ loss, double *__restrict__ row)
{
    double sum[4] = { 0.0, 0.0, 0.0, 0.0 };
    for (int i = threadIdx.x; i < nblocks; i += FL_FOLD) {
#pragma unroll
        for (int q = 0; q < 4; q++) sum[q] += (double)partials[4 * (size_t)i + q];
    }
    wave_sum(sum);
    if (threadIdx.x == 0) {
        const double count = sum[1];
        const double value = sum[0] / (count > 1.0 ? count : 1.0);
        loss[0] = (float)value;
        row[0] = value;
        row[1] = count;
        row[2] = count > 0.0 ? sum[2] / count : 0.0;
        row[3] = sum[3];
    }
}

template <int S>
__global__ __launch_bounds__(FL_THREADS) void flow_loss_bwd_kernel(long long HW, const float *__restrict__ flow,
    const uint16_t *__restrict__ gt, int gt_dwords, float flow_scale, const float *__restrict__ acc, int kind, float eps,
    const double *__restrict__ row, const float *__restrict__ grad_loss, float *__restrict__ grad_flow)
{
    const long long p0 = ((long long)blockIdx.x * FL_THREADS + threadIdx.x) * FL_PPL;
    if (p0 >= HW) return;
    const int n = HW - p0 < FL_PPL ? (int)(HW - p0) : FL_PPL;
    const double count = row[1];
    const float scale = grad_loss[0] / (float)(count > 1.0 ? count : 1.0);
    float u[FL_PPL], v[FL_PPL], w[FL_PPL], gu[FL_PPL], gv[FL_PPL];
    const float zero[FL_PPL] = { 0.f, 0.f, 0.f, 0.f };
    load4(flow, p0, n, u, 0.f);
    load4(flow + HW, p0, n, v, 0.f);
    const Codes c = load_codes<S>(gt, p0, n, gt_dwords != 0);
    if (acc) load4(acc, p0, n, w, 0.f);
    const float eps2 = eps * eps;
#pragma unroll
    for (int j = 0; j < FL_PPL; j++) {
        const bool m = c.m[j] > 32768;
        const float ru = u[j] - decode(c.u[j], flow_scale), rv = v[j] - decode(c.v[j], flow_scale);
        float du, dv;
        if (kind == EX4D_FLOW_L1) {
            du = (float)((ru > 0.f) - (ru < 0.f));
            dv = (float)((rv > 0.f) - (rv < 0.f));
        } else {
            const float rho = sqrtf(ru * ru + rv * rv + eps2);
            du = ru / rho;
            dv = rv / rho;
        }
        const float k = acc ? scale * w[j] : scale;
        gu[j] = m ? k * du : 0.f;
        gv[j] = m ? k * dv : 0.f;
    }
    store4(grad_flow, p0, n, gu);
    store4(grad_flow + HW, p0, n, gv);
    store4(grad_flow + 2 * HW, p0, n, zero);
}

inline long long blocks_of(long long HW) { return (HW + FL_WG_PIXELS - 1) / FL_WG_PIXELS; }

// what both calls refuse before any launch; NULL where the arguments are fine
const char *refusal(int H, int W, const void *flow, const void *gt, int pixel_stride, int kind, float eps)
{
    static char text[160];
    if (H <= 0 || W <= 0) { snprintf(text, sizeof(text), "flow loss: image %d x %d: H and W must be positive", H, W); return text; }
    if (blocks_of((long long)H * W) > 0x7fffffffLL) { snprintf(text, sizeof(text), "flow loss: image %d x %d: too many pixels for one launch", H, W); return text; }
    if (pixel_stride != 3 && pixel_stride != 4) {
        snprintf(text, sizeof(text), "flow loss: pixel_stride %d: encoded flow has 3 or 4 words per pixel", pixel_stride);
        return text;
    }
    if (kind != EX4D_FLOW_L1 && kind != EX4D_FLOW_CHARBONNIER) {
        snprintf(text, sizeof(text), "flow loss: kind %d: EX4D_FLOW_L1 (0) or EX4D_FLOW_CHARBONNIER (1)", kind);
        return text;
    }
    if (kind == EX4D_FLOW_CHARBONNIER && !(eps > 0.f && std::isfinite(eps))) {
        snprintf(text, sizeof(text), "flow loss: eps %g: Charbonnier needs a finite eps > 0", (double)eps);
        return text;
    }
    if (!flow) return "flow loss: flow is NULL";
    if (!gt) return "flow loss: gt is NULL";
    return nullptr;
}

}  // namespace

extern "C" {

size_t ex4d_flow_loss_scratch_floats(int32_t H, int32_t W)
{
    return (H <= 0 || W <= 0) ? 0 : 4 * (size_t)blocks_of((long long)H * W) + 64;
}

int ex4d_flow_loss_forward(int32_t H, int32_t W, const float *flow, const void *gt, int32_t pixel_stride, float flow_scale,
                           const float *acc, int32_t kind, float eps, float *loss, double *row, float *scratch, void *stream_)
{
    size_t cap = 0;
    ex4d_loss_error_buffer(&cap)[0] = 0;
    if (const char *why = refusal(H, W, flow, gt, pixel_stride, kind, eps)) return fail(why);
    if (!loss) return fail("flow loss: loss is NULL");
    if (!row) return fail("flow loss: row is NULL");
    if (!scratch) return fail("flow loss: scratch is NULL");
    const long long HW = (long long)H * W;
    const int nblocks = (int)blocks_of(HW), dwords = ((uintptr_t)gt & 3) == 0;
    const uint16_t *codes = static_cast<const uint16_t *>(gt);
    hipStream_t stream = (hipStream_t)stream_;
    if (pixel_stride == 3)
        hipLaunchKernelGGL(flow_loss_fwd_kernel<3>, dim3(nblocks), dim3(FL_THREADS), 0, stream, HW, flow, codes, dwords, flow_scale, acc, kind, eps, scratch);
    else
        hipLaunchKernelGGL(flow_loss_fwd_kernel<4>, dim3(nblocks), dim3(FL_THREADS), 0, stream, HW, flow, codes, dwords, flow_scale, acc, kind, eps, scratch);
    hipLaunchKernelGGL(flow_loss_finish_kernel, dim3(1), dim3(FL_FOLD), 0, stream, nblocks, scratch, loss, row);
    return launch_status("ex4d_flow_loss_forward");
}

int ex4d_flow_loss_backward(int32_t H, int32_t W, const float *flow, const void *gt, int32_t pixel_stride, float flow_scale,
                            const float *acc, int32_t kind, float eps, const double *row, const float *grad_loss, float *grad_flow,
                            void *stream_)
{
    size_t cap = 0;
    ex4d_loss_error_buffer(&cap)[0] = 0;
    if (const char *why = refusal(H, W, flow, gt, pixel_stride, kind, eps)) return fail(why);
    if (!row) return fail("flow loss: row is NULL");
    if (!grad_loss) return fail("flow loss: grad_loss is NULL");
    if (!grad_flow) return fail("flow loss: grad_flow is NULL");
    const long long HW = (long long)H * W;
    const int nblocks = (int)blocks_of(HW), dwords = ((uintptr_t)gt & 3) == 0;
    const uint16_t *codes = static_cast<const uint16_t *>(gt);
    hipStream_t stream = (hipStream_t)stream_;
    if (pixel_stride == 3)
        hipLaunchKernelGGL(flow_loss_bwd_kernel<3>, dim3(nblocks), dim3(FL_THREADS), 0, stream, HW, flow, codes, dwords, flow_scale, acc, kind, eps, row, grad_loss, grad_flow);
    else
        hipLaunchKernelGGL(flow_loss_bwd_kernel<4>, dim3(nblocks), dim3(FL_THREADS), 0, stream, HW, flow, codes, dwords, flow_scale, acc, kind, eps, row, grad_loss, grad_flow);
    return launch_status("ex4d_flow_loss_backward");
}

}  // extern "C"
