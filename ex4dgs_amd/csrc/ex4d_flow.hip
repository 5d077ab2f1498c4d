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
// THE PASS is the streaming pass of ex4d_pixel_stream.h: four consecutive pixels per lane, float planes through load4 / store4, a row of
// sums per workgroup, one wave folding the rows in a fixed order.  What is the flow loss's own: the codes of a lane's four pixels are
// 6 dwords (stride 3; u, v and the validity word of all four) or, at stride 4, a dword (u, v) and a 2-byte load (validity) per pixel:
// the fourth word is never read.  A base that is not 4-byte aligned and the last, partial lane of a frame go by 2-byte loads.  Invalid
// and out-of-range pixels are SELECTED out, never multiplied by zero: a NaN behind an invalid pixel stays out of every sum and every
// gradient.
// Forward: four float sums per workgroup (weighted rho, valid pixels, end-point error, valid pixels with a non-finite u or v: the last
// three at most 1024, exact) written to scratch; the finishing wave adds them in double and writes loss and row.  Backward: one launch,
// the count read from the forward's row on the device; all three planes of grad_flow are written.  No atomics, no allocation, no
// synchronisation.
#include "ex4d_internal.h"
#include "ex4d_pixel_stream.h"
#define EX4D_ERROR_BUFFER ex4d_loss_error_buffer        // ex4d_loss.hip: the text ex4d_loss_last_error returns
#include "ex4d_host_error.h"

namespace {

#define FL_SUMS 4                      // weighted rho, valid pixels, end-point error, non-finite valid pixels

// ---- the codes of the lane's pixels; pixels j >= n come back invalid (validity word 0)
struct Codes { int u[PS_PPL], v[PS_PPL], m[PS_PPL]; };

template <int S>
__device__ __forceinline__ Codes load_codes(const uint16_t *__restrict__ gt, long long p0, int n, bool dwords)
{
    Codes c;
    const uint16_t *q = gt + (size_t)p0 * S;
    if (dwords && n == PS_PPL) {                       // p0 is a multiple of 4: q is 4-byte aligned where gt is
        const uint32_t *d = reinterpret_cast<const uint32_t *>(q);
        if (S == 3) {
            uint32_t w[6];
#pragma unroll
            for (int k = 0; k < 6; k++) w[k] = d[k];
#pragma unroll
            for (int j = 0; j < PS_PPL; j++) {
                const int k = 3 * j;
                c.u[j] = (int)((w[k >> 1] >> (16 * (k & 1))) & 0xffffu);
                c.v[j] = (int)((w[(k + 1) >> 1] >> (16 * ((k + 1) & 1))) & 0xffffu);
                c.m[j] = (int)((w[(k + 2) >> 1] >> (16 * ((k + 2) & 1))) & 0xffffu);
            }
        } else {
#pragma unroll
            for (int j = 0; j < PS_PPL; j++) {
                const uint32_t a = d[2 * j];
                c.u[j] = (int)(a & 0xffffu);
                c.v[j] = (int)(a >> 16);
                c.m[j] = (int)q[4 * j + 2];
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < PS_PPL; j++) {
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

template <int S>
__global__ __launch_bounds__(PS_THREADS) void flow_loss_fwd_kernel(long long HW, const float *__restrict__ flow,
    const uint16_t *__restrict__ gt, int gt_dwords, float flow_scale, const float *__restrict__ acc, int kind, float eps,
    float *__restrict__ partials)
{
    __shared__ float s[FL_SUMS][PS_THREADS / 64];
    const long long p0 = first_pixel();
    const int n = pixels_from(p0, HW);
    float sums[FL_SUMS] = { 0.f, 0.f, 0.f, 0.f };
    if (n > 0) {
        float u[PS_PPL], v[PS_PPL], w[PS_PPL];
        load4(flow, p0, n, u, 0.f);
        load4(flow + HW, p0, n, v, 0.f);
        const Codes c = load_codes<S>(gt, p0, n, gt_dwords != 0);
        if (acc) load4(acc, p0, n, w, 0.f);
        const float eps2 = eps * eps;
#pragma unroll
        for (int j = 0; j < PS_PPL; j++) {
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
    // MIRRORS workgroup_row<float, FL_SUMS> of ex4d_pixel_stream.h, same additions in the same order: through the function the compiler
    // schedules the four LDS writes differently ("The streaming pixel pass, said once")
    wave_sum(sums);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < FL_SUMS; q++) s[q][wave] = sums[q];
    }
    __syncthreads();
    if (threadIdx.x < FL_SUMS) {
        const int q = threadIdx.x;
        partials[FL_SUMS * (size_t)blockIdx.x + q] = s[q][0] + s[q][1] + s[q][2] + s[q][3];
    }
}

__global__ __launch_bounds__(PS_FOLD) void flow_loss_finish_kernel(int nblocks, const float *__restrict__ partials,
    float *__restrict__ loss, double *__restrict__ row)
{
    // MIRRORS fold_rows<float, FL_SUMS> of ex4d_pixel_stream.h: through the function the four sums become four registers pairs where
    // this text gives one vector of four, and the loop's preamble is ordered differently
    double sum[FL_SUMS] = { 0.0, 0.0, 0.0, 0.0 };
    for (int i = threadIdx.x; i < nblocks; i += PS_FOLD) {
#pragma unroll
        for (int q = 0; q < FL_SUMS; q++) sum[q] += (double)partials[FL_SUMS * (size_t)i + q];
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
__global__ __launch_bounds__(PS_THREADS) void flow_loss_bwd_kernel(long long HW, const float *__restrict__ flow,
    const uint16_t *__restrict__ gt, int gt_dwords, float flow_scale, const float *__restrict__ acc, int kind, float eps,
    const double *__restrict__ row, const float *__restrict__ grad_loss, float *__restrict__ grad_flow)
{
    const long long p0 = first_pixel();
    if (p0 >= HW) return;                                // before pixels_from, not `n == 0` after it: that keeps this kernel's stream
    const int n = pixels_from(p0, HW);
    const double count = row[1];
    const float scale = grad_loss[0] / (float)(count > 1.0 ? count : 1.0);
    float u[PS_PPL], v[PS_PPL], w[PS_PPL], gu[PS_PPL], gv[PS_PPL];
    const float zero[PS_PPL] = { 0.f, 0.f, 0.f, 0.f };
    load4(flow, p0, n, u, 0.f);
    load4(flow + HW, p0, n, v, 0.f);
    const Codes c = load_codes<S>(gt, p0, n, gt_dwords != 0);
    if (acc) load4(acc, p0, n, w, 0.f);
    const float eps2 = eps * eps;
#pragma unroll
    for (int j = 0; j < PS_PPL; j++) {
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

// what both calls refuse before any launch; NULL where the arguments are fine
const char *refusal(int H, int W, const void *flow, const void *gt, int pixel_stride, int kind, float eps)
{
    static char text[160];
    const char *own = nullptr;
    if (pixel_stride != 3 && pixel_stride != 4) {
        snprintf(text, sizeof(text), "flow loss: pixel_stride %d: encoded flow has 3 or 4 words per pixel", pixel_stride);
        own = text;
    }
    return pixel_loss_refusal("flow loss", "EX4D_FLOW", H, W, own, kind, eps, nullptr, "flow", flow, gt);
}

}  // namespace

extern "C" {

size_t ex4d_flow_loss_scratch_floats(int32_t H, int32_t W)
{
    return (H <= 0 || W <= 0) ? 0 : FL_SUMS * (size_t)blocks_of((long long)H * W) + 64;
}

int ex4d_flow_loss_forward(int32_t H, int32_t W, const float *flow, const void *gt, int32_t pixel_stride, float flow_scale,
                           const float *acc, int32_t kind, float eps, float *loss, double *row, float *scratch, void *stream_)
{
    clear_error();
    if (const char *why = refusal(H, W, flow, gt, pixel_stride, kind, eps)) return fail(EX4D_ERR_ARG, why);
    if (!loss) return fail(EX4D_ERR_ARG, "flow loss: loss is NULL");
    if (!row) return fail(EX4D_ERR_ARG, "flow loss: row is NULL");
    if (!scratch) return fail(EX4D_ERR_ARG, "flow loss: scratch is NULL");
    const long long HW = (long long)H * W;
    const int nblocks = (int)blocks_of(HW), dwords = ((uintptr_t)gt & 3) == 0;
    const uint16_t *codes = static_cast<const uint16_t *>(gt);
    hipStream_t stream = (hipStream_t)stream_;
    if (pixel_stride == 3)
        hipLaunchKernelGGL(flow_loss_fwd_kernel<3>, dim3(nblocks), dim3(PS_THREADS), 0, stream, HW, flow, codes, dwords, flow_scale, acc, kind, eps, scratch);
    else
        hipLaunchKernelGGL(flow_loss_fwd_kernel<4>, dim3(nblocks), dim3(PS_THREADS), 0, stream, HW, flow, codes, dwords, flow_scale, acc, kind, eps, scratch);
    hipLaunchKernelGGL(flow_loss_finish_kernel, dim3(1), dim3(PS_FOLD), 0, stream, nblocks, scratch, loss, row);
    return launch_status("ex4d_flow_loss_forward");
}

int ex4d_flow_loss_backward(int32_t H, int32_t W, const float *flow, const void *gt, int32_t pixel_stride, float flow_scale,
                            const float *acc, int32_t kind, float eps, const double *row, const float *grad_loss, float *grad_flow,
                            void *stream_)
{
    clear_error();
    if (const char *why = refusal(H, W, flow, gt, pixel_stride, kind, eps)) return fail(EX4D_ERR_ARG, why);
    if (!row) return fail(EX4D_ERR_ARG, "flow loss: row is NULL");
    if (!grad_loss) return fail(EX4D_ERR_ARG, "flow loss: grad_loss is NULL");
    if (!grad_flow) return fail(EX4D_ERR_ARG, "flow loss: grad_flow is NULL");
    const long long HW = (long long)H * W;
    const int nblocks = (int)blocks_of(HW), dwords = ((uintptr_t)gt & 3) == 0;
    const uint16_t *codes = static_cast<const uint16_t *>(gt);
    hipStream_t stream = (hipStream_t)stream_;
    if (pixel_stride == 3)
        hipLaunchKernelGGL(flow_loss_bwd_kernel<3>, dim3(nblocks), dim3(PS_THREADS), 0, stream, HW, flow, codes, dwords, flow_scale, acc, kind, eps, row, grad_loss, grad_flow);
    else
        hipLaunchKernelGGL(flow_loss_bwd_kernel<4>, dim3(nblocks), dim3(PS_THREADS), 0, stream, HW, flow, codes, dwords, flow_scale, acc, kind, eps, row, grad_loss, grad_flow);
    return launch_status("ex4d_flow_loss_backward");
}

}  // extern "C"
