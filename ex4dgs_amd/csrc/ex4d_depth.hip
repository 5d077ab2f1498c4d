// Fused inverse-depth loss with a per-frame scale-and-shift fit, forward and backward, for gfx950 (include/ex4d_loss.h, "DEPTH").
//
// The reference carries a frame's depth as a 16-bit inverse-depth map (scene/dataset_readers.py:45 depth_path, utils/general_utils.py:32-36
// load_depth).  The kernels decode on load -- 2 (or 4) bytes per pixel -- and compare with the reciprocal of the rasterizer's `depth`
// output, float32 [H,W]:
//     g = v * code_scale,   valid = v finite and v > 0,   m = valid and (no acc or acc > 0)
//     x = 1.0f / depth,   gh = s g + o,   r = x - gh,   rho = |r|   or   sqrt(r^2 + eps^2)
//     loss = sum m w rho / max(sum m, 1),   w = acc[p] (a constant) or 1
// with (s, o) given, or the least-squares fit of gh to x over m.  This file is compiled with -ffp-contract=off: the multiply and the add
// of gh round separately, and the forward and the backward see the same residual.
//
// THE PASS is the streaming pass of ex4d_pixel_stream.h: four consecutive pixels per lane, float planes through load4 / store4, a row of
// sums per workgroup, one wave folding the rows in a fixed order.  What is the depth loss's own: the four uint16 codes of a lane go as
// one 8-byte vector where their address is 8-byte aligned, element by element otherwise and in the last, partial lane.  Pixels outside m
// are SELECTED out, never multiplied by zero.  Every sum is double from the lane on (a product of two floats is exact there).
// FIT forward: moments -> solve (the folding wave; writes float s, o to the head of scratch) -> loss -> finish (that wave again; writes
// loss and row).  GIVEN forward: loss -> finish.  Backward: one launch; s, o and n are read from the forward's row on the device, so
// the fit is a constant there.  No atomics, no allocation, no synchronisation.
#include "ex4d_internal.h"
#include "ex4d_pixel_stream.h"
#define EX4D_ERROR_BUFFER ex4d_loss_error_buffer        // ex4d_loss.hip: the text ex4d_loss_last_error returns
#include "ex4d_host_error.h"

namespace {

#define DP_MOMENTS 5                   // n, Sg, Sx, Sgg, Sgx
#define DP_SUMS 4                      // weighted rho, n, r^2, m pixels with a bad depth
#define DP_HEAD_BYTES 16               // scratch: float s, o (the fit), then the moments' rows, then the loss pass's rows

// ---- the raw ground-truth values of the lane's pixels; pixels j >= n come back 0 (no measurement)
template <int GT>
__device__ __forceinline__ void load_raw(const void *__restrict__ gt, long long p0, int n, float (&v)[PS_PPL])
{
    if (GT == EX4D_DEPTH_GT_F32) {
        load4(static_cast<const float *>(gt), p0, n, v, 0.f);
    } else {
        const uint16_t *q = static_cast<const uint16_t *>(gt) + p0;
        if (n == PS_PPL && ((uintptr_t)q & 7) == 0) {
            const uint2 t = *reinterpret_cast<const uint2 *>(q);
            v[0] = (float)(t.x & 0xffffu); v[1] = (float)(t.x >> 16);
            v[2] = (float)(t.y & 0xffffu); v[3] = (float)(t.y >> 16);
        } else {
#pragma unroll
            for (int j = 0; j < PS_PPL; j++) v[j] = j < n ? (float)q[j] : 0.f;
        }
    }
}

__device__ __forceinline__ bool measured(float v) { return v > 0.f && finite(v); }

// ---- a lane's pixels: depth, decoded ground truth, weight, mask
struct Pixels { float d[PS_PPL], g[PS_PPL], w[PS_PPL]; bool m[PS_PPL]; };

template <int GT>
__device__ __forceinline__ Pixels load_pixels(long long p0, int n, const float *__restrict__ depth, const void *__restrict__ gt,
                                              float code_scale, const float *__restrict__ acc)
{
    Pixels px;
    float v[PS_PPL];
    load4(depth, p0, n, px.d, 1.f);
    load_raw<GT>(gt, p0, n, v);
    if (acc) load4(acc, p0, n, px.w, 0.f);
#pragma unroll
    for (int j = 0; j < PS_PPL; j++) {
        px.g[j] = v[j] * code_scale;
        px.m[j] = measured(v[j]) && (!acc || px.w[j] > 0.f);
        if (!acc) px.w[j] = 1.f;
    }
    return px;
}

template <int GT>
__global__ __launch_bounds__(PS_THREADS) void depth_moments_kernel(long long HW, const float *__restrict__ depth,
    const void *__restrict__ gt, float code_scale, const float *__restrict__ acc, double *__restrict__ rows)
{
    const long long p0 = first_pixel();
    const int n = pixels_from(p0, HW);
    double sums[DP_MOMENTS] = { 0.0, 0.0, 0.0, 0.0, 0.0 };
    if (n > 0) {
        const Pixels px = load_pixels<GT>(p0, n, depth, gt, code_scale, acc);
#pragma unroll
        for (int j = 0; j < PS_PPL; j++) {
            const double g = (double)px.g[j], x = (double)(1.0f / px.d[j]);
            sums[0] += px.m[j] ? 1.0 : 0.0;
            sums[1] += px.m[j] ? g : 0.0;
            sums[2] += px.m[j] ? x : 0.0;
            sums[3] += px.m[j] ? g * g : 0.0;
            sums[4] += px.m[j] ? g * x : 0.0;
        }
    }
    workgroup_row(sums, rows);
}

__global__ __launch_bounds__(PS_FOLD) void depth_solve_kernel(int nblocks, const double *__restrict__ rows, float *__restrict__ fit)
{
    double sum[DP_MOMENTS];
    fold_rows(nblocks, rows, sum);
    if (threadIdx.x == 0) {
        const double n = sum[0], Sg = sum[1], Sx = sum[2], Sgg = sum[3], Sgx = sum[4];
        const double det = n * Sgg - Sg * Sg;
        double s = 0.0, o = Sx / (n > 1.0 ? n : 1.0);
        if (n >= 2.0 && det > 1e-10 * n * Sgg) {
            s = (n * Sgx - Sg * Sx) / det;
            o = (Sx - s * Sg) / n;
        }
        fit[0] = (float)s;
        fit[1] = (float)o;
    }
}

template <int GT>
__global__ __launch_bounds__(PS_THREADS) void depth_loss_kernel(long long HW, const float *__restrict__ depth,
    const void *__restrict__ gt, float code_scale, const float *__restrict__ acc, const float *__restrict__ fit, float scale, float offset,
    int kind, float eps, double *__restrict__ rows)
{
    const long long p0 = first_pixel();
    const int n = pixels_from(p0, HW);
    double sums[DP_SUMS] = { 0.0, 0.0, 0.0, 0.0 };
    if (n > 0) {
        const float s = fit ? fit[0] : scale, o = fit ? fit[1] : offset;
        const Pixels px = load_pixels<GT>(p0, n, depth, gt, code_scale, acc);
        const float eps2 = eps * eps;
#pragma unroll
        for (int j = 0; j < PS_PPL; j++) {
            const float d = px.d[j];
            const float r = 1.0f / d - (s * px.g[j] + o);
            const float rho = kind == EX4D_DEPTH_L1 ? fabsf(r) : sqrtf(r * r + eps2);
            const float term = px.w[j] * rho;
            sums[0] += px.m[j] ? (double)term : 0.0;
            sums[1] += px.m[j] ? 1.0 : 0.0;
            sums[2] += px.m[j] ? (double)r * (double)r : 0.0;
            sums[3] += (px.m[j] && !(d > 0.f && finite(d))) ? 1.0 : 0.0;
        }
    }
    workgroup_row(sums, rows);
}

__global__ __launch_bounds__(PS_FOLD) void depth_finish_kernel(int nblocks, const double *__restrict__ rows, const float *__restrict__ fit,
    float scale, float offset, float *__restrict__ loss, double *__restrict__ row)
{
    double sum[DP_SUMS];
    fold_rows(nblocks, rows, sum);
    if (threadIdx.x == 0) {
        const double count = sum[1];
        const double value = sum[0] / (count > 1.0 ? count : 1.0);
        loss[0] = (float)value;
        row[0] = value;
        row[1] = count;
        row[2] = (double)(fit ? fit[0] : scale);
        row[3] = (double)(fit ? fit[1] : offset);
        row[4] = count > 0.0 ? sqrt(sum[2] / count) : 0.0;
        row[5] = sum[3];
    }
}

template <int GT>
__global__ __launch_bounds__(PS_THREADS) void depth_loss_bwd_kernel(long long HW, const float *__restrict__ depth,
    const void *__restrict__ gt, float code_scale, const float *__restrict__ acc, int kind, float eps, const double *__restrict__ row,
    const float *__restrict__ grad_loss, float *__restrict__ grad_depth)
{
    const long long p0 = first_pixel();
    const int n = pixels_from(p0, HW);
    if (n == 0) return;
    const double count = row[1];
    const float s = (float)row[2], o = (float)row[3];
    const float k = grad_loss[0] / (float)(count > 1.0 ? count : 1.0);
    const Pixels px = load_pixels<GT>(p0, n, depth, gt, code_scale, acc);
    const float eps2 = eps * eps;
    float out[PS_PPL];
#pragma unroll
    for (int j = 0; j < PS_PPL; j++) {
        const float x = 1.0f / px.d[j];
        const float r = x - (s * px.g[j] + o);
        const float dr = kind == EX4D_DEPTH_L1 ? (float)((r > 0.f) - (r < 0.f)) : r / sqrtf(r * r + eps2);
        const float kw = acc ? k * px.w[j] : k;
        out[j] = px.m[j] ? kw * dr * -(x * x) : 0.f;
    }
    store4(grad_depth, p0, n, out);
}

// what both calls refuse before any launch; NULL where the arguments are fine
const char *refusal(int H, int W, const void *depth, const void *gt, int gt_type, float code_scale, int align, int kind, float eps)
{
    static char text[160], text_late[160];
    const char *own = nullptr, *late = nullptr;
    if (gt_type != EX4D_DEPTH_GT_U16 && gt_type != EX4D_DEPTH_GT_F32) {
        snprintf(text, sizeof(text), "depth loss: gt_type %d: EX4D_DEPTH_GT_U16 (0) or EX4D_DEPTH_GT_F32 (1)", gt_type);
        own = text;
    } else if (align != EX4D_DEPTH_ALIGN_GIVEN && align != EX4D_DEPTH_ALIGN_FIT) {
        snprintf(text, sizeof(text), "depth loss: align %d: EX4D_DEPTH_ALIGN_GIVEN (0) or EX4D_DEPTH_ALIGN_FIT (1)", align);
        own = text;
    }
    if (!(code_scale > 0.f && std::isfinite(code_scale))) {
        snprintf(text_late, sizeof(text_late), "depth loss: code_scale %g: must be finite and > 0", (double)code_scale);
        late = text_late;
    }
    return pixel_loss_refusal("depth loss", "EX4D_DEPTH", H, W, own, kind, eps, late, "depth", depth, gt);
}

}  // namespace

extern "C" {

size_t ex4d_depth_loss_scratch_bytes(int32_t H, int32_t W)
{
    if (H <= 0 || W <= 0 || blocks_of((long long)H * W) > 0x7fffffffLL) return 0;
    return DP_HEAD_BYTES + sizeof(double) * (DP_MOMENTS + DP_SUMS) * (size_t)blocks_of((long long)H * W);
}

int ex4d_depth_loss_forward(int32_t H, int32_t W, const float *depth, const void *gt, int32_t gt_type, float code_scale,
                            const float *acc, int32_t align, float scale, float offset, int32_t kind, float eps, float *loss,
                            double *row, void *scratch, void *stream_)
{
    clear_error();
    if (const char *why = refusal(H, W, depth, gt, gt_type, code_scale, align, kind, eps)) return fail(EX4D_ERR_ARG, why);
    if (align == EX4D_DEPTH_ALIGN_GIVEN && !(std::isfinite(scale) && std::isfinite(offset))) {
        char text[160];
        snprintf(text, sizeof(text), "depth loss: scale %g, offset %g: EX4D_DEPTH_ALIGN_GIVEN needs both finite", (double)scale, (double)offset);
        return fail(EX4D_ERR_ARG, text);
    }
    if (!loss) return fail(EX4D_ERR_ARG, "depth loss: loss is NULL");
    if (!row) return fail(EX4D_ERR_ARG, "depth loss: row is NULL");
    if (!scratch) return fail(EX4D_ERR_ARG, "depth loss: scratch is NULL");
    if ((uintptr_t)scratch & 7) return fail(EX4D_ERR_ARG, "depth loss: scratch is not 8-byte aligned");
    const long long HW = (long long)H * W;
    const int nblocks = (int)blocks_of(HW);
    float *head = static_cast<float *>(scratch);
    double *moments = reinterpret_cast<double *>(static_cast<char *>(scratch) + DP_HEAD_BYTES);
    double *sums = moments + DP_MOMENTS * (size_t)nblocks;
    const float *fit = align == EX4D_DEPTH_ALIGN_FIT ? head : nullptr;
    const bool u16 = gt_type == EX4D_DEPTH_GT_U16;
    hipStream_t stream = (hipStream_t)stream_;
    if (fit) {
        if (u16)
            hipLaunchKernelGGL(depth_moments_kernel<EX4D_DEPTH_GT_U16>, dim3(nblocks), dim3(PS_THREADS), 0, stream, HW, depth, gt, code_scale, acc, moments);
        else
            hipLaunchKernelGGL(depth_moments_kernel<EX4D_DEPTH_GT_F32>, dim3(nblocks), dim3(PS_THREADS), 0, stream, HW, depth, gt, code_scale, acc, moments);
        hipLaunchKernelGGL(depth_solve_kernel, dim3(1), dim3(PS_FOLD), 0, stream, nblocks, moments, head);
    }
    if (u16)
        hipLaunchKernelGGL(depth_loss_kernel<EX4D_DEPTH_GT_U16>, dim3(nblocks), dim3(PS_THREADS), 0, stream, HW, depth, gt, code_scale, acc, fit, scale, offset, kind, eps, sums);
    else
        hipLaunchKernelGGL(depth_loss_kernel<EX4D_DEPTH_GT_F32>, dim3(nblocks), dim3(PS_THREADS), 0, stream, HW, depth, gt, code_scale, acc, fit, scale, offset, kind, eps, sums);
    hipLaunchKernelGGL(depth_finish_kernel, dim3(1), dim3(PS_FOLD), 0, stream, nblocks, sums, fit, scale, offset, loss, row);
    return launch_status("ex4d_depth_loss_forward");
}

int ex4d_depth_loss_backward(int32_t H, int32_t W, const float *depth, const void *gt, int32_t gt_type, float code_scale,
                             const float *acc, int32_t align, int32_t kind, float eps, const double *row, const float *grad_loss,
                             float *grad_depth, void *stream_)
{
    clear_error();
    if (const char *why = refusal(H, W, depth, gt, gt_type, code_scale, align, kind, eps)) return fail(EX4D_ERR_ARG, why);
    if (!row) return fail(EX4D_ERR_ARG, "depth loss: row is NULL");
    if (!grad_loss) return fail(EX4D_ERR_ARG, "depth loss: grad_loss is NULL");
    if (!grad_depth) return fail(EX4D_ERR_ARG, "depth loss: grad_depth is NULL");
    const long long HW = (long long)H * W;
    const int nblocks = (int)blocks_of(HW);
    hipStream_t stream = (hipStream_t)stream_;
    if (gt_type == EX4D_DEPTH_GT_U16)
        hipLaunchKernelGGL(depth_loss_bwd_kernel<EX4D_DEPTH_GT_U16>, dim3(nblocks), dim3(PS_THREADS), 0, stream, HW, depth, gt, code_scale, acc, kind, eps, row, grad_loss, grad_depth);
    else
        hipLaunchKernelGGL(depth_loss_bwd_kernel<EX4D_DEPTH_GT_F32>, dim3(nblocks), dim3(PS_THREADS), 0, stream, HW, depth, gt, code_scale, acc, kind, eps, row, grad_loss, grad_depth);
    return launch_status("ex4d_depth_loss_backward");
}

}  // extern "C"
