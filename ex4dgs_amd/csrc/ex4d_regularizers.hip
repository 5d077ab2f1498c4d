// The motion regularisers of train.py:155-168 as a stand-alone op (include/ex4d_regularizers.h): loss value and dense gradients.
// The per-iteration hot path is the regularised sliced RAdam step (ex4d_optim.hip), which never materialises these gradients; this
// file serves autograd users, the dense-gradient trainer paths (whole tensors, or the element range a rank of the sharded optimizer
// owns: ex4d_reg_backward_range), the _xyz_disp term and the reported loss value.
// ffp-contract is off for this file: the gradient arithmetic (ex4d_reg_rows.h) is shared bit for bit with ex4d_optim.hip.
#include "ex4d_internal.h"
#include "ex4d_reg_rows.h"
#include "../../include/ex4d_regularizers.h"
#include <cstdio>

namespace {

#define REG_FWD_BLOCKS 1024       // fixed grid of the forward: the partial-sum layout does not depend on the model's size
#define REG_THREADS 256

// block-wide sum of three doubles in a fixed order (wave shuffles, then the waves' results through LDS); valid in thread 0
__device__ __forceinline__ void block_sum3(double (&x)[3], double (*lds)[3])
{
#pragma unroll
    for (int j = 0; j < 3; j++)
        for (int off = 32; off > 0; off >>= 1) x[j] += __shfl_down(x[j], off, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { lds[wave][0] = x[0]; lds[wave][1] = x[1]; lds[wave][2] = x[2]; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int j = 0; j < 3; j++) {
            double s = 0.0;
            for (int w = 0; w < REG_THREADS / 64; w++) s += lds[w][j];
            x[j] = s;
        }
}

// grid-stride over the Ns static rows and the Nd*K keyframe slices; double arithmetic on the float32 parameters
__global__ __launch_bounds__(REG_THREADS) void reg_fwd_kernel(const float *disp, long long Ns, const float *motion, const float *rot,
                                                              long long Nd, int K, double *partial)
{
    __shared__ double lds[REG_THREADS / 64][3];
    double acc[3] = {0.0, 0.0, 0.0};
    const long long stride = (long long)gridDim.x * REG_THREADS;
    const long long tid = (long long)blockIdx.x * REG_THREADS + threadIdx.x;
    if (disp)
        for (long long i = tid; i < Ns; i += stride) {
            const double x = disp[3 * i], y = disp[3 * i + 1], z = disp[3 * i + 2];
            acc[0] += log(sqrt(x * x + y * y + z * z) + 0.001);
        }
    const long long slices = Nd * K;
    for (long long s = tid; s < slices; s += stride) {
        const long long row = s / K;
        const int k = (int)(s - row * K);
        if (k == 0) continue;
        if (motion) {
            const float *p0 = motion + row * K * 3, *pk = p0 + 3 * k;
            const double x = (double)p0[0] - pk[0], y = (double)p0[1] - pk[1], z = (double)p0[2] - pk[2];
            acc[1] += sqrt(x * x + y * y + z * z);
        }
        if (rot) {
            const float *a = rot + (row * K + k) * 4, *b = a - 4;
            const double na = sqrt((double)a[0] * a[0] + (double)a[1] * a[1] + (double)a[2] * a[2] + (double)a[3] * a[3]);
            const double nb = sqrt((double)b[0] * b[0] + (double)b[1] * b[1] + (double)b[2] * b[2] + (double)b[3] * b[3]);
            const double dot = (double)a[0] * b[0] + (double)a[1] * b[1] + (double)a[2] * b[2] + (double)a[3] * b[3];
            acc[2] += 1.0 - dot / fmax(na, 1e-6) / fmax(nb, 1e-6);
        }
    }
    block_sum3(acc, lds);
    if (threadIdx.x == 0) { partial[3 * blockIdx.x] = acc[0]; partial[3 * blockIdx.x + 1] = acc[1]; partial[3 * blockIdx.x + 2] = acc[2]; }
}

__global__ __launch_bounds__(REG_THREADS) void reg_finish_kernel(const double *partial, double inv_s, double inv_d, double w0, double w1, double w2,
                                                                 float *out4)
{
    __shared__ double lds[REG_THREADS / 64][3];
    double acc[3] = {0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < REG_FWD_BLOCKS; b += REG_THREADS) { acc[0] += partial[3 * b]; acc[1] += partial[3 * b + 1]; acc[2] += partial[3 * b + 2]; }
    block_sum3(acc, lds);
    if (threadIdx.x == 0) {
        const double m0 = acc[0] * inv_s, m1 = acc[1] * inv_d, m2 = acc[2] * inv_d;
        out4[0] = (float)m0; out4[1] = (float)m1; out4[2] = (float)m2;
        out4[3] = (float)(w0 * m0 + w1 * m1 + w2 * m2);
    }
}

__device__ __forceinline__ float scaled(float coef, const float *upstream) { return upstream ? coef * upstream[0] : coef; }

// kinds of ex4d_reg_backward_range: ex4d_reg::KIND_MOTION (1, [rows,K,3]) and KIND_ROT (2, [rows,K,4]) keep reg_kind's numbering; 3 is static_reg
constexpr int KIND_STATIC = 3;   // [rows,3]: one slice per row, K plays no part
template <int KIND> constexpr int kind_width = KIND == ex4d_reg::KIND_ROT ? 4 : 3;

// gradient of slice s of the tensor: row s of [rows,3], or keyframe s % K of row s / K (the whole row is read where the term needs it)
template <int KIND>
__device__ __forceinline__ void slice_grad(const float *p, int K, long long s, float c, float (&r)[kind_width<KIND>])
{
    if constexpr (KIND == KIND_STATIC) ex4d_reg::static_grad(p + 3 * s, c, r);
    else {
        const long long row = s / K;
        const int k = (int)(s - row * K);
        if constexpr (KIND == ex4d_reg::KIND_MOTION) ex4d_reg::motion_grad(p + row * K * 3, K, k, c, r);
        else ex4d_reg::rot_grad(p + row * K * 4, K, k, c, r);
    }
}

// one thread per slice: a row of _xyz_disp (KIND_STATIC, K = 1) or a (row, keyframe) of a keyframe tensor
template <int KIND>
__global__ __launch_bounds__(REG_THREADS) void reg_bwd_kernel(const float *p, float *g, long long slices, int K, float coef, const float *upstream, int accumulate)
{
    constexpr int C = kind_width<KIND>;
    const long long s = (long long)blockIdx.x * REG_THREADS + threadIdx.x;
    if (s >= slices) return;
    float r[C];
    slice_grad<KIND>(p, K, s, scaled(coef, upstream), r);
#pragma unroll
    for (int j = 0; j < C; j++) g[s * C + j] = accumulate ? g[s * C + j] + r[j] : r[j];
}

// the same over the slices s0 .. s0 + slices - 1 that overlap the flat element range [lo, hi): g[0] belongs to element lo, and of a
// slice the range cuts only the elements inside it are written
template <int KIND>
__global__ __launch_bounds__(REG_THREADS) void reg_bwd_range_kernel(const float *p, float *g, long long s0, long long slices, int K, long long lo, long long hi,
                                                                    float coef, int accumulate)
{
    constexpr int C = kind_width<KIND>;
    const long long i = (long long)blockIdx.x * REG_THREADS + threadIdx.x;
    if (i >= slices) return;
    const long long s = s0 + i;
    float r[C];
    slice_grad<KIND>(p, K, s, coef, r);
    const long long e0 = s * C;
    if (e0 >= lo && e0 + C <= hi) {      // a whole slice (all but the range's two ends): the dense kernel's stores, no test per element
        float *o = g + (e0 - lo);
#pragma unroll
        for (int j = 0; j < C; j++) o[j] = accumulate ? o[j] + r[j] : r[j];
        return;
    }
#pragma unroll
    for (int j = 0; j < C; j++) {
        const long long e = e0 + j;
        if (e >= lo && e < hi) g[e - lo] = accumulate ? g[e - lo] + r[j] : r[j];
    }
}

thread_local char g_reg_err[256] = "";

inline unsigned blocks_for(long long n) { return (unsigned)((n + REG_THREADS - 1) / REG_THREADS); }

}  // namespace

extern "C" {

const char *ex4d_reg_last_error(void) { return g_reg_err; }

size_t ex4d_reg_scratch_bytes(void) { return (size_t)REG_FWD_BLOCKS * 3 * sizeof(double); }

int ex4d_reg_forward(const float *xyz_disp, int64_t Ns, const float *xyz_motion, const float *rotation_motion, int64_t Nd, int32_t K,
                     double static_reg, double motion_reg, double rot_reg, float *out4, void *scratch, void *stream_)
{
    g_reg_err[0] = 0;
    if (Ns < 0 || Nd < 0 || K < 0 || !out4 || !scratch || ((uintptr_t)scratch & 7) || (Nd > 0 && K < 1)) {
        snprintf(g_reg_err, sizeof(g_reg_err), "ex4d_reg_forward: negative size, K < 1, null output or scratch not 8-byte aligned");
        return EX4D_ERR_ARG;
    }
    hipStream_t stream = (hipStream_t)stream_;
    if (Ns == 0) xyz_disp = nullptr;
    if (Nd == 0 || K < 2) xyz_motion = rotation_motion = nullptr;
    const double inv_s = xyz_disp ? 1.0 / (double)Ns : 0.0;
    const double inv_d = (xyz_motion || rotation_motion) ? 1.0 / ((double)Nd * (K - 1)) : 0.0;
    hipLaunchKernelGGL(reg_fwd_kernel, dim3(REG_FWD_BLOCKS), dim3(REG_THREADS), 0, stream, xyz_disp, (long long)Ns, xyz_motion, rotation_motion,
                       (long long)Nd, (int)K, (double *)scratch);
    hipLaunchKernelGGL(reg_finish_kernel, dim3(1), dim3(REG_THREADS), 0, stream, (const double *)scratch, inv_s, inv_d, static_reg, motion_reg, rot_reg, out4);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_reg_err, sizeof(g_reg_err), "launch failed: %s", hipGetErrorString(e)); return EX4D_ERR_HIP; }
    return EX4D_OK;
}

int ex4d_reg_backward(const float *xyz_disp, float *g_xyz_disp, int64_t Ns, const float *xyz_motion, float *g_xyz_motion,
                      const float *rotation_motion, float *g_rotation_motion, int64_t Nd, int32_t K,
                      double static_reg, double motion_reg, double rot_reg, const float *upstream, int32_t accumulate, void *stream_)
{
    g_reg_err[0] = 0;
    if (Ns < 0 || Nd < 0 || (Nd > 0 && K < 1) || (g_xyz_disp && Ns > 0 && !xyz_disp) || (g_xyz_motion && Nd > 0 && !xyz_motion) ||
        (g_rotation_motion && Nd > 0 && !rotation_motion)) {
        snprintf(g_reg_err, sizeof(g_reg_err), "ex4d_reg_backward: negative size, K < 1 or a gradient without its parameter");
        return EX4D_ERR_ARG;
    }
    if ((Ns + REG_THREADS) / REG_THREADS > 0x7fffffffLL || (Nd * (int64_t)K + REG_THREADS) / REG_THREADS > 0x7fffffffLL) {
        snprintf(g_reg_err, sizeof(g_reg_err), "ex4d_reg_backward: too many elements for one launch");
        return EX4D_ERR_ARG;
    }
    hipStream_t stream = (hipStream_t)stream_;
    // a term that is off or has nothing to average has coefficient 0: accumulate leaves the gradient alone, a plain write zero-fills
    const float cs = Ns > 0 ? (float)(static_reg / (double)Ns) : 0.f;
    const double pairs = (double)Nd * (K - 1);
    const float cm = pairs > 0 ? (float)(motion_reg / pairs) : 0.f, cr = pairs > 0 ? (float)(rot_reg / pairs) : 0.f;
    if (g_xyz_disp && Ns > 0 && !(accumulate && cs == 0.f))
        hipLaunchKernelGGL(reg_bwd_kernel<KIND_STATIC>, dim3(blocks_for(Ns)), dim3(REG_THREADS), 0, stream, xyz_disp, g_xyz_disp, (long long)Ns, 1, cs, upstream,
                           (int)accumulate);
    if (g_xyz_motion && Nd > 0 && !(accumulate && cm == 0.f))
        hipLaunchKernelGGL(reg_bwd_kernel<ex4d_reg::KIND_MOTION>, dim3(blocks_for(Nd * K)), dim3(REG_THREADS), 0, stream, xyz_motion, g_xyz_motion,
                           (long long)Nd * K, (int)K, cm, upstream, (int)accumulate);
    if (g_rotation_motion && Nd > 0 && !(accumulate && cr == 0.f))
        hipLaunchKernelGGL(reg_bwd_kernel<ex4d_reg::KIND_ROT>, dim3(blocks_for(Nd * K)), dim3(REG_THREADS), 0, stream, rotation_motion, g_rotation_motion,
                           (long long)Nd * K, (int)K, cr, upstream, (int)accumulate);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_reg_err, sizeof(g_reg_err), "launch failed: %s", hipGetErrorString(e)); return EX4D_ERR_HIP; }
    return EX4D_OK;
}

int ex4d_reg_backward_range(int32_t kind, const float *param, int64_t rows, int32_t K, int64_t lo, int64_t hi, float *grad, double weight,
                            int32_t accumulate, void *stream_)
{
    g_reg_err[0] = 0;
    if (kind != ex4d_reg::KIND_MOTION && kind != ex4d_reg::KIND_ROT && kind != KIND_STATIC) {
        snprintf(g_reg_err, sizeof(g_reg_err), "ex4d_reg_backward_range: unknown kind %d (1 motion_reg, 2 rot_reg, 3 static_reg)", (int)kind);
        return EX4D_ERR_ARG;
    }
    if (kind == KIND_STATIC) K = 1;
    const int C = kind == ex4d_reg::KIND_ROT ? 4 : 3;
    if (rows < 0 || (rows > 0 && (K < 1 || rows > INT64_MAX / ((int64_t)K * C)))) {
        snprintf(g_reg_err, sizeof(g_reg_err), "ex4d_reg_backward_range: negative or overflowing size, or K < 1");
        return EX4D_ERR_ARG;
    }
    const int64_t numel = rows > 0 ? rows * K * C : 0;
    if (lo < 0 || hi > numel || lo > hi) {
        snprintf(g_reg_err, sizeof(g_reg_err), "ex4d_reg_backward_range: element range [%lld, %lld) is not inside the tensor's [0, %lld)", (long long)lo,
                 (long long)hi, (long long)numel);
        return EX4D_ERR_ARG;
    }
    if (lo == hi) return EX4D_OK;
    if (!param || !grad) {
        snprintf(g_reg_err, sizeof(g_reg_err), "ex4d_reg_backward_range: null parameter or gradient");
        return EX4D_ERR_ARG;
    }
    // the coefficient of ex4d_reg_backward: 0 where the term is off or has nothing to average (accumulate: nothing to add)
    const double count = kind == KIND_STATIC ? (double)rows : (double)rows * (K - 1);
    const float coef = count > 0 ? (float)(weight / count) : 0.f;
    if (accumulate && coef == 0.f) return EX4D_OK;
    const int64_t s0 = lo / C, slices = (hi - 1) / C - s0 + 1;          // the slices the range overlaps, cut ones included
    if ((slices + REG_THREADS) / REG_THREADS > 0x7fffffffLL) {
        snprintf(g_reg_err, sizeof(g_reg_err), "ex4d_reg_backward_range: too many elements for one launch");
        return EX4D_ERR_ARG;
    }
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid(blocks_for(slices)), block(REG_THREADS);
    if (kind == KIND_STATIC)
        hipLaunchKernelGGL(reg_bwd_range_kernel<KIND_STATIC>, grid, block, 0, stream, param, grad, (long long)s0, (long long)slices, 1, (long long)lo, (long long)hi,
                           coef, (int)accumulate);
    else if (kind == ex4d_reg::KIND_MOTION)
        hipLaunchKernelGGL(reg_bwd_range_kernel<ex4d_reg::KIND_MOTION>, grid, block, 0, stream, param, grad, (long long)s0, (long long)slices, (int)K,
                           (long long)lo, (long long)hi, coef, (int)accumulate);
    else
        hipLaunchKernelGGL(reg_bwd_range_kernel<ex4d_reg::KIND_ROT>, grid, block, 0, stream, param, grad, (long long)s0, (long long)slices, (int)K,
                           (long long)lo, (long long)hi, coef, (int)accumulate);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_reg_err, sizeof(g_reg_err), "launch failed: %s", hipGetErrorString(e)); return EX4D_ERR_HIP; }
    return EX4D_OK;
}

}  // extern "C"
