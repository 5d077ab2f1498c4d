// The motion regularisers of train.py:155-168 as a stand-alone op (include/ex4d_regularizers.h): loss value and dense gradients.
// The per-iteration hot path is the regularised sliced RAdam step (ex4d_optim.hip), which never materialises these gradients; this
// file serves autograd users, the dense-gradient trainer paths, the _xyz_disp term and the reported loss value.
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

__global__ __launch_bounds__(REG_THREADS) void reg_bwd_static_kernel(const float *disp, float *g, long long Ns, float coef, const float *upstream, int accumulate)
{
    const long long i = (long long)blockIdx.x * REG_THREADS + threadIdx.x;
    if (i >= Ns) return;
    float r[3];
    ex4d_reg::static_grad(disp + 3 * i, scaled(coef, upstream), r);
#pragma unroll
    for (int j = 0; j < 3; j++) g[3 * i + j] = accumulate ? g[3 * i + j] + r[j] : r[j];
}

// one thread per (row, keyframe) slice; kind: ex4d_reg::KIND_MOTION ([Nd,K,3]) or KIND_ROT ([Nd,K,4])
template <int KIND>
__global__ __launch_bounds__(REG_THREADS) void reg_bwd_keyframe_kernel(const float *p, float *g, long long Nd, int K, float coef, const float *upstream,
                                                                       int accumulate)
{
    constexpr int C = KIND == ex4d_reg::KIND_MOTION ? 3 : 4;
    const long long s = (long long)blockIdx.x * REG_THREADS + threadIdx.x;
    if (s >= Nd * K) return;
    const long long row = s / K;
    const int k = (int)(s - row * K);
    float r[C];
    const float c = scaled(coef, upstream);
    if constexpr (KIND == ex4d_reg::KIND_MOTION) ex4d_reg::motion_grad(p + row * K * C, K, k, c, r);
    else ex4d_reg::rot_grad(p + row * K * C, K, k, c, r);
#pragma unroll
    for (int j = 0; j < C; j++) g[s * C + j] = accumulate ? g[s * C + j] + r[j] : r[j];
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
        hipLaunchKernelGGL(reg_bwd_static_kernel, dim3(blocks_for(Ns)), dim3(REG_THREADS), 0, stream, xyz_disp, g_xyz_disp, (long long)Ns, cs, upstream, (int)accumulate);
    if (g_xyz_motion && Nd > 0 && !(accumulate && cm == 0.f))
        hipLaunchKernelGGL(reg_bwd_keyframe_kernel<ex4d_reg::KIND_MOTION>, dim3(blocks_for(Nd * K)), dim3(REG_THREADS), 0, stream, xyz_motion, g_xyz_motion,
                           (long long)Nd, (int)K, cm, upstream, (int)accumulate);
    if (g_rotation_motion && Nd > 0 && !(accumulate && cr == 0.f))
        hipLaunchKernelGGL(reg_bwd_keyframe_kernel<ex4d_reg::KIND_ROT>, dim3(blocks_for(Nd * K)), dim3(REG_THREADS), 0, stream, rotation_motion, g_rotation_motion,
                           (long long)Nd, (int)K, cr, upstream, (int)accumulate);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_reg_err, sizeof(g_reg_err), "launch failed: %s", hipGetErrorString(e)); return EX4D_ERR_HIP; }
    return EX4D_OK;
}

}  // extern "C"
