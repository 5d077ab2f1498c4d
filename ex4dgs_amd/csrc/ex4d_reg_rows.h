// Per-row float32 arithmetic of the motion regularisers' gradients (include/ex4d_regularizers.h), shared by the stand-alone dense
// backward (ex4d_regularizers.hip) and the regularised sliced RAdam step (ex4d_optim.hip): both must give identical bits, so both
// translation units are built with -ffp-contract=off and every sum here has one fixed order.
//   coef = weight / count, computed on the host in double, cast to float32 (times the upstream scalar in float32 where there is one).
#pragma once
#include <hip/hip_runtime.h>

namespace ex4d_reg {

enum { KIND_NONE = 0, KIND_MOTION = 1, KIND_ROT = 2 };

// static_reg: d/dd coef * log(|d| + 0.001) = d * coef / (|d| + 0.001) / |d|, 0 where |d| = 0
__device__ __forceinline__ void static_grad(const float *d, float coef, float (&g)[3])
{
    const float n = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const float s = n == 0.f ? 0.f : (coef / (n + 0.001f)) / n;
    g[0] = d[0] * s; g[1] = d[1] * s; g[2] = d[2] * s;
}

// motion_reg, the term of keyframe k >= 1: u = coef * (p0 - pk) / |p0 - pk| (0 where the two coincide).
// dL/dpk = -u,  dL/dp0 = sum of u over k = 1 .. K-1 in ascending k.
__device__ __forceinline__ void motion_unit(const float *p0, const float *pk, float coef, float (&u)[3])
{
    const float dx = p0[0] - pk[0], dy = p0[1] - pk[1], dz = p0[2] - pk[2];
    const float n = sqrtf(dx * dx + dy * dy + dz * dz);
    const float s = n == 0.f ? 0.f : coef / n;
    u[0] = dx * s; u[1] = dy * s; u[2] = dz * s;
}

// gradient of keyframe k of one row [K,3]
__device__ __forceinline__ void motion_grad(const float *row, int K, int k, float coef, float (&g)[3])
{
    float u[3];
    if (k > 0) {
        motion_unit(row, row + 3 * k, coef, u);
        g[0] = -u[0]; g[1] = -u[1]; g[2] = -u[2];
        return;
    }
    g[0] = g[1] = g[2] = 0.f;
    for (int kk = 1; kk < K; kk++) {
        motion_unit(row, row + 3 * kk, coef, u);
        g[0] += u[0]; g[1] += u[1]; g[2] += u[2];
    }
}

// rot_reg, one pair (a, b) of neighbouring keyframes: g += d/da of -coef <a,b> / max(|a|,1e-6) / max(|b|,1e-6)
//   = -b coef/(ca cb)  +  [|a| >= 1e-6] a <a,b> coef/(ca^2 cb |a|)
__device__ __forceinline__ void rot_pair_add(const float *a, const float *b, float coef, float (&g)[4])
{
    const float na = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3]);
    const float nb = sqrtf(b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + b[3] * b[3]);
    const float ca = fmaxf(na, 1e-6f), cb = fmaxf(nb, 1e-6f);
    const float dot = a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
    const float inv = (coef / ca) / cb;
    const float t = na >= 1e-6f ? ((dot * inv) / ca) / na : 0.f;
#pragma unroll
    for (int j = 0; j < 4; j++) g[j] += a[j] * t - b[j] * inv;
}

// gradient of keyframe k of one row [K,4]: the pair with k-1 first, then the pair with k+1
__device__ __forceinline__ void rot_grad(const float *row, int K, int k, float coef, float (&g)[4])
{
    g[0] = g[1] = g[2] = g[3] = 0.f;
    if (k > 0) rot_pair_add(row + 4 * k, row + 4 * (k - 1), coef, g);
    if (k + 1 < K) rot_pair_add(row + 4 * k, row + 4 * (k + 1), coef, g);
}

}  // namespace ex4d_reg
