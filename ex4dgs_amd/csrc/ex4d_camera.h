// The projection of a world-space point as the per-Gaussian forward does it, said once: ex4d_preprocess.hip (frustum test, pixel position)
// and ex4d_motion.hip (screen-space displacement) include this, so the pixel position and view depth of a mean carry the same bits in
// the rasterizer's geometry records and in the displacement.  Both files are compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

// column-major 4x4 (the [4,4] tensors of the reference, transposed in memory): the first three rows / all four of m * (p, 1)
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

// clip-space h = projmatrix * p, inv_w = 1 / (h.w + 1e-7f), NDC xy and p_view = viewmatrix * p (CR/auxiliary.h:267-281)
struct ProjectedPoint { float4 h; float inv_w, ndc_x, ndc_y; float3 p_view; };

__device__ __forceinline__ void project_point(float3 p, const float *vm, const float *pm, ProjectedPoint &out)
{
    out.h = xform4x4(p, pm);
    out.inv_w = 1.0f / (out.h.w + 0.0000001f);
    out.ndc_x = out.h.x * out.inv_w;
    out.ndc_y = out.h.y * out.inv_w;
    out.p_view = xform4x3(p, vm);
}

// ndc2Pix, CR/auxiliary.h:41-44: double precision, rounded to float once
__device__ __forceinline__ float ndc_to_pix(float ndc, int S) { return (float)((((double)ndc + 1.0) * (double)S - 1.0) * 0.5); }
