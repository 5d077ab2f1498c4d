// A streaming pass over the flat pixels of a frame with a deterministic reduction, said once: the device half of the per-pixel losses
// (ex4d_flow.hip, ex4d_depth.hip).
//
// TILING.  Pixels are p = y W + x over contiguous planes, so rows do not matter.  A lane owns PS_PPL = 4 consecutive pixels from
// first_pixel() (a multiple of 4), pixels_from(p0, HW) of them inside the frame: 4, fewer in the frame's last, partial lane, 0 beyond.
// A workgroup of PS_THREADS = 256 lanes owns PS_WG_PIXELS = 1024, a frame takes blocks_of(HW) workgroups.
//
// PLANE ACCESS.  load4 / store4 move a lane's pixels of a float plane as one 16-byte vector where the lane is whole and its first
// element is 16-byte aligned -- the same answer for every whole lane of a plane, since p0 is a multiple of 4: a plane at a 4-byte
// offset of an allocation, or the second plane of a frame whose H W is no multiple of 4, goes by single floats, as does the partial
// lane.  load4 fills the pixels beyond the frame with `fill`; store4 writes nothing there.
//
// REDUCTION.  The order of every addition is part of the contract: the tests compare bits between calls, and a forward's row feeds its
// backward.
//   wave_sum       within a wave the xor tree 32, 16, ..., 1: every lane ends with the wave's sum
//   workgroup_row  wave_sum, lane 0 of each wave to LDS, then s[0] + s[1] + s[2] + s[3]; thread q < N writes rows[N block + q].  V is
//                  what the kernel accumulates in: float (flow) or double (depth)
//   fold_rows      ONE WAVE (a launch of PS_FOLD = 64 threads) adds the workgroups' rows in double: lane i takes workgroups
//                  i, i + 64, ... in order, then wave_sum.  Src is the rows' type
// No atomics: equal inputs give equal bits.
//
// A NEW LOSS supplies its own loads of the ground truth, its per-pixel arithmetic into V sums[N] (pixels outside its mask SELECTED out,
// never multiplied by zero), a one-wave finish kernel that calls fold_rows and writes the loss and its row, and a backward that reads
// what it needs from that row on the device.  Its pass kernel is  p0 = first_pixel(); n = pixels_from(p0, HW); if (n > 0) { load4 ...;
// sums[q] += ... }  workgroup_row(sums, rows);  -- every thread of the workgroup reaches workgroup_row.  Scratch is N values of V per
// workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <cmath>
#include <cstdio>
#include "../../include/ex4d_loss.h"

#define PS_PPL 4
#define PS_THREADS 256
#define PS_FOLD 64
#define PS_WG_PIXELS (PS_PPL * PS_THREADS)
static_assert(PS_PPL == 4, "a lane's pixels are one float4 per plane");
static_assert(PS_THREADS == 4 * 64 && PS_FOLD == 64, "four waves per workgroup; the fold is one wave");
// the tiling the public header publishes per loss is this one
static_assert(EX4D_FLOW_PIXELS_PER_LANE == PS_PPL && EX4D_FLOW_THREADS == PS_THREADS && EX4D_FLOW_FOLD == PS_FOLD, "flow loss tiling");
static_assert(EX4D_DEPTH_PIXELS_PER_LANE == PS_PPL && EX4D_DEPTH_THREADS == PS_THREADS && EX4D_DEPTH_FOLD == PS_FOLD, "depth loss tiling");

namespace {

// ---- host: what the forward and the backward of a per-pixel loss refuse before any launch, in this order; NULL where the arguments
// are fine.  `loss` names the loss ("flow loss"), `macros` the prefix of its kind constants ("EX4D_FLOW"), `first` its rendered plane.
// The loss's own findings come in as texts in buffers of its own, NULL where it has none: `own` is reported after the image size,
// `late` between eps and the NULL pointers.
inline long long blocks_of(long long HW) { return (HW + PS_WG_PIXELS - 1) / PS_WG_PIXELS; }
static_assert(EX4D_FLOW_L1 == 0 && EX4D_FLOW_CHARBONNIER == 1 && EX4D_DEPTH_L1 == 0 && EX4D_DEPTH_CHARBONNIER == 1, "kind: L1 0, Charbonnier 1");

inline const char *pixel_loss_refusal(const char *loss, const char *macros, int H, int W, const char *own, int kind, float eps,
                                      const char *late, const char *first_name, const void *first, const void *gt)
{
    static char text[160];
    if (H <= 0 || W <= 0) { snprintf(text, sizeof(text), "%s: image %d x %d: H and W must be positive", loss, H, W); return text; }
    if (blocks_of((long long)H * W) > 0x7fffffffLL) { snprintf(text, sizeof(text), "%s: image %d x %d: too many pixels for one launch", loss, H, W); return text; }
    if (own) return own;
    if (kind != 0 && kind != 1) { snprintf(text, sizeof(text), "%s: kind %d: %s_L1 (0) or %s_CHARBONNIER (1)", loss, kind, macros, macros); return text; }
    if (kind == 1 && !(eps > 0.f && std::isfinite(eps))) { snprintf(text, sizeof(text), "%s: eps %g: Charbonnier needs a finite eps > 0", loss, (double)eps); return text; }
    if (late) return late;
    if (!first) { snprintf(text, sizeof(text), "%s: %s is NULL", loss, first_name); return text; }
    if (!gt) { snprintf(text, sizeof(text), "%s: gt is NULL", loss); return text; }
    return nullptr;
}

// ---- device: tiling
__device__ __forceinline__ long long first_pixel() { return ((long long)blockIdx.x * PS_THREADS + threadIdx.x) * PS_PPL; }
__device__ __forceinline__ int pixels_from(long long p0, long long HW) { return p0 >= HW ? 0 : (HW - p0 < PS_PPL ? (int)(HW - p0) : PS_PPL); }

// ---- a lane's n <= 4 consecutive elements of a float plane, from element p0 (a multiple of 4)
__device__ __forceinline__ void load4(const float *__restrict__ plane, long long p0, int n, float (&o)[PS_PPL], float fill)
{
    const float *q = plane + p0;
    if (n == PS_PPL && ((uintptr_t)q & 15) == 0) {
        const float4 t = *reinterpret_cast<const float4 *>(q);
        o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < PS_PPL; j++) o[j] = j < n ? q[j] : fill;
    }
}

__device__ __forceinline__ void store4(float *__restrict__ plane, long long p0, int n, const float (&v)[PS_PPL])
{
    float *q = plane + p0;
    if (n == PS_PPL && ((uintptr_t)q & 15) == 0) {
        *reinterpret_cast<float4 *>(q) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < PS_PPL; j++)
            if (j < n) q[j] = v[j];
    }
}

__device__ __forceinline__ bool finite(float x) { return fabsf(x) <= 3.402823466e+38f; }

// ---- N sums over the workgroup's 256 threads into one row of partials, then over the workgroups' rows (REDUCTION above)
template <typename V, int N>
__device__ __forceinline__ void wave_sum(V (&v)[N])
{
#pragma unroll
    for (int q = 0; q < N; q++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_xor(v[q], o, 64);
    }
}

template <typename V, int N>
__device__ __forceinline__ void workgroup_row(V (&sums)[N], V *__restrict__ rows)
{
    __shared__ V s[N][PS_THREADS / 64];
    wave_sum(sums);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < N; q++) s[q][wave] = sums[q];
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const int q = threadIdx.x;
        rows[N * (size_t)blockIdx.x + q] = s[q][0] + s[q][1] + s[q][2] + s[q][3];
    }
}

template <typename Src, int N>
__device__ __forceinline__ void fold_rows(int nblocks, const Src *__restrict__ rows, double (&sum)[N])
{
#pragma unroll
    for (int q = 0; q < N; q++) sum[q] = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += PS_FOLD) {
#pragma unroll
        for (int q = 0; q < N; q++) sum[q] += (double)rows[N * (size_t)i + q];
    }
    wave_sum(sum);
}

}  // namespace
