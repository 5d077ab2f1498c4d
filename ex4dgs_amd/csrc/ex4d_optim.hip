// Fused multi-tensor RAdam step for gfx950.
//
// torch.optim.RAdam over the reference's 15 parameter groups (scene/c_gaussian_model.py:430-449) runs ~10 element-wise
// passes per tensor: 3.2 ms per step for the 110 M parameters of a 1 M-Gaussian model on MI355X.  This is one launch that
// streams every tensor once: p, m, v read+write and g read = 28 B/element, 3.07 GB -> 0.38 ms at the 8 TB/s roofline.
// HBM-bound streaming: 16-byte loads/stores, 4096-element chunks, a chunk table in kernel arguments maps workgroups to
// tensors.  ffp-contract is off for this file: the update follows torch's op order in float32.
#include "ex4d_internal.h"
#include "ex4d_reg_rows.h"
#include "../../include/ex4d_optim.h"
#include <cmath>
#include <cstdio>

namespace {

#define RADAM_CHUNK 4096          // elements per workgroup (256 threads x 4 float4)

struct RadamSlot {
    float *p; const float *g; float *m; float *v;
    long long numel;
    float w1;          // 1 - beta1
    float beta2;
    float w2;          // 1 - beta2
    float bc1;         // 1 - beta1^t
    float lr;
    float sqrt_bc2;    // sqrt(1 - beta2^t)
    float rect;        // variance rectification, valid when rectified
    float eps;
    int rectified;     // rho_t > 5
    unsigned first_chunk;   // index of this tensor's first chunk in the launch
    int sanitize;      // gradient read through nan_to_num (train.py:244-247)
};

struct RadamArgs { RadamSlot slot[EX4D_RADAM_MAX_TENSORS]; int count; };

// torch.nan_to_num with its defaults: NaN -> 0, +inf -> FLT_MAX, -inf -> -FLT_MAX
__device__ __forceinline__ float nan_to_num(float g) { return g != g ? 0.f : fminf(fmaxf(g, -3.402823466e+38f), 3.402823466e+38f); }

__device__ __forceinline__ void radam_update(float &p, float g, float &m, float &v, const RadamSlot &s)
{
    if (s.sanitize) g = nan_to_num(g);
    m = m + s.w1 * (g - m);                       // exp_avg.lerp_(grad, 1 - beta1)
    v = v * s.beta2;                              // exp_avg_sq.mul_(beta2)
    v = v + (s.w2 * g) * g;                       //           .addcmul_(grad, grad, value=1 - beta2)
    const float mhat = m / s.bc1;
    float upd = mhat * s.lr;
    if (s.rectified) {
        const float adaptive = s.sqrt_bc2 / (sqrtf(v) + s.eps);
        upd = (upd * adaptive) * s.rect;
    }
    p = p - upd;
}

__global__ __launch_bounds__(256) void radam_kernel(const RadamArgs a)
{
    // which tensor owns this chunk (<= 32 slots, wave-uniform scan)
    int t = 0;
#pragma unroll 1
    for (int i = 1; i < a.count; i++) if (blockIdx.x >= a.slot[i].first_chunk) t = i;
    const RadamSlot &s = a.slot[t];
    const long long base = (long long)(blockIdx.x - s.first_chunk) * RADAM_CHUNK;
    const long long n = s.numel - base < RADAM_CHUNK ? s.numel - base : RADAM_CHUNK;
    float *p = s.p + base; const float *g = s.g + base; float *m = s.m + base; float *v = s.v + base;
    const bool vec = n == RADAM_CHUNK && ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
    if (vec) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int i = k * 256 + threadIdx.x;
            float4 pp = ((float4 *)p)[i], mm = ((float4 *)m)[i], vv = ((float4 *)v)[i];
            const float4 gg = ((const float4 *)g)[i];
            radam_update(pp.x, gg.x, mm.x, vv.x, s); radam_update(pp.y, gg.y, mm.y, vv.y, s);
            radam_update(pp.z, gg.z, mm.z, vv.z, s); radam_update(pp.w, gg.w, mm.w, vv.w, s);
            ((float4 *)p)[i] = pp; ((float4 *)m)[i] = mm; ((float4 *)v)[i] = vv;
        }
    } else {
        for (int i = threadIdx.x; i < n; i += 256) {
            float pp = p[i], mm = m[i], vv = v[i];
            radam_update(pp, g[i], mm, vv, s);
            p[i] = pp; m[i] = mm; v[i] = vv;
        }
    }
}

// ---- keyframe tensors with windowed gradients: one thread per (row, time slice) = C consecutive floats
struct SlicedSlot {
    RadamSlot s;             // p, m, v, coefficients (g unused)
    long long slices;        // rows * K
    int K, C, nw;
    int first[EX4D_RADAM_MAX_WINDOWS], count[EX4D_RADAM_MAX_WINDOWS];
    const float *grad[EX4D_RADAM_MAX_WINDOWS];
    const int *first_dev;    // optional: window positions in device memory (uniform loads)
    unsigned first_block;
};
struct SlicedArgs { SlicedSlot slot[EX4D_RADAM_MAX_SLICED]; int count; };

// gradient of flat element e = (row, kk, c) of a [rows, K, C] tensor from the windows (zero outside them); windows add in index order
__device__ __forceinline__ float sliced_grad(const SlicedSlot &t, const int (&first)[EX4D_RADAM_MAX_WINDOWS], long long row, int kk, int c)
{
    float g = 0.f;
    for (int w = 0; w < t.nw; w++) {
        const unsigned rel = (unsigned)(kk - first[w]);
        if (rel < (unsigned)t.count[w]) g += t.grad[w][((size_t)row * t.count[w] + rel) * t.C + c];
    }
    return g;
}

// same streaming structure as radam_kernel (4096-element chunks, 16-byte accesses to p, m, v); only the gradient differs: the few
// elements inside a window read it from the compact blocks, all others take 0 without touching memory
__global__ __launch_bounds__(256) void radam_sliced_kernel(const SlicedArgs a)
{
    int t = 0;
#pragma unroll 1
    for (int i = 1; i < a.count; i++) if (blockIdx.x >= a.slot[i].first_block) t = i;
    const SlicedSlot &s = a.slot[t];
    const long long base = (long long)(blockIdx.x - s.first_block) * RADAM_CHUNK;
    const long long n = s.s.numel - base < RADAM_CHUNK ? s.s.numel - base : RADAM_CHUNK;
    float *p = s.s.p + base, *m = s.s.m + base, *v = s.s.v + base;
    const bool vec = n == RADAM_CHUNK && ((((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
    int first[EX4D_RADAM_MAX_WINDOWS];
#pragma unroll
    for (int w = 0; w < EX4D_RADAM_MAX_WINDOWS; w++) first[w] = (s.first_dev && w < s.nw) ? s.first_dev[w] : s.first[w];
    if (vec) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int i = k * 256 + threadIdx.x;
            const long long e = base + 4 * (long long)i;
            long long sl = e / s.C;
            int c = (int)(e - sl * s.C);
            long long row = sl / s.K;
            int kk = (int)(sl - row * s.K);
            float g[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                g[j] = sliced_grad(s, first, row, kk, c);
                if (++c == s.C) { c = 0; if (++kk == s.K) { kk = 0; row++; } }
            }
            float4 pp = ((float4 *)p)[i], mm = ((float4 *)m)[i], vv = ((float4 *)v)[i];
            radam_update(pp.x, g[0], mm.x, vv.x, s.s); radam_update(pp.y, g[1], mm.y, vv.y, s.s);
            radam_update(pp.z, g[2], mm.z, vv.z, s.s); radam_update(pp.w, g[3], mm.w, vv.w, s.s);
            ((float4 *)p)[i] = pp; ((float4 *)m)[i] = mm; ((float4 *)v)[i] = vv;
        }
    } else {
        for (int i = threadIdx.x; i < n; i += 256) {
            const long long e = base + i;
            const long long sl = e / s.C, row = sl / s.K;
            float pp = p[i], mm = m[i], vv = v[i];
            radam_update(pp, sliced_grad(s, first, row, (int)(sl - row * s.K), (int)(e - sl * s.C)), mm, vv, s.s);
            p[i] = pp; m[i] = mm; v[i] = vv;
        }
    }
}

// ---- keyframe tensors with windowed gradients PLUS a motion regulariser formed from the row itself (train.py:159-168)
// motion_reg / rot_reg make the gradient dense over all K keyframes, but it is a function of the Gaussian's own row: keyframe k needs
// the PRE-update keyframe 0 (motion) or k-1, k+1 (rotation).  So a workgroup owns whole rows -- a block of R rows = one contiguous span
// of R K C floats (R a multiple of 4: 16-byte aligned for odd K C) -- stages p in LDS with 16-byte loads, forms the regulariser gradient
// of every slice from the LDS copy into a second LDS array, then streams p (from LDS), m, v with 16-byte accesses like the kernels
// above: 24 B per element plus the windows, the dense gradient never exists in memory.
#define REG_LDS_BYTES 32768       // p copy + regulariser gradient of one block of rows: five workgroups per CU
struct RegSlot {
    SlicedSlot t;            // first_block: this tensor's first workgroup
    long long rows;
    int kind;                // ex4d_reg::KIND_*
    int R;                   // rows per workgroup
    float coef;              // weight / (Nd (K-1))
};
struct RegArgs { RegSlot slot[EX4D_RADAM_MAX_SLICED]; int count; };

static int reg_block_rows(int K, int C)
{
    const long long per_row = 2LL * K * C * (long long)sizeof(float);
    long long R = REG_LDS_BYTES / per_row;
    R = R > 32 ? 32 : R & ~3LL;
    return (int)R;           // 0: four rows do not fit
}

__global__ __launch_bounds__(256) void radam_sliced_reg_kernel(const RegArgs a)
{
    extern __shared__ float4 lds4[];
    int ti = 0;
#pragma unroll 1
    for (int i = 1; i < a.count; i++) if (blockIdx.x >= a.slot[i].t.first_block) ti = i;
    const RegSlot &rs = a.slot[ti];
    const SlicedSlot &s = rs.t;
    const int K = s.K, C = s.C, KC = K * C;
    const long long row0 = (long long)(blockIdx.x - s.first_block) * rs.R;
    const int nrows = (int)(rs.rows - row0 < rs.R ? rs.rows - row0 : rs.R);
    const int n = nrows * KC;                              // floats of this workgroup's span (<= R K C <= REG_LDS_BYTES / 8)
    const long long base = row0 * KC;
    float *p = s.s.p + base, *m = s.s.m + base, *v = s.s.v + base;
    float *P = (float *)lds4, *G = P + rs.R * KC;          // R K C is a multiple of 4: G stays 16-byte aligned
    const bool vec = (n & 3) == 0 && ((((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
    const bool reg = rs.kind != ex4d_reg::KIND_NONE;
    int first[EX4D_RADAM_MAX_WINDOWS];
#pragma unroll
    for (int w = 0; w < EX4D_RADAM_MAX_WINDOWS; w++) first[w] = (s.first_dev && w < s.nw) ? s.first_dev[w] : s.first[w];

    if (vec) for (int i = threadIdx.x; i < n / 4; i += 256) ((float4 *)P)[i] = ((const float4 *)p)[i];
    else for (int i = threadIdx.x; i < n; i += 256) P[i] = p[i];
    __syncthreads();
    if (reg) {
        // one thread per (row, keyframe) slice: odd stride 3 (conflict-free) or one 16-byte LDS access per keyframe
        const int slices = nrows * K;
        if (rs.kind == ex4d_reg::KIND_MOTION) {
            for (int sl = threadIdx.x; sl < slices; sl += 256) {
                const int r = sl / K, k = sl - r * K;
                if (k == 0) continue;
                float g[3];
                ex4d_reg::motion_grad(P + r * KC, K, k, rs.coef, g);
                G[sl * 3] = g[0]; G[sl * 3 + 1] = g[1]; G[sl * 3 + 2] = g[2];
            }
            __syncthreads();
            // keyframe 0: the sum of the K-1 unit vectors (= minus the entries just written) in ascending k, the order of motion_grad
            for (int r = threadIdx.x; r < nrows; r += 256) {
                float *g = G + r * KC;
                float x = 0.f, y = 0.f, z = 0.f;
                for (int k = 1; k < K; k++) { x += -g[3 * k]; y += -g[3 * k + 1]; z += -g[3 * k + 2]; }
                g[0] = x; g[1] = y; g[2] = z;
            }
        } else {
            for (int sl = threadIdx.x; sl < slices; sl += 256) {
                const int r = sl / K, k = sl - r * K;
                float g[4];
                ex4d_reg::rot_grad(P + r * KC, K, k, rs.coef, g);
                ((float4 *)G)[sl] = make_float4(g[0], g[1], g[2], g[3]);
            }
        }
        __syncthreads();
    }
    if (vec) {
        for (int i = threadIdx.x; i < n / 4; i += 256) {
            const int e = 4 * i;
            int sl = e / C;
            int c = e - sl * C;
            int r = sl / K;
            int kk = sl - r * K;
            float g[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                g[j] = sliced_grad(s, first, row0 + r, kk, c);
                if (++c == C) { c = 0; if (++kk == K) { kk = 0; r++; } }
            }
            if (reg) { const float4 gg = ((const float4 *)G)[i]; g[0] += gg.x; g[1] += gg.y; g[2] += gg.z; g[3] += gg.w; }
            float4 pp = ((const float4 *)P)[i], mm = ((float4 *)m)[i], vv = ((float4 *)v)[i];
            radam_update(pp.x, g[0], mm.x, vv.x, s.s); radam_update(pp.y, g[1], mm.y, vv.y, s.s);
            radam_update(pp.z, g[2], mm.z, vv.z, s.s); radam_update(pp.w, g[3], mm.w, vv.w, s.s);
            ((float4 *)p)[i] = pp; ((float4 *)m)[i] = mm; ((float4 *)v)[i] = vv;
        }
    } else {
        for (int i = threadIdx.x; i < n; i += 256) {
            const int sl = i / C, r = sl / K;
            float g = sliced_grad(s, first, row0 + r, sl - r * K, i - sl * C);
            if (reg) g += G[i];
            float pp = P[i], mm = m[i], vv = v[i];
            radam_update(pp, g, mm, vv, s.s);
            p[i] = pp; m[i] = mm; v[i] = vv;
        }
    }
}

thread_local char g_optim_err[256] = "";

static void fill_coefficients(RadamSlot &s, double lr, long long step, double beta1, double beta2, double eps)
{
    // the Python-double scalar arithmetic of torch's RAdam, cast to float32 where it meets a tensor
    const double rho_inf = 2.0 / (1.0 - beta2) - 1.0;
    const double st = (double)step;
    const double bc1 = 1.0 - std::pow(beta1, st), bc2 = 1.0 - std::pow(beta2, st);
    const double rho_t = rho_inf - 2.0 * st * std::pow(beta2, st) / bc2;
    s.w1 = (float)(1.0 - beta1); s.beta2 = (float)beta2; s.w2 = (float)(1.0 - beta2);
    s.bc1 = (float)bc1; s.lr = (float)lr; s.sqrt_bc2 = (float)std::sqrt(bc2); s.eps = (float)eps;
    s.rectified = rho_t > 5.0;
    s.rect = s.rectified ? (float)std::sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t)) : 0.f;
}

// ---- what the three entry points share.  The bool helpers leave the fault's text in g_optim_err and return false.
static bool count_fits(int32_t count, int max, const void *tensors)
{
    if (count >= 0 && count <= max && (count == 0 || tensors)) return true;
    snprintf(g_optim_err, sizeof(g_optim_err), "count %d outside [0, %d]", count, max);
    return false;
}

// validates descriptor i and fills its slot, all but first_block: how many workgroups a tensor takes is the entry point's business
static bool fill_sliced(SlicedSlot &s, const Ex4dRadamSlicedTensor &t, int i, double beta1, double beta2, double eps)
{
    if (t.rows < 0 || t.K < 1 || (t.C != 3 && t.C != 4) || t.step < 1 || !t.param || !t.exp_avg || !t.exp_avg_sq ||
        t.n_windows < 0 || t.n_windows > EX4D_RADAM_MAX_WINDOWS) {
        snprintf(g_optim_err, sizeof(g_optim_err), "sliced tensor %d: bad shape, step < 1, null pointer or too many windows", i);
        return false;
    }
    s.s.p = t.param; s.s.g = nullptr; s.s.m = t.exp_avg; s.s.v = t.exp_avg_sq; s.s.numel = t.rows * t.K * t.C; s.s.first_chunk = 0; s.s.sanitize = 0;
    s.first_dev = t.first_dev;
    fill_coefficients(s.s, t.lr, t.step, beta1, beta2, eps);
    s.slices = t.rows * t.K; s.K = t.K; s.C = t.C; s.nw = t.n_windows;
    for (int w = 0; w < EX4D_RADAM_MAX_WINDOWS; w++) {
        const bool live = w < t.n_windows;
        if (live && (((t.first[w] < 0 || t.first[w] + t.count[w] > t.K) && !t.first_dev) || t.count[w] < 1 || t.count[w] > t.K || !t.grad[w])) {
            snprintf(g_optim_err, sizeof(g_optim_err), "sliced tensor %d: window %d outside [0, K) or null", i, w);
            return false;
        }
        s.first[w] = live ? t.first[w] : 0; s.count[w] = live ? t.count[w] : 0; s.grad[w] = live ? t.grad[w] : nullptr;
    }
    return true;
}

// appends a tensor's nb workgroups to the launch: `first` = the index of its first one
static bool append_blocks(unsigned &blocks, unsigned &first, long long nb)
{
    first = blocks;
    if (nb + blocks > 0x7fffffffLL) { snprintf(g_optim_err, sizeof(g_optim_err), "too many elements for one launch"); return false; }
    blocks += (unsigned)nb;
    return true;
}

template <class Args>
static int launch(void (*kernel)(Args), unsigned blocks, size_t lds, void *stream, const Args &a)
{
    if (blocks == 0) return EX4D_OK;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), lds, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_optim_err, sizeof(g_optim_err), "launch failed: %s", hipGetErrorString(e)); return EX4D_ERR_HIP; }
    return EX4D_OK;
}

}  // namespace

extern "C" {

const char *ex4d_optim_last_error(void) { return g_optim_err; }

int ex4d_radam_step(const Ex4dRadamTensor *tensors, int32_t count, double beta1, double beta2, double eps, void *stream_)
{
    g_optim_err[0] = 0;
    if (!count_fits(count, EX4D_RADAM_MAX_TENSORS, tensors)) return EX4D_ERR_ARG;
    RadamArgs a;
    a.count = 0;
    unsigned chunks = 0;
    for (int i = 0; i < count; i++) {
        const Ex4dRadamTensor &t = tensors[i];
        if (t.numel == 0) continue;
        if (t.numel < 0 || t.step < 1 || !t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq) {
            snprintf(g_optim_err, sizeof(g_optim_err), "tensor %d: null pointer, negative size or step < 1", i);
            return EX4D_ERR_ARG;
        }
        RadamSlot &s = a.slot[a.count++];
        s.p = t.param; s.g = t.grad; s.m = t.exp_avg; s.v = t.exp_avg_sq; s.numel = t.numel; s.sanitize = t.nan_to_num != 0;
        fill_coefficients(s, t.lr, t.step, beta1, beta2, eps);
        if (!append_blocks(chunks, s.first_chunk, (t.numel + RADAM_CHUNK - 1) / RADAM_CHUNK)) return EX4D_ERR_ARG;
    }
    return launch(radam_kernel, chunks, 0, stream_, a);
}

int ex4d_radam_step_sliced(const Ex4dRadamSlicedTensor *tensors, int32_t count, double beta1, double beta2, double eps, void *stream_)
{
    g_optim_err[0] = 0;
    if (!count_fits(count, EX4D_RADAM_MAX_SLICED, tensors)) return EX4D_ERR_ARG;
    SlicedArgs a;
    a.count = 0;
    unsigned blocks = 0;
    for (int i = 0; i < count; i++) {
        if (tensors[i].rows == 0) continue;
        SlicedSlot &s = a.slot[a.count];
        if (!fill_sliced(s, tensors[i], i, beta1, beta2, eps) ||
            !append_blocks(blocks, s.first_block, (s.s.numel + RADAM_CHUNK - 1) / RADAM_CHUNK)) return EX4D_ERR_ARG;
        a.count++;
    }
    return launch(radam_sliced_kernel, blocks, 0, stream_, a);
}

int32_t ex4d_radam_sliced_reg_rows(int32_t K, int32_t C)
{
    if (K < 1 || (C != 3 && C != 4)) return 0;
    return reg_block_rows(K, C);
}

int ex4d_radam_step_sliced_reg(const Ex4dRadamSlicedRegTensor *tensors, int32_t count, double beta1, double beta2, double eps, void *stream_)
{
    g_optim_err[0] = 0;
    if (!count_fits(count, EX4D_RADAM_MAX_SLICED, tensors)) return EX4D_ERR_ARG;
    RegArgs a;
    a.count = 0;
    unsigned blocks = 0;
    size_t lds = 0;
    for (int i = 0; i < count; i++) {
        const Ex4dRadamSlicedTensor &t = tensors[i].t;
        const int kind = tensors[i].reg_kind;
        if (t.rows == 0) continue;
        RegSlot &r = a.slot[a.count];
        if (!fill_sliced(r.t, t, i, beta1, beta2, eps)) return EX4D_ERR_ARG;
        if (kind < 0 || kind > 2 || (kind == ex4d_reg::KIND_MOTION && t.C != 3) || (kind == ex4d_reg::KIND_ROT && t.C != 4) ||
            (kind != 0 && tensors[i].reg_rows < t.rows)) {
            snprintf(g_optim_err, sizeof(g_optim_err), "sliced tensor %d: reg_kind %d does not fit C = %d, or reg_rows < rows", i, kind, t.C);
            return EX4D_ERR_ARG;
        }
        r.R = reg_block_rows(t.K, t.C);
        if (r.R < 4) {
            snprintf(g_optim_err, sizeof(g_optim_err), "sliced tensor %d: four rows of K = %d keyframes do not fit the %d bytes of LDS a workgroup stages "
                     "(dense gradients + ex4d_reg_backward + ex4d_radam_step take any K)", i, t.K, REG_LDS_BYTES);
            return EX4D_ERR_ARG;
        }
        // the mean's constant on the host in double; a term with nothing to average (K = 1) or weight 0 is a plain sliced step
        const double pairs = (double)tensors[i].reg_rows * (t.K - 1);
        r.coef = (kind != 0 && pairs > 0) ? (float)(tensors[i].reg_weight / pairs) : 0.f;
        r.kind = r.coef != 0.f ? kind : ex4d_reg::KIND_NONE;
        r.rows = t.rows;
        if (!append_blocks(blocks, r.t.first_block, (t.rows + r.R - 1) / r.R)) return EX4D_ERR_ARG;
        const size_t need = 2 * (size_t)r.R * t.K * t.C * sizeof(float);
        lds = need > lds ? need : lds;
        a.count++;
    }
    return launch(radam_sliced_reg_kernel, blocks, lds, stream_, a);
}

}  // extern "C"
