// Adaptive density control for gfx950 (include/ex4d_densify.h): the per-iteration statistics, the clone / split / prune
// classification with its scan, and the multi-tensor gather that builds every new tensor in one pass.
//
// The reference composes these steps from ~40 small torch ops per iteration (train.py:199-216) and, per densify call, three
// copies of all 15 parameters and both RAdam moments with boolean-mask indexing (a nonzero + host sync each).  Here:
//   densify_stats   one thread per row, ~100 B per Gaussian, no atomics, no host sync (capturable in a graph)
//   stats_merge     several ranks: the all-gathered pending blocks folded into the total in rank order, one streaming launch per group
//   densify_plan    classify (flag byte per row + packed block sums) -> scan of the block sums -> per-row destination map
//   densify_apply   every source element read once, every destination element written once, descriptors in kernel arguments
// ffp-contract is off for this file: the threshold decisions and the copied / transformed values follow torch's float32 op order.
#include "ex4d_internal.h"
#include "../../include/ex4d_densify.h"
#include <cstdio>

namespace {

#define DN_THREADS 256
#define DN_APPLY_CHUNK 4096                 // elements per workgroup of the gather (16 per thread)
#define DN_FIELD_BITS 9                     // packed per-block counters: 7 fields of 9 bits (a block counts at most 256 per field)
#define DN_FIELDS 7

enum { F_KEEP = 1, F_CLONE = 2, F_KEEP_CLONE = 4, F_SPLIT = 8, F_SPLIT_CLONE = 16, F_KEEP_CHILD = 32, F_KEEP_CHILD_CLONE = 64 };

thread_local char g_densify_err[256] = "";

// ---------------------------------------------------------------------------------------------------------------- statistics
__global__ __launch_bounds__(DN_THREADS) void densify_stats_kernel(float *__restrict__ st, long long n, long long row0,
                                                                    const int *__restrict__ radii, const float *__restrict__ vg,
                                                                    const float *__restrict__ eg, float timestamp, int flags)
{
    const long long i = (long long)blockIdx.x * DN_THREADS + threadIdx.x;
    if (i >= n) return;
    const long long r = row0 + i;
    const float rad = (float)radii[r];              // int32 radii meet float32 state: torch promotes the comparison to float
    float e0 = 0.f, e1 = 0.f, e2 = 0.f;
    if (eg) { e0 = eg[3 * r]; e1 = eg[3 * r + 1]; e2 = eg[3 * r + 2]; }
    if ((flags & EX4D_DENSIFY_PRUNE_STATS) && e0 > 0.f) {                         // mark_prune_stats (:1105): filter e0 > 0
        const float m = st[EX4D_STAT_MIN_RADII * n + i];
        st[EX4D_STAT_MIN_RADII * n + i] = rad < m ? rad : m;
    }
    if (!(flags & EX4D_DENSIFY_GRAD_STATS) || !(radii[r] > 0)) return;           // train.py:203-210: filter radii > 0
    const float m = st[EX4D_STAT_MAX_RADII * n + i];
    st[EX4D_STAT_MAX_RADII * n + i] = rad > m ? rad : m;
    const float gx = vg[3 * r], gy = vg[3 * r + 1];
    st[EX4D_STAT_GRAD_ACCUM * n + i] = st[EX4D_STAT_GRAD_ACCUM * n + i] + sqrtf(gx * gx + gy * gy);     // add_densification_stats (:1095)
    st[EX4D_STAT_DENOM * n + i] = st[EX4D_STAT_DENOM * n + i] + 1.f;
    if (!(flags & EX4D_DENSIFY_L1_STATS)) return;
    const float d = e0 < 1e-4f ? 1e-4f : e0;                                     // clamp_min(1e-4): NaN stays NaN
    const float l1 = e1 / d;                                                      // add_l1_ssim_stats (:1119)
    const float old_min = st[EX4D_STAT_ERROR_MIN * n + i];
    if (old_min > l1 && e0 > 0.01f) {                                             // both writes test the OLD minimum
        st[EX4D_STAT_ERROR_MIN_T * n + i] = timestamp;
        st[EX4D_STAT_ERROR_MIN * n + i] = l1;
    }
    st[EX4D_STAT_ERROR_ACCUM * n + i] = st[EX4D_STAT_ERROR_ACCUM * n + i] + l1;
    st[EX4D_STAT_SSIM_ACCUM * n + i] = st[EX4D_STAT_SSIM_ACCUM * n + i] + e2 / d;
    st[EX4D_STAT_ERROR_DENOM * n + i] = st[EX4D_STAT_ERROR_DENOM * n + i] + (e0 > 0.f ? 1.f : 0.f);
}

// ---------------------------------------------------------------------------------------------------------------- merge over ranks
#define DN_MERGE_COLS 4                     // Gaussians per thread and trip: one 16-byte access per statistic row
#define DN_MERGE_CHUNK (DN_THREADS * DN_MERGE_COLS)    // Gaussians per workgroup and trip
#define DN_MERGE_MAX_BLOCKS 1024            // 4 waves per SIMD on 256 compute units (the kernel holds two blocks of 36 values per lane); the rest is the grid-stride loop

typedef float merge_f4 __attribute__((ext_vector_type(4)));

// A row of a [9, n] block starts at r n floats: 16-byte aligned for every row only when n % 4 == 0, and the rows of the W + 1 blocks of
// one call have W + 1 different phases otherwise -- no head / body split aligns them all.  The 16-byte accesses are therefore made at
// float alignment: global memory on gfx950 takes unaligned wide accesses and the compiler emits global_load_dwordx4 /
// global_store_dwordx4 for a 4-byte-aligned 16-byte copy (the same machine code as for an aligned one); a wave whose rows are off phase
// touches 9 cache lines instead of 8.
__device__ __forceinline__ merge_f4 merge_load(const float *p)
{
    merge_f4 v;
    __builtin_memcpy(&v, p, sizeof(v));
    return v;
}
__device__ __forceinline__ void merge_store(float *p, merge_f4 v) { __builtin_memcpy(p, &v, sizeof(v)); }

__device__ __forceinline__ float stat_init(int r)
{
    return r < EX4D_STAT_MIN_RADII ? 0.f : (r == EX4D_STAT_ERROR_MIN_T ? -1.f : 1000.f);
}

// one Gaussian: the total's nine values t take a rank's nine pending values d (the table of ex4d_densify_stats_merge in the header)
__device__ __forceinline__ void merge_fold(float (&t)[EX4D_DENSIFY_STATS], const float (&d)[EX4D_DENSIFY_STATS])
{
#pragma unroll
    for (int r = EX4D_STAT_GRAD_ACCUM; r <= EX4D_STAT_ERROR_DENOM; r++) t[r] = t[r] + d[r];
    t[EX4D_STAT_MAX_RADII] = d[EX4D_STAT_MAX_RADII] > t[EX4D_STAT_MAX_RADII] ? d[EX4D_STAT_MAX_RADII] : t[EX4D_STAT_MAX_RADII];
    t[EX4D_STAT_MIN_RADII] = d[EX4D_STAT_MIN_RADII] < t[EX4D_STAT_MIN_RADII] ? d[EX4D_STAT_MIN_RADII] : t[EX4D_STAT_MIN_RADII];
    if (t[EX4D_STAT_ERROR_MIN] > d[EX4D_STAT_ERROR_MIN]) {           // strict, as densify_stats_kernel: a tie keeps the lower rank's, a NaN is never taken
        t[EX4D_STAT_ERROR_MIN_T] = d[EX4D_STAT_ERROR_MIN_T];
        t[EX4D_STAT_ERROR_MIN] = d[EX4D_STAT_ERROR_MIN];
    }
}

// Left fold of the ranks' pending blocks [world, 9, n] into total [9, n], rank 0 first; own (may be null) is reset to the initial
// values.  A thread owns four neighbouring Gaussians per trip: it loads their nine rows of the total and of every rank (each a 16-byte
// access, a rank's nine in flight while the previous rank's are folded), and writes the nine rows back.  The last n % 4 Gaussians go
// one per thread to the first block.  No thread reads what another writes.
__global__ __launch_bounds__(DN_THREADS) void stats_merge_kernel(float *__restrict__ total, const float *__restrict__ pending, int world, long long n,
                                                                  float *__restrict__ own)
{
    const long long quads = n >> 2;
    const long long stride = (long long)gridDim.x * DN_THREADS;
    for (long long q = (long long)blockIdx.x * DN_THREADS + threadIdx.x; q < quads; q += stride) {
        const long long c = q << 2;
        float t[DN_MERGE_COLS][EX4D_DENSIFY_STATS];
#pragma unroll
        for (int r = 0; r < EX4D_DENSIFY_STATS; r++) {
            const merge_f4 v = merge_load(total + r * n + c);
            t[0][r] = v.x; t[1][r] = v.y; t[2][r] = v.z; t[3][r] = v.w;
        }
#pragma unroll 2
        for (int w = 0; w < world; w++) {
            const float *p = pending + (long long)w * EX4D_DENSIFY_STATS * n + c;
            merge_f4 v[EX4D_DENSIFY_STATS];
#pragma unroll
            for (int r = 0; r < EX4D_DENSIFY_STATS; r++) v[r] = merge_load(p + r * n);
            float d[DN_MERGE_COLS][EX4D_DENSIFY_STATS];
#pragma unroll
            for (int r = 0; r < EX4D_DENSIFY_STATS; r++) { d[0][r] = v[r].x; d[1][r] = v[r].y; d[2][r] = v[r].z; d[3][r] = v[r].w; }
#pragma unroll
            for (int k = 0; k < DN_MERGE_COLS; k++) merge_fold(t[k], d[k]);
        }
#pragma unroll
        for (int r = 0; r < EX4D_DENSIFY_STATS; r++) {
            merge_f4 v;
            v.x = t[0][r]; v.y = t[1][r]; v.z = t[2][r]; v.w = t[3][r];
            merge_store(total + r * n + c, v);
        }
        if (own) {
#pragma unroll
            for (int r = 0; r < EX4D_DENSIFY_STATS; r++) {
                const float s = stat_init(r);
                merge_f4 v;
                v.x = s; v.y = s; v.z = s; v.w = s;
                merge_store(own + r * n + c, v);
            }
        }
    }
    const long long c = (quads << 2) + threadIdx.x;
    if (blockIdx.x == 0 && c < n) {
        float t[EX4D_DENSIFY_STATS], d[EX4D_DENSIFY_STATS];
#pragma unroll
        for (int r = 0; r < EX4D_DENSIFY_STATS; r++) t[r] = total[r * n + c];
        for (int w = 0; w < world; w++) {
            const float *p = pending + (long long)w * EX4D_DENSIFY_STATS * n + c;
#pragma unroll
            for (int r = 0; r < EX4D_DENSIFY_STATS; r++) d[r] = p[r * n];
            merge_fold(t, d);
        }
#pragma unroll
        for (int r = 0; r < EX4D_DENSIFY_STATS; r++) total[r * n + c] = t[r];
        if (own) {
#pragma unroll
            for (int r = 0; r < EX4D_DENSIFY_STATS; r++) own[r * n + c] = stat_init(r);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- NaN census
#define DN_NAN_UNROLL 4                     // 16-byte loads in flight per thread and trip
#define DN_NAN_MAX_BLOCKS 2048              // per array: enough waves to saturate the memory system, the rest is the grid-stride loop

__global__ void nan_flags_clear_kernel(int *__restrict__ flags2)
{
    if (threadIdx.x < 2) flags2[threadIdx.x] = 0;
}

// (bitwise, not short-circuit: every word of a 16-byte load is looked at, so the load stays one instruction)
__device__ __forceinline__ bool nan_bits(unsigned u) { return (u & 0x7fffffffu) > 0x7f800000u; }
__device__ __forceinline__ bool nan_bits4(const uint4 &v) { return nan_bits(v.x) | nan_bits(v.y) | nan_bits(v.z) | nan_bits(v.w); }

// Blocks [0, blocks_a) stream a, the others b.  An array is a scalar head up to the first 16-byte boundary (at most 3 floats), an
// aligned body of uint4 loads and a scalar tail (at most 3 floats); head and tail belong to the array's first block.  Every thread
// reaches the ballot; a wave that saw a NaN stores 1 -- all writers store the same value, so there is nothing to order.
__global__ __launch_bounds__(DN_THREADS) void nan_any_kernel(const float *__restrict__ a, long long n_a, const float *__restrict__ b, long long n_b,
                                                              unsigned blocks_a, int *__restrict__ flags2)
{
    const bool second = blockIdx.x >= blocks_a;
    const float *p = second ? b : a;
    const long long n = second ? n_b : n_a;
    const unsigned blk = second ? blockIdx.x - blocks_a : blockIdx.x;
    const unsigned nblk = second ? gridDim.x - blocks_a : blocks_a;
    long long head = (long long)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
    if (head > n) head = n;
    const long long n16 = (n - head) >> 2;
    const long long tail0 = head + 4 * n16;
    const uint4 *__restrict__ body = reinterpret_cast<const uint4 *>(p + head);
    bool found = false;
    const long long stride = (long long)nblk * DN_THREADS;
    long long i = (long long)blk * DN_THREADS + threadIdx.x;
    for (; i + (DN_NAN_UNROLL - 1) * stride < n16; i += DN_NAN_UNROLL * stride) {
        uint4 v[DN_NAN_UNROLL];
#pragma unroll
        for (int k = 0; k < DN_NAN_UNROLL; k++) v[k] = body[i + k * stride];
#pragma unroll
        for (int k = 0; k < DN_NAN_UNROLL; k++) found |= nan_bits4(v[k]);
    }
    for (; i < n16; i += stride) {
        found |= nan_bits4(body[i]);
    }
    if (blk == 0) {
        const long long t = threadIdx.x;
        if (t < head) found |= nan_bits(__float_as_uint(p[t]));
        if (tail0 + t < n) found |= nan_bits(__float_as_uint(p[tail0 + t]));
    }
    if (__ballot(found) != 0ull && (threadIdx.x & 63) == 0) flags2[second ? 1 : 0] = 1;
}

// ---------------------------------------------------------------------------------------------------------------- plan
__device__ __forceinline__ float max3(float a, float b, float c)
{
    // torch.max(dim=1).values propagates NaN, whichever column holds it
    const float m = (a != a || a >= b) ? a : b;
    return (m != m || m >= c) ? m : c;
}

struct PlanArgs {
    long long n;
    const float *stats, *scaling, *opacity, *xyz;
    int xyz_width, use_screen, mode;
    float grad_thr, dense_scale, big_scale, screen_size, min_opacity, l1_thres, max_ssim;
};

// prune_mask terms of densify_and_prune (:1034-1070) for a row whose statistics were just reset by densification_postfix:
// big_points_vs compares the reset max_radii2D (0), the l1 / ssim masks divide the reset accumulators (0 / clamp(0, 1e-4))
__device__ __forceinline__ bool prune_terms(const PlanArgs &a, float opacity_logit, float max_scale)
{
    const float sig = 1.f / (1.f + expf(-opacity_logit));
    bool p = sig < a.min_opacity;
    if (a.use_screen) p = p || (0.f > a.screen_size) || (max_scale > a.big_scale);
    const float l1 = 0.f / 1e-4f, ssim = 0.f / 1e-4f;
    p = p || (l1 > a.l1_thres);
    p = p || ((ssim < a.max_ssim) && (ssim > 0.f));
    return p;
}

__device__ unsigned classify(const PlanArgs &a, long long i)
{
    const long long n = a.n;
    if (a.mode == EX4D_PLAN_PRUNE_INVISIBLE) return a.stats[EX4D_STAT_ERROR_MIN_T * n + i] < 0.f ? 0u : F_KEEP;
    if (a.mode == EX4D_PLAN_PRUNE_SMALL) return a.stats[EX4D_STAT_MIN_RADII * n + i] < 5.f ? 0u : F_KEEP;
    if (a.mode == EX4D_PLAN_PRUNE_NAN) {
        bool nan = false;
        for (int k = 0; k < a.xyz_width; k++) { const float x = a.xyz[i * a.xyz_width + k]; nan = nan || x != x; }
        return nan ? 0u : F_KEEP;
    }
    // densify_and_prune: grads = accum / denom with NaN -> 0 (:1021-1025)
    float g = a.stats[EX4D_STAT_GRAD_ACCUM * n + i] / a.stats[EX4D_STAT_DENOM * n + i];
    if (g != g) g = 0.f;
    const float s0 = expf(a.scaling[3 * i]), s1 = expf(a.scaling[3 * i + 1]), s2 = expf(a.scaling[3 * i + 2]);
    const float ms = max3(s0, s1, s2);
    const bool clone = fabsf(g) >= a.grad_thr && ms <= a.dense_scale;                       // densify_and_clone (:966)
    // densify_and_split (:874) over the post-clone set: max_radii2D was reset to 0 by the clone's postfix; a clone's padded gradient is 0
    const bool big = a.use_screen && ((0.f > a.screen_size) || (ms > a.big_scale));
    const bool split = (g >= a.grad_thr && ms > a.dense_scale) || big;
    const bool split_clone = clone && ((0.f >= a.grad_thr && ms > a.dense_scale) || big);
    // children: log(exp(s) / (0.8 N)) stored, exp of it read back by the prune's big_points_ws
    const float c0 = expf(logf(s0 / 1.6f)), c1 = expf(logf(s1 / 1.6f)), c2 = expf(logf(s2 / 1.6f));
    const float op = a.opacity[i];
    const bool prune_row = prune_terms(a, op, ms);                 // original and clone: the same opacity and scales
    const bool prune_child = prune_terms(a, op, max3(c0, c1, c2));
    unsigned f = 0;
    if (!(split || prune_row)) f |= F_KEEP;
    if (clone) f |= F_CLONE;
    if (clone && !(split_clone || prune_row)) f |= F_KEEP_CLONE;
    if (split) f |= F_SPLIT;
    if (split_clone) f |= F_SPLIT_CLONE;
    if (split && !prune_child) f |= F_KEEP_CHILD;
    if (split_clone && !prune_child) f |= F_KEEP_CHILD_CLONE;
    return f;
}

__device__ __forceinline__ unsigned long long pack(unsigned f)
{
    unsigned long long p = 0;
#pragma unroll
    for (int k = 0; k < DN_FIELDS; k++) p |= (unsigned long long)((f >> k) & 1u) << (DN_FIELD_BITS * k);
    return p;
}

__device__ __forceinline__ int field(unsigned long long p, int k) { return (int)((p >> (DN_FIELD_BITS * k)) & ((1u << DN_FIELD_BITS) - 1)); }

__global__ __launch_bounds__(DN_THREADS) void plan_classify_kernel(const PlanArgs a, unsigned char *__restrict__ flags, int *__restrict__ block_sums)
{
    __shared__ unsigned long long red[DN_THREADS];
    const long long i = (long long)blockIdx.x * DN_THREADS + threadIdx.x;
    unsigned f = 0;
    if (i < a.n) {
        f = classify(a, i);
        flags[i] = (unsigned char)f;
    }
    red[threadIdx.x] = pack(f);
    __syncthreads();
    for (int s = DN_THREADS / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < DN_FIELDS) block_sums[(size_t)blockIdx.x * 8 + threadIdx.x] = field(red[0], threadIdx.x);
}

// one workgroup: exclusive scan of the per-block counters (in place), totals to counts[]
__global__ __launch_bounds__(DN_THREADS) void plan_scan_kernel(int *__restrict__ block_sums, int nb, int *__restrict__ counts)
{
    __shared__ int tot[DN_THREADS][8];
    __shared__ int total[8];
    const int per = (nb + DN_THREADS - 1) / DN_THREADS;
    const int b0 = min(nb, (int)threadIdx.x * per), b1 = min(nb, b0 + per);
    int s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = b0; b < b1; b++)
        for (int k = 0; k < DN_FIELDS; k++) s[k] += block_sums[(size_t)b * 8 + k];
    for (int k = 0; k < 8; k++) tot[threadIdx.x][k] = s[k];
    __syncthreads();
    if (threadIdx.x < DN_FIELDS) {
        int run = 0;
        for (int t = 0; t < DN_THREADS; t++) { const int v = tot[t][threadIdx.x]; tot[t][threadIdx.x] = run; run += v; }
        total[threadIdx.x] = run;
        counts[threadIdx.x] = run;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        counts[EX4D_CNT_ROWS] = total[EX4D_CNT_KEEP] + total[EX4D_CNT_KEEP_CLONE] + 2 * (total[EX4D_CNT_KEEP_CHILD] + total[EX4D_CNT_KEEP_CHILD_CLONE]);
    int run[8];
    for (int k = 0; k < 8; k++) run[k] = tot[threadIdx.x][k];
    for (int b = b0; b < b1; b++)
        for (int k = 0; k < DN_FIELDS; k++) { const int v = block_sums[(size_t)b * 8 + k]; block_sums[(size_t)b * 8 + k] = run[k]; run[k] += v; }
}

// per-row destination map: block-local exclusive scan of the packed flags + the block's offsets + the group totals
__global__ __launch_bounds__(DN_THREADS) void plan_map_kernel(long long n, const unsigned char *__restrict__ flags, const int *__restrict__ block_off,
                                                               const int *__restrict__ counts, int *__restrict__ map)
{
    __shared__ unsigned long long sc[DN_THREADS];
    const long long i = (long long)blockIdx.x * DN_THREADS + threadIdx.x;
    const unsigned f = i < n ? flags[i] : 0u;
    const unsigned long long mine = pack(f);
    sc[threadIdx.x] = mine;
    __syncthreads();
    for (int s = 1; s < DN_THREADS; s <<= 1) {                  // Hillis-Steele inclusive scan (fields never carry: <= 256 each)
        const unsigned long long v = threadIdx.x >= s ? sc[threadIdx.x - s] : 0ull;
        __syncthreads();
        sc[threadIdx.x] += v;
        __syncthreads();
    }
    if (i >= n) return;
    const unsigned long long ex = sc[threadIdx.x] - mine;
    const int *bo = block_off + (size_t)blockIdx.x * 8;
    int e[DN_FIELDS];
#pragma unroll
    for (int k = 0; k < DN_FIELDS; k++) e[k] = bo[k] + field(ex, k);
    const int keep = counts[EX4D_CNT_KEEP], keep_c = counts[EX4D_CNT_KEEP_CLONE], kch = counts[EX4D_CNT_KEEP_CHILD];
    const int nsplit = counts[EX4D_CNT_SPLIT_SEL];
    int4 d, w;
    d.x = (f & F_KEEP) ? e[EX4D_CNT_KEEP] : -1;                                                  // survivors, in row order
    d.y = (f & F_KEEP_CLONE) ? keep + e[EX4D_CNT_KEEP_CLONE] : -1;                               // surviving clones
    d.z = (f & F_KEEP_CHILD) ? keep + keep_c + e[EX4D_CNT_KEEP_CHILD] : -1;                      // children (copy 0) of split originals
    d.w = (f & F_KEEP_CHILD_CLONE) ? keep + keep_c + kch + e[EX4D_CNT_KEEP_CHILD_CLONE] : -1;    // ... of split clones
    w.x = (f & F_CLONE) ? e[EX4D_CNT_CLONE_SEL] : -1;                                            // clone jitter draw
    w.y = (f & F_SPLIT) ? e[EX4D_CNT_SPLIT_SEL] : -1;                                            // split draw (copy 0)
    w.z = (f & F_SPLIT_CLONE) ? nsplit + e[EX4D_CNT_SPLIT_SEL_CLONE] : -1;                       // split draw of the clone
    w.w = -1;
    int4 *m = (int4 *)(map + (size_t)i * EX4D_PLAN_MAP_INTS);
    m[0] = d;
    m[1] = w;
}

// ---------------------------------------------------------------------------------------------------------------- apply
struct ApplySlot {
    Ex4dDensifyTensor t;
    long long numel;                 // planes * rows * width
    unsigned first_chunk;
};
struct ApplyArgs {
    ApplySlot slot[EX4D_DENSIFY_MAX_TENSORS];
    Ex4dDensifyApplyGroup grp[2];
    int count;
};

__device__ __forceinline__ float clampf(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// duration-centre jitter of densify_and_clone / densify_and_split (:971-976, :906-911): len from the pre-jitter pair, c1 first
__device__ __forceinline__ void jitter(float &c0, float &c1, float z0, float z1, const Ex4dDensifyApplyGroup &g)
{
    float len = fabsf(c1 - c0) / 3.f;
    len = len < g.min_len ? g.min_len : len;
    const float n1 = c1 + len * z1, n0 = c0 + len * z0;
    c0 = clampf(n0, g.center_lo, g.center_hi);
    c1 = clampf(n1, g.center_lo, g.center_hi);
}

// build_rotation (utils/general_utils.py:106-127) row `c` of R(normalize(q)) applied to v
__device__ __forceinline__ float rot_row(const float *q4, int c, float v0, float v1, float v2)
{
    const float norm = sqrtf(q4[0] * q4[0] + q4[1] * q4[1] + q4[2] * q4[2] + q4[3] * q4[3]);
    const float r = q4[0] / norm, x = q4[1] / norm, y = q4[2] / norm, z = q4[3] / norm;
    float a, b, d;
    if (c == 0)      { a = 1.f - 2.f * (y * y + z * z); b = 2.f * (x * y - r * z); d = 2.f * (x * z + r * y); }
    else if (c == 1) { a = 2.f * (x * y + r * z); b = 1.f - 2.f * (x * x + z * z); d = 2.f * (y * z - r * x); }
    else             { a = 2.f * (x * z - r * y); b = 2.f * (y * z + r * x); d = 1.f - 2.f * (x * x + y * y); }
    return a * v0 + b * v1 + d * v2;
}

__global__ __launch_bounds__(DN_THREADS) void densify_apply_kernel(const ApplyArgs a)
{
    int t = 0;
#pragma unroll 1
    for (int k = 1; k < a.count; k++) if (blockIdx.x >= a.slot[k].first_chunk) t = k;
    const ApplySlot &s = a.slot[t];
    const Ex4dDensifyTensor &d = s.t;
    const Ex4dDensifyApplyGroup &g = a.grp[d.group];
    const long long base = (long long)(blockIdx.x - s.first_chunk) * DN_APPLY_CHUNK;
    const long long end = s.numel - base < DN_APPLY_CHUNK ? s.numel : base + DN_APPLY_CHUNK;
    const long long plane_elems = d.rows * d.width;
#pragma unroll 1
    for (long long e = base + threadIdx.x; e < end; e += DN_THREADS) {
        const long long plane = e / plane_elems;
        const long long rem = e - plane * plane_elems;
        const long long row = rem / d.width;
        const int col = (int)(rem - row * d.width);
        const int4 dst = *(const int4 *)(g.map + (size_t)row * EX4D_PLAN_MAP_INTS);
        if ((dst.x & dst.y & dst.z & dst.w) < 0) continue;              // all four -1: pruned, no new rows
        const float v = d.src[e];
        float *out = d.dst + plane * d.dst_rows * d.width + col;
        float v_orig = v, v_clone = v, v_child[2][2] = {{v, v}, {v, v}};   // [of original / of clone][copy]
        switch (d.rule) {
        case EX4D_RULE_COPY: break;
        case EX4D_RULE_ZERO_NEW: v_clone = 0.f; v_child[0][0] = v_child[0][1] = v_child[1][0] = v_child[1][1] = 0.f; break;
        case EX4D_RULE_CONST_NEW: v_clone = d.value; v_child[0][0] = v_child[0][1] = v_child[1][0] = v_child[1][1] = d.value; break;
        case EX4D_RULE_CHILD_SCALING: {
            const float c = logf(expf(v) / g.split_div);
            v_child[0][0] = v_child[0][1] = v_child[1][0] = v_child[1][1] = c;
            break;
        }
        case EX4D_RULE_CHILD_XYZ: {
            if (dst.z < 0 && dst.w < 0) break;
            const int K = d.width / 3, kf = col / 3, c = col - 3 * kf;
            const float *q = d.aux0 + ((size_t)row * K + kf) * 4;
            const float *ls = d.aux1 + (size_t)row * 3;
            const float sd0 = expf(ls[0]) * d.value, sd1 = expf(ls[1]) * d.value, sd2 = expf(ls[2]) * d.value;
            const int4 w = *(const int4 *)(g.map + (size_t)row * EX4D_PLAN_MAP_INTS + 4);
            for (int o = 0; o < 2; o++) {
                const int draw = o == 0 ? w.y : w.z;
                if (draw < 0) continue;
                for (int j = 0; j < 2; j++) {
                    const float *z = g.split_z + ((size_t)j * g.n_split + draw) * 3;
                    v_child[o][j] = rot_row(q, c, sd0 * z[0], sd1 * z[1], sd2 * z[2]) + v;
                }
            }
            break;
        }
        case EX4D_RULE_CENTER: {
            const int4 w = *(const int4 *)(g.map + (size_t)row * EX4D_PLAN_MAP_INTS + 4);
            const float c0 = d.src[row * 2], c1 = d.src[row * 2 + 1];
            float k0 = c0, k1 = c1;                                       // the clone's centres
            if (w.x >= 0) { jitter(k0, k1, g.clone_c0[w.x], g.clone_c1[w.x], g); v_clone = col ? k1 : k0; }
            for (int o = 0; o < 2; o++) {
                const int draw = o == 0 ? w.y : w.z;
                if (draw < 0) continue;
                for (int j = 0; j < 2; j++) {
                    const size_t q = (size_t)j * g.n_split + draw;
                    float a0 = o ? k0 : c0, a1 = o ? k1 : c1;
                    jitter(a0, a1, g.split_c0[q], g.split_c1[q], g);
                    v_child[o][j] = col ? a1 : a0;
                }
            }
            break;
        }
        case EX4D_RULE_STATS: {
            if (plane <= EX4D_STAT_MIN_RADII) {                           // densification_postfix resets these for every row
                const float r = plane == EX4D_STAT_MIN_RADII ? 1000.f : 0.f;
                v_orig = v_clone = v_child[0][0] = v_child[0][1] = v_child[1][0] = v_child[1][1] = r;
            } else {                                                      // error min / timestamp: kept, inherited by clones, children reset
                const float r = plane == EX4D_STAT_ERROR_MIN ? 1000.f : -1.f;
                v_child[0][0] = v_child[0][1] = v_child[1][0] = v_child[1][1] = r;
            }
            break;
        }
        default: break;
        }
        const long long W = d.width;
        if (dst.x >= 0) out[dst.x * W] = v_orig;
        if (dst.y >= 0) out[dst.y * W] = v_clone;
        if (dst.z >= 0) { out[dst.z * W] = v_child[0][0]; out[(dst.z + g.child_stride) * W] = v_child[0][1]; }
        if (dst.w >= 0) { out[dst.w * W] = v_child[1][0]; out[(dst.w + g.child_stride) * W] = v_child[1][1]; }
    }
}

inline int launch_error(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_densify_err, sizeof(g_densify_err), "%s: launch failed: %s", what, hipGetErrorString(e)); return EX4D_ERR_HIP; }
    return EX4D_OK;
}

inline long long num_blocks(long long n) { return (n + DN_THREADS - 1) / DN_THREADS; }

}  // namespace

// the text ex4d_densify_last_error returns, for ex4d_growth.hip (the same header, the same error channel)
char *ex4d_densify_error_buffer(size_t *capacity)
{
    *capacity = sizeof(g_densify_err);
    return g_densify_err;
}

extern "C" {

const char *ex4d_densify_last_error(void) { return g_densify_err; }

int ex4d_densify_stats(float *stats_s, int64_t ns, float *stats_d, int64_t nd, const int32_t *radii, const float *vgrad,
                       const float *egrad, float timestamp, int32_t flags, void *stream_)
{
    g_densify_err[0] = 0;
    const bool need_e = flags & (EX4D_DENSIFY_PRUNE_STATS | EX4D_DENSIFY_L1_STATS);
    if (ns < 0 || nd < 0 || (ns > 0 && !stats_s) || (nd > 0 && !stats_d) || ((ns + nd) > 0 && (!radii || !vgrad || (need_e && !egrad)))) {
        snprintf(g_densify_err, sizeof(g_densify_err), "densify_stats: negative size or null pointer");
        return EX4D_ERR_ARG;
    }
    hipStream_t stream = (hipStream_t)stream_;
    if (ns > 0) hipLaunchKernelGGL(densify_stats_kernel, dim3((unsigned)num_blocks(ns)), dim3(DN_THREADS), 0, stream, stats_s, (long long)ns, 0ll, radii, vgrad, egrad, timestamp, (int)flags);
    if (nd > 0) hipLaunchKernelGGL(densify_stats_kernel, dim3((unsigned)num_blocks(nd)), dim3(DN_THREADS), 0, stream, stats_d, (long long)nd, (long long)ns, radii, vgrad, egrad, timestamp, (int)flags);
    return launch_error("densify_stats");
}

int ex4d_densify_stats_merge(float *total, const float *pending, int32_t world, int64_t n, float *own_pending, void *stream_)
{
    g_densify_err[0] = 0;
    if (world < 0 || n < 0) {
        snprintf(g_densify_err, sizeof(g_densify_err), "densify_stats_merge: negative rank count or size");
        return EX4D_ERR_ARG;
    }
    if (world == 0 || n == 0) return EX4D_OK;
    const uintptr_t t0 = (uintptr_t)total, p0 = (uintptr_t)pending, o0 = (uintptr_t)own_pending;
    const uintptr_t block = (uintptr_t)EX4D_DENSIFY_STATS * (uintptr_t)n * sizeof(float);
    const uintptr_t t1 = t0 + block, p1 = p0 + block * (uintptr_t)world, o1 = o0 + block;
    if (!total || !pending || ((t0 | p0 | o0) & 3u)) {
        snprintf(g_densify_err, sizeof(g_densify_err), "densify_stats_merge: null or misaligned block");
        return EX4D_ERR_ARG;
    }
    if ((t0 < p1 && p0 < t1) || (own_pending && ((o0 < t1 && t0 < o1) || (o0 < p1 && p0 < o1)))) {
        snprintf(g_densify_err, sizeof(g_densify_err), "densify_stats_merge: the total, the pending blocks and the own block must not overlap");
        return EX4D_ERR_ARG;
    }
    const long long want = ((long long)n + DN_MERGE_CHUNK - 1) / DN_MERGE_CHUNK;
    const unsigned blocks = (unsigned)(want > DN_MERGE_MAX_BLOCKS ? DN_MERGE_MAX_BLOCKS : want);
    hipLaunchKernelGGL(stats_merge_kernel, dim3(blocks), dim3(DN_THREADS), 0, (hipStream_t)stream_, total, pending, (int)world, (long long)n, own_pending);
    return launch_error("densify_stats_merge");
}

size_t ex4d_densify_scratch_bytes(int64_t n)
{
    if (n <= 0) return 0;
    const size_t nb = (size_t)num_blocks(n);
    return ex4d_align_up((size_t)n) + ex4d_align_up(nb * 8 * sizeof(int));
}

int ex4d_densify_plan(int32_t mode, const Ex4dDensifyPlanGroup *grp, void *stream_)
{
    g_densify_err[0] = 0;
    if (!grp || mode < EX4D_PLAN_DENSIFY || mode > EX4D_PLAN_PRUNE_NAN) {
        snprintf(g_densify_err, sizeof(g_densify_err), "densify_plan: null group or unknown mode %d", mode);
        return EX4D_ERR_ARG;
    }
    const Ex4dDensifyPlanGroup &G = *grp;
    if (G.n < 0 || G.n > 0x7fffffffLL - 1 || (G.n > 0 && (!G.map || !G.counts || !G.scratch || !G.stats)) ||
        (G.n > 0 && mode == EX4D_PLAN_DENSIFY && (!G.scaling || !G.opacity)) ||
        (G.n > 0 && mode == EX4D_PLAN_PRUNE_NAN && (!G.xyz || G.xyz_width < 1))) {
        snprintf(g_densify_err, sizeof(g_densify_err), "densify_plan: bad size or null pointer");
        return EX4D_ERR_ARG;
    }
    hipStream_t stream = (hipStream_t)stream_;
    if (G.n == 0) {
        if (G.counts && hipMemsetAsync(G.counts, 0, EX4D_PLAN_COUNTS * sizeof(int32_t), stream) != hipSuccess) {
            snprintf(g_densify_err, sizeof(g_densify_err), "densify_plan: memset failed");
            return EX4D_ERR_HIP;
        }
        return EX4D_OK;
    }
    PlanArgs a;
    a.n = G.n; a.stats = G.stats; a.scaling = G.scaling; a.opacity = G.opacity; a.xyz = G.xyz; a.xyz_width = G.xyz_width;
    a.use_screen = G.use_screen; a.mode = mode; a.grad_thr = G.grad_thr; a.dense_scale = G.dense_scale; a.big_scale = G.big_scale;
    a.screen_size = G.screen_size; a.min_opacity = G.min_opacity; a.l1_thres = G.l1_thres; a.max_ssim = G.max_ssim;
    const long long nb = num_blocks(G.n);
    unsigned char *flags = (unsigned char *)G.scratch;
    int *block_sums = (int *)((char *)G.scratch + ex4d_align_up((size_t)G.n));
    hipLaunchKernelGGL(plan_classify_kernel, dim3((unsigned)nb), dim3(DN_THREADS), 0, stream, a, flags, block_sums);
    hipLaunchKernelGGL(plan_scan_kernel, dim3(1), dim3(DN_THREADS), 0, stream, block_sums, (int)nb, (int *)G.counts);
    hipLaunchKernelGGL(plan_map_kernel, dim3((unsigned)nb), dim3(DN_THREADS), 0, stream, (long long)G.n, flags, block_sums, (const int *)G.counts, (int *)G.map);
    return launch_error("densify_plan");
}

int ex4d_densify_apply(const Ex4dDensifyTensor *tensors, int32_t count, const Ex4dDensifyApplyGroup *groups, void *stream_)
{
    g_densify_err[0] = 0;
    if (count < 0 || count > EX4D_DENSIFY_MAX_TENSORS || (count > 0 && (!tensors || !groups))) {
        snprintf(g_densify_err, sizeof(g_densify_err), "densify_apply: count %d outside [0, %d] or null pointer", count, EX4D_DENSIFY_MAX_TENSORS);
        return EX4D_ERR_ARG;
    }
    ApplyArgs a;
    a.count = 0;
    if (count > 0) { a.grp[0] = groups[0]; a.grp[1] = groups[1]; }
    unsigned chunks = 0;
    for (int i = 0; i < count; i++) {
        const Ex4dDensifyTensor &t = tensors[i];
        const long long numel = (long long)t.planes * t.rows * t.width;
        if (t.rows == 0) continue;
        const bool stats = t.rule == EX4D_RULE_STATS;
        if (t.rows < 0 || t.dst_rows < 0 || t.width < 1 || t.planes < 1 || !t.src || (t.dst_rows > 0 && !t.dst) || t.group < 0 || t.group > 1 ||
            t.rule < EX4D_RULE_COPY || t.rule > EX4D_RULE_STATS || (stats && (t.planes != EX4D_DENSIFY_STATS || t.width != 1)) ||
            (t.planes != 1 && (t.planes != EX4D_DENSIFY_STATS || t.width != 1 || (t.rule != EX4D_RULE_COPY && !stats))) || !groups[t.group].map ||
            (t.rule == EX4D_RULE_CHILD_XYZ && (t.width % 3 != 0 || !t.aux0 || !t.aux1 || !groups[t.group].split_z)) ||
            (t.rule == EX4D_RULE_CENTER && (t.width != 2 || !groups[t.group].split_c0 || !groups[t.group].split_c1 ||
                                            !groups[t.group].clone_c0 || !groups[t.group].clone_c1))) {
            snprintf(g_densify_err, sizeof(g_densify_err), "densify_apply: tensor %d: bad shape, rule or null pointer", i);
            return EX4D_ERR_ARG;
        }
        ApplySlot &s = a.slot[a.count++];
        s.t = t; s.numel = numel; s.first_chunk = chunks;
        const long long c = (numel + DN_APPLY_CHUNK - 1) / DN_APPLY_CHUNK;
        if (c + chunks > 0x7fffffffLL) { snprintf(g_densify_err, sizeof(g_densify_err), "densify_apply: too many elements for one launch"); return EX4D_ERR_ARG; }
        chunks += (unsigned)c;
    }
    if (chunks == 0) return EX4D_OK;
    hipLaunchKernelGGL(densify_apply_kernel, dim3(chunks), dim3(DN_THREADS), 0, (hipStream_t)stream_, a);
    return launch_error("densify_apply");
}

int ex4d_nan_any(const float *a, int64_t n_a, const float *b, int64_t n_b, int32_t *flags2, void *stream_)
{
    g_densify_err[0] = 0;
    if (!flags2 || n_a < 0 || n_b < 0 || (n_a > 0 && !a) || (n_b > 0 && !b) || (((uintptr_t)a | (uintptr_t)b | (uintptr_t)flags2) & 3u)) {
        snprintf(g_densify_err, sizeof(g_densify_err), "nan_any: null flags, negative size, null or misaligned array");
        return EX4D_ERR_ARG;
    }
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(nan_flags_clear_kernel, dim3(1), dim3(64), 0, stream, (int *)flags2);
    unsigned blocks[2];
    const int64_t n[2] = { n_a, n_b };
    for (int k = 0; k < 2; k++) {
        // one block per DN_THREADS * DN_NAN_UNROLL 16-byte loads, at least one for a non-empty array (its head / tail)
        const long long per = (long long)DN_THREADS * DN_NAN_UNROLL * 4;
        const long long want = (n[k] + per - 1) / per;
        blocks[k] = n[k] == 0 ? 0u : (unsigned)(want > DN_NAN_MAX_BLOCKS ? DN_NAN_MAX_BLOCKS : want);
    }
    if (blocks[0] + blocks[1] > 0)
        hipLaunchKernelGGL(nan_any_kernel, dim3(blocks[0] + blocks[1]), dim3(DN_THREADS), 0, stream, a, (long long)n_a, b, (long long)n_b, blocks[0], (int *)flags2);
    return launch_error("nan_any");
}

}  // extern "C"
