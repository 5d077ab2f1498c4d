// Growth of the dynamic set for gfx950 (include/ex4d_densify.h, the "growth" part): dynamic-point extraction, duration expansion
// and the temporal-opacity adjustment of the reference's CGaussianModel (scene/c_gaussian_model.py:1147-1358).
//
// The reference composes an extraction from boolean-mask indexing over every parameter, both moments and 18 statistic tensors, and a
// full sort inside torch.quantile.  Here:
//   growth_scores    one thread per static row: the motion score of a visible row, -1 for an invisible one
//   growth_select    the two order statistics torch.quantile interpolates, by a radix select over four 8-bit histograms of the
//                    scores' bit patterns (non-negative floats order as unsigned integers; integer counts do not depend on the
//                    order of the atomics), then the threshold with torch's rank and lerp arithmetic
//   growth_classify  selected flag per row -> scan -> a destination map in the layout of ex4d_densify_plan (the static prune is
//                    ex4d_densify_apply) and the ascending list of selected source rows
//   growth_append    one multi-tensor launch: old dynamic rows copied, new rows generated from their static source rows
// ffp-contract is off for this file: decisions and generated values follow torch's float32 op order.
#include "ex4d_internal.h"
#include "../../include/ex4d_densify.h"
#define EX4D_ERROR_BUFFER ex4d_densify_error_buffer     // ex4d_densify.hip: the text ex4d_densify_last_error returns
#include "ex4d_host_error.h"

namespace {

#define GR_THREADS 256
#define GR_MAX_BLOCKS 2048                 // grid-stride kernels: enough workgroups to fill the chip, the rest is a loop
#define GR_APPEND_CHUNK 4096               // destination elements per workgroup of the append (16 per thread)
#define GR_BINS 256
#define GR_NAN_BITS 0x7fc00000u            // every NaN score is counted as this pattern: above every number, as torch sorts it

// select scratch, in 32-bit words: four histograms, then the state
enum { SS_HIST = 0, SS_COUNT = 4 * GR_BINS, SS_MAX, SS_PREFIX, SS_RANK, SS_BELOW, SS_LO_BITS, SS_NEED_NEXT, SS_NEXT_MIN, SS_WEIGHT, SS_WORDS };

inline unsigned grid_for(long long n)
{
    const long long nb = (n + GR_THREADS - 1) / GR_THREADS;
    return (unsigned)(nb < 1 ? 1 : (nb > GR_MAX_BLOCKS ? GR_MAX_BLOCKS : nb));
}

__device__ __forceinline__ float norm3(const float *p)
{
    return sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
}

// ---------------------------------------------------------------------------------------------------------------- scores
__global__ __launch_bounds__(GR_THREADS) void growth_scores_kernel(const float *__restrict__ xyz, const float *__restrict__ disp,
                                                                    const unsigned char *__restrict__ vis, const float *__restrict__ cam,
                                                                    long long n, float *__restrict__ score)
{
    const float cx = cam[0], cy = cam[1], cz = cam[2];
    for (long long i = (long long)blockIdx.x * GR_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * GR_THREADS) {
        float s = -1.f;
        if (vis[i]) {
            const float nrm = norm3(disp + 3 * i);
            const float d[3] = {xyz[3 * i] - cx, xyz[3 * i + 1] - cy, xyz[3 * i + 2] - cz};
            const float r = norm3(d);
            s = nrm / (r * r + 0.000001f);                       // norm, then square, as the reference writes it
            if (s != s) s = __uint_as_float(GR_NAN_BITS);
        }
        score[i] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------- select
// the bit pattern a score is selected by; false: the entry is absent (sign bit set and not a NaN)
__device__ __forceinline__ bool present_bits(float s, unsigned &bits)
{
    bits = __float_as_uint(s);
    if (s != s) { bits = GR_NAN_BITS; return true; }
    return !(bits & 0x80000000u);
}

// pass p histograms byte (3 - p) of the entries whose higher bytes equal the prefix found so far; pass 0 also counts and takes the max
__global__ __launch_bounds__(GR_THREADS) void select_hist_kernel(const float *__restrict__ score, long long n, int pass, unsigned *__restrict__ ws)
{
    __shared__ unsigned hist[GR_BINS];
    __shared__ unsigned red[GR_THREADS];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const unsigned prefix = pass ? ws[SS_PREFIX] : 0u;
    unsigned mx = 0;
    for (long long i = (long long)blockIdx.x * GR_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * GR_THREADS) {
        unsigned b;
        if (!present_bits(score[i], b)) continue;
        if (pass && (b >> (shift + 8)) != prefix) continue;
        atomicAdd(&hist[(b >> shift) & 255u], 1u);
        mx = b > mx ? b : mx;
    }
    red[threadIdx.x] = mx;
    __syncthreads();
    const unsigned h = hist[threadIdx.x];
    if (h) atomicAdd(&ws[SS_HIST + pass * GR_BINS + threadIdx.x], h);
    if (pass) return;
    for (int s = GR_THREADS / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] > red[threadIdx.x + s] ? red[threadIdx.x] : red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0 && red[0]) atomicMax(&ws[SS_MAX], red[0]);
}

// one workgroup: the bin of this pass that holds the rank, by an exclusive scan of its 256 counts
__global__ __launch_bounds__(GR_THREADS) void select_pick_kernel(int pass, float q, unsigned *__restrict__ ws)
{
    __shared__ unsigned sc[GR_THREADS];
    __shared__ unsigned rank_s;
    const unsigned mine = ws[SS_HIST + pass * GR_BINS + threadIdx.x];
    sc[threadIdx.x] = mine;
    __syncthreads();
    for (int s = 1; s < GR_THREADS; s <<= 1) {
        const unsigned v = threadIdx.x >= s ? sc[threadIdx.x - s] : 0u;
        __syncthreads();
        sc[threadIdx.x] += v;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        unsigned rank = ws[SS_RANK];
        if (pass == 0) {
            // torch.quantile: rank = q (n - 1) in float32, the order statistics at its floor and ceiling, weight = the fraction
            const unsigned count = sc[GR_THREADS - 1];
            ws[SS_COUNT] = count;
            const float rf = count ? q * (float)(count - 1u) : 0.f;
            const float lo = floorf(rf);
            rank = (unsigned)lo;
            if (count && rank > count - 1u) rank = count - 1u;           // q <= 1 keeps it inside; a guard for the index, not a path
            ws[SS_WEIGHT] = __float_as_uint(rf - lo);
            ws[SS_NEED_NEXT] = ceilf(rf) > lo ? 1u : 0u;
            ws[SS_BELOW] = 0u;
            ws[SS_PREFIX] = 0u;
            ws[SS_NEXT_MIN] = 0xffffffffu;
        }
        rank_s = rank;
    }
    __syncthreads();
    const unsigned rank = rank_s, incl = sc[threadIdx.x], excl = incl - mine;
    if (mine && excl <= rank && rank < incl) {                           // exactly one bin when the count is > 0
        ws[SS_PREFIX] = (ws[SS_PREFIX] << 8) | threadIdx.x;
        ws[SS_RANK] = rank - excl;
        ws[SS_BELOW] = ws[SS_BELOW] + excl;
        if (pass == 3) {
            // entries <= the lower statistic: those below its bin plus the bin (all equal by now); the upper one is the same value
            // when its index is still among them, else the smallest value above
            const unsigned le = ws[SS_BELOW] + mine;                      // BELOW was just updated by this thread
            const unsigned hi = (ws[SS_BELOW] + (rank - excl)) + 1u;      // index of the upper statistic when it differs
            ws[SS_LO_BITS] = ws[SS_PREFIX];
            if (ws[SS_NEED_NEXT] && hi < le) ws[SS_NEED_NEXT] = 0u;
        }
    }
}

// the smallest present value above the lower statistic
__global__ __launch_bounds__(GR_THREADS) void select_next_kernel(const float *__restrict__ score, long long n, unsigned *__restrict__ ws)
{
    __shared__ unsigned red[GR_THREADS];
    unsigned mn = 0xffffffffu;
    if (ws[SS_NEED_NEXT]) {
        const unsigned lo = ws[SS_LO_BITS];
        for (long long i = (long long)blockIdx.x * GR_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * GR_THREADS) {
            unsigned b;
            if (present_bits(score[i], b) && b > lo && b < mn) mn = b;
        }
    }
    red[threadIdx.x] = mn;
    __syncthreads();
    for (int s = GR_THREADS / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] < red[threadIdx.x + s] ? red[threadIdx.x] : red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0 && red[0] != 0xffffffffu) atomicMin(&ws[SS_NEXT_MIN], red[0]);
}

__global__ void select_finish_kernel(const unsigned *__restrict__ ws, float *__restrict__ result)
{
    if (threadIdx.x || blockIdx.x) return;
    const unsigned count = ws[SS_COUNT];
    float theta = __uint_as_float(GR_NAN_BITS), mx = 0.f;
    if (count) {
        mx = __uint_as_float(ws[SS_MAX]);
        const float den = mx + 0.000001f;
        const unsigned lo = ws[SS_LO_BITS];
        const unsigned hi = (ws[SS_NEED_NEXT] && ws[SS_NEXT_MIN] != 0xffffffffu) ? ws[SS_NEXT_MIN] : lo;
        // x / (max + 1e-6) is monotone: the order statistics of the normalised scores are the normalised order statistics
        const float a = __uint_as_float(lo) / den, b = __uint_as_float(hi) / den;
        const float w = __uint_as_float(ws[SS_WEIGHT]);
        const float diff = b - a;
        // torch's lerp, w < 0.5 ? a + w (b - a) : b - (b - a)(1 - w), whose multiply-add torch fuses (one rounding); 1 - w is exact from 0.5 on
        theta = w < 0.5f ? fmaf(w, diff, a) : fmaf(w - 1.f, diff, b);
    }
    result[EX4D_SELECT_THETA] = theta;
    result[EX4D_SELECT_MAX] = mx;
    result[EX4D_SELECT_COUNT] = __int_as_float((int)count);
    result[3] = 0.f;
}

// ---------------------------------------------------------------------------------------------------------------- classify
struct ClassifyArgs {
    long long n;
    const float *score, *result, *disp, *stats;
    float motion_abs, min_abs;
};

__global__ __launch_bounds__(GR_THREADS) void classify_flags_kernel(const ClassifyArgs a, unsigned char *__restrict__ flags, int *__restrict__ block_sums)
{
    __shared__ int red[GR_THREADS];
    const long long i = (long long)blockIdx.x * GR_THREADS + threadIdx.x;
    int sel = 0;
    if (i < a.n) {
        const float s = a.score[i];
        unsigned bits;
        if (present_bits(s, bits)) {
            const float theta = a.result[EX4D_SELECT_THETA], mx = a.result[EX4D_SELECT_MAX];
            const float u = s / (mx + 0.000001f);
            const float nrm = norm3(a.disp + 3 * i);
            sel = ((u > theta) || (nrm > a.motion_abs)) && (nrm > a.min_abs) && (a.stats[EX4D_STAT_ERROR_MIN_T * a.n + i] >= 0.f);
        }
        flags[i] = (unsigned char)sel;
    }
    red[threadIdx.x] = sel;
    __syncthreads();
    for (int s = GR_THREADS / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) block_sums[blockIdx.x] = red[0];
}

// one workgroup: exclusive scan of the per-block counts (in place), the totals
__global__ __launch_bounds__(GR_THREADS) void classify_scan_kernel(int *__restrict__ block_sums, int nb, long long n, int *__restrict__ counts,
                                                                    int *__restrict__ counts_out)
{
    __shared__ int tot[GR_THREADS];
    const int per = (nb + GR_THREADS - 1) / GR_THREADS;
    const int b0 = min(nb, (int)threadIdx.x * per), b1 = min(nb, b0 + per);
    int s = 0;
    for (int b = b0; b < b1; b++) s += block_sums[b];
    tot[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < GR_THREADS; t++) { const int v = tot[t]; tot[t] = run; run += v; }
        const int keep = (int)(n - run);
        counts[EX4D_CNT_KEEP] = keep;
        for (int k = EX4D_CNT_CLONE_SEL; k < EX4D_CNT_ROWS; k++) counts[k] = 0;
        counts[EX4D_CNT_ROWS] = keep;
        counts_out[0] = run;
        counts_out[1] = keep;
    }
    __syncthreads();
    int run = tot[threadIdx.x];
    for (int b = b0; b < b1; b++) { const int v = block_sums[b]; block_sums[b] = run; run += v; }
}

__global__ __launch_bounds__(GR_THREADS) void classify_map_kernel(long long n, const unsigned char *__restrict__ flags, const int *__restrict__ block_off,
                                                                   int *__restrict__ map, int *__restrict__ selected)
{
    __shared__ int sc[GR_THREADS];
    const long long i = (long long)blockIdx.x * GR_THREADS + threadIdx.x;
    const int mine = i < n ? flags[i] : 0;
    sc[threadIdx.x] = mine;
    __syncthreads();
    for (int s = 1; s < GR_THREADS; s <<= 1) {
        const int v = threadIdx.x >= s ? sc[threadIdx.x - s] : 0;
        __syncthreads();
        sc[threadIdx.x] += v;
        __syncthreads();
    }
    if (i >= n) return;
    const int before = block_off[blockIdx.x] + sc[threadIdx.x] - mine;       // selected rows before this one
    int4 d, w;
    d.x = mine ? -1 : (int)(i - before);
    d.y = d.z = d.w = -1;
    w.x = w.y = w.z = w.w = -1;
    int4 *m = (int4 *)(map + (size_t)i * EX4D_PLAN_MAP_INTS);
    m[0] = d;
    m[1] = w;
    if (mine) selected[before] = (int)i;
}

// ---------------------------------------------------------------------------------------------------------------- append
struct AppendSlot {
    Ex4dGrowthTensor t;
    long long numel;                 // destination elements
    unsigned first_chunk;
};
struct AppendArgs {
    AppendSlot slot[EX4D_GROWTH_MAX_TENSORS];
    Ex4dGrowthAppend g;
    int count;
};

__device__ __forceinline__ float clamp_lo_hi(float x, float lo, float hi)
{
    const float y = x < lo ? lo : x;      // torch.clamp: min(max(x, lo), hi), a NaN stays
    return y > hi ? hi : y;
}

__global__ __launch_bounds__(GR_THREADS) void growth_append_kernel(const AppendArgs a)
{
    int t = 0;
#pragma unroll 1
    for (int k = 1; k < a.count; k++) if (blockIdx.x >= a.slot[k].first_chunk) t = k;
    const AppendSlot &s = a.slot[t];
    const Ex4dGrowthTensor &d = s.t;
    const Ex4dGrowthAppend &g = a.g;
    const long long base = (long long)(blockIdx.x - s.first_chunk) * GR_APPEND_CHUNK;
    const long long end = s.numel - base < GR_APPEND_CHUNK ? s.numel : base + GR_APPEND_CHUNK;
    const long long dst_rows = d.old_rows + g.n_new;
#pragma unroll 1
    for (long long e = base + threadIdx.x; e < end; e += GR_THREADS) {
        float v;
        if (d.rule == EX4D_GROW_STATS) {
            const long long plane = e / dst_rows, row = e - plane * dst_rows;
            if (plane <= EX4D_STAT_MIN_RADII) v = plane == EX4D_STAT_MIN_RADII ? 1000.f : 0.f;      // "reset grad anyway": old and new rows
            else if (row < d.old_rows) v = d.old[plane * d.old_rows + row];
            else v = plane == EX4D_STAT_ERROR_MIN ? 1000.f : -1.f;
            d.dst[e] = v;
            continue;
        }
        const long long row = e / d.width;
        const int col = (int)(e - row * d.width);
        if (row < d.old_rows) { d.dst[e] = d.old[e]; continue; }
        const long long src = g.selected[row - d.old_rows];
        switch (d.rule) {
        case EX4D_GROW_COPY: v = d.src0[src * d.width + col]; break;
        case EX4D_GROW_XYZ: {
            // torch's bilinear resize (align_corners = False) of the two end points to K samples along the keyframe axis
            const int k = col / 3, c = col - 3 * k;
            const float x = d.src0[src * 3 + c], dv = d.src1[src * 3 + c];
            const float p0 = x - dv * g.interval / g.max_dur;
            const float p1 = x + dv * g.b_scale;
            const float scale = 2.f / (float)g.K;
            float at = scale * ((float)k + 0.5f) - 0.5f;
            at = at < 0.f ? 0.f : at;
            if (at < 1.f) v = (1.f - at) * p0 + at * p1;
            else v = p1;
            break;
        }
        case EX4D_GROW_ROTATION: v = d.src0[src * 4 + (col & 3)]; break;
        case EX4D_GROW_CENTER: {
            const float ts = g.stats[EX4D_STAT_ERROR_MIN_T * g.n_static + src];
            const float c = col == 0 ? (ts / 2.f + g.time_shift) / g.interval
                                     : ((g.max_dur + (ts < 0.f ? 0.f : ts)) / 2.f + g.time_shift) / g.interval;
            v = clamp_lo_hi(c, g.center_lo, g.center_hi);
            break;
        }
        case EX4D_GROW_VAR: {
            const float ts = g.stats[EX4D_STAT_ERROR_MIN_T * g.n_static + src];
            v = col == 0 ? ts + g.time_pad : g.max_dur - ts + g.time_pad;
            break;
        }
        default: v = 0.f; break;                                              // EX4D_GROW_ZERO
        }
        d.dst[e] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- expansion
// one wave per dynamic row: its K keyframes copied, the new ones extrapolated from the last one
__global__ __launch_bounds__(GR_THREADS) void growth_extrapolate_kernel(const float *__restrict__ src, float *__restrict__ dst, long long rows, int K,
                                                                         int K2, int C, int avg)
{
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (GR_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float *x = src + row * K * C;
    float *y = dst + row * K2 * C;
    for (int e = lane; e < K * C; e += 64) y[e] = x[e];
    for (int e = lane; e < (K2 - K) * C; e += 64) {
        const int j = e / C + 1, c = e - (j - 1) * C;
        const float anchor = x[(K - avg - 1) * C + c];
        float sum = 0.f;
        for (int q = 0; q < avg; q++) sum = sum + (x[(K - avg + q) * C + c] - anchor);
        const float diff = sum / (float)avg;
        y[(K - 1 + j) * C + c] = (float)j * diff + x[(K - 1) * C + c];
    }
}

__global__ __launch_bounds__(GR_THREADS) void growth_expand_opacity_kernel(const float2 *__restrict__ center, const float2 *__restrict__ var,
                                                                            float2 *__restrict__ center_out, float2 *__restrict__ var_out, long long rows,
                                                                            float shift, float late, float center_max)
{
    for (long long i = (long long)blockIdx.x * GR_THREADS + threadIdx.x; i < rows; i += (long long)gridDim.x * GR_THREADS) {
        const float2 c = center[i];
        float2 v = var[i];
        if ((c.x + shift > late) || (c.y + shift > late)) v.y = 1.f;
        float2 o;
        o.x = c.x > center_max ? center_max : c.x;
        o.y = c.y > center_max ? center_max : c.y;
        center_out[i] = o;
        var_out[i] = v;
    }
}

__global__ __launch_bounds__(GR_THREADS) void growth_adjust_opacity_kernel(const float2 *__restrict__ center, const float2 *__restrict__ var,
                                                                            float2 *__restrict__ center_out, float2 *__restrict__ var_out, long long rows,
                                                                            float lo, float hi)
{
    for (long long i = (long long)blockIdx.x * GR_THREADS + threadIdx.x; i < rows; i += (long long)gridDim.x * GR_THREADS) {
        const float2 c = center[i], v = var[i];
        float2 n = v;
        if ((c.x > hi) || (c.y > hi)) n.y = (v.y < 1.f ? 1.f : v.y) * 2.f;
        if ((c.x < lo) || (c.y < lo)) n.x = (v.x < 1.f ? 1.f : v.x) * 2.f;
        if (v.x < 0.5f) n.x = 0.5f;                                           // the test reads the OLD var and overrides the doubling
        if (v.y < 0.5f) n.y = 0.5f;
        float2 o;
        o.x = clamp_lo_hi(c.x, lo, hi);
        o.y = clamp_lo_hi(c.y, lo, hi);
        center_out[i] = o;
        var_out[i] = n;
    }
}

}  // namespace

extern "C" {

int ex4d_growth_scores(const float *xyz, const float *disp, const uint8_t *vis, const float *cam, int64_t n, float *score, void *stream)
{
    clear_error();
    if (n < 0 || (n > 0 && (!xyz || !disp || !vis || !cam || !score))) return fail(EX4D_ERR_ARG, "growth_scores: negative size or null pointer");
    if (n == 0) return EX4D_OK;
    hipLaunchKernelGGL(growth_scores_kernel, dim3(grid_for(n)), dim3(GR_THREADS), 0, (hipStream_t)stream, xyz, disp, vis, cam, (long long)n, score);
    return launch_status("growth_scores");
}

size_t ex4d_growth_select_scratch_bytes(void) { return ex4d_align_up(SS_WORDS * sizeof(unsigned)); }

int ex4d_growth_select(const float *score, int64_t n, float q, float *result, void *scratch, void *stream_)
{
    clear_error();
    if (n < 0 || n > 0x7fffffffLL || !result || !scratch || (n > 0 && !score) || !(q >= 0.f && q <= 1.f))
        return fail(EX4D_ERR_ARG, "growth_select: bad size, null pointer or q outside [0, 1]");
    hipStream_t stream = (hipStream_t)stream_;
    unsigned *ws = (unsigned *)scratch;
    if (hipMemsetAsync(ws, 0, SS_WORDS * sizeof(unsigned), stream) != hipSuccess) return fail(EX4D_ERR_HIP, "growth_select: memset failed");
    const unsigned grid = grid_for(n);
    for (int pass = 0; pass < 4; pass++) {
        hipLaunchKernelGGL(select_hist_kernel, dim3(grid), dim3(GR_THREADS), 0, stream, score, (long long)n, pass, ws);
        hipLaunchKernelGGL(select_pick_kernel, dim3(1), dim3(GR_THREADS), 0, stream, pass, q, ws);
    }
    hipLaunchKernelGGL(select_next_kernel, dim3(grid), dim3(GR_THREADS), 0, stream, score, (long long)n, ws);
    hipLaunchKernelGGL(select_finish_kernel, dim3(1), dim3(64), 0, stream, (const unsigned *)ws, result);
    return launch_status("growth_select");
}

int ex4d_growth_classify(const Ex4dGrowthClassify *args, void *stream_)
{
    clear_error();
    if (!args) return fail(EX4D_ERR_ARG, "growth_classify: null arguments");
    const Ex4dGrowthClassify &G = *args;
    if (G.n < 0 || G.n > 0x7fffffffLL - 1 || !G.counts || !G.counts_out ||
        (G.n > 0 && (!G.score || !G.result || !G.disp || !G.stats || !G.map || !G.selected || !G.scratch)))
        return fail(EX4D_ERR_ARG, "growth_classify: bad size or null pointer");
    hipStream_t stream = (hipStream_t)stream_;
    if (G.n == 0) {
        if (hipMemsetAsync(G.counts, 0, EX4D_PLAN_COUNTS * sizeof(int32_t), stream) != hipSuccess ||
            hipMemsetAsync(G.counts_out, 0, 2 * sizeof(int32_t), stream) != hipSuccess)
            return fail(EX4D_ERR_HIP, "growth_classify: memset failed");
        return EX4D_OK;
    }
    ClassifyArgs a;
    a.n = G.n; a.score = G.score; a.result = G.result; a.disp = G.disp; a.stats = G.stats; a.motion_abs = G.motion_abs; a.min_abs = G.min_abs;
    const long long nb = (G.n + GR_THREADS - 1) / GR_THREADS;
    unsigned char *flags = (unsigned char *)G.scratch;                         // the layout ex4d_densify_scratch_bytes sizes: n bytes, then 8 ints per block
    int *block_sums = (int *)((char *)G.scratch + ex4d_align_up((size_t)G.n));
    hipLaunchKernelGGL(classify_flags_kernel, dim3((unsigned)nb), dim3(GR_THREADS), 0, stream, a, flags, block_sums);
    hipLaunchKernelGGL(classify_scan_kernel, dim3(1), dim3(GR_THREADS), 0, stream, block_sums, (int)nb, (long long)G.n, (int *)G.counts, (int *)G.counts_out);
    hipLaunchKernelGGL(classify_map_kernel, dim3((unsigned)nb), dim3(GR_THREADS), 0, stream, (long long)G.n, (const unsigned char *)flags,
                       (const int *)block_sums, (int *)G.map, (int *)G.selected);
    return launch_status("growth_classify");
}

int ex4d_growth_append(const Ex4dGrowthTensor *tensors, int32_t count, const Ex4dGrowthAppend *args, void *stream_)
{
    clear_error();
    if (count < 0 || count > EX4D_GROWTH_MAX_TENSORS || !args || (count > 0 && !tensors))
        return fail(EX4D_ERR_ARG, "growth_append: count outside [0, EX4D_GROWTH_MAX_TENSORS] or null pointer");
    const Ex4dGrowthAppend &g = *args;
    if (g.n_new < 0 || g.n_static < g.n_new || (g.n_new > 0 && !g.selected) || g.K < 1)
        return fail(EX4D_ERR_ARG, "growth_append: bad row counts, null selection or K < 1");
    AppendArgs a;
    a.count = 0;
    a.g = g;
    unsigned chunks = 0;
    for (int i = 0; i < count; i++) {
        const Ex4dGrowthTensor &t = tensors[i];
        const bool stats = t.rule == EX4D_GROW_STATS;
        const bool reads_stats = t.rule == EX4D_GROW_CENTER || t.rule == EX4D_GROW_VAR;
        if (t.old_rows < 0 || t.width < 1 || t.rule < EX4D_GROW_COPY || t.rule > EX4D_GROW_STATS || (t.old_rows > 0 && !t.old) ||
            (stats && t.width != 1) || (t.rule == EX4D_GROW_XYZ && t.width != 3 * g.K) || (t.rule == EX4D_GROW_ROTATION && t.width != 4 * g.K) ||
            (reads_stats && t.width != 2) ||
            (g.n_new > 0 && ((reads_stats && !g.stats) || ((t.rule == EX4D_GROW_COPY || t.rule == EX4D_GROW_XYZ || t.rule == EX4D_GROW_ROTATION) && !t.src0) ||
                             (t.rule == EX4D_GROW_XYZ && !t.src1)))) {
            char text[96];
            snprintf(text, sizeof(text), "growth_append: tensor %d: bad shape, rule or null pointer", i);
            return fail(EX4D_ERR_ARG, text);
        }
        const long long numel = (stats ? (long long)EX4D_DENSIFY_STATS : (long long)t.width) * (t.old_rows + g.n_new);
        if (numel == 0) continue;
        if (!t.dst) return fail(EX4D_ERR_ARG, "growth_append: null destination");
        AppendSlot &s = a.slot[a.count++];
        s.t = t; s.numel = numel; s.first_chunk = chunks;
        const long long c = (numel + GR_APPEND_CHUNK - 1) / GR_APPEND_CHUNK;
        if (c + chunks > 0x7fffffffLL) return fail(EX4D_ERR_ARG, "growth_append: too many elements for one launch");
        chunks += (unsigned)c;
    }
    if (chunks == 0) return EX4D_OK;
    hipLaunchKernelGGL(growth_append_kernel, dim3(chunks), dim3(GR_THREADS), 0, (hipStream_t)stream_, a);
    return launch_status("growth_append");
}

int ex4d_growth_extrapolate(const float *src, float *dst, int64_t rows, int32_t K, int32_t K2, int32_t C, int32_t avg, void *stream)
{
    clear_error();
    if (rows < 0 || C < 1 || avg < 1 || avg >= K || K2 <= K || (rows > 0 && (!src || !dst)) || rows > 0x7fffffffLL)
        return fail(EX4D_ERR_ARG, "growth_extrapolate: needs 1 <= avg < K < K2, C >= 1 and non-null tensors");
    if (rows == 0) return EX4D_OK;
    const long long nb = (rows + GR_THREADS / 64 - 1) / (GR_THREADS / 64);
    hipLaunchKernelGGL(growth_extrapolate_kernel, dim3((unsigned)nb), dim3(GR_THREADS), 0, (hipStream_t)stream, src, dst, (long long)rows, (int)K, (int)K2,
                       (int)C, (int)avg);
    return launch_status("growth_extrapolate");
}

int ex4d_growth_expand_opacity(const float *center, const float *var, float *center_out, float *var_out, int64_t rows, float shift, float late,
                               float center_max, void *stream)
{
    clear_error();
    if (rows < 0 || (rows > 0 && (!center || !var || !center_out || !var_out))) return fail(EX4D_ERR_ARG, "growth_expand_opacity: negative size or null pointer");
    if (rows == 0) return EX4D_OK;
    hipLaunchKernelGGL(growth_expand_opacity_kernel, dim3(grid_for(rows)), dim3(GR_THREADS), 0, (hipStream_t)stream, (const float2 *)center, (const float2 *)var,
                       (float2 *)center_out, (float2 *)var_out, (long long)rows, shift, late, center_max);
    return launch_status("growth_expand_opacity");
}

int ex4d_growth_adjust_opacity(const float *center, const float *var, float *center_out, float *var_out, int64_t rows, float lo, float hi, void *stream)
{
    clear_error();
    if (rows < 0 || (rows > 0 && (!center || !var || !center_out || !var_out))) return fail(EX4D_ERR_ARG, "growth_adjust_opacity: negative size or null pointer");
    if (rows == 0) return EX4D_OK;
    hipLaunchKernelGGL(growth_adjust_opacity_kernel, dim3(grid_for(rows)), dim3(GR_THREADS), 0, (hipStream_t)stream, (const float2 *)center, (const float2 *)var,
                       (float2 *)center_out, (float2 *)var_out, (long long)rows, lo, hi);
    return launch_status("growth_adjust_opacity");
}

}  // extern "C"
