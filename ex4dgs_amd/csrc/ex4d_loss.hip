// Fused L1 + SSIM loss, forward and backward, for gfx950.
//
// Replaces l1_loss + ssim/_ssim of the reference (utils/loss_utils.py:22-25, :47-81; used at train.py:144-151) and their
// autograd graph: five depthwise 11x11 conv2d forward, their transposes backward, ~25 element-wise kernels.  Measured on
// MI355X at 1352x1014 the torch version costs 11.7 ms per iteration -- ten times the rasterizer it scores.
//
// The 11x11 window is the outer product of a 1-D Gaussian, so every convolution is separable.  Round 4: ROLLING WINDOW.  A workgroup
// owns a strip of 64 output columns and walks down a segment of SEG = 48 output rows, four image rows per iteration: the rows' 11-tap row
// pass (five moment maps x, y, x^2, y^2, xy per channel in the forward, the three derivative maps in the backward) goes into a ring of
// 16 rows in LDS, the column pass of the four output rows whose window is now complete reads 11 ring rows each.  Every input row is
// read ONCE per strip (rounds 2-3: 16x16 output tiles with a 26x26 halo each read 2.6x the image, and their 104-byte halo rows pulled
// whole 128-byte lines: 237 / 364 MB of HBM traffic per launch against 93 / 98 MB of algorithmic bytes); what is left is the 10-column
// overlap of neighbouring strips (74 / 64; neighbouring strips are given to the SAME XCD back to back, so most of it hits in that
// XCD's L2) and the 10 warm-up rows of a segment (74 / 64).  The next iteration's rows are in flight (registers) while the current
// one is convolved; two workgroup barriers per iteration (the row buffers alternate).
// Forward emits the loss partial sums, the two error maps and, per pixel and channel, the three partial derivatives of the SSIM map
// the backward needs; backward convolves those three maps with the same (symmetric) window and combines them with the pixel values:
//     d(sum ssim)/dx_p = conv(A)_p + 2 x_p conv(B)_p + y_p conv(C)_p,   A = dS/dmu1, B = dS/dE[x^2], C = dS/dE[xy].
//
// THE SCHEME IS WRITTEN ONCE (Stage, Tile, walk, block_sum below) and the four kernels -- the loss's forward and backward, and the two
// that score a rendered view, frame_metrics_kernel and frame_skssim_kernel -- pass in what differs: the maps they stage (ImagePair,
// DerivMaps), their row pass and their column pass.
//
// GROUND TRUTH AS DECODED (ex4d_l1_ssim_*_u8): the kernels are templates over the ground truth's element type -- float32 [C,H,W] planes,
// or uint8 [H,W,S] pixels (S = 3 or 4, as an image decoder leaves them) looked up in a 256-entry float table, which the uint8
// instantiations take as one more kernel argument.  Everything behind the load is the same code, so the two agree bit for bit on equal
// values; the float instantiations keep the signature and the loads they had.  THE TABLE travels in the kernel
// arguments (1 KB by value, as the 11 window taps do) and every workgroup copies it into LDS with one load per thread: the call
// allocates nothing, copies nothing host-to-device, does not synchronise, and a captured graph holds the table by value.  A table in
// global memory would need a per-call upload or an owner; constant-indexed kernel arguments cannot be indexed per lane.  LDS: 76 064 +
// 1 024 B forward, 58 752 + 1 024 B backward, both within the 80 KB of two workgroups per CU.  The bytes are fetched with byte loads
// (any alignment: frame i of a resident [N,H,W,3] store starts at an odd address for odd H W); the forward keeps the BYTE in flight
// across the convolution and looks it up when the row is committed to LDS, so the global load stays hidden as the float one is.
#include "ex4d_internal.h"
#include "../../include/ex4d_loss.h"
#include <cstdio>

namespace {

#define LH 5                        // window half width
#define SW 64                       // output columns of a strip
#define SIN (SW + 2 * LH)           // 74 input columns
#define SEG 48                      // output rows of a segment (22 x 22 = 484 workgroups at 1352x1014: one round at 2 per CU)
#define RPI 4                       // image rows per iteration (256 threads = RPI rows x SW columns)
#define RING 16                     // rows of row-pass results kept in LDS (>= 11 + RPI - 1, power of two)
#define CG 3                        // channels convolved together (the reference's images are RGB; more channels run in groups)

struct Window { float w[EX4D_SSIM_WINDOW]; };

// uint8 ground truth: what the _u8 instantiations take as their LAST kernel argument (the float ones have no such argument and keep the
// signature, and so the code, they had): bytes per pixel and the value of each byte
struct PixelTable { int S; float v[256]; };
struct PixelLds { const float *v; int S; };             // the workgroup's copy

// 256 threads, one entry each; the caller's next barrier publishes it.  (A function of its own so that only the _u8 instantiations own
// the 1 KB.)
__device__ __forceinline__ PixelLds table_to_lds(const PixelTable &t)
{
    __shared__ float s_table[256];
    s_table[threadIdx.x] = t.v[threadIdx.x];
    return PixelLds{ s_table, t.S };
}
__device__ __forceinline__ PixelLds table_to_lds() { return PixelLds{ nullptr, 0 }; }

// a byte in flight in a float register: its value as the register's bits, -1 for zero padding (conv2d padding=5 is the float 0, never v[0])
__device__ __forceinline__ float byte_bits(bool ok, const uint8_t *__restrict__ p, size_t o) { return __int_as_float(ok ? (int)p[o] : -1); }
__device__ __forceinline__ float byte_value(float bits, const float *v) { const int u = __float_as_int(bits); return u >= 0 ? v[u] : 0.f; }

// workgroup -> (strip, segment): consecutive workgroup ids round-robin over the 8 XCDs, so XCD x takes the contiguous run of work items
// [x * per, (x + 1) * per) in row-major (segment, strip) order: horizontally neighbouring strips share their halo columns in one L2
__device__ __forceinline__ int work_item_of_block(int nwork)
{
    const int per = (nwork + 7) >> 3;
    return (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
}

// ---- the static LDS of a kernel: the double buffer of an iteration's rows, NMAP staged maps of CG channels with HALF halo columns per
// side (+ 2 columns of padding), and the ring of NRING row-pass results per channel.  It exceeds the 64 KB a workgroup may take on
// older parts and is sized for gfx950's 160 KB per CU (two workgroups per CU): this file builds for gfx950-class LDS only
template <int NMAP, int NRING, int HALF>
struct Stage {
    static_assert(RING >= 2 * HALF + RPI && (RING & (RING - 1)) == 0, "the ring holds a window and an iteration");
    static_assert(RPI * 2 * HALF <= 256, "one halo load per thread");
    float in[2][NMAP][CG][RPI][SW + 2 * HALF + 2];      // [buffer][map][channel][row][column]
    float ring[CG][NRING][RING][SW];                    // row-pass results of the last RING image rows
};

// a kernel's whole LDS: its Stage, the NSUMS x 4 floats of its block_sum and, in a _u8 instantiation, the workgroup's copy of the table
template <typename St, int NSUMS, typename... Table>
constexpr bool two_workgroups_per_cu = sizeof(St) + NSUMS * 4 * sizeof(float) + (sizeof(Table::v) + ... + 0) <= 80 * 1024;

// ---- a workgroup's tile and a thread's roles in it.  Work item wi is strip wi % nsx, segment wi / nsx of an Ho x Wo output domain;
// output (oy, ox) reads image rows oy - HALF .. oy + HALF and the same columns where the image is PADDED with zeros (the 11-tap
// kernels), rows oy .. oy + 2 HALF and the same columns, all inside the image, where it is not (the output domain is the image less
// HALF pixels per side).  An iteration's rows: every thread takes column (tid & 63) of row (tid >> 6) in every plane (map x channel),
// threads 0 .. RPI * 2 HALF - 1 also one of the RPI x 2 HALF halo columns 64 .. -- two loads per plane with ONE pixel offset each (a
// flat element index decoded per load kept ~100 registers of hoisted address arithmetic alive)
template <int HALF, bool PADDED>
struct Tile {
    int col, rsub, hrow, hcol;
    bool has_halo;
    int x0, y0;                     // first output column / row
    int xr, yr;                     // first image column / row read
    int rows_out, n_in, n_it;       // output rows, image rows read (rows_out + 2 HALF), iterations
    int px, Wo;                     // this thread's output column; the output domain's width
    __device__ __forceinline__ Tile(int wi, int nsx, int Ho, int Wo_) : Wo(Wo_)
    {
        col = threadIdx.x & (SW - 1); rsub = threadIdx.x >> 6;
        hrow = (int)threadIdx.x / (2 * HALF); hcol = SW + (int)threadIdx.x % (2 * HALF);
        has_halo = threadIdx.x < RPI * 2 * HALF;
        x0 = (wi % nsx) * SW; y0 = (wi / nsx) * SEG;
        xr = x0 - (PADDED ? HALF : 0); yr = y0 - (PADDED ? HALF : 0);
        rows_out = (Ho - y0) < SEG ? (Ho - y0) : SEG;
        n_in = rows_out + 2 * HALF;
        n_it = (n_in + RPI - 1) / RPI;
        px = x0 + col;
    }
    // row ro of the segment (of this thread's column) is an output pixel
    __device__ __forceinline__ bool is_output(int ro) const { return ro >= 0 && ro < rows_out && px < Wo; }
};

// ---- what a walk stages.  load(map, channel, in_image, pixel offset) is the value kept in flight, commit(map, main, halo) makes of a
// thread's two values of a plane what goes to LDS (both under ONE test of a uniform condition: the compiler then keeps it a branch).
// The image and the ground truth of channels c0 .. c0 + nc - 1: float planes, or (the ground truth of a _u8 instantiation) the byte,
// which stays in flight and is looked up at commit.  Beyond the image a plane is 0 (conv2d padding=5; frame_skssim_kernel's feed
// masked outputs only).  clamp01: the image is clamped to [0,1] as torch.clamp does -- a NaN stays a NaN, the padding's 0 stays 0
template <typename T>
struct ImagePair {
    static constexpr bool kBytes = sizeof(T) == 1;
    const float *__restrict__ img;
    const T *__restrict__ gt;
    size_t HW;
    PixelLds px8;
    int c0, nc;
    bool clamp01;
    __device__ __forceinline__ float load(int map, int ch, bool ok, size_t o) const
    {
        ok = ok && ch < nc;
        if constexpr (kBytes) {
            if (map) return byte_bits(ok, gt, o * px8.S + (c0 + ch));
        }
        const float *src = (map ? (const float *)gt : img) + (size_t)(c0 + ch) * HW;
        return ok ? src[o] : 0.f;
    }
    __device__ __forceinline__ void commit(int map, float &vm, float &vh) const
    {
        if (map) {
            if constexpr (kBytes) { vm = byte_value(vm, px8.v); vh = byte_value(vh, px8.v); }
        } else if (clamp01) {
            const float a = vm, b = vh;                  // (arms that are values stay selects; read through the references they
            vm = a < 0.f ? 0.f : (a > 1.f ? 1.f : a);    // become divergent branches: 1 us of frame_skssim's 43)
            vh = b < 0.f ? 0.f : (b > 1.f ? 1.f : b);
        }
    }
};

// the forward's three derivative maps [3][C][H][W], channels c0 .. c0 + nc - 1
struct DerivMaps {
    const float *__restrict__ dmaps;
    size_t HW;
    int C, c0, nc;
    __device__ __forceinline__ float load(int map, int ch, bool ok, size_t o) const
    {
        const float *src = dmaps + ((size_t)map * C + c0 + ch) * HW;
        return (ok && ch < nc) ? src[o] : 0.f;
    }
    __device__ __forceinline__ void commit(int, float &, float &) const {}
};

// ---- the walk down a segment.  row_pass(buf, rin) convolves image row rin (relative to the first row read) of buffer buf into the
// ring, col_pass(ro) takes output row ro, whose window (ring rows ro .. ro + 2 HALF) is complete.  The leading barrier: the previous
// channel group is done with both buffers and the ring, and a _u8 instantiation's table is published
template <int NMAP, int NRING, int HALF, bool PADDED, typename Maps, typename RowPass, typename ColPass>
__device__ __forceinline__ void walk(const Tile<HALF, PADDED> &t, int H, int W, Stage<NMAP, NRING, HALF> &s, const Maps &maps,
                                     RowPass row_pass, ColPass col_pass)
{
    float rm[NMAP * CG], rh[NMAP * CG];
    auto fetch = [&](int it) {
        const int ym = t.yr + it * RPI + t.rsub, xm = t.xr + t.col;
        const int yh = t.yr + it * RPI + t.hrow, xh = t.xr + t.hcol;
        const bool okm = xm >= 0 && xm < W && ym >= 0 && ym < H, okh = t.has_halo && xh >= 0 && xh < W && yh >= 0 && yh < H;
        const size_t om = (size_t)ym * W + xm, oh = (size_t)yh * W + xh;
#pragma unroll
        for (int pl = 0; pl < NMAP * CG; pl++) {
            rm[pl] = maps.load(pl / CG, pl % CG, okm, om);
            rh[pl] = maps.load(pl / CG, pl % CG, okh, oh);
        }
    };
    auto commit = [&](int buf) {
#pragma unroll
        for (int pl = 0; pl < NMAP * CG; pl++) {
            float vm = rm[pl], vh = rh[pl];
            maps.commit(pl / CG, vm, vh);
            s.in[buf][pl / CG][pl % CG][t.rsub][t.col] = vm;
            if (t.has_halo) s.in[buf][pl / CG][pl % CG][t.hrow][t.hcol] = vh;
        }
    };
    __syncthreads();
    fetch(0);
    commit(0);
    __syncthreads();
    for (int it = 0; it < t.n_it; it++) {
        const int buf = it & 1;
        if (it + 1 < t.n_it) fetch(it + 1);             // in flight while this iteration's rows are convolved
        const int rin = it * RPI + t.rsub;
        if (rin < t.n_in) row_pass(buf, rin);
        __syncthreads();
        const int ro = rin - 2 * HALF;
        if (t.is_output(ro)) col_pass(ro);
        if (it + 1 < t.n_it) commit(buf ^ 1);
        __syncthreads();
    }
}

// ---- the 11-tap pieces.  The row pass of one channel: the five moment maps x, y, x^2, y^2, xy of the windows that start at sx, sy
__device__ __forceinline__ void moments_row(const Window &win, const float *sx, const float *sy, float (&m)[5])
{
    float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
    for (int k = 0; k < EX4D_SSIM_WINDOW; k++) {
        const float a = sx[k], b = sy[k], wk = win.w[k];
        m1 += wk * a; m2 += wk * b; e11 += wk * (a * a); e22 += wk * (b * b); e12 += wk * (a * b);
    }
    m[0] = m1; m[1] = m2; m[2] = e11; m[3] = e22; m[4] = e12;
}

// the column pass of one channel's N ring maps at output row ro
template <int N>
__device__ __forceinline__ void taps_col(const Window &win, const float (&ring)[N][RING][SW], int ro, int col, float (&m)[N])
{
#pragma unroll
    for (int q = 0; q < N; q++) m[q] = 0.f;
#pragma unroll
    for (int k = 0; k < EX4D_SSIM_WINDOW; k++) {
        const float wk = win.w[k];
        const int slot = (ro + k) & (RING - 1);
#pragma unroll
        for (int q = 0; q < N; q++) m[q] += wk * ring[q][slot][col];
    }
}

template <int N>
__device__ __forceinline__ void ring_put(float (&ring)[N][RING][SW], int rin, int col, const float (&m)[N])
{
#pragma unroll
    for (int q = 0; q < N; q++) ring[q][rin & (RING - 1)][col] = m[q];
}

// utils/loss_utils.py:61-74 from the window's five moments (mu1, mu2, E[x^2], E[y^2], E[xy])
struct Ssim { float a1, a2, b1, b2, inv, S; };
__device__ __forceinline__ Ssim ssim_of(const float (&m)[5])
{
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    const float mu1 = m[0], mu2 = m[1], e11 = m[2], e22 = m[3], e12 = m[4];
    const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
    const float s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu12;
    const float a1 = 2.f * mu12 + C1, a2 = 2.f * s12 + C2, b1 = mu1_sq + mu2_sq + C1, b2 = s1 + s2 + C2;
    const float inv = 1.f / (b1 * b2);
    return Ssim{ a1, a2, b1, b2, inv, (a1 * a2) * inv };
}

// ---- N sums over the workgroup's 256 threads: wave shuffle, then LDS; every thread returns with the four waves' totals added in a
// fixed order (no single-address atomics: they serialise ~12 ns each)
template <typename V, int N>
__device__ __forceinline__ void block_sum(V (&v)[N])
{
    __shared__ V s[N][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < N; q++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_xor(v[q], o, 64);
        if (lane == 0) s[q][wave] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < N; q++) v[q] = s[q][0] + s[q][1] + s[q][2] + s[q][3];
}

// a workgroup's N float partial sums -> partials[N * workgroup ..]
template <int N>
__device__ __forceinline__ void put_partials(float (&v)[N], float *__restrict__ partials)
{
    block_sum(v);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < N; q++) partials[N * blockIdx.x + q] = v[q];
    }
}

// the one workgroup of a finish kernel: the N columns of the workgroups' partials, added in double
template <int N>
__device__ __forceinline__ void sum_partials(int nblocks, const float *__restrict__ partials, double (&sum)[N])
{
#pragma unroll
    for (int q = 0; q < N; q++) sum[q] = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) {
#pragma unroll
        for (int q = 0; q < N; q++) sum[q] += (double)partials[N * i + q];
    }
    block_sum(sum);
}

template <typename T, typename... Table>
__global__ __launch_bounds__(256) void l1_ssim_fwd_kernel(int C, int H, int W, const float *__restrict__ img,
    const T *__restrict__ gt, Window win, float *__restrict__ l1_errors, float *__restrict__ ssim_errors,
    float *__restrict__ dmaps, float *__restrict__ partials, int nsx, int nsy, Table... table)
{
    using St = Stage<2, 5, LH>;                          // maps x | y; five moment maps
    static_assert(two_workgroups_per_cu<St, 2, Table...>, "l1_ssim_fwd_kernel: two workgroups per CU need <= 80 KB of LDS each");
    __shared__ St s;
    const PixelLds px8 = table_to_lds(table...);
    const int nwork = nsx * nsy;
    const int wi = work_item_of_block(nwork);
    const size_t HW = (size_t)H * W;
    float sums[2] = { 0.f, 0.f };                        // L1, SSIM
    if (wi < nwork) {
        const Tile<LH, true> t(wi, nsx, H, W);
        for (int c0 = 0; c0 < C; c0 += CG) {
            const int nc = (C - c0) < CG ? (C - c0) : CG;
            // an error map over the channel groups: the first stores, the others add, the last divides by C
            auto put_error = [&](float *map, int ro, float v) {
                if (!map) return;
                float *o = map + (size_t)(t.y0 + ro) * W + t.px;
                if (c0 != 0) v = *o + v;
                *o = (c0 + CG >= C) ? v / (float)C : v;
            };
            walk(t, H, W, s, ImagePair<T>{ img, gt, HW, px8, c0, nc, false },
                // ---- row pass: five moment maps per channel -> ring; the L1 term of the pixels of this row (they are output pixels when
                // the row lies inside the segment)
                [&](int buf, int rin) {
                    float l1 = 0.f;
#pragma unroll 1
                    for (int ch = 0; ch < nc; ch++) {
                        const float *sx = &s.in[buf][0][ch][t.rsub][t.col], *sy = &s.in[buf][1][ch][t.rsub][t.col];
                        float m[5];
                        moments_row(win, sx, sy, m);
                        ring_put(s.ring[ch], rin, t.col, m);
                        l1 += fabsf(sx[LH] - sy[LH]);
                    }
                    const int ro = rin - LH;             // this image row as an output row of the segment
                    if (t.is_output(ro)) {
                        sums[0] += l1;
                        put_error(l1_errors, ro, l1);
                    }
                },
                // ---- column pass: the SSIM map's value and its three partial derivatives
                [&](int ro) {
                    float ssim = 0.f;
#pragma unroll 1
                    for (int ch = 0; ch < nc; ch++) {
                        float m[5];
                        taps_col(win, s.ring[ch], ro, t.col, m);
                        const Ssim q = ssim_of(m);
                        ssim += q.S;
                        // partial derivatives of S w.r.t. (mu1, E[x^2], E[xy]) with the gt-side moments held fixed
                        const float dSda1 = q.a2 * q.inv, dSda2 = q.a1 * q.inv, dSdb1 = -q.S / q.b1, dSdb2 = -q.S / q.b2;
                        const float dA = 2.f * m[1] * (dSda1 - dSda2) + 2.f * m[0] * (dSdb1 - dSdb2);
                        const size_t o = (size_t)(c0 + ch) * HW + (size_t)(t.y0 + ro) * W + t.px;
                        dmaps[o] = dA;
                        dmaps[(size_t)C * HW + o] = dSdb2;
                        dmaps[2 * (size_t)C * HW + o] = 2.f * dSda2;
                    }
                    sums[1] += ssim;
                    put_error(ssim_errors, ro, ssim);
                });
        }
    }
    put_partials(sums, partials);
}

__global__ __launch_bounds__(256) void l1_ssim_finish_kernel(int nblocks, const float *__restrict__ partials, double inv_count,
    float lambda_dssim, float *__restrict__ loss)
{
    double sum[2];
    sum_partials(nblocks, partials, sum);
    if (threadIdx.x == 0) {
        const float l1 = (float)(sum[0] * inv_count), ss = (float)(sum[1] * inv_count);
        loss[0] = (1.0f - lambda_dssim) * l1 + lambda_dssim * (1.0f - ss);      // train.py:145
    }
}

template <typename T, typename... Table>
__global__ __launch_bounds__(256) void l1_ssim_bwd_kernel(int C, int H, int W, const float *__restrict__ img,
    const T *__restrict__ gt, Window win, const float *__restrict__ dmaps, const float *__restrict__ grad_loss,
    float lambda_dssim, float inv_count, float *__restrict__ grad_img, int nsx, int nsy, Table... table)
{
    constexpr bool kBytes = sizeof...(Table) != 0;
    using St = Stage<3, 3, LH>;                          // maps A | B | C; their three convolutions
    static_assert(two_workgroups_per_cu<St, 0, Table...>, "l1_ssim_bwd_kernel: two workgroups per CU need <= 80 KB of LDS each");
    __shared__ St s;
    const int nwork = nsx * nsy;
    const int wi = work_item_of_block(nwork);
    if (wi >= nwork) return;                             // (uniform: the whole workgroup)
    const PixelLds px8 = table_to_lds(table...);        // (read in the column pass, barriers later)
    const size_t HW = (size_t)H * W;
    const float gl = grad_loss[0];
    const Tile<LH, true> t(wi, nsx, H, W);
    for (int c0 = 0; c0 < C; c0 += CG) {
        const int nc = (C - c0) < CG ? (C - c0) : CG;
        walk(t, H, W, s, DerivMaps{ dmaps, HW, C, c0, nc },
            [&](int buf, int rin) {
#pragma unroll 1
                for (int ch = 0; ch < nc; ch++) {
                    const float *sa = &s.in[buf][0][ch][t.rsub][t.col], *sb = &s.in[buf][1][ch][t.rsub][t.col], *sc = &s.in[buf][2][ch][t.rsub][t.col];
                    float m[3] = { 0.f, 0.f, 0.f };
#pragma unroll
                    for (int k = 0; k < EX4D_SSIM_WINDOW; k++) { const float wk = win.w[k]; m[0] += wk * sa[k]; m[1] += wk * sb[k]; m[2] += wk * sc[k]; }
                    ring_put(s.ring[ch], rin, t.col, m);
                }
            },
            [&](int ro) {
#pragma clang loop unroll(disable) vectorize(disable)           // (two channels at a time take 34 registers more)
                for (int ch = 0; ch < nc; ch++) {
                    float m[3];
                    taps_col(win, s.ring[ch], ro, t.col, m);
                    const size_t o = (size_t)(c0 + ch) * HW + (size_t)(t.y0 + ro) * W + t.px;
                    float yv;
                    if constexpr (kBytes) yv = px8.v[gt[((size_t)(t.y0 + ro) * W + t.px) * px8.S + (c0 + ch)]];
                    else yv = gt[o];
                    const float xv = img[o];
                    const float dssim = m[0] + 2.f * xv * m[1] + yv * m[2];              // d(sum of ssim_map)/dx_p
                    const float diff = xv - yv;
                    const float sgn = (diff > 0.f) ? 1.f : ((diff < 0.f) ? -1.f : 0.f);  // d|x - y|/dx
                    grad_img[o] = gl * ((1.0f - lambda_dssim) * sgn * inv_count - lambda_dssim * dssim * inv_count);
                }
            });
    }
}

// ---- SCORING a rendered view (ex4d_frame_metrics*): render.py:64-88 / train.py:313-362 of the reference.  The forward's rolling window
// (same strips, segments, ring and work-item map; C = 3, one channel group) without what only training reads: no dmaps, no error maps,
// so the column pass stores nothing.  The image value is clamped (EX4D_METRICS_CLAMP) when its row is committed to LDS, so every metric
// and the bytes see the clamped value; squared error, non-finite count and the pixel's three bytes come from the centre tap of the
// row pass, where the L1 term comes from.  Four float partial sums per workgroup (a workgroup has at most 48 x 64 x 3 = 9 216 values:
// its count is exact in a float); frame_metrics_finish_kernel adds them in double and writes the row.

// the 8-bit value of an image value.  Default: torch's mul(255).add_(0.5).clamp_(0, 255).to(uint8) -- product and sum are rounded
// SEPARATELY, as the two torch kernels round them (this file is compiled with contraction on: the intrinsics never fuse); trunc:
// (clamp(x, 0, 1) * 255).byte().  A NaN fails every comparison and gives 0 (this library's choice: torch leaves it unspecified).
__device__ __forceinline__ uint8_t metrics_byte(float x, bool trunc)
{
    float t;
    if (trunc) t = __fmul_rn(x < 0.f ? 0.f : (x > 1.f ? 1.f : x), 255.f);
    else t = __fadd_rn(__fmul_rn(x, 255.f), 0.5f);
    return !(t > 0.f) ? (uint8_t)0 : (t >= 255.f ? (uint8_t)255 : (uint8_t)(int)t);
}

template <typename T, typename... Table>
__global__ __launch_bounds__(256) void frame_metrics_kernel(int H, int W, const float *__restrict__ img, const T *__restrict__ gt,
    Window win, int flags, uint8_t *__restrict__ out_u8, float *__restrict__ partials, int nsx, int nsy, Table... table)
{
    using St = Stage<2, 5, LH>;                          // maps x | y; five moment maps
    static_assert(two_workgroups_per_cu<St, 4, Table...>, "frame_metrics_kernel: two workgroups per CU need <= 80 KB of LDS each");
    __shared__ St s;
    const PixelLds px8 = table_to_lds(table...);
    const int nwork = nsx * nsy;
    const int wi = work_item_of_block(nwork);
    const bool clamp01 = (flags & EX4D_METRICS_CLAMP) != 0, trunc = (flags & EX4D_METRICS_QUANT_TRUNC) != 0;
    float sums[4] = { 0.f, 0.f, 0.f, 0.f };              // L1, squared error, SSIM, non-finite count
    if (wi < nwork) {
        const Tile<LH, true> t(wi, nsx, H, W);
        walk(t, H, W, s, ImagePair<T>{ img, gt, (size_t)H * W, px8, 0, CG, clamp01 },
            // ---- row pass -> ring; when the row lies inside the segment its pixels are output pixels: their L1 and squared-error
            // terms, their non-finite count and their bytes
            [&](int buf, int rin) {
                const int ro = rin - LH;
                const bool is_out = t.is_output(ro);
                uint8_t *o8 = (is_out && out_u8) ? out_u8 + ((size_t)(t.y0 + ro) * W + t.px) * 3 : nullptr;
                float l1 = 0.f, sq = 0.f, bad = 0.f;
#pragma unroll 1
                for (int ch = 0; ch < CG; ch++) {
                    const float *sx = &s.in[buf][0][ch][t.rsub][t.col], *sy = &s.in[buf][1][ch][t.rsub][t.col];
                    float m[5];
                    moments_row(win, sx, sy, m);
                    ring_put(s.ring[ch], rin, t.col, m);
                    const float x = sx[LH], d = x - sy[LH];
                    l1 += fabsf(d);
                    sq += d * d;
                    bad += fabsf(x) <= 3.402823466e+38f ? 0.f : 1.f;          // NaN or +-inf
                    if (o8) o8[ch] = metrics_byte(x, trunc);
                }
                if (is_out) { sums[0] += l1; sums[1] += sq; sums[3] += bad; }
            },
            [&](int ro) {
                float ssim = 0.f;
#pragma unroll 1
                for (int ch = 0; ch < CG; ch++) {
                    float m[5];
                    taps_col(win, s.ring[ch], ro, t.col, m);
                    ssim += ssim_of(m).S;
                }
                sums[2] += ssim;
            });
    }
    put_partials(sums, partials);
}

__global__ __launch_bounds__(256) void frame_metrics_finish_kernel(int nblocks, const float *__restrict__ partials, double inv_count,
    double *__restrict__ row)
{
    double sum[4];
    sum_partials(nblocks, partials, sum);
    if (threadIdx.x == 0) {
        const double mse = sum[1] * inv_count;
        row[0] = sum[0] * inv_count;
        row[1] = mse;
        row[2] = 20.0 * log10(1.0 / sqrt(mse));                               // utils/image_utils.py:17-19; +inf at mse 0
        row[3] = sum[2] * inv_count;
        row[4] = sum[3];
        row[5] = row[6] = row[7] = 0.0;
    }
}

// ---- scikit-image's SSIM of a rendered view (ex4d_frame_skssim*): render.py:78-79 of the reference,
//     sk_ssim(render, gt, data_range=R, multichannel=True, channel_axis=0),   R = 1 (SKSSIM) and R = 2 (SKSSIM2)
// on float32 [3,H,W] arrays, read as current scikit-image (0.22 and later) reads it: `multichannel` falls into **kwargs and is ignored,
// channel_axis=0 holds.  (Earlier releases either override channel_axis with -1 or ignore it; on a [3,H,W] array both fail with
// "win_size exceeds image extent", so there is no other working reading.)  Per channel: the 7x7 uniform means ux, uy, uxx, uyy, uxy of
// X, Y, XX, YY, XY; the sample covariances v = (49/48)(uxx - ux^2) ...; C1 = (0.01 R)^2, C2 = (0.03 R)^2;
// S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)); the mean of S over the positions whose window lies wholly inside
// the image (scikit-image crops 3 pixels per side: the border mode never matters); the mean of the three channel means.
// The rolling window of frame_metrics_kernel (strips, segments, ring, double-buffered fetch / commit, work-item map, byte lookup, clamp
// at commit) with three differences.  Strips and segments tile the OUTPUT domain (H-6) x (W-6): output (oy, ox) reads image rows
// oy .. oy+6 and columns ox .. ox+6, all inside the image -- no zero padding (the zeros a fetch beyond the image leaves feed masked
// outputs only).  The 7 equal taps are added directly in a fixed order, in both passes: a sum depends on the image position alone,
// never on where a strip or segment starts.  The second moments are CENTRED, not raw: the row pass keeps, per 7-pixel row of a
// window, the two row means mx, my and the sums A, B, C of (x-mx)^2, (y-my)^2, (x-mx)(y-my); the column pass combines the seven rows as
// the pairwise variance update does: ux = mean(mx), sum (x-ux)^2 = sum A + 7 sum (mx-ux)^2, likewise for y and xy, and v = that / 48.
// The same five window quantities as ux, uy, uxx, uyy, uxy, without the cancellation of uxx - ux^2: raw float32 sums of 49 products
// miss the 1e-6 bar on a low-variance pair (2e-6 where the ground truth is piecewise constant and the render adds noise of sigma
// 0.002: the accumulated rounding of sums near 40 against C2 = 9e-4), the centred ones are within 1e-9 there.  Every product is an
// explicit fmaf / __fmul_rn, so the x, y and xy terms of equal images are equal bits; both S come from the same five quantities;
// numerator and denominator are formed by the same float operations in the same order and divided with a correctly rounded division,
// so equal images score exactly 1.  Three float partial sums per workgroup: sum S(R=1), sum S(R=2), the count of positions whose
// S(R=1) is not finite (at most 48 x 64 x 3: exact).
#define SKH 3                       // window half width: 70 input columns of a strip
static_assert(EX4D_SKSSIM_WINDOW == 2 * SKH + 1, "frame_skssim_kernel: the window is the halo's");

// seven taps of a window, m = their mean, (A, B, C) = the sums of dx^2, dy^2, dx dy about the means (fixed order, explicit rounding)
__device__ __forceinline__ void sk_centred(const float (&a)[EX4D_SKSSIM_WINDOW], const float (&b)[EX4D_SKSSIM_WINDOW], float &ma, float &mb,
                                           float &A, float &B, float &C)
{
    float sa = a[0], sb = b[0];
#pragma unroll
    for (int k = 1; k < EX4D_SKSSIM_WINDOW; k++) { sa = __fadd_rn(sa, a[k]); sb = __fadd_rn(sb, b[k]); }
    ma = __fmul_rn(sa, 1.0f / 7.0f); mb = __fmul_rn(sb, 1.0f / 7.0f);
    A = B = C = 0.f;
#pragma unroll
    for (int k = 0; k < EX4D_SKSSIM_WINDOW; k++) {
        const float da = __fsub_rn(a[k], ma), db = __fsub_rn(b[k], mb);
        A = fmaf(da, da, A); B = fmaf(db, db, B); C = fmaf(da, db, C);
    }
}

// S for one data range from the five means' derived terms: 2 ux uy, ux^2 + uy^2, 2 vxy, vx + vy
__device__ __forceinline__ float sk_s(float m2xy, float mxxyy, float v2xy, float vxxyy, float C1, float C2)
{
    return __fdiv_rn(__fmul_rn(__fadd_rn(m2xy, C1), __fadd_rn(v2xy, C2)), __fmul_rn(__fadd_rn(mxxyy, C1), __fadd_rn(vxxyy, C2)));
}

template <typename T, typename... Table>
__global__ __launch_bounds__(256) void frame_skssim_kernel(int H, int W, const float *__restrict__ img, const T *__restrict__ gt,
    int flags, float *__restrict__ partials, int nsx, int nsy, Table... table)
{
    using St = Stage<2, 5, SKH>;                         // maps x | y; row results mx, my, A, B, C
    static_assert(two_workgroups_per_cu<St, 3, Table...>, "frame_skssim_kernel: two workgroups per CU need <= 80 KB of LDS each");
    __shared__ St s;
    const PixelLds px8 = table_to_lds(table...);
    const int nwork = nsx * nsy;
    const int wi = work_item_of_block(nwork);
    const bool clamp01 = (flags & EX4D_METRICS_CLAMP) != 0;
    const float inv_nm1 = 1.0f / 48.0f;                  // sample covariance (scikit-image's default): / (49 - 1)
    float sums[3] = { 0.f, 0.f, 0.f };                   // S(R=1), S(R=2), non-finite count
    if (wi < nwork) {
        const Tile<SKH, false> t(wi, nsx, H - 2 * SKH, W - 2 * SKH);
        walk(t, H, W, s, ImagePair<T>{ img, gt, (size_t)H * W, px8, 0, CG, clamp01 },
            // ---- row pass: means and centred sums of columns px .. px + 6 -> ring
            [&](int buf, int rin) {
#pragma unroll 1
                for (int ch = 0; ch < CG; ch++) {
                    const float *sx = &s.in[buf][0][ch][t.rsub][t.col], *sy = &s.in[buf][1][ch][t.rsub][t.col];
                    float a[EX4D_SKSSIM_WINDOW], b[EX4D_SKSSIM_WINDOW], m[5];
#pragma unroll
                    for (int k = 0; k < EX4D_SKSSIM_WINDOW; k++) { a[k] = sx[k]; b[k] = sy[k]; }
                    sk_centred(a, b, m[0], m[1], m[2], m[3], m[4]);
                    ring_put(s.ring[ch], rin, t.col, m);
                }
            },
            [&](int ro) {
#pragma unroll 1
                for (int ch = 0; ch < CG; ch++) {
                    float a[EX4D_SKSSIM_WINDOW], b[EX4D_SKSSIM_WINDOW], ux, uy, dxx, dyy, dxy;
                    float sxx = 0.f, syy = 0.f, sxy = 0.f;             // (the first add is exact)
#pragma unroll
                    for (int k = 0; k < EX4D_SKSSIM_WINDOW; k++) {
                        const int slot = (ro + k) & (RING - 1);
                        a[k] = s.ring[ch][0][slot][t.col]; b[k] = s.ring[ch][1][slot][t.col];
                        sxx = __fadd_rn(sxx, s.ring[ch][2][slot][t.col]); syy = __fadd_rn(syy, s.ring[ch][3][slot][t.col]);
                        sxy = __fadd_rn(sxy, s.ring[ch][4][slot][t.col]);
                    }
                    sk_centred(a, b, ux, uy, dxx, dyy, dxy);          // the seven row means about the window's mean
                    // the four sums of two products, each as ONE product rounded and the other fused into the sum: what contraction
                    // (on for this file; the rounded-operation intrinsics are plain operators to it) makes of them, stated so that
                    // the bits do not depend on which products a compiler picks.  Symmetric in x and y where the images are equal
                    const float txx = fmaf(7.0f, dxx, sxx), tyy = fmaf(7.0f, dyy, syy), txy = fmaf(7.0f, dxy, sxy);
                    const float m2xy = fmaf(ux, uy, __fmul_rn(ux, uy)), mxxyy = fmaf(uy, uy, __fmul_rn(ux, ux));
                    const float v2xy = fmaf(txy, inv_nm1, __fmul_rn(txy, inv_nm1)), vxxyy = fmaf(tyy, inv_nm1, __fmul_rn(txx, inv_nm1));
                    const float S1 = sk_s(m2xy, mxxyy, v2xy, vxxyy, 1e-4f, 9e-4f);           // data_range 1: (0.01)^2, (0.03)^2
                    const float S2 = sk_s(m2xy, mxxyy, v2xy, vxxyy, 4e-4f, 3.6e-3f);         // data_range 2: (0.02)^2, (0.06)^2
                    sums[0] += S1; sums[1] += S2;
                    sums[2] += fabsf(S1) <= 3.402823466e+38f ? 0.f : 1.f;                    // NaN or +-inf
                }
            });
    }
    put_partials(sums, partials);
}

// count: 3 (H-6)(W-6), the same for every channel, so the mean of the channel means is the overall mean; divided, not multiplied by a
// reciprocal: a sum of exact ones gives exactly 1
__global__ __launch_bounds__(256) void frame_skssim_finish_kernel(int nblocks, const float *__restrict__ partials, double count,
    double *__restrict__ row)
{
    double sum[3];
    sum_partials(nblocks, partials, sum);
    if (threadIdx.x == 0) {
        row[0] = sum[0] / count;
        row[1] = sum[1] / count;
        row[2] = sum[2];
        row[3] = 0.0;
    }
}

thread_local char g_loss_err[256] = "";

bool check_args(int C, int H, int W, const void *a, const void *b, const float *window)
{
    if (C <= 0 || H <= 0 || W <= 0 || !a || !b || !window) { snprintf(g_loss_err, sizeof(g_loss_err), "bad argument"); return false; }
    return true;
}

static inline int strips_of(int W) { return (W + SW - 1) / SW; }
static inline int segments_of(int H) { return (H + SEG - 1) / SEG; }
static inline int blocks_of(int H, int W) { return 8 * ((strips_of(W) * segments_of(H) + 7) / 8); }       // (padded: the XCD-aware work-item map)

Window window_of(const float *window)
{
    Window win;
    for (int i = 0; i < EX4D_SSIM_WINDOW; i++) win.w[i] = window[i];
    return win;
}

// what an entry point returns after its launches
int launched()
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_loss_err, sizeof(g_loss_err), "launch failed: %s", hipGetErrorString(e)); return EX4D_ERR_HIP; }
    return EX4D_OK;
}

// uint8 pixels: the host table (NULL: u / 255, the division PILtoTorch does, utils/general_utils.py:25) as the kernels take it, the
// trailing argument of a _u8 entry point's call below
PixelTable pixels_of(int32_t pixel_stride, const float *lut)
{
    PixelTable out;
    out.S = pixel_stride;
    for (int u = 0; u < 256; u++) out.v[u] = lut ? lut[u] : (float)u / 255.0f;
    return out;
}

bool check_pixels(const PixelTable &px)
{
    if (px.S == 3 || px.S == 4) return true;
    snprintf(g_loss_err, sizeof(g_loss_err), "pixel_stride %d: uint8 ground truth has 3 or 4 bytes per pixel", px.S);
    return false;
}

// ---- the entry points, for either kind of ground truth: float planes, or uint8 pixels with their table as the trailing argument
template <typename T, typename... Table>
int forward(int C, int H, int W, const float *img, const T *gt, float lambda_dssim, const float *window, float *loss, float *l1_errors,
            float *ssim_errors, float *dmaps, float *scratch, void *stream, const Table &... table)
{
    g_loss_err[0] = 0;
    if (!check_args(C, H, W, img, gt, window) || !loss || !dmaps || !scratch) { snprintf(g_loss_err, sizeof(g_loss_err), "bad argument"); return EX4D_ERR_ARG; }
    if (!(check_pixels(table) && ...)) return EX4D_ERR_ARG;
    const int nblocks = blocks_of(H, W);
    hipLaunchKernelGGL((l1_ssim_fwd_kernel<T, Table...>), dim3(nblocks), dim3(256), 0, (hipStream_t)stream, C, H, W, img, gt, window_of(window), l1_errors,
                       ssim_errors, dmaps, scratch, strips_of(W), segments_of(H), table...);
    hipLaunchKernelGGL(l1_ssim_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, nblocks, scratch,
                       1.0 / ((double)C * H * W), lambda_dssim, loss);
    return launched();
}

template <typename T, typename... Table>
int backward(int C, int H, int W, const float *img, const T *gt, float lambda_dssim, const float *window, const float *dmaps,
             const float *grad_loss, float *grad_img, void *stream, const Table &... table)
{
    g_loss_err[0] = 0;
    if (!check_args(C, H, W, img, gt, window) || !dmaps || !grad_loss || !grad_img) { snprintf(g_loss_err, sizeof(g_loss_err), "bad argument"); return EX4D_ERR_ARG; }
    if (!(check_pixels(table) && ...)) return EX4D_ERR_ARG;
    hipLaunchKernelGGL((l1_ssim_bwd_kernel<T, Table...>), dim3(blocks_of(H, W)), dim3(256), 0, (hipStream_t)stream, C, H, W, img, gt, window_of(window), dmaps,
                       grad_loss, lambda_dssim, (float)(1.0 / ((double)C * H * W)), grad_img, strips_of(W), segments_of(H), table...);
    return launched();
}

template <typename T, typename... Table>
int metrics(int H, int W, const float *img, const T *gt, const float *window, int flags, uint8_t *out_u8, double *row, float *scratch,
            void *stream, const Table &... table)
{
    g_loss_err[0] = 0;
    if (!check_args(3, H, W, img, gt, window) || !row || !scratch) { snprintf(g_loss_err, sizeof(g_loss_err), "bad argument"); return EX4D_ERR_ARG; }
    if (flags & ~(EX4D_METRICS_CLAMP | EX4D_METRICS_QUANT_TRUNC)) {
        snprintf(g_loss_err, sizeof(g_loss_err), "flags %d: EX4D_METRICS_CLAMP | EX4D_METRICS_QUANT_TRUNC only", flags);
        return EX4D_ERR_ARG;
    }
    if (!(check_pixels(table) && ...)) return EX4D_ERR_ARG;
    const int nblocks = blocks_of(H, W);
    hipLaunchKernelGGL((frame_metrics_kernel<T, Table...>), dim3(nblocks), dim3(256), 0, (hipStream_t)stream, H, W, img, gt, window_of(window), flags, out_u8,
                       scratch, strips_of(W), segments_of(H), table...);
    hipLaunchKernelGGL(frame_metrics_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, nblocks, scratch, 1.0 / (3.0 * H * W), row);
    return launched();
}

// scikit-image's SSIM: strips and segments of the output domain (H-6) x (W-6)
static inline int sk_blocks_of(int H, int W) { return blocks_of(H - 2 * SKH, W - 2 * SKH); }

template <typename T, typename... Table>
int skssim(int H, int W, const float *img, const T *gt, int flags, double *row, float *scratch, void *stream, const Table &... table)
{
    g_loss_err[0] = 0;
    if (!img || !gt || !row || !scratch) { snprintf(g_loss_err, sizeof(g_loss_err), "bad argument"); return EX4D_ERR_ARG; }
    if (H < EX4D_SKSSIM_WINDOW || W < EX4D_SKSSIM_WINDOW) {
        snprintf(g_loss_err, sizeof(g_loss_err), "image %d x %d: win_size exceeds image extent (H, W >= %d)", H, W, EX4D_SKSSIM_WINDOW);
        return EX4D_ERR_ARG;
    }
    if (flags & ~EX4D_METRICS_CLAMP) { snprintf(g_loss_err, sizeof(g_loss_err), "flags %d: EX4D_METRICS_CLAMP only", flags); return EX4D_ERR_ARG; }
    if (!(check_pixels(table) && ...)) return EX4D_ERR_ARG;
    const int Ho = H - 2 * SKH, Wo = W - 2 * SKH, nblocks = sk_blocks_of(H, W);
    hipLaunchKernelGGL((frame_skssim_kernel<T, Table...>), dim3(nblocks), dim3(256), 0, (hipStream_t)stream, H, W, img, gt, flags, scratch,
                       strips_of(Wo), segments_of(Ho), table...);
    hipLaunchKernelGGL(frame_skssim_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, nblocks, scratch, 3.0 * Ho * Wo, row);
    return launched();
}

}  // namespace

// the text ex4d_loss_last_error returns, for ex4d_frames.hip (the same header, the same error channel)
char *ex4d_loss_error_buffer(size_t *capacity)
{
    *capacity = sizeof(g_loss_err);
    return g_loss_err;
}

extern "C" {

const char *ex4d_loss_last_error(void) { return g_loss_err; }

size_t ex4d_l1_ssim_scratch_floats(int32_t H, int32_t W) { return 2 * (size_t)blocks_of(H, W) + 64; }

int ex4d_l1_ssim_forward(int32_t C, int32_t H, int32_t W, const float *img, const float *gt, float lambda_dssim,
                         const float *window, float *loss, float *l1_errors, float *ssim_errors, float *dmaps, float *scratch,
                         void *stream_)
{
    return forward(C, H, W, img, gt, lambda_dssim, window, loss, l1_errors, ssim_errors, dmaps, scratch, stream_);
}

int ex4d_l1_ssim_forward_u8(int32_t H, int32_t W, const float *img, const uint8_t *gt, int32_t pixel_stride, const float *lut,
                            float lambda_dssim, const float *window, float *loss, float *l1_errors, float *ssim_errors, float *dmaps,
                            float *scratch, void *stream_)
{
    return forward(3, H, W, img, gt, lambda_dssim, window, loss, l1_errors, ssim_errors, dmaps, scratch, stream_, pixels_of(pixel_stride, lut));
}

int ex4d_l1_ssim_backward(int32_t C, int32_t H, int32_t W, const float *img, const float *gt, float lambda_dssim,
                          const float *window, const float *dmaps, const float *grad_loss, float *grad_img, void *stream_)
{
    return backward(C, H, W, img, gt, lambda_dssim, window, dmaps, grad_loss, grad_img, stream_);
}

int ex4d_l1_ssim_backward_u8(int32_t H, int32_t W, const float *img, const uint8_t *gt, int32_t pixel_stride, const float *lut,
                             float lambda_dssim, const float *window, const float *dmaps, const float *grad_loss, float *grad_img, void *stream_)
{
    return backward(3, H, W, img, gt, lambda_dssim, window, dmaps, grad_loss, grad_img, stream_, pixels_of(pixel_stride, lut));
}

size_t ex4d_frame_metrics_scratch_floats(int32_t H, int32_t W) { return 4 * (size_t)blocks_of(H, W) + 64; }

int ex4d_frame_metrics(int32_t H, int32_t W, const float *img, const float *gt, const float *window, int32_t flags, uint8_t *out_u8,
                       double *row, float *scratch, void *stream_)
{
    return metrics(H, W, img, gt, window, flags, out_u8, row, scratch, stream_);
}

int ex4d_frame_metrics_u8(int32_t H, int32_t W, const float *img, const uint8_t *gt, int32_t pixel_stride, const float *lut,
                          const float *window, int32_t flags, uint8_t *out_u8, double *row, float *scratch, void *stream_)
{
    return metrics(H, W, img, gt, window, flags, out_u8, row, scratch, stream_, pixels_of(pixel_stride, lut));
}

size_t ex4d_frame_skssim_scratch_floats(int32_t H, int32_t W)
{
    return (H < EX4D_SKSSIM_WINDOW || W < EX4D_SKSSIM_WINDOW) ? 0 : 3 * (size_t)sk_blocks_of(H, W) + 64;
}

int ex4d_frame_skssim(int32_t H, int32_t W, const float *img, const float *gt, int32_t flags, double *row, float *scratch, void *stream_)
{
    return skssim(H, W, img, gt, flags, row, scratch, stream_);
}

int ex4d_frame_skssim_u8(int32_t H, int32_t W, const float *img, const uint8_t *gt, int32_t pixel_stride, const float *lut,
                         int32_t flags, double *row, float *scratch, void *stream_)
{
    return skssim(H, W, img, gt, flags, row, scratch, stream_, pixels_of(pixel_stride, lut));
}

}  // extern "C"
