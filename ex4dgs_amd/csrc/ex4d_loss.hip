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
// GROUND TRUTH AS DECODED (ex4d_l1_ssim_*_u8): both kernels are templates over the ground truth's element type -- float32 [C,H,W] planes,
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

// static LDS of the two kernels: the input double buffer + the ring of row-pass results.  Both exceed the 64 KB a workgroup may take on
// older parts and are sized for gfx950's 160 KB per CU (two workgroups per CU): this file builds for gfx950-class LDS only
static_assert(sizeof(float) * (2 * 2 * CG * RPI * (SIN + 2) + CG * 5 * RING * SW + 8) <= 80 * 1024, "l1_ssim_fwd_kernel: two workgroups per CU need <= 80 KB of LDS each");
static_assert(sizeof(float) * (2 * 3 * CG * RPI * (SIN + 2) + CG * 3 * RING * SW) <= 80 * 1024, "l1_ssim_bwd_kernel: two workgroups per CU need <= 80 KB of LDS each");

static_assert(sizeof(float) * (2 * 2 * CG * RPI * (SIN + 2) + CG * 5 * RING * SW + 8 + 256) <= 80 * 1024, "l1_ssim_fwd_kernel<uint8_t>: the table joins the same budget");
static_assert(sizeof(float) * (2 * 3 * CG * RPI * (SIN + 2) + CG * 3 * RING * SW + 256) <= 80 * 1024, "l1_ssim_bwd_kernel<uint8_t>: the table joins the same budget");

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

// (frame_metrics_kernel below repeats this kernel's fetch / commit / ring / barrier scheme: a fix to the window scheme belongs in both)
template <typename T, typename... Table>
__global__ __launch_bounds__(256) void l1_ssim_fwd_kernel(int C, int H, int W, const float *__restrict__ img,
    const T *__restrict__ gt, Window win, float *__restrict__ l1_errors, float *__restrict__ ssim_errors,
    float *__restrict__ dmaps, float *__restrict__ partials, int nsx, int nsy, Table... table)
{
    constexpr bool kBytes = sizeof...(Table) != 0;
    __shared__ float s_in[2][2][CG][RPI][SIN + 2];      // [buffer][x | y][channel][row][column]
    __shared__ float s_ring[CG][5][RING][SW];           // row-pass results of the last RING image rows
    __shared__ float s_red[2][4];
    const PixelLds px8 = table_to_lds(table...);        // (published by the barrier in front of the first fetch)
    const int nwork = nsx * nsy;
    const int wi = work_item_of_block(nwork);
    const int col = threadIdx.x & (SW - 1), rsub = threadIdx.x >> 6;
    const size_t HW = (size_t)H * W;
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    float l1_total = 0.f, ssim_total = 0.f;
    if (wi < nwork) {
        const int x0 = (wi % nsx) * SW, y0 = (wi / nsx) * SEG;
        const int rows_out = (H - y0) < SEG ? (H - y0) : SEG;
        const int n_in = rows_out + 2 * LH;              // image rows y0 - 5 .. y0 + rows_out + 4
        const int n_it = (n_in + RPI - 1) / RPI;
        const int px = x0 + col;
        // an iteration's rows: every thread takes column (tid & 63) of row (tid >> 6) in every plane (image x channel), threads 0 .. 39
        // also one of the 4 x 10 halo columns 64 .. 73 -- two loads per plane with ONE pixel offset each (a flat element index decoded
        // per load kept ~100 registers of hoisted address arithmetic alive)
        const int hrow = (int)threadIdx.x / (2 * LH), hcol = SW + (int)threadIdx.x % (2 * LH);
        const bool has_halo = threadIdx.x < RPI * 2 * LH;
        for (int c0 = 0; c0 < C; c0 += CG) {
            const int nc = (C - c0) < CG ? (C - c0) : CG;
            const bool first_group = c0 == 0, last_group = c0 + CG >= C;
            float rm[2 * CG], rh[2 * CG];
            auto fetch = [&](int it) {
                const int ym = y0 - LH + it * RPI + rsub, xm = x0 - LH + col;
                const int yh = y0 - LH + it * RPI + hrow, xh = x0 - LH + hcol;
                const bool okm = xm >= 0 && xm < W && ym >= 0 && ym < H, okh = has_halo && xh >= 0 && xh < W && yh >= 0 && yh < H;
                const size_t om = (size_t)ym * W + xm, oh = (size_t)yh * W + xh;
#pragma unroll
                for (int pl = 0; pl < 2 * CG; pl++) {
                    const int ch = pl % CG;
                    if constexpr (kBytes) {
                        if (pl / CG) {                   // the BYTE stays in flight; commit looks it up
                            rm[pl] = byte_bits(okm && ch < nc, gt, om * px8.S + (c0 + ch));
                            rh[pl] = byte_bits(okh && ch < nc, gt, oh * px8.S + (c0 + ch));
                        } else {
                            const float *src = img + (size_t)(c0 + ch) * HW;
                            rm[pl] = (okm && ch < nc) ? src[om] : 0.f;
                            rh[pl] = (okh && ch < nc) ? src[oh] : 0.f;
                        }
                    } else {
                        const float *src = ((pl / CG) ? gt : img) + (size_t)(c0 + ch) * HW;
                        rm[pl] = (okm && ch < nc) ? src[om] : 0.f;       // zero padding (conv2d padding=5)
                        rh[pl] = (okh && ch < nc) ? src[oh] : 0.f;
                    }
                }
            };
            auto commit = [&](int buf) {
#pragma unroll
                for (int pl = 0; pl < 2 * CG; pl++) {
                    float vm = rm[pl], vh = rh[pl];
                    if constexpr (kBytes) {
                        if (pl / CG) { vm = byte_value(vm, px8.v); vh = byte_value(vh, px8.v); }
                    }
                    s_in[buf][pl / CG][pl % CG][rsub][col] = vm;
                    if (has_halo) s_in[buf][pl / CG][pl % CG][hrow][hcol] = vh;
                }
            };
            __syncthreads();                             // (the previous channel group is done with both buffers and the ring)
            fetch(0);
            commit(0);
            __syncthreads();
            for (int it = 0; it < n_it; it++) {
                const int buf = it & 1;
                if (it + 1 < n_it) fetch(it + 1);        // in flight while this iteration's rows are convolved
                // ---- row pass of image row rin (relative to y0 - 5), five moment maps per channel -> ring; the L1 term of the pixels of
                // this row (they are output pixels when the row lies inside the segment)
                const int rin = it * RPI + rsub;
                if (rin < n_in) {
                    float l1 = 0.f;
#pragma unroll 1
                    for (int ch = 0; ch < nc; ch++) {
                        const float *sx = &s_in[buf][0][ch][rsub][col], *sy = &s_in[buf][1][ch][rsub][col];
                        float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
                        for (int k = 0; k < EX4D_SSIM_WINDOW; k++) {
                            const float a = sx[k], b = sy[k], wk = win.w[k];
                            m1 += wk * a; m2 += wk * b; e11 += wk * (a * a); e22 += wk * (b * b); e12 += wk * (a * b);
                        }
                        const int slot = rin & (RING - 1);
                        s_ring[ch][0][slot][col] = m1; s_ring[ch][1][slot][col] = m2; s_ring[ch][2][slot][col] = e11;
                        s_ring[ch][3][slot][col] = e22; s_ring[ch][4][slot][col] = e12;
                        l1 += fabsf(sx[LH] - sy[LH]);
                    }
                    const int ro = rin - LH;             // this image row as an output row of the segment
                    if (ro >= 0 && ro < rows_out && px < W) {
                        l1_total += l1;
                        if (l1_errors) {
                            float *o = l1_errors + (size_t)(y0 + ro) * W + px;
                            const float v = first_group ? l1 : *o + l1;
                            *o = last_group ? v / (float)C : v;
                        }
                    }
                }
                __syncthreads();
                // ---- column pass of output row ro: its window (image rows ro .. ro + 10 relative to y0 - 5) is complete
                const int ro = it * RPI + rsub - 2 * LH;
                if (ro >= 0 && ro < rows_out && px < W) {
                    float ssim = 0.f;
#pragma unroll 1
                    for (int ch = 0; ch < nc; ch++) {
                        float mu1 = 0.f, mu2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
                        for (int k = 0; k < EX4D_SSIM_WINDOW; k++) {
                            const float wk = win.w[k];
                            const int slot = (ro + k) & (RING - 1);
                            mu1 += wk * s_ring[ch][0][slot][col]; mu2 += wk * s_ring[ch][1][slot][col];
                            e11 += wk * s_ring[ch][2][slot][col]; e22 += wk * s_ring[ch][3][slot][col]; e12 += wk * s_ring[ch][4][slot][col];
                        }
                        // utils/loss_utils.py:61-74
                        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
                        const float s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu12;
                        const float a1 = 2.f * mu12 + C1, a2 = 2.f * s12 + C2, b1 = mu1_sq + mu2_sq + C1, b2 = s1 + s2 + C2;
                        const float inv = 1.f / (b1 * b2);
                        const float S = (a1 * a2) * inv;
                        ssim += S;
                        // partial derivatives of S w.r.t. (mu1, E[x^2], E[xy]) with the gt-side moments held fixed
                        const float dSda1 = a2 * inv, dSda2 = a1 * inv, dSdb1 = -S / b1, dSdb2 = -S / b2;
                        const float dA = 2.f * mu2 * (dSda1 - dSda2) + 2.f * mu1 * (dSdb1 - dSdb2);
                        const size_t o = (size_t)(c0 + ch) * HW + (size_t)(y0 + ro) * W + px;
                        dmaps[o] = dA;
                        dmaps[(size_t)C * HW + o] = dSdb2;
                        dmaps[2 * (size_t)C * HW + o] = 2.f * dSda2;
                    }
                    ssim_total += ssim;
                    if (ssim_errors) {
                        float *o = ssim_errors + (size_t)(y0 + ro) * W + px;
                        const float v = first_group ? ssim : *o + ssim;
                        *o = last_group ? v / (float)C : v;
                    }
                }
                if (it + 1 < n_it) commit(buf ^ 1);
                __syncthreads();
            }
        }
    }
    // per-workgroup partial sums (no single-address atomics: they serialise ~12 ns each)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { l1_total += __shfl_xor(l1_total, o, 64); ssim_total += __shfl_xor(ssim_total, o, 64); }
    if (lane == 0) { s_red[0][wave] = l1_total; s_red[1][wave] = ssim_total; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3];
        partials[2 * blockIdx.x + 1] = s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3];
    }
}

__global__ __launch_bounds__(256) void l1_ssim_finish_kernel(int nblocks, const float *__restrict__ partials, double inv_count,
    float lambda_dssim, float *__restrict__ loss)
{
    __shared__ double s[2][4];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) { a += (double)partials[2 * i]; b += (double)partials[2 * i + 1]; }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
    if (lane == 0) { s[0][wave] = a; s[1][wave] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float l1 = (float)((s[0][0] + s[0][1] + s[0][2] + s[0][3]) * inv_count);
        const float ss = (float)((s[1][0] + s[1][1] + s[1][2] + s[1][3]) * inv_count);
        loss[0] = (1.0f - lambda_dssim) * l1 + lambda_dssim * (1.0f - ss);      // train.py:145
    }
}

template <typename T, typename... Table>
__global__ __launch_bounds__(256) void l1_ssim_bwd_kernel(int C, int H, int W, const float *__restrict__ img,
    const T *__restrict__ gt, Window win, const float *__restrict__ dmaps, const float *__restrict__ grad_loss,
    float lambda_dssim, float inv_count, float *__restrict__ grad_img, int nsx, int nsy, Table... table)
{
    constexpr bool kBytes = sizeof...(Table) != 0;
    __shared__ float s_in[2][3][CG][RPI][SIN + 2];      // [buffer][map A | B | C][channel][row][column]
    __shared__ float s_ring[CG][3][RING][SW];
    const int nwork = nsx * nsy;
    const int wi = work_item_of_block(nwork);
    if (wi >= nwork) return;                             // (uniform: the whole workgroup)
    const PixelLds px8 = table_to_lds(table...);        // (read in the column pass, barriers later)
    const int col = threadIdx.x & (SW - 1), rsub = threadIdx.x >> 6;
    const size_t HW = (size_t)H * W;
    const float gl = grad_loss[0];
    const int x0 = (wi % nsx) * SW, y0 = (wi / nsx) * SEG;
    const int rows_out = (H - y0) < SEG ? (H - y0) : SEG;
    const int n_in = rows_out + 2 * LH;
    const int n_it = (n_in + RPI - 1) / RPI;
    const int px = x0 + col;
    const int hrow = (int)threadIdx.x / (2 * LH), hcol = SW + (int)threadIdx.x % (2 * LH);
    const bool has_halo = threadIdx.x < RPI * 2 * LH;
    for (int c0 = 0; c0 < C; c0 += CG) {
        const int nc = (C - c0) < CG ? (C - c0) : CG;
        float rm[3 * CG], rh[3 * CG];
        auto fetch = [&](int it) {
            const int ym = y0 - LH + it * RPI + rsub, xm = x0 - LH + col;
            const int yh = y0 - LH + it * RPI + hrow, xh = x0 - LH + hcol;
            const bool okm = xm >= 0 && xm < W && ym >= 0 && ym < H, okh = has_halo && xh >= 0 && xh < W && yh >= 0 && yh < H;
            const size_t om = (size_t)ym * W + xm, oh = (size_t)yh * W + xh;
#pragma unroll
            for (int pl = 0; pl < 3 * CG; pl++) {
                const int ch = pl % CG;
                const float *src = dmaps + ((size_t)(pl / CG) * C + c0 + ch) * HW;
                rm[pl] = (okm && ch < nc) ? src[om] : 0.f;
                rh[pl] = (okh && ch < nc) ? src[oh] : 0.f;
            }
        };
        auto commit = [&](int buf) {
#pragma unroll
            for (int pl = 0; pl < 3 * CG; pl++) {
                s_in[buf][pl / CG][pl % CG][rsub][col] = rm[pl];
                if (has_halo) s_in[buf][pl / CG][pl % CG][hrow][hcol] = rh[pl];
            }
        };
        __syncthreads();
        fetch(0);
        commit(0);
        __syncthreads();
        for (int it = 0; it < n_it; it++) {
            const int buf = it & 1;
            if (it + 1 < n_it) fetch(it + 1);
            const int rin = it * RPI + rsub;
            if (rin < n_in) {
#pragma unroll 1
                for (int ch = 0; ch < nc; ch++) {
                    const float *sa = &s_in[buf][0][ch][rsub][col], *sb = &s_in[buf][1][ch][rsub][col], *sc = &s_in[buf][2][ch][rsub][col];
                    float a = 0.f, b = 0.f, cc = 0.f;
#pragma unroll
                    for (int k = 0; k < EX4D_SSIM_WINDOW; k++) { const float wk = win.w[k]; a += wk * sa[k]; b += wk * sb[k]; cc += wk * sc[k]; }
                    const int slot = rin & (RING - 1);
                    s_ring[ch][0][slot][col] = a; s_ring[ch][1][slot][col] = b; s_ring[ch][2][slot][col] = cc;
                }
            }
            __syncthreads();
            const int ro = it * RPI + rsub - 2 * LH;
            if (ro >= 0 && ro < rows_out && px < W) {
#pragma unroll 1
                for (int ch = 0; ch < nc; ch++) {
                    float ca = 0.f, cb = 0.f, ccv = 0.f;
#pragma unroll
                    for (int k = 0; k < EX4D_SSIM_WINDOW; k++) {
                        const float wk = win.w[k];
                        const int slot = (ro + k) & (RING - 1);
                        ca += wk * s_ring[ch][0][slot][col]; cb += wk * s_ring[ch][1][slot][col]; ccv += wk * s_ring[ch][2][slot][col];
                    }
                    const size_t o = (size_t)(c0 + ch) * HW + (size_t)(y0 + ro) * W + px;
                    float yv;
                    if constexpr (kBytes) yv = px8.v[gt[((size_t)(y0 + ro) * W + px) * px8.S + (c0 + ch)]];
                    else yv = gt[o];
                    const float xv = img[o];
                    const float dssim = ca + 2.f * xv * cb + yv * ccv;                   // d(sum of ssim_map)/dx_p
                    const float diff = xv - yv;
                    const float sgn = (diff > 0.f) ? 1.f : ((diff < 0.f) ? -1.f : 0.f);  // d|x - y|/dx
                    grad_img[o] = gl * ((1.0f - lambda_dssim) * sgn * inv_count - lambda_dssim * dssim * inv_count);
                }
            }
            if (it + 1 < n_it) commit(buf ^ 1);
            __syncthreads();
        }
    }
}

// ---- SCORING a rendered view (ex4d_frame_metrics*): render.py:64-88 / train.py:313-362 of the reference.  The forward's rolling window
// (same strips, segments, ring and work-item map; C = 3, one channel group) without what only training reads: no dmaps, no error maps,
// so the column pass stores nothing.  The image value is clamped (EX4D_METRICS_CLAMP) when its row is committed to LDS, so every metric
// and the bytes see the clamped value; squared error, non-finite count and the pixel's three bytes come from the centre tap of the
// row pass, where the L1 term comes from.  Four float partial sums per workgroup (a workgroup has at most 48 x 64 x 3 = 9 216 values:
// its count is exact in a float); frame_metrics_finish_kernel adds them in double and writes the row.
static_assert(sizeof(float) * (2 * 2 * CG * RPI * (SIN + 2) + CG * 5 * RING * SW + 16 + 256) <= 80 * 1024, "frame_metrics_kernel: two workgroups per CU need <= 80 KB of LDS each, the table included");

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
    constexpr bool kBytes = sizeof...(Table) != 0;
    __shared__ float s_in[2][2][CG][RPI][SIN + 2];      // [buffer][x | y][channel][row][column]
    __shared__ float s_ring[CG][5][RING][SW];           // row-pass results of the last RING image rows
    __shared__ float s_red[4][4];
    const PixelLds px8 = table_to_lds(table...);        // (published by the barrier in front of the first fetch)
    const int nwork = nsx * nsy;
    const int wi = work_item_of_block(nwork);
    const int col = threadIdx.x & (SW - 1), rsub = threadIdx.x >> 6;
    const size_t HW = (size_t)H * W;
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    const bool clamp01 = (flags & EX4D_METRICS_CLAMP) != 0, trunc = (flags & EX4D_METRICS_QUANT_TRUNC) != 0;
    float l1_total = 0.f, sq_total = 0.f, ssim_total = 0.f, bad_total = 0.f;
    if (wi < nwork) {
        const int x0 = (wi % nsx) * SW, y0 = (wi / nsx) * SEG;
        const int rows_out = (H - y0) < SEG ? (H - y0) : SEG;
        const int n_in = rows_out + 2 * LH;              // image rows y0 - 5 .. y0 + rows_out + 4
        const int n_it = (n_in + RPI - 1) / RPI;
        const int px = x0 + col;
        const int hrow = (int)threadIdx.x / (2 * LH), hcol = SW + (int)threadIdx.x % (2 * LH);
        const bool has_halo = threadIdx.x < RPI * 2 * LH;
        float rm[2 * CG], rh[2 * CG];
        auto fetch = [&](int it) {
            const int ym = y0 - LH + it * RPI + rsub, xm = x0 - LH + col;
            const int yh = y0 - LH + it * RPI + hrow, xh = x0 - LH + hcol;
            const bool okm = xm >= 0 && xm < W && ym >= 0 && ym < H, okh = has_halo && xh >= 0 && xh < W && yh >= 0 && yh < H;
            const size_t om = (size_t)ym * W + xm, oh = (size_t)yh * W + xh;
#pragma unroll
            for (int pl = 0; pl < 2 * CG; pl++) {
                const int ch = pl % CG;
                if constexpr (kBytes) {
                    if (pl / CG) {                       // the BYTE stays in flight; commit looks it up
                        rm[pl] = byte_bits(okm, gt, om * px8.S + ch);
                        rh[pl] = byte_bits(okh, gt, oh * px8.S + ch);
                        continue;
                    }
                }
                const float *src = ((pl / CG) ? (const float *)gt : img) + (size_t)ch * HW;
                rm[pl] = okm ? src[om] : 0.f;            // zero padding (conv2d padding=5)
                rh[pl] = okh ? src[oh] : 0.f;
            }
        };
        auto commit = [&](int buf) {
#pragma unroll
            for (int pl = 0; pl < 2 * CG; pl++) {
                float vm = rm[pl], vh = rh[pl];
                if (pl / CG) {
                    if constexpr (kBytes) { vm = byte_value(vm, px8.v); vh = byte_value(vh, px8.v); }
                } else if (clamp01) {                    // torch.clamp: a NaN stays a NaN (the padding's 0 stays 0)
                    vm = vm < 0.f ? 0.f : (vm > 1.f ? 1.f : vm);
                    vh = vh < 0.f ? 0.f : (vh > 1.f ? 1.f : vh);
                }
                s_in[buf][pl / CG][pl % CG][rsub][col] = vm;
                if (has_halo) s_in[buf][pl / CG][pl % CG][hrow][hcol] = vh;
            }
        };
        __syncthreads();                                 // (the table)
        fetch(0);
        commit(0);
        __syncthreads();
        for (int it = 0; it < n_it; it++) {
            const int buf = it & 1;
            if (it + 1 < n_it) fetch(it + 1);            // in flight while this iteration's rows are convolved
            // ---- row pass of image row rin (relative to y0 - 5) -> ring; when the row lies inside the segment its pixels are output
            // pixels: their L1 and squared-error terms, their non-finite count and their bytes
            const int rin = it * RPI + rsub;
            if (rin < n_in) {
                const int ro = rin - LH;
                const bool is_out = ro >= 0 && ro < rows_out && px < W;
                uint8_t *o8 = (is_out && out_u8) ? out_u8 + ((size_t)(y0 + ro) * W + px) * 3 : nullptr;
                float l1 = 0.f, sq = 0.f, bad = 0.f;
#pragma unroll 1
                for (int ch = 0; ch < CG; ch++) {
                    const float *sx = &s_in[buf][0][ch][rsub][col], *sy = &s_in[buf][1][ch][rsub][col];
                    float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
                    for (int k = 0; k < EX4D_SSIM_WINDOW; k++) {
                        const float a = sx[k], b = sy[k], wk = win.w[k];
                        m1 += wk * a; m2 += wk * b; e11 += wk * (a * a); e22 += wk * (b * b); e12 += wk * (a * b);
                    }
                    const int slot = rin & (RING - 1);
                    s_ring[ch][0][slot][col] = m1; s_ring[ch][1][slot][col] = m2; s_ring[ch][2][slot][col] = e11;
                    s_ring[ch][3][slot][col] = e22; s_ring[ch][4][slot][col] = e12;
                    const float x = sx[LH], d = x - sy[LH];
                    l1 += fabsf(d);
                    sq += d * d;
                    bad += fabsf(x) <= 3.402823466e+38f ? 0.f : 1.f;          // NaN or +-inf
                    if (o8) o8[ch] = metrics_byte(x, trunc);
                }
                if (is_out) { l1_total += l1; sq_total += sq; bad_total += bad; }
            }
            __syncthreads();
            // ---- column pass of output row ro: its window (image rows ro .. ro + 10 relative to y0 - 5) is complete
            const int ro = it * RPI + rsub - 2 * LH;
            if (ro >= 0 && ro < rows_out && px < W) {
                float ssim = 0.f;
#pragma unroll 1
                for (int ch = 0; ch < CG; ch++) {
                    float mu1 = 0.f, mu2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
                    for (int k = 0; k < EX4D_SSIM_WINDOW; k++) {
                        const float wk = win.w[k];
                        const int slot = (ro + k) & (RING - 1);
                        mu1 += wk * s_ring[ch][0][slot][col]; mu2 += wk * s_ring[ch][1][slot][col];
                        e11 += wk * s_ring[ch][2][slot][col]; e22 += wk * s_ring[ch][3][slot][col]; e12 += wk * s_ring[ch][4][slot][col];
                    }
                    // utils/loss_utils.py:61-74, in the forward's order of operations
                    const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
                    const float s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu12;
                    const float a1 = 2.f * mu12 + C1, a2 = 2.f * s12 + C2, b1 = mu1_sq + mu2_sq + C1, b2 = s1 + s2 + C2;
                    const float inv = 1.f / (b1 * b2);
                    ssim += (a1 * a2) * inv;
                }
                ssim_total += ssim;
            }
            if (it + 1 < n_it) commit(buf ^ 1);
            __syncthreads();
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        l1_total += __shfl_xor(l1_total, o, 64); sq_total += __shfl_xor(sq_total, o, 64);
        ssim_total += __shfl_xor(ssim_total, o, 64); bad_total += __shfl_xor(bad_total, o, 64);
    }
    if (lane == 0) { s_red[0][wave] = l1_total; s_red[1][wave] = sq_total; s_red[2][wave] = ssim_total; s_red[3][wave] = bad_total; }
    __syncthreads();
    if (threadIdx.x < 4)
        partials[4 * blockIdx.x + threadIdx.x] = s_red[threadIdx.x][0] + s_red[threadIdx.x][1] + s_red[threadIdx.x][2] + s_red[threadIdx.x][3];
}

__global__ __launch_bounds__(256) void frame_metrics_finish_kernel(int nblocks, const float *__restrict__ partials, double inv_count,
    double *__restrict__ row)
{
    __shared__ double s[4][4];
    double a[4] = { 0.0, 0.0, 0.0, 0.0 };
    for (int i = threadIdx.x; i < nblocks; i += 256) {
#pragma unroll
        for (int q = 0; q < 4; q++) a[q] += (double)partials[4 * i + q];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 4; q++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a[q] += __shfl_xor(a[q], o, 64);
        if (lane == 0) s[q][wave] = a[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double mse = (s[1][0] + s[1][1] + s[1][2] + s[1][3]) * inv_count;
        row[0] = (s[0][0] + s[0][1] + s[0][2] + s[0][3]) * inv_count;
        row[1] = mse;
        row[2] = 20.0 * log10(1.0 / sqrt(mse));                               // utils/image_utils.py:17-19; +inf at mse 0
        row[3] = (s[2][0] + s[2][1] + s[2][2] + s[2][3]) * inv_count;
        row[4] = s[3][0] + s[3][1] + s[3][2] + s[3][3];
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
#define SKH 3                       // window half width
#define SKIN (SW + 2 * SKH)         // 70 input columns of a strip
#define SKRING 16                   // ring rows (>= EX4D_SKSSIM_WINDOW + RPI - 1, power of two)
static_assert(EX4D_SKSSIM_WINDOW == 2 * SKH + 1 && SKRING >= EX4D_SKSSIM_WINDOW + RPI - 1 && (SKRING & (SKRING - 1)) == 0, "frame_skssim_kernel: the ring holds a window and an iteration");
static_assert(RPI * 2 * SKH <= 256, "frame_skssim_kernel: one halo load per thread");
static_assert(sizeof(float) * (2 * 2 * CG * RPI * (SKIN + 2) + CG * 5 * SKRING * SW + 12 + 256) <= 80 * 1024, "frame_skssim_kernel: two workgroups per CU need <= 80 KB of LDS each, the table included");

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
    constexpr bool kBytes = sizeof...(Table) != 0;
    __shared__ float s_in[2][2][CG][RPI][SKIN + 2];     // [buffer][x | y][channel][row][column]
    __shared__ float s_ring[CG][5][SKRING][SW];         // row-pass results (mx, my, A, B, C) of the last SKRING image rows
    __shared__ float s_red[3][4];
    const PixelLds px8 = table_to_lds(table...);        // (published by the barrier in front of the first fetch)
    const int nwork = nsx * nsy;
    const int wi = work_item_of_block(nwork);
    const int col = threadIdx.x & (SW - 1), rsub = threadIdx.x >> 6;
    const size_t HW = (size_t)H * W;
    const int Ho = H - 2 * SKH, Wo = W - 2 * SKH;       // the output domain
    const bool clamp01 = (flags & EX4D_METRICS_CLAMP) != 0;
    const float inv_nm1 = 1.0f / 48.0f;                  // sample covariance (scikit-image's default): / (49 - 1)
    float s1_total = 0.f, s2_total = 0.f, bad_total = 0.f;
    if (wi < nwork) {
        const int x0 = (wi % nsx) * SW, y0 = (wi / nsx) * SEG;           // first output column / row = first image column / row read
        const int rows_out = (Ho - y0) < SEG ? (Ho - y0) : SEG;
        const int n_in = rows_out + 2 * SKH;             // image rows y0 .. y0 + rows_out + 5
        const int n_it = (n_in + RPI - 1) / RPI;
        const int px = x0 + col;                         // this thread's output column
        const int hrow = (int)threadIdx.x / (2 * SKH), hcol = SW + (int)threadIdx.x % (2 * SKH);
        const bool has_halo = threadIdx.x < RPI * 2 * SKH;
        float rm[2 * CG], rh[2 * CG];
        auto fetch = [&](int it) {
            const int ym = y0 + it * RPI + rsub, xm = x0 + col;
            const int yh = y0 + it * RPI + hrow, xh = x0 + hcol;
            const bool okm = xm < W && ym < H, okh = has_halo && xh < W && yh < H;
            const size_t om = (size_t)ym * W + xm, oh = (size_t)yh * W + xh;
#pragma unroll
            for (int pl = 0; pl < 2 * CG; pl++) {
                const int ch = pl % CG;
                if constexpr (kBytes) {
                    if (pl / CG) {                       // the BYTE stays in flight; commit looks it up
                        rm[pl] = byte_bits(okm, gt, om * px8.S + ch);
                        rh[pl] = byte_bits(okh, gt, oh * px8.S + ch);
                        continue;
                    }
                }
                const float *src = ((pl / CG) ? (const float *)gt : img) + (size_t)ch * HW;
                rm[pl] = okm ? src[om] : 0.f;            // (beyond the image: read by masked outputs only)
                rh[pl] = okh ? src[oh] : 0.f;
            }
        };
        auto commit = [&](int buf) {
#pragma unroll
            for (int pl = 0; pl < 2 * CG; pl++) {
                float vm = rm[pl], vh = rh[pl];
                if (pl / CG) {
                    if constexpr (kBytes) { vm = byte_value(vm, px8.v); vh = byte_value(vh, px8.v); }
                } else if (clamp01) {                    // torch.clamp: a NaN stays a NaN
                    vm = vm < 0.f ? 0.f : (vm > 1.f ? 1.f : vm);
                    vh = vh < 0.f ? 0.f : (vh > 1.f ? 1.f : vh);
                }
                s_in[buf][pl / CG][pl % CG][rsub][col] = vm;
                if (has_halo) s_in[buf][pl / CG][pl % CG][hrow][hcol] = vh;
            }
        };
        __syncthreads();                                 // (the table)
        fetch(0);
        commit(0);
        __syncthreads();
        for (int it = 0; it < n_it; it++) {
            const int buf = it & 1;
            if (it + 1 < n_it) fetch(it + 1);            // in flight while this iteration's rows are summed
            // ---- row pass of image row rin (relative to y0): means and centred sums of columns px .. px + 6 -> ring
            const int rin = it * RPI + rsub;
            if (rin < n_in) {
                const int slot = rin & (SKRING - 1);
#pragma unroll 1
                for (int ch = 0; ch < CG; ch++) {
                    const float *sx = &s_in[buf][0][ch][rsub][col], *sy = &s_in[buf][1][ch][rsub][col];
                    float a[EX4D_SKSSIM_WINDOW], b[EX4D_SKSSIM_WINDOW], m1, m2, e11, e22, e12;
#pragma unroll
                    for (int k = 0; k < EX4D_SKSSIM_WINDOW; k++) { a[k] = sx[k]; b[k] = sy[k]; }
                    sk_centred(a, b, m1, m2, e11, e22, e12);
                    s_ring[ch][0][slot][col] = m1; s_ring[ch][1][slot][col] = m2; s_ring[ch][2][slot][col] = e11;
                    s_ring[ch][3][slot][col] = e22; s_ring[ch][4][slot][col] = e12;
                }
            }
            __syncthreads();
            // ---- column pass of output row ro: its window (image rows ro .. ro + 6 relative to y0) is complete
            const int ro = it * RPI + rsub - 2 * SKH;
            if (ro >= 0 && ro < rows_out && px < Wo) {
#pragma unroll 1
                for (int ch = 0; ch < CG; ch++) {
                    float a[EX4D_SKSSIM_WINDOW], b[EX4D_SKSSIM_WINDOW], ux, uy, dxx, dyy, dxy;
                    float sxx = 0.f, syy = 0.f, sxy = 0.f;             // (the first add is exact)
#pragma unroll
                    for (int k = 0; k < EX4D_SKSSIM_WINDOW; k++) {
                        const int slot = (ro + k) & (SKRING - 1);
                        a[k] = s_ring[ch][0][slot][col]; b[k] = s_ring[ch][1][slot][col];
                        sxx = __fadd_rn(sxx, s_ring[ch][2][slot][col]); syy = __fadd_rn(syy, s_ring[ch][3][slot][col]);
                        sxy = __fadd_rn(sxy, s_ring[ch][4][slot][col]);
                    }
                    sk_centred(a, b, ux, uy, dxx, dyy, dxy);          // the seven row means about the window's mean
                    const float vx = __fmul_rn(fmaf(7.0f, dxx, sxx), inv_nm1), vy = __fmul_rn(fmaf(7.0f, dyy, syy), inv_nm1);
                    const float vxy = __fmul_rn(fmaf(7.0f, dxy, sxy), inv_nm1);
                    const float mxx = __fmul_rn(ux, ux), myy = __fmul_rn(uy, uy), mxy = __fmul_rn(ux, uy);
                    const float m2xy = __fadd_rn(mxy, mxy), mxxyy = __fadd_rn(mxx, myy), v2xy = __fadd_rn(vxy, vxy), vxxyy = __fadd_rn(vx, vy);
                    const float S1 = sk_s(m2xy, mxxyy, v2xy, vxxyy, 1e-4f, 9e-4f);           // data_range 1: (0.01)^2, (0.03)^2
                    const float S2 = sk_s(m2xy, mxxyy, v2xy, vxxyy, 4e-4f, 3.6e-3f);         // data_range 2: (0.02)^2, (0.06)^2
                    s1_total += S1; s2_total += S2;
                    bad_total += fabsf(S1) <= 3.402823466e+38f ? 0.f : 1.f;                  // NaN or +-inf
                }
            }
            if (it + 1 < n_it) commit(buf ^ 1);
            __syncthreads();
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1_total += __shfl_xor(s1_total, o, 64); s2_total += __shfl_xor(s2_total, o, 64); bad_total += __shfl_xor(bad_total, o, 64);
    }
    if (lane == 0) { s_red[0][wave] = s1_total; s_red[1][wave] = s2_total; s_red[2][wave] = bad_total; }
    __syncthreads();
    if (threadIdx.x < 3)
        partials[3 * blockIdx.x + threadIdx.x] = s_red[threadIdx.x][0] + s_red[threadIdx.x][1] + s_red[threadIdx.x][2] + s_red[threadIdx.x][3];
}

// count: 3 (H-6)(W-6), the same for every channel, so the mean of the channel means is the overall mean; divided, not multiplied by a
// reciprocal: a sum of exact ones gives exactly 1
__global__ __launch_bounds__(256) void frame_skssim_finish_kernel(int nblocks, const float *__restrict__ partials, double count,
    double *__restrict__ row)
{
    __shared__ double s[3][4];
    double a[3] = { 0.0, 0.0, 0.0 };
    for (int i = threadIdx.x; i < nblocks; i += 256) {
#pragma unroll
        for (int q = 0; q < 3; q++) a[q] += (double)partials[3 * i + q];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 3; q++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a[q] += __shfl_xor(a[q], o, 64);
        if (lane == 0) s[q][wave] = a[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        row[0] = (s[0][0] + s[0][1] + s[0][2] + s[0][3]) / count;
        row[1] = (s[1][0] + s[1][1] + s[1][2] + s[1][3]) / count;
        row[2] = s[2][0] + s[2][1] + s[2][2] + s[2][3];
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

// the two launches of a forward / the one of a backward, for either kind of ground truth (the arguments were checked by the caller)
template <typename T, typename... Table>
int launch_forward(int C, int H, int W, const float *img, const T *gt, float lambda_dssim, const float *window, float *loss,
                          float *l1_errors, float *ssim_errors, float *dmaps, float *scratch, hipStream_t stream, const Table &... table)
{
    Window win;
    for (int i = 0; i < EX4D_SSIM_WINDOW; i++) win.w[i] = window[i];
    const int nblocks = blocks_of(H, W);
    hipLaunchKernelGGL((l1_ssim_fwd_kernel<T, Table...>), dim3(nblocks), dim3(256), 0, stream, C, H, W, img, gt, win, l1_errors, ssim_errors, dmaps, scratch,
                       strips_of(W), segments_of(H), table...);
    hipLaunchKernelGGL(l1_ssim_finish_kernel, dim3(1), dim3(256), 0, stream, nblocks, scratch,
                       1.0 / ((double)C * H * W), lambda_dssim, loss);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_loss_err, sizeof(g_loss_err), "launch failed: %s", hipGetErrorString(e)); return EX4D_ERR_HIP; }
    return EX4D_OK;
}

template <typename T, typename... Table>
int launch_backward(int C, int H, int W, const float *img, const T *gt, float lambda_dssim, const float *window, const float *dmaps,
                           const float *grad_loss, float *grad_img, hipStream_t stream, const Table &... table)
{
    Window win;
    for (int i = 0; i < EX4D_SSIM_WINDOW; i++) win.w[i] = window[i];
    hipLaunchKernelGGL((l1_ssim_bwd_kernel<T, Table...>), dim3(blocks_of(H, W)), dim3(256), 0, stream, C, H, W, img, gt, win, dmaps, grad_loss, lambda_dssim,
                       (float)(1.0 / ((double)C * H * W)), grad_img, strips_of(W), segments_of(H), table...);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_loss_err, sizeof(g_loss_err), "launch failed: %s", hipGetErrorString(e)); return EX4D_ERR_HIP; }
    return EX4D_OK;
}

// uint8 pixels + the host table (NULL: u / 255, the division PILtoTorch does, utils/general_utils.py:25) as the kernels take them
bool pixels_of(const uint8_t *gt, int32_t pixel_stride, const float *lut, PixelTable *out)
{
    if (!gt || (pixel_stride != 3 && pixel_stride != 4)) {
        snprintf(g_loss_err, sizeof(g_loss_err), !gt ? "bad argument" : "pixel_stride %d: uint8 ground truth has 3 or 4 bytes per pixel", (int)pixel_stride);
        return false;
    }
    out->S = pixel_stride;
    for (int u = 0; u < 256; u++) out->v[u] = lut ? lut[u] : (float)u / 255.0f;
    return true;
}

template <typename T, typename... Table>
int launch_metrics(int H, int W, const float *img, const T *gt, const float *window, int flags, uint8_t *out_u8, double *row,
                   float *scratch, hipStream_t stream, const Table &... table)
{
    Window win;
    for (int i = 0; i < EX4D_SSIM_WINDOW; i++) win.w[i] = window[i];
    const int nblocks = blocks_of(H, W);
    hipLaunchKernelGGL((frame_metrics_kernel<T, Table...>), dim3(nblocks), dim3(256), 0, stream, H, W, img, gt, win, flags, out_u8, scratch,
                       strips_of(W), segments_of(H), table...);
    hipLaunchKernelGGL(frame_metrics_finish_kernel, dim3(1), dim3(256), 0, stream, nblocks, scratch, 1.0 / (3.0 * H * W), row);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_loss_err, sizeof(g_loss_err), "launch failed: %s", hipGetErrorString(e)); return EX4D_ERR_HIP; }
    return EX4D_OK;
}

bool check_metrics_args(int H, int W, const void *img, const void *gt, const float *window, int flags, const double *row, const float *scratch)
{
    if (!check_args(3, H, W, img, gt, window) || !row || !scratch) { snprintf(g_loss_err, sizeof(g_loss_err), "bad argument"); return false; }
    if (flags & ~(EX4D_METRICS_CLAMP | EX4D_METRICS_QUANT_TRUNC)) { snprintf(g_loss_err, sizeof(g_loss_err), "flags %d: EX4D_METRICS_CLAMP | EX4D_METRICS_QUANT_TRUNC only", flags); return false; }
    return true;
}

// scikit-image's SSIM: strips and segments of the output domain (H-6) x (W-6)
static inline int sk_blocks_of(int H, int W) { return blocks_of(H - 2 * SKH, W - 2 * SKH); }

template <typename T, typename... Table>
int launch_skssim(int H, int W, const float *img, const T *gt, int flags, double *row, float *scratch, hipStream_t stream, const Table &... table)
{
    const int Ho = H - 2 * SKH, Wo = W - 2 * SKH, nblocks = sk_blocks_of(H, W);
    hipLaunchKernelGGL((frame_skssim_kernel<T, Table...>), dim3(nblocks), dim3(256), 0, stream, H, W, img, gt, flags, scratch,
                       strips_of(Wo), segments_of(Ho), table...);
    hipLaunchKernelGGL(frame_skssim_finish_kernel, dim3(1), dim3(256), 0, stream, nblocks, scratch, 3.0 * Ho * Wo, row);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_loss_err, sizeof(g_loss_err), "launch failed: %s", hipGetErrorString(e)); return EX4D_ERR_HIP; }
    return EX4D_OK;
}

bool check_skssim_args(int H, int W, const void *img, const void *gt, int flags, const double *row, const float *scratch)
{
    if (!img || !gt || !row || !scratch) { snprintf(g_loss_err, sizeof(g_loss_err), "bad argument"); return false; }
    if (H < EX4D_SKSSIM_WINDOW || W < EX4D_SKSSIM_WINDOW) {
        snprintf(g_loss_err, sizeof(g_loss_err), "image %d x %d: win_size exceeds image extent (H, W >= %d)", H, W, EX4D_SKSSIM_WINDOW);
        return false;
    }
    if (flags & ~EX4D_METRICS_CLAMP) { snprintf(g_loss_err, sizeof(g_loss_err), "flags %d: EX4D_METRICS_CLAMP only", flags); return false; }
    return true;
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
    g_loss_err[0] = 0;
    if (!check_args(C, H, W, img, gt, window) || !loss || !dmaps || !scratch) { snprintf(g_loss_err, sizeof(g_loss_err), "bad argument"); return EX4D_ERR_ARG; }
    return launch_forward(C, H, W, img, gt, lambda_dssim, window, loss, l1_errors, ssim_errors, dmaps, scratch, (hipStream_t)stream_);
}

int ex4d_l1_ssim_backward(int32_t C, int32_t H, int32_t W, const float *img, const float *gt, float lambda_dssim,
                          const float *window, const float *dmaps, const float *grad_loss, float *grad_img, void *stream_)
{
    g_loss_err[0] = 0;
    if (!check_args(C, H, W, img, gt, window) || !dmaps || !grad_loss || !grad_img) { snprintf(g_loss_err, sizeof(g_loss_err), "bad argument"); return EX4D_ERR_ARG; }
    return launch_backward(C, H, W, img, gt, lambda_dssim, window, dmaps, grad_loss, grad_img, (hipStream_t)stream_);
}

int ex4d_l1_ssim_forward_u8(int32_t H, int32_t W, const float *img, const uint8_t *gt, int32_t pixel_stride, const float *lut,
                            float lambda_dssim, const float *window, float *loss, float *l1_errors, float *ssim_errors, float *dmaps,
                            float *scratch, void *stream_)
{
    g_loss_err[0] = 0;
    PixelTable px;
    if (!check_args(3, H, W, img, gt, window) || !loss || !dmaps || !scratch) { snprintf(g_loss_err, sizeof(g_loss_err), "bad argument"); return EX4D_ERR_ARG; }
    if (!pixels_of(gt, pixel_stride, lut, &px)) return EX4D_ERR_ARG;
    return launch_forward(3, H, W, img, gt, lambda_dssim, window, loss, l1_errors, ssim_errors, dmaps, scratch, (hipStream_t)stream_, px);
}

int ex4d_l1_ssim_backward_u8(int32_t H, int32_t W, const float *img, const uint8_t *gt, int32_t pixel_stride, const float *lut,
                             float lambda_dssim, const float *window, const float *dmaps, const float *grad_loss, float *grad_img, void *stream_)
{
    g_loss_err[0] = 0;
    PixelTable px;
    if (!check_args(3, H, W, img, gt, window) || !dmaps || !grad_loss || !grad_img) { snprintf(g_loss_err, sizeof(g_loss_err), "bad argument"); return EX4D_ERR_ARG; }
    if (!pixels_of(gt, pixel_stride, lut, &px)) return EX4D_ERR_ARG;
    return launch_backward(3, H, W, img, gt, lambda_dssim, window, dmaps, grad_loss, grad_img, (hipStream_t)stream_, px);
}

size_t ex4d_frame_metrics_scratch_floats(int32_t H, int32_t W) { return 4 * (size_t)blocks_of(H, W) + 64; }

int ex4d_frame_metrics(int32_t H, int32_t W, const float *img, const float *gt, const float *window, int32_t flags, uint8_t *out_u8,
                       double *row, float *scratch, void *stream_)
{
    g_loss_err[0] = 0;
    if (!check_metrics_args(H, W, img, gt, window, flags, row, scratch)) return EX4D_ERR_ARG;
    return launch_metrics(H, W, img, gt, window, flags, out_u8, row, scratch, (hipStream_t)stream_);
}

int ex4d_frame_metrics_u8(int32_t H, int32_t W, const float *img, const uint8_t *gt, int32_t pixel_stride, const float *lut,
                          const float *window, int32_t flags, uint8_t *out_u8, double *row, float *scratch, void *stream_)
{
    g_loss_err[0] = 0;
    PixelTable px;
    if (!check_metrics_args(H, W, img, gt, window, flags, row, scratch)) return EX4D_ERR_ARG;
    if (!pixels_of(gt, pixel_stride, lut, &px)) return EX4D_ERR_ARG;
    return launch_metrics(H, W, img, gt, window, flags, out_u8, row, scratch, (hipStream_t)stream_, px);
}

size_t ex4d_frame_skssim_scratch_floats(int32_t H, int32_t W)
{
    return (H < EX4D_SKSSIM_WINDOW || W < EX4D_SKSSIM_WINDOW) ? 0 : 3 * (size_t)sk_blocks_of(H, W) + 64;
}

int ex4d_frame_skssim(int32_t H, int32_t W, const float *img, const float *gt, int32_t flags, double *row, float *scratch, void *stream_)
{
    g_loss_err[0] = 0;
    if (!check_skssim_args(H, W, img, gt, flags, row, scratch)) return EX4D_ERR_ARG;
    return launch_skssim(H, W, img, gt, flags, row, scratch, (hipStream_t)stream_);
}

int ex4d_frame_skssim_u8(int32_t H, int32_t W, const float *img, const uint8_t *gt, int32_t pixel_stride, const float *lut,
                         int32_t flags, double *row, float *scratch, void *stream_)
{
    g_loss_err[0] = 0;
    PixelTable px;
    if (!check_skssim_args(H, W, img, gt, flags, row, scratch)) return EX4D_ERR_ARG;
    if (!pixels_of(gt, pixel_stride, lut, &px)) return EX4D_ERR_ARG;
    return launch_skssim(H, W, img, gt, flags, row, scratch, (hipStream_t)stream_, px);
}

}  // extern "C"
