// Resizing decoded 8-bit frames for gfx950, bit for bit as PIL's Image.resize does (include/ex4d_loss.h, "RESIZING"): what the
// reference does on the host for every frame it loads (PILtoTorch, utils/general_utils.py:23-24; 2704 x 2028 -> 1352 x 1014 for the
// N3V scenes, scene/cameras.py:255).
//
// PIL's 8-bit resize is integer arithmetic behind a coefficient table built in double precision: the table is built here on the host
// (ex4d_resize_u8_table; this file is compiled with -ffp-contract=off so that no multiply-add of it fuses), uploaded once by the
// caller, and two kernels apply it:
//   resize_h_kernel   [rows, W_in, 3] -> [rows, W_out, 3]: one lane per output pixel, three int32 accumulators, the n taps of the pixel
//                     read from the row.  One general path for every ksize (100 -> 1 has 201 taps).
//   resize_v_kernel   [H_in, B] -> [H_out, B] over rows of B = 3 W_out flat bytes: a lane owns one 4-byte-aligned dword of the output
//                     row (four accumulators, the coefficient the same for the whole row), and the up to three bytes before the
//                     first and after the last whole dword of a row go one byte per lane.  Rows start at any byte address (odd B, a
//                     frame inside a store), so the alignment is worked out per row; the source dword of a lane sits at the same
//                     column of other rows and is fetched as four bytes at whatever alignment it has.
// Integer only, no atomics, no LDS.  At 2028 x 2704 -> 1014 x 1352 the two launches take 25 us, 0.18 of the HBM peak.
#include "ex4d_internal.h"
#include "../../include/ex4d_loss.h"
#include <cmath>
#include <cstring>
#include <vector>
#define EX4D_ERROR_BUFFER ex4d_loss_error_buffer        // ex4d_loss.hip: the text ex4d_loss_last_error returns
#include "ex4d_host_error.h"

namespace {

#define RZ_BITS 22                          // PIL's PRECISION_BITS: 32 - 8 - 2
#define RZ_THREADS 256
static_assert(EX4D_RESIZE_H_PIXELS * EX4D_RESIZE_H_ROWS == RZ_THREADS, "horizontal pass: one lane per pixel of the workgroup's tile");
static_assert(EX4D_RESIZE_V_BYTES / 4 * EX4D_RESIZE_V_ROWS == RZ_THREADS, "vertical pass: one lane per dword of the workgroup's tile");
static_assert(EX4D_RESIZE_H_PIXELS == 64 && EX4D_RESIZE_V_BYTES / 4 == 64, "a wave is one row of a tile: the row's table entry is uniform in it");

// ---- the table (host, double precision, PIL's precompute_coeffs and normalize_coeffs_8bpc)
double filter_value(int filter, double x)
{
    if (filter == EX4D_FILTER_BOX) return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
    if (x < 0.0) x = -x;
    if (filter == EX4D_FILTER_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
    const double a = -0.5;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

bool filter_support(int filter, double *s)
{
    switch (filter) {
    case EX4D_FILTER_BILINEAR: *s = 1.0; return true;
    case EX4D_FILTER_BICUBIC: *s = 2.0; return true;
    case EX4D_FILTER_BOX: *s = 0.5; return true;
    }
    return false;
}

inline bool size_ok(int v) { return v >= 1 && v <= EX4D_FRAME_MAX_SIZE; }

// support and ksize of one axis
void axis_of(int in, int out, double s, double *scale, double *fs, double *sup, int *ksize)
{
    *scale = (double)in / (double)out;
    *fs = *scale < 1.0 ? 1.0 : *scale;
    *sup = s * *fs;
    *ksize = (int)ceil(*sup) * 2 + 1;
}

// clamp(acc >> 22, 0, 255), written as the clamp of the accumulator followed by the shift.  Not a matter of taste: for the shift followed
// by the clamp the compiler selects gfx950's v_ashr_pk_u8_i32 (two results packed into the low 16 bits) and then uses the register as
// if its upper 16 bits were zero; on the MI355X they are not -- bytes 2 and 3 of every dword the vertical pass stored came out OR-ed
// with the upper half of an accumulator (found by the byte-equality tests).  The build refuses an object that holds the instruction
// (isa_check.packed_shift_clamps).
__device__ __forceinline__ int clip8(int acc)
{
    const int top = (256 << RZ_BITS) - 1;
    acc = acc < 0 ? 0 : (acc > top ? top : acc);
    return acc >> RZ_BITS;
}

// The table entry of output element i, made safe: whatever words the caller uploaded, the taps stay inside [0, in).
struct Taps { const int32_t *k; int first, n; };

__device__ __forceinline__ Taps taps_of(const int32_t *__restrict__ table, int i, int in)
{
    const int ksize = table[0];
    const int32_t *e = table + 1 + (size_t)i * (size_t)(ksize + 2);
    Taps t;
    t.first = min(max(e[0], 0), in);
    t.n = max(min(min(e[1], ksize), in - t.first), 0);
    t.k = e + 2;
    return t;
}

// ---- horizontal: src [rows, W_in, 3] -> dst [rows, W_out, 3]
__global__ void __launch_bounds__(RZ_THREADS)
resize_h_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const int32_t *__restrict__ table, int rows, int W_in, int W_out)
{
    const int x = blockIdx.x * EX4D_RESIZE_H_PIXELS + threadIdx.x;
    const int y = blockIdx.y * EX4D_RESIZE_H_ROWS + threadIdx.y;
    if (x >= W_out || y >= rows) return;
    const Taps t = taps_of(table, x, W_in);
    const uint8_t *p = src + ((size_t)y * W_in + t.first) * 3;
    int a0 = 1 << (RZ_BITS - 1), a1 = a0, a2 = a0;
    for (int i = 0; i < t.n; ++i) {
        const int k = t.k[i];
        a0 += (int)p[3 * i] * k;
        a1 += (int)p[3 * i + 1] * k;
        a2 += (int)p[3 * i + 2] * k;
    }
    uint8_t *q = dst + ((size_t)y * W_out + x) * 3;
    q[0] = (uint8_t)clip8(a0);
    q[1] = (uint8_t)clip8(a1);
    q[2] = (uint8_t)clip8(a2);
}

// ---- vertical: src [H_in, B] -> dst [H_out, B], B flat bytes per row
__global__ void __launch_bounds__(RZ_THREADS)
resize_v_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const int32_t *__restrict__ table, int H_in, int H_out, int B)
{
    const int y = blockIdx.y * EX4D_RESIZE_V_ROWS + threadIdx.y;
    if (y >= H_out) return;
    uint8_t *drow = dst + (size_t)y * B;
    const int head = min((int)((4 - ((uintptr_t)drow & 3)) & 3), B);      // bytes before the row's first aligned dword
    const int ndw = (B - head) >> 2;                                         // dwords wholly inside the row
    const int tail = B - head - 4 * ndw;
    const int item = blockIdx.x * (EX4D_RESIZE_V_BYTES / 4) + threadIdx.x;   // dwords first, then the head and tail bytes
    if (item >= ndw + head + tail) return;
    const Taps t = taps_of(table, y, H_in);
    const int half = 1 << (RZ_BITS - 1);
    if (item < ndw) {
        const int c = head + 4 * item;
        const uint8_t *p = src + (size_t)t.first * B + c;
        int a0 = half, a1 = half, a2 = half, a3 = half;
        for (int i = 0; i < t.n; ++i, p += B) {
            const int k = t.k[i];
            uint32_t v;
            __builtin_memcpy(&v, p, 4);                  // four bytes inside the row, at any alignment
            a0 += (int)(v & 255u) * k;
            a1 += (int)((v >> 8) & 255u) * k;
            a2 += (int)((v >> 16) & 255u) * k;
            a3 += (int)(v >> 24) * k;
        }
        *reinterpret_cast<uint32_t *>(drow + c) = (uint32_t)clip8(a0) | ((uint32_t)clip8(a1) << 8) | ((uint32_t)clip8(a2) << 16) | ((uint32_t)clip8(a3) << 24);
    } else {
        const int j = item - ndw;
        const int c = j < head ? j : head + 4 * ndw + (j - head);
        const uint8_t *p = src + (size_t)t.first * B + c;
        int a = half;
        for (int i = 0; i < t.n; ++i, p += B) a += (int)p[0] * t.k[i];
        drow[c] = (uint8_t)clip8(a);
    }
}

inline unsigned blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" {

size_t ex4d_resize_u8_table_words(int32_t in, int32_t out, int32_t filter)
{
    double s, scale, fs, sup;
    int ksize;
    if (!size_ok(in) || !size_ok(out) || !filter_support(filter, &s)) return 0;
    axis_of(in, out, s, &scale, &fs, &sup, &ksize);
    return 1 + (size_t)out * (size_t)(ksize + 2);
}

int ex4d_resize_u8_table(int32_t in, int32_t out, int32_t filter, int32_t *words)
{
    clear_error();
    double s, scale, fs, sup;
    int ksize;
    if (!size_ok(in) || !size_ok(out)) return fail(EX4D_ERR_ARG, "resize_u8_table: sizes are 1 .. 16384 per axis");
    if (!filter_support(filter, &s)) return fail(EX4D_ERR_ARG, "resize_u8_table: unknown filter (bilinear 2, bicubic 3, box 4; Lanczos and Hamming depend on libm and are not offered)");
    if (!words) return fail(EX4D_ERR_ARG, "resize_u8_table: null table");
    axis_of(in, out, s, &scale, &fs, &sup, &ksize);
    const double ss = 1.0 / fs;
    std::vector<double> w((size_t)ksize);
    words[0] = ksize;
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - sup + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + sup + 0.5);
        if (xmax > in) xmax = in;
        int n = xmax - xmin;
        if (n < 0) n = 0;
        if (n > ksize) n = ksize;                        // cannot happen: 2 sup + 1 <= ksize
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            w[x] = filter_value(filter, (x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        int32_t *e = words + 1 + (size_t)xx * (size_t)(ksize + 2);
        e[0] = xmin;
        e[1] = n;
        for (int x = 0; x < ksize; ++x) {
            if (x >= n) { e[2 + x] = 0; continue; }
            double v = w[x];
            if (ww != 0.0) v /= ww;
            e[2 + x] = v < 0 ? (int)(-0.5 + v * (double)(1 << RZ_BITS)) : (int)(0.5 + v * (double)(1 << RZ_BITS));
        }
    }
    return EX4D_OK;
}

size_t ex4d_resize_u8_scratch_bytes(int32_t H_in, int32_t W_in, int32_t H_out, int32_t W_out)
{
    if (!size_ok(H_in) || !size_ok(W_in) || !size_ok(H_out) || !size_ok(W_out)) return 0;
    return (H_in != H_out && W_in != W_out) ? (size_t)H_in * (size_t)W_out * 3 : 0;
}

int ex4d_resize_u8(int32_t H_in, int32_t W_in, int32_t H_out, int32_t W_out, int32_t pixel_stride, const uint8_t *src, uint8_t *dst,
                   const int32_t *table_x, const int32_t *table_y, uint8_t *scratch, void *stream_)
{
    clear_error();
    hipStream_t stream = (hipStream_t)stream_;
    if (pixel_stride == 4)
        return fail(EX4D_ERR_ARG, "resize_u8: four-byte pixels are refused: PIL resizes RGBA on premultiplied colour, which gives other colour bytes than its RGB resize; drop the fourth byte first");
    if (pixel_stride != 3) return fail(EX4D_ERR_ARG, "resize_u8: pixel_stride must be 3");
    if (!size_ok(H_in) || !size_ok(W_in) || !size_ok(H_out) || !size_ok(W_out)) return fail(EX4D_ERR_ARG, "resize_u8: sizes are 1 .. 16384 per axis");
    const bool horiz = W_in != W_out, vert = H_in != H_out;
    if (!src || !dst || (horiz && !table_x) || (vert && !table_y) || (horiz && vert && !scratch))
        return fail(EX4D_ERR_ARG, "resize_u8: null frame, table or scratch");
    const dim3 threads_h(EX4D_RESIZE_H_PIXELS, EX4D_RESIZE_H_ROWS), threads_v(EX4D_RESIZE_V_BYTES / 4, EX4D_RESIZE_V_ROWS);
    if (!horiz && !vert) {
        if (hipMemcpyAsync(dst, src, (size_t)H_in * W_in * 3, hipMemcpyDeviceToDevice, stream) != hipSuccess) return fail(EX4D_ERR_HIP, "resize_u8: copy failed");
        return EX4D_OK;
    }
    const uint8_t *vsrc = src;
    if (horiz) {
        uint8_t *hdst = vert ? scratch : dst;
        const dim3 grid(blocks(W_out, EX4D_RESIZE_H_PIXELS), blocks(H_in, EX4D_RESIZE_H_ROWS));
        hipLaunchKernelGGL(resize_h_kernel, grid, threads_h, 0, stream, src, hdst, table_x, H_in, W_in, W_out);
        const int rc = launch_status("resize_u8 (horizontal)");
        if (rc != EX4D_OK) return rc;
        vsrc = hdst;
    }
    if (vert) {
        const int B = 3 * W_out;
        // a row has at most B / 4 whole dwords and six head and tail bytes
        const dim3 grid(blocks(B / 4 + 6, EX4D_RESIZE_V_BYTES / 4), blocks(H_out, EX4D_RESIZE_V_ROWS));
        hipLaunchKernelGGL(resize_v_kernel, grid, threads_v, 0, stream, vsrc, dst, table_y, H_in, H_out, B);
        return launch_status("resize_u8 (vertical)");
    }
    return EX4D_OK;
}

}  // extern "C"
