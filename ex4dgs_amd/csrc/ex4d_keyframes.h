// Keyframe interpolation of the positions, said once: the device arithmetic of x(t) and of its adjoint, and the host's knowledge of
// the interpolators (which exist, which keyframes each reads, how a launch picks its instantiation).  ex4d_attributes.hip (attribute
// forward / backward) and ex4d_motion.hip (displacement between two timestamps) call the device functions, so x(t) and its keyframe
// gradients carry the same bits in both; both are compiled with -ffp-contract=off: same float32 operation order as the reference's
// tensor arithmetic.  ex4d_trainer.hip uses the host part.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdio>
#include "../../include/ex4d_attributes.h"

// ---- host: the interpolators ------------------------------------------------------------------
static inline bool ex4d_known_interp(int32_t interp) { return interp == EX4D_INTERP_CUBE || interp == EX4D_INTERP_LINEAR || interp == EX4D_INTERP_PCHIP; }
#define EX4D_UNKNOWN_INTERP_FMT "unknown interpolator %d (0 cube, 1 linear, 2 pchip)"

// LAUNCH(I) with the compile-time interpolator I of a known `interp`
#define EX4D_DISPATCH_INTERP(interp, LAUNCH)                                  \
    do {                                                                      \
        if ((interp) == EX4D_INTERP_LINEAR) LAUNCH(EX4D_INTERP_LINEAR);       \
        else if ((interp) == EX4D_INTERP_PCHIP) LAUNCH(EX4D_INTERP_PCHIP);    \
        else LAUNCH(EX4D_INTERP_CUBE);                                        \
    } while (0)

// keyframes the position interpolator reads at keyframe index k: k .. k+1 (linear) or k-1 .. k+2 (cube, pchip); the slerp's k, k+1 lie
// inside both.  Host and device: the sliced gradients are windows of `count` rows of 3 floats per dynamic Gaussian.
struct Ex4dKeyWindow { int first, count; };
constexpr Ex4dKeyWindow ex4d_key_window(int interp, int k) { return interp == EX4D_INTERP_LINEAR ? Ex4dKeyWindow{ k, 2 } : Ex4dKeyWindow{ k - 1, 4 }; }

// the window of a's timestamp lies inside [0, K) (nothing to check without dynamic rows); t >= 0 names the timestamp in the refusal
static inline bool ex4d_check_key_window(const Ex4dAttrParams *a, int32_t interp, int t, char *err, size_t err_size)
{
    if (a->Nd <= 0) return true;
    const Ex4dKeyWindow w = ex4d_key_window(interp, 0);
    const int before = -w.first, after = w.first + w.count - 1;
    if (a->k >= before && (int64_t)a->k + after < (int64_t)a->K) return true;
    char of[16] = "";
    if (t >= 0) snprintf(of, sizeof(of), " of t%d", t);
    snprintf(err, err_size, "keyframe index %d%s needs k-%d..k+%d inside [0,%d)", a->k, of, before, after, a->K);
    return false;
}

// ---- device: x(t) and its adjoint -------------------------------------------------------------
// One component of the monotone Hermite slopes (utils/interpolations.py:72-73): a = y[k+1]-y[k], b = y[k]-y[k-1], s = y[k+1]-y[k-1], each
// its own subtraction; m = a*b > 0 ? (a*b)/s*2 : 0.  The quotient is formed (and, in the adjoint, differentiated) whether kept or not.
struct PchipSlope { float a, b, s, p; bool keep; };

__device__ __forceinline__ float pchip_slope(float ym, float y0, float yp, PchipSlope &m)
{
    m.a = yp - y0; m.b = y0 - ym; m.s = yp - ym;
    m.p = m.a * m.b;
    m.keep = m.p > 0.f;
    const float q = m.p / m.s * 2.0f;
    return m.keep ? q : 0.f;
}

// what autograd hands back through where / *2 / div / mul for a slope gradient g_m: the gradients of a, b and s
__device__ __forceinline__ void pchip_slope_adjoint(const PchipSlope &m, float g_m, float &g_a, float &g_b, float &g_s)
{
    const float g_q = (m.keep ? g_m : 0.f) * 2.0f;
    const float g_p = g_q / m.s;
    g_s = -g_q * ((m.p / m.s) / m.s);
    g_a = g_p * m.b;
    g_b = g_p * m.a;
}

// static row i at the timestamp of `a`: x(t) = xyz + (disp * t) / duration (c_gaussian_model.py:180)
__device__ __forceinline__ void static_position(const Ex4dAttrParams &a, int i, const float *__restrict__ xyz, const float *__restrict__ xyz_disp, float *m)
{
#pragma unroll
    for (int c = 0; c < 3; c++) m[c] = xyz[3 * (size_t)i + c] + (xyz_disp[3 * (size_t)i + c] * a.t) / a.duration;
}

// dynamic row j at the timestamp of `a`, from its window of xyz_motion [Nd,K,3]
template <int INTERP>
__device__ __forceinline__ void keyframe_position(const Ex4dAttrParams &a, size_t j, const float *__restrict__ xyz_motion, float *m)
{
    const float *y = xyz_motion + (j * a.K + ex4d_key_window(INTERP, a.k).first) * 3;
    if (INTERP == EX4D_INTERP_LINEAR) {
        // keyframes k, k+1 with the weights 1-delta, delta (interpolations.py:6-7, c_gaussian_model.py:107)
#pragma unroll
        for (int c = 0; c < 3; c++) m[c] = y[c] * a.h00 + y[3 + c] * a.h01;
    } else {
        // Hermite over keyframes k-1..k+2: Catmull-Rom slopes (interpolations.py:81-93, c_gaussian_model.py:118) or the monotone
        // ones of pchip (interpolations.py:65-77, c_gaussian_model.py:143)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float y0 = y[c], y1 = y[3 + c], y2 = y[6 + c], y3 = y[9 + c];
            float mk, mk1;
            if (INTERP == EX4D_INTERP_PCHIP) {
                PchipSlope s0, s1;
                mk = pchip_slope(y0, y1, y2, s0); mk1 = pchip_slope(y1, y2, y3, s1);
            } else {
                mk = (y2 - y0) / 2.0f; mk1 = (y3 - y1) / 2.0f;
            }
            m[c] = a.h00 * y1 + a.h10 * mk + a.h01 * y2 + a.h11 * mk1;
        }
    }
}

// the keyframe gradients of dynamic row j for the position gradient gm at the timestamp of `a`: gy is the row's window, [4,3]
// (linear: [2,3]), in global memory (attribute backward, dense or sliced) or in registers (motion backward).  Only pchip reads xyz_motion.
template <int INTERP>
__device__ __forceinline__ void keyframe_position_adjoint(const Ex4dAttrParams &a, size_t j, const float *__restrict__ xyz_motion, const float *gm, float *gy)
{
    if (INTERP == EX4D_INTERP_LINEAR) {
#pragma unroll
        for (int c = 0; c < 3; c++) { gy[c] = gm[c] * a.h00; gy[3 + c] = gm[c] * a.h01; }
    } else if (INTERP == EX4D_INTERP_PCHIP) {
        const float *y = xyz_motion + (j * a.K + ex4d_key_window(INTERP, a.k).first) * 3;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            PchipSlope s0, s1;
            (void)pchip_slope(y[c], y[3 + c], y[6 + c], s0);
            (void)pchip_slope(y[3 + c], y[6 + c], y[9 + c], s1);
            float ga0, gb0, gs0, ga1, gb1, gs1;
            pchip_slope_adjoint(s0, a.h10 * gm[c], ga0, gb0, gs0);
            pchip_slope_adjoint(s1, a.h11 * gm[c], ga1, gb1, gs1);
            // a = y[k+1]-y[k], b = y[k]-y[k-1], s = y[k+1]-y[k-1] of m_k; the same one keyframe on for m_{k+1}
            gy[c] = -gb0 - gs0;
            gy[3 + c] = a.h00 * gm[c] + (gb0 - ga0) + (-gb1 - gs1);
            gy[6 + c] = a.h01 * gm[c] + (ga0 + gs0) + (gb1 - ga1);
            gy[9 + c] = ga1 + gs1;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            gy[c] = -(a.h10 * gm[c]) / 2.0f;
            gy[3 + c] = a.h00 * gm[c] - (a.h11 * gm[c]) / 2.0f;
            gy[6 + c] = (a.h10 * gm[c]) / 2.0f + a.h01 * gm[c];
            gy[9 + c] = (a.h11 * gm[c]) / 2.0f;
        }
    }
}
