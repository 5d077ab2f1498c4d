/*
 * ex4d_attributes.h -- C ABI of the fused per-frame attribute evaluation of the static + keyframe-interpolated
 * dynamic Gaussians, the producer of the five tensors the rasterizer boundary consumes.
 *
 * Replaces, as one forward and one backward call, the reference's Python getters and their autograd graph:
 *   CGaussianModel.get_xyz_at_t / get_rotation_at_t        scene/c_gaussian_model.py:170-215
 *   get_scaling / get_features / get_opacity_at_t          scene/c_gaussian_model.py:330-375
 *   cube_interpolate / quat_slerp_interp_uniiterval / time_bigaussian   utils/interpolations.py:81-93, :33-52, :55-61
 *   linear_interp_uniiterval / pchip_interpolate           utils/interpolations.py:6-7, :65-77
 * Rotations are interpolated by 'slerp'; positions by the interpolator the caller names (ModelParams.interp_type): 'cube' (the
 * configuration of configs/N3V and configs/techni; what the entry points without _ex compute), 'linear' or 'pchip'.
 *
 * All pointers are device pointers (float32, contiguous, shapes as in CGaussianModel); `stream` is a hipStream_t.
 * Outputs are [Ns+Nd, ...] with the static rows first (c_gaussian_model.py:193, :215, :374).
 */
#ifndef EX4D_ATTRIBUTES_H_INCLUDED
#define EX4D_ATTRIBUTES_H_INCLUDED

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The position interpolator of the dynamic Gaussians (c_gaussian_model.py:98-146).
 *   CUBE    Catmull-Rom Hermite over keyframes k-1 .. k+2; valid k: 1 .. K-3.
 *   LINEAR  y[k]*(1-delta) + y[k+1]*delta over keyframes k, k+1; valid k: 0 .. K-2.  Its model has time_shift = time_pad, not
 *           time_pad + interval.
 *   PCHIP   Hermite with the monotone slopes m = (a*b > 0) ? (a*b)/s*2 : 0, a = y[k+1]-y[k], b = y[k]-y[k-1], s = y[k+1]-y[k-1];
 *           keyframes k-1 .. k+2; valid k: 1 .. K-3.  Its backward is the adjoint autograd forms of exactly these operations: the
 *           quotient is differentiated even where the comparison drops it, so a component with s == 0 exactly (a constant track,
 *           y[k+1] == y[k-1]) gets NaN gradients on the keyframes the quotient touches, as in the reference.  Such rows go NaN in
 *           the optimizer and are removed by prune_nan_points, as there. */
enum { EX4D_INTERP_CUBE = 0, EX4D_INTERP_LINEAR = 1, EX4D_INTERP_PCHIP = 2 };

/* Host-evaluated scalars of one timestamp t (Python numbers in the reference, c_gaussian_model.py:184-186, :364):
 * t' = t + time_shift; k = t' // interval; delta = (t' % interval) / interval; Hermite basis at delta
 * (utils/interpolations.py:83-86, evaluated in double, used as float32); tau = t' / interval; var_min = var_pad / interval.
 * Linear: h00 = 1 - delta, h01 = delta (Python numbers times a float32 tensor, interpolations.py:7), h10 = h11 = 0. */
typedef struct Ex4dAttrParams {
    int32_t Ns, Nd;            /* static / dynamic Gaussian counts */
    int32_t K;                 /* keyframes per dynamic Gaussian (_xyz_motion.shape[1]) */
    int32_t k;                 /* keyframe index of this timestamp; slices k-1 .. k+2 are read (linear: k, k+1) */
    float t, duration;         /* static positions: _xyz + _xyz_disp * t / duration */
    float delta;               /* slerp parameter in [0,1) */
    float h00, h10, h01, h11;  /* Hermite basis at delta (linear: the two weights in h00, h01) */
    float tau;                 /* time in keyframe units for the bi-Gaussian opacity window */
    float var_min;             /* var_pad / interval */
} Ex4dAttrParams;

const char *ex4d_attributes_last_error(void);

/* Forward.  Parameters in CGaussianModel order; outputs means3D[N,3], rotations[N,4], opacities[N,1], scales[N,3], shs[N,16,3].
 * shs may be NULL (then the four feature tensors are not read): the rasterizer can take them as they are, see Ex4dSplitSH in
 * ex4d_rasterizer.h; likewise g_shs may be NULL in the backward (the four feature gradients are then not written). */
int ex4d_attributes_forward(const Ex4dAttrParams *a,
    const float *xyz /*[Ns,3]*/, const float *xyz_disp /*[Ns,3]*/, const float *rotation /*[Ns,4]*/, const float *opacity /*[Ns,1]*/,
    const float *scaling /*[Ns,3]*/, const float *features_dc /*[Ns,1,3]*/, const float *features_rest /*[Ns,15,3]*/,
    const float *xyz_motion /*[Nd,K,3]*/, const float *rotation_motion /*[Nd,K,4]*/, const float *opacity_motion /*[Nd,1]*/,
    const float *opacity_duration_center /*[Nd,2,1]*/, const float *opacity_duration_var /*[Nd,2,1]*/,
    const float *scaling_motion /*[Nd,3]*/, const float *features_dc_motion /*[Nd,1,3]*/, const float *features_rest_motion /*[Nd,15,3]*/,
    float *means3D, float *rotations, float *opacities, float *scales, float *shs, void *stream);

/* Backward: every gradient tensor is fully written (the dense keyframe gradients are zero-filled, then the 4 position / 2
 * rotation slices of this timestamp are set), so callers may pass uninitialised memory. */
int ex4d_attributes_backward(const Ex4dAttrParams *a,
    const float *opacity, const float *scaling, const float *rotation_motion, const float *opacity_motion,
    const float *opacity_duration_center, const float *opacity_duration_var, const float *scaling_motion,
    const float *g_means3D, const float *g_rotations, const float *g_opacities, const float *g_scales, const float *g_shs,
    float *g_xyz, float *g_xyz_disp, float *g_rotation, float *g_opacity, float *g_scaling, float *g_features_dc, float *g_features_rest,
    float *g_xyz_motion, float *g_rotation_motion, float *g_opacity_motion, float *g_opacity_duration_center,
    float *g_opacity_duration_var, float *g_scaling_motion, float *g_features_dc_motion, float *g_features_rest_motion, void *stream);

/* The same backward with the keyframe gradients as SLICES instead of dense tensors: g_xyz_motion_slices[Nd,4,3] holds the gradients of
 * keyframes slices[0] .. slices[0]+3, g_rotation_motion_slices[Nd,2,4] those of keyframes slices[2], slices[2]+1 -- every other time
 * slice of the dense gradient is zero for this timestamp.  slices = int32[4] {xyz first, xyz count (4), rotation first, rotation count (2)},
 * written on the host (the slice hint an optimizer / gradient exchange needs; this is the cube interpolator's window, see
 * ex4d_attributes_backward_sliced_ex for the others).  No zero fill of 7 K floats per dynamic Gaussian, and
 * ex4d_radam_step_sliced (ex4d_optim.h) consumes the slices directly. */
int ex4d_attributes_backward_sliced(const Ex4dAttrParams *a,
    const float *opacity, const float *scaling, const float *rotation_motion, const float *opacity_motion,
    const float *opacity_duration_center, const float *opacity_duration_var, const float *scaling_motion,
    const float *g_means3D, const float *g_rotations, const float *g_opacities, const float *g_scales, const float *g_shs,
    float *g_xyz, float *g_xyz_disp, float *g_rotation, float *g_opacity, float *g_scaling, float *g_features_dc, float *g_features_rest,
    float *g_xyz_motion_slices, float *g_rotation_motion_slices, float *g_opacity_motion, float *g_opacity_duration_center,
    float *g_opacity_duration_var, float *g_scaling_motion, float *g_features_dc_motion, float *g_features_rest_motion,
    int32_t *slices, void *stream);

/* The scalars of one timestamp for `interp`, from the model's Python numbers: the arithmetic above in double, Python's `//` and `%`.
 * Pure host code (no GPU needed).  EX4D_ERR_ARG for an unknown interpolator; the keyframe index is checked by the calls below. */
int ex4d_attr_time_scalars(int32_t interp, double duration, double interval, double time_shift, double var_pad,
                           int32_t Ns, int32_t Nd, int32_t K, double timestamp, Ex4dAttrParams *out);

/* The three calls above with the position interpolator as an argument (EX4D_INTERP_*); the ones above are these with EX4D_INTERP_CUBE.
 * An unknown interpolator and a keyframe index outside the interpolator's valid range are refused with EX4D_ERR_ARG before anything
 * is launched.  The backward calls also take xyz_motion[Nd,K,3]: the pchip adjoint depends on the keyframe positions (it may be NULL
 * for the other two).  Sliced: the position window is {k, 2} for linear -- g_xyz_motion_slices is [Nd,2,3] -- and {k-1, 4} otherwise;
 * `slices` says which. */
int ex4d_attributes_forward_ex(const Ex4dAttrParams *a, int32_t interp,
    const float *xyz, const float *xyz_disp, const float *rotation, const float *opacity,
    const float *scaling, const float *features_dc, const float *features_rest,
    const float *xyz_motion, const float *rotation_motion, const float *opacity_motion,
    const float *opacity_duration_center, const float *opacity_duration_var,
    const float *scaling_motion, const float *features_dc_motion, const float *features_rest_motion,
    float *means3D, float *rotations, float *opacities, float *scales, float *shs, void *stream);

int ex4d_attributes_backward_ex(const Ex4dAttrParams *a, int32_t interp, const float *xyz_motion,
    const float *opacity, const float *scaling, const float *rotation_motion, const float *opacity_motion,
    const float *opacity_duration_center, const float *opacity_duration_var, const float *scaling_motion,
    const float *g_means3D, const float *g_rotations, const float *g_opacities, const float *g_scales, const float *g_shs,
    float *g_xyz, float *g_xyz_disp, float *g_rotation, float *g_opacity, float *g_scaling, float *g_features_dc, float *g_features_rest,
    float *g_xyz_motion, float *g_rotation_motion, float *g_opacity_motion, float *g_opacity_duration_center,
    float *g_opacity_duration_var, float *g_scaling_motion, float *g_features_dc_motion, float *g_features_rest_motion, void *stream);

int ex4d_attributes_backward_sliced_ex(const Ex4dAttrParams *a, int32_t interp, const float *xyz_motion,
    const float *opacity, const float *scaling, const float *rotation_motion, const float *opacity_motion,
    const float *opacity_duration_center, const float *opacity_duration_var, const float *scaling_motion,
    const float *g_means3D, const float *g_rotations, const float *g_opacities, const float *g_scales, const float *g_shs,
    float *g_xyz, float *g_xyz_disp, float *g_rotation, float *g_opacity, float *g_scaling, float *g_features_dc, float *g_features_rest,
    float *g_xyz_motion_slices, float *g_rotation_motion_slices, float *g_opacity_motion, float *g_opacity_duration_center,
    float *g_opacity_duration_var, float *g_scaling_motion, float *g_features_dc_motion, float *g_features_rest_motion,
    int32_t *slices, void *stream);

/* ---- Motion: the displacement of every Gaussian between two timestamps t0 and t1 (ex4d_motion.hip).
 *
 * a0, a1 are the scalars of t0 and t1 (ex4d_attr_time_scalars, same model); only the position tensors are read.
 *   EX4D_MOTION_WORLD   out = x(t1) - x(t0), one float32 subtraction per component; x(t) is exactly the float32 value
 *                       ex4d_attributes_forward_ex writes to means3D for that timestamp (its position arithmetic is restated).
 *   EX4D_MOTION_SCREEN  out = (u1 - u0, v1 - v0, z1 - z0): (u, v) is the pixel position the rasterizer's preprocess computes for that
 *                       mean (full projection, inv_w = 1 / (w + 1e-7f), ndc2Pix in double), z its view depth -- the bits the geometry
 *                       records hold.  Needs viewmatrix[16], projmatrix[16] (device, column-major as the rasterizer takes them), W, H.
 *                       A row whose view depth is <= min_depth at either timestamp gets exactly (0, 0, 0) and zero gradients; no other
 *                       culling (the rasterizer culls by the frame it renders).  Units: pixels and scene depth per (t1 - t0): fed
 *                       to the rasterizer as dir3D, out_flow is the optical flow in pixels.
 * out is [Ns+Nd,3], static rows first, every row written (callers may pass uninitialised memory).  One launch, no atomics, no host
 * read-back: graph-capturable.  Ns == 0 or Nd == 0 is legal.
 *
 * Refused with EX4D_ERR_ARG before anything is launched (text: ex4d_motion_last_error): an unknown interpolator or space, a keyframe
 * index outside the interpolator's valid range at either timestamp, a0 and a1 that disagree in Ns, Nd or K, screen space without
 * matrices or image size. */
enum { EX4D_MOTION_WORLD = 0, EX4D_MOTION_SCREEN = 1 };

const char *ex4d_motion_last_error(void);

int ex4d_motion_forward(const Ex4dAttrParams *a0, const Ex4dAttrParams *a1, int32_t interp, int32_t space,
    const float *xyz /*[Ns,3]*/, const float *xyz_disp /*[Ns,3]*/, const float *xyz_motion /*[Nd,K,3]*/,
    const float *viewmatrix, const float *projmatrix, int32_t W, int32_t H, float min_depth,
    float *out /*[Ns+Nd,3]*/, void *stream);

/* Backward of the above for g_out[Ns+Nd,3].  g_xyz[Ns,3] and g_xyz_disp[Ns,3] are fully written (world space: g_xyz is exact zeros).
 * The keyframe gradient comes as TWO WINDOWS, without a dense zero fill: g_win0 holds the gradients of keyframes windows[0] ..
 * windows[0]+windows[1]-1 that flow through x(t0), g_win1 those of windows[2] .. through x(t1); each is [Nd,4,3] ([Nd,2,3] under
 * linear) and fully written.  windows = int32[4] {first0, count, first1, count}, written on the host: {k0-1, 4, k1-1, 4}, linear
 * {k0, 2, k1, 2} -- the form ex4d_radam_step_sliced takes as two windows of one tensor.  The dense gradient is window 0 plus
 * window 1, summed in that order where they overlap.  The adjoints are those of ex4d_attributes_backward_ex (pchip: NaN on the
 * keyframes the quotient touches where y[k+1] == y[k-1], as there). */
int ex4d_motion_backward(const Ex4dAttrParams *a0, const Ex4dAttrParams *a1, int32_t interp, int32_t space,
    const float *xyz, const float *xyz_disp, const float *xyz_motion,
    const float *viewmatrix, const float *projmatrix, int32_t W, int32_t H, float min_depth,
    const float *g_out, float *g_xyz, float *g_xyz_disp, float *g_win0, float *g_win1, int32_t *windows, void *stream);

#ifdef __cplusplus
}
#endif
#endif
