/*
 * ex4d_regularizers.h -- C ABI of the three motion regularisers the reference adds to the loss of every iteration from
 * iteration ~400 on (train.py:155-168; every shipped configuration switches static_reg and motion_reg on):
 *     static  = mean_i        log(|_xyz_disp[i]| + 0.001)                                           over the Ns static Gaussians
 *     motion  = mean_{i,k>=1} |_xyz_motion[i,0] - _xyz_motion[i,k]|                                 (against keyframe 0, not the neighbour)
 *     rot     = mean_{i,k>=1} 1 - <r_k, r_{k-1}> / max(|r_k|, 1e-6) / max(|r_{k-1}|, 1e-6)          on _rotation_motion
 * Quirks kept: the norm's gradient is 0 where the norm is 0 (torch's norm backward); clamp_min passes no gradient to a norm below
 * 1e-6, but the clamped value still divides.  A mean over nothing (Ns = 0, Nd = 0 or K = 1) is 0 with zero gradients here.
 *
 * None of the gradients needs a global reduction: each is a function of one Gaussian's own row, the means only contribute the constants
 * 1/Ns and 1/(Nd (K-1)).  ex4d_radam_step_sliced_reg (ex4d_optim.h) therefore forms the keyframe terms inside the optimizer step from
 * the row it is about to update; the functions here are the stand-alone form (loss value, dense gradients for autograd and for the
 * dense-gradient paths).  Both share one per-row arithmetic (csrc/ex4d_reg_rows.h): the same bits either way.
 *
 * Several ranks: the term is added ONCE per optimizer step, last, to the gradient summed over ranks and views -- never before the
 * exchange.  The replicated optimizer adds ex4d_reg_backward to the reduced buffers (or runs the fused step on the gathered windows);
 * the sharded optimizer adds ex4d_reg_backward_range to the element range it owns, or hands its owned rows to the fused step.
 */
#ifndef EX4D_REGULARIZERS_H_INCLUDED
#define EX4D_REGULARIZERS_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char *ex4d_reg_last_error(void);

/* bytes of device scratch ex4d_reg_forward needs (per-workgroup partial sums in double; independent of the model's size) */
size_t ex4d_reg_scratch_bytes(void);

/* out4 (device float[4]) <- {static mean, motion mean, rot mean, static_reg*static + motion_reg*motion + rot_reg*rot}.
 * xyz_disp [Ns,3], xyz_motion [Nd,K,3], rotation_motion [Nd,K,4]: device, a NULL tensor (or zero rows) contributes a mean of 0.
 * Evaluated in double from the float32 parameters; per-workgroup partial sums and a one-block finish: no atomics, no host
 * synchronisation, the same bits on every call, capturable in a graph. */
int ex4d_reg_forward(const float *xyz_disp, int64_t Ns, const float *xyz_motion, const float *rotation_motion, int64_t Nd, int32_t K,
                     double static_reg, double motion_reg, double rot_reg, float *out4, void *scratch, void *stream);

/* Dense gradients of  static_reg*static + motion_reg*motion + rot_reg*rot  times *upstream (device float, NULL = 1):
 * g_xyz_disp [Ns,3], g_xyz_motion [Nd,K,3], g_rotation_motion [Nd,K,4]; a NULL gradient pointer skips that tensor.
 * accumulate = 0: every element is written once (zeros where the term is off); 1: added to what is there.
 * The per-row float32 arithmetic is the one of ex4d_radam_step_sliced_reg. */
int ex4d_reg_backward(const float *xyz_disp, float *g_xyz_disp, int64_t Ns, const float *xyz_motion, float *g_xyz_motion,
                      const float *rotation_motion, float *g_rotation_motion, int64_t Nd, int32_t K,
                      double static_reg, double motion_reg, double rot_reg, const float *upstream, int32_t accumulate, void *stream);

/* The gradient of ONE term over a flat element range [lo, hi) of its tensor: what a rank of the sharded optimizer adds to the summed
 * gradient of the elements it owns (dist.ShardedRAdam cuts dense tensors into element ranges, in the middle of rows and keyframes).
 * kind 1: motion_reg on [rows,K,3], 2: rot_reg on [rows,K,4] (reg_kind of ex4d_optim.h), 3: static_reg on [rows,3] (K is ignored).
 * param: base of the WHOLE tensor; rows: its full row count, the one of the mean's 1/rows or 1/(rows (K-1)); grad[0] belongs to
 * element lo (a view of a shard buffer).  A row the range cuts is read whole, elements outside [lo, hi) are not written.
 * Every element gets the bits ex4d_reg_backward gives it (upstream NULL): the same per-row arithmetic, the same coefficient.
 * accumulate = 0: every element of the range is written once (zeros where the term is off: weight 0, K = 1); 1: added.
 * lo == hi: EX4D_OK without a launch; lo < 0, hi > numel, lo > hi or an unknown kind: EX4D_ERR_ARG.  One launch of plain vector
 * stores, no atomics, capturable in a graph. */
int ex4d_reg_backward_range(int32_t kind, const float *param, int64_t rows, int32_t K, int64_t lo, int64_t hi, float *grad, double weight,
                            int32_t accumulate, void *stream);

#ifdef __cplusplus
}
#endif
#endif
