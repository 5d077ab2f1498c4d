/*
 * ex4d_trainer.h -- C ABI of the compiled host path of one training iteration.
 *
 * One call = the per-iteration device work of the reference's training loop for one view (train.py:124-153, :244-255), driven from C++
 * with a workspace that lives across iterations -- no Python, no autograd graph, no per-iteration allocation:
 *     ex4d_attributes_forward                  (getters of scene/c_gaussian_model.py:170-215, :330-375)
 *  -> ex4d_forward_split_sh                    (render: gaussian_renderer/__init__.py:19-124, the SH tensors as the model stores them)
 *  -> ex4d_l1_ssim_forward / _backward         (train.py:144-151, utils/loss_utils.py; their _u8 forms in ex4d_trainer_step_u8)
 *  -> ex4d_backward_split_sh
 *  -> ex4d_attributes_backward_sliced          (keyframe gradients as the 4 / 2 touched time slices)
 *  -> ex4d_radam_step + ex4d_radam_step_sliced (scene/c_gaussian_model.py:430-449, train.py:250)
 * all on the caller's stream.  The rasterizer's scratch buffers are capacity-bounded arenas of the trainer (grown geometrically when
 * a frame needs more), so the only host <-> device synchronisation of an iteration is the instance-count read-back the reference has
 * too (rasterizer_impl.cu:298-299), which overlaps the depth sort.
 *
 * SCOPE: this is the render + L1/SSIM + regularisers + RAdam core of the iteration, and -- through ex4d_trainer_step_ex -- the
 * per-frame steps the reference's default schedule adds around it: the l1_accum error hook on the flow output (train.py:148-153:
 * viewspace_l1points.grad is output 7), the densification statistics (train.py:199-216, ex4d_densify_stats on the trainer's own
 * tensors), an iteration whose optimizer step is skipped (train.py densifies before optimizer.step()) and the NaN gate of
 * prune_nan_points (train.py:253).  The regularisers static_reg / motion_reg / rot_reg (train.py:156-168) are off until
 * ex4d_trainer_set_regularizers gives them weights; the keyframe terms, dense over all K, are formed inside
 * ex4d_radam_step_sliced_reg, so the keyframe gradients stay slices.  Density control and growth themselves (ex4d_densify.h) change
 * the row counts: the caller reads the moments (ex4d_trainer_read 200 + i / 300 + i) and the step count, destroys the trainer,
 * creates one over the new tensors and writes them back (ex4d_trainer_write, ex4d_trainer_set_step); an in-place resize of the
 * workspace is not part of this interface.  What the loop changes over time is settable: ex4d_trainer_set_lr (the position
 * learning-rate schedule, update_learning_rate) and ex4d_trainer_set_sh_degree (oneupSHdegree every 1000 iterations).
 * _opacity_duration_var's gradient is read through nan_to_num like train.py:244-247 does before optimizer.step().
 *
 * The 15 parameter tensors stay the caller's (device pointers, CGaussianModel order, float32 contiguous); they are updated in place.
 * Optimizer state (exp_avg, exp_avg_sq, step counts) and every intermediate belong to the trainer.
 */
#ifndef EX4D_TRAINER_H_INCLUDED
#define EX4D_TRAINER_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EX4D_TRAINER_PARAMS 15      /* _xyz _xyz_disp _rotation _opacity _scaling _features_dc _features_rest _xyz_motion _rotation_motion
                                       _opacity_motion _opacity_duration_center _opacity_duration_var _scaling_motion _features_dc_motion
                                       _features_rest_motion   (ex4dgs_amd/attributes.py: PARAM_ORDER) */

typedef struct Ex4dTrainerConfig {
    int32_t Ns, Nd, K;                  /* static / dynamic Gaussians, keyframes per dynamic Gaussian */
    int32_t W, H;
    int32_t sh_degree;                  /* active SH degree (0..3) */
    float tanfovx, tanfovy, kernel_size;
    float min_depth, max_depth;
    double duration, interval, time_shift, var_pad;     /* the Python numbers of c_gaussian_model.py:184-186, :364 */
    float lambda_dssim;
    float window[11];                   /* normalised 1-D SSIM taps (utils/loss_utils.py:32-34), float32 as the reference computes them */
    double lr[EX4D_TRAINER_PARAMS];
    double beta1, beta2, eps;
    int32_t optimizer;                  /* 0: gradients only (ex4d_trainer_grad reads them), 1: RAdam step */
} Ex4dTrainerConfig;

typedef struct Ex4dTrainer Ex4dTrainer;

const char *ex4d_trainer_last_error(void);

/* params: HOST array of the 15 device pointers.  Returns NULL on failure (ex4d_trainer_last_error). */
Ex4dTrainer *ex4d_trainer_create(const Ex4dTrainerConfig *cfg, float *const *params);
void ex4d_trainer_destroy(Ex4dTrainer *t);

/* The host-side scalars of one timestamp exactly as the Python reference computes them (float floor division / modulo / ** in double,
 * then float32) -- what ex4d_trainer_step passes to ex4d_attributes_forward; exported so that the arithmetic can be pinned without a GPU.
 * This is ex4d_attr_time_scalars (ex4d_attributes.h) for the cube interpolator; a trainer told another one uses that call with it. */
struct Ex4dAttrParams;
void ex4d_trainer_time_scalars(const Ex4dTrainerConfig *cfg, double timestamp, struct Ex4dAttrParams *out);

/* One iteration at timestamp t for the camera (viewmatrix [16], projmatrix [16], campos [3]: device), background [3] (device) against
 * gt_image [3,H,W] (device).  Asynchronous on `stream` apart from the instance-count read-back.  Returns EX4D_OK or an error code of
 * ex4d_rasterizer.h.  *num_rendered (host, may be NULL) receives the instance count. */
int ex4d_trainer_step(Ex4dTrainer *t, double timestamp, const float *viewmatrix, const float *projmatrix, const float *campos,
                      const float *background, const float *gt_image, void *stream, int32_t *num_rendered);

/* The same iteration with the per-frame policy steps of the reference's loop; opt = NULL is ex4d_trainer_step. */
typedef struct Ex4dTrainerStepOptions {
    int32_t l1_accum;        /* 1: train.py:148-153 -- stack([acc[0], l1_errors, ssim_errors]) (output 8) is dL_dout_flow; dir3D stays
                                NULL (zeros), so dL_ddir [P,3] is the per-Gaussian error gradient (e0, e1, e2): output 7 */
    int32_t skip_optimizer;  /* 1: gradients and statistics only; no regulariser backward, no RAdam, step count not advanced */
    int32_t stats_flags;     /* EX4D_DENSIFY_* of ex4d_densify.h, 0 = no statistics; PRUNE_STATS / L1_STATS need l1_accum.  Counted once
                                per step, after an overflowing asynchronous frame has been re-run */
    int32_t nan_census;      /* 1: after the optimizer step, flag NaN rows of _xyz / _xyz_motion (ex4d_nan_any) for ex4d_trainer_report */
    float *stats_s, *stats_d;   /* caller-owned [9,Ns] / [9,Nd] blocks (DensityStats.static / .dynamic) */
} Ex4dTrainerStepOptions;
int ex4d_trainer_step_ex(Ex4dTrainer *t, double timestamp, const float *viewmatrix, const float *projmatrix, const float *campos,
                         const float *background, const float *gt_image, void *stream, int32_t *num_rendered,
                         const Ex4dTrainerStepOptions *opt);
/* ex4d_trainer_step_ex against ground truth as decoded: gt_u8 is DEVICE uint8 [H,W,pixel_stride] (3 or 4 bytes per pixel, any byte
 * alignment -- a frame of a resident store), lut the HOST table of ex4d_l1_ssim_forward_u8 (NULL = u / 255).  The same sequence with
 * every option, report and re-run; its two loss calls are the _u8 ones, and a re-run frame reads gt_u8 again, so the frame has to
 * stay as it is until the step's work on `stream` is done.  opt = NULL is the plain step. */
int ex4d_trainer_step_u8(Ex4dTrainer *t, double timestamp, const float *viewmatrix, const float *projmatrix, const float *campos,
                         const float *background, const uint8_t *gt_u8, int32_t pixel_stride, const float *lut /* host [256] or NULL */,
                         void *stream, int32_t *num_rendered, const Ex4dTrainerStepOptions *opt);

/* What a loop reads back per iteration: at the end of every ex4d_trainer_step_ex with options the loss word and the two census flags
 * are copied to pinned host memory behind an event; ex4d_trainer_report waits for that event -- the one wait that stands for
 * loss.item() and the count read-back of prune_nan_points.  nan_static / nan_dynamic: 1 = some element of _xyz / _xyz_motion is NaN
 * (0 when the step did not ask for the census).  EX4D_ERR_ARG before the first such step. */
typedef struct Ex4dTrainerReport {
    float loss;
    int32_t nan_static, nan_dynamic;
    int32_t reserved;
} Ex4dTrainerReport;
int ex4d_trainer_report(Ex4dTrainer *t, Ex4dTrainerReport *out);

/* The per-group learning rates (15, PARAM order) / the active SH degree used from the next step on: update_learning_rate
 * (c_gaussian_model.py:451-470) and oneupSHdegree (train.py:113-114) of the reference change them during training. */
int ex4d_trainer_set_lr(Ex4dTrainer *t, const double *lr15);
int ex4d_trainer_set_sh_degree(Ex4dTrainer *t, int32_t degree);
/* on != 0: the rasterizer forward runs ASYNCHRONOUSLY (ex4d_rasterizer.h: Ex4dParams.instance_capacity) -- no instance-count read-back
 * in the middle of the frame; the binning arena is sized for 1.25 x the largest instance count seen (the first frame runs synchronously
 * and seeds it), the frame's status is looked at once, right before the optimizer step, and a frame that overflowed its capacity is run
 * again before anything is applied: same parameters as the synchronous path.  ex4d_trainer_replays counts such re-runs. */
int ex4d_trainer_set_async(Ex4dTrainer *t, int32_t on);
int64_t ex4d_trainer_replays(const Ex4dTrainer *t);
/* The position interpolator of the dynamic Gaussians (EX4D_INTERP_* of ex4d_attributes.h; the default is EX4D_INTERP_CUBE): the step
 * then runs ex4d_attributes_forward_ex / _backward_sliced_ex with it and hands the 2-slice (linear) or 4-slice position window to
 * ex4d_radam_step_sliced / _reg; gradient 7 is [Nd,2,3] for linear.  The configuration is as before: the caller passes the model's own
 * time_shift (time_pad for linear, time_pad + interval otherwise).  Allowed before the first step of this handle only: EX4D_ERR_ARG
 * afterwards and for an unknown value.  A trainer created after density control replaced the tensors is told again. */
int ex4d_trainer_set_interp(Ex4dTrainer *t, int32_t interp);
/* Weights of the motion regularisers (ex4d_regularizers.h) from the next step on, as they act at that iteration -- the iteration gates
 * of train.py:156-163 are the caller's (regularizers.regularizer_weights).  All 0 (the default) = off: the sequence above, unchanged.
 * On: ex4d_reg_forward fills output 6, _xyz_disp's term is added to its gradient, the keyframe terms go through
 * ex4d_radam_step_sliced_reg.  Needs optimizer = 1; EX4D_ERR_ARG when K is too large for that step. */
int ex4d_trainer_set_regularizers(Ex4dTrainer *t, double static_reg, double motion_reg, double rot_reg);

/* Device pointers into the trainer's workspace, valid until the next step / destroy:
 * what = 0 loss [1], 1 render [3,H,W], 2 radii int32 [P], 3 dL_dmeans2D [P,3] (viewspace gradient, densification statistics),
 *        4 depth [1,H,W], 5 acc [1,H,W], 6 regularisers float[4] = {static mean, motion mean, rot mean, weighted sum} of the last step
 *        that had them on (zeros before); the loss of what = 0 stays the L1/SSIM loss,
 *        7 error gradient [P,3] (dL_ddir: (e0, e1, e2) of the last l1_accum step), 8 hook [3,H,W] (plane 0 is
 *        output 5; planes 1, 2 = l1_errors, ssim_errors of the last l1_accum step). */
const void *ex4d_trainer_output(const Ex4dTrainer *t, int32_t what);
/* Gradient of parameter i of the last step: dense [shape of the parameter] except i = 7 (_xyz_motion: [Nd,4,3]) and i = 8
 * (_rotation_motion: [Nd,2,4]), the slices of ex4d_attributes_backward_sliced; slices4 (host int32[4], may be NULL) receives
 * {xyz first, 4, rotation first, 2}.  Under the linear interpolator gradient 7 is [Nd,2,3] and the hint {xyz first, 2, ...}. */
const float *ex4d_trainer_grad(const Ex4dTrainer *t, int32_t i, int32_t *slices4);
/* Asynchronous device-to-device copy of one of the buffers above into caller memory (bindings that cannot wrap a raw pointer):
 * what = 0..8 as in ex4d_trainer_output, 100 + i = gradient of parameter i, 200 + i = exp_avg and 300 + i = exp_avg_sq of parameter i
 * (optimizer = 1 only; the parameter's shape).  `bytes` must not exceed the buffer's size. */
int ex4d_trainer_read(const Ex4dTrainer *t, int32_t what, void *dst, size_t bytes, void *stream);
/* The inverse of ex4d_trainer_read for the optimizer state: what = 200 + i / 300 + i only; src is device memory.  With the step count
 * below this moves a trainer's state into the one created after density control replaced the parameter tensors. */
int ex4d_trainer_write(Ex4dTrainer *t, int32_t what, const void *src, size_t bytes, void *stream);
/* RAdam's step count (the number of optimizer steps applied so far). */
int ex4d_trainer_get_step(const Ex4dTrainer *t, int64_t *step);
int ex4d_trainer_set_step(Ex4dTrainer *t, int64_t step);
/* bytes of device memory the trainer holds (workspace + optimizer state + arenas) */
size_t ex4d_trainer_bytes(const Ex4dTrainer *t);

#ifdef __cplusplus
}
#endif
#endif
