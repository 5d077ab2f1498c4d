// Compiled host path of one training iteration (include/ex4d_trainer.h): host code only -- it sequences the C-ABI entry points of
// this library on the caller's stream with a persistent workspace.  Nothing here runs on the CPU in place of a kernel.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>

#include "../../include/ex4d_attributes.h"
#include "../../include/ex4d_densify.h"
#include "../../include/ex4d_loss.h"
#include "../../include/ex4d_optim.h"
#include "../../include/ex4d_rasterizer.h"
#include "../../include/ex4d_regularizers.h"
#include "../../include/ex4d_trainer.h"
#include "ex4d_keyframes.h"

namespace {

// positions in the parameter order of EX4D_TRAINER_PARAMS (include/ex4d_trainer.h)
enum { XYZ, XYZ_DISP, ROTATION, OPACITY, SCALING, FEATURES_DC, FEATURES_REST, XYZ_MOTION, ROTATION_MOTION, OPACITY_MOTION,
       OPACITY_DURATION_CENTER, OPACITY_DURATION_VAR, SCALING_MOTION, FEATURES_DC_MOTION, FEATURES_REST_MOTION };
static_assert(FEATURES_REST_MOTION + 1 == EX4D_TRAINER_PARAMS, "one name per parameter");

thread_local char t_err[512] = "";

int tfail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(t_err, sizeof(t_err), fmt, ap);
    va_end(ap);
    return code;
}

// a device buffer that only ever grows (the rasterizer's opaque scratch buffers: the binning buffer depends on the frame's instance count)
struct Arena {
    void *ptr = nullptr;
    size_t cap = 0;
    size_t *total = nullptr;
    void *get(size_t bytes)
    {
        if (bytes <= cap) return ptr;
        // growth is rare (first frames, then never or when a view sees ~25 % more instances than any before it); hipFree waits for the
        // kernels still using the old buffer
        const size_t want = bytes + bytes / 4 + 256;
        void *p = nullptr;
        if (hipMalloc(&p, want) != hipSuccess) return nullptr;
        if (ptr) (void)hipFree(ptr);
        if (total) *total += want - cap;
        ptr = p; cap = want;
        return ptr;
    }
};
void *arena_alloc(void *user, size_t bytes) { return static_cast<Arena *>(user)->get(bytes); }

}  // namespace

struct Ex4dTrainer {
    Ex4dTrainerConfig cfg;
    int P = 0;
    size_t HW = 0;
    size_t bytes = 0;
    int64_t step = 0;
    float *param[EX4D_TRAINER_PARAMS] = {};
    int64_t numel[EX4D_TRAINER_PARAMS] = {};
    int64_t grad_numel[EX4D_TRAINER_PARAMS] = {};
    float *grad[EX4D_TRAINER_PARAMS] = {}, *m[EX4D_TRAINER_PARAMS] = {}, *v[EX4D_TRAINER_PARAMS] = {};
    int32_t slices[4] = { 0, 0, 0, 0 };
    // position interpolator of the dynamic Gaussians (ex4d_trainer_set_interp); frames counts the steps this handle has run
    int32_t interp = EX4D_INTERP_CUBE;
    int64_t frames = 0;
    // per-frame tensors
    float *means3D = nullptr, *rotations = nullptr, *opacities = nullptr, *scales = nullptr;
    float *color = nullptr, *depth = nullptr, *acc = nullptr, *flow = nullptr, *loss = nullptr, *dmaps = nullptr, *loss_scratch = nullptr;
    float *grad_img = nullptr, *grad_loss = nullptr;
    int32_t *idx = nullptr, *radii = nullptr;
    float *g_means2D = nullptr, *g_opacity = nullptr, *g_means3D = nullptr, *g_scales = nullptr,
          *g_rotations = nullptr, *g_dir = nullptr;
    void *bwd_scratch = nullptr;
    Arena geom, binning, img;
    // asynchronous rasterizer forward (ex4d_trainer_set_async): capacity of the binning buffer in tile instances (0 = not known yet: the
    // next frame runs synchronously and seeds it), the frame status in pinned host memory, the event behind the forward
    bool async = false;
    uint32_t capacity = 0;
    Ex4dFrameStatus *status = nullptr;
    hipEvent_t status_ev = nullptr;
    int64_t replays = 0;
    // motion regularisers (ex4d_trainer_set_regularizers): weights of the next steps, their float[4] output, the forward's scratch
    double reg_w[3] = { 0.0, 0.0, 0.0 };
    float *reg_out = nullptr;
    double *reg_scratch = nullptr;
    // the l1_accum hook [3,H,W] (train.py:148-153): plane 0 IS the accumulation image (`acc` points at it: the rasterizer forward writes
    // it in place), planes 1 and 2 receive l1_errors / ssim_errors from the loss forward of an l1_accum step
    float *hook = nullptr;
    // the report of ex4d_trainer_step_ex: the loss word and the two census flags are neighbours on the device ({loss, nan_static,
    // nan_dynamic, unused}: `loss` points at word 0), so one 16-byte copy brings them to pinned host memory behind report_ev
    int32_t *report_dev = nullptr;
    Ex4dTrainerReport *report = nullptr;
    hipEvent_t report_ev = nullptr;
    bool report_pending = false, report_census = false;
    void *owned[96] = {};
    int n_owned = 0;

    template <typename T> bool take(T *&p, size_t count, bool zero = false)
    {
        p = nullptr;
        if (count == 0) return true;
        void *q = nullptr;
        if (hipMalloc(&q, count * sizeof(T)) != hipSuccess) return false;
        if (zero && hipMemset(q, 0, count * sizeof(T)) != hipSuccess) { (void)hipFree(q); return false; }
        owned[n_owned++] = q;
        bytes += count * sizeof(T);
        p = static_cast<T *>(q);
        return true;
    }
};

extern "C" {

const char *ex4d_trainer_last_error(void) { return t_err; }

void ex4d_trainer_destroy(Ex4dTrainer *t)
{
    if (!t) return;
    (void)hipDeviceSynchronize();
    for (int i = 0; i < t->n_owned; i++) (void)hipFree(t->owned[i]);
    if (t->geom.ptr) (void)hipFree(t->geom.ptr);
    if (t->binning.ptr) (void)hipFree(t->binning.ptr);
    if (t->img.ptr) (void)hipFree(t->img.ptr);
    if (t->status) (void)hipHostFree(t->status);
    if (t->status_ev) (void)hipEventDestroy(t->status_ev);
    if (t->report) (void)hipHostFree(t->report);
    if (t->report_ev) (void)hipEventDestroy(t->report_ev);
    delete t;
}

Ex4dTrainer *ex4d_trainer_create(const Ex4dTrainerConfig *cfg, float *const *params)
{
    t_err[0] = 0;
    if (!cfg || !params) { tfail(1, "null config / parameter list"); return nullptr; }
    if (cfg->Ns < 0 || cfg->Nd < 0 || cfg->Ns + cfg->Nd <= 0 || cfg->W <= 0 || cfg->H <= 0 || (cfg->Nd > 0 && cfg->K < 4)
        || cfg->sh_degree < 0 || cfg->sh_degree > 3 || !(cfg->interval > 0.0)) {
        tfail(1, "trainer config out of range (Ns %d, Nd %d, K %d, %dx%d, SH degree %d)", cfg->Ns, cfg->Nd, cfg->K, cfg->W, cfg->H, cfg->sh_degree);
        return nullptr;
    }
    Ex4dTrainer *t = new (std::nothrow) Ex4dTrainer();
    if (!t) { tfail(3, "out of host memory"); return nullptr; }
    t->cfg = *cfg;
    t->P = cfg->Ns + cfg->Nd;
    t->HW = (size_t)cfg->W * cfg->H;
    t->geom.total = t->binning.total = t->img.total = &t->bytes;
    const int64_t Ns = cfg->Ns, Nd = cfg->Nd, K = cfg->K;
    const int64_t n[EX4D_TRAINER_PARAMS] = { Ns * 3, Ns * 3, Ns * 4, Ns, Ns * 3, Ns * 3, Ns * 45, Nd * K * 3, Nd * K * 4, Nd, Nd * 2, Nd * 2, Nd * 3, Nd * 3, Nd * 45 };
    bool ok = true;
    for (int i = 0; i < EX4D_TRAINER_PARAMS && ok; i++) {
        t->param[i] = params[i];
        t->numel[i] = n[i];
        t->grad_numel[i] = i == XYZ_MOTION ? Nd * ex4d_key_window(t->interp, 0).count * 3 : (i == ROTATION_MOTION ? Nd * 2 * 4 : n[i]);
        if (n[i] > 0 && !params[i]) { tfail(1, "parameter %d is NULL but has %lld elements", i, (long long)n[i]); ok = false; break; }
        ok = ok && t->take(t->grad[i], (size_t)t->grad_numel[i]);
        if (cfg->optimizer) ok = ok && t->take(t->m[i], (size_t)n[i], true) && t->take(t->v[i], (size_t)n[i], true);
    }
    const size_t P = (size_t)t->P, HW = t->HW;
    ok = ok && t->take(t->means3D, 3 * P) && t->take(t->rotations, 4 * P) && t->take(t->opacities, P) && t->take(t->scales, 3 * P)
            && t->take(t->color, 3 * HW) && t->take(t->depth, HW) && t->take(t->hook, 3 * HW) && t->take(t->flow, 3 * HW) && t->take(t->idx, HW)
            && t->take(t->radii, P) && t->take(t->report_dev, 4, true) && t->take(t->dmaps, 9 * HW)
            && t->take(t->loss_scratch, ex4d_l1_ssim_scratch_floats(cfg->H, cfg->W)) && t->take(t->grad_img, 3 * HW) && t->take(t->grad_loss, 1)
            && t->take(t->g_means2D, 3 * P) && t->take(t->g_opacity, P) && t->take(t->g_means3D, 3 * P)
            && t->take(t->g_scales, 3 * P) && t->take(t->g_rotations, 4 * P) && t->take(t->g_dir, 3 * P);
    if (ok) {
        void *s = nullptr;
        ok = t->take(reinterpret_cast<unsigned char *&>(s), ex4d_backward_scratch_bytes(t->P));
        t->bwd_scratch = s;
    }
    t->acc = t->hook;
    t->loss = reinterpret_cast<float *>(t->report_dev);
    ok = ok && t->take(t->reg_out, 4, true) && t->take(t->reg_scratch, ex4d_reg_scratch_bytes() / sizeof(double));
    if (ok) {
        const float one = 1.0f;
        ok = hipMemcpy(t->grad_loss, &one, sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) {
        if (!t_err[0]) tfail(3, "device allocation failed (%s)", hipGetErrorString(hipGetLastError()));
        ex4d_trainer_destroy(t);
        return nullptr;
    }
    return t;
}

// ex4d_attr_time_scalars for the cube interpolator, from the configuration (the arithmetic lives there)
void ex4d_trainer_time_scalars(const Ex4dTrainerConfig *cfg, double timestamp, Ex4dAttrParams *out)
{
    const Ex4dTrainerConfig &c = *cfg;
    (void)ex4d_attr_time_scalars(EX4D_INTERP_CUBE, c.duration, c.interval, c.time_shift, c.var_pad, c.Ns, c.Nd, c.K, timestamp, out);
}

int ex4d_trainer_step(Ex4dTrainer *t, double timestamp, const float *viewmatrix, const float *projmatrix, const float *campos,
                      const float *background, const float *gt_image, void *stream, int32_t *num_rendered)
{
    return ex4d_trainer_step_ex(t, timestamp, viewmatrix, projmatrix, campos, background, gt_image, stream, num_rendered, nullptr);
}

// the frame's ground truth: float32 [3,H,W] planes (f32) or uint8 [H,W,S] pixels with their host table (u8; include/ex4d_loss.h)
struct GroundTruth {
    const float *f32;
    const uint8_t *u8;
    int32_t pixel_stride;
    const float *lut;
};

// The one body of ex4d_trainer_step, _step_ex and _step_u8: they differ in which pair of loss entry points reads the ground truth.
static int step_body(Ex4dTrainer *t, double timestamp, const float *viewmatrix, const float *projmatrix, const float *campos,
                     const float *background, const GroundTruth &gt, void *stream, int32_t *num_rendered,
                     const Ex4dTrainerStepOptions *opt)
{
    t_err[0] = 0;
    if (!t || !viewmatrix || !projmatrix || !campos || !background || (!gt.f32 && !gt.u8)) return tfail(EX4D_ERR_ARG, "null argument");
    if (gt.u8 && gt.pixel_stride != 3 && gt.pixel_stride != 4)
        return tfail(EX4D_ERR_ARG, "pixel_stride %d: uint8 ground truth has 3 or 4 bytes per pixel", (int)gt.pixel_stride);
    const Ex4dTrainerConfig &c = t->cfg;
    const bool l1_accum = opt && opt->l1_accum, skip_optimizer = opt && opt->skip_optimizer, census = opt && opt->nan_census;
    const int32_t stats_flags = opt ? opt->stats_flags : 0;
    const int32_t error_stats = EX4D_DENSIFY_PRUNE_STATS | EX4D_DENSIFY_L1_STATS;
    if (stats_flags & ~(EX4D_DENSIFY_GRAD_STATS | error_stats)) return tfail(EX4D_ERR_ARG, "unknown statistics flags 0x%x", (unsigned)stats_flags);
    if ((stats_flags & error_stats) && !l1_accum)
        return tfail(EX4D_ERR_ARG, "PRUNE_STATS / L1_STATS read the error gradient: the step needs l1_accum");
    if (stats_flags && ((c.Ns > 0 && !opt->stats_s) || (c.Nd > 0 && !opt->stats_d))) return tfail(EX4D_ERR_ARG, "statistics asked for without their blocks");
    if (opt && !t->report) {
        if (hipHostMalloc((void **)&t->report, sizeof(Ex4dTrainerReport), hipHostMallocDefault) != hipSuccess) { t->report = nullptr; return tfail(EX4D_ERR_HIP, "pinned report allocation failed"); }
        memset(t->report, 0, sizeof(Ex4dTrainerReport));
        if (hipEventCreateWithFlags(&t->report_ev, hipEventDisableTiming) != hipSuccess) { t->report_ev = nullptr; return tfail(EX4D_ERR_HIP, "event creation failed"); }
    }
    float *const l1_errors = l1_accum ? t->hook + t->HW : nullptr, *const ssim_errors = l1_accum ? t->hook + 2 * t->HW : nullptr;
    const float *const dL_dout_flow = l1_accum ? t->hook : nullptr;
    Ex4dAttrParams a;
    if (ex4d_attr_time_scalars(t->interp, c.duration, c.interval, c.time_shift, c.var_pad, c.Ns, c.Nd, c.K, timestamp, &a))
        return tfail(EX4D_ERR_ARG, "time scalars: %s", ex4d_attributes_last_error());
    t->frames += 1;
    float *const *p = t->param;
    if (ex4d_attributes_forward_ex(&a, t->interp, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11], p[12], p[13], p[14],
                                t->means3D, t->rotations, t->opacities, t->scales, nullptr, stream))
        return tfail(EX4D_ERR_HIP, "attributes forward: %s", ex4d_attributes_last_error());

    Ex4dParams prm;
    prm.P = t->P; prm.D = c.sh_degree; prm.M = 16; prm.W = c.W; prm.H = c.H; prm.tanfovx = c.tanfovx; prm.tanfovy = c.tanfovy;
    prm.kernel_size = c.kernel_size; prm.scale_modifier = 1.0f; prm.min_depth = c.min_depth; prm.max_depth = c.max_depth;
    prm.prefiltered = 0; prm.debug = 0; prm.prepare_backward = 1; prm.instance_capacity = 0; prm.assume_no_flow = 0; prm.reserved = 0;
    Ex4dSplitSH sh;
    sh.dc[0] = p[FEATURES_DC]; sh.rest[0] = p[FEATURES_REST]; sh.dc[1] = p[FEATURES_DC_MOTION]; sh.rest[1] = p[FEATURES_REST_MOTION]; sh.n_static = c.Ns;
    Ex4dSplitSHGrad gsh;
    gsh.dc[0] = t->grad[FEATURES_DC]; gsh.rest[0] = t->grad[FEATURES_REST]; gsh.dc[1] = t->grad[FEATURES_DC_MOTION]; gsh.rest[1] = t->grad[FEATURES_REST_MOTION];
    gsh.n_static = c.Ns;
    float *const *g = t->grad;
    // Asynchronous mode: the forward does not wait for the instance count (the reference's one host synchronisation per frame,
    // rasterizer_impl.cu:298-299); the frame's status is looked at once, right before the optimizer step -- by then every kernel of the
    // frame is enqueued, the GPU has work for the rest of the iteration, and the status copy (it sits behind the tile scan, early in the
    // frame) has usually landed.  A frame whose instance count exceeded the capacity is simply run again with a larger one before anything
    // is applied: the parameters see exactly the gradients of the synchronous path.
    for (int attempt = 0; ; attempt++) {
        const bool async_frame = t->async && t->capacity > 0;
        prm.instance_capacity = async_frame ? (int32_t)t->capacity : 0;
        prm.assume_no_flow = async_frame ? 1 : 0;            // (dir3D is NULL: no Gaussian carries a flow vector)
        int32_t R = 0;
        int rc = ex4d_forward_split_sh(&prm, background, t->means3D, nullptr, &sh, t->opacities, t->scales, t->rotations, nullptr,
                                       viewmatrix, projmatrix, campos, nullptr, arena_alloc, &t->geom, arena_alloc, &t->binning, arena_alloc, &t->img,
                                       t->color, t->radii, t->depth, t->acc, t->flow, t->idx, stream,
                                       async_frame ? reinterpret_cast<int32_t *>(t->status) : &R);
        if (rc) return tfail(rc, "rasterizer forward: %s", ex4d_last_error());
        if (async_frame) {
            if (hipEventRecord(t->status_ev, (hipStream_t)stream) != hipSuccess) return tfail(EX4D_ERR_HIP, "event record failed");
            R = (int32_t)t->capacity;                        // the backward lays the buffers out for the capacity
        }

        // (a frame re-run after an overflow reads the same ground truth again)
        if (gt.u8 ? ex4d_l1_ssim_forward_u8(c.H, c.W, t->color, gt.u8, gt.pixel_stride, gt.lut, c.lambda_dssim, c.window, t->loss, l1_errors, ssim_errors,
                                            t->dmaps, t->loss_scratch, stream)
                  : ex4d_l1_ssim_forward(3, c.H, c.W, t->color, gt.f32, c.lambda_dssim, c.window, t->loss, l1_errors, ssim_errors, t->dmaps, t->loss_scratch, stream))
            return tfail(EX4D_ERR_HIP, "loss forward: %s", ex4d_loss_last_error());
        if (gt.u8 ? ex4d_l1_ssim_backward_u8(c.H, c.W, t->color, gt.u8, gt.pixel_stride, gt.lut, c.lambda_dssim, c.window, t->dmaps, t->grad_loss, t->grad_img, stream)
                  : ex4d_l1_ssim_backward(3, c.H, c.W, t->color, gt.f32, c.lambda_dssim, c.window, t->dmaps, t->grad_loss, t->grad_img, stream))
            return tfail(EX4D_ERR_HIP, "loss backward: %s", ex4d_loss_last_error());

        rc = ex4d_backward_split_sh(&prm, R, background, t->means3D, t->radii, &sh, t->scales, t->rotations, nullptr, viewmatrix, projmatrix, campos,
                                    nullptr, t->depth, t->acc, t->geom.ptr, t->binning.ptr, t->img.ptr, t->grad_img, nullptr, dL_dout_flow, nullptr,
                                    t->g_means2D, nullptr, t->g_opacity, t->g_means3D, nullptr, &gsh, t->g_scales, t->g_rotations, t->g_dir,
                                    t->bwd_scratch, stream);
        if (rc) return tfail(rc, "rasterizer backward: %s", ex4d_last_error());

        if (ex4d_attributes_backward_sliced_ex(&a, t->interp, p[XYZ_MOTION], p[3], p[4], p[8], p[9], p[10], p[11], p[12],
                                            t->g_means3D, t->g_rotations, t->g_opacity, t->g_scales, nullptr,
                                            g[0], g[1], g[2], g[3], g[4], nullptr, nullptr, g[7], g[8], g[9], g[10], g[11], g[12], nullptr, nullptr,
                                            t->slices, stream))
            return tfail(EX4D_ERR_HIP, "attributes backward: %s", ex4d_attributes_last_error());

        uint32_t count = (uint32_t)R;
        if (async_frame) {
            if (hipEventSynchronize(t->status_ev) != hipSuccess) return tfail(EX4D_ERR_HIP, "event wait failed");
            count = t->status->num_rendered;
        }
        if (num_rendered) *num_rendered = (int32_t)count;
        const uint32_t want = count + count / 4 + 4096;      // 25 % headroom over the largest frame seen
        const bool overflow = async_frame && count > t->capacity;
        if (t->async && want > t->capacity) t->capacity = want < 0x7FFFFFFFu ? want : 0x7FFFFFFFu;
        if (!overflow) break;
        if (attempt >= 2) return tfail(EX4D_ERR_HIP, "internal: the frame overflowed its instance capacity three times");
        t->replays++;
    }

    // train.py:199-216 on the frame that counts: a frame re-run after an overflow has left the loop exactly once
    if (stats_flags) {
        const int rc = ex4d_densify_stats(opt->stats_s, c.Ns, opt->stats_d, c.Nd, t->radii, t->g_means2D, l1_accum ? t->g_dir : nullptr,
                                          (float)timestamp, stats_flags, stream);
        if (rc) return tfail(rc, "statistics: %s", ex4d_densify_last_error());
    }

    const bool reg = !skip_optimizer && (t->reg_w[0] != 0.0 || t->reg_w[1] != 0.0 || t->reg_w[2] != 0.0);
    if (reg) {
        // train.py:155-168: the three terms at this iteration's parameters; the L1/SSIM loss stays in loss[1]
        if (ex4d_reg_forward(p[XYZ_DISP], c.Ns, p[XYZ_MOTION], p[ROTATION_MOTION], c.Nd, c.K, t->reg_w[0], t->reg_w[1], t->reg_w[2], t->reg_out, t->reg_scratch, stream))
            return tfail(EX4D_ERR_HIP, "regularisers: %s", ex4d_reg_last_error());
        // _xyz_disp's term joins its dense gradient; the keyframe terms are formed inside the sliced optimizer step below
        if (c.optimizer && ex4d_reg_backward(p[XYZ_DISP], g[XYZ_DISP], c.Ns, nullptr, nullptr, nullptr, nullptr, 0, 1, t->reg_w[0], 0.0, 0.0, nullptr, 1, stream))
            return tfail(EX4D_ERR_HIP, "regularisers: %s", ex4d_reg_last_error());
    }
    if (c.optimizer && !skip_optimizer) {
        t->step += 1;
        Ex4dRadamTensor dense[EX4D_TRAINER_PARAMS];
        Ex4dRadamSlicedRegTensor slr[2];
        int nd = 0, ns = 0;
        for (int i = 0; i < EX4D_TRAINER_PARAMS; i++) {
            if (t->numel[i] == 0) continue;
            if (i == XYZ_MOTION || i == ROTATION_MOTION) {
                const bool motion = i == XYZ_MOTION;
                Ex4dRadamSlicedRegTensor &sr = slr[ns++];
                memset(&sr, 0, sizeof(sr));
                Ex4dRadamSlicedTensor &s = sr.t;
                sr.reg_kind = motion ? 1 : 2; sr.reg_weight = t->reg_w[motion ? 1 : 2]; sr.reg_rows = c.Nd;
                s.param = p[i]; s.exp_avg = t->m[i]; s.exp_avg_sq = t->v[i]; s.rows = c.Nd; s.K = c.K; s.C = motion ? 3 : 4;
                s.lr = c.lr[i]; s.step = t->step; s.n_windows = 1;
                s.first[0] = t->slices[motion ? 0 : 2]; s.count[0] = t->slices[motion ? 1 : 3]; s.grad[0] = g[i];
            } else {
                Ex4dRadamTensor &q = dense[nd++];
                memset(&q, 0, sizeof(q));
                q.nan_to_num = i == OPACITY_DURATION_VAR;      // train.py:244-247: its gradient goes through nan_to_num() before optimizer.step()
                q.param = p[i]; q.grad = g[i]; q.exp_avg = t->m[i]; q.exp_avg_sq = t->v[i]; q.numel = t->numel[i]; q.lr = c.lr[i]; q.step = t->step;
            }
        }
        if (nd && ex4d_radam_step(dense, nd, c.beta1, c.beta2, c.eps, stream)) return tfail(EX4D_ERR_HIP, "RAdam: %s", ex4d_optim_last_error());
        if (ns && reg) {
            if (ex4d_radam_step_sliced_reg(slr, ns, c.beta1, c.beta2, c.eps, stream)) return tfail(EX4D_ERR_HIP, "RAdam (sliced, regularised): %s", ex4d_optim_last_error());
        } else if (ns) {
            Ex4dRadamSlicedTensor sl[2];
            for (int i = 0; i < ns; i++) sl[i] = slr[i].t;
            if (ex4d_radam_step_sliced(sl, ns, c.beta1, c.beta2, c.eps, stream)) return tfail(EX4D_ERR_HIP, "RAdam (sliced): %s", ex4d_optim_last_error());
        }
    }
    if (opt) {
        // train.py:253 (prune_nan_points' gate, c_gaussian_model.py:1230, :1234) at the parameters the optimizer step just left
        const int rc = census ? ex4d_nan_any(p[XYZ], t->numel[XYZ], p[XYZ_MOTION], t->numel[XYZ_MOTION], t->report_dev + 1, stream) : EX4D_OK;
        if (rc) return tfail(rc, "NaN census: %s", ex4d_densify_last_error());
        if (hipMemcpyAsync(t->report, t->report_dev, sizeof(Ex4dTrainerReport), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess
            || hipEventRecord(t->report_ev, (hipStream_t)stream) != hipSuccess)
            return tfail(EX4D_ERR_HIP, "report copy failed: %s", hipGetErrorString(hipGetLastError()));
        t->report_pending = true;
        t->report_census = census;
    }
    return EX4D_OK;
}

int ex4d_trainer_step_ex(Ex4dTrainer *t, double timestamp, const float *viewmatrix, const float *projmatrix, const float *campos,
                         const float *background, const float *gt_image, void *stream, int32_t *num_rendered,
                         const Ex4dTrainerStepOptions *opt)
{
    return step_body(t, timestamp, viewmatrix, projmatrix, campos, background, GroundTruth{ gt_image, nullptr, 0, nullptr }, stream, num_rendered, opt);
}

int ex4d_trainer_step_u8(Ex4dTrainer *t, double timestamp, const float *viewmatrix, const float *projmatrix, const float *campos,
                         const float *background, const uint8_t *gt_u8, int32_t pixel_stride, const float *lut, void *stream,
                         int32_t *num_rendered, const Ex4dTrainerStepOptions *opt)
{
    return step_body(t, timestamp, viewmatrix, projmatrix, campos, background, GroundTruth{ nullptr, gt_u8, pixel_stride, lut }, stream, num_rendered, opt);
}

int ex4d_trainer_report(Ex4dTrainer *t, Ex4dTrainerReport *out)
{
    t_err[0] = 0;
    if (!t || !out) return tfail(EX4D_ERR_ARG, "null argument");
    if (!t->report_pending) return tfail(EX4D_ERR_ARG, "no step with options has run: nothing to report");
    if (hipEventSynchronize(t->report_ev) != hipSuccess) return tfail(EX4D_ERR_HIP, "event wait failed");
    *out = *t->report;
    if (!t->report_census) out->nan_static = out->nan_dynamic = 0;      // flags of an earlier census are not this step's
    out->reserved = 0;
    return EX4D_OK;
}

int ex4d_trainer_set_async(Ex4dTrainer *t, int32_t on)
{
    t_err[0] = 0;
    if (!t) return tfail(EX4D_ERR_ARG, "null argument");
    if (on && !t->status) {
        if (hipHostMalloc((void **)&t->status, sizeof(Ex4dFrameStatus), hipHostMallocDefault) != hipSuccess) { t->status = nullptr; return tfail(EX4D_ERR_HIP, "pinned status allocation failed"); }
        if (hipEventCreateWithFlags(&t->status_ev, hipEventDisableTiming) != hipSuccess) { t->status_ev = nullptr; return tfail(EX4D_ERR_HIP, "event creation failed"); }
    }
    t->async = on != 0;
    return EX4D_OK;
}

int64_t ex4d_trainer_replays(const Ex4dTrainer *t) { return t ? t->replays : 0; }

int ex4d_trainer_set_interp(Ex4dTrainer *t, int32_t interp)
{
    t_err[0] = 0;
    if (!t) return tfail(EX4D_ERR_ARG, "null argument");
    if (!ex4d_known_interp(interp)) return tfail(EX4D_ERR_ARG, EX4D_UNKNOWN_INTERP_FMT, (int)interp);
    if (t->frames > 0) return tfail(EX4D_ERR_ARG, "the interpolator is fixed once a step has run: set it right after ex4d_trainer_create");
    t->interp = interp;
    // the position window of the sliced keyframe gradient (the buffer was taken for the cube's, the widest)
    t->grad_numel[XYZ_MOTION] = (int64_t)t->cfg.Nd * ex4d_key_window(interp, 0).count * 3;
    return EX4D_OK;
}

int ex4d_trainer_set_regularizers(Ex4dTrainer *t, double static_reg, double motion_reg, double rot_reg)
{
    t_err[0] = 0;
    if (!t) return tfail(EX4D_ERR_ARG, "null argument");
    if (!(static_reg >= 0.0) || !(motion_reg >= 0.0) || !(rot_reg >= 0.0)) return tfail(EX4D_ERR_ARG, "regulariser weight negative or NaN");
    const bool on = static_reg != 0.0 || motion_reg != 0.0 || rot_reg != 0.0;
    if (on && !t->cfg.optimizer) return tfail(EX4D_ERR_ARG, "regularisers join the gradients inside the optimizer step: the trainer was built without one");
    if (on && t->cfg.Nd > 0 && (ex4d_radam_sliced_reg_rows(t->cfg.K, 3) == 0 || ex4d_radam_sliced_reg_rows(t->cfg.K, 4) == 0))
        return tfail(EX4D_ERR_ARG, "K = %d keyframes do not fit the regularised sliced optimizer step", t->cfg.K);
    t->reg_w[0] = static_reg; t->reg_w[1] = t->cfg.Nd > 0 ? motion_reg : 0.0; t->reg_w[2] = t->cfg.Nd > 0 ? rot_reg : 0.0;
    return EX4D_OK;
}

int ex4d_trainer_set_lr(Ex4dTrainer *t, const double *lr15)
{
    t_err[0] = 0;
    if (!t || !lr15) return tfail(EX4D_ERR_ARG, "null argument");
    for (int i = 0; i < EX4D_TRAINER_PARAMS; i++) {
        if (!(lr15[i] >= 0.0)) return tfail(EX4D_ERR_ARG, "learning rate %d is negative or NaN", i);
        t->cfg.lr[i] = lr15[i];
    }
    return EX4D_OK;
}

int ex4d_trainer_set_sh_degree(Ex4dTrainer *t, int32_t degree)
{
    t_err[0] = 0;
    if (!t || degree < 0 || degree > 3) return tfail(EX4D_ERR_ARG, "SH degree outside [0, 3]");
    t->cfg.sh_degree = degree;
    return EX4D_OK;
}

const void *ex4d_trainer_output(const Ex4dTrainer *t, int32_t what)
{
    if (!t) return nullptr;
    switch (what) {
    case 0: return t->loss;
    case 1: return t->color;
    case 2: return t->radii;
    case 3: return t->g_means2D;
    case 4: return t->depth;
    case 5: return t->acc;
    case 6: return t->reg_out;
    case 7: return t->g_dir;
    case 8: return t->hook;
    default: return nullptr;
    }
}

const float *ex4d_trainer_grad(const Ex4dTrainer *t, int32_t i, int32_t *slices4)
{
    if (!t || i < 0 || i >= EX4D_TRAINER_PARAMS) return nullptr;
    if (slices4) memcpy(slices4, t->slices, sizeof(t->slices));
    return t->grad[i];
}

int ex4d_trainer_read(const Ex4dTrainer *t, int32_t what, void *dst, size_t bytes, void *stream)
{
    t_err[0] = 0;
    if (!t || !dst) return tfail(EX4D_ERR_ARG, "null argument");
    const void *src = nullptr;
    size_t have = 0;
    const size_t P = (size_t)t->P, HW = t->HW;
    if (what >= 100 && what < 100 + EX4D_TRAINER_PARAMS) { src = t->grad[what - 100]; have = (size_t)t->grad_numel[what - 100] * sizeof(float); }
    else if (what >= 200 && what < 200 + EX4D_TRAINER_PARAMS) { src = t->m[what - 200]; have = t->cfg.optimizer ? (size_t)t->numel[what - 200] * sizeof(float) : 0; }
    else if (what >= 300 && what < 300 + EX4D_TRAINER_PARAMS) { src = t->v[what - 300]; have = t->cfg.optimizer ? (size_t)t->numel[what - 300] * sizeof(float) : 0; }
    else {
        src = ex4d_trainer_output(t, what);
        const size_t sizes[9] = { sizeof(float), 3 * HW * sizeof(float), P * sizeof(int32_t), 3 * P * sizeof(float), HW * sizeof(float), HW * sizeof(float),
                                  4 * sizeof(float), 3 * P * sizeof(float), 3 * HW * sizeof(float) };
        if (what >= 0 && what < 9) have = sizes[what];
    }
    if (bytes > have || (bytes > 0 && !src)) return tfail(EX4D_ERR_ARG, "buffer %d holds %zu bytes, %zu requested", what, have, bytes);
    if (bytes && hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
        return tfail(EX4D_ERR_HIP, "device copy failed: %s", hipGetErrorString(hipGetLastError()));
    return EX4D_OK;
}

int ex4d_trainer_write(Ex4dTrainer *t, int32_t what, const void *src, size_t bytes, void *stream)
{
    t_err[0] = 0;
    if (!t || !src) return tfail(EX4D_ERR_ARG, "null argument");
    void *dst = nullptr;
    size_t have = 0;
    if (what >= 200 && what < 200 + EX4D_TRAINER_PARAMS) { dst = t->m[what - 200]; have = (size_t)t->numel[what - 200] * sizeof(float); }
    else if (what >= 300 && what < 300 + EX4D_TRAINER_PARAMS) { dst = t->v[what - 300]; have = (size_t)t->numel[what - 300] * sizeof(float); }
    else return tfail(EX4D_ERR_ARG, "buffer %d cannot be written: only the optimizer state (200 + i, 300 + i) can", what);
    if (!t->cfg.optimizer) return tfail(EX4D_ERR_ARG, "the trainer was built without an optimizer: it has no state to write");
    if (bytes > have || (bytes > 0 && !dst)) return tfail(EX4D_ERR_ARG, "buffer %d holds %zu bytes, %zu given", what, have, bytes);
    if (bytes && hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
        return tfail(EX4D_ERR_HIP, "device copy failed: %s", hipGetErrorString(hipGetLastError()));
    return EX4D_OK;
}

int ex4d_trainer_get_step(const Ex4dTrainer *t, int64_t *step)
{
    t_err[0] = 0;
    if (!t || !step) return tfail(EX4D_ERR_ARG, "null argument");
    *step = t->step;
    return EX4D_OK;
}

int ex4d_trainer_set_step(Ex4dTrainer *t, int64_t step)
{
    t_err[0] = 0;
    if (!t || step < 0) return tfail(EX4D_ERR_ARG, "null trainer or negative step count");
    t->step = step;
    return EX4D_OK;
}

size_t ex4d_trainer_bytes(const Ex4dTrainer *t) { return t ? t->bytes : 0; }

}  // extern "C"
