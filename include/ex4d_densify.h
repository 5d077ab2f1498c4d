/*
 * ex4d_densify.h -- C ABI of adaptive density control: per-iteration densification statistics, the clone / split / prune
 * classification with its compaction, and one multi-tensor gather that builds the new parameter, moment and statistic tensors.
 *
 * Restates scene/c_gaussian_model.py of the reference: add_densification_stats (:1095), mark_prune_stats (:1105),
 * add_l1_ssim_stats (:1119), densify_and_clone (:966), densify_and_split (:874), densification_postfix (:789-844),
 * densify_and_prune (:1019), prune_invisible (:1074), prune_small (:1087), prune_nan_points (:1229) and the optimizer-state
 * edits of _prune_optimizer / cat_tensors_to_optimizer (:700-787).  DESIGN.md section 7 lists the quirks kept.
 *
 * A model has two groups: static rows (g = 0) and dynamic rows (g = 1).  The statistics of a group are ONE float32 block
 * [EX4D_DENSIFY_STATS, n] (structure of arrays), row order EX4D_STAT_*.  The caller owns all memory; every call takes a
 * hipStream_t and never synchronises it.
 */
#ifndef EX4D_DENSIFY_H_INCLUDED
#define EX4D_DENSIFY_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EX4D_DENSIFY_STATS 9
enum {
    EX4D_STAT_GRAD_ACCUM = 0,    /* xyz_gradient_accum / motion_xyz_gradient_accum            init 0 */
    EX4D_STAT_DENOM = 1,         /* denom / motion_denom                                      init 0 */
    EX4D_STAT_ERROR_ACCUM = 2,   /* xyz_error_accum / motion_xyz_error_mean                   init 0 */
    EX4D_STAT_SSIM_ACCUM = 3,    /* xyz_ssim_error_accum / motion_xyz_ssim_error_accum        init 0 */
    EX4D_STAT_ERROR_DENOM = 4,   /* error_denom / motion_error_denom                          init 0 */
    EX4D_STAT_MAX_RADII = 5,     /* max_radii2D / motion_max_radii2D                          init 0 */
    EX4D_STAT_MIN_RADII = 6,     /* min_radii2D / motion_min_radii2D                          init 1000 */
    EX4D_STAT_ERROR_MIN = 7,     /* xyz_error_min / motion_xyz_error_min                      init 1000 */
    EX4D_STAT_ERROR_MIN_T = 8    /* xyz_error_min_timestamp / motion_xyz_error_min_timestamp  init -1 */
};

/* ---- per-iteration statistics: one thread per row, no atomics, no host synchronisation (graph-capturable) */
#define EX4D_DENSIFY_PRUNE_STATS 1     /* mark_prune_stats: filter e0 > 0, min_radii = min(min_radii, radii) */
#define EX4D_DENSIFY_GRAD_STATS 2      /* the `iteration < densify_until_iter` block: filter radii > 0, max_radii, add_densification_stats */
#define EX4D_DENSIFY_L1_STATS 4        /* ... and add_l1_ssim_stats inside that block */

/* stats_s [9, ns], stats_d [9, nd] (may be NULL when nd == 0); radii int32 [ns + nd]; vgrad = dL/dmeans2D float [ns + nd, 3];
 * egrad = the error channels (e0, e1, e2) float [ns + nd, 3], may be NULL when neither PRUNE_STATS nor L1_STATS is set. */
int ex4d_densify_stats(float *stats_s, int64_t ns, float *stats_d, int64_t nd, const int32_t *radii, const float *vgrad,
                       const float *egrad, float timestamp, int32_t flags, void *stream);

/* ---- merge of the ranks' statistics (multi-rank training): every rank accumulates ex4d_densify_stats into a PENDING block that
 * starts at the initial values above, the pending blocks are all-gathered, and this call folds them into the running TOTAL of one
 * group -- a left fold in rank order, rank 0 first, so every rank computes the same bits.  total [9, n] (read and written); pending
 * [world, 9, n] contiguous, block w from rank w; own_pending [9, n] or NULL: the caller's own pending block, reset to the initial
 * values by the same launch.  Per element, with t of the total and d of a rank:
 *     GRAD_ACCUM, DENOM, ERROR_ACCUM, SSIM_ACCUM, ERROR_DENOM    t = t + d                  (float32 add)
 *     MAX_RADII                                                  t = d > t ? d : t
 *     MIN_RADII                                                  t = d < t ? d : t
 *     ERROR_MIN / ERROR_MIN_T                                    if (t_min > d_min) { t_ts = d_ts; t_min = d_min; }
 * The last comparison is the strict one of ex4d_densify_stats: on a tie the lower rank keeps its timestamp, a NaN minimum is never
 * taken and a NaN total never replaced.  A pending block at the initial values leaves the total unchanged bit for bit (a sum row
 * holding -0.0 excepted: -0.0 + 0 is +0.0; sums that start at +0 never reach -0.0).  world == 0 or n == 0: valid, nothing is done
 * (own_pending is not written).  Refused before any HIP call, with "densify_stats_merge: negative rank count or size", "...: null or
 * misaligned block" (float alignment is all that is asked) or "...: the total, the pending blocks and the own block must not overlap".
 * One launch, no atomics, no host synchronisation (graph-capturable). */
int ex4d_densify_stats_merge(float *total, const float *pending, int32_t world, int64_t n, float *own_pending, void *stream);

/* ---- the gate of prune_nan_points (:1230, :1234: isnan().any() per group) without a read-back: flags2[0] = any(isnan(a[0 .. n_a))),
 * flags2[1] likewise for b; either array may be empty (n = 0, pointer then unused, may be NULL).  a and b need only float alignment.
 * flags2 (device int32[2]) is fully written: cleared by a kernel of the library, then one launch streams both arrays.  No atomics, no
 * host synchronisation (graph-capturable). */
int ex4d_nan_any(const float *a, int64_t n_a, const float *b, int64_t n_b, int32_t *flags2, void *stream);

/* ---- classification + compaction of one group */
enum { EX4D_PLAN_DENSIFY = 0, EX4D_PLAN_PRUNE_INVISIBLE = 1, EX4D_PLAN_PRUNE_SMALL = 2, EX4D_PLAN_PRUNE_NAN = 3 };

/* counts[] written by ex4d_densify_plan (device int32 [EX4D_PLAN_COUNTS]) */
enum {
    EX4D_CNT_KEEP = 0,           /* surviving original rows */
    EX4D_CNT_CLONE_SEL = 1,      /* rows selected for clone (= clone jitter draws) */
    EX4D_CNT_KEEP_CLONE = 2,     /* surviving clones */
    EX4D_CNT_SPLIT_SEL = 3,      /* original rows selected for split */
    EX4D_CNT_SPLIT_SEL_CLONE = 4,/* clones selected for split (only through the max_screen_size terms) */
    EX4D_CNT_KEEP_CHILD = 5,     /* surviving children per copy, of split originals */
    EX4D_CNT_KEEP_CHILD_CLONE = 6,/* ... of split clones */
    EX4D_CNT_ROWS = 7            /* rows after the call: KEEP + KEEP_CLONE + 2 (KEEP_CHILD + KEEP_CHILD_CLONE) */
};
#define EX4D_PLAN_COUNTS 8
#define EX4D_PLAN_MAP_INTS 8     /* per source row: dst_orig, dst_clone, dst_child (copy 0, of the row), dst_child_of_clone (copy 0),
                                    clone draw, split draw, split draw of the clone, unused; -1 = none */

typedef struct Ex4dDensifyPlanGroup {
    int64_t n;                   /* rows of the group (0: the call does nothing for it) */
    const float *stats;          /* device [9, n] */
    const float *scaling;        /* device [n, 3]: log scales (DENSIFY) */
    const float *opacity;        /* device [n]: opacity logits (DENSIFY) */
    const float *xyz;            /* device [n, xyz_width] (PRUNE_NAN: any NaN in the row prunes it) */
    int32_t xyz_width;
    int32_t use_screen;          /* max_screen_size (static) / max_dynamic_screen_size (dynamic) was given */
    float grad_thr;              /* max_grad / max_dgrad */
    float dense_scale;           /* percent_dense * extent (float32, as torch compares) */
    float big_scale;             /* 0.1 * extent */
    float screen_size;
    float min_opacity;
    float l1_thres;
    float max_ssim;
    int32_t reserved;
    int32_t *map;                /* device [n, EX4D_PLAN_MAP_INTS] (written) */
    int32_t *counts;             /* device [EX4D_PLAN_COUNTS] (written) */
    void *scratch;               /* device, ex4d_densify_scratch_bytes(n) */
} Ex4dDensifyPlanGroup;

size_t ex4d_densify_scratch_bytes(int64_t n);
int ex4d_densify_plan(int32_t mode, const Ex4dDensifyPlanGroup *group, void *stream);

/* ---- the multi-tensor gather.  For every source row with a map entry >= 0 the kernel writes that destination row; what a
 * new row (clone / child) holds is the descriptor's rule.  A surviving original row is always a copy, except for the reset
 * statistic rows of EX4D_RULE_STATS. */
enum {
    EX4D_RULE_COPY = 0,          /* every destination copies the source row (parameters, and every tensor of a prune) */
    EX4D_RULE_ZERO_NEW = 1,      /* new rows 0 (exp_avg, exp_avg_sq) */
    EX4D_RULE_CONST_NEW = 2,     /* new rows = value (_opacity_duration_var: 2) */
    EX4D_RULE_CHILD_SCALING = 3, /* children log(exp(s) / (0.8 N)) */
    EX4D_RULE_CHILD_XYZ = 4,     /* children R(normalize(q_k)) (sigma exp(s) * z) + x_k per keyframe k; aux0 = rotations [n, K, 4], aux1 = log scales [n, 3] */
    EX4D_RULE_CENTER = 5,        /* clones and children: duration centres jittered by len * z and clamped (children of clones: twice) */
    EX4D_RULE_STATS = 6          /* a [9, n] statistics block after densification_postfix */
};

typedef struct Ex4dDensifyTensor {
    const float *src;
    float *dst;
    int64_t rows;                /* source rows */
    int64_t dst_rows;            /* destination rows (plane stride of a statistics block) */
    int32_t width;               /* floats per row */
    int32_t planes;              /* 1, or EX4D_DENSIFY_STATS for a statistics block */
    int32_t rule;
    int32_t group;               /* 0 static, 1 dynamic: which Ex4dDensifyApplyGroup */
    const float *aux0, *aux1;
    float value;                 /* EX4D_RULE_CONST_NEW; EX4D_RULE_CHILD_XYZ: sigma (1 static, 2 dynamic) */
    int32_t reserved;
} Ex4dDensifyTensor;

typedef struct Ex4dDensifyApplyGroup {
    const int32_t *map;          /* device [rows, EX4D_PLAN_MAP_INTS] from ex4d_densify_plan */
    int64_t child_stride;        /* KEEP_CHILD + KEEP_CHILD_CLONE: destination distance of copy 1 from copy 0 */
    int64_t n_split;             /* SPLIT_SEL + SPLIT_SEL_CLONE: draw distance of copy 1 from copy 0 */
    const float *split_z;        /* device [2 n_split, 3] standard normal: split samples, copy-major */
    const float *split_c1, *split_c0;   /* device [2 n_split]: children's centre jitter (c1 drawn first) */
    const float *clone_c1, *clone_c0;   /* device [CLONE_SEL]: clones' centre jitter */
    float min_len;               /* 2 / interval */
    float center_lo, center_hi;  /* (time_shift + 1) / interval, (time_shift + duration - 1) / interval */
    float split_div;             /* 0.8 N */
} Ex4dDensifyApplyGroup;

#define EX4D_DENSIFY_MAX_TENSORS 24
int ex4d_densify_apply(const Ex4dDensifyTensor *tensors, int32_t count, const Ex4dDensifyApplyGroup *groups, void *stream);

const char *ex4d_densify_last_error(void);

/* ---- growth of the dynamic set: extract_dynamic_points_from_static (:1147), expand_duration (:1243), adjust_temp_opa (:1330).
 * Errors of these calls are read with ex4d_densify_last_error as well. */

/* score[i] = |disp_i| / (|xyz_i - cam|^2 + 1e-6) for a visible row, -1 for an invisible one (float32, the reference's op order).
 * xyz, disp float [n, 3]; vis uint8 [n] (0 = invisible); cam = 3 device floats; score float [n] (written). */
int ex4d_growth_scores(const float *xyz, const float *disp, const uint8_t *vis, const float *cam, int64_t n, float *score, void *stream);

/* The threshold of torch.quantile(u, q), linear interpolation, over u = s / (max s + 1e-6), s = the entries of `score` without a
 * sign bit (a NaN counts as present and makes the threshold NaN): a radix select of the two order statistics, no sort.
 * result (device, written): [EX4D_SELECT_THETA] the threshold, [EX4D_SELECT_MAX] max s, [EX4D_SELECT_COUNT] the number of present
 * entries as int32 bits, [3] unused.  No present entry: threshold NaN, max 0, count 0. */
enum { EX4D_SELECT_THETA = 0, EX4D_SELECT_MAX = 1, EX4D_SELECT_COUNT = 2 };
#define EX4D_SELECT_WORDS 4
size_t ex4d_growth_select_scratch_bytes(void);
int ex4d_growth_select(const float *score, int64_t n, float q, float *result, void *scratch, void *stream);

/* Classification of the static rows and its compaction.  Selected: score present and (u > theta or |disp| > motion_abs) and
 * |disp| > min_abs and error-min timestamp >= 0.  map is written in EX4D_PLAN_MAP_INTS layout (a selected row has no destination)
 * and counts in EX4D_PLAN_COUNTS layout, so ex4d_densify_apply prunes the static tensors with them; selected[j] is the source row of
 * the j-th selected row (ascending), counts_out = {selected, kept}. */
typedef struct Ex4dGrowthClassify {
    int64_t n;                   /* static rows */
    const float *score;          /* device [n] from ex4d_growth_scores */
    const float *result;         /* device [EX4D_SELECT_WORDS] from ex4d_growth_select */
    const float *disp;           /* device [n, 3] */
    const float *stats;          /* device [9, n]: the static statistics block */
    float motion_abs;            /* motion_thres * extent */
    float min_abs;               /* min_motion_thres * extent */
    int32_t *map;                /* device [n, EX4D_PLAN_MAP_INTS] (written) */
    int32_t *counts;             /* device [EX4D_PLAN_COUNTS] (written) */
    int32_t *selected;           /* device [n] (the first counts_out[0] entries written) */
    int32_t *counts_out;         /* device [2] (written) */
    void *scratch;               /* device, ex4d_densify_scratch_bytes(n) */
} Ex4dGrowthClassify;

int ex4d_growth_classify(const Ex4dGrowthClassify *args, void *stream);

/* The dynamic append: every destination tensor is the old dynamic rows followed by one new row per selected static row. */
enum {
    EX4D_GROW_COPY = 0,          /* new row = row of src0 (width floats): features, scaling, opacity */
    EX4D_GROW_ZERO = 1,          /* new row = 0 (moments) */
    EX4D_GROW_XYZ = 2,           /* width 3 K: bilinear resize of xyz - disp interval / max_dur and xyz + disp (1 + interval / max_dur) to K samples; src0 = xyz, src1 = disp */
    EX4D_GROW_ROTATION = 3,      /* width 4 K: the row of src0 [n, 4] repeated K times */
    EX4D_GROW_CENTER = 4,        /* width 2: the duration centres from the static error-min timestamp */
    EX4D_GROW_VAR = 5,           /* width 2: (t + time_pad, max_dur - t + time_pad) */
    EX4D_GROW_STATS = 6          /* a [9, rows] block: rows GRAD_ACCUM .. MIN_RADII reset for every row, ERROR_MIN / ERROR_MIN_T kept for old rows, 1000 / -1 for new ones */
};

typedef struct Ex4dGrowthTensor {
    const float *old;            /* device [old_rows, width] ([9, old_rows] for EX4D_GROW_STATS); may be NULL when old_rows == 0 */
    float *dst;                  /* device [old_rows + n_new, width] (written) */
    const float *src0, *src1;    /* static sources of the rule */
    int64_t old_rows;
    int32_t width;
    int32_t rule;
} Ex4dGrowthTensor;

typedef struct Ex4dGrowthAppend {
    const int32_t *selected;     /* device [n_new] from ex4d_growth_classify */
    int64_t n_new;
    int64_t n_static;            /* rows of the static tensors (plane stride of stats) */
    const float *stats;          /* device [9, n_static] */
    int32_t K;                   /* keyframes of the new rows */
    float interval, max_dur;
    float b_scale;               /* 1 + interval / max_dur */
    float time_shift, time_pad;
    float center_lo, center_hi;  /* (time_shift + 1) / interval, (time_shift + max_dur - 1) / interval */
} Ex4dGrowthAppend;

#define EX4D_GROWTH_MAX_TENSORS 28
int ex4d_growth_append(const Ex4dGrowthTensor *tensors, int32_t count, const Ex4dGrowthAppend *args, void *stream);

/* expand_duration: dst [rows, K2, C] = the K keyframes of src [rows, K, C] followed by K2 - K extrapolated ones,
 * dst[K - 1 + j] = j d + src[K - 1], d = the mean over a = 0 .. avg - 1 of src[K - avg + a] - src[K - avg - 1] (summed in
 * ascending a).  1 <= avg < K < K2. */
int ex4d_growth_extrapolate(const float *src, float *dst, int64_t rows, int32_t K, int32_t K2, int32_t C, int32_t avg, void *stream);

/* expand_duration's opacity edits.  center / var [rows, 2]: var_out[:, 1] = 1 where either centre + shift > late, else var[:, 1];
 * var_out[:, 0] = var[:, 0]; center_out = min(center, center_max). */
int ex4d_growth_expand_opacity(const float *center, const float *var, float *center_out, float *var_out, int64_t rows, float shift,
                               float late, float center_max, void *stream);

/* adjust_temp_opa: centres clamped to [lo, hi]; var[:, 1] = max(var, 1) 2 where either centre > hi, var[:, 0] likewise where either
 * centre < lo; then 0.5 wherever the OLD var is < 0.5. */
int ex4d_growth_adjust_opacity(const float *center, const float *var, float *center_out, float *var_out, int64_t rows, float lo, float hi,
                               void *stream);

#ifdef __cplusplus
}
#endif
#endif
