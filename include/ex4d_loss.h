/*
 * ex4d_loss.h -- C ABI of the fused L1 + SSIM training loss, forward and backward.
 *
 * Replaces, as one forward and one backward call, what train.py:144-151 of the reference builds out of
 * utils/loss_utils.py:22-25 (l1_loss) and :47-81 (ssim/_ssim: five depthwise 11x11 Gaussian-window conv2d, sigma 1.5,
 * zero padding 5) plus its autograd graph:
 *     loss        = (1 - lambda) * mean|img - gt| + lambda * (1 - mean(ssim_map))
 *     l1_errors   = mean_c |img - gt|          [H,W]      (train.py:149, hook tensor of the flow channel)
 *     ssim_errors = mean_c ssim_map            [H,W]      (train.py:150)
 * All pointers are device pointers (float32, [C,H,W] contiguous) except `window`, a HOST array of the 11 normalised 1-D
 * Gaussian taps (loss_utils.py:32-34; the 2-D window is their outer product, :38-39).  `stream` is a hipStream_t.
 */
#ifndef EX4D_LOSS_H_INCLUDED
#define EX4D_LOSS_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EX4D_SSIM_WINDOW 11

const char *ex4d_loss_last_error(void);

/* floats of scratch the forward needs besides its outputs (per-workgroup partial sums) */
size_t ex4d_l1_ssim_scratch_floats(int32_t H, int32_t W);

/* Forward.  loss[1]; l1_errors / ssim_errors [H,W] (either may be NULL); dmaps[3][C][H][W] receives the three per-pixel
 * partial derivatives dS/dmu1, dS/dE[x^2], dS/dE[xy] of the SSIM map that the backward convolves (kept for backward). */
int ex4d_l1_ssim_forward(int32_t C, int32_t H, int32_t W, const float *img, const float *gt, float lambda_dssim,
                         const float *window /* host [11] */, float *loss, float *l1_errors, float *ssim_errors,
                         float *dmaps, float *scratch, void *stream);

/* Backward: grad_img[C,H,W] = grad_loss[0] * dloss/dimg (fully written). */
int ex4d_l1_ssim_backward(int32_t C, int32_t H, int32_t W, const float *img, const float *gt, float lambda_dssim,
                          const float *window /* host [11] */, const float *dmaps, const float *grad_loss /* device [1] */,
                          float *grad_img, void *stream);

/* The same two calls on ground truth as an image decoder leaves it: gt is DEVICE uint8 [H,W,S] (pixel_stride S = 3 or 4 bytes per
 * pixel, any byte alignment), channel c < 3 of pixel (y,x) is lut[gt[(y*W + x)*S + c]]; a fourth byte per pixel is never read (the
 * reference takes [:3], scene/__init__.py:201).  lut: HOST [256] floats read during the call, as window is -- the reference's
 * (u / 255.0 / im_scale).clamp(0, 1) or any other table; NULL = (float)u / 255.0f.  C = 3; outputs, dmaps and
 * ex4d_l1_ssim_scratch_floats exactly as above, bit for bit what the float calls give on the looked-up [3,H,W] image.  No allocation,
 * no copy, no synchronisation: the table travels in the kernel arguments, so the calls can be captured into a graph (which then holds
 * the table by value). */
int ex4d_l1_ssim_forward_u8(int32_t H, int32_t W, const float *img, const uint8_t *gt, int32_t pixel_stride,
                            const float *lut /* host [256] or NULL */, float lambda_dssim, const float *window /* host [11] */,
                            float *loss, float *l1_errors, float *ssim_errors, float *dmaps, float *scratch, void *stream);
int ex4d_l1_ssim_backward_u8(int32_t H, int32_t W, const float *img, const uint8_t *gt, int32_t pixel_stride,
                             const float *lut /* host [256] or NULL */, float lambda_dssim, const float *window /* host [11] */,
                             const float *dmaps, const float *grad_loss /* device [1] */, float *grad_img, void *stream);

/* SCORING a rendered view (render.py:64-88, train.py:313-362 of the reference): one pass over a float32 [3,H,W] image and its ground
 * truth -- float32 [3,H,W], or uint8 [H,W,S] through lut exactly as above -- gives the L1, the MSE, the PSNR of
 * utils/image_utils.py:17-19 and the mean of the SSIM map of loss_utils.py:47-81, and optionally the image as 8-bit pixels.  No
 * derivative maps, no error maps.  row: DEVICE double[8], all eight written on every call:
 *     row[0] mean|x - y|   row[1] mean (x - y)^2   row[2] 20 log10(1 / sqrt(row[1])) (+inf at MSE 0, as torch gives)
 *     row[3] mean of the SSIM map   row[4] number of non-finite image values (exact)   row[5..7] 0
 * where x is the image value AS SCORED: with EX4D_METRICS_CLAMP, clamp(v, 0, 1) (train.py:342; NaN stays NaN, +-inf become 1 / 0 and
 * are then no longer counted in row[4]).  The sums are float per workgroup and double across workgroups.
 * out_u8: DEVICE uint8 [H,W,3] (any byte alignment) or NULL.  Default bytes: (uint8)clamp(x * 255 + 0.5, 0, 255), the product and the
 * sum rounded separately as torch's mul and add are (torchvision's save_image, render.py:75); with EX4D_METRICS_QUANT_TRUNC:
 * (uint8)(clamp(x, 0, 1) * 255) (train.py:101).  +inf gives 255, -inf gives 0.  A NaN gives 0: torch leaves that conversion
 * unspecified, 0 is this library's choice.
 * scratch: ex4d_frame_metrics_scratch_floats(H, W) floats.  window and lut are HOST arrays read during the call.  No allocation, no
 * copy, no synchronisation: the calls can be captured into a graph.  C is 3 only: render.py scores RGB. */
#define EX4D_METRICS_CLAMP 1
#define EX4D_METRICS_QUANT_TRUNC 2
size_t ex4d_frame_metrics_scratch_floats(int32_t H, int32_t W);
int ex4d_frame_metrics(int32_t H, int32_t W, const float *img, const float *gt, const float *window /* host [11] */,
                       int32_t flags, uint8_t *out_u8 /* [H,W,3] or NULL */, double *row /* device [8] */, float *scratch,
                       void *stream);
int ex4d_frame_metrics_u8(int32_t H, int32_t W, const float *img, const uint8_t *gt, int32_t pixel_stride,
                          const float *lut /* host [256] or NULL */, const float *window /* host [11] */, int32_t flags,
                          uint8_t *out_u8 /* [H,W,3] or NULL */, double *row /* device [8] */, float *scratch, void *stream);

/* RESIZING a decoded frame to the training resolution, bit for bit as PIL's 8-bit Image.resize does (the reference's
 * PILtoTorch(image, resolution), utils/general_utils.py:23-24: resample=2, bilinear with its support scaled by the reduction): two
 * fixed-point passes, horizontal then vertical, with the intermediate image rounded to bytes between them.  Per axis of input size
 * `in` and output size `out`, filter f of support s, in double precision with no contracted multiply-add:
 *     scale = in / out;  fs = max(scale, 1);  sup = s * fs;  ksize = (int)ceil(sup) * 2 + 1;  ss = 1 / fs
 *     per output element xx:  center = (xx + 0.5) * scale
 *         xmin = max((int)(center - sup + 0.5), 0);  xmax = min((int)(center + sup + 0.5), in);  n = xmax - xmin
 *         w[x] = f((x + xmin - center + 0.5) * ss), x < n;  ww = w[0] + w[1] + ...;  w[x] /= ww where ww != 0
 *         k[x] = (int)(w[x] * 2^22 + 0.5) for w[x] >= 0, else (int)(w[x] * 2^22 - 0.5)
 * and a pass computes acc = 2^21 + sum_{x<n} src[xmin + x] * k[x] in int32 and writes clamp(acc >> 22, 0, 255).  A pass whose input
 * size equals its output size is skipped; if both are, the frame is copied.
 * filter: PIL's resample numbers.  BILINEAR f(x) = 1 - |x| on |x| < 1, s = 1;  BOX f = 1 on (-0.5, 0.5], s = 0.5;  BICUBIC a = -0.5,
 * s = 2.  (Lanczos and Hamming go through libm's sin / cos: not offered.)
 * ex4d_resize_u8_table is HOST code: it fills ex4d_resize_u8_table_words(in, out, filter) words of one axis -- ksize, then per output
 * element xmin, n and ksize coefficients (the unused ones zero); the caller uploads them once per (in, out, filter).  The words count
 * is 0 for a refused size or filter.
 * ex4d_resize_u8: src DEVICE uint8 [H_in,W_in,3], dst DEVICE uint8 [H_out,W_out,3], tightly packed, at any byte alignment; table_x
 * (W_in -> W_out) and table_y (H_in -> H_out) DEVICE tables, either may be NULL where its pass is skipped; scratch:
 * ex4d_resize_u8_scratch_bytes bytes (the [H_in,W_out,3] intermediate; 0 where a pass is skipped), written before it is read.  No
 * byte outside src is read, none outside dst and the scratch is written, every byte of dst is written.  Sizes 1 .. EX4D_FRAME_MAX_SIZE
 * per axis in any ratio.  pixel_stride must be 3: PIL resizes four-byte (RGBA) pixels on premultiplied colour, which gives other
 * colour bytes than the RGB resize, and that is not reproduced here.  No allocation, no host-device copy, no synchronisation: the
 * call can be captured into a graph.
 * Tiling: the horizontal pass gives a workgroup EX4D_RESIZE_H_ROWS rows of EX4D_RESIZE_H_PIXELS output pixels, one lane per pixel; the
 * vertical pass gives it EX4D_RESIZE_V_ROWS output rows of EX4D_RESIZE_V_BYTES flat bytes (3 W_out per row), four bytes per lane. */
#define EX4D_FILTER_BILINEAR 2
#define EX4D_FILTER_BICUBIC 3
#define EX4D_FILTER_BOX 4
#define EX4D_FRAME_MAX_SIZE 16384
#define EX4D_RESIZE_H_PIXELS 64
#define EX4D_RESIZE_H_ROWS 4
#define EX4D_RESIZE_V_BYTES 256
#define EX4D_RESIZE_V_ROWS 4
size_t ex4d_resize_u8_table_words(int32_t in, int32_t out, int32_t filter);
int ex4d_resize_u8_table(int32_t in, int32_t out, int32_t filter, int32_t *host_words);
size_t ex4d_resize_u8_scratch_bytes(int32_t H_in, int32_t W_in, int32_t H_out, int32_t W_out);
int ex4d_resize_u8(int32_t H_in, int32_t W_in, int32_t H_out, int32_t W_out, int32_t pixel_stride, const uint8_t *src, uint8_t *dst,
                   const int32_t *table_x /* device */, const int32_t *table_y /* device */, uint8_t *scratch, void *stream);

/* FLOW: supervising the rendered motion (render(..., flow_to=t1): the rasterizer's `opticalflow` output in pixels) with the ground
 * truth the reference's data layer carries (utils/general_utils.py:39-53 read_opticalflow / decode_flow, scene/cameras.py:85,102
 * opticalflow_path): a 16-bit three-channel image, decoded on load.
 *   flow  DEVICE float32 [3,H,W]: u, v, depth change.  The third plane is never read.
 *   gt    DEVICE uint16 [H,W,S], pixel_stride S = 3 or 4 words per pixel, at any 2-byte alignment (hence void *); word 0 = u, word 1 = v,
 *         word 2 = validity, as decode_flow indexes them; a fourth word is never read.
 *   acc   DEVICE float32 [H,W] (the rasterizer's accumulated alpha) or NULL: a per-pixel weight, a constant with no gradient.
 * Decode, the bits of the reference's float32 arithmetic (one rounding: the subtraction and the division are exact):
 *     g = (float)(code - 32768) / 256 * flow_scale,     m = code2 > 32768
 * flow_scale carries read_opticalflow's resolution[1] / rows; the encoded frame is at render resolution (cv2's INTER_AREA resize of
 * encoded flow is not offered).  Loss, this library's definition, float32 per pixel:
 *     r = (flow_u - g_u, flow_v - g_v)
 *     rho = |r_u| + |r_v|  (EX4D_FLOW_L1)   or   sqrt(r_u^2 + r_v^2 + eps^2)  (EX4D_FLOW_CHARBONNIER; eps finite and > 0)
 *     loss = sum m w rho / max(sum m, 1),   w = acc[p] or 1
 * Invalid pixels are selected out: nothing behind them, a NaN included, reaches a sum or a gradient.  A NaN in a VALID rendered pixel
 * propagates into the loss.
 * Forward: loss DEVICE float[1]; row DEVICE double[4], all four written on every call:
 *     row[0] the loss   row[1] number of valid pixels (exact)   row[2] mean end-point error sqrt(r_u^2 + r_v^2) over the valid pixels,
 *     unweighted, 0 when there are none   row[3] number of valid pixels whose rendered u or v is not finite (exact)
 * The sums are float per workgroup and double across workgroups, in a fixed order: equal inputs give equal bits.
 * scratch: ex4d_flow_loss_scratch_floats(H, W) floats (0 for a refused size).
 * Backward: grad_flow DEVICE [3,H,W], fully written: planes 0 and 1 grad_loss[0] * m w / max(count, 1) * d rho / d r -- sign(r) with
 * sign(0) = 0 for L1, r / rho for Charbonnier -- and exact zeros in plane 2, at every invalid pixel, and everywhere when no pixel is
 * valid.  row: the forward's row of the same inputs (its count is read on the device); grad_loss DEVICE float[1].
 * Refused before any launch, with a message: H or W <= 0, a stride other than 3 or 4, an unknown kind, Charbonnier with eps <= 0 or
 * not finite, a NULL required pointer.  No allocation, no copy, no synchronisation, no atomics: the calls can be captured into a graph.
 * Tiling: a lane owns EX4D_FLOW_PIXELS_PER_LANE consecutive pixels of the flat [H W] index, a workgroup has EX4D_FLOW_THREADS lanes, and
 * the one wave that adds the workgroups' partial sums takes EX4D_FLOW_FOLD of them per step. */
#define EX4D_FLOW_L1 0
#define EX4D_FLOW_CHARBONNIER 1
#define EX4D_FLOW_PIXELS_PER_LANE 4
#define EX4D_FLOW_THREADS 256
#define EX4D_FLOW_FOLD 64
size_t ex4d_flow_loss_scratch_floats(int32_t H, int32_t W);
int ex4d_flow_loss_forward(int32_t H, int32_t W, const float *flow, const void *gt, int32_t pixel_stride, float flow_scale,
                           const float *acc, int32_t kind, float eps, float *loss, double *row /* device [4] */, float *scratch,
                           void *stream);
int ex4d_flow_loss_backward(int32_t H, int32_t W, const float *flow, const void *gt, int32_t pixel_stride, float flow_scale,
                            const float *acc, int32_t kind, float eps, const double *row /* device [4] */,
                            const float *grad_loss /* device [1] */, float *grad_flow, void *stream);

/* DEPTH: supervising the rendered depth (the rasterizer's `depth` output, the alpha-normalised mean depth of CR/forward.cu:426-435) with
 * the ground truth the reference's data layer carries (scene/dataset_readers.py:45 depth_path; utils/general_utils.py:32-36 load_depth):
 * a 16-bit INVERSE-depth map, decoded on load.  Monocular inverse depth is known up to a scale and a shift, so the loss can fit both per
 * frame, on the device.
 *   depth DEVICE float32 [H,W].
 *   gt    DEVICE [H,W]: gt_type EX4D_DEPTH_GT_U16 = uint16 codes at any 2-byte alignment (hence void *), EX4D_DEPTH_GT_F32 = float32
 *         values (what load_depth returns after its host resize).  Raw value v = (float)code or the float itself; the ground truth is
 *         VALID where v is finite and v > 0 (code 0: no measurement).
 *   acc   DEVICE float32 [H,W] (the rasterizer's accumulated alpha) or NULL.  With acc: w = acc[p], and a pixel counts only where
 *         acc > 0 (a pixel nothing was composited into carries max_depth, not a depth).  Without: w = 1.  A constant with no gradient.
 * Per pixel, float32 (this file's kernels are compiled with -ffp-contract=off):
 *     g = v * code_scale            one rounding: code_scale 1 gives load_depth's values, 2^-16 the usual normalised inverse depth;
 *                                   equal values give equal bits in both ground-truth types
 *     m = valid and (acc == NULL or acc > 0)
 *     x = 1.0f / depth              IEEE division: the rendered inverse depth
 *     gh = s * g + o                a multiply, then an add
 *     r = x - gh;   rho = |r|  (EX4D_DEPTH_L1)   or   sqrt(r^2 + eps^2)  (EX4D_DEPTH_CHARBONNIER; eps finite and > 0)
 *     loss = sum m w rho / max(n, 1),   n = sum m
 * Pixels outside m are selected out: nothing behind them, a NaN included, reaches a sum or a gradient.  A non-finite or non-positive
 * depth INSIDE m propagates and is counted in row[5].
 * Alignment:
 *   EX4D_DEPTH_ALIGN_GIVEN  s = scale, o = offset: the per-image constants a COLMAP-scaled pipeline supplies.
 *   EX4D_DEPTH_ALIGN_FIT    the unweighted least-squares fit of gh to x over m, from five float64 sums n, Sg, Sx, Sgg, Sgx (products
 *                           formed in double, where a product of two floats is exact), added in a fixed order: per lane, per workgroup,
 *                           then across workgroups by one finishing wave.  det = n Sgg - Sg^2.  If n >= 2 and det > 1e-10 n Sgg:
 *                           s = (n Sgx - Sg Sx) / det, o = (Sx - s Sg) / n; otherwise s = 0, o = Sx / max(n, 1).  The relative
 *                           threshold makes a constant ground truth degenerate whatever the last bits of the sums are: a design
 *                           constant, not a measurement.  s and o are rounded to float32 once; those floats are what the loss pass
 *                           and the backward use.  scale and offset are ignored.
 * Forward: loss DEVICE float[1]; row DEVICE double[6], all six written on every call:
 *     row[0] the loss   row[1] n (exact)   row[2] s as used   row[3] o as used   row[4] sqrt(sum m r^2 / n), unweighted, 0 when n = 0
 *     row[5] number of m pixels whose depth is not finite or <= 0 (exact)
 * loss[0] is row[0] rounded once.  Every sum is double from the lane on.  scratch: ex4d_depth_loss_scratch_bytes(H, W) bytes (0 for a
 * refused size), 8-byte aligned.
 * Backward: grad_depth DEVICE [H,W], fully written: grad_loss[0] * m w / max(n, 1) * rho'(r) * (-x x), rho'(r) = sign(r) with
 * sign(0) = 0 for L1 and r / rho for Charbonnier.  THE FIT IS DETACHED: s, o and n are read from row, the forward's row of the same
 * inputs, as constants.  Exact zeros outside m, and everywhere when n = 0.  grad_loss DEVICE float[1].
 * Refused before any launch, with a message: H or W <= 0, an unknown kind, align or gt_type, Charbonnier with eps <= 0 or not finite,
 * code_scale not finite or <= 0, GIVEN with a non-finite scale or offset, a NULL required pointer, a scratch that is not 8-byte aligned.
 * No allocation, no copy, no synchronisation, no atomics: the calls can be captured into a graph.  Equal inputs give equal bits.
 * Launches: FIT forward four (moments, solve, loss, finish), GIVEN forward two (loss, finish), backward one.
 * Tiling: a lane owns EX4D_DEPTH_PIXELS_PER_LANE consecutive pixels of the flat [H W] index, a workgroup has EX4D_DEPTH_THREADS lanes, and
 * the one wave that adds the workgroups' partial sums takes EX4D_DEPTH_FOLD of them per step. */
#define EX4D_DEPTH_L1 0
#define EX4D_DEPTH_CHARBONNIER 1
#define EX4D_DEPTH_ALIGN_GIVEN 0
#define EX4D_DEPTH_ALIGN_FIT 1
#define EX4D_DEPTH_GT_U16 0
#define EX4D_DEPTH_GT_F32 1
#define EX4D_DEPTH_PIXELS_PER_LANE 4
#define EX4D_DEPTH_THREADS 256
#define EX4D_DEPTH_FOLD 64
size_t ex4d_depth_loss_scratch_bytes(int32_t H, int32_t W);
int ex4d_depth_loss_forward(int32_t H, int32_t W, const float *depth, const void *gt, int32_t gt_type, float code_scale,
                            const float *acc, int32_t align, float scale, float offset, int32_t kind, float eps, float *loss,
                            double *row /* device [6] */, void *scratch, void *stream);
int ex4d_depth_loss_backward(int32_t H, int32_t W, const float *depth, const void *gt, int32_t gt_type, float code_scale,
                             const float *acc, int32_t align, int32_t kind, float eps, const double *row /* device [6] */,
                             const float *grad_loss /* device [1] */, float *grad_depth, void *stream);

/* scikit-image's SSIM of a rendered view: the SKSSIM and SKSSIM2 entries of render.py:78-79,
 *     sk_ssim(render, gt, data_range=R, multichannel=True, channel_axis=0)   with R = 1 and R = 2,
 * as scikit-image 0.22 and later read that call (multichannel is ignored, channel_axis=0 holds; earlier releases fail on a [3,H,W]
 * array).  Per channel, over the (H-6) x (W-6) positions whose 7x7 window lies wholly inside the image: the uniform means ux, uy, uxx,
 * uyy, uxy, the sample covariances v = (49/48)(uxx - ux^2) ..., C1 = (0.01 R)^2, C2 = (0.03 R)^2,
 *     S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),
 * its mean per channel, and the mean of the three channels.  One pass gives both R.  row: DEVICE double[4], all four written on every
 * call:
 *     row[0] SKSSIM (R = 1)   row[1] SKSSIM2 (R = 2)   row[2] number of scored positions whose S(R = 1) is not finite (exact)   row[3] 0
 * img, gt, pixel_stride and lut exactly as in ex4d_frame_metrics / _u8.  flags: EX4D_METRICS_CLAMP only (scores clamp(img, 0, 1): a
 * NaN stays a NaN, +-inf become 1 / 0); any other bit is refused, as are H < 7 and W < 7 (scikit-image raises there).
 * scratch: ex4d_frame_skssim_scratch_floats(H, W) floats (0 for a refused size).  No allocation, no copy, no synchronisation: the calls
 * can be captured into a graph.  Equal image and ground truth score exactly 1. */
#define EX4D_SKSSIM_WINDOW 7
size_t ex4d_frame_skssim_scratch_floats(int32_t H, int32_t W);
int ex4d_frame_skssim(int32_t H, int32_t W, const float *img, const float *gt, int32_t flags, double *row /* device [4] */,
                      float *scratch, void *stream);
int ex4d_frame_skssim_u8(int32_t H, int32_t W, const float *img, const uint8_t *gt, int32_t pixel_stride,
                         const float *lut /* host [256] or NULL */, int32_t flags, double *row /* device [4] */, float *scratch,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif
