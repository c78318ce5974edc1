/*
 * rain_loss.h — C ABI of the fused training loss:
 *   loss = (1 - lambda) * mean|img - gt| + lambda * (1 - SSIM(img, gt))
 * with the reference's SSIM (utils/loss_utils.py:22-53: 11x11 Gaussian window, sigma 1.5, zero
 * padding, C1 = 0.01^2, C2 = 0.03^2) and L1 (loss_utils.py:6-7), as used by train.py:113-114.
 *
 * Forward writes the scalar loss and three per-pixel maps (dS/dmu1, dS/dE[x^2], dS/dE[xy], already
 * scaled by -lambda/(C*H*W)) that the backward blurs back onto the image.  Deterministic: block
 * partial sums are reduced in a fixed order.
 */
#ifndef RAIN_LOSS_H
#define RAIN_LOSS_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of workspace the forward needs: 3*C*H*W floats of maps + per-block partial sums */
size_t rl_workspace_bytes(int C, int H, int W);

/* img, gt: [C,H,W] fp32 contiguous device arrays; window: 11 HOST floats (the reference's 1-D
 * gaussian(11, 1.5), normalised in fp32); out: loss[0] = total loss (device scalar); parts (device,
 * optional) = {total, L1 term, mean SSIM}. */
int rl_l1_ssim_forward(const float* img, const float* gt, int C, int H, int W, float lambda, const float* window,
                       void* workspace, size_t workspace_bytes, float* loss, float* parts, void* stream);

/* dimg = grad_loss[0] * dLoss/dimg (grad_loss: device scalar). */
int rl_l1_ssim_backward(const float* img, const float* gt, int C, int H, int W, float lambda, const float* window,
                        const void* workspace, const float* grad_loss, float* dimg, void* stream);

/* Forward and backward in one call, for a caller that needs both at once (a training step):
 * loss / parts exactly as rl_l1_ssim_forward, dimg exactly as rl_l1_ssim_backward; the finalize of
 * the loss rides on the backward launch (one launch less).  Not in the reference: its loss is
 * autograd over utils/loss_utils.py:22-53; this entry is the fused step's shortcut. */
int rl_l1_ssim_forward_backward(const float* img, const float* gt, int C, int H, int W, float lambda,
                                const float* window, void* workspace, size_t workspace_bytes, float* loss,
                                float* parts, const float* grad_loss, float* dimg, void* stream);

/*
 * Geometric regulariser on the rasterizer's aux maps (rain_amd/csrc/geom_loss.hip; no reference
 * counterpart): depth-normal consistency plus an optional metric depth prior.
 *
 * depth D [H,W] = sum a T z, alpha A [H,W] = sum a T, normal N [3,H,W] = sum a T n (fp32, contiguous,
 * unnormalised, as rr_forward_render_aux leaves them); gt_depth [H,W], 0 = no measurement.
 *   ok(p) = A(p) >= alpha_min,  z = D / A where ok,  r(p) = (((2x+1)/W - 1) tanfovx, ((2y+1)/H - 1) tanfovy, 1),
 *   P = z r.  Interior pixels with ok at p and its four axis neighbours:
 *   t_u = P(x+1,y) - P(x-1,y), t_v = P(x,y+1) - P(x,y-1), c = t_v x t_u, valid = |c|^2 > 0, n_d = c / |c|
 *   (a fronto-parallel plane gives (0,0,-1)).
 *   L_n = (1/HW) sum_valid (A - N . n_d),  L_d = (1/HW) sum_{ok, gt > 0} |z - gt|  (sign(0) = 0),
 *   loss = lambda_normal L_n + lambda_depth L_d,  parts = {loss, L_n, L_d, number of valid pixels}.
 * The masks are constants; gradients reach D, A (directly and through z) and N.
 * A term is evaluated only when its weight is non-zero and its map is given: normal may be NULL
 * with lambda_normal == 0 (then L_n and the valid count are 0 and d_normal may be NULL), gt_depth
 * may be NULL with lambda_depth == 0.  A non-zero weight without its map is an error (code 1).
 * Deterministic: no atomics, the loss is reduced from block partials in a fixed order.  Kernels
 * run on `stream`, no host synchronisation.  The 16-byte access form is used when W is a multiple
 * of 4 and every pointer is 16-byte aligned; calls that agree on that give bitwise equal results.
 */

/* bytes of workspace: 7 H W floats (the stencil's four depth gradients and n_d) + block partials */
size_t rl_geom_workspace_bytes(int H, int W);

/* loss[0] = the loss, parts (device, optional) as above; the workspace carries what the backward needs. */
int rl_geom_forward(const float* depth, const float* alpha, const float* normal, const float* gt_depth, int H, int W,
                    float tanfovx, float tanfovy, float alpha_min, float lambda_normal, float lambda_depth,
                    void* workspace, size_t workspace_bytes, float* loss, float* parts, void* stream);

/* d_depth [H,W], d_alpha [H,W], d_normal [3,H,W] = grad_loss[0] * dLoss/d(map) (grad_loss: device scalar);
 * every pixel is written.  `workspace` as rl_geom_forward left it for the same arguments. */
int rl_geom_backward(const float* depth, const float* alpha, const float* normal, const float* gt_depth, int H, int W,
                     float tanfovx, float tanfovy, float alpha_min, float lambda_normal, float lambda_depth,
                     const void* workspace, const float* grad_loss, float* d_depth, float* d_alpha, float* d_normal,
                     void* stream);

/* Both at once in two launches (the loss finalize rides on the second): loss / parts bitwise
 * rl_geom_forward's, the gradients bitwise rl_geom_backward's. */
int rl_geom_forward_backward(const float* depth, const float* alpha, const float* normal, const float* gt_depth,
                             int H, int W, float tanfovx, float tanfovy, float alpha_min, float lambda_normal,
                             float lambda_depth, void* workspace, size_t workspace_bytes, float* loss, float* parts,
                             const float* grad_loss, float* d_depth, float* d_alpha, float* d_normal, void* stream);

/*
 * Depth-distortion loss on the rasterizer's accumulated alpha A [H,W] and depth-moment maps
 * moments [2,H,W] = (M1, M2) (include/rain_raster.h rr_forward_render_dist):
 *   L = lambda_dist * (1/HW) sum_p (A M2 - M1^2)                       (no clamp)
 *   dL/dA = lambda_dist/HW M2,  dL/dM1 = -2 lambda_dist/HW M1,  dL/dM2 = lambda_dist/HW A.
 * loss[0] = L; parts (device, optional) = {L, the unweighted mean}.  Deterministic like rl_geom_*:
 * per-block partial sums in double reduced in a fixed order, no atomics, no host synchronisation.
 * Return codes as rl_geom_* (1 bad argument, 2 HIP error, 3 workspace too small).
 */
size_t rl_dist_workspace_bytes(int H, int W); /* the block partials */

int rl_dist_forward(const float* alpha, const float* moments, int H, int W, float lambda_dist, void* workspace,
                    size_t workspace_bytes, float* loss, float* parts, void* stream);

/* d_alpha [H,W], d_moments [2,H,W] = grad_loss[0] * dL/d(map) (grad_loss: device scalar).  d_moments is
 * overwritten.  accumulate_alpha != 0: the alpha gradient is ADDED to what d_alpha holds (one rounded
 * product, one add per pixel), so that rl_geom_*'s alpha gradient and this one combine without another
 * launch; 0: d_alpha is overwritten.  Needs no workspace. */
int rl_dist_backward(const float* alpha, const float* moments, int H, int W, float lambda_dist,
                     const float* grad_loss, float* d_alpha, float* d_moments, int accumulate_alpha, void* stream);

/* Both at once in two launches (the loss finalize rides on the second): loss / parts bitwise
 * rl_dist_forward's, the gradients bitwise rl_dist_backward's. */
int rl_dist_forward_backward(const float* alpha, const float* moments, int H, int W, float lambda_dist,
                             void* workspace, size_t workspace_bytes, float* loss, float* parts,
                             const float* grad_loss, float* d_alpha, float* d_moments, int accumulate_alpha,
                             void* stream);

const char* rl_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
