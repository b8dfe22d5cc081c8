/* sgrender.h -- C ABI of libsgrender.so: the MI355X (gfx950) implementation of the
 * spherical-Gaussian x microfacet render path of lzqsd/InverseRenderingOfIndoorScene.
 *
 * The reference has no native layer: this path is ~105 eager aten launches made from
 * Python.  The boundary a maintainer would bind is therefore the
 * reference's own Python call boundary, and each entry point below names the reference
 * call it replaces (file:line relative to the reference checkout).  INTEGRATION.md shows
 * the ctypes stub that goes on the reference side.
 *
 * Conventions
 *   - all tensors are fp32, contiguous, device (HBM) pointers; the layouts are the
 *     reference's NCHW-style layouts, spelled out per argument;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); every call
 *     only enqueues work on that stream: no allocation, no host synchronisation;
 *   - return value: 0 on success, otherwise a hipError_t (> 0) or one of the
 *     SGR_ERR_* codes (< 0); sgr_last_error() returns a thread-local description;
 *   - pointers marked "nullable" may be NULL to skip that output / input;
 *   - `premap`: 1 = `lamb` / `weight` are the light decoders' raw outputs and the entry point applies
 *     tan(pi/2 * 0.999 x) first (output2env.output2env, models.py:396-400); 0 = they are post-tan already
 *     (output2env.fromSGtoIm); 2 (backward entry points) = they are the post-tan values a forward call returned
 *     (`lamb_tan` / `weight_tan`), and the gradients are still those w.r.t. the RAW inputs -- the backward then
 *     applies the chain rule d tan = 0.999 pi/2 (1 + y^2) from y alone instead of re-evaluating 4K tangents per cell.
 *     3 (sgr_fused_fwd, sgr_fused_bwd_sg, sgr_fused_fwd_recon(_tan), sgr_fused_bwd_recon; where sgr_heads_prologue_supported
 *     says so) = `axis` / `lamb` / `weight` are the light decoders' LAST-CONVOLUTION outputs: the output activations of
 *     models.py:336-346 (1.01 tanh -> unit axis / clamp(0.5 (. + 1), 0, 1)) run as the
 *     kernels' prologue, then the tan pre-map; the backward entry points return the gradients w.r.t. those raw outputs
 *     (the heads' chain rule is their epilogue).  Same shapes; no intermediate tensors.
 *
 * Shapes:  bn images; K = SGNum lobes per cell (<= SGR_MAX_LOBES); env grid R x C
 *   (envRow x envCol == the renderingLayer ctor's imHeight x imWidth); J = eh*ew
 *   quadrature directions per cell; BRDF maps are imH x imW with imH/R == imW/C in {1, 2}
 *   (other ratios: pool first -- the host layer uses torch's adaptive_avg_pool2d, the reference's own op -- and pass R x C maps).
 */
#ifndef SGRENDER_H_
#define SGRENDER_H_

#ifdef __cplusplus
extern "C" {
#endif

#define SGR_ABI_VERSION 6
#define SGR_MAX_LOBES 32

#define SGR_OK 0
#define SGR_ERR_BAD_ARG (-1)        /* NULL required pointer, non-positive size */
#define SGR_ERR_UNSUPPORTED (-2)    /* K > SGR_MAX_LOBES, pooling ratio not in {1,2} */

int sgr_abi_version(void);
const char* sgr_last_error(void);

/* Direction table of output2env.__init__ (models.py:353-363) and renderingLayer.__init__
 * (models.py:437-452), device layout used by every kernel below (`dirs` argument):
 *   dirs[j*4 + {0,1,2,3}] = (l_x, l_y, l_z, omega_j),  j = e*ew + a,  padded with zero rows
 *   up to Jpad = sgr_dirs_padded(eh*ew) directions (a multiple of 32); followed by the same
 *   table in separable form (l_j = (s_e ca_a, s_e sa_a, c_e)):
 *   rows[e*8 + ..] = (s_e, c_e, omega_e, s_e^2, 2 s_e c_e, c_e^2, 0, 0)  for e < eh rounded up to even,
 *   cols (8*ew floats): (ca_a, sa_a) for a < ew/2, then at float offset ew (ca_a^2, 2 ca_a sa_a, sa_a^2, 0)
 *   for a < ew/2 (the second half row is the exact negation of the first), then at float offset 4*ew
 *   (ca_a, ca_a+1, sa_a, sa_a+1) per azimuth pair a = 0, 2, .. < ew/2 (operands of the packed-fp32 kernels).
 * Host-side helper: fills `out_host` (sgr_dirs_floats(eh, ew) floats of host memory). */
int sgr_dirs_padded(int J);
int sgr_dirs_floats(int eh, int ew);
int sgr_fill_direction_table(float* out_host, int eh, int ew);

/* View vectors of renderingLayer.__init__ (models.py:415-430): out_host[3*R*C]. */
int sgr_fill_view_vectors(float* out_host, int R, int C, float fov_deg, const float* camera_pos3);

/* output2env.output2env (models.py:391-404) when premap != 0, output2env.fromSGtoIm
 * (models.py:371-389) when premap == 0.
 *   axis   [bn,K,3,R,C]   lamb [bn,K,R,C]   weight [bn,3K,R,C] (channel k*3+rgb)
 *   env    [bn,3,R,C,eh,ew]  (out)
 *   lamb_tan [bn,K,R,C], weight_tan [bn,3K,R,C]  (out, nullable; post-tan values the
 *   reference returns alongside the env image) */
int sgr_sg_to_env_fwd(const float* axis, const float* lamb, const float* weight, const float* dirs,
                      float* env, float* lamb_tan, float* weight_tan,
                      int bn, int K, int R, int C, int eh, int ew, int premap, void* stream);

/* renderingLayer.forwardEnv (models.py:461-522).
 *   albedo, normal [bn,3,imH,imW]   rough [bn,1,imH,imW]   env [bn,3,R,C,eh,ew]
 *   view [3,R,C] (sgr_fill_view_vectors)   diffuse, spec [bn,3,R,C] (out) */
int sgr_render_env_fwd(const float* albedo, const float* normal, const float* rough, const float* env,
                       const float* dirs, const float* view, float* diffuse, float* spec,
                       int bn, int R, int C, int eh, int ew, int imH, int imW, float F0, void* stream);

/* Fused output2env.output2env + renderingLayer.forwardEnv (wrapperBRDFLight.py:177,194
 * back to back): one pass, the env image is written only if `env` is non-NULL. */
int sgr_fused_fwd(const float* albedo, const float* normal, const float* rough,
                  const float* axis, const float* lamb, const float* weight,
                  const float* dirs, const float* view,
                  float* env /* nullable */, float* diffuse, float* spec,
                  int bn, int K, int R, int C, int eh, int ew, int imH, int imW, float F0,
                  int premap, void* stream);

/* sgr_fused_fwd that also returns the post-tan sharpness / intensity (nullable; the values output2env.output2env
 * returns next to the env image, models.py:396-404) for the backward entry points' premap = 2 mode. */
int sgr_fused_fwd_tan(const float* albedo, const float* normal, const float* rough,
                      const float* axis, const float* lamb, const float* weight,
                      const float* dirs, const float* view,
                      float* env /* nullable */, float* lamb_tan /* nullable */, float* weight_tan /* nullable */,
                      float* diffuse, float* spec,
                      int bn, int K, int R, int C, int eh, int ew, int imH, int imW, float F0,
                      int premap, void* stream);

/* Backward of output2env.output2env / fromSGtoIm (torch.autograd of models.py:371-404).
 *   g_env [bn,3,R,C,eh,ew] in;  g_axis [bn,K,3,R,C], g_lamb [bn,K,R,C], g_weight [bn,3K,R,C] out.
 *   With premap == 1 the inputs are the raw decoder outputs and the gradients are w.r.t.
 *   those (chain rule through tan applied); premap == 2: the same gradients from post-tan inputs;
 *   with premap == 0 they are w.r.t. the post-tan lamb / weight (fromSGtoIm). */
int sgr_sg_to_env_bwd(const float* g_env, const float* axis, const float* lamb, const float* weight,
                      const float* dirs, float* g_axis, float* g_lamb, float* g_weight,
                      int bn, int K, int R, int C, int eh, int ew, int premap, void* stream);

/* Backward of the fused pass w.r.t. the SG parameters (what trainLight.py needs:
 * wrapperBRDFLight.py:194 detaches albedo, the BRDF nets are frozen, trainLight.py:121-144).
 *   g_env (nullable) is the cotangent of the env image coming from other consumers (the
 *   reconstruction loss, wrapperBRDFLight.py:179-188); the quadrature's own contribution
 *   to dL/dEnv is recomputed in-kernel from g_diffuse / g_spec and never written to HBM. */
int sgr_fused_bwd_sg(const float* g_env /* nullable */, const float* g_diffuse, const float* g_spec,
                     const float* albedo, const float* normal, const float* rough,
                     const float* axis, const float* lamb, const float* weight,
                     const float* dirs, const float* view,
                     float* g_axis, float* g_lamb, float* g_weight,
                     int bn, int K, int R, int C, int eh, int ew, int imH, int imW, float F0,
                     int premap, void* stream);

/* dL/dEnv of renderingLayer.forwardEnv alone (autograd of models.py:511-520):
 *   g_env[b,c,r,cc,j] = omega_j ndl_j (g_diffuse_c A_c/pi + g_spec_c spec_j)   (out, dense) */
int sgr_render_env_bwd_env(const float* g_diffuse, const float* g_spec,
                           const float* albedo, const float* normal, const float* rough,
                           const float* dirs, const float* view, float* g_env,
                           int bn, int R, int C, int eh, int ew, int imH, int imW, float F0, void* stream);

/* d/d{albedo, normal, rough} of renderingLayer.forwardEnv (autograd of models.py:461-522,
 * including the 2x2 pooling, the normal renormalisation and the local-frame construction).
 * The env image is either given (`env` non-NULL: the un-fused API) or re-evaluated from the
 * SG parameters (`env` NULL: the fused API; premap as in sgr_fused_fwd).
 *   g_albedo, g_normal [bn,3,imH,imW], g_rough [bn,1,imH,imW]  (out, fully written) */
int sgr_render_bwd_brdf(const float* g_diffuse, const float* g_spec,
                        const float* albedo, const float* normal, const float* rough,
                        const float* env /* nullable */,
                        const float* axis, const float* lamb, const float* weight /* nullable trio */,
                        const float* dirs, const float* view,
                        float* g_albedo, float* g_normal, float* g_rough,
                        int bn, int K, int R, int C, int eh, int ew, int imH, int imW, float F0,
                        int premap, void* stream);

/* ---- scale-invariant regressions and the render loss ------------------------------------- */

/* Floats of scratch the loss entry points need for a batch of bn images. */
int sgr_loss_workspace_floats(int bn);

/* Render loss of wrapperBRDFLight.py:170-171,192,197-207 for this rank's shard:
 *   im_small = avgpool(im), seg_small = avgpool(seg)              (:170-171)
 *   (kd, ks) = LSregressDiffSpec coefficients of (diffuse, spec, im_small)   (models.py:23-84)
 *   rendered = clamp(kd diffuse + ks spec, 0, 1)                  (:203)
 *   parts[0] = sum (rendered - im_small)^2 seg_small,  parts[1] = sum seg_small   (:192,205-207)
 * The caller forms renderErr = parts[0] / max(parts[1], 1e-5) / 3 (after summing parts over
 * ranks when the batch is sharded).  No host synchronisation.
 *   diffuse, spec [bn,3,R,C]   im [bn,3,imH,imW]   seg [bn,1,imH,imW]   (imH/R == imW/C in {1,2})
 *   out: im_small, rendered [bn,3,R,C]; seg_small [bn,1,R,C]; coef [bn,2]; parts [2] */
int sgr_render_loss_fwd(const float* diffuse, const float* spec, const float* im, const float* seg,
                        float* im_small, float* seg_small, float* rendered, float* coef, float* parts,
                        float* workspace, int bn, int R, int C, int imH, int imW, void* stream);

/* The same three passes, with the loss value formed by the third one when the batch is not sharded (no separate
 * sgr_loss_finalize launch):  *loss = parts[0] / max(parts[1], 1e-5) / divisor,  *scale = d loss / d parts[0]
 * (wrapperBRDFLight.py:192,205-207: divisor 3).  loss and scale may both be NULL (= sgr_render_loss_fwd: all-reduce
 * parts over the ranks, then sgr_loss_finalize).  Three launches; the batch totals are folded by the last workgroup of
 * the third pass to arrive, in a fixed order (bit-reproducible). */
int sgr_render_loss_fwd_total(const float* diffuse, const float* spec, const float* im, const float* seg,
                              float* im_small, float* seg_small, float* rendered, float* coef, float* parts,
                              float* loss /* [1], nullable */, float* scale /* [1], nullable */, float divisor,
                              float* workspace, int bn, int R, int C, int imH, int imW, void* stream);

/* ABI 5.  sgr_render_loss_fwd_total on one rank (loss / scale required) that also writes
 *   g_diffuse, g_spec [bn,3,R,C] = weight * d loss / d{diffuse, spec}
 * from its third pass -- bit-identical to sgr_render_loss_bwd_scaled(NULL, weight, scale, ...) without that fourth launch.  For callers
 * that form their gradients ahead of the backward call (the fused light objective: wrapperBRDFLight.py:192-207 + trainLight.py:237). */
int sgr_render_loss_fwd_total_grads(const float* diffuse, const float* spec, const float* im, const float* seg,
                                    float* im_small, float* seg_small, float* rendered, float* coef, float* parts,
                                    float* loss /* [1] */, float* scale /* [1] */, float divisor, float weight,
                                    float* g_diffuse, float* g_spec,
                                    float* workspace, int bn, int R, int C, int imH, int imW, void* stream);

/* d parts[0] / d{diffuse, spec} times *g_num (a device scalar); coefficients are constants as in
 * the reference (detached, models.py:54,76; wrapperBRDFLight.py:197-201). */
int sgr_render_loss_bwd(const float* g_num, const float* diffuse, const float* spec,
                        const float* im_small, const float* seg_small, const float* coef,
                        float* g_diffuse, float* g_spec, int bn, int R, int C, void* stream);

/* The two steps around the all-reduce of `parts` under batch sharding, kept on the device:
 *   sgr_loss_finalize:  *loss = parts[0] / max(parts[1], 1e-5) / divisor  (renderErr, wrapperBRDFLight.py:192,205-207:
 *                       divisor 3; reconstErr, :179-188: divisor 3 * envHeight * envWidth),  *scale = d loss / d parts[0]
 *                       (two separate device scalars: one is returned to the caller, the other kept for the backward pass);
 *   sgr_render_loss_bwd_scaled:  sgr_render_loss_bwd with *g_num = *g_loss * weight * *g_scale (g_scale = scale; a NULL device
 *                       scalar = 1; `weight` is a host float: the render weight of trainLight.py:237 travels as a kernel argument,
 *                       not through a cached device tensor -- ABI 4). */
int sgr_loss_finalize(const float* parts /* [2], rank-summed */, float* loss /* [1] */, float* scale /* [1] */, float divisor, void* stream);

int sgr_render_loss_bwd_scaled(const float* g_loss /* nullable */, float weight, const float* g_scale /* nullable */, const float* diffuse, const float* spec,
                               const float* im_small, const float* seg_small, const float* coef,
                               float* g_diffuse, float* g_spec, int bn, int R, int C, void* stream);

/* models.LSregress (models.py:7-21): coef[b] = clamp(<pred_b,gt_b> / max(<pred_b,pred_b>,1e-5), 1e-3, 1e3);
 * n elements per image. */
int sgr_lsregress_coef(const float* pred, const float* gt, float* coef, float* workspace,
                       int bn, long long n, void* stream);

/* models.LSregressDiffSpec (models.py:23-84): coef[b] = (c_im c_d, c_im c_s); n elements per image. */
int sgr_lsregress_diffspec_coef(const float* diffuse, const float* spec, const float* im, float* coef,
                                float* workspace, int bn, int n, void* stream);

/* utils.predToShading (utils.py:156-195): per-cell cosine-weighted irradiance of the
 * SG mixture, shading[b,c,r,cc] = max(sum_j env_c(l_j) cos(El_j) sin(El_j), 0) over an eh x ew hemisphere grid
 * (the reference uses 16 x 32).  Needs ew in {16, 32}, K <= 24 (SGR_ERR_UNSUPPORTED otherwise).
 *   axis [bn,K,3,R,C]  lamb [bn,K,R,C]  weight [bn,3K,R,C]  ->  shading [bn,3,R,C] */
int sgr_sg_shading(const float* axis, const float* lamb, const float* weight, const float* dirs, float* shading,
                   int bn, int K, int R, int C, int eh, int ew, int premap, void* stream);

/* ---- reconstruction loss ------------------------------------------------ */

int sgr_recon_workspace_floats(int bn, int R, int C);

/* Log-L2 env reconstruction loss of wrapperBRDFLight.py:172-188 for this rank's shard (two HBM streaming
 * passes over the predicted and the ground-truth env images):
 *   mask[b,p] = seg_small[b,p] * env_ind[b] * [mean_{c,j} env_gt > 0.001]                         (:172-174)
 *   coef[b]   = clamp(<env mask, env_gt mask> / max(<env mask, env mask>, 1e-5), 1e-3, 1e3)       (models.LSregress)
 *   parts[0]  = sum mask (log(coef env + offset) - log(env_gt + offset))^2,  parts[1] = sum mask  (:179,183-187)
 * The caller forms reconstErr = parts[0] / max(parts[1], 1e-5) / 3 / (eh*ew) (after summing parts over ranks).
 *   env, env_gt [bn,3,R,C,eh,ew]   seg_small [bn,1,R,C]   env_ind [bn]
 *   out: mask [bn,R*C], coef [bn], parts [2] */
int sgr_recon_loss_fwd(const float* env, const float* env_gt, const float* seg_small, const float* env_ind,
                       float* mask, float* coef, float* parts, float* workspace,
                       int bn, int R, int C, int eh, int ew, float offset, void* stream);

/* g_env = *g_num * d parts[0] / d env  (coef is a constant, models.py:13);  g_env [bn,3,R,C,eh,ew] out. */
int sgr_recon_loss_bwd(const float* g_num, const float* env, const float* env_gt, const float* mask,
                       const float* coef, float* g_env,
                       int bn, int R, int C, int eh, int ew, float offset, void* stream);

/* Whether premap = 3 (decoder heads as a prologue, see Conventions) is available for a configuration: envWidth 16 or 32,
 * 6 < SGNum <= 24, the default kernels (no SGR_*_MODE override). */
int sgr_heads_prologue_supported(int K, int R, int C, int eh, int ew);

/* ---- trainLight objective without the env image (fully fused) --------------
 * wrapperBRDFLight.py:172-207 in two heavy passes; neither the predicted env image (:177) nor its
 * cotangent is ever written.  Needs ew == 16 or 32 and K <= 24 (sgr_fused_recon_supported; SGR_ERR_UNSUPPORTED
 * otherwise -- use sgr_fused_fwd + sgr_recon_loss_* there).  Workspace is shared by the two calls. */
int sgr_fused_recon_supported(int K, int R, int C, int eh, int ew);
int sgr_fused_recon_workspace_floats(int bn, int R, int C);

/* Forward: sgr_fused_fwd without the env output, plus the statistics of sgr_recon_loss_fwd stage 0 taken on
 * the fly against env_gt:  diffuse, spec [bn,3,R,C];  mask [bn,R*C];  coef [bn] (LSregress scale, models.py:7-21);
 * parts (nullable) = (0, sum mask) for this rank's shard: what a sharded caller all-reduces before the backward pass. */
int sgr_fused_fwd_recon(const float* albedo, const float* normal, const float* rough, const float* axis,
                        const float* lamb, const float* weight, const float* dirs, const float* view,
                        const float* env_gt, const float* seg_small, const float* env_ind,
                        float* diffuse, float* spec, float* mask, float* coef, float* parts, float* workspace,
                        int bn, int K, int R, int C, int eh, int ew, int imH, int imW, float F0, int premap,
                        void* stream);

/* sgr_fused_fwd_recon that also returns the post-tan sharpness / intensity for sgr_fused_bwd_recon(premap = 2). */
int sgr_fused_fwd_recon_tan(const float* albedo, const float* normal, const float* rough, const float* axis,
                            const float* lamb, const float* weight, const float* dirs, const float* view,
                            const float* env_gt, const float* seg_small, const float* env_ind,
                            float* lamb_tan /* nullable */, float* weight_tan /* nullable */,
                            float* diffuse, float* spec, float* mask, float* coef, float* parts, float* workspace,
                            int bn, int K, int R, int C, int eh, int ew, int imH, int imW, float F0, int premap,
                            void* stream);

/* sgr_fused_fwd_recon_tan with the object mask at its own resolution: seg [bn,1,segH,segW], (segH, segW) = (R, C) or (2R, 2C);
 * the latter is pooled 2x2 by the kernel (wrapperBRDFLight.py:171: adaptive_avg_pool2d's sum order), no separate pooling pass. */
int sgr_fused_fwd_recon_seg(const float* albedo, const float* normal, const float* rough, const float* axis,
                            const float* lamb, const float* weight, const float* dirs, const float* view,
                            const float* env_gt, const float* seg, int segH, int segW, const float* env_ind,
                            float* lamb_tan /* nullable */, float* weight_tan /* nullable */,
                            float* diffuse, float* spec, float* mask, float* coef, float* parts /* nullable */, float* workspace,
                            int bn, int K, int R, int C, int eh, int ew, int imH, int imW, float F0, int premap,
                            void* stream);

/* ABI 5.  The forward half of the light objective on ONE rank (wrapperBRDFLight.py:167-207 up to the two loss values) in four launches:
 * sgr_fused_fwd_recon_seg's statistics kernel, then sgr_render_loss_fwd_total's three passes with (i) the per-image fold of the env
 * statistics (coef_env, the mask sums in recon_workspace) as an extra workgroup per image of the first pass and (ii), when g_diffuse /
 * g_spec are given, ren_weight * d renderErr / d{diffuse, spec} written by the third -- what sgr_fused_fwd_recon_seg +
 * sgr_render_loss_fwd_total + sgr_render_loss_bwd_scaled did in six.  im [bn,3,imH,imW], seg [bn,1,imH,imW] with (imH, imW) = (R, C) or
 * (2R, 2C); BRDF maps brdfH x brdfW as in sgr_fused_fwd; the outputs are those of the calls it replaces (render_err = *loss, scale_r =
 * *scale with divisor 3).  Follow with sgr_fused_bwd_recon_total on the same recon_workspace. */
int sgr_light_objective_fwd(const float* albedo, const float* normal, const float* rough, const float* axis, const float* lamb,
                            const float* weight, const float* dirs, const float* view, const float* env_gt, const float* im,
                            const float* seg, const float* env_ind, float* lamb_tan /* nullable */, float* weight_tan /* nullable */,
                            float* diffuse, float* spec, float* mask, float* coef_env, float* im_small, float* seg_small,
                            float* rendered, float* coef_ds, float* parts_r, float* render_err, float* scale_r, float ren_weight,
                            float* g_diffuse /* nullable pair */, float* g_spec, float* recon_workspace, float* loss_workspace,
                            int bn, int K, int R, int C, int eh, int ew, int imH, int imW, int brdfH, int brdfW, float F0, int premap,
                            void* stream);

/* Backward of  objective = (render terms, through g_diffuse / g_spec) + rec_weight * reconstErr,
 *   reconstErr = num / max(den, 1e-5) / 3 / (eh*ew),  num = sum mask (log(coef env + offset) - log(env_gt + offset))^2,
 * w.r.t. the SG parameters, with env recomputed in registers.  den = *den_global when given (the mask sum
 * all-reduced over ranks) else this shard's own.  Also returns parts = (num, local sum mask): the loss value
 * comes out of the same pass.  g_axis [bn,K,3,R,C]  g_lamb [bn,K,R,C]  g_weight [bn,3K,R,C].
 * ABI 4: the three gradient outputs may be NULL together (g_diffuse / g_spec are then ignored and may be NULL too): the pass
 * skips its gradient half -- no shading frame, no cotangents, no accumulators -- and only returns parts: the loss value for
 * forward-only callers of the objective (evaluation loops under torch.no_grad(), testLight.py). */
int sgr_fused_bwd_recon(const float* albedo, const float* normal, const float* rough, const float* axis,
                        const float* lamb, const float* weight, const float* dirs, const float* view,
                        const float* env_gt, const float* mask, const float* coef, const float* den_global,
                        const float* g_diffuse /* nullable with the gradients */, const float* g_spec,
                        float* g_axis /* nullable trio */, float* g_lamb, float* g_weight, float* parts, float* workspace,
                        int bn, int K, int R, int C, int eh, int ew, int imH, int imW, float F0, int premap,
                        float offset, float rec_weight, void* stream);

/* sgr_fused_bwd_recon for an unsharded batch (den = this shard's own mask sum), with the objective's scalar tail taken in the same
 * fold (no sgr_objective_finalize launch):  *recon_err = num / max(den, 1e-5) / (3 eh ew),
 * *objective = ren_weight * *render_err + rec_weight * *recon_err  (trainLight.py:237).  applied2 (nullable): slot 0 of
 * sgr_rescale_inplace_flip's pair is set to 1 (the gradients are those of the objective itself). */
int sgr_fused_bwd_recon_total(const float* albedo, const float* normal, const float* rough, const float* axis,
                              const float* lamb, const float* weight, const float* dirs, const float* view,
                              const float* env_gt, const float* mask, const float* coef,
                              const float* g_diffuse, const float* g_spec,
                              float* g_axis, float* g_lamb, float* g_weight, float* parts, float* workspace,
                              int bn, int K, int R, int C, int eh, int ew, int imH, int imW, float F0, int premap,
                              float offset, float rec_weight, const float* render_err, float ren_weight,
                              float* objective, float* recon_err, float* applied2, void* stream);

/* ABI 6: sgr_fused_bwd_recon / sgr_fused_bwd_recon_total that also return the objective's gradients w.r.t. the BRDF maps:
 * g_albedo [bn,3,imH,imW], g_normal [bn,3,imH,imW], g_rough [bn,1,imH,imW] (imH x imW = 1x or 2x the env grid, the 2x2 pooling's adjoint
 * applied).  They are ren_weight x d renderErr / d map: the reconstruction term does not depend on the maps, so they come from the render
 * layer's BRDF backward from the SG lobes (sgr_render_bwd_brdf with env = NULL) driven by g_diffuse / g_spec, launched after the objective's
 * pass.  The three are given together (with the SG gradient trio) or all NULL, which is the plain entry point (SGR_ERR_BAD_ARG otherwise);
 * premap 3 with them is SGR_ERR_UNSUPPORTED (activate the decoder outputs with sgr_light_heads_fwd and call sgr_render_bwd_brdf). */
int sgr_fused_bwd_recon_brdf(const float* albedo, const float* normal, const float* rough, const float* axis,
                             const float* lamb, const float* weight, const float* dirs, const float* view,
                             const float* env_gt, const float* mask, const float* coef, const float* den_global,
                             const float* g_diffuse, const float* g_spec,
                             float* g_axis, float* g_lamb, float* g_weight,
                             float* g_albedo /* nullable trio */, float* g_normal, float* g_rough,
                             float* parts, float* workspace, int bn, int K, int R, int C, int eh, int ew, int imH, int imW,
                             float F0, int premap, float offset, float rec_weight, void* stream);
int sgr_fused_bwd_recon_total_brdf(const float* albedo, const float* normal, const float* rough, const float* axis,
                                   const float* lamb, const float* weight, const float* dirs, const float* view,
                                   const float* env_gt, const float* mask, const float* coef,
                                   const float* g_diffuse, const float* g_spec,
                                   float* g_axis, float* g_lamb, float* g_weight,
                                   float* g_albedo /* nullable trio */, float* g_normal, float* g_rough,
                                   float* parts, float* workspace, int bn, int K, int R, int C, int eh, int ew, int imH, int imW,
                                   float F0, int premap, float offset, float rec_weight, const float* render_err, float ren_weight,
                                   float* objective, float* recon_err, float* applied2, void* stream);

/* Tail of the light objective on the device: *recon_err = parts_e[0] / max(parts_e[1], 1e-5) / divisor_e (divisor 3 * eh * ew,
 * wrapperBRDFLight.py:179-188), *objective = ren_w * *render_err + rec_w * *recon_err (trainLight.py:237).  parts_e = (numerator,
 * env-mask sum), rank-summed by the caller when the batch is sharded. */
int sgr_objective_finalize(const float* render_err, const float* parts_e, float ren_w, float rec_w, float divisor_e,
                           float* objective, float* recon_err, void* stream);

/* Cotangent scaling for gradients produced ahead of the backward call: x[i][0..n[i]) *= *scale / *applied in
 * place (i < count <= 4; x, n are HOST arrays of device pointers / lengths), then *applied = *scale.  Skipped on the
 * device when the two are equal (the cotangent of a scalar objective is normally 1).  No host sync. */
int sgr_rescale_inplace(float* const* x, const long long* n, int count, const float* scale, float* applied, void* stream);

/* The same in ONE launch (1 <= count <= 4): `applied2` holds two slots, the factor currently applied in applied2[parity]; on
 * return the new one (*scale) is in applied2[1 - parity] -- the caller flips its parity after every call. */
int sgr_rescale_inplace_flip(float* const* x, const long long* n, int count, const float* scale, float* applied2, int parity,
                             void* stream);

/* ---- light-decoder output heads --------------------------------------------
 * The activations at the end of models.decoderLight.forward (models.py:336-346) for the three decoders
 * and, if `packed` is given, the cascade hand-off tensor envmapsPred of wrapperBRDFLight.py:167-168:
 *   axis   [bn,K,3,R,C] = a / max(|a|, 1e-6),  a = 1.01 tanh(x_axis)        (mode 0)
 *   lamb   [bn,K,R,C]   = clamp(0.5 (1.01 tanh(x_lamb) + 1), 0, 1)          (mode 1)
 *   weight [bn,3K,R,C]  = clamp(0.5 (1.01 tanh(x_weight) + 1), 0, 1)        (mode 2)
 *   packed [bn,7K,R,C]  = axis (3K channels) | lamb (K) | weight (3K)        (nullable)
 * x_* are the dconvFinal outputs ([bn,3K,R,C], [bn,K,R,C], [bn,3K,R,C]). */
int sgr_light_heads_fwd(const float* x_axis, const float* x_lamb, const float* x_weight,
                        float* axis, float* lamb, float* weight, float* packed,
                        int bn, int K, int R, int C, void* stream);

/* Cotangents may come through the separate outputs, the packed tensor, or both (each nullable; they add).
 * Clamp passes the cotangent on the closed interval, like torch; the norm clamp blocks it below 1e-6. */
int sgr_light_heads_bwd(const float* x_axis, const float* x_lamb, const float* x_weight,
                        const float* g_axis, const float* g_lamb, const float* g_weight, const float* g_packed,
                        float* gx_axis, float* gx_lamb, float* gx_weight,
                        int bn, int K, int R, int C, void* stream);

/* ---- glue either side of the path ---------------------------------------------- */

/* Floats of workspace for the two calls below. */
int sgr_glue_workspace_floats(int bn);

/* testReal.py:421-432: the global light / albedo scale after LSregressDiffSpec, kept on the device
 * (the reference reads four sums back with .item()):
 *   cDiff = sum(diffuse_scaled) / sum(diffuse),  cSpec = sum(spec_scaled) / sum(spec)      (sums over all n elements)
 *   cSpec < 1e-3 ?  cAlbedo = 1 / max(albedo), cLight = cDiff / cAlbedo
 *                :  cLight = cSpec, cAlbedo = clip(cDiff / cLight, 1e-3, 1 / max(albedo)), cLight = cDiff / cAlbedo
 * out4 = (cLight, cAlbedo, cDiff, cSpec).  n = elements of the four render images, n_albedo = elements of albedo. */
int sgr_light_albedo_scale(const float* diffuse_scaled, const float* diffuse, const float* spec_scaled, const float* spec,
                           const float* albedo, float* out4, float* workspace, long long n, long long n_albedo, void* stream);

/* wrapperBRDFLight.py:138-156: input of the light encoder from the BRDF predictions,
 *   out [bn,11,H,W] = cat( resize(im), resize(albedo / max(mean_b(albedo), 1e-10) / 3), 0.5 (resize(normal) + 1),
 *                          0.5 (resize(rough) + 1), resize(depth / max(mean_b(depth), 1e-10) / 3) )
 * with resize = F.interpolate(., [H,W], mode='bilinear') (align_corners=False), the means per image over all channels;
 * also writes the normalised albedo_norm [bn,3,h,w] and depth_norm [bn,1,h,w] the wrapper returns (:139-147).
 * im, albedo, normal [bn,3,h,w]; rough, depth [bn,1,h,w].  The reference uses H x W = 480 x 640. */
int sgr_light_input_fwd(const float* im, const float* albedo, const float* normal, const float* rough, const float* depth,
                        float* out, float* albedo_norm, float* depth_norm, float* workspace, int bn, int h, int w, int H, int W,
                        void* stream);

/* ---- the bilateral solver layer (BilateralLayer.py:20-124, BilateralGrid.py:43-207) ------------------------------
 * Batched over B images of H x W pixels (N = H*W) and C = 1..3 target channels, fp64 inside, nothing read back to the host.
 * nvertices <= N, so image b owns the slots [b*N, (b+1)*N) of every per-vertex array; nvert[b] stays on the device.
 * The grid ("grid tensors" below; vertex indices are per image):
 *   pix2vert int32 [B,N]      pixel -> vertex (vertices = distinct 5-D hashes in ascending order, np.unique's numbering)
 *   perm     int32 [B,N]      pixels sorted by vertex, ascending pixel index inside a vertex
 *   seg      int32 [B,N]      vertex -> first position of its pixels in perm
 *   nbr      int32 [B,N,10]   vertex -> neighbour along -+x, -+y, -+luma, -+U, -+V; -1 = absent
 *   nvert    int32 [B]
 *   m, n     fp64  [B,N]      the bistochastisation's diagonals (BilateralGrid.py:106-118)
 * Contract: BilateralGrid.solve / solveForGrad with scipy's cg(rtol = cg_tol, atol = 0, maxiter = cg_maxiter). */

/* Bytes of workspace for the calls below (the largest of them); negative = SGR_ERR_*.  Pure host function. */
long long sgr_bs_workspace_bytes(int B, int H, int W, int C);

/* keys [B*N] int64 = image index * 2^44 + 5-D hash + 2^43 of every pixel of image [B,3,H,W] (fp32, the guide in [0,1]; coordinates
 * in fp64 as BilateralGrid.py:43-60).  The caller sorts them with ANY STABLE sort, keeping the sorted positions' original
 * indices (int64, 0..B*N-1), and hands both to sgr_bs_grid_build.  Colour bandwidths below 0.25 are unsupported. */
int sgr_bs_grid_keys(const float* image, long long* keys, int B, int H, int W, double sigma_luma, double sigma_chroma,
                     double sigma_spatial, void* stream);

/* The grid tensors from the sorted keys: vertex numbering, neighbour table, ten bistochastisation sweeps. */
int sgr_bs_grid_build(const long long* sorted_keys, const long long* sorted_index, int* pix2vert, int* perm, int* seg, int* nbr,
                      int* nvert, double* m, double* n, void* workspace, int B, int H, int W, void* stream);

/* BilateralGrid.solve: out [B,C,H,W] = slice(yhat), yhat [B,N,C] fp64 (kept for the backward).  pred [B,C,H,W], conf [B,H,W]. */
int sgr_bs_solve_fwd(const int* pix2vert, const int* perm, const int* seg, const int* nbr, const int* nvert, const double* m,
                     const double* n, const float* pred, const float* conf, float* out, double* yhat, void* workspace, int B, int C,
                     int H, int W, double lam, double A_diag_min, double cg_tol, int cg_maxiter, void* stream);

/* BilateralGrid.solveForGrad: g_pred [B,C,H,W] = slice(yb) conf, g_conf [B,H,W] = sum_c slice(-yb yhat) + slice(yb) pred. */
int sgr_bs_solve_bwd(const int* pix2vert, const int* perm, const int* seg, const int* nbr, const int* nvert, const double* m,
                     const double* n, const float* g_out, const float* pred, const float* conf, const double* yhat, float* g_pred,
                     float* g_conf, void* workspace, int B, int C, int H, int W, double lam, double A_diag_min, double cg_tol,
                     int cg_maxiter, void* stream);

/* ---- the BRDF-stage training objectives (wrapperBRDF.py:109-130 = trainBRDF.py:248-286, wrapperNYU.py:97-111, wrapperIIW.py:88-109) ----
 * Predictions and ground truth: albedo / normal [bn,3,H,W], rough / depth [bn,1,H,W]; masks seg_brdf, seg_all, seg_depth [bn,1,H,W] with
 * values in [0,1] (not assumed binary).  A NULL prediction (with its ground truth NULL too) leaves that term out: it is neither read nor
 * written and its error is 0.  seg_brdf masks albedo and roughness, seg_all masks the normal, seg_depth (NULL = seg_all) the depth.
 * `albedo_pred` / `depth_pred` are the wrappers' tensors of those names (after 0.5 (decoder + 1)).  Contract: DESIGN.md section 8b.
 *   coef   [bn,2]  the (albedo, depth) LSregress coefficients (models.py:13-14), 0 for an absent term
 *   parts  [8]     (numAlbedo, numNormal, numRough, numDepth, numAngle, nObj, nAll, nDep): this rank's batch totals, to be summed over
 *                  ranks when the batch is sharded
 *   values [6]     (total, albedoErr, normalErr, roughErr, depthErr, angleMean in degrees) with the denominators through max(., 1e-5)
 *                  and total = w_albedo albedoErr + w_normal normalErr + w_rough roughErr + w_depth depthErr */

/* Floats of workspace for sgr_brdf_objective_fwd.  Pure host function. */
int sgr_brdf_objective_workspace_floats(int bn);

/* Three launches: coef, parts and -- unless `values` is NULL (sharded batches: all-reduce parts, then sgr_brdf_objective_finalize) -- values. */
int sgr_brdf_objective_fwd(const float* albedo_pred, const float* albedo, const float* normal_pred, const float* normal,
                           const float* rough_pred, const float* rough, const float* depth_pred, const float* depth,
                           const float* seg_brdf, const float* seg_all, const float* seg_depth, float* coef, float* parts, float* values,
                           float* workspace, int bn, int H, int W, float w_albedo, float w_normal, float w_rough, float w_depth,
                           float depth_offset, void* stream);

/* values [6] from the (rank-summed) parts [8]. */
int sgr_brdf_objective_finalize(const float* parts, float* values, float w_albedo, float w_normal, float w_rough, float w_depth,
                                void* stream);

/* One launch: the gradients of  g_total total + g_albedo_err albedoErr + ... + g_depth_err depthErr  with respect to the predictions.
 * The five upstream gradients are device scalars, each nullable (= 0).  g_*_pred: nullable = not wanted (that term's planes are not
 * read).  The coefficients are constants (models.py:13 detaches them); the albedo clamp passes gradient on 0 <= albedo_pred coef <= 1.
 * `parts` holds the GLOBAL denominators (after the all-reduce when sharded). */
int sgr_brdf_objective_bwd(const float* g_total, const float* g_albedo_err, const float* g_normal_err, const float* g_rough_err,
                           const float* g_depth_err, const float* albedo_pred, const float* albedo, const float* normal_pred,
                           const float* normal, const float* rough_pred, const float* rough, const float* depth_pred, const float* depth,
                           const float* seg_brdf, const float* seg_all, const float* seg_depth, const float* coef, const float* parts,
                           float* g_albedo_pred, float* g_normal_pred, float* g_rough_pred, float* g_depth_pred, int bn, int H, int W,
                           float w_albedo, float w_normal, float w_rough, float w_depth, float depth_offset, void* stream);

/* The IIW ranking objective of a whole batch (models.py:526-563 per image, wrapperIIW.py:105-109 over the batch).
 *   albedo_pred [B,3,H,W];  *_point int32 [B,N,4] = (r1,c1,r2,c2);  *_weight [B,N];  *_num int32 [B] (clamped to 0..N; entries at or
 *   beyond it are ignored whatever they hold; a judgement with a row or column outside the image counts as weight 0 and is never
 *   dereferenced; an image with num == 0 contributes 0).  out2 = (eqLoss, darkerLoss).  2 (n_eq + n_darker) <= 4096. */
int sgr_ranking_loss_workspace_floats(int B);
int sgr_ranking_loss_fwd(const float* albedo_pred, const int* eq_point, const float* eq_weight, const int* eq_num,
                         const int* darker_point, const float* darker_weight, const int* darker_num, float* out2, float* workspace,
                         int B, int H, int W, int n_eq, int n_darker, float tau, void* stream);
/* g_albedo_pred [B,3,H,W] (dense, zero off the judged pixels) for the device scalars g_eq, g_darker (nullable = 0).  Judgements that
 * share a pixel are added in a fixed order (sorted endpoint records): bit-reproducible, no float atomics. */
int sgr_ranking_loss_bwd(const float* g_eq, const float* g_darker, const float* albedo_pred, const int* eq_point,
                         const float* eq_weight, const int* eq_num, const int* darker_point, const float* darker_weight,
                         const int* darker_num, float* g_albedo_pred, int B, int H, int W, int n_eq, int n_darker, float tau,
                         void* stream);

/* ---- the cascade-1 BRDF encoder's input (wrapperBRDF.py:56-100 = wrapperBRDFLight.py:58-92,106-108, trainFineTune*_cascade1.py:368-374,
 * testReal.py:439-449).  Contract: DESIGN.md section 8c.
 *   out [bn,17,H,W] = cat( im, norm(resize(albedo)), resize(normal'), resize(rough'), norm(resize(depth)),
 *                          resize(c_im c_d diffuse), resize(c_im c_s spec) )
 *   im [bn,3,H,W]; albedo, normal [bn,3,h,w]; rough, depth [bn,1,h,w]; diffuse, spec [bn,3,R,C].  A source of H x W is taken as it is,
 *   one smaller than H x W along an axis is resized with F.interpolate(., [H,W], mode='bilinear') (align_corners=False); any other
 *   source size is refused (the reference would fail in its torch.cat).
 *   remap      x' = 0.5 (x + 1) for normal and rough, applied before the resize; otherwise x' = x
 *   regress    (c_d, c_s, c_im) = models.LSregressDiffSpec (models.py:23-84) against adaptive_avg_pool2d(im, (R,C)); otherwise all 1
 *   normalize  norm(x) = x / max(mean over the resized map of image b, 1e-10) / 3.0; otherwise norm(x) = x
 *   coef [bn,2] = (c_im c_d, c_im c_s).
 * At most three launches on `stream`, nothing read back, bit-identical runs, image b independent of the rest of the batch. */

/* Floats of workspace for sgr_brdf_input_fwd.  Pure host function. */
int sgr_brdf_input_workspace_floats(int bn);

int sgr_brdf_input_fwd(const float* im, const float* albedo, const float* normal, const float* rough, const float* depth,
                       const float* diffuse, const float* spec, float* out, float* coef, float* workspace, int bn, int H, int W, int h,
                       int w, int R, int C, int regress, int normalize, int remap, void* stream);

/* ---- BRDF-decoder output heads (models.decoder0.forward, models.py:189-203, and the wrappers' 0.5 (x + 1) on the albedo and depth
 * decoders: wrapperBRDF.py, wrapperBRDFLight.py:112-115, wrapperNYU.py:89-92, wrapperIIW.py:83-86).  Contract: DESIGN.md section 8d.
 * With s(x) = clamp(1.01 tanh(x), -1, 1):
 *   albedo [bn,3,H,W] = s(x_c)                                   (mode 0)
 *   normal [bn,3,H,W] = t_c / max(|t|, 1e-6),  t_c = s(x_c)      (mode 1)
 *   rough  [bn,1,H,W] = (s(x_0) + s(x_1) + s(x_2)) / 3           (mode 2)
 *   depth  [bn,1,H,W] = s((x_0 + x_1 + x_2) / 3)                 (mode 4)
 * x_* are the dconvFinal outputs, [bn,3,H,W] each.  A NULL x leaves that decoder out: nothing is read or written for it.  `unit` != 0:
 * albedo and depth in the wrappers' form, 0.5 (. + 1).  One launch on `stream`, no workspace, bit-identical runs. */
int sgr_brdf_heads_fwd(const float* x_albedo, const float* x_normal, const float* x_rough, const float* x_depth, float* albedo,
                       float* normal, float* rough, float* depth, int bn, int H, int W, int unit, void* stream);

/* One launch: gx_* [bn,3,H,W] for the cotangents g_* (shaped like the outputs).  A NULL g is a zero cotangent; a NULL gx is not wanted
 * (that decoder's tensors are not read).  The clamp passes the cotangent on the closed interval, like torch; below |t| = 1e-6 the norm
 * path of the normal is blocked and the gradient is g / 1e-6 (the reference: NaN).  tanh is recomputed from x. */
int sgr_brdf_heads_bwd(const float* x_albedo, const float* x_normal, const float* x_rough, const float* x_depth, const float* g_albedo,
                       const float* g_normal, const float* g_rough, const float* g_depth, float* gx_albedo, float* gx_normal,
                       float* gx_rough, float* gx_depth, int bn, int H, int W, int unit, void* stream);

/* ---- CNN stage glue: GroupNorm + ReLU (+ skip concat + 2x bilinear upsample), the repeated stage of models.encoder0 / decoder0 /
 * encoderLight / decoderLight around its convolution (models.py:122-127, 160-183, 262-267, 307-330).  Contract: DESIGN.md section 8e.
 *   Cs == 0 (skip NULL):  out [B,C,H,W]        = relu(group_norm(x, G, weight, bias, eps))
 *   Cs >= 1:              out [B,C+Cs,2H,2W]   = interpolate(cat([relu(group_norm(x)), skip], 1), scale_factor=2, mode='bilinear')
 * x [B,C,H,W] and skip [B,Cs,H,W] are read through their element strides (x_strides / skip_strides: four long long each, host memory,
 * read during the call), so channels-last tensors need no copy; out, the gradients and the cotangent are contiguous.  weight, bias [C].
 * stats [B,G,4] = (mean, the mean's fp32 remainder, rstd, var) is written by the forward and is all the backward needs besides x.
 * Moments are double-precision (sum, sum of squares) folds.  Forward: two launches; backward: at most three; no atomics, bit-identical
 * runs, image b independent of the rest of the batch, the same bits for every layout of x and skip. */

/* Floats of workspace (8-byte aligned, owned by the caller) for the forward (backward == 0) or the backward of the plain (upcat == 0) or
 * the upsampling form.  Pure host function; 0 for sizes the entry points refuse. */
long long sgr_gn_stage_workspace_floats(int B, int C, int G, int H, int W, int upcat, int backward);

int sgr_gn_stage_fwd(const float* x, const float* weight, const float* bias, const float* skip, float* out, float* stats, float* workspace,
                     int B, int C, int G, int Cs, int H, int W, const long long* x_strides, const long long* skip_strides, float eps,
                     void* stream);

/* g: the cotangent of out.  dx [B,C,H,W], dweight [C], dbias [C], dskip [B,Cs,H,W]: a NULL one is not wanted and costs nothing; x, weight,
 * bias, stats and the workspace are needed only when dx, dweight or dbias is. */
int sgr_gn_stage_bwd(const float* g, const float* x, const float* weight, const float* bias, const float* stats, float* dx, float* dweight,
                     float* dbias, float* dskip, float* workspace, int B, int C, int G, int Cs, int H, int W, const long long* x_strides,
                     void* stream);

/* The same two with x, skip, out, the cotangent g, dx and dskip in bfloat16 (the 16 bits of an element as unsigned short; strides in
 * elements); weight, bias, stats, dweight, dbias and the workspace (sgr_gn_stage_workspace_floats, the same sizes) stay fp32.  Contract
 * (DESIGN.md section 8j): every bf16 result is the fp32 entry point's result on the upcast tensors, rounded once to bf16, round to nearest
 * even, bit for bit; stats, dweight and dbias are the fp32 entry point's bits.  The same kernels instantiated on the element type: the same
 * launches, sums in the same order, the same guarantees and the same refusals (with the fp32 entry points' messages). */
int sgr_gn_stage_fwd_bf16(const unsigned short* x, const float* weight, const float* bias, const unsigned short* skip, unsigned short* out,
                          float* stats, float* workspace, int B, int C, int G, int Cs, int H, int W, const long long* x_strides,
                          const long long* skip_strides, float eps, void* stream);

int sgr_gn_stage_bwd_bf16(const unsigned short* g, const unsigned short* x, const float* weight, const float* bias, const float* stats,
                          unsigned short* dx, float* dweight, float* dbias, unsigned short* dskip, float* workspace, int B, int C, int G,
                          int Cs, int H, int W, const long long* x_strides, void* stream);

/* ---- The same stage with the reference's resize-to-skip branch taken (models.py:165-166, 170-171, 175-176, 180-181, 185-186; decoderLight:
 * 312-313 ... 332-333): y = relu(group_norm(x)) [B,C,H,W] is resized to Hs x Ws by interpolate(., [Hs, Ws], mode='bilinear') first.
 *   Cs == 0 (skip NULL):  out [B,C,Hs,Ws]       = the resized map                                   (the final stage)
 *   Cs >= 1:              out [B,C+Cs,2Hs,2Ws]  = interpolate(cat([resized, skip], 1), scale_factor=2, mode='bilinear'),  skip [B,Cs,Hs,Ws]
 * Domain, per axis: H <= Hs <= 2H and W <= Ws <= 2W (equal sizes included); anything else is refused as "outside the resize domain".
 * The index rule is torch's for a given output size: scale = (float)H / (float)Hs in fp32, s = max(scale (o + 0.5) - 0.5, 0); a resized
 * value is rounded to fp32 before the 2x stage reads it.  Everything else -- strides, stats, workspace alignment, NULL gradients -- as
 * sgr_gn_stage_*.  Forward: two launches; backward: at most four (three when Cs == 0); no atomics, bit-identical runs. */
long long sgr_gn_resize_workspace_floats(int B, int C, int G, int H, int W, int Hs, int Ws, int upcat, int backward);

int sgr_gn_resize_fwd(const float* x, const float* weight, const float* bias, const float* skip, float* out, float* stats, float* workspace,
                      int B, int C, int G, int Cs, int H, int W, int Hs, int Ws, const long long* x_strides, const long long* skip_strides,
                      float eps, void* stream);

/* g: the cotangent of out.  dx [B,C,H,W], dweight [C], dbias [C], dskip [B,Cs,Hs,Ws]. */
int sgr_gn_resize_bwd(const float* g, const float* x, const float* weight, const float* bias, const float* stats, float* dx, float* dweight,
                      float* dbias, float* dskip, float* workspace, int B, int C, int G, int Cs, int H, int W, int Hs, int Ws,
                      const long long* x_strides, void* stream);

/* ---- The upsampling stage for D sibling decoders at once: the reference runs four decoder0 and three decoderLight
 * instances on the same encoder features, so at a stage every sibling has the same shapes and the same skip.  1 <= D <= SGR_GN_MAX_SIBLINGS.
 * xs, weights, biases, outs, gs, dxs, dweights, dbiases: host arrays of D device pointers, read during the call (no device-side table,
 * no copy: the calls capture in a HIP graph).  x_strides: D x 4 element strides, sibling after sibling.  stats [D,B,G,4].  skip is required.
 *   outs[d], stats[d]              the bits of sgr_gn_stage_fwd / sgr_gn_resize_fwd for (xs[d], weights[d], biases[d], skip)
 *   dxs[d], dweights[d], dbiases[d]  the bits of the single backward for gs[d]
 *   dskip                          ((s_0 + s_1) + s_2) + ..., fp32, in sibling order, s_d the single backward's dskip for gs[d] as it
 *                                  stands in registers (the bf16 form rounds the sum once); with D == 1 the single backward's bits
 * gs[d] == NULL: sibling d has no cotangent -- it is left out of the sum and gets no dx / dweight / dbias.  A NULL array of gradients, or a
 * NULL entry, is not wanted.  Forward: two launches for all D; backward: at most three (resize: four); no atomics, bit-identical runs,
 * image b independent of the rest of the batch, the same bits for every layout of xs[d] and skip.  D C + Cs and D G at most 65535.
 * Workspace: D blocks of the single operator's size (rounded up to 16 bytes), 16-byte aligned for 128-bit accesses, 8-byte at least. */
#define SGR_GN_MAX_SIBLINGS 8

long long sgr_gn_stage_siblings_workspace_floats(int D, int B, int C, int G, int H, int W, int backward);

int sgr_gn_stage_siblings_fwd(int D, const float* const* xs, const float* const* weights, const float* const* biases, const float* skip,
                              float* const* outs, float* stats, float* workspace, int B, int C, int G, int Cs, int H, int W,
                              const long long* x_strides, const long long* skip_strides, float eps, void* stream);

int sgr_gn_stage_siblings_bwd(int D, const float* const* gs, const float* const* xs, const float* const* weights, const float* const* biases,
                              const float* stats, float* const* dxs, float* const* dweights, float* const* dbiases, float* dskip,
                              float* workspace, int B, int C, int G, int Cs, int H, int W, const long long* x_strides, void* stream);

/* bf16 I/O as sgr_gn_stage_fwd_bf16 / _bwd_bf16: xs, skip, outs, gs, dxs and dskip in bfloat16 */
int sgr_gn_stage_siblings_fwd_bf16(int D, const unsigned short* const* xs, const float* const* weights, const float* const* biases,
                                   const unsigned short* skip, unsigned short* const* outs, float* stats, float* workspace, int B, int C,
                                   int G, int Cs, int H, int W, const long long* x_strides, const long long* skip_strides, float eps,
                                   void* stream);

int sgr_gn_stage_siblings_bwd_bf16(int D, const unsigned short* const* gs, const unsigned short* const* xs, const float* const* weights,
                                   const float* const* biases, const float* stats, unsigned short* const* dxs, float* const* dweights,
                                   float* const* dbiases, unsigned short* dskip, float* workspace, int B, int C, int G, int Cs, int H, int W,
                                   const long long* x_strides, void* stream);

/* the resize-to-skip form (fp32 only, as sgr_gn_resize_*): skip [B,Cs,Hs,Ws], outs[d] [B,C+Cs,2Hs,2Ws] */
long long sgr_gn_resize_siblings_workspace_floats(int D, int B, int C, int G, int H, int W, int Hs, int Ws, int backward);

int sgr_gn_resize_siblings_fwd(int D, const float* const* xs, const float* const* weights, const float* const* biases, const float* skip,
                               float* const* outs, float* stats, float* workspace, int B, int C, int G, int Cs, int H, int W, int Hs, int Ws,
                               const long long* x_strides, const long long* skip_strides, float eps, void* stream);

int sgr_gn_resize_siblings_bwd(int D, const float* const* gs, const float* const* xs, const float* const* weights, const float* const* biases,
                               const float* stats, float* const* dxs, float* const* dweights, float* const* dbiases, float* dskip,
                               float* workspace, int B, int C, int G, int Cs, int H, int W, int Hs, int Ws, const long long* x_strides,
                               void* stream);

/* The statistics of sgr_gn_stage_fwd without its apply pass: stats [B,G,4] of x [B,C,H,W] (read through x_strides), the same bits
 * sgr_gn_stage_fwd writes.  workspace: sgr_gn_stage_workspace_floats(B, C, G, H, W, 0, 0) floats, 8-byte aligned.  Two launches. */
int sgr_gn_moments(const float* x, float* stats, float* workspace, int B, int C, int G, int H, int W, const long long* x_strides, float eps,
                   void* stream);

/* ---- The BRDF decoders' final step, x_orig = dconvFinal(dpadFinal(dx6)) (models.py:155-156, 187): ReplicationPad2d(1) followed by
 * Conv2d(C -> 3, kernel 3, stride 1), without the padded copy.  Contract: DESIGN.md section 8g.  With cl(t, n) = min(max(t, 0), n - 1):
 *   out[b,o,i,j] = bias[o] + sum_{c,kh,kw} weight[o,c,kh,kw] y[b,c,cl(i+kh-1,H),cl(j+kw-1,W)]
 * x [B,C,H,W] is read through its element strides (x_strides: four long long, host memory, read during the call); weight [O,C,3,3],
 * bias [O], out [B,O,H,W], the cotangent and the gradients are contiguous.  O must be 3 and C at most 256; anything else is refused with
 * SGR_ERR_UNSUPPORTED and a message that names the composition to use.
 * stats == NULL: y = x.  stats [B,G,4] (sgr_gn_moments or sgr_gn_stage_fwd) with gn_weight, gn_bias [C]: y = relu(group_norm(x)) is formed
 * on load, with the bits sgr_gn_stage_fwd would have written, and never stored (G is ignored without stats).
 * Forward: one launch, no workspace.  Backward: one launch for dy, two for dweight / dbias; no atomics, bit-identical runs, image b
 * independent of the rest of the batch, the same bits for every layout of x. */

/* Floats of workspace (owned by the caller) for sgr_final_conv_bwd's dweight / dbias.  Pure host function; 0 for sizes the entry points refuse. */
long long sgr_final_conv_workspace_floats(int B, int C, int O, int H, int W);

int sgr_final_conv_fwd(const float* x, const float* weight, const float* bias, const float* gn_weight, const float* gn_bias, const float* stats,
                       float* out, int B, int C, int O, int G, int H, int W, const long long* x_strides, void* stream);

/* g: the cotangent of out.  dy [B,C,H,W] is the gradient at y (with a prologue: at the ReLU's output, unmasked -- sgr_gn_stage_bwd with
 * Cs == 0 masks it and carries it on to x); dweight [O,C,3,3], dbias [O].  A NULL one is not wanted and costs nothing: dy needs weight,
 * dweight needs x (and, with stats, the GroupNorm parameters: y is recomputed, not read), dweight / dbias need the workspace. */
int sgr_final_conv_bwd(const float* g, const float* x, const float* weight, const float* gn_weight, const float* gn_bias, const float* stats,
                       float* dy, float* dweight, float* dbias, float* workspace, int B, int C, int O, int G, int H, int W,
                       const long long* x_strides, void* stream);

/* ---- The light decoders' final pad + 3x3 convolution (csrc/sgr_light_final_conv.hip) --------------------------------
 * out = Conv2d(C -> O, k = 3)(ReplicationPad2d(1)(y)) -- x_orig = dconvFinal(dpadFinal(dx6)) of models.decoderLight (models.py:297-302, 334).
 * fp32; 1 <= O <= 48; C a multiple of 16 in 16..256; H, W >= 1, H * W < 2^26, B <= 65535.  y [B,C,H,W] is read through y_strides (4 element
 * strides, non-negative in the plane); everything else is contiguous: weight [O,C,3,3], bias [O], out [B,O,H,W].  Anything else returns
 * SGR_ERR_UNSUPPORTED and a message that names the composition to use, and launches nothing.
 * The forward and the data gradient run on the fp32-input matrix instruction (exact fp32, a fixed k-ordered fmaf chain); the weight and
 * bias gradients run on the vector ALU.  Forward: one launch, no workspace.  Backward: one launch for dy, two for dweight / dbias; no
 * atomics, bit-identical runs, image b independent of the rest of the batch, the same bits for every layout of y. */

/* Floats of workspace (owned by the caller) for sgr_light_final_conv_bwd's dweight / dbias.  Pure host function; 0 for sizes the entry points refuse. */
long long sgr_light_final_conv_workspace_floats(int B, int C, int O, int H, int W);

int sgr_light_final_conv_fwd(const float* y, const float* weight, const float* bias, float* out, int B, int C, int O, int H, int W,
                             const long long* y_strides, void* stream);

/* g: the cotangent of out.  dy [B,C,H,W], dweight [O,C,3,3], dbias [O].  A NULL one is not wanted and costs nothing: dy needs weight, dweight
 * needs y, dweight / dbias need the workspace. */
int sgr_light_final_conv_bwd(const float* g, const float* y, const float* weight, float* dy, float* dweight, float* dbias, float* workspace,
                             int B, int C, int O, int H, int W, const long long* y_strides, void* stream);

/* ---- The encoders' pad + 4x4 stride-2 convolution (csrc/sgr_encoder_conv.hip) -------------------------------------------
 * out = Conv2d(C -> O, k = 4, stride = 2)(pad(x)) with pad = ReplicationPad2d(1) (pad_mode 0) or ZeroPad2d(1) (pad_mode 1): encoder0.conv1 /
 * conv2 and encoderLight.preProcess[1] / [5] / conv1 of models.py:93-115, 122-126, 213-246, 254-266.  fp32; 1 <= C <= 160; O a multiple of
 * 16 in 16..128; H, W >= 2; Ho = H / 2, Wo = W / 2 (rounded down), Ho * Wo < 2^26; B <= 65535.  x [B,C,H,W] is read through x_strides (4
 * element strides, non-negative in the plane); everything else is contiguous: weight [O,C,4,4], bias [O], out [B,O,Ho,Wo].  Anything else
 * returns SGR_ERR_UNSUPPORTED and a message that names the composition to use (the deeper encoder layers stay F.pad + F.conv2d), and
 * launches nothing.  The forward, the data gradient and the weight gradient run on the fp32-input matrix instruction (exact fp32, a fixed
 * k-ordered fmaf chain); the bias gradient and, in replicate mode, the data gradient of the first and last row and column run on the vector
 * ALU.  No atomics: bit-identical runs, image b independent of the rest of the batch, the same bits for every layout of x. */

/* Floats of workspace (owned by the caller) for sgr_encoder_conv_bwd's dweight / dbias.  Pure host function; 0 for sizes the entry points refuse. */
long long sgr_encoder_conv_workspace_floats(int B, int C, int O, int H, int W);

int sgr_encoder_conv_fwd(const float* x, const float* weight, const float* bias, float* out, int B, int C, int O, int H, int W,
                         const long long* x_strides, int pad_mode, void* stream);

/* g: the cotangent of out.  dx [B,C,H,W], dweight [O,C,4,4], dbias [O].  A NULL one is not wanted and costs nothing: dx needs weight, dweight
 * needs x, dweight / dbias need the workspace. */
int sgr_encoder_conv_bwd(const float* g, const float* x, const float* weight, float* dx, float* dweight, float* dbias, float* workspace,
                         int B, int C, int O, int H, int W, const long long* x_strides, int pad_mode, void* stream);

/* The same convolution over S sources, 1 <= S <= SGR_ENCODER_CONV_MAX_SOURCES: the bits of sgr_encoder_conv_fwd / _bwd on the concatenation
 * of the sources along the channels, which is never written.  xs[i] is [B, channels[i], H, W], fp32, read through strides[4 i .. 4 i + 3];
 * channels[i] >= 1 and their sum C <= 160; weight [O,C,4,4].  xs, channels and strides are host arrays, read during the call: the table
 * travels in the kernel arguments, so a call captures in a HIP graph.  The forward is one launch.  dxs[i], contiguous
 * [B, channels[i], H, W], is the matching channel slice of the concatenation's dx; a NULL dxs[i] (or a NULL dxs) is not wanted, and its
 * channels are in no launch's range: the data gradient and, in replicate mode, its border launch run once per source that wants one.  xs
 * may be NULL when dweight is.  The workspace is sgr_encoder_conv_workspace_floats(B, C, O, H, W) floats.  S == 1 is sgr_encoder_conv_fwd /
 * _bwd, launch for launch.  Refusals return SGR_ERR_UNSUPPORTED with a message that names torch.cat(xs, 1) + F.pad + F.conv2d, and launch
 * nothing. */
#define SGR_ENCODER_CONV_MAX_SOURCES 4
int sgr_encoder_conv_cat_fwd(int S, const float* const* xs, const int* channels, const long long* strides, const float* weight, const float* bias,
                             float* out, int B, int O, int H, int W, int pad_mode, void* stream);
int sgr_encoder_conv_cat_bwd(int S, const float* g, const float* const* xs, const int* channels, const long long* strides, const float* weight,
                             float* const* dxs, float* dweight, float* dbias, float* workspace, int B, int O, int H, int W, int pad_mode, void* stream);

/* ---- the synthetic loader's batch preparation (dataLoader.py:118-154, 251-259, 286-310) ----
 * What BatchLoader.__getitem__ computes per sample between the decoded, resized files and the dataBatch tensors, for a whole batch on the
 * device.  Inputs of the training step: no adjoints.  uint8 tensors are HWC as PIL hands them over, fp32 ones as the HDR reader does.
 * No float atomics and nothing across workgroups: bit-identical runs, image b independent of the batch; nothing visits the host, so every
 * call captures in a HIP graph.  A size the kernels do not serve returns SGR_ERR_UNSUPPORTED with a message that names the numpy
 * composition of the reference, and launches nothing. */

/* seg_u8 [bn,H,W,Cin], channel 0: seg = 0.5 ((u8 - 127.5) / 127.5 + 1) in fp32; segArea = 0.49 < seg < 0.51, segEnv = seg < 0.1,
 * segObj = seg > 0.9, with erode != 0 eroded by a 7 x 7 box whose outside counts as set.  Outputs [bn,1,H,W] fp32 of exact 0 / 1. */
int sgr_loader_masks(const unsigned char* seg_u8, float* segArea, float* segEnv, float* segObj, int bn, int H, int W, int Cin, int erode,
                     void* stream);

/* hdr [bn,H,W,3] fp32.  v[b] = element k (0-based) of the ascending sort of hdr * seg (seg as above, broadcast over the channels): a radix
 * select over the order-preserving integer image of the floats, one workgroup per image.  scale[b] = num[b] / max(v[b], 0.1f); num NULL
 * means fp32(0.95 - 0.05), the TEST rule.  im [bn,3,H,W] = clip(scale hdr, 0, 1) with the channel axis reversed.  NaN / inf in hdr are
 * outside the domain (v is then some element of the data; nothing faults). */
int sgr_loader_scale_hdr(const float* hdr, const unsigned char* seg_u8, const float* num, float* im, float* scale, float* v, int bn, int H,
                         int W, int Cin, long long k, void* stream);

/* albedo = (0.5 ((u8 - 127.5) / 127.5 + 1))^2.2 and normal = n / sqrt(max(|n|^2, 1e-5)) from [bn,H,W,3], rough = channel 0 of
 * (u8 - 127.5) / 127.5 from [bn,H,W,rough_channels]; outputs [bn,C,H,W].  A NULL input is not wanted (at least one is). */
int sgr_loader_brdf_maps(const unsigned char* albedo_u8, const unsigned char* normal_u8, const unsigned char* rough_u8, float* albedo,
                         float* normal, float* rough, int bn, int H, int W, int rough_channels, void* stream);

/* env_raw [bn, rawH = R 16, rawW = C 32, 3] -> out [bn,3,R,C,envHeight,envWidth], 8 x 16 (the mean of 2 x 2 blocks,
 * ((a00 + a01) + (a10 + a11)) * 0.25f) or 16 x 32, times scale[b]; output channel k is file channel k.  env_ind [bn] (NULL: all ones):
 * an image with env_ind[b] == 0 gives exact zeros and its raw block is not read.  env_raw and out are 16-byte aligned. */
int sgr_loader_envmaps(const float* env_raw, const float* scale, const float* env_ind, float* out, int bn, int rawH, int rawW, int envHeight,
                       int envWidth, void* stream);

/* ---- testReal's output stage and the image writers (testReal.py:542-657, utils.py:65-76, 102-154) ----
 * From fp32 predictions on the device to tensors that are ready to write: uint8 HWC images and the env image's .npz layout.  No adjoints.
 * No float atomics and nothing across images: bit-identical runs, image b independent of its batch; nothing visits the host, so every
 * call captures in a HIP graph.  A refusal launches nothing. */
#define SGR_EXPORT_ALBEDO 0       /* C 3: t = 255 (x scale[b])^(1/2.2), resized                                     :544-556, 591-601 */
#define SGR_EXPORT_NORMAL 1       /* C 3: t = 255 * 0.5 (n + 1), resized                                            :559-567 */
#define SGR_EXPORT_ROUGH 2        /* C 1: t = 255 * 0.5 (r + 1), resized                                            :570-575, 604-609 */
#define SGR_EXPORT_DEPTH 3        /* C 1: d = x / max(mean(x[b]), 1e-10) * 3, resized; t = 255 / clip(d + 1, 1e-6, 10)   :578-587, 612-621 */
#define SGR_EXPORT_RENDERED 4     /* C 3: a = (x / max(x[b]))^(1/2.2), resized; t = clip(a, 0, 1) * 255              :649-657 */
#define SGR_EXPORT_SHADING 5      /* C 3: t = 255 clip(x / mean(x[b]) / 3, 0, 1)^(1/2.2), no resize                  :638-643 */
#define SGR_EXPORT_IMAGE 6        /* C 1 or 3 (1: three equal channels): t = 255 clip(x, 0, 1), no resize            utils.py:65-76 */
#define SGR_EXPORT_IMAGE_GAMMA 7  /*                                     t = 255 clip(x, 0, 1)^(1/2.2), no resize */

/* Floats of workspace sgr_export_image needs for `kind` (0: none -- the kind has no statistic); negative = SGR_ERR_*. */
long long sgr_export_image_workspace_floats(int kind, int B);

/* x [B,C,h,w] fp32, read through its element strides (x_strides: four long long, host memory, read during the call) -> out
 * [B,nh,nw,Cout] uint8, contiguous; Cout = C, for the two image kinds 3.  byte = (uint8) min(max(t, 0), 255) by truncation, a NaN gives 0.
 * The resize is OpenCV's INTER_LINEAR for float data: per axis f = (float)((d + 0.5) * ((double)in / out) - 0.5), s = floor(f), f -= s,
 * s < 0 -> (0, 0), s >= in - 1 -> (in - 1, 0); columns first, S[s] (1 - f) + S[s + 1] f, then rows, in fp32.  Kinds without a resize
 * need (nh, nw) == (h, w).  scale [B] (albedo only; NULL: 1).  bgr != 0 reverses the channels.  1 / 2.2 is formed in double and used as
 * fp32.  A kind with a statistic runs one more launch that leaves 64 partials per image in `workspace`. */
int sgr_export_image(const float* x, const long long* x_strides, const float* scale, unsigned char* out, float* workspace, int kind, int B, int C,
                     int h, int w, int nh, int nw, int bgr, void* stream);

/* utils.writeEnvToFile for every image: env [B,3,R,C,eh,ew] read through its six element strides -> out [B,Hm,Wm,3] uint8.  interY =
 * R / nrows, interX = C / ncols; cells r = 0, interY, .. and c = 0, interX, .. give ceil(R / interY) x ceil(C / interX) tiles (that can be
 * more than nrows x ncols), tile (i, j) at (i (eh + gap), j (ew + gap)); Hm = tiles_y (eh + gap) + gap, Wm alike; background 255;
 * t = 255 clip(v, 0, 1)^(1/2.2).  nrows > R or ncols > C is SGR_ERR_BAD_ARG.  Cells that are not sampled are not read. */
int sgr_export_env_mosaic(const float* env, const long long* env_strides, unsigned char* out, int B, int R, int C, int eh, int ew, int nrows,
                          int ncols, int gap, int bgr, void* stream);

/* env [B,3,R,C,eh,ew] contiguous -> out [B,R,C,eh,ew,3], out[..., j] = env[:, flip ? 2 - j : j]: exact copies.  128-bit accesses when
 * eh ew % 4 == 0 and both pointers are 16-byte aligned, element by element otherwise. */
int sgr_export_env_hwc(const float* env, float* out, int B, int R, int C, int eh, int ew, int flip, void* stream);

/* ---- the real-image loaders' batch preparation (nyuDataLoader.py:75-131, iiwDataLoader.py:136-137, 205-214) ----
 * From the decoded files, in the readers' layout, to the fp32 CHW tensors of the batch.  Inputs of the training step: no adjoints.  No
 * atomics and nothing across images: bit-identical runs, image b independent of its batch; nothing visits the host, so every call captures
 * in a HIP graph.  A refusal launches nothing. */

/* im_u8, normal_u8, seg_u8 [bn,Hs,Ws,3] uint8 in cv2.imread's channel order, depth [bn,Hs,Ws] fp32 -> normal [bn,3,H,W], depth, segNormal,
 * segDepth [bn,1,H,W], im [bn,3,H,W], contiguous fp32, in ONE launch.  Per source pixel, in fp32: output channel k of im and normal is file
 * channel 2 - k; im0 = 0.5 ((2 (u8 / 255)^2.2 - 1) + 1); n = (u8 - 127.5) / 127.5, n / sqrt(max(|n|^2, 1e-5)); segNormal0 =
 * 0.5 ((u8 - 127.5) / 127.5 + 1) of file channel 2.  crop [bn,4] int32 = (rs, cs, cropH, cropW): the array that is resized; NULL: the whole
 * source.  The kernel cannot refuse a rectangle it reads from device memory: one that leaves the source is moved and cut to lie inside it
 * (rs to [0, Hs - 1], cropH to [1, Hs - rs], columns alike), so nothing outside the source is ever read.  The resize to (H, W) is OpenCV's
 * INTER_LINEAR for float data (sgr_export_image above), the border clamp against the crop; equal sizes give the mapped values unchanged.
 * After it: segDepth = (depth > 1) && (depth < 10) as 0 / 1; normal / max(|normal|, 1e-5).  flip [bn] bytes (non-zero: output column x
 * takes column W - 1 - x in all five outputs and normal[0] is negated).  colour [bn,3] double: im = (float)((double)im * colour[b][c]).
 * crop, flip and colour come all three (TRAIN) or not at all (TEST).  128-bit stores when W % 4 == 0 and every output is 16-byte aligned. */
int sgr_nyu_prepare(const unsigned char* im_u8, const unsigned char* normal_u8, const unsigned char* seg_u8, const float* depth, const int* crop,
                    const unsigned char* flip, const double* colour, float* out_normal, float* out_depth, float* out_seg_normal,
                    float* out_seg_depth, float* out_im, int bn, int Hs, int Ws, int H, int W, void* stream);

/* im_u8 [bn,H,W,3] uint8 in PIL's channel order (resized and cropped on the host) -> out [bn,3,H,W] fp32 = (u8 / 255)^2.2 divided by its
 * maximum over the image, which is the value of the image's largest byte.  An all-black image gives 0 / 0 = NaN, as numpy does.
 * workspace: 64 * bn floats (the first launch leaves 64 partial maxima per image there). */
int sgr_iiw_image(const unsigned char* im_u8, float* out, float* workspace, int bn, int H, int W, void* stream);

/* ---- the evaluation metrics of the reference (CompareWHDR.py:8-66, CompareNormal.py:18-42, CompareDepth.py:16-32) ----
 * From the predictions on the device to one number per image.  Contract: DESIGN.md section 8o.  No float atomics, sums in double in a fixed
 * order: bit-identical runs, image b independent of its batch; nothing visits the host, so every call captures in a HIP graph.  A refusal
 * launches nothing. */

/* reflectance: fp32 (is_u8 == 0) or bytes (is_u8 != 0: divided by 255 in the kernel, the saved PNG's route), three channels, addressed by
 * strides [4] = (image, channel, row, column) in ELEMENTS -- [B,3,H,W] and [B,H,W,3] alike.  point int32 [B,N,4] = (r1, c1, r2, c2), weight
 * fp32 [B,N], label int32 [B,N] (0 'E', 1 '1', 2 '2'), num int32 [B] (clamped to 0..N; entries at or beyond it are ignored whatever they
 * hold).  Per judgement l = max(1e-10, (c0 + c1 + c2) / 3) in fp32; '1' if l2 / l1 > 1 + delta, else '2' if l1 / l2 > 1 + delta, else 'E'.
 * A weight <= 0 is skipped; a label outside 0..2 or a row or column outside the image counts as weight 0 and is never dereferenced.
 * sums [B,6] doubles = error, error_equal, error_inequal, weight, weight_equal, weight_inequal; out3 [3,B] fp32 = error / weight (0 / 0 = NaN
 * where the reference returns None), error_equal / (weight_equal + 1e-10), error_inequal / (weight_inequal + 1e-10). */
int sgr_eval_whdr(const void* reflectance, const long long* strides, int is_u8, const int* point, const float* weight, const int* label,
                  const int* num, double* sums, float* out3, int B, int H, int W, int N, float delta, void* stream);

/* doubles of the `partials` workspace of the two entries below: 64 * per * B with per = 3 (normal angle) or 5 (depth) */
long long sgr_eval_partials_doubles(int B, int per);

/* normal_pred fp32 [B,3,h,w] by strides [4] in elements, resized to H x W by OpenCV's INTER_LINEAR rule and NOT renormalised; normal_gt uint8
 * [B,H,W,3] contiguous in RGB order, gt = (byte - 127.5) / 127.5 divided by its norm; mask uint8 [B,H,W,mask_channels] contiguous
 * (mask_channels 1 or 3): a pixel counts when the minimum of its channels == 255.  theta [B,H,W] fp32 = acos(clip(dot, -1, 1)) / pi * 180 at
 * EVERY pixel (workspace and error image), keys [B,H,W] uint32 and partials (64 * 3 * B doubles): workspaces.  mean [B] = the double sum of
 * the counted angles / count; median [B] = numpy's (the middle element, or (a + b) * 0.5f of the two middle ones, by a radix select of both
 * ranks in one run); count [B] int32.  count == 0, or a NaN among the counted angles: NaN for both. */
int sgr_eval_normal_angle(const float* normal_pred, const long long* strides, const unsigned char* normal_gt, const unsigned char* mask,
                          int mask_channels, float* theta, unsigned* keys, double* partials, float* mean, float* median, int* count, int B,
                          int h, int w, int H, int W, void* stream);

/* depth_pred fp32 [B,h,w] and depth_gt fp32 [B,H,W], each by strides [3] = (image, row, column) in elements; the prediction is resized to
 * H x W by OpenCV's rule.  mask = 1 < gt < 10 (strict); both maps become log(x + 1e-20) in fp32 and lose their mean over ALL pixels;
 * rmse [B] = sqrt(sum mask (d - g)^2 / sum mask), from five double sums in one pass; count [B] int32 = sum mask; an empty mask gives NaN.
 * partials: 64 * 5 * B doubles. */
int sgr_eval_depth_log_rmse(const float* depth_pred, const long long* pred_strides, const float* depth_gt, const long long* gt_strides,
                            double* partials, float* rmse, int* count, int B, int h, int w, int H, int W, void* stream);

/* ---- PIL's antialiased resize of 8-bit images (dataLoader.py:223-224, iiwDataLoader.py:112-134: Image.resize(size, Image.ANTIALIAS)) ----
 * uint8 HWC in, uint8 HWC out: the bytes Pillow's ImagingResample gives, by integer arithmetic on a table of fixed-point coefficients
 * (22 fractional bits) that the host builds in double.  Contract: DESIGN.md section 8p.  filter: PIL's codes, 1 lanczos (the reference's
 * ANTIALIAS), 2 bilinear, 3 bicubic, 4 box, 5 hamming; 0 (nearest) is another code path of PIL's and is refused.  The source box is the whole
 * image; reducing_gap is not offered.  No atomics, nothing across images: bit-identical runs, image b independent of its batch; a call does
 * no host-device traffic, so it captures in a HIP graph.  A refusal launches nothing. */
#define SGR_PIL_RESIZE_AUTO 0
#define SGR_PIL_RESIZE_TWO_PASS 1     /* a launch per pass that runs, a uint8 intermediate in the workspace */
#define SGR_PIL_RESIZE_TILED 2        /* one launch, both passes through LDS; SGR_ERR_UNSUPPORTED where the tiles do not fit */

/* ints of one axis' table: 4 + 2 out_size + out_size ksize, ksize = 2 ceil(support max(in_size / out_size, 1)) + 1; negative = SGR_ERR_*. */
long long sgr_pil_resize_table_ints(int in_size, int out_size, int filter);

/* Host function, host memory: table[0] = ksize, [1] = 1 when some |k| >= 2^23 (the kernels then multiply in 32 bits, not 24), [2] = in_size,
 * [3] = out_size, then (xmin, xmax) per output index, then ksize coefficients per output index (zero past xmax).  In double, libm's sin and
 * cos, operation by operation as PIL.  SGR_ERR_UNSUPPORTED when a row has 2^21 + 255 sum |k| > 2^31 - 1 (the int32 sum could overflow). */
int sgr_pil_resize_table(int in_size, int out_size, int filter, int* table);

/* window: NULL (the whole resized image) or four ints (r0, c0, h, w), host memory: only that rectangle is computed.  Bytes of workspace
 * sgr_pil_resize_u8 needs on the two_pass route: bn x (the source rows the window's rows read) x (w C rounded up to 4) when both passes
 * run, else 0; negative = SGR_ERR_*. */
long long sgr_pil_resize_workspace_bytes(int bn, int H, int W, int C, int outH, int outW, const int* window, int filter);

/* 1 where the tiled route takes this geometry: both passes run, ksize <= 32 on both axes and the source extent of every 16 x 64 tile of the
 * window fits its LDS tiles (24 KiB of source bytes, 12 KiB of horizontally resized bytes); 0 otherwise; negative = SGR_ERR_*. */
int sgr_pil_resize_tiled_fits(int H, int W, int C, int outH, int outW, const int* window, int filter);

/* The route SGR_PIL_RESIZE_AUTO takes: SGR_PIL_RESIZE_TILED where the geometry fits and the launch has at least 256 tiles (bn x tiles of the
 * window; where tiled measured faster beyond the spread), else SGR_PIL_RESIZE_TWO_PASS; negative = SGR_ERR_*. */
int sgr_pil_resize_route(int bn, int H, int W, int C, int outH, int outW, const int* window, int filter);

/* src [bn,H,W,C] uint8 contiguous, C 1 or 3 -> dst [bn,h,w,C] uint8 contiguous, the window of the image resized to outH x outW (dst ==
 * resize-then-slice).  htable / vtable: the tables of (W, outW) and (H, outH) in DEVICE memory; NULL allowed for an axis whose size does not
 * change (that pass is skipped, not run as an identity; equal sizes copy).  The horizontal pass runs first, over the source rows the window's
 * rows read only, and is rounded to uint8 before the vertical pass.  workspace: device memory, may be NULL when the route needs none.
 * Bounds read from a table are cut to the source before use: a table that is not the geometry's gives wrong bytes, never a wild access. */
int sgr_pil_resize_u8(const unsigned char* src, int bn, int H, int W, int C, unsigned char* dst, int outH, int outW, const int* window,
                      int filter, const int* htable, const int* vtable, unsigned char* workspace, int path, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SGRENDER_H_ */
