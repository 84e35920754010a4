/* libsivae_hip — C ABI of the MI355X (gfx950 / CDNA4) Soft-IntroVAE training kernels.
 *
 * The reference (taldatech/soft-intro-vae-pytorch) has NO native layer: its hot path is a chain of
 * ATen ops issued from soft_intro_vae/train_soft_intro_vae.py.  This header is the drop-in boundary a
 * replacement shared library must export; each entry point names the reference op (file:line, all
 * relative to the reference checkout) whose arithmetic it reproduces.
 *
 * Conventions (all functions):
 *   - return int: 0 = ok; >0 = hipError_t of the launch; <0 = argument error (SIVAE_ERR_*).
 *   - never allocate, never synchronise, never touch global state: re-entrant, one stream per call.
 *   - all tensors are caller-owned device buffers, fp32, contiguous NCHW (or [rows][cols] where said).
 *   - scratch memory is passed as (workspace, workspace_bytes); sizes come from *_workspace_bytes().
 *   - `stream` is a hipStream_t (void* here so that the header needs no HIP include).
 */
#ifndef SIVAE_HIP_H
#define SIVAE_HIP_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIVAE_OK 0
#define SIVAE_ERR_NULL -1      /* a required pointer is null */
#define SIVAE_ERR_SHAPE -2     /* unsupported / inconsistent shape */
#define SIVAE_ERR_KSIZE -3     /* kernel size not in {1,3,5} */
#define SIVAE_ERR_WORKSPACE -4 /* workspace missing or too small */
#define SIVAE_ERR_RANGE -5     /* tensor too large for the kernels' 32-bit addressing */
#define SIVAE_ERR_MODE -6      /* unknown mode / flag value */

typedef void* sivae_stream_t;

/* ---- probes ---------------------------------------------------------------------------------- */
int sivae_abi_version(void);
const char* sivae_arch(void); /* "gfx950" */
int sivae_device_count(void);

/* ---- convolution (stride 1, padding k/2, k in {1,3,5}) ------------------------------------------
 * nn.Conv2d call sites: ResidualBlock conv_expand/conv1/conv2 train_soft_intro_vae.py:51-61, Encoder
 * stem :89, Decoder predict :159; nn.Linear :109,:146 run through ks = 1 with H = W = 1.
 * Weights are consumed in a packed GEMM layout produced by sivae_pack_conv_weight:
 *   mode 0 = forward operand, mode 1 = data-gradient operand (transposed + 180-degree flipped). */
int sivae_conv_ck(int ks);
int sivae_conv_ci_pad(int ks, int ci);
int sivae_conv_co_pad(int co);
size_t sivae_pack_conv_weight_bytes(int Co, int Ci, int ks, int mode);
int sivae_pack_conv_weight(const float* w /*[Co][Ci][ks][ks]*/, float* wp, int Co, int Ci, int ks, int mode,
                           sivae_stream_t stream);
/* Batched form (round 4): ONE launch rebuilds one operand form of EVERY weight of a network after its optimizer step
 * (torch.optim.Adam.step of train_soft_intro_vae.py:588,622 changes all of them; 35 per-weight launches of 5-11 us became
 * 5).  A job table lives in device memory and is reused from step to step (the packed buffers do not move):
 *   sivae_pack_job_fill   writes job `index` of a HOST table (sivae_pack_job_bytes() bytes per job) for operand form
 *                         0 direct (ks, mode) / 1 Winograd F(2x2,3x3) (mode) / 2 Winograd F(4x4,3x3) (mode) /
 *                         3 upsample-phase forward / 4 upsample-phase data gradient / 5 Winograd F(4x4,3x3) pre-split
 *                         into three bf16 pieces (mode; sivae_pack_wino4_b6_weight) / 6 bf16 operand slabs of the bf16
 *                         mode (ks incl. the code 51, mode; sivae_bf16_pack_conv_weight); dst = the buffer the per-weight
 *                         sivae_pack_* call of that form writes; returns the job's block count (its blocks are
 *                         [first_block, first_block + count) of the launch) or an error code (< 0)
 *   sivae_pack_batch      the launch: jobs_dev = the uploaded table, block_job_dev[b] = job index of block b (uint16) */
int sivae_pack_job_bytes(void);
int sivae_pack_job_fill(void* jobs_host, int index, int form, const float* w, float* dst, int Co, int Ci, int ks, int mode,
                        int first_block);
int sivae_pack_batch(int form, const void* jobs_dev, const unsigned short* block_job_dev, int n_blocks,
                     sivae_stream_t stream);

/* y[B][Co][H][W] (+)= conv(x', wp) + bias.
 *   x' = x, or LeakyReLU((x-pro_mean[c])*pro_invstd[c]*pro_gamma[c]+pro_beta[c], pro_slope) when
 *        pro_mean != NULL (producer BatchNorm2d + LeakyReLU fused into the load, :58-59,:90-91);
 *   upsample != 0: x is [B][Ci][H/2][W/2] and is read through nn.Upsample(2,'nearest') (:155);
 *   stats_partial != NULL: per-pixel-tile per-channel {sum, sumsq} of y, [n_px_tiles][Co][2], for the
 *        consumer BatchNorm2d (see sivae_bn_stats_from_conv_ws);
 *   accumulate != 0: y += result (used to sum the two branches of the residual data gradient).
 * The data gradient of the same conv is this function on dy with the mode-1 pack (Ci/Co swapped):
 * aten::convolution_backward (input half). */
int sivae_conv2d_fwd_num_px_tiles(int B, int Co, int H, int W);
int sivae_conv2d_fwd(const float* x, const float* wp, float* y, const float* bias, const float* pro_mean,
                     const float* pro_invstd, const float* pro_gamma, const float* pro_beta, float pro_slope,
                     float* stats_partial, int B, int Ci, int Co, int H, int W, int ks, int upsample,
                     int accumulate, sivae_stream_t stream);

/* Winograd F(2x2,3x3) version of sivae_conv2d_fwd for ks == 3 (same nn.Conv2d(k=3,s=1,p=1) of
 * soft_intro_vae/train_soft_intro_vae.py:56-61; same fused prologue / upsample / epilogues): 2.25x fewer
 * multiplies on the fp32 matrix pipe.  `up` is the transformed filter U = G g G^T from
 * sivae_pack_wino_weight (mode 0 forward, mode 1 data gradient).  Handles even H >= 8 and even W >= 16, and the 8x8 / 4x4 maps
 * (sivae_conv2d_wino_supported); stats_partial has sivae_conv2d_wino_num_px_tiles(B, H, W) rows.  bias must be
 * NULL (SIVAE_ERR_MODE otherwise): no 3x3 conv of the model has one. */
size_t sivae_pack_wino_weight_bytes(int Co, int Ci, int mode);
int sivae_pack_wino_weight(const float* w /*[Co][Ci][3][3]*/, float* up, int Co, int Ci, int mode,
                           sivae_stream_t stream);
int sivae_conv2d_wino_supported(int H, int W);
int sivae_conv2d_wino_num_px_tiles(int B, int H, int W);
int sivae_conv2d_wino_fwd(const float* x, const float* up, float* y, const float* bias, const float* pro_mean,
                          const float* pro_invstd, const float* pro_gamma, const float* pro_beta, float pro_slope,
                          float* stats_partial, int B, int Ci, int Co, int H, int W, int upsample, int accumulate,
                          sivae_stream_t stream);

/* Split-K form of sivae_conv2d_wino_fwd for launches that would leave most of the chip idle (the deep 4x4 / 8x8 layers
 * at small batch: the 16-image per-GPU shard of config 4): the input-channel range is cut into
 * sivae_conv2d_wino_splitk(...) slices computed by separate work items into `workspace`, and a fixed-order reduce kernel
 * sums them into y (+= with accumulate) and writes per-image {sum, sumsq} rows.  With 1 slice it IS
 * sivae_conv2d_wino_fwd.  stats_partial has sivae_conv2d_wino_splitk_stats_rows(...) rows. */
int sivae_conv2d_wino_splitk(int B, int Ci, int Co, int H, int W);
size_t sivae_conv2d_wino_splitk_workspace_bytes(int B, int Ci, int Co, int H, int W);
int sivae_conv2d_wino_splitk_stats_rows(int B, int Ci, int Co, int H, int W);
int sivae_conv2d_wino_fwd_splitk(const float* x, const float* up, float* y, const float* pro_mean,
                                 const float* pro_invstd, const float* pro_gamma, const float* pro_beta, float pro_slope,
                                 float* stats_partial, int B, int Ci, int Co, int H, int W, int upsample, int accumulate,
                                 void* workspace, size_t workspace_bytes, sivae_stream_t stream);

/* 3x3 conv of a nearest-2x-upsampled input (nn.Upsample :155 -> ResidualBlock.conv1 :56), computed on the low-resolution
 * tensor: four output-parity phases, each a 2x2 conv run as Winograd F(2x2,2x2) — 36 multiplies per 4x4 output pixels
 * instead of 64 (sivae_conv2d_wino_fwd with upsample) or 144 (direct).  x_half is [B][Ci][H/2][W/2], y is
 * [B][Co][H][W]; same BatchNorm+LeakyReLU prologue and BatchNorm-partials epilogue (stats_partial has
 * sivae_conv2d_wino_up_num_px_tiles(B, H, W) rows).  Forward only (the data gradient keeps the F(2x2,3x3) kernel).
 * Supported maps: H >= 16 even, W >= 32 with W % 4 == 0 (the kernel writes four output pixels per 16-byte store; y must be
 * 16-byte aligned). */
size_t sivae_pack_wino_up_weight_bytes(int Co, int Ci);
int sivae_pack_wino_up_weight(const float* w /*[Co][Ci][3][3]*/, float* up, int Co, int Ci, sivae_stream_t stream);
int sivae_conv2d_wino_up_supported(int H, int W);
int sivae_conv2d_wino_up_num_px_tiles(int B, int H, int W);
int sivae_conv2d_wino_up_fwd(const float* x_half, const float* up, float* y, const float* pro_mean,
                             const float* pro_invstd, const float* pro_gamma, const float* pro_beta, float pro_slope,
                             float* stats_partial, int B, int Ci, int Co, int H, int W, sivae_stream_t stream);

/* Data gradient of the same op with respect to the low-resolution input (replaces the full-resolution F(2x2,3x3) data
 * gradient followed by nn.Upsample's 2x2 block sum): one 2x2 conv over the 4*C parity planes dy[2i+p][2j+q] of
 * dy [B][C][2Hs][2Ws] (read in place with stride-2 addressing) as Winograd F(2x2,2x2) with the phases folded into K.
 * dx is [B][N][Hs][Ws] (N = the conv's input channels); accumulate != 0: dx += result.
 * sivae_space_to_depth2 materialises the parity planes ([B][4][C][Hs][Ws]); the kernels do not need it. */
int sivae_space_to_depth2(const float* in /*[B][C][2Hs][2Ws]*/, float* out /*[B][4][C][Hs][Ws]*/, int B, int C, int Hs,
                          int Ws, sivae_stream_t stream);
size_t sivae_pack_wino_up_dgrad_weight_bytes(int Co, int Ci);
int sivae_pack_wino_up_dgrad_weight(const float* w /*[Co][Ci][3][3]*/, float* ud, int Co, int Ci,
                                    sivae_stream_t stream);
int sivae_conv2d_wino_up_dgrad_supported(int Hs, int Ws);
int sivae_conv2d_wino_up_dgrad(const float* dy, const float* ud, float* dx, int B, int C, int N, int Hs, int Ws,
                               int accumulate, sivae_stream_t stream);
/* Split-K form for small shards (16 images per GPU: 512 -> 512 @16x16 is 128 work items each walking 4 x 512 planes):
 * _splitk = number of K slices the run would use (1: the plain kernel), _splitk_workspace_bytes = size of the partial
 * outputs (0 when 1 slice), _splitk_run = sliced kernel + fixed-order reduce (same numbers as the plain entry up to the
 * fp32 summation order of the slices). */
int sivae_conv2d_wino_up_dgrad_splitk(int B, int C, int N, int Hs, int Ws);
size_t sivae_conv2d_wino_up_dgrad_splitk_workspace_bytes(int B, int C, int N, int Hs, int Ws);
int sivae_conv2d_wino_up_dgrad_splitk_run(const float* dy, const float* ud, float* dx, int B, int C, int N, int Hs,
                                          int Ws, int accumulate, void* workspace, size_t workspace_bytes,
                                          sivae_stream_t stream);

/* Weight gradient of the same op in the phase form (dU_pq = sum_tiles (A dY_pq A^T).(B^T d_pq B), F(2x2,2x2);
 * dW folded back from the four 2x2 phase filters): 36 multiplies per 4x4 dy pixels instead of 64.  x_half is
 * [B][Ci][Hs][Ws], dy [B][Co][2Hs][2Ws], dw [Co][Ci][3][3]; deterministic two-pass reduction. */
int sivae_conv2d_wino_up_wgrad_supported(int Hs, int Ws);
size_t sivae_conv2d_wino_up_wgrad_workspace_bytes(int B, int Ci, int Co, int Hs, int Ws);
int sivae_conv2d_wino_up_wgrad(const float* x_half, const float* dy, float* dw, int B, int Ci, int Co, int Hs, int Ws,
                               void* workspace, size_t workspace_bytes, sivae_stream_t stream);

/* sivae_conv2d_wino_fwd used as a DATA GRADIENT whose output y = dL/dh feeds the backward of
 * h = LeakyReLU(BatchNorm(bn_x)) (:58-59): the epilogue also reads bn_x (same shape as y) and leaves per pixel tile
 * {sum g, sum g*xhat}, g = y * LeakyReLU'(z), in bnbwd_partial [sivae_conv2d_wino_num_px_tiles(B,H,W)][Co][2] —
 * the first reduction pass of the BatchNorm backward; sivae_bn_bwd_from_partials finishes it. */
int sivae_conv2d_wino_dgrad_bnbwd(const float* dy, const float* up, float* y, const float* bn_x, const float* bn_mean,
                                  const float* bn_invstd, const float* bn_gamma, const float* bn_beta, float slope,
                                  float* bnbwd_partial, int B, int Ci, int Co, int H, int W, sivae_stream_t stream);
int sivae_bn_bwd_from_partials(const float* dy, const float* x, const float* mean, const float* invstd,
                               const float* gamma, const float* beta, float slope, const float* partials, int n_tiles,
                               float* dx, float* dgamma, float* dbeta, int B, int C, int HW, void* workspace,
                               size_t workspace_bytes, sivae_stream_t stream);

/* Winograd-domain weight gradient for ks == 3 (dU = sum_tiles (A dY A^T) . (B^T d B), dW = G^T dU G): the
 * weight half of aten::convolution_backward for the nn.Conv2d(k=3) layers (:56-61) with 2.25x fewer multiplies;
 * same prologue / upsample options and the same deterministic two-pass reduction as sivae_conv2d_wgrad.
 * Maps: sivae_conv2d_wino_wgrad_supported(H, W) (even H >= 8, even W >= 16). */
int sivae_conv2d_wino_wgrad_supported(int H, int W);
size_t sivae_conv2d_wino_wgrad_workspace_bytes(int B, int Ci, int Co, int H, int W);
int sivae_conv2d_wino_wgrad(const float* x, const float* dy, float* dw, const float* pro_mean,
                            const float* pro_invstd, const float* pro_gamma, const float* pro_beta, float pro_slope,
                            int B, int Ci, int Co, int H, int W, int upsample, void* workspace,
                            size_t workspace_bytes, sivae_stream_t stream);

/* dw[Co][Ci][ks][ks] = weight gradient (aten::convolution_backward, weight half); x is read with the
 * same optional prologue / upsample addressing as the forward. Deterministic split-K. */
size_t sivae_conv2d_wgrad_workspace_bytes(int B, int Ci, int Co, int H, int W, int ks);
int sivae_conv2d_wgrad(const float* x, const float* dy, float* dw, const float* pro_mean,
                       const float* pro_invstd, const float* pro_gamma, const float* pro_beta, float pro_slope,
                       int B, int Ci, int Co, int H, int W, int ks, int upsample, void* workspace,
                       size_t workspace_bytes, sivae_stream_t stream);

/* ---- 1x1 convolution as a streaming kernel (ResidualBlock.conv_expand :50-54, forward and data gradient) ---------
 * y[b][co][p] (+)= sum_ci W[co][ci] x[b][ci][p] over planes of HW pixels; wp is the ks = 1 direct pack of
 * sivae_pack_conv_weight (mode 0 forward, mode 1 data gradient).  x goes straight from 16-byte global loads into the MFMA
 * B operand (a lane's four consecutive pixels serve four column tiles), the 64-channel weight tile lives in LDS, outputs
 * leave as 16-byte stores.  _supported: HW % 4 == 0, Ci even and <= 256. */
int sivae_conv1x1_stream_supported(int B, int Ci, int Co, int HW);
int sivae_conv1x1_stream(const float* x, const float* wp, float* y, int B, int Ci, int Co, int HW, int accumulate,
                         sivae_stream_t stream);

/* ---- 5x5 convolution FROM <= 3 channels INTO <= 64 with the whole contraction merged (K = 3*25 = 75) -----------
 * The encoder stem's forward (:88-89: nn.Conv2d(cdim, 64, 5, 1, 2)) and the data gradient of Decoder.predict (:159):
 * y[co][px] = sum_k W[co][k] X[k][px], k = (ci, kh, kw); 38 MFMA k-steps per 32x32 outputs instead of 50, weights in
 * registers.  pack mode 0: w [n_big][n_small][5][5] (forward); mode 1: w [n_small][n_big][5][5] (data gradient:
 * taps flipped, channels transposed).  stats_partial (optional): [sivae_conv5_k75_num_px_tiles(B, H, W)][Co][2]
 * {sum, sumsq} partials for the BatchNorm that follows the stem. */
size_t sivae_pack_conv5_k75_bytes(void);
int sivae_pack_conv5_k75(const float* w, float* wq, int n_small, int n_big, int mode, sivae_stream_t stream);
int sivae_conv5_k75_supported(int Ci, int Co);
int sivae_conv5_k75_num_px_tiles(int B, int H, int W);
int sivae_conv5_k75_fwd(const float* x, const float* wq, float* y, const float* bias, float* stats_partial, int B,
                        int Ci, int Co, int H, int W, sivae_stream_t stream);

/* ---- 5x5 convolutions with <= 3 channels on one side (Decoder.predict :159, Encoder stem :89) -------------
 * The small channel count is merged with the kernel column into one 16-wide MFMA dimension.
 *   pack: n_small = the <=3 side, n_big = the other; mode 0 = forward operand of a [n_small][n_big][5][5]
 *         weight (predict), mode 1 = data-gradient operand of a [n_big][n_small][5][5] weight (stem).
 *   sivae_conv5_smallco_fwd: y[B][Co<=3][H][W] = conv5x5(x[B][Ci][H][W]) + bias.
 *   sivae_conv5_edge_wgrad:  dw[Co][Ci][5][5] with min(Ci, Co) <= 3 (deterministic split over pixels). */
size_t sivae_pack_conv5_smallco_bytes(int n_small, int n_big);
int sivae_pack_conv5_smallco(const float* w, float* wq, int n_small, int n_big, int mode, sivae_stream_t stream);
int sivae_conv5_smallco_fwd(const float* x, const float* wq, float* y, const float* bias, int B, int Ci, int Co,
                            int H, int W, sivae_stream_t stream);
size_t sivae_conv5_edge_wgrad_workspace_bytes(int B, int Ci, int Co, int H, int W);
int sivae_conv5_edge_wgrad(const float* x, const float* dy, float* dw, int B, int Ci, int Co, int H, int W,
                           void* workspace, size_t workspace_bytes, sivae_stream_t stream);

/* ---- BatchNorm2d (training mode) + LeakyReLU + residual add ----------------------------------------
 * nn.BatchNorm2d(eps 1e-5, momentum 0.1) :58,:62,:90 ; nn.LeakyReLU(0.2) :59,:63,:91 ; torch.add :74.
 * running_var gets the unbiased variance, num_batches_tracked (int64, device) is incremented.  Statistics from the conv
 * epilogue's partials, the running-buffer replay, the apply pass and the backward take `seg_images` / `nseg` and are
 * declared under "segmented batches" below: one segment (seg_images == B, nseg = 1) is the unsegmented op. */
size_t sivae_bn_workspace_bytes(int B, int C, int HW);
int sivae_bn_stats(const float* x, int B, int C, int HW, float eps, float momentum, float* running_mean,
                   float* running_var, long long* num_batches_tracked, float* mean_out, float* invstd_out,
                   void* workspace, size_t workspace_bytes, sivae_stream_t stream);
/* ---- synchronised BatchNorm for data-parallel runs (opt-in): the shard's per-channel {sum, sumsq}
 * (fp64 [C][2]) from the conv-epilogue partials — the caller all-reduces it — and the finalize from the (global) sums
 * and the global element count.  Backward: `reduce` leaves the local {sum dz, sum dz*xhat} (fp64 [C][2]), `apply`
 * takes the local sums (-> dgamma, dbeta) and the all-reduced sums + global count (-> dx, dz). */
int sivae_bn_sums_from_conv(const float* partials, int n_tiles, int C, double* sums, sivae_stream_t stream);
int sivae_bn_finalize_sums(const double* sums, int C, double count, float eps, float momentum, float* running_mean,
                           float* running_var, long long* num_batches_tracked, float* mean_out, float* invstd_out,
                           sivae_stream_t stream);
int sivae_bn_bwd_reduce(const float* dy, const float* y, const float* x, const float* mean, const float* invstd,
                        const float* gamma, const float* beta, int act_mode, float slope, double* sums, int B, int C,
                        int HW, void* workspace, size_t workspace_bytes, sivae_stream_t stream);
int sivae_bn_bwd_apply(const float* dy, const float* y, const float* x, const float* mean, const float* invstd,
                       const float* gamma, const float* beta, int act_mode, float slope, const double* sums_local,
                       const double* sums_global, double count_global, float* dx, float* dz_out, float* dgamma,
                       float* dbeta, int B, int C, int HW, void* workspace, size_t workspace_bytes,
                       sivae_stream_t stream);
/* out[c] = sum over (B, HW) — bias gradient of Decoder.predict (:159). Workspace as sivae_bn_workspace_bytes. */
int sivae_channel_sum(const float* x, float* out, int B, int C, int HW, void* workspace, size_t workspace_bytes,
                      sivae_stream_t stream);

/* ---- pooling / upsampling / ReLU --------------------------------------------------------------------
 * nn.AvgPool2d(2) :92,:98 (floor semantics for odd sizes); nn.Upsample(scale_factor=2, 'nearest') :155;
 * nn.ReLU(True) :147. rows = B*C. */
int sivae_avgpool2_fwd(const float* x, float* y, int rows, int Hin, int Win, sivae_stream_t stream);
int sivae_avgpool2_bwd(const float* dy, float* dx, int rows, int Hin, int Win, sivae_stream_t stream);
int sivae_upsample2_fwd(const float* x, float* y, int rows, int H, int W, sivae_stream_t stream);
int sivae_upsample2_bwd(const float* dy, float* dx, int rows, int H, int W, sivae_stream_t stream);
int sivae_relu_fwd(const float* x, float* y, size_t n, sivae_stream_t stream);
int sivae_relu_bwd(const float* dy, const float* y, float* dx, size_t n, sivae_stream_t stream);
int sivae_add_inplace(float* y, const float* x, size_t n, sivae_stream_t stream);

/* ---- sampler and losses -------------------------------------------------------------------------------
 * reparameterize :254-265 ; calc_kl :231-251 ; calc_reconstruction_loss :268-294 ; expELBO :580-581.
 * mu / logvar are [B][Z] with leading dimension ld (the two halves of the encoder fc output). */
int sivae_reparam_fwd(const float* mu, const float* logvar, int ld, const float* eps, float* z, int B, int Z,
                      sivae_stream_t stream);
int sivae_reparam_bwd(const float* dz, const float* logvar, int ld, const float* eps, float* dmu, float* dlogvar,
                      int ldg, int B, int Z, sivae_stream_t stream);
int sivae_kl_fwd(const float* logvar, const float* mu, int ld, float mu_o, float logvar_o, float* out /*[B]*/,
                 int B, int Z, sivae_stream_t stream);
int sivae_kl_bwd(const float* g, int g_per_sample, float g_scale, const float* logvar, const float* mu, int ld,
                 float mu_o, float logvar_o, float* dlogvar, float* dmu, int ldg, int B, int Z,
                 sivae_stream_t stream);
/* the same with TENSOR priors (calc_kl's mu_o / logvar_o may be tensors, :237-243): device pointers read through
 * broadcast strides in elements (row stride, column stride; 0 = broadcast), i.e. 0-d, [Z], [1][Z], [B][1] or [B][Z]
 * priors without a host round trip.  Gradients are those with respect to logvar / mu. */
int sivae_kl_fwd_t(const float* logvar, const float* mu, int ld, const float* mu_o, int mu_o_rs, int mu_o_cs,
                   const float* logvar_o, int lv_o_rs, int lv_o_cs, float* out /*[B]*/, int B, int Z,
                   sivae_stream_t stream);
int sivae_kl_bwd_t(const float* g, int g_per_sample, float g_scale, const float* logvar, const float* mu, int ld,
                   const float* mu_o, int mu_o_rs, int mu_o_cs, const float* logvar_o, int lv_o_rs, int lv_o_cs,
                   float* dlogvar, float* dmu, int ldg, int B, int Z, sivae_stream_t stream);
/* loss_type: 0 mse, 1 l1, 2 bce.  rowsum: out[b] = sum_i term(x[b,i], recon[b,i]). */
size_t sivae_recon_workspace_bytes(int B, int D);
int sivae_recon_rowsum_fwd(const float* x, const float* recon, int loss_type, float* out, int B, int D,
                           void* workspace, size_t workspace_bytes, sivae_stream_t stream);
/* g_mode 0: g[B] per sample, 1: scalar g[0], 2: per element g[B*D]; effective grad = g * g_scale. */
int sivae_recon_bwd(const float* x, const float* recon, int loss_type, const float* g, int g_mode, float g_scale,
                    float* d_recon, float* d_x, int B, int D, sivae_stream_t stream);
int sivae_recon_elem_fwd(const float* x, const float* recon, int loss_type, float* out, size_t numel,
                         sivae_stream_t stream);
int sivae_vec_sum(const float* v, int n, float scale, float* out, sivae_stream_t stream);
/* e[b] = exp(-2*scale*(beta_rec*L[b] + beta_neg*KL[b])), out[0] = mean_b e[b]. */
int sivae_expelbo_fwd(const float* L, const float* KL, float scale, float beta_rec, float beta_neg, int B,
                      float* e, float* out, sivae_stream_t stream);
int sivae_expelbo_bwd(const float* gout, const float* e, float scale, float beta_rec, float beta_neg, int B,
                      float* dL, float* dKL, sivae_stream_t stream);
/* Weighted sum of up to six device scalars in one launch, terms added in index order: out[0] = sum_i w_i * p_i[0], i < n.
 * Replaces the 0-dim torch arithmetic of lossE / lossD (train_soft_intro_vae.py:583-586, :618-620). */
int sivae_lincomb(const float* p0, const float* p1, const float* p2, const float* p3, const float* p4, const float* p5,
                  float w0, float w1, float w2, float w3, float w4, float w5, int n, float* out, sivae_stream_t stream);
/* its gradient: out[i] = g[0] * w_i, i < n. */
int sivae_lincomb_bwd(const float* g, float w0, float w1, float w2, float w3, float w4, float w5, int n, float* out,
                      sivae_stream_t stream);
/* Philox4x32-10 standard normals (replaces torch.randn / randn_like :264,:547 in fast mode). */
int sivae_randn(float* out, size_t n, unsigned long long seed, unsigned long long offset, sivae_stream_t stream);
/* same stream with its position kept in device memory (*offset_dev is read, then advanced by ceil(n/4)): nothing
 * that a captured HIP graph bakes in changes between replays. */
int sivae_randn_dev(float* out, size_t n, unsigned long long seed, unsigned long long* offset_dev,
                    sivae_stream_t stream);

/* ---- optimizer ------------------------------------------------------------------------------------------
 * torch.optim.Adam(lr, betas=(0.9,0.999), eps=1e-8) :450-451, one launch over a flat parameter buffer. */
int sivae_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                    float step_size /* lr / (1 - beta1^t) */, float beta1, float beta2, float eps,
                    float bias_correction2_sqrt /* sqrt(1 - beta2^t) */, float grad_scale,
                    sivae_stream_t stream);

/* the same Adam step with its state on the device (for whole-iteration HIP graphs): state = double[4]
 * {t, lr, lr/(1-beta1^t), sqrt(1-beta2^t)}; the call advances t and refreshes the two factors before the update. */
int sivae_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double* state,
                        double beta1, double beta2, float eps, float grad_scale, sivae_stream_t stream);

/* grad[i] += s0[i] + s1[i] + s2[i] + s3[i] (s1 .. s3 may be NULL): folds the per-use parameter-gradient slabs of one backward pass
 * into the flat gradient buffer — the reference's `loss.backward()` accumulation `p.grad += g` (:571, :619) for
 * parameters used by several passes, as ONE launch per network instead of one torch add per tensor and use. */
int sivae_sum_slabs(float* grad, const float* s0, const float* s1, const float* s2, const float* s3, size_t n,
                    sivae_stream_t stream);

/* ---- input side ------------------------------------------------------------------------------
 * uint8 image batch [B][C][H][W] (nhwc == 0) or [B][H][W][C] (nhwc != 0) -> fp32 NCHW * scale, sample b mirrored
 * horizontally when flip[b] != 0 (flip may be NULL): the reference's random mirror + transforms.ToTensor()
 * (dataset.py:27-28,46,68-70; train_soft_intro_vae.py:379) done on the device, on the prefetch stream. */
int sivae_u8_to_f32(const unsigned char* src, float* dst, const int* flip, int B, int C, int H, int W, int nhwc,
                    float scale, sivae_stream_t stream);

/* ---- output side -----------------------------------------------------------------------------
 * generated images fp32 -> uint8 with the reference's quantisation for the FID network
 * (metrics/fid_score.py:247-249: np.clip(images * 255, 0, 255).astype(np.uint8)): dst = trunc(clamp(src*scale, 0, 255)).
 * src and dst 16-byte aligned. */
int sivae_f32_to_u8(const float* src, unsigned char* dst, size_t numel, float scale, sivae_stream_t stream);

/* ---- nn.Linear (Encoder.fc :109,:121 / Decoder.fc :146,:166) as small-M GEMMs -------------------------------------
 * x [B][K], W [N][K] (nn.Linear.weight), y [B][N], all fp32 row-major; B <= 256, K % 4 == 0, N % 4 == 0
 * (sivae_linear_supported; other shapes run as 1x1 convolutions through sivae_conv2d_fwd / _wgrad).
 * One wave per 32 output columns x a slice of the contraction (~1000 waves per call instead of cdiv(N,128) blocks),
 * fixed-order reduction of the slices -> deterministic.  relu != 0 fuses the nn.ReLU after Decoder.fc (:147). */
int sivae_linear_supported(int B, int K, int N);
size_t sivae_linear_workspace_bytes(int B, int K, int N);
int sivae_linear_fwd(const float* x, const float* w, const float* bias, float* y, int relu, int B, int K, int N,
                     void* workspace, size_t workspace_bytes, sivae_stream_t stream);
int sivae_linear_dgrad(const float* dy, const float* w, float* dx, int B, int K, int N, void* workspace,
                       size_t workspace_bytes, sivae_stream_t stream);
int sivae_linear_wgrad(const float* dy, const float* x, float* dw, int B, int K, int N, sivae_stream_t stream);

/* ---- bf16 mode (config 3 of BASELINE.json: "CelebA 128x128 ... bf16") -----------------------------------------
 * The reference trains in fp32 only (soft_intro_vae/train_soft_intro_vae.py:376-440 has no autocast / GradScaler), so
 * this mode is build-defined: activations and activation gradients are stored in bf16, the convolutions run on
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation, BatchNorm statistics / parameter gradients / master weights / Adam
 * stay fp32, the loss kernels above stay fp32 (Decoder.predict writes fp32 NCHW).
 * Activation layout ("blocked NCHW"): x[b][c/8][h][w][c%8] bf16, channel count padded to a multiple of 16 with zeros
 * (sivae_bf16_cblocks(C) 8-channel blocks).  Same nn.Conv2d / nn.BatchNorm2d / nn.LeakyReLU / nn.AvgPool2d /
 * nn.Upsample call sites as the fp32 entry points above (:51-75, :88-99, :153-159). */
int sivae_bf16_cblocks(int C);
/* fp32 NCHW <-> blocked bf16 (padded channels written as 0; `scale` multiplies on the way in) */
int sivae_bf16_from_f32_nchw(const float* src, void* dst, int B, int C, int H, int W, float scale,
                             sivae_stream_t stream);
int sivae_bf16_to_f32_nchw(const void* src, float* dst, int B, int C, int H, int W, sivae_stream_t stream);
/* kw-packed form of the RGB-side 5x5 layers (Encoder stem train_soft_intro_vae.py:88, Decoder.predict :159; C <= 3):
 * the 5 kernel columns move into the channel dimension, so the 5x5 conv over / into C channels runs as a 5-tap conv
 * (ks code 51 of the conv / weight-gradient entry points: 5 rows x 1 column) over / into 5C <= 15 channels.
 *   im2col: dst (blocked bf16, 16 channels) [kw*C + c][h][w] = src (fp32 NCHW) [c][h][w + sgn*(kw-2)], 0 outside
 *   fold:   dst (fp32 NCHW, C channels) [c][h][w] = bias[c] + sum_kw g (fp32 NCHW, 5C channels) [kw*C + c][h][w + sgn*(kw-2)]
 * sgn = +1 / -1.  (stem: im2col +1 of the image, fold -1 for its input gradient; predict: fold +1 for its output,
 * im2col -1 of its output gradient.) */
int sivae_bf16_im2col_kw5(const float* src, void* dst, int B, int C, int H, int W, int sgn, sivae_stream_t stream);
int sivae_bf16_fold_kw5(const float* g, const float* bias, float* dst, int B, int C, int H, int W, int sgn,
                        sivae_stream_t stream);
/* fp32 master weight [Co][Ci][ks][ks] -> bf16 MFMA-operand slabs; mode 0 forward, mode 1 data gradient.
 * ks is 1, 3, 5 or the code 51 = 5 rows x 1 column (weight [Co][Ci][5][1]) in all bf16 conv entry points */
size_t sivae_bf16_pack_conv_weight_bytes(int Co, int Ci, int ks, int mode);
int sivae_bf16_pack_conv_weight(const float* w, void* wp, int Co, int Ci, int ks, int mode, sivae_stream_t stream);
/* y (+)= conv(x', wp) + bias with the fusions of sivae_conv2d_fwd (producer BatchNorm+LeakyReLU prologue — 3x3 only —,
 * upsample addressing, {sum, sumsq} partials of the rounded output, accumulate).  out_f32_nchw != 0: y is float
 * [B][Co][H][W] (Co <= 32, no stats: Decoder.predict :159).  stats_partial has sivae_bf16_conv2d_num_px_tiles(B, Co, H, W, ks) rows and
 * feeds sivae_bn_stats_from_conv_ws unchanged.  The data gradient is this function on dy with the mode-1 pack. */
int sivae_bf16_conv2d_num_px_tiles(int B, int Co, int H, int W, int ks);
int sivae_bf16_conv2d_fwd(const void* x, const void* wp, void* y, const float* bias, const float* pro_mean,
                          const float* pro_invstd, const float* pro_gamma, const float* pro_beta, float pro_slope,
                          float* stats_partial, int B, int Ci, int Co, int H, int W, int ks, int upsample,
                          int accumulate, int out_f32_nchw, sivae_stream_t stream);
/* split-K form for small grids (the 512-channel 8x8 / 4x4 layers: 64-256 blocks each walking 32 chunks): the
 * input-channel range is cut into sivae_bf16_conv2d_splitk(...) slices (1: not split) written as fp32 partials into
 * `workspace` and summed in a fixed order by a reduce kernel that rounds to bf16 and leaves per-image {sum, sumsq} rows
 * (stats_partial has sivae_bf16_conv2d_splitk_stats_rows(...) rows).  3x3, no bias, bf16 output only. */
int sivae_bf16_conv2d_splitk(int B, int Ci, int Co, int H, int W, int ks);
size_t sivae_bf16_conv2d_splitk_workspace_bytes(int B, int Ci, int Co, int H, int W, int ks);
int sivae_bf16_conv2d_splitk_stats_rows(int B, int Ci, int Co, int H, int W, int ks);
int sivae_bf16_conv2d_fwd_splitk(const void* x, const void* wp, void* y, const float* pro_mean,
                                 const float* pro_invstd, const float* pro_gamma, const float* pro_beta, float pro_slope,
                                 float* stats_partial, int B, int Ci, int Co, int H, int W, int ks, int upsample,
                                 int accumulate, void* workspace, size_t workspace_bytes, sivae_stream_t stream);
/* y_half [B][Co][H/2][W/2] (blocked bf16) (+)= the 2x2 block sums of conv3x3(x): the data gradient of a 3x3 conv that read
 * its input through nearest-2x upsample addressing, the adjoint of the nn.Upsample (train_soft_intro_vae.py:155) folded
 * into the epilogue (four fp32 accumulators summed, one rounding; the full-resolution gradient is never written).  wp: the
 * mode-1 pack; H, W even; never split-K (the caller keeps the two-launch form where sivae_bf16_conv2d_splitk(...) > 1). */
int sivae_bf16_conv2d_fwd_pool(const void* x, const void* wp, void* y_half, int B, int Ci, int Co, int H, int W,
                               int accumulate, sivae_stream_t stream);
/* dw [Co][Ci][ks][ks] fp32 = weight gradient (aten::convolution_backward, weight half); x' as above (prologue 3x3
 * only, upsample addressing); deterministic two-pass reduction over pixel slices */
size_t sivae_bf16_conv2d_wgrad_workspace_bytes(int B, int Ci, int Co, int H, int W, int ks);
int sivae_bf16_conv2d_wgrad(const void* x, const void* dy, float* dw, const float* pro_mean, const float* pro_invstd,
                            const float* pro_gamma, const float* pro_beta, float pro_slope, int B, int Ci, int Co,
                            int H, int W, int ks, int upsample, void* workspace, size_t workspace_bytes,
                            sivae_stream_t stream);
/* y = LeakyReLU((x-mean)*invstd*gamma+beta + res): res NULL, same shape, or (res_up) [B][C][H/2][W/2] read through
 * nearest-2x addressing; y and/or y_pool = AvgPool2d(2)(y) are written (either may be NULL, not both).  sign_mask (may be
 * NULL): sivae_bf16_bn_signmask_bytes(...) bytes, one per 8-channel pixel vector, bit e = (output e > 0) — the backward
 * reads it (1/16 of the tensor) instead of the saved output, and a pooled block need not write its full-resolution y. */
size_t sivae_bf16_bn_signmask_bytes(int B, int C, int H, int W);
int sivae_bf16_bn_apply_act(const void* x, const void* res, int res_up, const float* mean, const float* invstd,
                            const float* gamma, const float* beta, float slope, void* y, void* y_pool,
                            unsigned char* sign_mask, int B, int C, int H, int W, sivae_stream_t stream);
/* backward of the above: dy (or, dy_pooled, the gradient of y_pool); activation sign from sign_mask, else from y, else —
 * both NULL — recomputed from x (no residual; needs beta); dx, dz = gradient of the residual branch (NULL to skip;
 * dz_sum: its 2x2 block sums [B][C][H/2][W/2]), dgamma / dbeta (NULL to skip) */
size_t sivae_bf16_bn_bwd_workspace_bytes(int B, int C, int H, int W);
int sivae_bf16_bn_bwd(const void* dy, int dy_pooled, const void* y, const unsigned char* sign_mask, const void* x,
                      const float* mean, const float* invstd, const float* gamma, const float* beta, float slope,
                      void* dx, void* dz, int dz_sum, float* dgamma, float* dbeta, int B, int C, int H, int W,
                      void* workspace, size_t workspace_bytes, sivae_stream_t stream);
/* The same backward as ONE launch that reads dy and x once (bf16_bn_fused.hip, round 4; the bf16 counterpart of
 * sivae_bn_bwd_fused): raw vectors held in registers across a grid barrier, or a barrier-free launch where a channel
 * block's plane set fits one block.  Power-of-two maps (sivae_bf16_bn_bwd_fused_supported); `state` = the barrier state
 * of sivae_bn_bwd_fused (sivae_bn_bwd_fused_state_uints() unsigned ints, zeroed once, one buffer per stream). */
int sivae_bf16_bn_bwd_fused_supported(int B, int C, int H, int W);
size_t sivae_bf16_bn_bwd_fused_workspace_bytes(int B, int C, int H, int W);
int sivae_bf16_bn_bwd_fused(const void* dy, int dy_pooled, const void* y, const unsigned char* sign_mask, const void* x,
                            const float* mean, const float* invstd, const float* gamma, const float* beta, float slope,
                            void* dx, void* dz, int dz_sum, float* dgamma, float* dbeta, int B, int C, int H, int W,
                            unsigned int* state, void* workspace, size_t workspace_bytes, sivae_stream_t stream);
/* SEGMENTED batches of the bf16 mode (see "segmented batches" below: B = nseg * seg_images images laid end to end, mean /
 * invstd [nseg][C], gamma / beta [C], dgamma / dbeta summed over the passes in pass order).  The bf16 convolutions have
 * no BatchNorm prologue in the default configuration (functional16.MATERIALIZE_H), their statistics rows are in image
 * order, and the weight gradients sum over the whole batch — so the two BatchNorm kernels are all that needs a _seg form
 * for the pass pairs of train_soft_intro_vae.py:567-568, :601-608 to run as one launch per layer.  seg_images == B is the
 * plain form (the entry points above forward to these). */
int sivae_bf16_bn_apply_act_seg(const void* x, const void* res, int res_up, const float* mean, const float* invstd,
                                const float* gamma, const float* beta, float slope, void* y, void* y_pool,
                                unsigned char* sign_mask, int B, int C, int H, int W, int seg_images,
                                sivae_stream_t stream);
int sivae_bf16_bn_bwd_fused_seg_supported(int B, int C, int H, int W, int seg_images);
size_t sivae_bf16_bn_bwd_fused_seg_workspace_bytes(int B, int C, int H, int W, int seg_images);
int sivae_bf16_bn_bwd_fused_seg(const void* dy, int dy_pooled, const void* y, const unsigned char* sign_mask,
                                const void* x, const float* mean, const float* invstd, const float* gamma,
                                const float* beta, float slope, void* dx, void* dz, int dz_sum, float* dgamma,
                                float* dbeta, int B, int C, int H, int W, int seg_images, unsigned int* state,
                                void* workspace, size_t workspace_bytes, sivae_stream_t stream);
int sivae_bf16_upsample2_fwd(const void* x, void* y, int B, int C, int Hs, int Ws, sivae_stream_t stream);
int sivae_bf16_upsample2_bwd(const void* dy, void* dx, int B, int C, int Hs, int Ws, sivae_stream_t stream);
int sivae_bf16_add_inplace(void* y, const void* x, size_t nvec, sivae_stream_t stream);

/* ---- segmented batches: several passes of a network through the SAME weights as one launch ---------
 * The reference's iteration runs pairs of independent passes through unchanged weights — model(rec.detach()) /
 * model(fake.detach()) train_soft_intro_vae.py:567-568, encode(rec) / encode(fake) :601-605, decode(z_rec) /
 * decode(z_fake) :607-608, bootstrap decode_target x2 soft_intro_vae_bootstrap/train_soft_intro_vae_bootstrap.py:635-636.
 * The engine lays such passes end to end in ONE batch of B = nseg * seg_images images ("segments", pass g = images
 * [g*seg_images, (g+1)*seg_images)).  Convolutions do not care; training-mode nn.BatchNorm2d (:58,:62,:90) must keep
 * ONE set of batch statistics PER PASS, so the BatchNorm entry points below take `seg_images` (or `nseg`) and every fused
 * BatchNorm prologue has a _seg form: mean / invstd are [nseg][C], gamma / beta / running buffers [C]; dgamma / dbeta are
 * summed over the passes; the running buffers receive one momentum update per pass in pass order.  seg_images == B
 * (nseg = 1) is the unsegmented op, bit for bit: there is no other fp32 entry point for it. */
/* statistics from the conv epilogue's partials ([n_tiles][C][2] rows in image order, n_tiles % nseg == 0), one-stage */
int sivae_bn_stats_from_conv_seg(const float* partials, int n_tiles, int nseg, int seg_rev, int B_seg, int C, int HW,
                                 float eps, float momentum, float* running_mean, float* running_var,
                                 long long* num_batches_tracked, float* mean_out, float* invstd_out,
                                 sivae_stream_t stream);
/* one more running-stat update per pass from saved batch statistics (a forward pass replayed from cached
 * activations still counts as one BatchNorm call of the reference); count = seg_images*H*W; seg_rev: last pass first. */
int sivae_bn_update_running_seg(const float* mean, const float* invstd, int nseg, int seg_rev, int C, double count,
                                float eps, float momentum, float* running_mean, float* running_var,
                                long long* num_batches_tracked, sivae_stream_t stream);
/* sivae_bn_stats_from_conv_seg with a scratch buffer: from 2048 partial rows per pass on (the 256x256 / 128x128 layers at
 * batch 128) the rows are folded in two coalesced stages instead of one strided walk per channel; same statistics, same
 * running-buffer updates (nn.BatchNorm2d training-mode forward, train_soft_intro_vae.py:57,62,90).  The workspace size is 0
 * (and the pointer may be NULL) where the one-stage form is used. */
size_t sivae_bn_stats_from_conv_workspace_bytes(int n_tiles, int nseg, int C);
int sivae_bn_stats_from_conv_ws(const float* partials, int n_tiles, int nseg, int seg_rev, int B_seg, int C, int HW,
                                float eps, float momentum, float* running_mean, float* running_var,
                                long long* num_batches_tracked, float* mean_out, float* invstd_out, void* workspace,
                                size_t workspace_bytes, sivae_stream_t stream);
/* y = LeakyReLU((x-mean[c])*invstd[c]*gamma[c]+beta[c] (+ res), slope); slope = 1 -> identity act; res may be NULL.
 *   y_pooled != NULL: also writes AvgPool2d(2) (:92,:98) of the result in the same pass: y [B][C][H][W] (kept for
 *     backward) and y_pooled [B][C][H/2][W/2]; y may be NULL with y_pooled (pooled output only: the stem, whose backward
 *     recomputes the activation from the conv output); H even, W % 4 == 0; not with res_up.
 *   res_up != 0: res is stored at half resolution [B][C][H/2][W/2] and read through nn.Upsample(2,'nearest') (:155)
 *     addressing — the upsampled tensor is never written; H even, W % 4 == 0.
 *   otherwise H and W count only as H * W (a [B][C] input goes as H = 1, W = 1). */
int sivae_bn_apply_act_seg(const float* x, const float* res, int res_up, const float* mean, const float* invstd,
                           const float* gamma, const float* beta, float slope, float* y, float* y_pooled, int B, int C,
                           int H, int W, int seg_images, sivae_stream_t stream);
/* The same op with the LeakyReLU sign mask as an extra output (1 bit per element: pre-activation > 0; element e -> bit
 * e&7 of byte e>>3).  The apply pass of "LeakyReLU(BN(x) + res)" (ResidualBlock output, train_soft_intro_vae.py:71-74)
 * writes it next to its output and the backward reads it instead of the saved output: 1/32 of a tensor per backward pass,
 * and an encoder block (output consumed only through the AvgPool2d behind it, :95-99) never writes its full-resolution
 * output.  y_pooled, res_up as above.  mask: sivae_bn_signmask_bytes() bytes.  H even, W % 8 == 0. */
size_t sivae_bn_signmask_bytes(int B, int C, int HW);
int sivae_bn_apply_act_signmask_seg(const float* x, const float* res, int res_up, const float* mean,
                                    const float* invstd, const float* gamma, const float* beta, float slope, float* y,
                                    float* y_pooled, unsigned char* mask, int B, int C, int H, int W, int seg_images,
                                    sivae_stream_t stream);
/* backward of the above, every variant in one entry: dz = dy*(s>0?1:slope); dx = BN backward of dz; dz_out (optional) =
 * gradient of the residual branch; dgamma/dbeta optional.  act_mode selects where the LeakyReLU sign s comes from:
 *   0 no activation, 1 the saved OUTPUT y (valid since slope > 0), 2 recomputed from x (needs beta; used when the
 *   BatchNorm output was never stored because it was fused into the next conv's load), 3 the sign mask the apply pass
 *   wrote (y may be NULL; H even, W % 8 == 0).
 * dy_pooled != 0: dy is the gradient of AvgPool2d(2)(output) at half resolution [B][C][H/2][W/2] (:92,:98); the pool's
 *   adjoint (0.25 * dy_half[h>>1][w>>1]) is applied on load.  dz_sum != 0 (act_mode 1 or 3): dz_out = 2x2 block sums of the
 *   residual-branch gradient [B][C][H/2][W/2] — the adjoint of the nn.Upsample (:155) in front of a decoder block —
 *   instead of the full-resolution dz.  Either: H even, W % 4 == 0; not both.  Without them H and W count only as H * W.
 * workspace: sivae_bn_workspace_bytes(seg_images, nseg * C, H * W).
 * counters: NULL, or >= C zero-initialised unsigned ints the call leaves zero (caller-owned, one stream at a time): the
 * per-channel finalize then runs inside the reduction kernel instead of as its own launch — same fixed summation order */
int sivae_bn_bwd_seg(const float* dy, const float* y, const unsigned char* mask, const float* x, const float* mean,
                     const float* invstd, const float* gamma, const float* beta, int act_mode, float slope, float* dx,
                     float* dz_out, float* dgamma, float* dbeta, int B, int C, int H, int W, int dy_pooled, int dz_sum,
                     int seg_images, unsigned int* counters, void* workspace, size_t workspace_bytes,
                     sivae_stream_t stream);
/* The same backward as ONE persistent launch that reads dy and x once and writes dx once (bn_fused.hip, round 4): the
 * chip's register files hold the activations between the reduction phase and the dx phase, (segment, channel) plane sets are
 * walked in groups separated by a grid barrier, per-channel sums are folded in a fixed order (deterministic).  Replaces
 * the backward of nn.BatchNorm2d + nn.LeakyReLU (+ torch.add) of train_soft_intro_vae.py:57-63,71-74,90-91 like
 * sivae_bn_bwd_seg, with the same argument meaning.  `state`: sivae_bn_bwd_fused_state_uints() unsigned ints, zeroed ONCE
 * by the caller and then left consistent by every call (one buffer per stream).  Power-of-two maps only
 * (sivae_bn_bwd_fused_supported); the grid (2 blocks per CU) must be fully resident: not to be run concurrently with
 * another persistent kernel on the device. */
int sivae_bn_bwd_fused_supported(int B, int C, int H, int W, int seg_images);
size_t sivae_bn_bwd_fused_workspace_bytes(int B, int C, int H, int W, int seg_images);
int sivae_bn_bwd_fused_state_uints(void);
/* Grid-barrier timeout (round 5): a persistent launch whose grid is not fully resident no longer traps — after
 * SIVAE_BN_FUSED_SPIN_LIMIT polls (default 2^24, tens of seconds) the waiting block sets word
 * sivae_bn_bwd_fused_poison_word() of `state` and every block leaves the kernel (that launch's outputs are garbage, later
 * launches on the same state return at once).  The host reads that word where it reads results back anyway, raises, and
 * zeroes the whole state (sivae_hip.ops.bn_fused_check).  Plans also refuse the persistent form under a CU mask
 * (HSA_CU_MASK / ROC_GLOBAL_CU_MASK), with SIVAE_BN_FUSED_PERSISTENT=0, or when the runtime reports fewer than two
 * resident blocks per CU: sivae_bn_bwd_fused_supported() then returns 0 for plane sets that need the barrier and the
 * callers keep the three-launch form.  (The timeout path is exercised without a hook in this library: the test
 * corrupts the caller-owned `state` so that the arrivals never add up and shortens the spin limit for that call; the
 * resource-holding "squatter" kernel of the co-residency tests lives in tests/support/, not here.) */
int sivae_bn_bwd_fused_poison_word(void);
int sivae_bn_bwd_fused(const float* dy, const float* y, const unsigned char* mask, const float* x, const float* mean,
                       const float* invstd, const float* gamma, const float* beta, int act_mode, float slope, float* dx,
                       float* dz_out, float* dgamma, float* dbeta, int B, int C, int H, int W, int dy_pooled, int dz_sum,
                       int seg_images, unsigned int* state, void* workspace, size_t workspace_bytes,
                       sivae_stream_t stream);
/* Winograd 3x3 forward / data gradient and weight gradient with a segmented BatchNorm prologue (pro_* may be NULL: then
 * only the row order of stats_partial matters — image order, so rows [g*n/nseg, (g+1)*n/nseg) are pass g).  On 8x8 /
 * 4x4 maps seg_images must be a multiple of 2 / 4 (a tile block holds that many images). */
int sivae_conv2d_wino_fwd_seg(const float* x, const float* up, float* y, const float* pro_mean,
                              const float* pro_invstd, const float* pro_gamma, const float* pro_beta, float pro_slope,
                              float* stats_partial, int B, int Ci, int Co, int H, int W, int upsample, int accumulate,
                              int seg_images, sivae_stream_t stream);
int sivae_conv2d_wino_fwd_splitk_seg(const float* x, const float* up, float* y, const float* pro_mean,
                                     const float* pro_invstd, const float* pro_gamma, const float* pro_beta,
                                     float pro_slope, float* stats_partial, int B, int Ci, int Co, int H, int W,
                                     int upsample, int accumulate, int seg_images, void* workspace,
                                     size_t workspace_bytes, sivae_stream_t stream);
int sivae_conv2d_wino_wgrad_seg(const float* x, const float* dy, float* dw, const float* pro_mean,
                                const float* pro_invstd, const float* pro_gamma, const float* pro_beta, float pro_slope,
                                int B, int Ci, int Co, int H, int W, int upsample, int seg_images, void* workspace,
                                size_t workspace_bytes, sivae_stream_t stream);

/* ---- Winograd F(4x4,3x3) for the large-map 3x3 convs (nn.Conv2d k=3, train_soft_intro_vae.py:56-61) ----
 * 36 multiplies per 4x4 output tile: 1.78x fewer matrix-pipe passes than F(2x2,3x3) (sivae_conv2d_wino_fwd) at 1.2e-5
 * relative error per layer in fp32 (3.3e-5 on the reconstruction of the six-level network end to end).  Maps: H % 16 == 0,
 * W % 32 == 0.  up: [6][Ci_pad][Co_pad][6] from sivae_pack_wino4_weight (mode 0 forward, 1 data gradient).
 * stats_partial: [sivae_conv2d_wino4_num_px_tiles][Co][2] rows in image order (sivae_bn_stats_from_conv_ws / _seg). */
size_t sivae_pack_wino4_weight_bytes(int Co, int Ci, int mode);
int sivae_pack_wino4_weight(const float* w, float* up, int Co, int Ci, int mode, sivae_stream_t stream);
int sivae_conv2d_wino4_supported(int H, int W); /* 1: H % 16 == 0, W % 32 == 0; 2 / 3 / 4: 16 x 16 / 8 x 8 / 4 x 4 maps — a
                                                     work item (32 x 16 pixels) is a grid of 2 x 1 / 4 x 2 / 8 x 4 whole
                                                     images (round 6: the 8 x 8 and 4 x 4 maps of the deep 512-channel
                                                     blocks, res_in_8 / res_in_4 of train_soft_intro_vae.py:100-103,
                                                     153-158), every seam zero padding: B and seg_images must be multiples
                                                     of sivae_conv2d_wino4_images_per_item; stats rows per item; 0 otherwise */
int sivae_conv2d_wino4_images_per_item(int H, int W); /* 1, 2, 8, 32 for modes 1..4; 0: unsupported map */
/* Round 6: the data gradient of conv3x3(Upsample2(x)) with respect to the low-resolution x (conv1 behind nn.Upsample,
 * train_soft_intro_vae.py:155,56) in one F(4x4,3x3) pass: dx[B][N][H/2][W/2] (+)= the 2x2 block sums of conv3x3^T(dy[B][C][H][W]),
 * the block sum folded into the output transform.  up: sivae_pack_wino4_weight(w[C][N][3][3], mode 1).  H % 16 == 0, W % 32 == 0.
 * `_pays`: N <= 64 and a work item for every CU (there the phase-folded sivae_conv2d_wino_up_dgrad splits K over wave pairs). */
int sivae_conv2d_wino4_dgrad_pool_pays(int B, int C, int N, int H, int W);
int sivae_conv2d_wino4_dgrad_pool(const float* dy, const float* up, float* dx, int B, int C, int N, int H, int W,
                                  int accumulate, sivae_stream_t stream);
/* modes 3 / 4 only: 1 when the image-grid launch (with its split-K plan) is expected to beat F(2x2,3x3) — enough
 * (slices x items) for every CU and a long enough K slice (measured: profiles/r6_wino4_small_maps_vs_f23.txt) */
int sivae_conv2d_wino4_small_pays(int B, int Ci, int Co, int H, int W);
int sivae_conv2d_wino4_pays(int B, int Ci, int Co, int H, int W); /* supported AND >= one work item per CU */
int sivae_conv2d_wino4_num_px_tiles(int B, int H, int W);
int sivae_conv2d_wino4_fwd(const float* x, const float* up, float* y, float* stats_partial, int B, int Ci, int Co, int H,
                           int W, int accumulate, sivae_stream_t stream);
/* the same with the producer BatchNorm2d + LeakyReLU fused into the input read (:58-59; pro_* as in sivae_conv2d_fwd);
 * seg_images > 0: segmented batch with pro_mean / pro_invstd [B / seg_images][Ci]; segments * padded Ci <= 1024 */
int sivae_conv2d_wino4_fwd_pro(const float* x, const float* up, float* y, const float* pro_mean, const float* pro_invstd,
                               const float* pro_gamma, const float* pro_beta, float pro_slope, float* stats_partial,
                               int B, int Ci, int Co, int H, int W, int accumulate, int seg_images,
                               sivae_stream_t stream);

/* split-K form of the F(4x4,3x3) forward / data gradient for launches with fewer work items than CUs (the deep layers of
 * the per-GPU shards): sivae_conv2d_wino4_splitk -> number of K slices S (1 = the plain kernel); for S > 1 the partial
 * outputs go through `workspace` ([S][B][Co][H][W]), are summed in a fixed order, and stats_partial is [B][Co][2] (per
 * image) instead of per pixel tile.  pro_mean may be NULL (no prologue); seg_images as in sivae_conv2d_wino4_fwd_pro. */
int sivae_conv2d_wino4_splitk(int B, int Ci, int Co, int H, int W);
size_t sivae_conv2d_wino4_splitk_workspace_bytes(int B, int Ci, int Co, int H, int W);
int sivae_conv2d_wino4_fwd_splitk(const float* x, const float* up, float* y, const float* pro_mean, const float* pro_invstd,
                                  const float* pro_gamma, const float* pro_beta, float pro_slope, float* stats_partial, int B,
                                  int Ci, int Co, int H, int W, int accumulate, int seg_images, void* workspace,
                                  size_t workspace_bytes, sivae_stream_t stream);

/* The same F(4x4,3x3) forward / data gradient with its 36 frequency GEMMs on the BF16 matrix pipe and FP32-EXACT products
 * (conv_wino4_b6.hip, round 5): every fp32 operand is split into three bf16 pieces by truncation (exact), a product is the
 * fp32 sum of six of the nine piece products (the dropped terms are <= 2^-24 of it) — the accuracy of v_mfma_f32_32x32x2_f32
 * (profiles/r4_probe_bf16x6_accuracy.txt), at 1/2.7 of its matrix cycles.  Replaces the same nn.Conv2d(k=3, s=1, p=1)
 * (soft_intro_vae/train_soft_intro_vae.py:56-61) with the same argument meaning as sivae_conv2d_wino4_fwd_pro /
 * sivae_conv2d_wino4_fwd_splitk (pro_mean may be NULL; no limit on segments x channels: the prologue parameters are read
 * through scalar loads); `up` = the pre-split operand of sivae_pack_wino4_b6_weight ([j][Ci_pad/16][Co_pad/32][i][piece]
 * blocks of 64 lanes x 8 bf16, 1.5x the bytes of the fp32 pack); maps: modes 1 and 2 of sivae_conv2d_wino4_supported; the split-K plan
 * and workspace are those of sivae_conv2d_wino4_splitk / _splitk_workspace_bytes. */
size_t sivae_pack_wino4_b6_weight_bytes(int Co, int Ci, int mode);
int sivae_pack_wino4_b6_weight(const float* w, void* up, int Co, int Ci, int mode, sivae_stream_t stream);
int sivae_conv2d_wino4_b6_fwd(const float* x, const void* up, float* y, const float* pro_mean, const float* pro_invstd,
                              const float* pro_gamma, const float* pro_beta, float pro_slope, float* stats_partial, int B,
                              int Ci, int Co, int H, int W, int accumulate, int seg_images, sivae_stream_t stream);
int sivae_conv2d_wino4_b6_fwd_splitk(const float* x, const void* up, float* y, const float* pro_mean,
                                     const float* pro_invstd, const float* pro_gamma, const float* pro_beta,
                                     float pro_slope, float* stats_partial, int B, int Ci, int Co, int H, int W,
                                     int accumulate, int seg_images, void* workspace, size_t workspace_bytes,
                                     sivae_stream_t stream);

/* Winograd F(4x4,3x3) weight gradient (conv_wino4_wgrad.hip) — the weight half of aten::convolution_backward of the
 * nn.Conv2d(k=3) layers (soft_intro_vae/train_soft_intro_vae.py:56-61) on maps with H % 4 == 0, W % 16 == 0:
 * dw[Co][Ci][3][3] from x [B][Ci][H][W] (or, pro_mean != NULL, LeakyReLU(BatchNorm(x)) recomputed on load; per-segment
 * statistics [nseg][Ci] when seg_images > 0, nseg = B / seg_images <= 2) and dy [B][Co][H][W]; x / dy 16-byte aligned.
 * `pays`: supported AND enough stages for one block per CU.  Round 6: also the 8 x 8 and 4 x 4 maps (the deep 512-channel
 * blocks): a stage's 4 x 16 pixel strip is then 2 / 4 whole images side by side (every seam zero padding) and B and
 * seg_images must be multiples of sivae_conv2d_wino4_wgrad_images_per_stage (1 for W >= 16). */
int sivae_conv2d_wino4_wgrad_supported(int H, int W);
int sivae_conv2d_wino4_wgrad_images_per_stage(int H, int W);
int sivae_conv2d_wino4_wgrad_pays(int B, int Ci, int Co, int H, int W);
size_t sivae_conv2d_wino4_wgrad_workspace_bytes(int B, int Ci, int Co, int H, int W);
int sivae_conv2d_wino4_wgrad(const float* x, const float* dy, float* dw, const float* pro_mean, const float* pro_invstd,
                             const float* pro_gamma, const float* pro_beta, float pro_slope, int B, int Ci, int Co, int H,
                             int W, int seg_images, void* workspace, size_t workspace_bytes, sivae_stream_t stream);

/* ---- point clouds: the 3-D Soft-IntroVAE (pointcloud.hip) ------------------------------------------------------
 * ChamferLoss.forward (soft_intro_vae_3d/losses/chamfer_loss.py:11-17): preds [B][M][3], gts [B][N][3] ->
 * loss[b] = sum_j min_i |G_i - P_j|^2 + sum_i min_j |G_i - P_j|^2, both directions in one launch, with the nearest-
 * neighbour indices idx_p [B][M] (into gts) and idx_g [B][N] (into preds), int32, lowest index on a tie.  The distance is
 * the direct form dx^2 + dy^2 + dz^2 (the reference's |x|^2 + |y|^2 - 2 x.y of :19-35 cancels in fp32).  Block partials
 * go through the workspace and are folded in fp64.  Any M, N >= 1; B <= 65535.
 * _bwd: its gradient from g [B] and the forward's indices; dpreds or dgts may be NULL (not both).  No atomics: a lane
 * scans the other side's index array for its own index in ascending order. */
size_t sivae_chamfer_workspace_bytes(int B, int M, int N);
int sivae_chamfer_fwd(const float* preds, const float* gts, int* idx_p, int* idx_g, float* loss, int B, int M, int N,
                      void* workspace, size_t workspace_bytes, sivae_stream_t stream);
int sivae_chamfer_bwd(const float* g, const float* preds, const float* gts, const int* idx_p, const int* idx_g,
                      float* dpreds, float* dgts, int B, int M, int N, sivae_stream_t stream);
/* nn.ReLU -> nn.BatchNorm1d over a [B][C][N] (soft_intro_vae_3d/models/vae.py:105-128: the activation comes FIRST), from
 * the conv output a; relu(a) is never stored.  _stats: mean / invstd of relu(a) per channel and the running-buffer update
 * of sivae_bn_stats (running_mean / running_var NULL together: no update).  _apply: y = gamma (relu(a) - mean) invstd +
 * beta (eval mode: mean / invstd from the running buffers).  _bwd: dbeta = sum dy, dgamma = sum dy rhat,
 * da = [a > 0] gamma invstd (dy - dbeta / m - rhat dgamma / m), m = B N; ReLU's derivative at 0 is 0.  Any N >= 1;
 * 16-byte accesses when N % 4 == 0 and the tensors are 16-byte aligned.  One workspace size serves _stats and _bwd. */
size_t sivae_relu_bn_workspace_bytes(int B, int C, int N);
int sivae_relu_bn_stats(const float* a, int B, int C, int N, float eps, float momentum, float* running_mean,
                        float* running_var, long long* num_batches_tracked, float* mean_out, float* invstd_out,
                        void* workspace, size_t workspace_bytes, sivae_stream_t stream);
int sivae_relu_bn_apply(const float* a, const float* mean, const float* invstd, const float* gamma, const float* beta,
                        float* y, int B, int C, int N, sivae_stream_t stream);
int sivae_relu_bn_bwd(const float* dy, const float* a, const float* mean, const float* invstd, const float* gamma,
                      float* da, float* dgamma, float* dbeta, int B, int C, int N, void* workspace, size_t workspace_bytes,
                      sivae_stream_t stream);
/* output.max(dim=2) (soft_intro_vae_3d/models/vae.py:141): x [B][C][N] -> vals [B][C] and the int32 argmax [B][C]
 * (lowest index on a tie); _bwd writes g [B][C] at the argmax of an otherwise zero dx [B][C][N] in one kernel. */
int sivae_max_points_fwd(const float* x, float* vals, int* arg, int B, int C, int N, sivae_stream_t stream);
int sivae_max_points_bwd(const float* g, const int* arg, float* dx, int B, int C, int N, sivae_stream_t stream);
/* The encoder's last stage in one piece: max over the points of BatchNorm1d(ReLU(a)), a [B][C][N], without y or the max's
 * dense gradient in memory.  _fwd: mean / invstd from sivae_relu_bn_stats (eval mode: the running mean and
 * rsqrt(running_var + eps)); y = relu(a) * (gamma invstd) + (beta - mean gamma invstd) is formed in registers by the
 * function sivae_relu_bn_apply's kernel stores, so vals [B][C] and the int32 arg [B][C] are bit-identical to
 * sivae_max_points_fwd(sivae_relu_bn_apply(a)): a NaN is the maximum, the lowest index wins among ties and among NaNs.
 * _bwd: from g [B][C] and the forward's arg.  dy is g at arg and zero elsewhere, so dbeta = sum_b g and
 * dgamma = invstd (sum_b g relu(a[b][c][arg]) - mean dbeta) are sums over B values per channel (fp64, fixed order; arg is
 * clamped into the row), then one pass reads a and writes da = [a > 0] gamma invstd (dy - dbeta / m - rhat dgamma / m),
 * m = B N.  No workspace, no atomics; 16-byte accesses when N % 4 == 0 and a (and da) are 16-byte aligned. */
int sivae_relu_bn_max_fwd(const float* a, const float* mean, const float* invstd, const float* gamma, const float* beta,
                          float* vals, int* arg, int B, int C, int N, sivae_stream_t stream);
int sivae_relu_bn_max_bwd(const float* g, const int* arg, const float* a, const float* mean, const float* invstd,
                          const float* gamma, float* da, float* dgamma, float* dbeta, int B, int C, int N,
                          sivae_stream_t stream);

/* ---- point clouds: the JSD validation metric (pc_jsd.hip) ----------------------------------------------------------
 * _entropy_of_occupancy_grid (soft_intro_vae_3d/metrics/jsd.py:97-126, the NearestNeighbors fit and the per-point Python
 * loop): S clouds of N points, read in place through three ELEMENT strides (cloud, point, coordinate), against the table
 * of grid-cell centres cells [G][3] in the reference's order (row-major over (i, j, k), cells outside the sphere dropped
 * when clipping is on, _unit_cube_grid_point_cloud :139-157).  counters[c] = points whose nearest centre is c,
 * bernoulli[c] = clouds with at least one such point (may be NULL); both int32 [G], zeroed here.  lut [res^3] maps a cell
 * of the full cube to its table index (-1: dropped), axis [res] holds the float32 centre coordinates of one axis.
 * A point whose own cube cell is in the table takes that cell; any other point is compared with EVERY table entry
 * (direct-form float32 distances, lowest index on a tie).  status [2] (zeroed here): [0] points with a non-finite
 * coordinate (skipped), [1] points that took the exhaustive comparison.  2 <= res <= 64; SIVAE_ERR_RANGE for
 * S N >= 2^31.  Integer atomics only: two runs are bit-identical. */
int sivae_occupancy_grid(const float* pcs, long long stride_s, long long stride_n, long long stride_c, int S, int N,
                         const float* cells, const int* lut, const float* axis, int res, int G, int* counters,
                         int* bernoulli, int* status, sivae_stream_t stream);
/* _pc_to_voxel_distribution (metrics/jsd.py:63-72): counts [n_voxels^3] int32 (zeroed here) of
 * int((clamp(x, -0.5, 0.4999) + 0.5) * n_voxels) per coordinate, linear index (ix n + iy) n + iz, in the reference's
 * float32 operations (separately rounded add and multiply).  status [1] (zeroed here): points with a NaN coordinate
 * (skipped).  The same three element strides as above. */
int sivae_voxel_histogram(const float* pc, long long stride_s, long long stride_n, long long stride_c, int S, int N,
                          int n_voxels, int* counts, int* status, sivae_stream_t stream);
/* _js_divergence (metrics/jsd.py:25-42) of two count vectors of n entries, int32 (flag 0) or float64 (flag 1): both are
 * normalised, out[0] = H((P + Q) / 2) - (H(P) + H(Q)) / 2 with base-2 entropies and 0 log 0 = 0, in float64, one block,
 * fixed reduction order.  A zero total gives NaN, as the reference's 0 / 0 does. */
int sivae_js_divergence(const void* P, const void* Q, int p_is_f64, int q_is_f64, int n, double* out,
                        sivae_stream_t stream);

/* ---- point clouds: minimum matching distance, coverage and 1-NN accuracy (pc_eval.hip) -----------------------------
 * What soft_intro_vae_3d/README.md:47-48 asks for after evaluation/generate_data_for_metrics.py has saved its arrays: the
 * all-pairs Chamfer matrix of two sets of clouds.  sample: S clouds of M points, ref: R clouds of N points, each read in
 * place through three ELEMENT strides (cloud, point, coordinate) as sivae_occupancy_grid reads its clouds.  With
 * a_j = min_i |P_j - Q_i|^2 and b_i = min_j |P_j - Q_i|^2 (direct form dx^2 + dy^2 + dz^2, fp32),
 *   D[s][r] = sum_j f(a_j) / m + sum_i f(b_i) / n,   f(t) = t or sqrt(t) (use_sqrt), m = M, n = N (normalize) or 1,
 * float32 [S][R]; one call writes the rows s0 <= s < s1 (the caller bounds the length of one launch with the range).
 * Every distance is computed once and serves both minima; no nearest-neighbour indices.  The sums are taken in fp64 in a
 * fixed order: two runs are bit-identical.  A cloud with a NaN or infinite coordinate makes every entry of its row or
 * column non-finite and changes no other entry.  Any M, N >= 1; SIVAE_ERR_RANGE for S R >= 2^31 - 1; SIVAE_ERR_SHAPE for
 * an empty or out-of-range row range; SIVAE_ERR_MODE for a flag that is not 0 or 1.  The workspace (sized for s1 - s0
 * rows) is only used when M > 2048 and N > 2048; its size is 0 otherwise, the pointer must still not be NULL. */
size_t sivae_chamfer_matrix_workspace_bytes(int rows, int R, int M, int N);
int sivae_chamfer_matrix(const float* sample, long long sample_stride_s, long long sample_stride_n,
                         long long sample_stride_c, const float* ref, long long ref_stride_s, long long ref_stride_n,
                         long long ref_stride_c, float* D, int S, int R, int M, int N, int s0, int s1, int normalize,
                         int use_sqrt, void* workspace, size_t workspace_bytes, sivae_stream_t stream);
/* Row and column minima of a contiguous float32 D [S][R] in one launch: row_min / row_arg [S] (the coverage side:
 * the reference cloud each sample matches), col_min / col_arg [R] (the minimum-matching-distance side).  int32 indices,
 * the lowest index wins a tie; +inf and NaN entries never win, and a row or column without any other entry yields
 * (+inf, 0).  SIVAE_ERR_RANGE for S R >= 2^31 - 1. */
int sivae_match_min(const float* D, int S, int R, float* row_min, int* row_arg, float* col_min, int* col_arg,
                    sivae_stream_t stream);
/* 1-nearest-neighbour accuracy, the third figure people report beside MMD and COV in the evaluation that
 * soft_intro_vae_3d/README.md:47-48 sends the arrays of evaluation/generate_data_for_metrics.py to: a leave-one-out test
 * over the union of the two sets, which needs each set's matrix against ITSELF.
 * sivae_chamfer_matrix_self: D [S][S] float32 for ONE set of S clouds of M points (three element strides as above).  For
 * i <= j, D[i][j] is bit for bit the entry sivae_chamfer_matrix computes for (sample = ref = clouds): same flags, same
 * arithmetic, same fixed summation order, the diagonal included and computed (exactly 0 for finite clouds); D[j][i] is a
 * copy of D[i][j] (for M = N that arithmetic is symmetric in its two clouds bit for bit, so the whole matrix equals the
 * full one's).  A cloud with a non-finite coordinate makes its row and its column non-finite.  Only the pairs i <= j are
 * computed, enumerated by FOLDED rows: folded row f in [0, ceil(S / 2)) has the S + 1 columns c; c < S - f is the pair
 * (f, f + c), any other c the pair (S - 1 - f, S - 1 - f + c - (S - f)); for odd S the middle row (S - 1 - f == f) has only
 * its first S - f columns.  One call computes the folded rows f0 <= f < f1 (the caller bounds a launch with the range) and
 * stores both D[i][j] and D[j][i] of each pair.  SIVAE_ERR_SHAPE for non-positive sizes or a range outside
 * 0 <= f0 < f1 <= ceil(S / 2); SIVAE_ERR_RANGE for S S >= 2^31 - 1; SIVAE_ERR_MODE for a flag that is not 0 or 1.  The
 * workspace (sized for f1 - f0 folded rows: M words per launched block) is only used when M > 2048; its size is 0
 * otherwise, the pointer must still not be NULL (SIVAE_ERR_WORKSPACE). */
size_t sivae_chamfer_matrix_self_workspace_bytes(int frows, int S, int M);
int sivae_chamfer_matrix_self(const float* clouds, long long stride_s, long long stride_n, long long stride_c, float* D,
                              int S, int M, int f0, int f1, int normalize, int use_sqrt, void* workspace,
                              size_t workspace_bytes, sivae_stream_t stream);
/* The joint leave-one-out nearest neighbour behind 1-NN accuracy (same citation).  Dss [S][S], Dsr [S][R], Drr [R][R]:
 * contiguous float32.  The T = S + R items are the samples 0 .. S - 1 and the references S .. T - 1; the distance from
 * item t to item u != t is read from ROW t of the joint matrix [[Dss, Dsr], [Dsr^T, Drr]]:
 *   t < S, u < S: Dss[t][u];   t < S, u >= S: Dsr[t][u - S];   t >= S, u < S: Dsr[u][t - S];   t >= S, u >= S: Drr[t - S][u - S]
 * (for a Dss or Drr that is not symmetric, this row rule is the definition).  The entry u = t is never a candidate,
 * whatever it holds.  nn_arg[t] (int32 [T]) is the u of the smallest distance, the lowest u on a tie, nn_val[t] (float32
 * [T]) that distance; +inf and NaN never win; an item with no candidate left gives (+inf, -1).  No atomics, no workspace:
 * two runs are bit-identical.  SIVAE_ERR_RANGE for (S + R)(S + R) >= 2^31 - 1. */
int sivae_nn1_loo(const float* Dss, const float* Dsr, const float* Drr, int S, int R, float* nn_val, int* nn_arg,
                  sivae_stream_t stream);

/* ---- point clouds: the earth mover's distance matrix (pc_emd.hip) --------------------------------------------------
 * MMD-EMD / COV-EMD, the two remaining figures of the tables soft_intro_vae_3d/README.md:47-48 points to (the notebook's
 * minimum_mathing_distance / coverage with use_EMD): the all-pairs matrix of the APPROXIMATE-MATCHING earth mover's
 * distance of Fan, Su and Guibas ("A point set generation network for 3D object reconstruction from a single image",
 * CVPR 2017; the approxmatch / matchcost pair).  For a left cloud A [n][3] and a right cloud B [m][3], with
 * d2(k, l) = |A_k - B_l|^2 in the direct form (fp32):
 *   big = max(n, m);  remL[k] = big / n;  remR[l] = big / m   (real division; the original divides as integers, which
 *   cost = 0                                                   is the same for n = m)
 *   for j = 7, 6, ..., -2:   level = -4^j, and 0 at j = -2;   w(k, l) = exp(level d2(k, l))
 *     1. suml[k] = 1e-9 + sum_l w(k, l) remR[l];   ratioL[k] = remL[k] / suml[k]
 *     2. sumr[l] = remR[l] sum_k w(k, l) ratioL[k];   ratioR[l] = remR[l] min(remR[l] / (sumr[l] + 1e-9), 1);
 *        remR[l] = max(0, remR[l] - sumr[l])
 *     3. t(k, l) = w(k, l) ratioL[k] ratioR[l];   cost += sum_kl t(k, l) sqrt(d2(k, l));
 *        remL[k] = max(0, remL[k] - sum_l t(k, l))
 *   EMD(A, B) = cost / big (normalize) or cost.
 * D[s][r] = EMD(left = ref_r, right = sample_s), float32 [S][R]; the quantity is not symmetric.  Arguments, strides, the
 * row range s0 <= s < s1 and the return codes are sivae_chamfer_matrix's.  The weights are exp2 of level log2(e) d2 (the
 * hardware's exponential), d2 is recomputed in each of the thirty sweeps.  Every per-point sum of a level is fp32 in index
 * order, the cost's included (sum_l t sqrt(d2) of one left point, up to 4096 terms); those per-point, per-level costs are
 * added in fp64 in a fixed order: D does not depend on the grid, the row range, the strides or the run.  A cloud
 * with a NaN or infinite coordinate makes every entry of its row or column NaN (found while loading) and changes no other
 * entry.  1 <= M, N <= 4096 (both clouds are held in LDS); SIVAE_ERR_RANGE beyond, and for S R >= 2^31 - 1.  No
 * workspace is used: the size is 0, the pointer must still not be NULL. */
size_t sivae_emd_matrix_workspace_bytes(int rows, int R, int M, int N);
int sivae_emd_matrix(const float* sample, long long sample_stride_s, long long sample_stride_n, long long sample_stride_c,
                     const float* ref, long long ref_stride_s, long long ref_stride_n, long long ref_stride_c, float* D,
                     int S, int R, int M, int N, int s0, int s1, int normalize, void* workspace, size_t workspace_bytes,
                     sivae_stream_t stream);
/* The same quantity as a reconstruction loss (reference: soft_intro_vae_3d/train_soft_intro_vae_3d.py:171-176 accepts
 * 'earth_mover' next to 'chamfer'; the project it derives from trains with losses/earth_mover_distance.py::EMD on the
 * approxmatch / matchcost / matchcostgrad extension).  For a batch of cloud pairs left [B][N][3] and right [B][M][3]
 * (float32, element strides as above, 1 <= N, M <= 4096):
 *   cost[b] = EMD(left = left_b, right = right_b), exactly the quantity above (ten levels, steps 1 - 3, the direct-form
 *   d2, big = max(N, M)): with t_j(k, l) the step-3 weight of level j, cost = sum_j sum_kl t_j(k, l) sqrt(d2(k, l)),
 *   divided by big when normalize.  cost[b] is bit for bit the D[0][0] of sivae_emd_matrix(sample = right_b, ref = left_b).
 * The gradient is matchcostgrad's: the plan t is HELD CONSTANT (it is not the derivative through the ratios),
 *   dleft[b][k]  =   sum_j sum_l t_j(k, l) (A_k - B_l) / sqrt(d2(k, l))
 *   dright[b][l] = - sum_j sum_k t_j(k, l) (A_k - B_l) / sqrt(d2(k, l))
 * both divided by big when normalize.  A pair with d2 == 0 contributes zero: the reciprocal root is taken of
 * max(d2, FLT_MIN) (the original's max(d, 1e-20)) and the difference is zero there.  Because the plan moves with the
 * points, finite differences of cost do NOT reproduce these gradients (torch.autograd.gradcheck does not apply); with the
 * plan fixed the cost is 1-homogeneous, so sum_k A_k . dleft[k] + sum_l B_l . dright[l] = cost, and the two gradients sum
 * to zero per coordinate.
 * The order is the original's: EMD()(preds, gts) has left = preds, right = gts.
 * dleft (contiguous [B][N][3]) and dright (contiguous [B][M][3]) may each be NULL: only the sums asked for are formed (the
 * left one rides on the step-3 sweep, the right one takes a fourth sweep per level, own l over staged k, forming the same
 * t = (w ratioL[k]) ratioR[l] in the same order).  If pair b has a NaN or infinite coordinate, cost[b] and every element
 * of both gradient slices of b are NaN, written outright; no other pair changes a bit.  No atomics: every per-point sum
 * of a level is fp32 in index order, the levels are added in level order, the cost total is formed as above; every
 * output element is written once.  Two runs are bit-identical, whatever the grid, the batch split or the strides.
 * SIVAE_ERR_NULL for a missing left / right / cost, SIVAE_ERR_SHAPE for a non-positive size, SIVAE_ERR_RANGE beyond
 * 4096 points or for 3 B max(N, M) >= 2^31 - 1, SIVAE_ERR_MODE for a normalize other than 0 / 1, SIVAE_ERR_WORKSPACE
 * for a NULL or too small workspace: all returned before any device call.  No workspace is used: the size is 0, the
 * pointer must still not be NULL. */
size_t sivae_emd_loss_workspace_bytes(int B, int N, int M);
int sivae_emd_loss(const float* left, long long left_stride_b, long long left_stride_n, long long left_stride_c,
                   const float* right, long long right_stride_b, long long right_stride_n, long long right_stride_c,
                   float* cost, float* dleft, float* dright, int B, int N, int M, int normalize, void* workspace,
                   size_t workspace_bytes, sivae_stream_t stream);

/* ---- FID: fp64 activation moments and the products of the Frechet distance (fid.hip) ---------------------------------
 * The image variants' validation metric (soft_intro_vae/train_soft_intro_vae.py:283-296 calls
 * metrics/fid_score.py::calculate_fid_given_dataset), everything but the Inception network.  All arithmetic is fp64 on
 * v_mfma_f64_16x16x4_f64; one block owns each 64 x 64 output tile and walks the summed index in ascending order: no
 * atomics, two runs are bit-identical.  Every pointer must be aligned for its element type (SIVAE_ERR_SHAPE).
 *
 * sivae_fid_moments replaces the host-side activation store and np.mean / np.cov of fid_score.py:197, :202-203, :262-265,
 * :349-350, :375-376: A [n][d] float32 (row stride in elements, >= d; unit column stride), each element converted to
 * fp64 on load; G [d][d] (contiguous fp64) += A^T A on the 64 x 64 block tiles with column tile >= row tile (the tiles
 * below are never touched; inside a diagonal tile both halves are computed and are bit-identical mirrors), s [d]
 * (fp64) += column sums, rows added in ascending order.  Rows >= n and columns >= d are masked, not read.  Any n >= 0
 * (n = 0 launches nothing); 1 <= d <= 8192, SIVAE_ERR_SHAPE otherwise. */
int sivae_fid_moments(const float* A, long long row_stride, int n, int d, double* G, double* s, sivae_stream_t stream);
/* The statistics of (n, s, G) (fid_score.py:349-350): mu [d] = s / n, sigma [d][d] = (G - s s^T / n) / (n - 1) written as
 * the full symmetric matrix from G's entries on and above the diagonal (exactly symmetric).  n = 1 gives NaN in sigma,
 * as np.cov does; n <= 0 is SIVAE_ERR_SHAPE. */
int sivae_fid_finalize(const double* G, const double* s, long long n, int d, double* mu, double* sigma,
                       sivae_stream_t stream);
/* C [M][N] = X^T Y for fp64 X [K][M], Y [K][N] (row strides ldx >= M, ldy >= N, ldc >= N in elements; C must not
 * overlap X or Y): the products behind the matrix square root of fid_score.py:307.  symmetric = 1 (M == N, for a product
 * that is symmetric by construction): only the tiles with column tile >= row tile are computed and every entry on or
 * above the diagonal is stored at (i, j) and (j, i), so C is exactly symmetric.  K >= 1, 1 <= M, N <= 8192
 * (SIVAE_ERR_SHAPE); SIVAE_ERR_MODE for a flag that is not 0 or 1. */
int sivae_fid_xty_f64(const double* X, long long ldx, const double* Y, long long ldy, double* C, long long ldc, int K,
                      int M, int N, int symmetric, sivae_stream_t stream);

/* ---- pairwise figures on the FID features: precision / recall, density / coverage, KID (feat_pairs.hip) --------------
 * Everything is a reduction over X Y^T of two sets of feature rows, float32 [n][d] with unit column stride and any row
 * stride (ld >= d, in elements), every element converted to fp64 on load; 1 <= d <= 8192, n >= 1 (SIVAE_ERR_SHAPE).  One
 * tile body computes a 64 x 64 tile of X Y^T on v_mfma_f64_16x16x4_f64, the summed index ascending; rows are read with
 * 16-byte loads where the base is 16-byte aligned and ld % 4 == 0, with scalar loads otherwise.  The squared distance is
 *   sqdist(x, y) = max(0, |x|^2 + |y|^2 - 2 x.y)            (fp64 throughout; the products of fp32 values are exact)
 * with the squared norms of sivae_feat_row_sqnorm, so |sqdist - sum_k (x_k - y_k)^2| <= 2 (d + 3) 2^-53 (|x| + |y|)^2:
 * two equal rows give a distance within that bound of 0, not exactly 0.  Inputs must be finite (the callers check the
 * norms).  No atomics: every output element has one owner, and two runs are bit-identical.  Pointers must be aligned
 * for their element type (SIVAE_ERR_SHAPE).
 *
 * out[i] = sum_k X[i][k]^2, k ascending. */
int sivae_feat_row_sqnorm(const float* X, long long ld, int n, int d, double* out, sivae_stream_t stream);
/* D[i][j] = sqdist(x_i, y_j), D [nx][ny] fp64 with row stride ldd >= ny: the plain matrix, for sets small enough to hold
 * it; one block per output tile.  SIVAE_ERR_RANGE above 2^31 - 1 tiles. */
int sivae_feat_sqdist(const float* X, long long ldx, int nx, const double* nrmx, const float* Y, long long ldy, int ny,
                      const double* nrmy, int d, double* D, long long ldd, sivae_stream_t stream);
/* best [nx][k] fp64, every row ascending (+inf before the first call): row i <- the k smallest of its values and
 * sqdist(x_i, y_j) for j in [c0, c1), 0 <= c0 <= c1 <= ny; with self = 1 the pair j == i is left out by index, not by
 * value.  1 <= k <= 8.  One block owns 64 rows of X and walks the columns: the state lives in `best` so that the caller
 * can cut [0, ny) into launches, and since merging smallest values is exact the result is the same for every cutting. */
int sivae_feat_knn_update(const float* X, long long ldx, int nx, const double* nrmx, const float* Y, long long ldy, int ny,
                          const double* nrmy, int c0, int c1, int d, int k, int self, double* best,
                          sivae_stream_t stream);
/* count[j] += #{ i in [c0, c1) : sqdist(q_j, x_i) <= radius[i] }, count int32 [nq], radius fp64 [nx], 0 <= c0 <= c1 <=
 * nx: in how many of the balls around the rows of X the row q_j lies.  One block owns 64 rows of Q; exact for every
 * cutting of [0, nx). */
int sivae_feat_within_update(const float* Q, long long ldq, int nq, const double* nrmq, const float* X, long long ldx,
                             int nx, const double* nrmx, const double* radius, int c0, int c1, int d, int* count,
                             sivae_stream_t stream);
/* out[s] = sum_{i < m, j < n} (gamma x_si . y_sj + coef0)^degree for the S subsets X [S][m][d], Y [S][n][d] (subset
 * strides in elements), i == j left out with skip_diag = 1; degree 1 .. 4 by repeated multiplication (SIVAE_ERR_MODE).
 * One block per (subset, 64-row strip) adds its entries in a fixed order into the workspace, a second launch adds the
 * strips of a subset in ascending order: a subset's sum does not depend on the other subsets of the launch. */
size_t sivae_feat_poly_workspace_bytes(int S, int m);
int sivae_feat_poly_sums(const float* X, long long x_stride_s, long long ldx, const float* Y, long long y_stride_s,
                         long long ldy, int S, int m, int n, int d, double gamma, double coef0, int degree, int skip_diag,
                         double* out, void* workspace, size_t workspace_bytes, sivae_stream_t stream);

/* ---- the style variant's non-conv layers: fused instance-norm chains and the blur (style.hip) ------------------------
 * What follows every 3x3 convolution of style_soft_intro_vae/net.py, one forward and one backward kernel per chain.
 * float32, NCHW contiguous, any B, C >= 1 and any H, W with H W >= 2 (torch's InstanceNorm refuses a single element:
 * SIVAE_ERR_SHAPE); SIVAE_ERR_RANGE for B C > 2^31 - 1 or H W > 2^30 - 1.  One block owns one (b, c) plane; planes up
 * to 65536 elements (forward) / 16384 elements (backward) stay in registers between the statistics and the apply step
 * (one read per direction), larger ones are read again.  Every pointer must be 4-byte aligned (SIVAE_ERR_SHAPE); where
 * every plane is 16-byte aligned the kernels use 16-byte accesses, anywhere else guarded scalar ones over the SAME
 * partition of the plane (an H W that is no multiple of 4 ends in a scalar tail), so the alignment changes no bit.
 * No atomics.  Every sum runs in a fixed order (a thread's elements in index order in fp32; lanes, then waves, in fp64):
 * two runs are bit-identical, and one plane's results depend neither on B, on C nor on the other planes.  Null
 * pointers, shapes and modes are refused before any launch.
 *
 * sivae_style_dec_fwd replaces net.py:169-185 and :189-205 (DecodeBlock.forward: noise injection, bias,
 * F.leaky_relu(x, 0.2), nn.InstanceNorm2d(affine=False), style_mod of net.py:32-34):
 *   mode 1: noise [B][1][H][W],  u = x + noise_weight[c] noise[b][h][w]
 *   mode 2: noise [1][1][H][W], the same plane for every sample (the reference's 'batch_constant')
 *   mode 0: no noise tensor (noise and noise_weight may be NULL),  u = x + s k exp(-x^2 / (2 s^2)), k = 0.8 / sqrt(2 pi),
 *           s = sqrt(layer + 1)  (layer >= 0)
 *   t = lrelu_0.2(u + bias[c]);  per plane m = mean t, v = mean (t - m)^2, r = 1 / sqrt(v + eps), xh = (t - m) r
 *   y = xh (style[b][c] + 1) + style[b][C + c]                                  (style [B][2 C])
 * Outputs y [B][C][H][W], mean = m [B][C], rstd = r [B][C].  SIVAE_ERR_MODE for another mode; SIVAE_ERR_NULL for a
 * missing x / bias / style / output, and for a missing noise or noise_weight in modes 1 and 2; SIVAE_ERR_SHAPE for a
 * negative layer or eps. */
int sivae_style_dec_fwd(const float* x, const float* noise, const float* noise_weight, const float* bias,
                        const float* style, float* y, float* mean, float* rstd, int B, int C, int H, int W, int mode,
                        int layer, float eps, sivae_stream_t stream);
/* Its backward from dy and the forward's inputs, mean and rstd; t is recomputed, never stored.  With sums over a plane:
 *   dstyle[b][C + c] = sum dy;   dstyle[b][c] = sum dy xh
 *   dt = r (style[b][c] + 1) (dy - dstyle[b][C + c] / HW - xh dstyle[b][c] / HW)
 *   dp = dt (t > 0 ? 1 : 0.2)                      (torch's LeakyReLU gradient: the slope 0.2 at 0)
 *   dbias[c] = sum_{b, hw} dp;   dnoise_weight[c] = sum_{b, hw} dp noise   (modes 1, 2)
 *   dx = dp (modes 1, 2);   dx = dp (1 - k (x / s) exp(-x^2 / (2 s^2)))   (mode 0)
 * dx, dnoise_weight [C], dbias [C] and dstyle [B][2 C] may each be NULL: only what is asked for is computed (nothing is
 * launched when all four are NULL); a dnoise_weight in mode 0 is SIVAE_ERR_MODE.  The sums over b run in ascending b in
 * a second small launch, from per-plane fp64 partials in the workspace (2 B C doubles, 8-byte aligned), which is needed
 * only when dbias or dnoise_weight is asked for: SIVAE_ERR_WORKSPACE then for a NULL or too small one. */
size_t sivae_style_dec_bwd_workspace_bytes(int B, int C);
int sivae_style_dec_bwd(const float* dy, const float* x, const float* noise, const float* noise_weight, const float* bias,
                        const float* style, const float* mean, const float* rstd, float* dx, float* dnoise_weight,
                        float* dbias, float* dstyle, int B, int C, int H, int W, int mode, int layer, void* workspace,
                        size_t workspace_bytes, sivae_stream_t stream);
/* sivae_style_enc_fwd replaces net.py:94-101 and :113-121 (EncodeBlock.forward: bias, F.leaky_relu(x, 0.2), the style
 * statistics (mean, std), nn.InstanceNorm2d(affine=False)):
 *   t = lrelu_0.2(x + bias[c]);  m = mean t, v = mean (t - m)^2;  std = sqrt(v) (no eps);  xn = (t - m) / sqrt(v + eps)
 * Outputs xn [B][C][H][W], mean [B][C], std [B][C]; all three are differentiable. */
int sivae_style_enc_fwd(const float* x, const float* bias, float* xn, float* mean, float* stddev, int B, int C, int H,
                        int W, float eps, sivae_stream_t stream);
/* Its backward from (dxn, dmean, dstd), each of which may be NULL (a zero gradient), with r = 1 / sqrt(std^2 + eps):
 *   dt = r (dxn - mean dxn - xn mean(dxn xn)) + dmean / HW + dstd (t - m) / (HW std)
 *   dp = dt (t > 0 ? 1 : 0.2);   dx = dp;   dbias[c] = sum_{b, hw} dp  (ascending b, as above; workspace: B C doubles)
 * Where std == 0 (a constant plane) the reference's gradient is NaN (the square root's derivative at 0): this kernel
 * DROPS the dstd term there, and every gradient stays finite.  dx and dbias may each be NULL. */
size_t sivae_style_enc_bwd_workspace_bytes(int B, int C);
int sivae_style_enc_bwd(const float* dxn, const float* dmean, const float* dstd, const float* x, const float* bias,
                        const float* mean, const float* stddev, float* dx, float* dbias, int B, int C, int H, int W,
                        float eps, void* workspace, size_t workspace_bytes, sivae_stream_t stream);
/* The depthwise [1, 2, 1] x [1, 2, 1] / 16 filter with zero padding (net.py:49-60, Blur), y [B][C][H][W] from x, any
 * H, W >= 1; y must not overlap x.  The filter is its own adjoint: the same call is the backward (dx from dy).  Rows
 * first, (l + 2 c) + r, then (top + 2 mid) + bottom, times 1 / 16. */
int sivae_style_blur(const float* x, float* y, int B, int C, int H, int W, sivae_stream_t stream);
/* The blur folded into the chain next to it: the four entry points below are the ones above with the blurred tensor never
 * stored.  Arguments, shapes, refusals, the partition of a plane and the order of every sum are those of the plain entry
 * point, and every output is, bit for bit, what the two calls it replaces give (the stencil is sivae_style_blur's own).
 *
 * sivae_style_dec_blur_fwd replaces net.py:49-60 with :166-185 (DecodeBlock.forward: the blur behind conv_1, then the
 * first layer): sivae_style_dec_fwd of blur(x).  x is the UNBLURRED tensor; the kernel takes the 9 taps from it. */
int sivae_style_dec_blur_fwd(const float* x, const float* noise, const float* noise_weight, const float* bias,
                             const float* style, float* y, float* mean, float* rstd, int B, int C, int H, int W, int mode,
                             int layer, float eps, sivae_stream_t stream);
/* Its backward from dy, the UNBLURRED x and the forward's mean and rstd: blur(x) is taken by the same 9 taps, the gradient
 * g with respect to blur(x) is sivae_style_dec_bwd's dx, and dx = blur(g) (the filter is its own adjoint).  dstyle, dbias
 * and dnoise_weight are sivae_style_dec_bwd's of blur(x).  Where sivae_style_dec_blur_bwd_fused(H, W) is 1 (H W <= 16384,
 * a plane the kernel stages in 64 KiB of LDS) dx leaves as blur(g): one launch.  Where it is 0, dx receives g and the
 * caller finishes with sivae_style_blur(dx -> another buffer).  Workspace as sivae_style_dec_bwd's. */
size_t sivae_style_dec_blur_bwd_workspace_bytes(int B, int C);
int sivae_style_dec_blur_bwd_fused(int H, int W);
int sivae_style_dec_blur_bwd(const float* dy, const float* x, const float* noise, const float* noise_weight,
                             const float* bias, const float* style, const float* mean, const float* rstd, float* dx,
                             float* dnoise_weight, float* dbias, float* dstyle, int B, int C, int H, int W, int mode,
                             int layer, void* workspace, size_t workspace_bytes, sivae_stream_t stream);
/* sivae_style_enc_blur_fwd replaces net.py:94-101 with :110 (EncodeBlock.forward: the first norm, then the blur in front
 * of conv_2): the outputs are bxn = blur(xn) [B][C][H][W] and sivae_style_enc_fwd's mean and std; xn is not written (a
 * neighbour's xn is recomputed from x).  Any plane size. */
int sivae_style_enc_blur_fwd(const float* x, const float* bias, float* bxn, float* mean, float* stddev, int B, int C, int H,
                             int W, float eps, sivae_stream_t stream);
/* Its backward: sivae_style_enc_bwd with dxn = blur(dbxn), read from dbxn (which may be NULL) by 9 taps.  dmean, dstd, the
 * dropped dstd term on a constant plane and the workspace are sivae_style_enc_bwd's.  Any plane size. */
size_t sivae_style_enc_blur_bwd_workspace_bytes(int B, int C);
int sivae_style_enc_blur_bwd(const float* dbxn, const float* dmean, const float* dstd, const float* x, const float* bias,
                             const float* mean, const float* stddev, float* dx, float* dbias, int B, int C, int H, int W,
                             float eps, void* workspace, size_t workspace_bytes, sivae_stream_t stream);

/* ---- the style variant's RGB layers and the level-of-detail blend (rgb.hip) -------------------------------------------
 * ToRGB and FromRGB of style_soft_intro_vae/net.py with what Generator.decode2 and the encoders' encode2 do around them
 * while a new resolution fades in.  float32, NCHW contiguous.  K is the image channel count, 1 <= K <= 4
 * (SIVAE_ERR_SHAPE otherwise), C >= 1 the feature channel count, B <= 65535 and H W <= 2^30 - 1 (SIVAE_ERR_RANGE).
 *   lrelu2(t) = lrelu_0.2(lrelu_0.2(t)); its derivative is 1 for t > 0 and 0.04 otherwise (torch's rule twice).
 *   lerp(a, b, s) is torch's scalar-weight formula: |s| < 0.5: a + s (b - a); otherwise b - (b - a)(1 - s), 1 - s in fp32.
 *   up2 is nearest-neighbour 2x upsampling; avg2 the 2 x 2 average ((p00 + p01) + (p10 + p11)) / 4.
 * Every pointer must be 4-byte aligned (SIVAE_ERR_SHAPE); where every tensor that is walked plane-wise is 16-byte aligned
 * and the plane size a multiple of 4 the kernels use 16-byte accesses, anywhere else guarded scalar ones over the same
 * partition, so the alignment changes no bit.  No atomics; every sum runs in an order fixed by (C, H W): two runs are
 * bit-identical and a sample's forward result does not depend on the batch.  Each tensor of C planes is read at most once
 * per direction.  Null pointers, shapes, flags and workspaces are refused before any launch.
 *
 * sivae_to_rgb_fwd (net.py:229-231, and :563-571 with prev): x [B][C][H][W], w [K][C], bias [K] -> y [B][K][H][W]
 *   conv[b][k][p] = bias[k] + sum_c w[k][c] x[b][c][p]
 *   prev == NULL: y = conv;   prev [B][K][H/2][W/2]: y = lerp(up2(prev), conv, blend)   (H, W even: SIVAE_ERR_SHAPE) */
int sivae_to_rgb_fwd(const float* x, const float* w, const float* bias, const float* prev, float blend, float* y, int B,
                     int C, int H, int W, int K, sivae_stream_t stream);
/* Its backward from dy [B][K][H][W]; has_prev says whether the forward blended (0 / 1, SIVAE_ERR_MODE otherwise):
 *   g = dy (plain);   g = dy blend (blended: d lerp / d conv = blend on both branches)
 *   dx[b][c][p] = sum_k w[k][c] g[b][k][p];   dw[k][c] = sum_{b,p} g[b][k][p] x[b][c][p];   dbias[k] = sum_{b,p} g[b][k][p]
 *   dprev[b][k][q] = (1 - blend) ((dy00 + dy01) + (dy10 + dy11)) over the four pixels of q   (has_prev only: SIVAE_ERR_MODE)
 * dx, dw, dbias and dprev may each be NULL: only what is asked for is computed; x is read only for dw and may be NULL
 * otherwise.  dw and dbias go through per-block fp32 partials in the workspace (16-byte aligned,
 * sivae_to_rgb_bwd_workspace_bytes) that a second small launch adds in block order in fp64; SIVAE_ERR_WORKSPACE for a
 * NULL, misaligned or too small one when either is asked for. */
size_t sivae_to_rgb_bwd_workspace_bytes(int B, int C, int H, int W, int K);
int sivae_to_rgb_bwd(const float* dy, const float* x, const float* w, int has_prev, float blend, float* dx, float* dw,
                     float* dbias, float* dprev, int B, int C, int H, int W, int K, void* workspace, size_t workspace_bytes,
                     sivae_stream_t stream);
/* sivae_from_rgb_fwd (net.py:215-219 followed by :270-271, and :289-294 with pool and other): img [B][K][H][W],
 * w [C][K], bias [C].  H, W are the IMAGE's; the features are Ho x Wo = H x W, or H/2 x W/2 with pool = 1 (H, W even:
 * SIVAE_ERR_SHAPE; a pool that is not 0 / 1: SIVAE_ERR_MODE):
 *   u = img (pool 0);   u = avg2(img) (pool 1)
 *   t[b][c][p] = bias[c] + sum_k w[c][k] u[b][k][p];   a = lrelu2(t)
 *   other == NULL: y = a;   other [B][C][Ho][Wo]: y = lerp(a, other, blend)
 * Output y [B][C][Ho][Wo]. */
int sivae_from_rgb_fwd(const float* img, const float* w, const float* bias, int pool, const float* other, float blend,
                       float* y, int B, int C, int H, int W, int K, sivae_stream_t stream);
/* Its backward from dy [B][C][Ho][Wo]; t is recomputed from img, nothing of C planes is saved.  has_other says whether
 * the forward blended (0 / 1):
 *   da = dy lrelu2'(t) (plain);   da = (dy (1 - blend)) lrelu2'(t) (blended)
 *   dw[c][k] = sum_{b,p} da[b][c][p] u[b][k][p];   dbias[c] = sum_{b,p} da[b][c][p]
 *   du[b][k][p] = sum_c w[c][k] da[b][c][p];   dimg = du (pool 0);   dimg = du / 4 at each of the four source pixels (pool 1)
 *   dother = dy blend   (has_other only: SIVAE_ERR_MODE)
 * dimg [B][K][H][W], dw, dbias and dother may each be NULL (nothing is launched when all four are).  Workspace as above,
 * needed when dw or dbias is asked for. */
size_t sivae_from_rgb_bwd_workspace_bytes(int B, int C, int H, int W, int K, int pool);
int sivae_from_rgb_bwd(const float* dy, const float* img, const float* w, const float* bias, int pool, int has_other,
                       float blend, float* dimg, float* dw, float* dbias, float* dother, int B, int C, int H, int W, int K,
                       void* workspace, size_t workspace_bytes, sivae_stream_t stream);

/* ---- multi-tensor launches for the style variant's optimizer (multi_tensor.hip) ----------------------------------------
 * One launch walks many float32 tensors.  The lists are HOST arrays of n_tensors entries: device addresses as uint64,
 * element counts as size_t, step sizes as float.  A launch carries its share of the list BY VALUE in the kernel
 * arguments (sivae_mt_table_bytes() <= 4096 of them): at most sivae_mt_max_tensors() tensors and sivae_mt_max_chunks()
 * chunks of sivae_mt_chunk_elems() elements, one block per chunk; a longer list is cut into as many launches as it needs
 * and a tensor of more chunks than a launch has room for goes on in the next one (sivae_mt_launches() says how many
 * launches a list of element counts takes; it touches no device).  Nothing is allocated, copied or synchronised, there
 * are no atomics and no workspace.  A tensor whose addresses are all 16-byte aligned is walked with 16-byte accesses,
 * any other with scalar ones over the same elements: an element's result depends on its own inputs alone, so a tensor
 * is bit-identical alone, among others, at any 4-byte-aligned address and across a cut between two launches.
 * Refused before any launch: SIVAE_ERR_SHAPE for a negative n_tensors or an address that is not 4-byte aligned,
 * SIVAE_ERR_NULL for a null array or a null address of a tensor with elements, SIVAE_ERR_RANGE for beta2 outside
 * [0, 1), a non-finite one_minus_beta2, a negative or non-finite eps, a non-finite weight.  n_tensors == 0 and tensors
 * of zero elements are legal and launch nothing.
 *
 * sivae_mt_lreq_adam replaces the loop of style_soft_intro_vae/custom_adam.py:52-95 (LREQAdam.step: mul_, addcmul_,
 * sqrt, add_, addcdiv_ per tensor) for the tensors that have a gradient; per element, every operation rounded to fp32
 * with IEEE square root and division and no contraction:
 *   v <- beta2 v + one_minus_beta2 (g g);   p <- p - step_sizes[t] (g / (sqrtf(v) + eps))
 * with step_sizes[t] = lr sqrt(1 - beta2^step) lr_equalization_coef formed by the caller in double.  No clamps: a
 * non-finite g makes that element of p and v non-finite and no other. */
int sivae_mt_max_tensors(void);
int sivae_mt_max_chunks(void);
int sivae_mt_chunk_elems(void);
int sivae_mt_table_bytes(void);
int sivae_mt_launches(const void* numel, int n_tensors);
int sivae_mt_lreq_adam(const void* params, const void* grads, const void* exp_avg_sq, const void* numel,
                       const void* step_sizes, int n_tensors, float beta2, float one_minus_beta2, float eps,
                       sivae_stream_t stream);
/* sivae_mt_lerp replaces the loop body of style_soft_intro_vae/model.py:328-329 (p.data.lerp_(p_other.data, w)), torch's
 * formula with d = src - dst:  |w| < 0.5: dst <- dst + w d;  otherwise: dst <- src - d (1 - w), 1 - w formed in fp32. */
int sivae_mt_lerp(const void* dst, const void* src, const void* numel, int n_tensors, float weight, sivae_stream_t stream);

/* ---- the style variant's mapping networks and style assembly (mapping.hip, and one epilogue of linear.hip) ---------------
 * What style_soft_intro_vae/net.py and model.py leave between the latent and the networks.  fp32, rows [rows][cols]
 * contiguous.  Every pointer must be 4-byte aligned (SIVAE_ERR_SHAPE); where every row of every tensor of a call is 16-byte
 * aligned the kernels use 16-byte accesses, anywhere else guarded scalar ones over the same partition, so the alignment
 * changes no bit.  No atomics, no workspace; every sum runs in an order fixed by the shape alone.  A tensor of 2^31 or
 * more elements is SIVAE_ERR_RANGE, a non-positive size SIVAE_ERR_SHAPE, all returned before any launch.
 *
 * sivae_linear_lrelu_fwd: sivae_linear_fwd with LeakyReLU(slope) behind the bias (a MappingBlock, net.py:748-751):
 *   y = v > 0 ? v : v slope, v = x W^T + bias, one multiply as torch's.  Same shapes, workspace and codes as
 *   sivae_linear_fwd; a slope outside [0, 1] is SIVAE_ERR_MODE.  (ReLU is not this with slope 0: fmaxf differs on -0 and
 *   NaN; sivae_linear_fwd is unchanged.) */
int sivae_linear_lrelu_fwd(const float* x, const float* w, const float* bias, float* y, float slope, int B, int K, int N,
                           void* workspace, size_t workspace_bytes, sivae_stream_t stream);
/* Its way back to the pre-activation, from the saved OUTPUT y [B][N] (its sign is the pre-activation's), with the bias
 * gradient, in one pass over dy:
 *   dz[b][n] = dy[b][n] (y[b][n] > 0 ? 1 : slope)   (the slope at 0 is `slope`, torch's rule)
 *   dbias[n] = sum_b dz[b][n], ascending b, accumulated in fp64
 * y == NULL: a layer without activation, dz = dy.  dz and dbias may each be NULL (nothing is launched when both are). */
int sivae_lrelu_bias_bwd(const float* dy, const float* y, float slope, float* dz, float* dbias, int B, int N,
                         sivae_stream_t stream);
/* pixel_norm (net.py:29-30) over the rows of x [B][Z], any B, Z >= 1:
 *   r[b] = 1 / sqrt(mean_z x[b][z]^2 + eps) (the mean and r formed in fp64, kept in rfac [B] for the backward)
 *   y = x r;   dx = r dy - x r^3 mean_z(dy x)
 * A row of zeros gives y = 0 and dx = dy / sqrt(eps).  eps < 0 is SIVAE_ERR_SHAPE. */
int sivae_pixel_norm_fwd(const float* x, float* y, float* rfac, int B, int Z, float eps, sivae_stream_t stream);
int sivae_pixel_norm_bwd(const float* dy, const float* x, const float* rfac, float* dx, int B, int Z,
                         sivae_stream_t stream);
/* The style assembly of SoftIntroVAEModelTL.generate (model.py:176-200) from s [B][Z] to styles [B][L][Z], in the
 * reference's order:
 *   update_avg = 1: avg[l] <- lerp(avg[l], mean_b s[b], avg_weight) for every l (avg [L][Z], updated in place by a first
 *                   small launch; avg_weight = 1 - beta formed by the caller, outside [0, 1]: SIVAE_ERR_MODE; the mean runs
 *                   in ascending b in fp64);
 *   s2 != NULL:     layers l >= mix_cutoff take s2 [B][Z] (0 <= mix_cutoff <= L, SIVAE_ERR_SHAPE otherwise);
 *   truncate = 1:   styles[b][l] = lerp(avg[l], styles[b][l], psi) for l < trunc_cutoff (0 <= trunc_cutoff <= L), with the
 *                   UPDATED avg.
 * lerp is torch's formula.  Without s2, update_avg and truncate the result is the broadcast of s, bit for bit.
 * update_avg or truncate without avg is SIVAE_ERR_NULL; a flag that is not 0 / 1 SIVAE_ERR_MODE. */
int sivae_styles_fwd(const float* s, const float* s2, int mix_cutoff, float* avg, int update_avg, float avg_weight,
                     int truncate, float psi, int trunc_cutoff, float* styles, int B, int L, int Z, sivae_stream_t stream);
/* Its backward (avg takes no gradient, as under the reference's no_grad): with c_l = psi for l < trunc_cutoff and 1 otherwise
 *   ds[b] = sum_{l < mix_cutoff} c_l dstyles[b][l];   ds2[b] = sum_{l >= mix_cutoff} c_l dstyles[b][l]   (ascending l)
 * has_s2 = 0: every layer belongs to ds (mix_cutoff is ignored) and a ds2 is SIVAE_ERR_MODE.  ds and ds2 may each be NULL. */
int sivae_styles_bwd(const float* dstyles, int has_s2, int mix_cutoff, int truncate, float psi, int trunc_cutoff, float* ds,
                     float* ds2, int B, int L, int Z, sivae_stream_t stream);

/* ---- the style variant's fused_scale convolutions (scale_conv.hip) --------------------------------------------------------
 * style_soft_intro_vae/net.py:77,:138 (transform_kernel=True, lreq.py:142-164): stride-2 convolutions over the 4x4 kernel
 * S(w) summed from four shifted copies of a 3x3 weight.  They are the 3x3 convolution of a nearest-2x upsampled input
 * ("up") and its adjoint ("down"), which sivae_conv2d_wino_up_fwd / _dgrad / _wgrad and their routes compute, on the weight
 *   T(w)[o][i][a][b] = w[i][o][2 - a][2 - b].
 * sivae_conv3x3_flip_transpose is T with a scale, one multiply per element (exact for 1 and 0.25):
 *   dst[s][r][2 - a][2 - b] = scale * src[r][s][a][b],   src [R][S][3][3], dst [S][R][3][3], src and dst not aliased.
 * Used both ways: parameter -> effective operand, and effective weight gradient -> the parameter's gradient.  Both
 * pointers may be any 4-byte-aligned address (SIVAE_ERR_SHAPE otherwise).  SIVAE_ERR_NULL for a missing pointer,
 * SIVAE_ERR_SHAPE for a non-positive size, SIVAE_ERR_RANGE for 9 R S > 2^31 - 1, all before any launch.  No workspace. */
int sivae_conv3x3_flip_transpose(const float* src, float* dst, int R, int S, float scale, sivae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIVAE_HIP_H */
