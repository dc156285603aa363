/*
 * mvldm.h -- C ABI of libmvldm_hip.so: the MI355X (gfx950) kernels behind the multi-view
 * latent-diffusion denoising path of mohammadasim98/mv-ldm.
 *
 * The reference has no FFI of its own (it is pure Python on top of torch + diffusers); the
 * "interface each entry point replaces" is therefore the Python call it stands in for, cited per
 * function as /root/reference path:line (or the diffusers==0.27.2 class the reference instantiates).
 * Plain pointers and sizes only: no torch types.  All pointers are DEVICE pointers unless marked
 * "host".  All entry points return 0 on success or a negative MVLDM_ERR_*; text via
 * mvldm_last_error().  Kernels are enqueued on the given hipStream_t and never synchronise,
 * allocate or free (graph-capture safe); scratch comes from caller-provided workspaces.
 *
 * Data layout: activations are NHWC ("token-major": [image][pixel][channel]) in the activation
 * dtype (bf16 / f16 / f32); weights are pre-packed [n_pad][k_pad] K-major in the activation dtype by
 * mvldm_pack_weight(); biases, norm affine parameters, statistics and the DDIM state are fp32.
 */
#ifndef MVLDM_H
#define MVLDM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3 (round 3): + mvldm_gather_rows, mvldm_ddpm_cfg_step, mvldm_ema_update; plan ops MVLDM_OP_PAR_BEGIN / _NEXT / _END and
 * MVLDM_OP_GATHER_ROWS / MVLDM_OP_ATTN_MERGE; bits 8-9 of mvldm_wgrad_desc.accumulate select the weight-gradient kernel form.  Everything of version 2 is
 * unchanged (additive).
 * 4 (round 5): + mvldm_pack_skinny and tile 15 / k_order 2 of mvldm_igemm_fwd (the skinny-M weight-streaming GEMM); additive over 3.
 * 5 (round 6): + tile 19 of mvldm_igemm_fwd (register-staged Linear), tile 13's bits 13 / 14, mvldm_build_flags; additive over 4.
 * 7: + mvldm_image_metrics, mvldm_image_metrics_workspace_bytes; additive over 6.
 *    + mvldm_lpips_prep / _relu / _tap / _fold, mvldm_lpips_workspace_bytes, mvldm_lpips_tap_slots (LPIPS around the implicit GEMM): new
 *    symbols only, no struct, enum or op kind changes, so the number stays 7.
 *    + mvldm_dists_prep / _stats / _l2pool / _fold, mvldm_dists_workspace_bytes, mvldm_dists_stat_slots (DISTS around the implicit GEMM):
 *    new symbols only again, the number stays 7.
 *    + mvldm_fid_prep / _pool / _accumulate / _compute, mvldm_fid_workspace_bytes, mvldm_fid_pool_slots (FID, feature = 64, around the
 *    implicit GEMM): new symbols only, the number stays 7.
 *    + mvldm_inception_prep / _unfold / _maxpool / _avgpool / _concat / _features, mvldm_inception_workspace_bytes, mvldm_frechet_accumulate /
 *    _compute, mvldm_frechet_workspace_bytes (Clean-FID: the whole Inception-v3 and a Frechet distance up to 2048 features): new symbols
 *    only, the number stays 7.
 *    + mvldm_kid_compute, mvldm_kid_workspace_bytes (Clean-KID: the subset Gram sums on the fp64 matrix cores): new symbols only, the number
 *    stays 7.
 *    + mvldm_crop_shim, mvldm_crop_shim_workspace_bytes, mvldm_crop_shim_axis (the dataset readers' crop shim): new symbols only, the
 *    number stays 7.
 *    + mvldm_crop_shim_flip (the crop shim with a per-image mirrored read, for the training loader's augmentation shim): new symbol only,
 *    the number stays 7.
 *    + mvldm_jpeg_probe / _entropy / _coef_count / _workspace_bytes / _decode / _idct_host (baseline JPEG frames: entropy decoding on the
 *    host, dequantisation, inverse DCT, upsampling and colour on the device): new symbols and enums only, the number stays 7.
 *    + mvldm_jpeg_scan_room / _scan_prepare / _entropy_chunk_subseqs / _entropy_device / _entropy_emul_host and the reason
 *    MVLDM_JPEG_RESTART (the Huffman scan decoded on the device): new symbols and one new enum value only, the number stays 7.
 *    + mvldm_png_unfilter / _unfilter_host and the MVLDM_PNG_* enums (PNG frames: inflate on the host, row unfiltering and colour expansion
 *    on the device): new symbols and enums only, the number stays 7.
 *    + mvldm_png_inflate / _inflate_host / _inflate_room (PNG frames: IDAT inflated on the device, opt-in): new symbols only, the number
 *    stays 7.
 *    + mvldm_jpeg_rst_room / _rst_need / _rst_prepare / _rst_entropy_device / _rst_entropy_emul_host (the Huffman scan of frames with
 *    restart intervals decoded on the device, opt-in): new symbols only, the number stays 7. */
#define MVLDM_ABI_VERSION 7

typedef void* mvldm_stream_t; /* hipStream_t */

enum { MVLDM_F32 = 0, MVLDM_BF16 = 1, MVLDM_F16 = 2 };
enum { MVLDM_OK = 0, MVLDM_ERR_ARG = -1, MVLDM_ERR_HIP = -2, MVLDM_ERR_UNSUPPORTED = -3 };

/* epilogue selector of the implicit GEMM */
enum { MVLDM_EPI_NONE = 0, MVLDM_EPI_SILU = 1, MVLDM_EPI_GEGLU = 2, MVLDM_EPI_GELU = 3 /* exact (erf) GELU: the ViT feed-forward of the
       "standard" multi-view block, src/model/transformer/feed_forward.py:31-40 */ };
/* elementwise op selector */
enum { MVLDM_ELT_COPY = 0, MVLDM_ELT_SILU = 1, MVLDM_ELT_GELU = 2 };

int mvldm_abi_version(void);
/* bit 0: the library was compiled with -DMVLDM_EXPERIMENTS (its kernels read the A/B environment knobs of tools/; the product build reads none) */
int mvldm_build_flags(void);
const char* mvldm_last_error(void);
/* cu_count / hbm_bytes of the current device; arch receives e.g. "gfx950" */
int mvldm_device_info(int* cu_count, size_t* hbm_bytes, char* arch, int arch_len);

/* ------------------------------------------------------------------------------------------------
 * Implicit GEMM: 3x3 / 1x1 convolution and Linear, one kernel family.
 *   replaces  torch.nn.Conv2d / torch.nn.Linear as called from diffusers ResnetBlock2D
 *             (conv1/conv2/conv_shortcut/time_emb_proj; mvunet.py:121,150,159,177), Downsample2D /
 *             Upsample2D (mvunet.py:145-148,198-200), conv_in/conv_out (mvunet.py:113,205),
 *             Transformer2DModel proj_in/proj_out + Attention to_q/k/v/to_out + GEGLU FF
 *             (mvunet.py:131-134,158), and SpatialTransformer3D proj_in/proj_out, CrossAttention
 *             projections, FeedForward (src/model/denoiser/mvdream/attention.py:60-87,174-205,416-439).
 *   out[m][n] = epi( sum_k A[m][k] * W[n][k] + bias[n] + row_bias[img(m)][n] ) * out_scale + residual[m][n]
 *   A is gathered on the fly from up to two NHWC sources concatenated along C (the UNet skip concat,
 *   mvunet.py:176, never materialised); k = (tap, channel); optional nearest x2 upsampling of the
 *   input (Upsample2D) and stride 2 (Downsample2D; pad=0 gives the VAE's asymmetric (0,1,0,1) pad).
 *   GEGLU: W rows are packed in alternating 32-row blocks [value | gate]; out has n_out/2 columns.
 */
typedef struct mvldm_igemm_desc {
    const void* src0;      /* [n_img][h_in][w_in][c0] */
    const void* src1;      /* [n_img][h_in][w_in][c1] or NULL */
    const void* weight;    /* packed [n_pad][k_pad], k_pad = roundup(ksize^2*(c0+c1), 128 bytes) */
    const float* bias;     /* [n_out] or NULL */
    const float* row_bias; /* [n_img][row_bias_ld] (time-embedding projection) or NULL */
    const void* residual;  /* [m][n_dst] activation dtype or NULL */
    void* dst;             /* [m][n_dst], n_dst = n_out (GEGLU: n_out/2) */
    float* workspace;      /* split-K scratch, >= splitk*m*n_pad floats when splitk > 1 */
    int32_t c0, c1;
    int32_t n_img, h_in, w_in, h_out, w_out;
    int32_t ksize, stride, pad, upsample;   /* ksize 1 | 3 (2 with upsample >= 2).  upsample: 0 none; 1 nearest-2x source
                                               indexing in front of a 3x3 conv (diffusers Upsample2D); 2 + 2*py + px = sub-pixel
                                               phase (py, px) of the same conv decomposed into four 2x2 convs on the LOW-resolution
                                               image (h_out = h_in, w_out = w_in; rows are scattered to (2i+py, 2j+px) of dst) */
    int32_t n_out, n_pad, k_pad;
    int32_t row_bias_ld;
    int32_t epilogue;   /* MVLDM_EPI_* */
    int32_t act_dtype;  /* dtype of src/weight/residual */
    int32_t dst_dtype;  /* act_dtype or MVLDM_F32 */
    int32_t splitk;     /* >= 1; 0 = let the library choose (needs workspace) */
    int32_t tile;       /* 0 = auto; else force a tile config (tests / tuning / plan-time selection): 1..11 implicit-GEMM tiles (igemm_small.hip: 1..5, igemm_large.hip: 6..8, igemm_xl.hip: 9..10, igemm_halo.hip: 11),
                           12 = persistent Linear with the epilogue pipelined under the next tile (linear_pp.hip: 1x1, one or two
                           sources, K >= 320 a multiple of 64, 16-bit in and out; any other problem is an error, not a fallback),
                           13 = persistent wide Linear (linear_pw.hip), 14 = weight-stationary Linear for K = 320 (linear_ws.hip),
                           17 = 256 x 320 tile with the pixel halo resident in LDS (igemm_halo.hip, round 5: one-source 3x3 / stride 1 / pad 1 convs
                                on maps up to 24 pixels wide; anything else runs as tile 7, same values),
                           18 = 192 x 128 tile with a 4-slot ring (igemm_xl.hip; 1x1 / 3x3, no upsampling forms, no GEGLU: refused),
                           19 = register-staged persistent Linear (linear_rs.hip, round 6: 256 x 256 tiles, 4 waves of 128 x 128, the K-steps in
                                flight held in registers; 1x1, one or two sources, K >= 256 a multiple of 128, 16-bit in and out, bias /
                                residual / GEGLU; any other problem is an error, not a fallback),
                           15 = skinny-M weight-streaming GEMM (skinny.hip, round 5: launches of a few hundred rows -- one scene at the
                                8x8 / 4x4 levels, mvunet.py:150-200 -- whose cost is the weight stream): `weight` is the FRAGMENT-ORDER
                                pack of mvldm_pack_skinny (k_order must be 2), whole K per workgroup, no split-K slab and no reduce launch;
                                1x1 / 3x3 (stride 1 or 2) / 2x2 phase convs, one or two sources, channels in multiples of 64, every
                                epilogue; bits 8-13 = its configuration (0 = rule; a configuration that does not fit is an error).
                           Bits 0-5 = the tile id; bits 8-11 / 12 = tuning overrides (XCD grid, register-prefetch loop); tile 13 only:
                           bit 13 = L2 prefetch of the activation rows, bit 14 = issue a K-step's LDS-DMA pieces in one burst behind its
                           barrier (the form before round 6; the default spreads them over three sub-steps -- same values, A/B) */
    int32_t k_order;    /* K order of the packed weight: 0 = (tap, channel); 1 = (64-channel block, tap, channel); 2 = the k_order-1
                           sequence in MFMA-fragment order (mvldm_pack_skinny; tile 15 only) */
    int32_t dst_ld;     /* row stride of dst in elements; 0 = n_dst (dense).  > n_dst writes into a wider buffer */
    float out_scale;
    size_t workspace_bytes;
} mvldm_igemm_desc;
int mvldm_igemm_fwd(const mvldm_igemm_desc* d, mvldm_stream_t stream);
/* bytes of split-K workspace the auto heuristic may use for this problem */
size_t mvldm_igemm_workspace_bytes(const mvldm_igemm_desc* d);

/* Pack a PyTorch-layout fp32 weight ([n_out][c_in][k][k] conv or [n_out][c_in] linear) into the
 * kernel layout: dst[n'][ (ky*k+kx)*c_pad + c ], zero padded to [n_pad][k_pad]; `geglu` != 0
 * interleaves rows n and n + n_out/2 in blocks of 32; `k_order` 1 stores k as (channel block of 64 [32 for
 * f32], tap, channel in block) so that the 9 taps of one channel block are consecutive K-tiles (their
 * activation reads hit L2 instead of crossing the fabric 9 times); needs c_pad % 64 == 0.  replaces: nothing in the reference (weights
 * there stay in torch layout); this is the one-time load-time transform.
 * `transpose` != 0 packs the weight of the DATA-GRADIENT convolution instead (backward of Conv2d / Linear w.r.t. its input):
 * rows are `n_rows` INPUT channels starting at `c_off` (a skip-concat conv yields two gradients: two packs), K runs over
 * (tap, output channel) with the taps flipped: dst[r][(tap', n)] = src[n][c_off + r][taps-1-tap']; c_pad then pads n_out,
 * n_pad pads n_rows. */
int mvldm_pack_weight(const float* src, void* dst, int n_out, int c_in, int ksize, int c_pad, int n_pad,
                      int k_pad, int geglu, int k_order, int dst_dtype, int transpose, int c_off, int n_rows,
                      mvldm_stream_t stream);

/* Re-order a K-major 16-bit pack made with k_order 1 (`packed`: [n_pad][k_pad], n_pad % 64 == 0, k_pad % 64 == 0) into the
 * fragment order tile 15 of mvldm_igemm_fwd streams: 16-byte unit ((nt * (k_pad/32) + kg) * 64 + lane) of dst =
 * packed[row(nt, lane & 15)][32 kg + 8 (lane >> 4) .. + 7], i.e. one v_mfma_f32_16x16x32 A-operand fragment (16 output columns x 32 k)
 * is 1 KB of consecutive bytes and a 16-column tile is one contiguous stream over K.  row(nt, r) = 16 nt + r, except for a GEGLU
 * pack (`geglu` != 0: rows alternate [32 value | 32 gate]) where tiles (2q, 2q+1) are the value / gate rows of output columns
 * 16 q .. 16 q + 15.  Same byte count as `packed`.  replaces: nothing in the reference (a load-time transform like mvldm_pack_weight). */
int mvldm_pack_skinny(const void* packed, void* dst, int n_pad, int k_pad, int geglu, int dtype, mvldm_stream_t stream);
/* Host-side query (no GPU work): the tile-15 configuration the library's rule picks for the problem `d` describes (pointers may be the
 * K-major ones: only shapes, dtypes, alignment and the epilogue are looked at), or 0 when tile 15 cannot compute it (an image larger than
 * a workgroup's row tiles, f32, channels that are not multiples of 64 ...).  Plan builders ask before they commit an op to tile 15. */
int mvldm_igemm_skinny_config(const mvldm_igemm_desc* d);

/* The same transform for MANY weights in one launch (round 3): after an optimizer step the training path re-packs every
 * trained weight (forward + data-gradient packs, ~380 of them) -- as one launch per pack these are latency-bound (7 ms for
 * 7.4 GB).  A job is the argument list of mvldm_pack_weight(); mvldm_pack_job_prepare() validates it and fills `kind`
 * and `blocks` (host side, no GPU work).  The caller sets `block0` = exclusive prefix sum of `blocks` over the job list,
 * copies the list to the device and passes it with `total_blocks` = the sum.  Output bytes are identical to n_jobs calls
 * of mvldm_pack_weight().  replaces: nothing in the reference (torch keeps one weight layout; its optimizer step is the
 * last touch). */
typedef struct mvldm_pack_job {
    const float* src; void* dst;
    int n_out, c_in, ksize, c_pad, n_pad, k_pad, geglu, k_order, transpose, c_off, n_rows;
    int kind;        /* filled by mvldm_pack_job_prepare: which packer body */
    int blocks;      /* filled by mvldm_pack_job_prepare: workgroups of this job */
    int block0;      /* caller: first workgroup of this job inside the batched launch */
} mvldm_pack_job;
int mvldm_pack_job_prepare(mvldm_pack_job* job /* host */, int dst_dtype);
/* `block_job` (device, total_blocks int32, may be NULL): the job index of every workgroup -- one load instead of a binary
 * search over the job list per workgroup (a workgroup moves only 4-18 KB). */
int mvldm_pack_weight_batch(const mvldm_pack_job* jobs /* device */, int n_jobs, const int32_t* block_job, int total_blocks,
                            int dst_dtype, mvldm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * GroupNorm (+ optional SiLU), NHWC.   replaces torch.nn.GroupNorm + SiLU in ResnetBlock2D
 * (norm1/norm2 + nonlinearity), conv_norm_out + conv_act (mvunet.py:203-204), Transformer2DModel.norm
 * and SpatialTransformer3D.norm (mvdream/attention.py:96-97,423).  Statistics in fp64.
 * The input may be the channel concatenation of two tensors x0 [.., c0] | x1 [.., c1] (x1 NULL, c1 0
 * otherwise): the up-path skip concat (mvunet.py:176) feeds norm1 directly and is never materialised;
 * groups are taken over the concatenated c0+c1 channels and y is [n_img][hw][c0+c1].
 * stats_ws: >= n_img * MVLDM_GN_MAX_CHUNKS * groups * 2 doubles.
 * stats_out (optional): fp32 [n_img][groups][2] = (mean, rstd), saved for mvldm_groupnorm_bwd.
 */
#define MVLDM_GN_MAX_CHUNKS 32
int mvldm_groupnorm_fwd(const void* x0, const void* x1, void* y, const float* gamma, const float* beta, int n_img,
                        int hw, int c0, int c1, int groups, float eps, int silu, int dtype, void* stats_ws,
                        float* stats_out, mvldm_stream_t stream);
/* how many times that call moves the tensor over HBM: 2 (one launch, the (image, channel-span) slab stays in registers:
 * 1 read + 1 write) or 3 (statistics launch + apply launch: 2 reads + 1 write).  Host-side query (no GPU work) for the
 * byte accounting of plans and benches. */
int mvldm_groupnorm_passes(int n_img, int hw, int c, int groups, int dtype);

/* LayerNorm over the last dim of [rows][c].  replaces torch.nn.LayerNorm in BasicTransformerBlock
 * (diffusers) and BasicTransformerBlock3D norm1-3 (mvdream/attention.py:286-288,363-367). */
int mvldm_layernorm_fwd(const void* x, void* y, const float* gamma, const float* beta, int rows, int c, float eps,
                        int dtype, mvldm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Attention: out = softmax(q k^T * scale) v per (segment, head), flash-style (scores never leave
 * the chip), fp32 online softmax, QK^T accumulated in fp32 (ATTN_PRECISION=fp32,
 * mvdream/attention.py:20,185-188).   replaces CrossAttention.forward core
 * (mvdream/attention.py:180-203: the 3-D attention over all views' tokens and the per-view
 * attention) and diffusers Attention's F.scaled_dot_product_attention.
 * q/k/v/out are row-major token matrices; head h occupies columns [h*head_dim, (h+1)*head_dim);
 * ld_* are row strides in elements, so q/k/v may alias one fused [tokens][3C] projection.
 * seg: device int32 [n_seg][4] = {q_row0, q_len, kv_row0, kv_len}.
 * lse (optional): fp32 [heads][lse_ld], entry [h][q row] = log2-domain log-sum-exp of the scaled scores of query row
 * `q row` (P = exp2(s * scale * log2(e) - lse)): saved for mvldm_attention_bwd.
 */
int mvldm_attention_fwd(const void* q, const void* k, const void* v, void* out, int ld_q, int ld_k, int ld_v,
                        int ld_o, int heads, int head_dim, const int32_t* seg, int n_seg, int max_q_len,
                        float scale, int dtype, float* lse, int lse_ld, mvldm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Sinusoidal timestep projection.   replaces diffusers Timesteps(320, flip_sin_to_cos=True, shift 0)
 * (mvunet.py:107).  out[i] = [cos(t_i * f) | sin(t_i * f)] (flip) or [sin | cos]; freqs: fp32 [dim/2]
 * table built on the host exactly as the reference does (exp(-ln(10000) * j / half)).
 */
int mvldm_timestep_embed_fwd(const int64_t* timesteps, const float* freqs, void* out, int n, int dim,
                             int flip_sin_to_cos, int dst_dtype, mvldm_stream_t stream);

/* elementwise y = f(x) with dtype conversion; n elements.  SiLU on the time embedding
 * (ResnetBlock2D: time_emb_proj(nonlinearity(temb))). */
int mvldm_eltwise_fwd(const void* x, void* y, size_t n, int op, int src_dtype, int dst_dtype, mvldm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fused classifier-free-guidance compose + DDIM update (eta = 0, epsilon prediction).
 *   replaces  DiffusionWrapper.step's tail (src/model/diffusion_wrapper.py:444,451-453) and
 *             diffusers DDIMScheduler.step.
 *   eps  = eps_u + cfg_scale * (eps_c - eps_u)            (use_cfg) | eps_c
 *   x0   = (x - sqrt(1-a_t) * eps) / sqrt(a_t);  x' = sqrt(a_prev) * x0 + sqrt(1-a_prev) * eps
 * evaluated in fp32 with separately rounded mul/add/div in exactly that order (bit-identical to
 * the torch CPU fp32 expression given the same eps).
 * eps: fp32 NHWC [n_img_total][hw][c]; x_t / x_next: fp32 NHWC [n_tgt][hw][c];
 * cond_img / uncond_img: device int32 [n_tgt] image index of target view t in the conditional /
 * unconditional pass (uncond_img NULL => no CFG).
 * coef: device fp32 [n_steps][4] = {sqrt(1-a_t), sqrt(a_t), sqrt(a_prev), sqrt(1-a_prev)}; step_ptr:
 * device int32 current step index (read only here; advanced by mvldm_ddim_advance) so that one
 * captured graph serves every step.
 * If unet_in != NULL the new latents are also scattered (activation dtype) into channels [0,c) of
 * the UNet input rows cond_img[t] and uncond_img[t] ([n_img_total][hw][unet_in_c]).
 * n_steps: rows of coef (the step index is clamped to [0, n_steps-1], so a replay past the end of the
 * schedule never reads out of bounds).  clip_range > 0: diffusers `clip_sample=True` --
 * x0 = clamp(x0, -clip_range, clip_range) before the update (`clip_sample_range`, default 1.0); 0 = off
 * (the released config, config/model/scheduler/ddim.yaml:9).
 */
int mvldm_ddim_cfg_step(const float* eps, const float* x_t, float* x_next, const int32_t* cond_img,
                        const int32_t* uncond_img, int n_tgt, int hw, int c, float cfg_scale, const float* coef,
                        const int32_t* step_ptr, void* unet_in, int unet_in_c, int unet_in_dtype, int n_steps,
                        float clip_range, mvldm_stream_t stream);
/* SCHEDULER["ddpm"].step (src/model/scheduler/__init__.py:19-22; called at diffusion_wrapper.py:451 when the config names the DDPM
 * scheduler): diffusers' DDPMScheduler.step for epsilon prediction with variance_type "fixed_small", optionally behind the CFG compose
 * of diffusion_wrapper.py:444 (eps_u NULL => no CFG), on flat fp32 arrays of n elements:
 *   e = eps_u + cfg_scale (eps_c - eps_u);  x0 = (x_t - coef[0] e) / coef[1];  [x0 = clamp(x0, +-clip_range) if clip_range > 0];
 *   x_next = coef[2] x0 + coef[3] x_t + coef[4] noise
 * coef (device fp32 [5]) = {sqrt(1-a_t), sqrt(a_t), sqrt(a_prev) b_t / (1-a_t), sqrt(alpha_t) (1-a_prev) / (1-a_t), sqrt(variance)};
 * the host passes coef[4] = 0 at t = 0, where diffusers adds no noise (noise may then be NULL).  Separately rounded fp32 operations in
 * diffusers' order: bit-identical to the torch CPU expression given the same inputs. */
int mvldm_ddpm_cfg_step(const float* eps_c, const float* eps_u, const float* x_t, const float* noise, float* x_next, size_t n,
                        float cfg_scale, const float* coef, float clip_range, mvldm_stream_t stream);
/* step_ptr += 1; timesteps[tgt_rows[i]] = t_table[min(step, n_steps-1)] for i < n_rows (the
 * per-image timestep vector the UNet reads: context views stay at 0, diffusion_wrapper.py:419-428) */
int mvldm_ddim_advance(int32_t* step_ptr, const int64_t* t_table, int n_steps, int64_t* timesteps,
                       const int32_t* tgt_rows, int n_rows, mvldm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Layout plumbing at the boundary: NCHW fp32 <-> NHWC activation dtype with channel offset/padding.
 *   replaces the torch.concat input assembly of DiffusionWrapper.step / .sample
 *   (diffusion_wrapper.py:429-432,476-481), the `inputs * 2.0 - 1.0` / `(1 / 0.18215) * latents` /
 *   `(image / 2 + 0.5).clamp(0, 1)` arithmetic around the VAE (:281,293,298).
 * nchw_to_nhwc: dst[img_map ? img_map[i] : i][pix][dst_c_off + ch] = src[i][ch][pix] * scale + shift
 *   (img_map: device int32 [n_img] or NULL).
 */
int mvldm_nchw_to_nhwc(const float* src, void* dst, int n_img, int c, int hw, int dst_c, int dst_c_off,
                       int dst_dtype, float scale, float shift, const int32_t* img_map, mvldm_stream_t stream);
int mvldm_nhwc_to_nchw(const void* src, float* dst, int n_img, int c, int hw, int src_c, int src_c_off,
                       int src_dtype, float scale, float shift, int clamp01, mvldm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Camera ray grid of the latent image.   replaces DiffusionWrapper.ray_encode with the raw [origin | direction]
 * encoding (diffusion_wrapper.py:301-322, generate_image_rays :169-190; src/geometry/projection.py:74-138:
 * sample_image_grid, unproject, get_world_rays).  extrinsics: fp32 [n_cam][4][4] camera-to-world;
 * intrinsics: fp32 [n_cam][3][3] normalised.  Per latent pixel (i, j): xy = ((j+.5)/w, (i+.5)/h),
 * d = normalize(K^-1 [x y 1]), direction = R d, origin = translation.  Outputs (either may be NULL):
 * out_nchw fp32 [n_cam][C][h*w]; out_nhwc: channels [nhwc_c_off, +C) of an NHWC buffer [..][h*w][nhwc_c]
 * in nhwc_dtype, camera i -> image img_map[i] (NULL: i).
 * Encodings of the (origin, direction) pair (diffusion_wrapper.py:98-127,301-322):
 *   MVLDM_RAYS_RAW        [o | d]: 6 channels (the released config: use_ray_encoding = srt_ray_encoding = false)
 *   MVLDM_RAYS_POSITIONAL src/model/encodings/positional_encoding.py:8-36 on o (n_origin_octaves) then d (n_dir_octaves):
 *                         per coordinate, per octave f: sin(x * 2 pi 2^f), sin(x * 2 pi 2^f + pi/2); 6 * octaves channels each
 *                         (0 octaves: that part is passed through raw, `nn.Identity`)
 *   MVLDM_RAYS_SRT        src/model/srt/layers.py:11-58 (RayEncoder): [sin(o 2^f pi) | cos(o 2^f pi) | sin(d 2^f pi) | cos(...)]
 * plucker != 0: o is replaced by o x d first (diffusion_wrapper.py:309-310).  The channel count is mvldm_ray_channels().
 */
enum { MVLDM_RAYS_RAW = 0, MVLDM_RAYS_POSITIONAL = 1, MVLDM_RAYS_SRT = 2 };
int mvldm_ray_channels(int mode, int n_origin_octaves, int n_dir_octaves);
int mvldm_ray_encode(const float* extrinsics, const float* intrinsics, int n_cam, int h, int w, float* out_nchw,
                     void* out_nhwc, int nhwc_c, int nhwc_c_off, int nhwc_dtype, const int32_t* img_map, int mode,
                     int n_origin_octaves, int n_dir_octaves, int plucker, mvldm_stream_t stream);

/* AutoencoderKL.encode(x).latent_dist.sample() * scale (diffusion_wrapper.py:283; diffusers
 * DiagonalGaussianDistribution): moments fp32 NCHW [n][2c][hw] = [mean | logvar], noise / out fp32 [n][c][hw];
 * out = (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise) * scale. */
int mvldm_posterior_sample(const float* moments, const float* noise, float* out, int n, int c, int hw, float scale,
                           mvldm_stream_t stream);

/* ================================================================================================
 * Training: the backward kernels of the same path.   replaces torch.autograd through
 * MultiViewUNet.forward inside DiffusionWrapper.training_step (src/model/diffusion_wrapper.py:324-411:
 * add_noise :370, denoiser.forward :401, F.mse_loss :405-411) and the optimizer step Lightning drives for it
 * (configure_optimizers :1111-1122: AdamW lr 2e-5 + LinearLR warm-up, config/experiment/baseline.yaml:62-73;
 * Trainer(gradient_clip_val=0.1, accumulate_grad_batches=2), src/main.py:119-136, config/main.yaml:82-84).
 * Data gradients of convolutions / Linears are mvldm_igemm_fwd on weights packed with `transpose` (above).
 * ================================================================================================ */

/* Weight gradient of a convolution / Linear: grad[n][c][ky][kx] (PyTorch fp32 layout; [n][c] for a Linear)
 *   = / += sum over output pixels m of dy[m][n] * A[m][(tap, c)], A = the forward pass's on-the-fly gather
 * (two sources concatenated along C, stride, zero padding, nearest-2x upsampling: same fields as mvldm_igemm_desc).
 * dy: [m][dy_ld] activation dtype, columns [0, n_out) used -- a column slice of a wider matrix (fused QKV / all
 * time_emb_proj at once) is addressed by offsetting the pointer.  c_in <= c0 + c1: padding channels of the gather
 * (conv_in: 11 -> 16) are dropped from grad.  workspace: fp32 split-K slabs, >= n_out * ksize^2 * (c0+c1) * 4 bytes
 * (more lets small layers split the pixel range over more workgroups); reduced in a fixed order: deterministic. */
typedef struct mvldm_wgrad_desc {
    const void* src0; const void* src1; const void* dy;
    float* grad;
    float* workspace; size_t workspace_bytes;
    int32_t c0, c1, c_in;
    int32_t n_img, h_in, w_in, h_out, w_out;
    int32_t ksize, stride, pad, upsample;      /* upsample: 0 | 1 (nearest-2x gather in front of a 3x3 conv) */
    int32_t n_out, dy_ld;
    int32_t act_dtype;
    int32_t accumulate;                        /* bit 0: 0 grad = ..., 1 grad += ... (accumulation over micro-batches);
                                                * bits 8-9: kernel form, 0 = the library's rule, 1 = register-staged [128 n x 64 c] tile,
                                                * 2 = wide LDS-DMA [320 n x 128 c] tile (refused where it does not apply);
                                                * bits 10-12: workgroup target of the pixel split, 0 = the library's, else 64 << code */
} mvldm_wgrad_desc;
int mvldm_igemm_wgrad(const mvldm_wgrad_desc* d, mvldm_stream_t stream);

/* Column sums of a [n_seg * rows_per_seg][ld] activation matrix, columns [0, n): bias gradients (per_seg = 0:
 * dst[n] (+)= sum over all rows) and the gradient of the per-image time-embedding row added by ResnetBlock2D
 * (per_seg = 1: dst[seg][n] (ld_dst) (+)= sum over the rows of image seg).  workspace: fp32, 16-byte aligned,
 * >= (1024 + n_seg) * roundup(n, 8) floats. */
int mvldm_colsum(const void* x, float* dst, float* workspace, size_t workspace_bytes, int n_seg, int rows_per_seg, int n,
                 int ld, int ld_dst, int per_seg, int accumulate, int dtype, mvldm_stream_t stream);

/* GroupNorm(+SiLU) backward (NHWC, optional two-source concat input as in the forward): dx0 / dx1 written,
 * dgamma / dbeta ACCUMULATED (+=) -- or WRITTEN (=) when `silu` (here) / `dtype` (mvldm_layernorm_bwd) carries
 * MVLDM_NORM_BWD_STORE: the first write of an accumulation window needs no zeroed gradient.  stats: the forward's stats_out.  workspace: fp32,
 * >= n_img * (MVLDM_GN_MAX_CHUNKS * (c0+c1) + groups) * 2 floats, 16-byte aligned. */
#define MVLDM_NORM_BWD_STORE 0x100
int mvldm_groupnorm_bwd(const void* x0, const void* x1, const void* dy, void* dx0, void* dx1, const float* gamma,
                        const float* beta, const float* stats, float* dgamma, float* dbeta, int n_img, int hw, int c0,
                        int c1, int groups, int silu, int dtype, float* workspace, size_t workspace_bytes,
                        mvldm_stream_t stream);
/* LayerNorm backward over [rows][c]: dx written, dgamma / dbeta accumulated.  workspace: fp32, >= 512 * c * 2 floats, 16-byte aligned. */
int mvldm_layernorm_bwd(const void* x, const void* dy, void* dx, const float* gamma, float* dgamma, float* dbeta,
                        int rows, int c, float eps, int dtype, float* workspace, size_t workspace_bytes,
                        mvldm_stream_t stream);

/* Flash-attention backward (probabilities recomputed from `lse`; see mvldm_attention_fwd for the layout conventions).
 * dq/dk/dv may be column slices of one [tokens][3C] gradient of a fused QKV projection.  delta: fp32 scratch
 * [heads][stat_ld] (written here: sum_d dout * out per query row); lse: [heads][stat_ld] from the forward.
 * total_q_rows: number of query rows covered by the segments (rows 0 .. total_q_rows-1 of q/out/dout). */
typedef struct mvldm_attn_bwd_desc {
    const void* q; const void* k; const void* v; const void* out; const void* dout;
    void* dq; void* dk; void* dv;
    const float* lse; float* delta;
    const int32_t* seg;
    int32_t ld_q, ld_k, ld_v, ld_o, ld_do, ld_dq, ld_dk, ld_dv;
    int32_t heads, head_dim, n_seg, max_q_len, max_kv_len, total_q_rows, stat_ld, dtype;
    float scale;
} mvldm_attn_bwd_desc;
int mvldm_attention_bwd(const mvldm_attn_bwd_desc* d, mvldm_stream_t stream);

/* Elementwise training ops on [rows][d] activation matrices:
 *   MVLDM_TE_SILU_BWD   out = b * silu'(a)                      (a: pre-activation, dtype a_dtype; b: upstream gradient)
 *   MVLDM_TE_ADD        out += a                                 (gradient accumulation; b unused)
 *   MVLDM_TE_GEGLU_FWD  out[rows][d] = a[:, :d] * gelu(a[:, d:])            (a: [rows][2d]; diffusers GEGLU / mvdream attention.py:60-73)
 *   MVLDM_TE_GEGLU_BWD  out[rows][2d] = d/da of the above times b[rows][d]
 *   MVLDM_TE_GELU_BWD   out = b * gelu'(a)                      (a: pre-activation) */
enum { MVLDM_TE_SILU_BWD = 0, MVLDM_TE_ADD = 1, MVLDM_TE_GEGLU_FWD = 2, MVLDM_TE_GEGLU_BWD = 3, MVLDM_TE_GELU_BWD = 4 };
int mvldm_train_eltwise(int op, const void* a, const void* b, void* out, size_t rows, int d, int a_dtype, int dtype,
                        mvldm_stream_t stream);
/* backward of nearest-2x upsampling: dx[n][i][j][c] = sum of the 2x2 block of du [n][2h][2w][c] */
int mvldm_pool2x2_sum(const void* du, void* dx, int n_img, int h, int w, int c, int dtype, mvldm_stream_t stream);
/* backward of a stride-2 subsampling: out [n][2h][2w][c] = x [n][h][w][c] at the even positions, zero elsewhere */
int mvldm_zero_insert2x(const void* x, void* out, int n_img, int h, int w, int c, int dtype, mvldm_stream_t stream);

/* DDIMScheduler.add_noise (diffusion_wrapper.py:370) fused with the UNet-input assembly: channels [dst_c_off, +c) of NHWC
 * image img_map[i] = sqrt(a_t) * x0[i] + sqrt(1 - a_t) * noise[i]; x0 / noise fp32 NCHW [n][c][hw], coef fp32 [n][2]. */
int mvldm_add_noise(const float* x0, const float* noise, const float* coef, void* dst, int n, int c, int hw, int dst_c,
                    int dst_c_off, int dst_dtype, const int32_t* img_map, mvldm_stream_t stream);
/* F.mse_loss(pred[:, v_c:], noise, reduction="mean") (diffusion_wrapper.py:405-411) and its gradient: pred fp32 NHWC
 * [n_img][hw][c]; target t is image tgt_img[t]; noise fp32 NCHW [n_tgt][c][hw].  loss[0] (+)= loss_scale * mean;
 * dpred (optional, [n_img][hw][dpred_c], zero-filled by the caller) = grad_scale * 2 (pred - noise) / N at the target
 * images.  workspace: 256 doubles. */
int mvldm_mse_loss(const float* pred, const float* noise, const int32_t* tgt_img, int n_tgt, int hw, int c, float* loss,
                   int accumulate, float loss_scale, void* dpred, int dpred_c, int dpred_dtype, float grad_scale,
                   double* workspace, mvldm_stream_t stream);

/* ---- f16 dynamic loss scaling (torch.amp.GradScaler under Lightning's `16-mixed`) ----------------------------------
 * The whole scaler lives in ONE device record owned by the trainer; recorded plans and graph replays hold its address,
 * never its values, so the scale S can change while they stay recorded.  One optimizer step with the scaler:
 *   backward (dY of the loss carries S) -> mvldm_grad_norm_amp (norm of the UNSCALED gradients, found_inf)
 *   -> mvldm_adamw_step_amp (skips the whole update when found_inf) -> mvldm_amp_update (one launch). */
typedef struct mvldm_amp_state {
    float scale;              /* S: dY of the loss and therefore every fp32 weight gradient carries it */
    int32_t growth_tracker;   /* successful steps since the last change of S (torch's _growth_tracker) */
    int32_t adam_step;        /* AdamW steps TAKEN (bias correction); does not advance on a skipped step */
    int32_t found_inf;        /* set by mvldm_grad_norm_amp, cleared by mvldm_amp_update */
    int32_t skipped;          /* optimizer steps skipped so far */
    int32_t reserved[3];
} mvldm_amp_state;
/* mvldm_mse_loss with dpred additionally multiplied by *amp_scale (device, fp32: the S of mvldm_amp_state) before the
 * rounding to dpred_dtype; the loss itself stays unscaled.  amp_scale NULL: exactly mvldm_mse_loss.  (Not to be confused
 * with loss_scale, the 1/accumulate factor of the reported loss.) */
int mvldm_mse_loss_amp(const float* pred, const float* noise, const int32_t* tgt_img, int n_tgt, int hw, int c, float* loss,
                       int accumulate, float loss_scale, void* dpred, int dpred_c, int dpred_dtype, float grad_scale,
                       const float* amp_scale, double* workspace, mvldm_stream_t stream);

/* torch.nn.utils.clip_grad_norm_ over a flat fp32 gradient buffer (Lightning gradient_clip_val, src/main.py:131):
 * norm_out[0] = total norm, norm_out[1] = min(1, max_norm / (total + 1e-6)) (max_norm <= 0: 1), norm_out[2] = this
 * buffer's sum of squares.  sumsq_in (optional, device): use this total sum of squares instead (a sharded optimizer
 * all-reduces the per-rank norm_out[2] first).  workspace: 1024 doubles.  g: 16-byte aligned when n >= 4 (it is read in
 * 16-byte vectors), else MVLDM_ERR_ARG and nothing is launched. */
int mvldm_grad_norm(const float* g, size_t n, const float* sumsq_in, float max_norm, float* norm_out, double* workspace,
                    mvldm_stream_t stream);
/* torch.optim.AdamW step (decoupled weight decay, no amsgrad) on flat fp32 master parameters:
 * g' = g * grad_scale * clip[1] (clip optional: norm_out of mvldm_grad_norm); step >= 1 is the 1-based step count. */
int mvldm_adamw_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                     float weight_decay, int step, float grad_scale, const float* clip, mvldm_stream_t stream);
/* mvldm_grad_norm on gradients that carry the loss scale S of `amp` (device): the squares are summed in fp64 and the sum
 * multiplied by 1/S^2 there, so norm_out[0..2] are the UNSCALED total norm, clip coefficient (the coefficient of
 * clip_grad_norm_ after GradScaler.unscale_) and this buffer's sum of squares -- a large but finite scaled gradient never
 * overflows the fp32 norm_out[2].  sumsq_in, when given, is taken as already unscaled.  amp->found_inf = the total sum of
 * squares is not finite (under ZeRO-1 sumsq_in is the all-reduced value, identical on every rank: every rank decides alike). */
int mvldm_grad_norm_amp(const float* g, size_t n, const float* sumsq_in, float max_norm, float* norm_out, mvldm_amp_state* amp,
                        double* workspace, mvldm_stream_t stream);
/* mvldm_adamw_step with the step taken from the device: amp->found_inf set -> p, m, v untouched; otherwise
 * g' = g * grad_scale * clip[1] / S and the bias correction uses step amp->adam_step + 1 (mvldm_amp_update advances it). */
int mvldm_adamw_step_amp(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                         float weight_decay, float grad_scale, const float* clip, const mvldm_amp_state* amp, mvldm_stream_t stream);
/* torch._amp_update_scale_ on the record, one thread: found_inf -> S *= backoff_factor, growth_tracker = 0, skipped += 1;
 * else growth_tracker += 1, adam_step += 1 and, when growth_tracker reaches growth_interval, S *= growth_factor (if that is
 * finite) and growth_tracker = 0.  found_inf is cleared.  "Reaches" is >=: a tracker already above the interval (a record
 * resumed under a shorter one) grows at its next taken step, where torch's == would never grow again. */
int mvldm_amp_update(mvldm_amp_state* amp, float growth_factor, float backoff_factor, int growth_interval, mvldm_stream_t stream);

/* DiffusionWrapper.on_before_zero_grad -> self.ema.update_parameters(self.denoiser) (diffusion_wrapper.py:138-142,152-154):
 * torch.optim.swa_utils.AveragedModel with get_ema_multi_avg_fn(0.995), i.e. avg.lerp_(p, weight) with weight = 1 - decay, on the flat
 * fp32 parameter buffer (the first update is a plain copy, done by the caller).  avg += weight (p - avg), torch's lerp arithmetic. */
int mvldm_ema_update(float* avg, const float* p, size_t n, float weight, mvldm_stream_t stream);

/* dst row (dst_index ? dst_index[k] : k) = src row (src_index ? src_index[k] : k), k < n_rows; rows of row_bytes bytes (a multiple of
 * 16); src and dst may be the same buffer as long as no destination row is also a source row.  Used by the fused CFG forward: the
 * unconditional pass of DiffusionWrapper.step (diffusion_wrapper.py:437-441) feeds the target views the SAME latents, mask, rays and
 * timestep as the conditional pass, the context views never change during sampling, and every layer before the first multi-view
 * attention block works per image -- those layers run once per step on the target views (and once per sample on the context views)
 * and the feature maps are copied to the rows that need them (mv_ldm_amd/mvunet.py, `dup`). */
int mvldm_gather_rows(const void* src, void* dst, const int32_t* src_index, const int32_t* dst_index, int n_rows, size_t row_bytes,
                      mvldm_stream_t stream);

/* Merge two softmax-attention results of the SAME queries over DISJOINT key sets (the flash-attention combine): with the
 * log-sum-exp outputs of mvldm_attention_fwd (log2 domain, [heads][lse_ld]) lse = log2(2^lse_a + 2^lse_b) and
 * out = oa 2^(lse_a - lse) + ob 2^(lse_b - lse), per head.  Rows are addressed per image of `tokens` rows: image k of the merge reads
 * rows a_img[k] * tokens + t of oa / lse_a, b_img[k] * tokens + t of ob / lse_b and writes row out_img[k] * tokens + t of out (out may
 * be oa or ob when the image maps keep reads and writes of different k apart).  Used in the first multi-view block of the fused CFG
 * forward: the target views' queries and keys are identical in the conditional and the unconditional pass there, so their scores over
 * the target keys are computed once (the unconditional result) and the conditional result adds the context views' keys
 * (mvdream/attention.py:174-205 evaluated once for both passes of diffusion_wrapper.py:435-441). */
int mvldm_attention_merge(const void* oa, const float* lse_a, const void* ob, const float* lse_b, void* out, const int32_t* a_img,
                          const int32_t* b_img, const int32_t* out_img, int n_img, int tokens, int heads, int head_dim, int ld_a, int ld_b,
                          int ld_o, int lse_ld_a, int lse_ld_b, int dtype, mvldm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Image metrics: PSNR and SSIM of n_img image pairs, fp32 NCHW [n_img][c][h][w] contiguous (what last_stage_decode returns and
 * the batches carry), one launch plus a fold; psnr[n_img], ssim[n_img] fp32.
 *   replaces  compute_psnr (src/evaluation/metrics.py:17-24): both images clipped to [0, 1], -10 log10(mean squared difference
 *             over c h w); identical images give +inf;
 *             compute_ssim (src/evaluation/metrics.py:58-73): skimage.metrics.structural_similarity(win_size=11,
 *             gaussian_weights=True, channel_axis=0, data_range=1.0) per image, NOT clipped: Gaussian taps of sigma 1.5 (11, normalised),
 *             S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)), C1 = 1e-4, C2 = 9e-4, variances scaled by 121/120 when
 *             use_sample_covariance != 0 (skimage's default), averaged over the map cropped by 5 pixels per side and over channels.
 * The sums are fp64 partials in `workspace` (mvldm_image_metrics_workspace_bytes; 0 for a refused shape), folded in a fixed order:
 * no atomics, bit-identical from run to run, and an image's scores do not depend on n_img or its position.  Refused: h or w < 11,
 * c < 1, a null pointer, a workspace that is too small. */
size_t mvldm_image_metrics_workspace_bytes(int n_img, int c, int h, int w);
int mvldm_image_metrics(const float* pred, const float* gt, int n_img, int c, int h, int w, int use_sample_covariance, float* psnr,
                        float* ssim, double* workspace, size_t workspace_bytes, mvldm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * LPIPS: the glue between the thirteen 3x3 convolutions of LPIPS(net="vgg")'s VGG-16 trunk (mvldm_igemm_fwd, with their bias) and
 * the per-pixel distance.
 *   replaces  compute_lpips (src/evaluation/metrics.py:43-54): lpips.LPIPS(net="vgg").forward(ground_truth, predicted,
 *             normalize=True)[:, 0, 0, 0] -- the package's ScalingLayer, vgg16.features slices relu1_2 / 2_2 / 3_3 / 4_3 / 5_3,
 *             normalize_tensor (x / (sqrt(sum_c x^2) + 1e-10)), the 1x1 `lin` layers and spatial_average, summed over the five taps.
 * A pair batch is 2 n_img NHWC images in the compute dtype `dtype`: rows [0, n_img) the first input, rows [n_img, 2 n_img) the
 * second.  All four run eagerly on `stream`, never synchronise or allocate, and refuse on the host before any launch (src/evaluation/metrics.py:43-54
 * for each):
 *   mvldm_lpips_prep   in0, in1: fp32 NCHW [n_img][3][h][w] -> dst NHWC [2 n_img][h][w][c_pad], x' = ((2x - 1) - shift_c) / scale_c
 *                      with shift = (-.030, -.088, -.188), scale = (.458, .448, .450); the 2x - 1 only when normalize != 0; inputs not
 *                      clipped; c_pad = 4 (f32) / 8 (16 bit), the pad channels zero.  Refused: h or w < 16 (four pool stages need one
 *                      pixel left), a null pointer.
 *   mvldm_lpips_relu   in-place ReLU of n elements (a multiple of the 16-byte chunk): after the convs that are no tap.
 *   mvldm_lpips_tap    feat: the PRE-activation output [2 n_img][h][w][c] of a stage's last conv; weight: fp32 [c], the stage's lin
 *                      layer.  Per pixel of pair i, with a = relu(feat[i]), b = relu(feat[n_img + i]), na = sqrt(sum_c a_c^2):
 *                      d = sum_c weight_c (a_c / (na + 1e-10) - b_c / (nb + 1e-10))^2, summed in fp32 over channels and a wave's pixels,
 *                      then in fp64: workgroup k of image i writes workspace[i * slots_per_image + slot0 + k], k <
 *                      mvldm_lpips_tap_slots(h, w, c) (no atomics: the same bits on every run, for every n_img and position).
 *                      pooled (may be null): the 2x2 max-pooled ReLU map [2 n_img][h / 2][w / 2][c]; a last odd row / column is not
 *                      pooled and still counts in d.  Refused: c no multiple of 64 or > 512, a workspace that is too small, a null pointer.
 *   mvldm_lpips_fold   out[i] (fp32) = sum over the taps l = 0..4 of (sum of tap l's partials of image i) / ((h >> l)(w >> l)), for
 *                      the layout mvldm_lpips_workspace_bytes(n_img, h, w) describes: per image the slots of tap 0 (h x w, 64
 *                      channels), tap 1 (h/2 x w/2, 128), tap 2 (256), tap 3 (512), tap 4 (512), in this order.
 * mvldm_lpips_workspace_bytes is 0 for a refused shape (n_img < 1, h or w < 16), mvldm_lpips_tap_slots for a refused map or c. */
size_t mvldm_lpips_workspace_bytes(int n_img, int h, int w);
int mvldm_lpips_tap_slots(int h, int w, int c);
int mvldm_lpips_prep(const float* in0, const float* in1, void* dst, int n_img, int h, int w, int c_pad, int dtype, int normalize,
                     mvldm_stream_t stream);
int mvldm_lpips_relu(void* x, size_t n, int dtype, mvldm_stream_t stream);
int mvldm_lpips_tap(const void* feat, const float* weight, void* pooled, int n_img, int h, int w, int c, int dtype, double* workspace,
                    size_t workspace_bytes, int slot0, int slots_per_image, mvldm_stream_t stream);
int mvldm_lpips_fold(const double* workspace, size_t workspace_bytes, int n_img, int h, int w, float* out, mvldm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * DISTS: the glue between the thirteen 3x3 convolutions of DISTS' VGG-16 trunk (mvldm_igemm_fwd, with their bias; the ReLU after the
 * convs that are no tap is mvldm_lpips_relu) and the structure / texture statistics.
 *   replaces  compute_dists (src/evaluation/metrics.py:27-40): DISTS_pytorch.DISTS().forward(ground_truth, predicted) -- the trunk
 *             input (x - mean) / std, vgg16.features cut after relu1_2 / 2_2 / 3_3 / 4_3 / 5_3 with an L2pooling in place of every
 *             max-pool, and per channel of the six taps (the raw image, then the five stages; 3 + 64 + 128 + 256 + 512 + 512 = 1475
 *             channels) S1 = (2 mx my + c1) / (mx^2 + my^2 + c1), S2 = (2 cov + c2) / (vx + vy + c2), c1 = c2 = 1e-6, means over the
 *             map's pixels; score = 1 - sum_c (alpha_c S1_c + beta_c S2_c) / (sum alpha + sum beta).
 * A pair batch is 2 n_img NHWC images in the compute dtype `dtype`: rows [0, n_img) the first input, rows [n_img, 2 n_img) the
 * second.  All four run eagerly on `stream`, never synchronise or allocate, and refuse on the host before any launch
 * (src/evaluation/metrics.py:27-40 for each):
 *   mvldm_dists_prep    in0, in1: fp32 NCHW [n_img][3][h][w] in [0, 1] (not clipped) -> dst NHWC [2 n_img][h][w][c_pad],
 *                       x' = (x - mean_c) / std_c with mean = (.485, .456, .406), std = (.229, .224, .225); c_pad = 4 (f32) / 8 (16 bit),
 *                       the pad channels zero.  Refused: h or w < 1, a null or unaligned pointer.
 *   mvldm_dists_stats   feat: the PRE-activation output [2 n_img][h][w][c] of a stage's last conv (feat_b null), ReLU applied on load; or,
 *                       with c = 3 and dtype MVLDM_F32, feat and feat_b the two RAW fp32 NCHW inputs [n_img][3][h][w] (tap 0: never a
 *                       rounded copy).  Per pair i and channel, with a = relu(feat[i]), b = relu(feat[n_img + i]): the five sums over the
 *                       pixels  sum a, sum b, sum a^2, sum b^2, sum a b,  accumulated in fp64 from the first product on.  Workgroup k
 *                       (k < mvldm_dists_stat_slots(h, w, c), a band of 512 pixels at c = 64, 256 above, 4096 at c = 3) writes its
 *                       partial of sum s, channel ch to workspace[i * doubles_per_pair + offset + (k * 5 + s) * c + ch]
 *                       (no atomics: the same bits on every run, for every n_img and position).  Refused: c not 3 or a multiple of 64
 *                       in 64 ... 512, [offset, offset + slots * 5 * c) outside doubles_per_pair, a workspace below
 *                       n_img * doubles_per_pair * 8 bytes, a null or unaligned pointer, h or w < 1.
 *   mvldm_dists_l2pool  feat as above (c a multiple of 64) -> out [2 n_img][ceil(h / 2)][ceil(w / 2)][c] =
 *                       sqrt(sum_{i,j < 3} g_ij relu(feat)[2y - 1 + i][2x - 1 + j]^2 + 1e-12), g = outer((1, 2, 1), (1, 2, 1)) / 16
 *                       (hanning(5)[1:-1], normalised), zeros outside the map; fp32 arithmetic, rounded once to `dtype` at the store.
 *   mvldm_dists_fold    out[i] (fp32) = sum_c (alpha_c (mx - my)^2 / (mx^2 + my^2 + c1) + beta_c (vx + vy - 2 cov) / (vx + vy + c2))
 *                       / (sum alpha + sum beta), which equals the score above and is exactly 0 for identical inputs; fp64, each
 *                       channel's partials summed in slot order, the channels in a fixed tree.  alpha, beta: fp32 [1475] in tap order.
 *                       The layout is the one mvldm_dists_workspace_bytes(n_img, h, w) describes: per pair, tap after tap, the
 *                       slots * 5 * c doubles of tap 0 (h x w, 3 channels), tap 1 (h x w, 64), tap 2 (ceil(h/2) x ceil(w/2), 128),
 *                       tap 3 (256), tap 4 (512), tap 5 (512), each map half the one before, rounded up.
 * mvldm_dists_workspace_bytes is 0 for a refused shape (n_img, h or w < 1, or too large), mvldm_dists_stat_slots for a refused map or c.
 * There is no minimum edge: a 1 x 1 image is valid (every variance is 0, every S2 is c2 / c2 = 1).
 * Parity with the DISTS_pytorch package and its published weights is unpinned: the arithmetic above is a restatement. */
size_t mvldm_dists_workspace_bytes(int n_img, int h, int w);
int mvldm_dists_stat_slots(int h, int w, int c);
int mvldm_dists_prep(const float* in0, const float* in1, void* dst, int n_img, int h, int w, int c_pad, int dtype, mvldm_stream_t stream);
int mvldm_dists_stats(const void* feat, const void* feat_b, int n_img, int h, int w, int c, int dtype, double* workspace,
                      size_t workspace_bytes, int offset, int doubles_per_pair, mvldm_stream_t stream);
int mvldm_dists_l2pool(const void* feat, void* out, int n_img, int h, int w, int c, int dtype, mvldm_stream_t stream);
int mvldm_dists_fold(const double* workspace, size_t workspace_bytes, int n_img, int h, int w, const float* alpha, const float* beta,
                     float* out, mvldm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * FID (feature = 64): the glue between the three 3x3 convolutions of the Inception-v3 stem (mvldm_igemm_fwd, BatchNorm folded into
 * weight and bias; the ReLU after the first two is mvldm_lpips_relu) and the Frechet distance of two sets of 64 features.
 *   replaces  torchmetrics' FrechetInceptionDistance(feature=64, normalize=True) as src/evaluation/metric_computer.py:22,65-68 uses it:
 *             update(imgs, real) -- (imgs * 255).byte(), torch-fidelity's TensorFlow-1 bilinear resize to 299 x 299, (x - 128) / 128,
 *             Conv2d_1a_3x3 / 2a / 2b with BatchNorm(eps 1e-3) and ReLU, MaxPool(3, 2), the mean over the map, .double(), sum f and
 *             sum f^T f per side -- and compute(): mu = sum / n, Sigma = (sum f^T f - n mu^T mu) / (n - 1),
 *             fid = |mu1 - mu2|^2 + tr Sigma1 + tr Sigma2 - 2 sum_i Re sqrt(eig_i(Sigma1 Sigma2)).
 * All four run eagerly on `stream`, never synchronise or allocate, use no atomics (the same bits on every run) and refuse on the host
 * before any launch:
 *   mvldm_fid_prep        src: NCHW [n_img][3][h][w], fp32 in [0, 1] (src_u8 = 0: quantised as trunc(min(max(x * 255, 0), 255)), the
 *                         product in fp32 -- the package's .byte() wraps outside [0, 1], this clamps) or uint8 (src_u8 = 1) -> dst NHWC
 *                         [n_img][oh][ow][c_pad] in `dtype`, c_pad = 4 (f32) / 8 (16 bit), the pad channels zero.  Output (oy, ox) reads
 *                         the source at y = float(oy) * (float(h) / float(oh)) (fp32, no half-pixel centres), y0 = trunc(y),
 *                         y1 = min(y0 + 1, h - 1), dy = y - y0, likewise x; v0 = a00 + (a01 - a00) dx, v1 = a10 + (a11 - a10) dx,
 *                         v = v0 + (v1 - v0) dy, all fp32, not contracted; stores (v - 128) / 128.  Refused: an edge below 1, a c_pad
 *                         the implicit GEMM would refuse, a null or unaligned pointer.
 *   mvldm_fid_pool        feat: the PRE-activation NHWC [n_img][h][w][c], c a multiple of 64 up to 512.  ReLU, max-pool 3x3 / stride 2 /
 *                         no padding / floor (oh = (h - 3) / 2 + 1), and the sum of the pooled map per channel, fp64 from the first
 *                         add; the pooled map is never written.  Workgroup k (k < mvldm_fid_pool_slots(h, w, c): a band of
 *                         ceil(512 / ow) output rows) writes its partial of channel ch to workspace[(i * slots + k) * c + ch].
 *                         Refused: h or w < 3, another c, a workspace below n_img * slots * c * 8 bytes, a null or unaligned pointer.
 *   mvldm_fid_accumulate  workspace: the partials above, followed by room for n_img * c doubles (mvldm_fid_workspace_bytes covers both).
 *                         f[i][ch] = (the partials of image i in band order) / (oh * ow), written behind the partials and, if
 *                         `features` is not null, to features[n_img][c]; then state[0] += n_img, state[1 + a] += sum_i f[i][a],
 *                         state[1 + c + a c + b] += sum_i f[i][a] f[i][b], each sum over the images in order and added to the state
 *                         once.  `state`: 1 + c + c c doubles on the device, zero before the first call; null: the features only.
 *   mvldm_fid_compute     c must be 64.  One workgroup; mu, Sigma and everything after in fp64, the matrices in LDS.  Sigma1 = V D V^T by
 *                         cyclic Jacobi (round-robin ordering: 32 disjoint rotations a round, 63 rounds a sweep; converged when
 *                         off(A) <= 1e-22 |A|_F, at most 30 sweeps), then the eigenvalues lambda of D^1/2 V^T Sigma2 V D^1/2 (the spectrum of
 *                         Sigma1^1/2 Sigma2 Sigma1^1/2, real and symmetric) the same way; score (fp32) = |mu1 - mu2|^2 + (tr Sigma1 +
 *                         tr Sigma2) - 2 sum_i sqrt(max(lambda_i, 0)).  info (8 doubles): sweeps and final off(A) / |A|_F of the first
 *                         solve, of the second, the number of solves that stopped at the sweep cap, the score in fp64, sum sqrt, and
 *                         the other three terms.  A solve that stops at the cap, or a state of fewer than 2 samples, stores NaN as
 *                         the score.  Identical states score about -1e-8 times the scale, not 0.
 * mvldm_fid_workspace_bytes and mvldm_fid_pool_slots are 0 for a refused shape.
 * Parity with torchmetrics / torch-fidelity and their published weights is unpinned: the arithmetic above is a restatement. */
size_t mvldm_fid_workspace_bytes(int n_img, int h, int w, int c);
int mvldm_fid_pool_slots(int h, int w, int c);
int mvldm_fid_prep(const void* src, int src_u8, void* dst, int n_img, int h, int w, int oh, int ow, int c_pad, int dtype,
                   mvldm_stream_t stream);
int mvldm_fid_pool(const void* feat, int n_img, int h, int w, int c, int dtype, double* workspace, size_t workspace_bytes,
                   mvldm_stream_t stream);
int mvldm_fid_accumulate(double* workspace, size_t workspace_bytes, int n_img, int h, int w, int c, double* features, double* state,
                         mvldm_stream_t stream);
int mvldm_fid_compute(const double* state1, const double* state2, int c, float* score, double* info, mvldm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Clean-FID: what `cleanfid.fid.compute_fid(dir, "gt_images")` (src/scripts/compute_fid.py:44-47; mode "clean", model inception_v3)
 * needs around the 94 convolutions of Inception-v3 (mvldm_igemm_fwd, BatchNorm folded into weight and bias), and the Frechet distance of
 * two sets of up to 2048 features.  Everything runs eagerly on `stream`, never synchronises or allocates, uses no atomics (the same bits
 * on every run) and refuses on the host before any launch: a null or unaligned pointer, an unknown dtype, channels that are no whole
 * 16-byte chunks, an operand past the 32-bit offset range of the convolutions, a workspace that is too small.
 *   mvldm_inception_prep      replaces cleanfid's resize_single_channel (compute_fid.py:46 -> cleanfid/resize.py, mode "clean"):
 *                             src NCHW [n_img][3][h][w], uint8 (src_u8 = 1) or fp32 in [0, 1] (src_u8 = 0: multiplied by 255 in fp32 and NOT
 *                             quantised) -> dst NHWC [n_img][oh][ow][c_pad] in `dtype`, c_pad = 4 (f32) / 8 (16 bit), pad channels zero.
 *                             PIL's Image.resize(BICUBIC) on a float32 plane: antialiased and separable, horizontally first, a pass whose
 *                             size stays is skipped.  Per axis scale = in / out, filterscale = max(scale, 1), support = 2 filterscale;
 *                             output i: center = (i + 0.5) scale, xmin = max(0, int(center - support + 0.5)), xmax = min(in,
 *                             int(center + support + 0.5)), k_j = cubic((j + xmin - center + 0.5) (1 / filterscale)) with a = -0.5,
 *                             divided by their sum; the sum over the taps in double, in tap order, rounded to float32 at the end of each
 *                             pass.  Then clip to [0, 255] and (v - 128) / 128 in fp32.  workspace: [n_img][3][h][ow] float32, the
 *                             horizontal pass's output (mvldm_inception_workspace_bytes(n_img, h, ow)).
 *   mvldm_inception_unfold    src NHWC [n_img][h][w][c] -> dst [n_img][h][w][kh kw c]: the kh x kw window around each pixel (stride 1,
 *                             padding kh / 2, kw / 2), tap-major then channel, zero outside the map.  The 1 x 7, 7 x 1, 1 x 3, 3 x 1 and
 *                             5 x 5 convolutions of torchvision's InceptionA / C / D / E blocks are then 1 x 1 convolutions whose weight is
 *                             permuted to [n_out][kh][kw][c_in].  kh, kw odd, up to 7.
 *   mvldm_inception_maxpool   F.max_pool2d(x, 3, stride, pad), stride 1 or 2, pad 0 or 1 (as -inf), the output size floored;
 *   mvldm_inception_avgpool   F.avg_pool2d(x, 3, 1, 1, count_include_pad=False): the sum of the taps inside the map in fp64, divided by their
 *                             number, rounded once;
 *   mvldm_inception_concat    dst = src (relu = 1: max(src, 0)), src a contiguous [rows][c].  All three write channels [dst_c_off,
 *                             dst_c_off + c) of rows of dst_ld channels: torch.cat(branches, 1) without a pass of its own.
 *   mvldm_inception_features  feat NHWC [n_img][h][w][c] (after its ReLU) -> features[n_img][c] fp64: adaptive_avg_pool2d(x, 1), the pixels
 *                             in order, fp64 from the first add.
 *   mvldm_frechet_accumulate  state[0] += n, state[1 + a] += sum_i f[i][a], state[1 + d + a d + b] += sum_i f[i][a] f[i][b], the rows in
 *                             order and added to the state once; d a multiple of 64 up to 2048 (np.mean / np.cov of cleanfid's
 *                             get_folder_features output, kept as sums).
 *   mvldm_frechet_compute     cleanfid.fid.frechet_distance: mu = sum / n, Sigma = (sum f^T f - n mu^T mu) / (n - 1); Sigma1 = V D V^T, then
 *                             the eigenvalues lambda of D^1/2 V^T Sigma2 V D^1/2 (the spectrum of Sigma1^1/2 Sigma2 Sigma1^1/2; the package
 *                             takes Re sqrtm(Sigma1 Sigma2)); score (fp32) = |mu1 - mu2|^2 + (tr Sigma1 + tr Sigma2) - 2 sum_i
 *                             sqrt(max(lambda_i, 0)), all in fp64 with the matrices in the workspace (mvldm_frechet_workspace_bytes(d):
 *                             16 + 4 d + 4 d d doubles).  Both eigen-solves are one-sided Jacobi (Hestenes) on the columns of G = A V:
 *                             round-robin ordering, d / 2 disjoint column pairs a round, one launch a round with one workgroup a pair;
 *                             the rotation of a pair comes from its three dot products and is applied when |g_p . g_q| >
 *                             tol |g_p| |g_q|, tol = sqrt(d) 2^-52 (and |g_p| |g_q| > tol^2 |A|_F^2: two columns of round-off
 *                             are left alone).  30 sweeps are enqueued; a sweep in which no pair passed tol sets a
 *                             flag in the workspace that makes the launches behind it return at once -- the host reads nothing.  The
 *                             first solve's eigenvalues are v_i . g_i, the second's |g_i|.  info (8 doubles): sweeps and the last
 *                             sweep's largest |g_p . g_q| / (|g_p| |g_q|) of the first solve, of the second, the solves that were still
 *                             rotating in sweep 30 (then the score is NaN, as for a state of fewer than 2 samples), the score in fp64,
 *                             sum sqrt, and the other three terms.
 * The two *_workspace_bytes are 0 for a refused shape.  Parity with clean-fid, PIL and the published weights: the resize is pinned against
 * PIL's own output (tests/golden/cleanfid_resize.npz), the rest is a restatement ("parity unpinned"). */
size_t mvldm_inception_workspace_bytes(int n_img, int h, int ow);
int mvldm_inception_prep(const void* src, int src_u8, void* dst, int n_img, int h, int w, int oh, int ow, int c_pad, int dtype,
                         void* workspace, size_t workspace_bytes, mvldm_stream_t stream);
int mvldm_inception_unfold(const void* src, void* dst, int n_img, int h, int w, int c, int kh, int kw, int pad_h, int pad_w, int dtype,
                           mvldm_stream_t stream);
int mvldm_inception_maxpool(const void* src, void* dst, int n_img, int h, int w, int c, int stride, int pad, int dst_ld, int dst_c_off,
                            int dtype, mvldm_stream_t stream);
int mvldm_inception_avgpool(const void* src, void* dst, int n_img, int h, int w, int c, int dst_ld, int dst_c_off, int dtype,
                            mvldm_stream_t stream);
int mvldm_inception_concat(const void* src, void* dst, size_t rows, int c, int dst_ld, int dst_c_off, int relu, int dtype,
                           mvldm_stream_t stream);
int mvldm_inception_features(const void* feat, int n_img, int h, int w, int c, int dtype, double* features, mvldm_stream_t stream);
int mvldm_frechet_accumulate(const double* features, int n, int d, double* state, mvldm_stream_t stream);
size_t mvldm_frechet_workspace_bytes(int d);
int mvldm_frechet_compute(const double* state1, const double* state2, int d, double* workspace, size_t workspace_bytes, float* score,
                          double* info, mvldm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Clean-KID: `cleanfid.fid.compute_kid(dir, "gt_images")` (src/scripts/compute_fid.py:44-47) behind the features, i.e. the package's
 * kernel_distance(feats1, feats2, num_subsets, max_subset_size) with the subsets as an explicit input:
 *   x_s = rows idx2[s][0 .. m) of f2 [n2][d], y_s = rows idx1[s][0 .. m) of f1 [n1][d]   (the package draws the x side first)
 *   A_s = sum_{i != j} (x_i . x_j / d + 1)^3 + sum_{i != j} (y_i . y_j / d + 1)^3,  B_s = sum_{i, j} (x_i . y_j / d + 1)^3
 *   per_subset[s] = A_s / (m - 1) - 2 B_s / m,  kid = sum_s per_subset[s] / num_subsets / m
 * all in fp64 (the package's features and products are float32).  No m x m matrix is ever stored: a workgroup owns one 64 x 64 tile of
 * one Gram of one subset, gathers the rows through LDS in 128-byte pieces, multiplies on v_mfma_f64_16x16x4_f64, cubes, masks (rows and
 * columns at or beyond m, the diagonal of the two symmetric Grams) and reduces the tile in a fixed tree to one double of the workspace;
 * the symmetric Grams run only the tile pairs a <= b and count a < b twice.  A second launch adds a subset's tiles in index order, a
 * third the subsets in order: no floating-point atomics, the same bits on every call; nothing allocates or synchronises.
 *   mvldm_kid_workspace_bytes  num_subsets (T (T + 1) + T T + 2) doubles, T = ceil(m / 64); 0 for m < 2 or num_subsets < 1.
 *   mvldm_kid_compute          score (fp32) = (float)info[0]; per_subset [num_subsets] may be NULL (the values then stay in the
 *                              workspace); info (4 doubles): kid in fp64, the mean over s of scale_s / m with scale_s = |A_s| / (m - 1) +
 *                              2 |B_s| / m (what an error of the sums is measured against), m, the number of subsets with an index
 *                              outside [0, n).  Such an index is clamped before it is used as an address -- no read leaves f1[0 .. n1 d)
 *                              or f2[0 .. n2 d) --, its subset's value is NaN and so is the score; the other subsets are unaffected.
 *                              MVLDM_ERR_ARG: m < 2, m > min(n1, n2), num_subsets < 1, a short workspace, a null or unaligned pointer
 *                              (f1, f2: 16 bytes).  MVLDM_ERR_UNSUPPORTED: d no multiple of 64 or above 2048 (the widths
 *                              mvldm_frechet_* takes).
 * Parity with the clean-fid package is unpinned (it is not installed): the arithmetic above is a restatement. */
size_t mvldm_kid_workspace_bytes(int m, int num_subsets);
int mvldm_kid_compute(const double* f1, int n1, const double* f2, int n2, int d, const int32_t* idx1, const int32_t* idx2, int num_subsets,
                      int m, double* workspace, size_t workspace_bytes, float* score, double* per_subset /* [num_subsets], may be NULL */,
                      double* info /* [4] */, mvldm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Crop shim: `rescale_and_crop(images, intrinsics, shape)` (src/dataset/shims/crop_shim.py:11-75) for the images -- what every dataset
 * reader of the reference applies before a batch leaves it.  Per image: quantise to bytes, Image.resize((w_s, h_s), Image.LANCZOS) on the
 * 8-bit RGB image, centre crop to h_out x w_out, / 255.
 *   geometry  scale = max(h_out / h, w_out / w) in double; h_s = round(h scale), w_s = round(w scale), half to even as Python's round;
 *             one of them must meet its target (else MVLDM_ERR_ARG, the reference's assert); row = (h_s - h_out) / 2,
 *             col = (w_s - w_out) / 2, floored.  scaled_hw (host int[2], may be NULL) receives h_s, w_s: the caller scales fx by
 *             w_s / w_out and fy by h_s / h_out.
 *   src       src_u8 = 1: uint8 [n_img][h][w][3], a decoded image as PIL hands it over; src_u8 = 0: fp32 [n_img][3][h][w] in [0, 1],
 *             quantised as the reference does -- x 255 in fp32, clamp to [0, 255], truncate (not round: 0.999999 is 254, there as
 *             here).
 *   resize    PIL's 8-bit resample, bit for bit: per axis scale = in / out, filterscale = max(scale, 1), support = 3 filterscale;
 *             output i: center = (i + 0.5) scale, xmin = max(0, int(center - support + 0.5)), xmax = min(in, int(center + support +
 *             0.5)), w_j = lanczos3((j + xmin - center + 0.5) / filterscale) divided by their sum in tap order, all in double on the
 *             host; k_j = int(w_j 2^22 +- 0.5), the sign of the 0.5 that of w_j; pixel = clip((2^21 + sum_j px_j k_j) >> 22, 0, 255)
 *             in int32 (arithmetic shift).  Horizontally first, with a uint8 image between the passes; a pass whose size stays is
 *             the identity.  Only the columns [col, col + w_out) and rows [row, row + h_out) are computed, and the horizontal pass
 *             only runs over the source rows their taps read.
 *   dst       fp32 [n_img][3][h_out][w_out] = byte / 255 (one correctly rounded fp32 divide).
 *   workspace the uint8 image between the passes, [n_img][3][rows read][roundup(w_out, 4)]: mvldm_crop_shim_workspace_bytes (0 for
 *             a refused shape); a smaller one is MVLDM_ERR_ARG.
 * The bounds and coefficients of an axis are kept on the device per (device, in, out, first output, outputs) for the life of the
 * process.  The FIRST call with a new geometry builds them on the host, allocates and uploads (hipMalloc + hipMemcpy: the one
 * exception to "never allocates"; inside a stream capture it is refused with MVLDM_ERR_UNSUPPORTED instead); every later call is two
 * launches, reads nothing back and may be captured.  Pointers: 4-byte aligned.  Sources up to 65536 x 16384 (h x w).
 * mvldm_crop_shim_axis writes the host-side tables of outputs [offset, offset + count) of an axis n_in -> n_out (bounds [count][2]:
 * first tap, taps; coefs [count][ksize], either may be NULL) and returns ksize, or a negative MVLDM_ERR_*: what the tests compare
 * with PIL's own tables without a device.
 * mvldm_crop_shim_flip is mvldm_crop_shim of images of which some are mirrored along w first -- `apply_augmentation_shim`
 * (src/dataset/shims/augmentation_shim.py:16-36), which flips the full-size image BEFORE rescale_and_crop.  flip: one byte per image on
 * the device (non-zero: mirrored), or NULL for none, which is mvldm_crop_shim.  The flip happens at the source read: a flagged image's
 * horizontal pass stages the window's source columns [x0, x1) in flipped coordinates, i.e. columns [w - x1, w - x0) reversed; tables,
 * workspace, the vertical pass and the launch count are the same, so one call serves a batch that mixes both.  Flipping the result
 * instead would not give the reference's bytes: PIL's tables are not mirror-symmetric (xmin = (int)(center - support + 0.5) truncates,
 * the centre crop floors an odd margin). */
size_t mvldm_crop_shim_workspace_bytes(int n_img, int h, int w, int h_out, int w_out);
int mvldm_crop_shim(const void* src, int src_u8, float* dst, int n_img, int h, int w, int h_out, int w_out, void* workspace,
                    size_t workspace_bytes, int* scaled_hw /* host [2], may be NULL */, mvldm_stream_t stream);
int mvldm_crop_shim_flip(const void* src, int src_u8, float* dst, int n_img, int h, int w, int h_out, int w_out,
                         const uint8_t* flip /* device, n_img bytes; NULL: none */, void* workspace, size_t workspace_bytes,
                         int* scaled_hw /* host [2], may be NULL */, mvldm_stream_t stream);
int mvldm_crop_shim_axis(int n_in, int n_out, int offset, int count, int32_t* bounds /* host */, int32_t* coefs /* host */, int coefs_len);

/* ------------------------------------------------------------------------------------------------
 * JPEG frames: what `Image.open(BytesIO(frame)).convert("RGB")` gives for the dataset's frames (src/dataset/dataset_re10k.py:157-169,
 * `convert_images`), bit for bit with Pillow on libjpeg / libjpeg-turbo (ISLOW inverse DCT, fancy upsampling: the library's defaults).
 * The serial half -- markers and the Huffman-coded scan -- runs on the host, without Pillow, into a buffer the caller owns; the
 * parallel half -- dequantise, inverse DCT, chroma upsampling, colour conversion: integer and exactly specified -- runs on the device.
 *   streams   baseline sequential (SOF0), Huffman coded, 8-bit samples, 8-bit quantisation tables, ONE scan that interleaves every
 *             component, restart intervals (DRI / RSTn) included; 1 component (sampling 1 x 1), or 3 components that libjpeg reads
 *             as YCbCr (a JFIF APP0, or ids 1, 2, 3 and no Adobe APP14) with luma sampling 1 x 1, 2 x 1 or 2 x 2 and 1 x 1 chroma:
 *             MVLDM_JPEG_GRAY / _444 / _422 / _420.  Anything else is refused with a MVLDM_JPEG_* reason (> 0): the caller decodes that
 *             frame some other way (mv_ldm_amd: through Pillow).  No read leaves data[0 .. len); every loop over the stream is
 *             bounded by len.
 *   layout    mcux = ceil(w / (8 hmax)), mcuy = ceil(h / (8 vmax)); component c has a grid of bh_c x bw_c = (mcuy v_c) x (mcux h_c)
 *             blocks (MCU-padded) and cw_c x ch_c = ceil(w h_c / hmax) x ceil(h v_c / vmax) real samples.  coef: int16, per frame the
 *             components one after another, per component the blocks row-major over its grid, per block the 64 QUANTISED
 *             coefficients in natural (row-major, de-zigzagged) order: mvldm_jpeg_coef_count values (0 for a refused shape).
 *             qt: uint16 [3][64] per frame, the table of component c in natural order (unused ones zero).
 *   guard     S = sum_k |coef_k qt_k| of a block.  A frame with a block above B = 5905 is refused (MVLDM_JPEG_RANGE): only below it do
 *             libjpeg's 64-bit C code, libjpeg-turbo's 16-bit SIMD code and an int32 kernel agree.  Derivation: csrc/jpeg_common.h.
 *   idct      value = coef qt in int32; jidctint.c: CONST_BITS 13, PASS1_BITS 2, columns first with DESCALE(., 11), then rows with
 *             DESCALE(., 18), DESCALE(x, n) = (x + (1 << (n - 1))) >> n (arithmetic); even part z1 = (in2 + in6) 4433, tmp2 = z1 - in6
 *             15137, tmp3 = z1 + in2 6270, tmp0 / tmp1 = (in0 +- in4) << 13; odd part on in7, in5, in3, in1 with z5 = (z3 + z4) 9633 and
 *             the constants 2446, 16819, 25172, 12299, -7373, -20995, -16069, -3196; sample = clip(x + 128, 0, 255).
 *   upsample  jdsample.c's fancy upsampling on the component's REAL size (the row above the first is the first, the row below the last
 *             real row is the last real row).  h2v1: out[2i] = (3 in[i] + in[i-1] + 1) >> 2, out[2i+1] = (3 in[i] + in[i+1] + 2) >> 2,
 *             out[0] = in[0], the last odd output is in[last].  h2v2: s[i] = 3 near[i] + far[i] (far: the row above for an even
 *             output row, below for an odd one); out[2i] = (3 s[i] + s[i-1] + 8) >> 4, out[2i+1] = (3 s[i] + s[i+1] + 7) >> 4, the
 *             first (4 s[0] + 8) >> 4, the last (4 s[last] + 7) >> 4.  A component of one or two samples per row is replicated
 *             instead, as libjpeg does (jinit_upsampler: the filters need downsampled_width > 2).
 *   colour    cb, cr centred by -128: R = y + ((91881 cr + 32768) >> 16), G = y + ((-22554 cb - 46802 cr + 32768) >> 16),
 *             B = y + ((116130 cb + 32768) >> 16), each clipped to [0, 255]; grayscale writes y three times.
 *   dst       uint8 [n_img][h][w][3]: what mvldm_crop_shim takes with src_u8 = 1.
 * mvldm_jpeg_probe (host) reads the markers up to the scan: info[0..7] = h, w, sampling (MVLDM_JPEG_GRAY ...), reason, blocks of
 * component 0, blocks of each chroma component, mcux, mcuy.  h and w are set as soon as a frame header was read (0 otherwise), the
 * rest only for a supported stream.  Returns the reason: 0 supported, > 0 a MVLDM_JPEG_* reason, MVLDM_ERR_ARG for a null pointer.
 * mvldm_jpeg_entropy (host) decodes the scan into coef (room for coef_len values; a supported frame that needs more is MVLDM_ERR_ARG and
 * nothing is written) and qt; max_s (may be NULL) receives the largest S of the blocks decoded.  Returns like the probe, with
 * MVLDM_JPEG_RANGE for a frame outside the guard.  After a refusal the contents of coef and qt are unspecified, but nothing outside
 * coef[0 .. coef_len) and qt[0 .. 192) is ever written.  Both keep no state and may run on many threads at once.
 * mvldm_jpeg_decode (device) turns n_img frames of ONE (h, w, sampling) into pixels: jpeg_idct_kernel (every block of every component
 * of every frame -> uint8 planes in the workspace, 64 bytes per block: mvldm_jpeg_workspace_bytes), then jpeg_color_kernel.  Two
 * launches, no allocation, nothing read back; may be captured.  coef [n_img][coef_count], qt [n_img][3][64], dst, workspace: device
 * pointers, 4-byte aligned; a null or misaligned pointer, a short workspace or a refused shape is MVLDM_ERR_ARG.  It trusts the
 * coefficients: values outside the guard give wrapped int32 arithmetic, never an access outside the buffers.
 * mvldm_jpeg_idct_host (host) is the same arithmetic (the same inline functions) for one frame in plain C++: what the CPU tests pin to
 * Pillow and a sanitizer build exercises.  Edges up to 16384. */
enum { MVLDM_JPEG_GRAY = 0, MVLDM_JPEG_444 = 1, MVLDM_JPEG_422 = 2, MVLDM_JPEG_420 = 3 };
enum {
    MVLDM_JPEG_OK = 0,
    MVLDM_JPEG_NOT_JPEG = 1,    /* no SOI at the start */
    MVLDM_JPEG_TRUNCATED = 2,   /* the stream ends inside a marker segment or inside the scan */
    MVLDM_JPEG_CORRUPT = 3,     /* a segment, a Huffman table, a code, a coefficient index or a restart marker that cannot be */
    MVLDM_JPEG_PROGRESSIVE = 4, /* SOF2 */
    MVLDM_JPEG_CODING = 5,      /* any other frame type: extended, lossless, hierarchical, arithmetic coding */
    MVLDM_JPEG_PRECISION = 6,   /* samples or quantisation tables that are not 8-bit */
    MVLDM_JPEG_COMPONENTS = 7,  /* neither 1 nor 3 components */
    MVLDM_JPEG_SAMPLING = 8,    /* sampling factors outside the four layouts */
    MVLDM_JPEG_COLORSPACE = 9,  /* 3 components libjpeg would not read as YCbCr */
    MVLDM_JPEG_SCANS = 10,      /* a scan that does not hold every component */
    MVLDM_JPEG_SIZE = 11,       /* an edge of 0 or above 16384 */
    MVLDM_JPEG_RANGE = 12       /* a block outside the range guard */
};
int mvldm_jpeg_probe(const uint8_t* data /* host */, size_t len, int32_t* info /* host [8] */);
size_t mvldm_jpeg_coef_count(int h, int w, int sampling);
int mvldm_jpeg_entropy(const uint8_t* data /* host */, size_t len, int16_t* coef /* host */, size_t coef_len, uint16_t* qt /* host [192] */,
                       int32_t* max_s /* host, may be NULL */);
size_t mvldm_jpeg_workspace_bytes(int n_img, int h, int w, int sampling);
int mvldm_jpeg_decode(const int16_t* coef, const uint16_t* qt, uint8_t* dst, int n_img, int h, int w, int sampling, void* workspace,
                      size_t workspace_bytes, mvldm_stream_t stream);
int mvldm_jpeg_idct_host(const int16_t* coef /* host */, const uint16_t* qt /* host [192] */, uint8_t* dst /* host [h][w][3] */, int h, int w,
                         int sampling);

/* ------------------------------------------------------------------------------------------------
 * JPEG frames: the scan on the device.  An opt-in second way to the coefficients mvldm_jpeg_decode takes: the host only removes the byte
 * stuffing and builds the tables (mvldm_jpeg_scan_prepare); the Huffman-coded scan is decoded by a self-synchronising decoder (Klein and
 * Wiseman; Weissenberger and Schmidt) in mvldm_jpeg_entropy_device.  The result is mvldm_jpeg_entropy's, value for value.
 *   streams   those of mvldm_jpeg_entropy WITHOUT restart intervals: a frame with DRI != 0 is MVLDM_JPEG_RESTART, and the caller decodes
 *             its scan with mvldm_jpeg_entropy.  The scan ends at the first 0xFF followed by a non-zero byte; after optional 0xFF fill
 *             bytes that marker must be EOI (else MVLDM_JPEG_CORRUPT; no marker before len: MVLDM_JPEG_TRUNCATED).
 *   scan      the entropy-coded bytes with every FF 00 reduced to FF, in stream order, at a 16-byte aligned offset of a packed buffer the
 *             caller owns, followed by zeros up to mvldm_jpeg_scan_room(bytes) = round_up(bytes, 16) + 16.  The device reads aligned
 *             dwords and swaps their bytes; the widest read for a symbol that starts at the last bit ends 12 bytes past the scan.
 *             mvldm_jpeg_scan_room(len) is also the room a frame of len encoded bytes can need: destuffing only shrinks.
 *   desc      int32 [4] per frame: byte offset of the scan in the packed buffer (a multiple of 16), bit_len (8 x destuffed bytes), bytes
 *             occupied with the padding, 0.  The device checks a descriptor against scan_bytes before it reads the scan.
 *   tables    MVLDM_JPEG_TABLE_BYTES per frame: six Huffman tables of MVLDM_JPEG_HUFF_TABLE_BYTES -- component 0's DC, its AC, component
 *             1's DC, ... as the scan header's td / ta select them (a shared table is stored twice; grayscale leaves four zero) -- then
 *             qt uint16 [3][64] as above.  A table: uint16 look[512] ((length << 8) | symbol of every code of up to 9 bits by its
 *             first 9 bits, 0 for a longer one), int32 maxcode[18] (largest code of length l, -1 if none; [17] above every code), int32
 *             valoff[18] (index of the first symbol of length l minus its code), uint8 vals[256].
 *   state     (p, b, k): bit position, block within the MCU (0 .. hmax vmax + 1; selects the component and so the tables), zigzag
 *             position (0: the next symbol is a DC category).  One step decodes one symbol and its magnitude bits, and it is a total
 *             function of the state and the bits: what mvldm_jpeg_entropy refuses is a FAULT, after which the decode goes on by a
 *             fixed rule -- a code that does not exist skips one bit, a DC category above 15 counts as 0, a coefficient index above
 *             63 consumes its bits and ends the block -- and a symbol whose bits run past bit_len gives DEAD (p = bit_len and a
 *             flag), which passes through everything after it.  No read leaves the padded scan, whatever the bits are.  Faults are
 *             not absorbing because a decoder started at a wrong bit faults constantly and would then never meet the true sequence
 *             of states; they count only where the entry state is known to be true (the write pass, below).
 *   decoder   one workgroup per frame.  The scan is cut into subsequences of subseq_bits (0: the default, 512; else a multiple of 32 in
 *             32 .. 65536), one per thread; a chunk is mvldm_jpeg_entropy_chunk_subseqs() = 1024 of them, and the workgroup walks the
 *             chunks in order.  Cold pass: every thread decodes its subsequence from (its first bit, 0, 0) -- thread 0 from the true
 *             state -- and leaves its exit state.  Rounds: thread i takes thread i - 1's exit as its entry and decodes again if that
 *             changed, until no entry changed or as many rounds ran as the chunk has subsequences: after r rounds the first r + 1
 *             subsequences are right whatever the stream is, so the bound is also the proof.  Write pass: a scan of the blocks each
 *             thread completed gives its first block; it decodes once more and stores every coefficient at mvldm_jpeg_entropy's
 *             address (the DC DIFFERENCE in [0]), each store guarded by block < blocks of the frame.  The slots are zeroed by a memset
 *             in front of the kernel on the same stream.  A second kernel sums the DC differences per component in scan order (64-bit),
 *             and computes the guard's S of every block.
 *   accepted  when the write pass meets no fault in front of the frame's last block, that block completes with fewer than 8 bits left
 *             (where mvldm_jpeg_entropy stops reading; what the remaining bits would decode to is not looked at), and every DC prefix
 *             fits int16 -- else MVLDM_JPEG_CORRUPT -- and no S exceeds the guard, else MVLDM_JPEG_RANGE.
 *   status    int32 [4] per frame: reason, largest S (0 unless the reason is OK or RANGE: mvldm_jpeg_entropy's max_s), the largest number
 *             of rounds a chunk took, 0.
 * mvldm_jpeg_scan_prepare (host; no state, any number of threads) reads data[0 .. len) and writes scan[scan_off .. scan_off + desc[2]),
 * desc and tables; info (may be NULL) is mvldm_jpeg_probe's.  Returns the reason: what mvldm_jpeg_probe returns, MVLDM_JPEG_RESTART,
 * CORRUPT / TRUNCATED for the scan's end; MVLDM_ERR_ARG for a null pointer, an offset that is no multiple of 16, a scan_room below
 * scan_off + mvldm_jpeg_scan_room(len) or above 2^31 - 1.  After a refusal nothing outside those ranges was written.
 * mvldm_jpeg_entropy_device (device) decodes n_img prepared frames of ONE (h, w, sampling): a memset and two launches, no allocation,
 * nothing read back; may be captured.  scan, desc, tables, coef [n_img][coef_count], qt [n_img][3][64], status: device pointers, 16-byte
 * aligned (status, desc: 4); a null or misaligned pointer, a refused shape or subseq_bits is MVLDM_ERR_ARG.  After a refusal a frame's
 * coef slot is unspecified; nothing outside coef, qt and status is written.
 * mvldm_jpeg_entropy_emul_host (host) is the same algorithm with loops for threads and the same step function (csrc/jpeg_huff_common.h),
 * chunk_subseqs subsequences to a chunk (0: the device's): the same coef, qt and status, rounds included when the chunk sizes agree. */
#define MVLDM_JPEG_HUFF_TABLE_BYTES 1424
#define MVLDM_JPEG_TABLE_BYTES 8928
enum { MVLDM_JPEG_RESTART = 13 }; /* restart intervals: not on the device entropy path */
size_t mvldm_jpeg_scan_room(size_t len);
int mvldm_jpeg_scan_prepare(const uint8_t* data /* host */, size_t len, uint8_t* scan /* host */, size_t scan_off, size_t scan_room,
                            int32_t* desc /* host [4] */, uint8_t* tables /* host [MVLDM_JPEG_TABLE_BYTES] */, int32_t* info /* host [8], may be NULL */);
int mvldm_jpeg_entropy_chunk_subseqs(void);
int mvldm_jpeg_entropy_device(const uint8_t* scan, size_t scan_bytes, const int32_t* desc, const uint8_t* tables, int n_img, int h, int w,
                              int sampling, int16_t* coef, uint16_t* qt, int32_t* status, int subseq_bits, mvldm_stream_t stream);
int mvldm_jpeg_entropy_emul_host(const uint8_t* scan /* host */, size_t scan_bytes, const int32_t* desc /* host */, const uint8_t* tables /* host */,
                                 int n_img, int h, int w, int sampling, int16_t* coef /* host */, uint16_t* qt /* host */, int32_t* status /* host */,
                                 int subseq_bits, int chunk_subseqs);

/* ------------------------------------------------------------------------------------------------
 * JPEG frames: restart intervals on the device.  An opt-in THIRD way to the coefficients: the device entropy decoder above for frames
 * with and without restart intervals (DRI / RSTn).  mvldm_jpeg_scan_prepare and mvldm_jpeg_entropy_device keep their behaviour (a frame
 * with DRI is still MVLDM_JPEG_RESTART there).  The result is mvldm_jpeg_entropy's, value for value: coefficients, tables, reason, S.
 *   streams   those of mvldm_jpeg_entropy.  A frame with DRI = Ri has ceil(MCUs / Ri) intervals; one without DRI, or with Ri at or above
 *             its MCUs, is ONE interval of all its MCUs.  Between two intervals stands RSTn (after optional 0xFF fill bytes), n counting
 *             0 .. 7 in order; behind the last, EOI as above.  A stream whose markers are not exactly these -- one missing, one too
 *             many, one out of order, the data ending first -- is refused by prepare with the reason mvldm_jpeg_entropy gives it.
 *   region    a frame's part of the packed buffer, at a 16-byte aligned offset: the interval table -- int32 pairs (byte offset of the
 *             interval inside the region, its exact bit length), rounded up to 16 bytes -- then every interval destuffed (FF 00 -> FF;
 *             fill bytes and markers dropped) at a 4-byte aligned offset, then zeros up to round_up(bytes behind the table, 16) + 16.
 *             The device reads aligned dwords relative to an interval's first byte; a bit position is relative to its interval.
 *   desc      int32 [4] per frame: byte offset of the region (a multiple of 16), intervals, bytes occupied, Ri (MCUs of the frame when
 *             it is one interval).  The device refuses (MVLDM_JPEG_CORRUPT) a descriptor that does not fit scan_bytes or whose interval
 *             count is not ceil(MCUs / Ri), and a table with any pair that is misaligned, empty, inside the table or whose widest read
 *             (12 bytes past its last) leaves the bytes occupied -- before it reads a bit of the frame's scan.
 *   room      mvldm_jpeg_rst_need(data, len): what this frame can occupy (from its header: table of its intervals, scan bytes, one byte
 *             of alignment per interval, padding; 0 for a frame the parser refuses).  mvldm_jpeg_rst_room(len) bounds it for any frame of
 *             len encoded bytes (an interval every two bytes): a multiple of 16, about 5.5 len.
 *   decoder   one workgroup per frame.  Subsequences of subseq_bits never cross an interval: interval g has ceil(bits_g / subseq_bits),
 *             each decoded against the interval's end, so DEAD stays inside it.  The first subsequence of an interval has the true
 *             entry (its first bit, 0, 0) and never takes a predecessor's exit; every other one takes the exit of the one before it,
 *             so the induction above holds per interval and a chunk needs at most as many rounds as it has subsequences.  The
 *             workgroup walks the intervals in batches: the longest run of whole intervals whose subsequence counts sum to at most
 *             1024 is one chunk; an interval of more than 1024 is walked alone in chunks of 1024 with the carry.  Write pass: a thread's
 *             first block is g Ri (blocks of an MCU) plus the blocks completed by earlier subsequences of the same interval; every store
 *             is guarded by block < min(end of interval g, blocks of the frame).  The second kernel's DC sums restart at every
 *             interval (a segmented 64-bit scan); the int16 test applies to every prefix.
 *   accepted  when no fault stands in front of any interval's last block, every interval's last block completes with fewer than 8 bits
 *             of that interval left, every DC prefix fits int16 -- else MVLDM_JPEG_CORRUPT -- and no S exceeds the guard (_RANGE).
 *   status    int32 [4] per frame: reason, largest S, the largest number of rounds a chunk took, intervals (0: descriptor refused).
 * mvldm_jpeg_rst_prepare (host; no state, any number of threads) reads data[0 .. len) and writes scan[scan_off .. scan_off + desc[2]),
 * desc and tables (the blob above); info (may be NULL) is mvldm_jpeg_probe's.  Returns the reason: what mvldm_jpeg_probe returns, or
 * mvldm_jpeg_entropy's for a broken marker structure; MVLDM_ERR_ARG for a null pointer, an offset that is no multiple of 16 or beyond
 * scan_room, a scan_room above 2^31 - 1, or fewer than mvldm_jpeg_rst_need bytes behind the offset.  After a refusal nothing outside
 * scan[scan_off .. scan_off + mvldm_jpeg_rst_need), desc and tables was written.
 * mvldm_jpeg_rst_entropy_device (device): mvldm_jpeg_entropy_device's arguments and rules; a memset and two launches
 * (jpeg_rst_scan_kernel, jpeg_rst_dc_kernel), no allocation, nothing read back; may be captured.
 * mvldm_jpeg_rst_entropy_emul_host (host): the same algorithm with loops for threads and the same inline functions
 * (csrc/jpeg_huff_common.h); the same coef, qt and status, rounds included when the chunk sizes agree. */
size_t mvldm_jpeg_rst_room(size_t len);
size_t mvldm_jpeg_rst_need(const uint8_t* data /* host */, size_t len);
int mvldm_jpeg_rst_prepare(const uint8_t* data /* host */, size_t len, uint8_t* scan /* host */, size_t scan_off, size_t scan_room,
                           int32_t* desc /* host [4] */, uint8_t* tables /* host [MVLDM_JPEG_TABLE_BYTES] */, int32_t* info /* host [8], may be NULL */);
int mvldm_jpeg_rst_entropy_device(const uint8_t* scan, size_t scan_bytes, const int32_t* desc, const uint8_t* tables, int n_img, int h, int w,
                                  int sampling, int16_t* coef, uint16_t* qt, int32_t* status, int subseq_bits, mvldm_stream_t stream);
int mvldm_jpeg_rst_entropy_emul_host(const uint8_t* scan /* host */, size_t scan_bytes, const int32_t* desc /* host */, const uint8_t* tables /* host */,
                                     int n_img, int h, int w, int sampling, int16_t* coef /* host */, uint16_t* qt /* host */, int32_t* status /* host */,
                                     int subseq_bits, int chunk_subseqs);

/* ------------------------------------------------------------------------------------------------
 * PNG frames: row unfiltering and colour expansion on the device.  What `Image.open(BytesIO(frame)).convert("RGB")` gives for a PNG
 * (the reference writes its frames and ground-truth trees through Pillow, which picks a filter per row), bit for bit: alpha dropped,
 * grey replicated, palette entries looked up; tRNS, gAMA and iCCP play no part.  The caller (mv_ldm_amd/ops.py png_decode) parses the
 * chunks, checks their CRCs and inflates IDAT on the host; the device does the rest.
 *   streams   one buffer of inflated streams.  Frame i is h rows of 1 + stride bytes (filter byte, then the filtered row), stride =
 *             ceil(w * channels * depth / 8), at byte desc[i][0]: no row is aligned, none is assumed to be.  h, w: 1 .. 16384, common to
 *             the call.  Non-interlaced only.
 *   desc      int32 [MVLDM_PNG_DESC_INTS] per frame: stream offset, colour type, bit depth, offset of the frame's palette in `palettes`
 *             (bytes), palette entries (1 .. 256), 0, 0, 0.  Colour type 2, 6, 0 or 4 at depth 8; colour type 3 at depth 1, 2, 4 or 8.
 *             A descriptor of another format, or one whose stream (h * (1 + stride) bytes) or palette (3 bytes per entry) does not fit
 *             its buffer, is refused: status MVLDM_PNG_DESC, nothing of the frame is read and nothing is written for it.
 *   filters   None / Sub / Up / Average / Paeth per row, modulo 256; bytes left of the first pixel and the row above the first are 0;
 *             Average floors the 9-bit sum; Paeth is p = a + b - c in integers, ties in the order a, b, c.  A filter byte above 4 is
 *             treated as None (the caller refuses such a frame before any launch).
 *   dst       MVLDM_PNG_DST_U8: uint8 [n_img][h][w][3] (what mvldm_jpeg_decode writes and mvldm_crop_shim takes); MVLDM_PNG_DST_F32:
 *             fp32 [n_img][3][h][w] holding k / 255 correctly rounded (the bits of torch's `k.float() / 255`).
 *   status    int32 per frame: MVLDM_PNG_OK, MVLDM_PNG_DESC, or MVLDM_PNG_PALETTE_INDEX -- a pixel's palette index lies beyond the PLTE
 *             entries: it is written as black and the caller decodes that frame elsewhere.
 * mvldm_png_unfilter (device): one launch, one wave per frame.  Average and Paeth are serial along a row and need the row above, so the
 * wave walks bands of 64 rows as a skewed wavefront: lane r reconstructs unit t - r (a pixel, or a byte of pixels below 8 bits) at step
 * t and takes the two units it needs from the row above out of lane r - 1's registers; a band's last row waits in LDS for lane 0 of the
 * next band.  Nothing is allocated and nothing is read back, so the call can be captured.
 * mvldm_png_unfilter_host (host; no state, any number of threads) is the same arithmetic (csrc/png_common.h) row by row in plain C++ on
 * host pointers: what the CPU tests pin to Pillow.  It takes sizes from untrusted files and applies the same descriptor check. */
enum { MVLDM_PNG_DST_U8 = 0, MVLDM_PNG_DST_F32 = 1 };
#define MVLDM_PNG_DESC_INTS 8
enum {
    MVLDM_PNG_OK = 0,
    MVLDM_PNG_NOT_PNG = 1,       /* no PNG signature, or no IHDR first */
    MVLDM_PNG_TRUNCATED = 2,     /* the file ends inside a chunk, or has no IDAT / IEND */
    MVLDM_PNG_CRC = 3,           /* a chunk whose CRC does not match (critical or not: Pillow raises on either) */
    MVLDM_PNG_INTERLACE = 4,     /* Adam7 */
    MVLDM_PNG_DEPTH16 = 5,       /* 16-bit samples */
    MVLDM_PNG_GREY_BITS = 6,     /* grey below 8 bits */
    MVLDM_PNG_FORMAT = 7,        /* a colour type / bit depth / compression / filter method outside the PNG specification */
    MVLDM_PNG_SIZE = 8,          /* an edge of 0 or above 16384 */
    MVLDM_PNG_NO_PLTE = 9,       /* colour type 3 without a palette (or one of no entries, more than 256, or a length no multiple of 3) */
    MVLDM_PNG_FILTER = 10,       /* a filter byte above 4 */
    MVLDM_PNG_LENGTH = 11,       /* an inflated length other than h * (1 + stride) */
    MVLDM_PNG_INFLATE = 12,      /* zlib refuses the IDAT stream */
    MVLDM_PNG_PALETTE_INDEX = 13,/* status only: a palette index beyond the PLTE entries */
    MVLDM_PNG_DESC = 14          /* status only: a descriptor that does not fit its buffers */
};
int mvldm_png_unfilter(const uint8_t* streams, size_t stream_bytes, const int32_t* desc, const uint8_t* palettes, size_t palette_bytes, void* dst,
                       int dst_kind, int n_img, int h, int w, int32_t* status, mvldm_stream_t stream);
int mvldm_png_unfilter_host(const uint8_t* streams /* host */, size_t stream_bytes, const int32_t* desc /* host */, const uint8_t* palettes /* host */,
                            size_t palette_bytes, void* dst /* host */, int dst_kind, int n_img, int h, int w, int32_t* status /* host */);

/* ------------------------------------------------------------------------------------------------
 * PNG frames: IDAT inflated on the device (opt-in: mv_ldm_amd/ops.py png_decode(inflate="device")).  n zlib streams (RFC 1950 around
 * RFC 1951), one per frame, are inflated into the slots mvldm_png_unfilter reads, so that the upload is the file's IDAT bytes and not the
 * inflated stream.  The caller still walks the chunks and checks their CRCs, and copies a frame's IDAT bodies back to back.
 *   z         one buffer of zlib streams, 16-byte aligned.  Frame i's stream is zdesc[i][1] bytes at byte zdesc[i][0] (a multiple of 16)
 *             followed by zeros up to mvldm_png_inflate_room(bytes) = round_up(bytes, 16) + 16: the decoder reads aligned dwords.
 *   zdesc     int32 [MVLDM_PNG_ZDESC_INTS] per frame: offset, bytes, 0, 0.
 *   streams, desc   the output buffer and mvldm_png_unfilter's descriptors: frame i is written at byte desc[i][0] and has to be exactly
 *             need = h * (1 + stride) bytes.  A descriptor png_unfilter would refuse (the no-frame descriptor of a frame the host
 *             refused among them), or a zdesc that does not fit `z`, gives MVLDM_PNG_DESC: nothing of the frame is read or written.
 *   zstatus   int32 per frame, apart from mvldm_png_unfilter's status.  MVLDM_PNG_OK: the slot holds the inflated stream.
 *             MVLDM_PNG_LENGTH: the stream inflates to more or fewer than `need` bytes.  MVLDM_PNG_FILTER: a row's filter byte is
 *             above 4.  MVLDM_PNG_INFLATE: anything else -- a header other than CM = 8, CINFO <= 7, a multiple of 31, FDICT = 0; a
 *             reserved block type; a stored block whose length and complement disagree; a code set zlib refuses (over-subscribed, or
 *             incomplete other than a single one-bit code or a distance code of no codes; no end-of-block code; more than 286 / 30
 *             codes; a repeat with nothing before it or past the end); bits that match no code; length codes 286 / 287, distance
 *             codes 30 / 31; a distance beyond the bytes written so far; a stream that ends before its final block or its trailer
 *             does; an Adler-32 (computed on the device) other than the trailer's; a byte behind the trailer.
 *             After a refusal the slot's contents are unspecified; nothing outside the slot and the status word is written.
 * Stored, fixed and dynamic blocks in any sequence, empty stored blocks (Z_SYNC_FLUSH, Z_FULL_FLUSH), matches of 3 .. 258 bytes at
 * distances 1 .. 32768, overlapping ones included.
 * mvldm_png_inflate (device): one launch, one wave per frame, 37 KiB of LDS (a 32 KiB sliding window, two decode tables, a queue of 64
 * symbols).  One lane decodes symbols; the wave builds a dynamic block's tables, copies stored blocks and matches, writes runs of
 * literals, and sums the Adler-32.  Every loop is bounded by 8 * bytes + 16 steps, every read stays inside the padded stream, every
 * write is guarded by its position in the slot.  Nothing is allocated and nothing is read back, so the call can be captured.
 * mvldm_png_inflate_host (host; no state, any number of threads) runs the same step functions (csrc/inflate_common.h) with loops in
 * place of lanes: the same bytes and the same status. */
#define MVLDM_PNG_ZDESC_INTS 4
size_t mvldm_png_inflate_room(size_t bytes);
int mvldm_png_inflate(const uint8_t* z, size_t z_bytes, const int32_t* zdesc, uint8_t* streams, size_t stream_bytes, const int32_t* desc, int n_img, int h,
                      int w, int32_t* zstatus, mvldm_stream_t stream);
int mvldm_png_inflate_host(const uint8_t* z /* host */, size_t z_bytes, const int32_t* zdesc /* host */, uint8_t* streams /* host */, size_t stream_bytes,
                           const int32_t* desc /* host */, int n_img, int h, int w, int32_t* zstatus /* host */);

/* ------------------------------------------------------------------------------------------------
 * Plans: a whole forward (UNet walk, VAE decoder, DDIM step) as a flat list of the ops above with
 * all pointers resolved -- built once by the host (mv_ldm_amd/plan.py), executed here without
 * touching Python, optionally captured into a hipGraph.   replaces MultiViewUNet.forward's module
 * walk (mvunet.py:90-208) and the per-step Python of DiffusionWrapper.step/sample.
 */
enum {
    MVLDM_OP_IGEMM = 1, MVLDM_OP_GROUPNORM, MVLDM_OP_LAYERNORM, MVLDM_OP_ATTENTION, MVLDM_OP_TIMESTEP_EMBED,
    MVLDM_OP_ELTWISE, MVLDM_OP_DDIM_STEP, MVLDM_OP_DDIM_ADVANCE, MVLDM_OP_NCHW_TO_NHWC, MVLDM_OP_NHWC_TO_NCHW,
    MVLDM_OP_MEMCPY, MVLDM_OP_RAY_ENCODE, MVLDM_OP_POSTERIOR_SAMPLE,
    MVLDM_OP_WGRAD, MVLDM_OP_ATTENTION_BWD, MVLDM_OP_GROUPNORM_BWD, MVLDM_OP_LAYERNORM_BWD, MVLDM_OP_COLSUM,
    MVLDM_OP_TRAIN_ELTWISE, MVLDM_OP_POOL2X2, MVLDM_OP_ZERO_INSERT, MVLDM_OP_ADD_NOISE, MVLDM_OP_MSE_LOSS, MVLDM_OP_FILL_ZERO,
    /* markers (no payload): the ops between PAR_BEGIN and PAR_END form lanes separated by PAR_NEXT; the caller declares the lanes
     * mutually independent (disjoint outputs and workspaces).  mvldm_plan_run / _capture put lane 0 on the caller's stream and the
     * others on the plan's own side streams, forked and joined with events -- under capture these become parallel branches of the
     * hipGraph (the four sub-pixel phase convs of an upsampler, a resnet's 1x1 shortcut beside its main chain: what fills the chip at
     * one or two scenes).  mvldm_op_run and mvldm_plan_profile treat them as no-ops (serial order is always valid). */
    MVLDM_OP_PAR_BEGIN, MVLDM_OP_PAR_NEXT, MVLDM_OP_PAR_END,
    MVLDM_OP_GATHER_ROWS, MVLDM_OP_ATTN_MERGE
};

typedef struct mvldm_op {
    int32_t kind;
    int32_t tag; /* caller-defined label (layer id) echoed by the profiler */
    union {
        mvldm_igemm_desc igemm;
        struct { const void* x; const void* x1; void* y; const float* gamma; const float* beta; void* stats_ws;
                 int32_t n_img, hw, c0, c1, groups, silu, dtype; float eps; float* stats_out; } groupnorm;
        struct { const void* x; void* y; const float* gamma; const float* beta;
                 int32_t rows, c, dtype; float eps; } layernorm;
        struct { const void* q; const void* k; const void* v; void* out; const int32_t* seg;
                 int32_t ld_q, ld_k, ld_v, ld_o, heads, head_dim, n_seg, max_q_len, dtype; float scale;
                 float* lse; int32_t lse_ld; } attention;
        struct { const int64_t* timesteps; const float* freqs; void* out;
                 int32_t n, dim, flip, dst_dtype; } temb;
        struct { const void* x; void* y; size_t n; int32_t op, src_dtype, dst_dtype; } eltwise;
        struct { const float* eps; const float* x_t; float* x_next; const int32_t* cond_img; const int32_t* uncond_img;
                 const float* coef; const int32_t* step_ptr; void* unet_in;
                 int32_t n_tgt, hw, c, unet_in_c, unet_in_dtype; float cfg_scale; int32_t n_steps; float clip_range; } ddim;
        struct { int32_t* step_ptr; const int64_t* t_table; int64_t* timesteps; const int32_t* tgt_rows;
                 int32_t n_steps, n_rows; } advance;
        struct { const void* src; void* dst; int32_t n_img, c, hw, other_c, other_c_off, dtype, clamp01;
                 float scale, shift; const int32_t* img_map; } layout;
        struct { const float* extrinsics; const float* intrinsics; float* out_nchw; void* out_nhwc; const int32_t* img_map;
                 int32_t n_cam, h, w, nhwc_c, nhwc_c_off, nhwc_dtype, mode, n_origin_octaves, n_dir_octaves, plucker; } rays;
        struct { const float* moments; const float* noise; float* out; int32_t n, c, hw; float scale; } posterior;
        mvldm_wgrad_desc wgrad;
        mvldm_attn_bwd_desc attention_bwd;
        struct { const void* x0; const void* x1; const void* dy; void* dx0; void* dx1; const float* gamma; const float* beta;
                 const float* stats; float* dgamma; float* dbeta; float* workspace; size_t workspace_bytes;
                 int32_t n_img, hw, c0, c1, groups, silu, dtype; } groupnorm_bwd;
        struct { const void* x; const void* dy; void* dx; const float* gamma; float* dgamma; float* dbeta; float* workspace;
                 size_t workspace_bytes; int32_t rows, c, dtype; float eps; } layernorm_bwd;
        struct { const void* x; float* dst; float* workspace; size_t workspace_bytes;
                 int32_t n_seg, rows_per_seg, n, ld, ld_dst, per_seg, accumulate, dtype; } colsum;
        struct { const void* a; const void* b; void* out; size_t rows; int32_t op, d, a_dtype, dtype; } train_eltwise;
        struct { const void* src; void* dst; int32_t n_img, h, w, c, dtype; } resample;      /* pool2x2 / zero_insert2x */
        struct { const float* x0; const float* noise; const float* coef; void* dst; const int32_t* img_map;
                 int32_t n, c, hw, dst_c, dst_c_off, dst_dtype; } add_noise;
        struct { const float* pred; const float* noise; const int32_t* tgt_img; float* loss; void* dpred; double* workspace;
                 int32_t n_tgt, hw, c, accumulate, dpred_c, dpred_dtype; float loss_scale, grad_scale;
                 const float* amp_scale; /* optional: mvldm_mse_loss_amp's S pointer */ } mse;
        struct { void* dst; size_t bytes; } fill;
        struct { const void* src; void* dst; size_t bytes; } memcpy_;
        struct { const void* src; void* dst; const int32_t* src_index; const int32_t* dst_index; size_t row_bytes; int32_t n_rows; } gather;
        struct { const void* oa; const void* ob; void* out; const float* lse_a; const float* lse_b; const int32_t* a_img; const int32_t* b_img;
                 const int32_t* out_img; int32_t n_img, tokens, heads, head_dim, ld_a, ld_b, ld_o, lse_ld_a, lse_ld_b, dtype; } attn_merge;
    } u;
} mvldm_op;

typedef struct mvldm_plan mvldm_plan;
int mvldm_op_run(const mvldm_op* op, mvldm_stream_t stream);                   /* one op, eagerly */
int mvldm_plan_create(const mvldm_op* ops, int n_ops, mvldm_plan** out);      /* ops: host array, copied */
int mvldm_plan_num_ops(const mvldm_plan* p);
int mvldm_plan_run(mvldm_plan* p, mvldm_stream_t stream);                      /* eager launches */
int mvldm_plan_run_range(mvldm_plan* p, int first, int last, mvldm_stream_t stream);
int mvldm_plan_capture(mvldm_plan* p, mvldm_stream_t stream);                  /* record into a hipGraph */
int mvldm_plan_replay(mvldm_plan* p, mvldm_stream_t stream);                   /* launch the captured graph */
/* hipEvent-bracket every op on `stream` (eager), `iters` passes; per_op_ms: host float[n_ops] averages */
int mvldm_plan_profile(mvldm_plan* p, mvldm_stream_t stream, int iters, float* per_op_ms);
void mvldm_plan_destroy(mvldm_plan* p);

#ifdef __cplusplus
}
#endif
#endif /* MVLDM_H */
