/*
 * clipk.h — C-ABI of the MI355X-native CoOp/CoCoOp hot path (libclipk.so).
 *
 * Plain pointers + sizes + a hipStream_t (passed as void*); no torch types.
 * Every device pointer is owned by the caller (the torch caching allocator in
 * the Python host). Kernels never allocate. Encoder handles hold only HOST-side
 * pointer tables to caller-owned, packed, frozen weights.
 *
 * Return value: CLIPK_OK (0); a negative CLIPK_E* for bad arguments (checked on
 * the host BEFORE any launch); a positive hipError_t from a failed launch.
 *
 * Reference interfaces replaced (PyTorch ops inside the reference hot path):
 *   clipk_gemm            nn.Linear / MHA in_proj,out_proj / mlp.c_fc,c_proj / @proj
 *                         (PromptSRC/clip/model.py:171-177, 429; trainers/coop.py:204)
 *   clipk_layernorm_*     LayerNorm (model.py:153-159) fwd / input-grad bwd
 *   clipk_attention_*     nn.MultiheadAttention SDPA core (model.py:181-183, mask 592-598)
 *   clipk_im2col          VisionTransformer.conv1 patch embed as GEMM (model.py:376,402)
 *   clipk_vit_embed_ln    cls cat + pos add + ln_pre (model.py:405-420)
 *   clipk_prompt_assemble PromptLearner.forward cat + TextEncoder pos add
 *                         (trainers/coop.py:259-296, cocoop.py:173-198, coop.py:197)
 *   clipk_ctx_grad        autograd of that cat w.r.t. ctx (coop.py:265, cocoop.py:186-194)
 *   clipk_cosine_logits_* CustomCLIP normalize + logit_scale.exp() * imf @ txt^T
 *                         (coop.py:356-363, cocoop.py:238-251)
 *   clipk_ce_loss         nn.CrossEntropyLoss / MultiClassFocalLoss fwd+bwd
 *                         (coop.py:131-163,324; cocoop.py:66-101,233)
 *   clipk_mixup_images    mixup_data: lam * x + (1 - lam) * x[perm] (independentVL.py:435-449)
 *   clipk_ce_loss_mix     mixup_criterion on CE / focal fwd+bwd (independentVL.py:451-460)
 *   clipk_ntxent_loss     LogitsNTXentLoss / ImageNTXentLoss fwd+bwd
 *                         (coop.py:72-123; independentVL.py:73-112)
 *   clipk_src_head        PromptSRC's normalisations, logits, CE / focal + L1 + KL objective
 *                         fwd+bwd (promptsrc.py:171-213, 296-323)
 *   clipk_probe_head      the linear probe's nn.Linear head on frozen image features plus
 *                         CE / focal, fwd+bwd (this package's LinearProbeCLIP)
 *   clipk_lora_*          LoRA on attn.in_proj_weight: the merged weights W0 + s B A and the
 *                         adapters' gradients (this package's LoRA; loralib's Linear / MergedLinear
 *                         with merged weights, and autograd's dA / dB)
 *   clipk_meta_net_*      CoCoOp Meta-Net Linear-ReLU-Linear (cocoop.py:139-143,182-185)
 *   clipk_sgd_step        torch.optim.SGD momentum/wd step (dassl optim/optimizer.py:105-113)
 *   clipk_sgd_step_multi  the same over a param group's tensors in one launch
 *   clipk_adam_step_multi torch.optim.Adam / AdamW / Adam(amsgrad=True) step over a param
 *                         group's tensors in one launch (dassl optim/optimizer.py adam,
 *                         amsgrad, adamw)
 *   clipk_text_*          TextEncoder.forward + its input-grad backward (coop.py:195-205)
 *   clipk_vit_forward     VisionTransformer.forward (model.py:401-431), frozen, fwd only
 *   clipk_conv2d_nhwc     nn.Conv2d (1x1, 3x3 pad 1) + eval BatchNorm2d + residual + ReLU of
 *                         Bottleneck / the stem (model.py:10-56, 94-150)
 *   clipk_avgpool2_nhwc   nn.AvgPool2d(2) (model.py:27, 34-40, 115)
 *   clipk_attnpool        AttentionPool2d (model.py:58-91)
 *   clipk_resnet_forward  ModifiedResNet.forward (model.py:135-150), frozen, fwd only
 */
#ifndef CLIPK_H
#define CLIPK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* element types. CLIPK_F32S (GEMM input type only): fp32 activations times a weight packed by
 * clipk_split_pack -- the fp32-class GEMM on 16-bit MFMA of PREC "fp32s" (clipk_gemm).
 * CLIPK_F32S16 (GEMM input type only): the same product for an fp16-valued weight (every lo part
 * of its clipk_split_pack output zero, as for every released CLIP checkpoint -- the reference
 * loads them from the fp16 archive, PromptSRC/clip/clip.py:154-180), whose B operand is the
 * COMPACT weight of clipk_split_hi16: fp16 [N, K] = CLIPK_SPLIT_SCALE * W exactly, 2 B per element
 * (ldb == K). The hi(a) lo(b) product, exactly zero, is not formed: 2 MFMAs per product instead of
 * 3, and half of B's bytes staged; results bitwise those of CLIPK_F32S on the packed weight. */
enum { CLIPK_F32 = 0, CLIPK_F16 = 1, CLIPK_BF16 = 2, CLIPK_F32S = 3, CLIPK_F32S16 = 4 };

/* status codes (hipError_t values > 0 pass through) */
enum {
  CLIPK_OK = 0,
  CLIPK_EINVAL = -1,     /* null pointer / bad enum */
  CLIPK_ESHAPE = -2,     /* shape violates a kernel constraint */
  CLIPK_EDTYPE = -3,     /* unsupported dtype combination */
  CLIPK_EWORKSPACE = -4, /* workspace too small */
  CLIPK_ERANGE = -5,     /* an input outside the range the kernel supports (clipk_split_pack,
                            clipk_split_hi16) */
  CLIPK_EHIP = -6        /* a HIP runtime call of a synchronous check failed (clipk_split_*) */
};

/* GEMM epilogues:  acc = A[M,K] . B[N,K]^T  (fp32 accumulate)                         */
enum {
  CLIPK_EPI_BIAS = 0,       /* out(out_dtype) = acc + bias                                */
  CLIPK_EPI_BIAS_RES = 1,   /* out = acc + bias + res; out and res both f32, or both the
                               16-bit in_dtype (16-bit residual stream)                  */
  CLIPK_EPI_BIAS_QGELU = 2, /* out = quickgelu(acc + bias); out2 (optional) = acc + bias */
  CLIPK_EPI_DQGELU = 3,     /* out = acc * quickgelu'(aux)                                */
  CLIPK_EPI_NONE = 4        /* out = acc                                                  */
};
/* Operand flag OR-ed into epi: A is a pre-activation h and the GEMM consumes quickgelu(h)
 * (applied to each 16-B chunk of A as it is staged into LDS), so the producer of h need
 * not also write quickgelu(h) (the text c_proj forward). 16-bit in_dtype only. */
enum { CLIPK_A_QGELU = 0x100 };
/* Epilogue flag OR-ed into epi, training's QuickGELU pair (replaces keeping the pre-activation,
 * PromptSRC/clip/model.py:162-164, 177): with CLIPK_EPI_BIAS_QGELU, out2 = quickgelu'(acc + bias)
 * instead of acc + bias; with CLIPK_EPI_DQGELU, aux already holds quickgelu'(h) and
 * out = acc * aux. The forward epilogue has sigmoid(1.702 h) in hand (three more VALU per element);
 * the backward epilogue drops its exp + rcp per element. Also accepted by clipk_gemm_ln (fold
 * form of EPI_BIAS_QGELU) and clipk_gemm_splitk (EPI_BIAS_QGELU). */
enum { CLIPK_QGELU_DERIV = 0x200 };
/* PREC fp32s operand flags OR-ed into epi (split in_dtype CLIPK_F32S / CLIPK_F32S16, fp32 out).
 * The split GEMM forms each activation's fp16 parts hi = fp16(x), lo = fp16(x - hi) itself; a
 * PRE-SPLIT operand holds them already: [rows, K] 4-byte elements, per 8 consecutive k 16 B of hi
 * parts then 16 B of lo parts (clipk_split_pack's layout at scale 1).
 *  CLIPK_OUT_SPLIT: out is stored pre-split (the fp32 result's parts; for the next GEMM's A).
 *    clipk_gemm (EPI_BIAS_QGELU [| QGELU_DERIV], EPI_DQGELU | QGELU_DERIV) and the folds
 *    clipk_gemm_ln / clipk_gemm_ln_gamma (c_fc).
 *  CLIPK_A_SPLIT: A is given pre-split, as such a producer wrote it; the GEMM forms no split.
 *    clipk_gemm (EPI_NONE, EPI_BIAS_RES, EPI_DQGELU | QGELU_DERIV), the producer form of
 *    clipk_gemm_ln, clipk_gemm_ln_gamma (A = the split parts of x * gamma, which the call then
 *    does not apply again: clipk_gemm_ln_stats_split writes them) and clipk_gemm_ln_stats_split.
 *  (CLIPK_OUT2_SPLIT_GAMMA: internal to clipk_gemm_ln_stats_split.)
 * Results are bitwise those of the same GEMMs on the fp32 values: the parts are the ones the GEMM
 * would form (PREC fp32s: the split VALU leaves the K loop's critical path). */
enum { CLIPK_OUT_SPLIT = 0x400, CLIPK_A_SPLIT = 0x800, CLIPK_OUT2_SPLIT_GAMMA = 0x1000 };

const char* clipk_version(void);
/* sha256 (hex) over the sources this library was built from: csrc/{*.hip,*.h,Makefile} and
 * include/clipk.h, in file-name order, each as "<sha256 of content>  <relative path>\n"
 * (fsp_amd/_native.py source_digest; the loader refuses a library built from another tree). */
const char* clipk_source_digest(void);
const char* clipk_strerror(int status);
int clipk_device_arch_ok(void); /* 1 if device 0 is gfx950 */

/* ---------------------------------------------------------------- primitives */
/* Constraints: N % 128 == 0, K % 64 == 0 (16-bit) or K % 32 == 0 (f32); lda,ldb,ldo
 * multiples of 8 elements; A/B of in_dtype; bias/res fp32; aux of aux_dtype. */
int clipk_gemm(int in_dtype, int out_dtype, int epi, int M, int N, int K,
               const void* A, int lda, const void* B, int ldb,
               const float* bias, const void* res, int ldr,
               void* out, int ldo, void* out2, const void* aux, int aux_dtype, int ldaux,
               void* stream);

/* fp32-class GEMM on the 16-bit MFMA (PREC "fp32s"; the reference runs these Linear layers in
 * fp32, PromptSRC/clip/model.py:171-177, 699). clipk_split_pack stores W [N, K] (fp32, row
 * stride ldw) as CLIPK_SPLIT_SCALE * W split into fp16 parts hi = fp16(x), lo = fp16(x - hi):
 * per 8 consecutive k, 16 B of hi then 16 B of lo (4 B per element, the out buffer holds
 * N * K * 4 bytes; K % 32 == 0). |W| must stay below 65504 / CLIPK_SPLIT_SCALE: the call
 * checks it (one pass over W, then a stream synchronisation: packing runs once per model) and
 * returns CLIPK_ERANGE for a larger or non-finite value. clipk_gemm(in_dtype = CLIPK_F32S, ...)
 * then takes A fp32 [M, K] and B = the packed weight (ldb must equal K) and forms every product as hi(a) hi(b) + hi(a) lo(b) + lo(a) hi(b) with
 * v_mfma_f32_16x16x32_f16 (fp32 accumulate; A split in registers as its fragments are read),
 * scaled by 1 / CLIPK_SPLIT_SCALE before the epilogue: ~22 significant bits per operand, the
 * fp32 result to ~1e-6 relative. out / res / aux fp32 (epilogues as above). */
#define CLIPK_SPLIT_SCALE 64.0f
int clipk_split_pack(int N, int K, const float* W, int ldw, void* out, void* stream);
/* *result = 1 when every lo part of clipk_split_pack's output `packed` ([N, K] split elements) is
 * zero (the weight is fp16-valued: clipk_split_hi16 may compact it for CLIPK_F32S16), 0 when not.
 * Returns CLIPK_OK, or a negative status (CLIPK_EHIP for a failed HIP call; *result untouched).
 * One pass, then a stream synchronisation (checked once per weight, at model construction). */
int clipk_split_lo_zero(int N, int K, const void* packed, int* result, void* stream);
/* The CLIPK_F32S16 B operand: out fp16 [N, K] = the hi parts of clipk_split_pack's output `packed`
 * (= CLIPK_SPLIT_SCALE * W exactly). CLIPK_ERANGE when a lo part is nonzero (W is not fp16-valued;
 * out is then unspecified). One pass, then a stream synchronisation. */
int clipk_split_hi16(int N, int K, const void* packed, void* out, void* stream);

/* Split-K form of clipk_gemm for small M (the ViT at training batch sizes, whose 128x128
 * tile grid would leave most CUs idle): the K range is cut into `splits` slices whose fp32
 * partials go to the caller's workspace ws ([splits][M][N] fp32), then one elementwise pass
 * sums them in slice order (deterministic) and applies the epilogue. Same arguments and
 * epilogues as clipk_gemm except EPI_DQGELU; splits <= 0 picks clipk_gemm_auto_splits;
 * one slice is plain clipk_gemm (ws unused). */
int clipk_gemm_auto_splits(int in_dtype, int M, int N, int K);
size_t clipk_gemm_splitk_ws_bytes(int M, int N, int splits);
int clipk_gemm_splitk(int in_dtype, int out_dtype, int epi, int M, int N, int K,
                      const void* A, int lda, const void* B, int ldb,
                      const float* bias, const void* res, int ldr,
                      void* out, int ldo, void* out2, int splits, void* ws, size_t ws_bytes,
                      void* stream);

/* LayerNorm folded into the GEMM that consumes it (the text encoder's ln_1 -> attn.in_proj
 * and ln_2 -> mlp.c_fc, PromptSRC/clip/model.py:153-159, 185-188):
 *   LN(x) W^T + b = rstd * (x W'^T - mean * s) + c,  W' = W diag(gamma) (in_dtype),
 *   s_j = sum_k W'[j,k], c_j = b_j + sum_k beta_k W[j,k] (fp32),
 * so the GEMM reads the residual stream x itself and no normalised copy is written.
 * Two modes, 16-bit in_dtype == out dtype, or in_dtype CLIPK_F32S (A, out, res fp32; B = W'
 * split-packed by clipk_split_pack; s summed over the packed value, (hi + lo) / 64):
 *  - colsum == NULL: EPI_BIAS_RES (the residual-stream producer); in addition, per row m and
 *    64-column group g of the ROUNDED output, stats[(m * N/64 + g) * 2 + {0, 1}] = (sum, sum of
 *    squared deviations from the group's mean) (fp32);
 *  - colsum != NULL (stats NULL): EPI_BIAS or EPI_BIAS_QGELU with A = x, B = W', bias = c,
 *    colsum = s and rnb = per-row (rstd, -rstd * mean) pairs of A's rows (fp32 [M][2]).
 * clipk_ln_stats_merge turns a producer's partials (width / 64 per row) into any of mean, rstd
 * (fp32 [rows]) and rnb (exact pairwise merge in a fixed order, eps 1e-5). Shape constraints as
 * clipk_gemm. */
/* The fold with the LayerNorm weight on A (PREC fp32s, in_dtype CLIPK_F32S / CLIPK_F32S16; the
 * consumer form of clipk_gemm_ln): A = x fp32 [M, K] (K <= 1024), B = W packed (ldb == K), each
 * x[m, k] * gamma[k] rounded to fp32 before its split; colsum = rowsums of W diag(gamma) over the
 * packed value / 64 (fp32 [N]), bias = b + W beta, rnb as in clipk_gemm_ln. Keeps an fp16-valued
 * W fp16-valued, so CLIPK_F32S16's 2 MFMAs per product apply to the folded GEMMs too. */
int clipk_gemm_ln_gamma(int in_dtype, int epi, int M, int N, int K, const void* A, int lda, const void* B, int ldb,
                        const float* bias, void* out, int ldo, void* out2, const float* colsum, const float* rnb,
                        const float* gamma, void* stream);
int clipk_gemm_ln(int in_dtype, int epi, int M, int N, int K, const void* A, int lda, const void* B, int ldb,
                  const float* bias, const void* res, int ldr, void* out, int ldo, void* out2,
                  float* stats, const float* colsum, const float* rnb, void* stream);
/* The statistics producer of clipk_gemm_ln (EPI_BIAS_RES [| CLIPK_A_SPLIT], colsum NULL), in_dtype
 * CLIPK_F32S16, that also stores out2 [M, N] = the pre-split form (CLIPK_OUT_SPLIT) of out * gamma,
 * the fp32 products the next fold (clipk_gemm_ln_gamma, gamma = its LayerNorm weight) would form:
 * that fold then reads out2 with CLIPK_A_SPLIT. The residual stream out stays fp32. */
int clipk_gemm_ln_stats_split(int in_dtype, int epi, int M, int N, int K, const void* A, int lda, const void* B,
                              int ldb, const float* bias, const void* res, int ldr, void* out, int ldo, float* stats,
                              const float* gamma, void* out2, void* stream);
int clipk_ln_stats_merge(int rows, int width, const float* stats, float* mean, float* rstd, float* rnb,
                         void* stream);
/* clipk_ln_stats_merge(M, K, stats, mean, rstd, rnb) followed by the fold clipk_gemm_ln(...,
 * colsum, rnb) (res NULL), as ONE launch where the library covers the shape in-kernel (16-bit,
 * K = 512, the 192-row tile configuration: the batch-1 text encoder's LN-fold GEMMs), else as
 * those two calls. Outputs are bitwise those of the two calls: out / out2, mean and rstd
 * (optional) and rnb (required). Replaces the merge launch between a producer and its fold
 * (PromptSRC/clip/model.py:153-159, 185-188: ln_1 / ln_2 of each residual block). */
int clipk_gemm_ln_merge(int in_dtype, int epi, int M, int N, int K, const void* A, int lda, const void* B,
                        int ldb, const float* bias, void* out, int ldo, void* out2, const float* stats,
                        const float* colsum, float* mean, float* rstd, float* rnb, void* stream);
/* 1 when clipk_gemm_ln_merge runs the shape as one launch, 0 when as the two calls. */
int clipk_gemm_ln_merge_fused(int in_dtype, int M, int N, int K);
/* PREC fp32s tile policy query (in_dtype CLIPK_F32S / CLIPK_F32S16; epi with its operand flags as
 * the launching call takes it; lnm 0 for clipk_gemm, 1 / 2 for clipk_gemm_ln's producer / fold, 4
 * for clipk_gemm_ln_gamma): the height of the ping-pong tile such a launch takes at (M, N) -- 192,
 * or 256 for the pre-split classes built at 256 rows (split mode 2: the c_fc and qkv folds with
 * CLIPK_A_SPLIT) where (tiles on the busiest CU) x (cost of one tile) is smaller; 0 where the
 * shape does not run the ping-pong tiles. Knob CLIPK_GEMM_T256 (read once per process): 0 never
 * 256 rows, 1 (default) by that rule, 2 always where built. Outputs are bitwise the same at
 * either height. clipk_gemm_t256_cost: the rule's cost of a 256-row tile over a 192-row one for
 * the launch's class, 0 where none is built. */
int clipk_gemm_split_tile_rows(int in_dtype, int epi, int lnm, int M, int N);
double clipk_gemm_t256_cost(int in_dtype, int epi, int lnm);
/* Benchmark knob: force the 16-bit GEMM tile configuration (0: 128x128, 1: 256x256
 * (persistent above 2 x CUs tiles), 2: 256x128, 3: 256x256 non-persistent, 6: 192x256;
 * -1 = automatic by shape; other values: CLIPK_EINVAL). Not needed for normal use. */
int clipk_gemm_set_config(int cfg);

/* Image preprocessing (Dassl/torchvision Resize+CenterCrop / RandomResizedCrop+flip,
 * ToTensor, Normalize; transforms.py:206-354): Pillow-exact bicubic resampling of a crop
 * window of each uint8 HWC image (src: packed images), from host-built fixed-point tables
 * (fsp_amd/data/preprocess.py documents desc/tables); out fp32 [B,3,S,S] normalised with
 * mean/std, or the uint8 pixels when out_uint8. tmp: sum over images of rows*S*3 bytes. */
int clipk_image_resample(int B, int S, int rows_max, const void* src, const long long* desc,
                         const int* tables, void* tmp, const float* mean, const float* stdv,
                         int out_uint8, void* out, void* stream);

/* clipk_image_resample on images that stay where they lie: desc[0] of every image is the ABSOLUTE
 * device address of its first byte (an image bank's chunk, an upload buffer, or both in one batch),
 * so there is no src argument. The same two kernels, arithmetic, desc and tables otherwise. The
 * caller checks every window against the image's rows and row stride: the kernels read
 * desc[0] + ((desc[3] + r) * desc[1] + desc[2] + tap) * 3 + c without a bound of their own. */
int clipk_image_resample_at(int B, int S, int rows_max, const long long* desc, const int* tables, void* tmp,
                            const float* mean, const float* stdv, int out_uint8, void* out, void* stream);

/* The coefficient tables of clipk_image_resample, built on the device (csrc/resample_ops.h: Pillow's
 * precompute_coeffs + normalize_coeffs_8bpc for the bicubic filter, every step in double and in
 * Pillow's order, the sum of a row's taps taken tap after tap by one thread). params: DEVICE int64
 * [B, CLIPK_RESAMPLE_PARAMS], per image
 *   [0] window width w, [1] resized width rw, [2] output window origin ox, [3] h-table offset,
 *   [4] h ksize, [5] window height h, [6] resized height rh, [7] oy, [8] v-table offset, [9] v ksize,
 *   [10] S (rows per table, <= the argument S), [11] ty0 (subtracted from the v rows' first tap).
 * Writes into tables (int32, offsets in ints: desc[6] / desc[8] of clipk_image_resample) per image
 * S h rows for the outputs ox .. ox + S - 1 of w -> rw and S v rows for oy .. oy + S - 1 of h -> rh,
 * each (first tap, taps used, ksize coefficients, zero past the taps used): the block
 * fsp_amd/data/preprocess.py _tables builds on the host, bit for bit. ksize must be the
 * filter's 2 * ceil(2 * max(in / out, 1)) + 1 of its axis (a row never has more taps); it is the
 * caller's to compute, as the row stride bounds every write. One thread per row, B * 2 * S rows.
 * CLIPK_EINVAL: a null pointer; CLIPK_ESHAPE: B < 0, S <= 0. B == 0: CLIPK_OK, nothing launched.
 * clipk_resample_tables_host: the same arguments with HOST pointers (stream ignored), the same
 * header functions in a plain loop; it also checks every record (extents >= 1, 0 <= origin,
 * origin + S <= resized extent, S within 1..argument S, ksize the filter's, offsets >= 0) and
 * returns CLIPK_ESHAPE before writing anything when one fails. */
enum { CLIPK_RESAMPLE_PARAMS = 12 };
int clipk_resample_tables(int B, int S, const long long* params, int* tables, void* stream);
int clipk_resample_tables_host(int B, int S, const long long* params, int* tables, void* stream);

/* Colour augmentations on the resampled pixels (torchvision ColorJitter / RandomGrayscale on PIL
 * images, i.e. Pillow's ImageEnhance.Brightness / Contrast / Color, convert("HSV") and convert("L");
 * csrc/preprocess.hip "colour stage", DESIGN §3 "Colour kernels"): every uint8 result is Pillow's.
 * pix: uint8 planar [B,3,S,S], what clipk_image_resample(out_uint8 = 1) writes. prog: HOST int32
 * [B, CLIPK_COLOR_DESC] -- per image [0] the number of ops n (0..CLIPK_COLOR_MAX_OPS), [1..5] the
 * op codes in the order they run, [6..10] their parameters (the bits of the fp32 blend factor for
 * BRIGHTNESS / CONTRAST / SATURATION, the integer shift 0..255 for HUE, unused for GRAYSCALE), [11]
 * zero. The call checks prog on the host, then copies it to prog_dev (device, B * CLIPK_COLOR_DESC
 * * 4 bytes, caller-owned) on the stream and launches ONE kernel. out: fp32 [B,3,S,S] =
 * ((float)v / 255.0f - mean[c]) / stdv[c], the expression of clipk_image_resample's epilogue (an
 * image with n = 0 is bitwise that call's out_uint8 = 0 output), or the uint8 pixels when out_uint8.
 * One workgroup per image; the image lives in LDS while its program runs when 3 * S * S bytes fit
 * (S <= 224), otherwise the same code runs in place in pix, whose contents are then unspecified
 * afterwards. out must not be pix. B == 0: CLIPK_OK, nothing launched. CLIPK_EINVAL: pix, prog,
 * prog_dev or out null, mean / stdv null without out_uint8, out == pix, an unknown op code, a blend
 * factor that is negative or not finite, a shift outside 0..255; CLIPK_ESHAPE: B < 0, S <= 0, S >
 * 4096, n outside 0..CLIPK_COLOR_MAX_OPS. */
enum { CLIPK_COLOR_BRIGHTNESS = 1, CLIPK_COLOR_CONTRAST = 2, CLIPK_COLOR_SATURATION = 3,
       CLIPK_COLOR_HUE = 4, CLIPK_COLOR_GRAYSCALE = 5 };
enum { CLIPK_COLOR_MAX_OPS = 5, CLIPK_COLOR_DESC = 12 };
int clipk_image_color(int B, int S, void* pix, const int* prog, int* prog_dev, const float* mean,
                      const float* stdv, int out_uint8, void* out, void* stream);

/* clipk_image_color followed, in the same launch, by PIL.ImageFilter.GaussianBlur on the image
 * (Pillow's approximation: three box passes of a fractional radius along x over every row, then
 * three along y over every column, each on the uint8 output of the one before, edges repeating
 * the edge pixel; csrc/color_ops.h box_line, DESIGN §3 "Blur"): every uint8 result is Pillow's.
 * The arguments are clipk_image_color's, but prog is HOST int32 [B, CLIPK_COLORBLUR_DESC] and
 * prog_dev holds B * CLIPK_COLORBLUR_DESC * 4 bytes: per image [0..11] as in clipk_image_color,
 * [12] the integer box radius r (-1: this image is not blurred and takes clipk_image_color's path,
 * bit for bit; 0..CLIPK_BLUR_MAX_RADIUS otherwise), [13] ww and [14] fw, the 24-bit fixed-point
 * weights of the 2r + 1 inner samples and of the two outer ones (fsp_amd/data/preprocess.py
 * gaussian_blur_params derives r, ww, fw from sigma as Pillow does), [15] zero. One output of a
 * pass is (sum_inner * ww + sum_outer * fw + 2^23) >> 24 in 32 unsigned bits. The same errors as
 * clipk_image_color, and CLIPK_EINVAL for r outside -1..CLIPK_BLUR_MAX_RADIUS or, with r >= 0,
 * ww outside 1..2^24, fw < 0, or (2r + 1) * ww + 2 * fw > 2^24 (the 32-bit sum would overflow);
 * checked on the host before anything is copied or launched. */
enum { CLIPK_COLORBLUR_DESC = 16, CLIPK_BLUR_MAX_RADIUS = 7 };
int clipk_image_color_blur(int B, int S, void* pix, const int* prog, int* prog_dev, const float* mean,
                           const float* stdv, int out_uint8, void* out, void* stream);

/* Diagnostic: per-block / per-tile s_memrealtime marks of the last GEMM launch, recorded
 * only when the process runs with CLIPK_GEMM_STAMP set (synchronises the device). */
int clipk_gemm_stamps(void* host, size_t bytes);

/* cls cat + pos add + ln_pre with n_vpt visual prompt rows appended per image (IVLP / MaPLe /
 * PromptSRC, model.py:413-420, 465-472): x[b*(L+n_vpt) + t] = ln_pre(t < L ? embed(b, t) :
 * vpt[t-L]) (prompts get no positional embedding). */
int clipk_vit_embed_ln_vpt(int B, int L, int n_vpt, int width, const float* patch, const float* cls,
                           const float* pos, const float* vpt, const float* gamma, const float* beta, float* x,
                           void* stream);

/* Deep prompts (ResidualAttentionBlock_IVLP / _MaPLe.forward, model.py:229-256, 287-331): the
 * rows a layer's learnable tokens replace. rows[p*n_per + i] = i-th row taking prompt row p.
 * inject: dst[rows[p*n_per+i]] = (dst dtype) src[p]   (src [n_ctx, width] fp32).
 * collect: out[p] (+= when accumulate) sum_i src[rows[p*n_per+i]] in a fixed order, then those
 * rows of src (and of src2, a second copy of the same stream, when given) are zeroed. */
int clipk_rows_inject(int dst_dtype, int n_ctx, int n_per, int width, const float* src, const int* rows,
                      void* dst, int ldd, void* stream);
int clipk_rows_collect(int src_dtype, int n_ctx, int n_per, int width, void* src, int lds, void* src2,
                       int src2_dtype, int lds2, const int* rows, float* out, int accumulate, int zero_src,
                       void* stream);

/* y = LN(x[row]) for rows r in [0,rows): x row = in_rows ? in_rows[r] : r.
 * out of out_dtype with row stride ldo; mean/rstd (optional, fp32 [rows]). width%64==0, <=1024 */
int clipk_layernorm_fwd(int out_dtype, int rows, int width, const float* x, int ldx,
                        const int* in_rows, const float* gamma, const float* beta,
                        void* out, int ldo, float* mean, float* rstd, void* stream);
/* same with x of x_dtype (fp32 or 16-bit: the 16-bit text residual stream) */
int clipk_layernorm_fwd_x(int x_dtype, int out_dtype, int rows, int width, const void* x, int ldx,
                          const int* in_rows, const float* gamma, const float* beta,
                          void* out, int ldo, float* mean, float* rstd, void* stream);

/* dx = LN-input-grad(dy; x, gamma, mean, rstd) (+ dres). dy of dy_dtype; x row = x_rows ? x_rows[r] : r;
 * outputs written at row out_rows ? out_rows[r] : r of dx (f32) and dx_lp (lp_dtype, optional;
 * lp_dtype CLIPK_F32S: dx_lp in the pre-split form of CLIPK_A_SPLIT, the next split GEMMs' A). */
int clipk_layernorm_bwd(int dy_dtype, int rows, int width, const void* dy, int lddy, const float* x, int ldx,
                        const int* x_rows, const float* gamma, const float* mean, const float* rstd,
                        const float* dres, int lddres, float* dx, void* dx_lp, int lp_dtype,
                        const int* out_rows, int ldo, void* stream);
/* same with x of x_dtype */
int clipk_layernorm_bwd_x(int x_dtype, int dy_dtype, int rows, int width, const void* dy, int lddy,
                          const void* x, int ldx, const int* x_rows, const float* gamma,
                          const float* mean, const float* rstd, const float* dres, int lddres,
                          float* dx, void* dx_lp, int lp_dtype, const int* out_rows, int ldo,
                          void* stream);
/* same with the residual gradient dres of dres_dtype: fp32, or lp_dtype (a 16-bit residual-
 * gradient stream; dres may then alias dx_lp, updated in place). dx (fp32) may be NULL when
 * dx_lp is given. */
int clipk_layernorm_bwd_x2(int x_dtype, int dy_dtype, int rows, int width, const void* dy, int lddy,
                           const void* x, int ldx, const int* x_rows, const float* gamma,
                           const float* mean, const float* rstd, const void* dres, int dres_dtype,
                           int lddres, float* dx, void* dx_lp, int lp_dtype, const int* out_rows,
                           int ldo, void* stream);

/* Multi-head self-attention core on packed qkv rows [(s*L+t), 3*heads*64] (head dim 64):
 * out[(s*L+t), h*64+d]; lse[(s*L+t)*heads + h] (optional) = logsumexp of scaled scores. */
int clipk_attention_fwd(int dtype, int nseq, int L, int heads, int causal,
                        const void* qkv, int ldqkv, void* out, int ldo, float* lse, void* stream);
/* The same with flags (0: exactly clipk_attention_fwd):
 * CLIPK_ATTN_SPLIT -- fp32 tensors on the 16-bit MFMA (PREC fp32s), any L > 16, causal or not: every
 * operand element x is taken as hi = fp16(x), lo = fp16(x - hi) and every product (Q.K^T, P.V) as
 * hi.hi + hi.lo + lo.hi with fp32 accumulation, the three-term rule of CLIPK_F32S; softmax, lse and
 * 1 / l stay fp32. No range scaling: a part beyond fp16's range gives inf / NaN outputs. For
 * L <= 16 the flagged call runs the exact-fp32 short kernel of the unflagged one.
 * CLIPK_ATTN_OUT_SPLIT -- out is stored in the pre-split form of CLIPK_A_SPLIT (per 8 consecutive
 * columns 16 B of hi parts, then 16 B of lo parts, of the fp32 o the call stores without the flag:
 * bitwise the parts a split GEMM forms from it), for out_proj's A; lse is unchanged. Valid only
 * together with CLIPK_ATTN_SPLIT, L > 16 and ldo % 8 == 0. clipk_attention_bwd reads o as fp32
 * values: it must not be handed such an o.
 * CLIPK_EINVAL, before any launch: a flag with a 16-bit dtype, CLIPK_ATTN_OUT_SPLIT outside the
 * conditions above, an unknown bit. */
enum { CLIPK_ATTN_SPLIT = 1, CLIPK_ATTN_OUT_SPLIT = 2 };
int clipk_attention_fwd_ex(int dtype, int nseq, int L, int heads, int causal,
                           const void* qkv, int ldqkv, void* out, int ldo, float* lse, int flags,
                           void* stream);

/* Input-grad backward of the attention core, any L (L <= 16: one MFMA tile; longer: two MFMA
 * passes, dK/dV per key tile and dQ per query tile; VALU for fp32): dqkv (grad_dtype) from qkv
 * and the saved forward output ofwd (dtype), dout (grad_dtype) and lse. */
int clipk_attention_bwd(int dtype, int grad_dtype, int nseq, int L, int heads, int causal,
                        const void* qkv, int ldqkv, const void* ofwd, int ldof, const void* dout,
                        int lddo, const float* lse, void* dqkv, int lddqkv, void* stream);

/* Shared-prefix packed attention (text, causal). Rows of group g (stride R) hold the P
 * prefix rows shared by all sequences of the group, then each sequence's own rows. The
 * class rows are covered in order by ntiles tiles of <= 16 rows holding whole sequences:
 * tiles[2t], tiles[2t+1] = (group-relative first row, rows); row_first[r] (r < R) = first
 * row of the sequence that row r belongs to (0 for prefix rows). A class row attends to all
 * P prefix keys plus the rows of its own sequence causally; the prefix rows attend among
 * themselves causally. 1 <= P <= 16. Exact restatement of the causal attention of the
 * unpacked [C, L] prompts (attention_prefix.hip). */
int clipk_attention_prefix_fwd(int dtype, int G, int P, int R, int ntiles, const int* tiles,
                               const int* row_first, int heads, const void* qkv, int ldqkv, void* out,
                               int ldo, float* lse, void* stream);
/* Backward; ws >= clipk_attention_prefix_ws_bytes(G, ntiles, heads) holds the per-chunk fp32
 * partial dK/dV of the prefix rows (reduced in a fixed order). grad_dtype CLIPK_F32S (dtype
 * CLIPK_F32, PREC fp32s): fp32 dout, dqkv stored in the pre-split form of CLIPK_A_SPLIT (the qkv
 * input-grad GEMM's A; ldqkv % 8 == 0), the parts of the same fp32 values. */
size_t clipk_attention_prefix_ws_bytes(int G, int ntiles, int heads);
int clipk_attention_prefix_bwd(int dtype, int grad_dtype, int G, int P, int R, int ntiles,
                               const int* tiles, const int* row_first, int heads, const void* qkv,
                               int ldqkv, const void* ofwd, int ldof, const void* dout, int lddo,
                               const float* lse, void* dqkv, int lddqkv, void* ws, size_t ws_bytes,
                               void* stream);

/* The same with flags: CLIPK_PREFIX_CLS_GROUP0 -- every group's class rows read their q|k|v from
 * group 0's rows (the text encoder's layer 0, where the class rows enter every group with the
 * same values: clipk_encoder_set_input_rows; rows [P, R) of groups >= 1 of qkv are then never
 * read, so no copies of group 0's are written). Prefix rows, outputs, dout, lse per group.
 * CLIPK_PREFIX_SPLIT -- fp32 tensors on the 16-bit MFMA (PREC fp32s): every operand element x is
 * taken as hi = fp16(x), lo = fp16(x - hi) and every product (Q.K^T, P.V; in the backward dO.V^T,
 * dS.K, dS^T.Q, P^T.dO) as hi.hi + hi.lo + lo.hi with fp32 accumulation, the three-term rule of
 * CLIPK_F32S; softmax, lse and delta = sum_j P.dP stay fp32. Valid only with dtype CLIPK_F32 (the
 * backward: grad_dtype CLIPK_F32 or CLIPK_F32S), otherwise CLIPK_EINVAL; combines with
 * CLIPK_PREFIX_CLS_GROUP0. The backward accepts ofwd and does not read it. A part beyond fp16's
 * range gives inf / NaN outputs. Without the flag the fp32 calls run the exact-fp32 kernels.
 * CLIPK_PREFIX_OUT_SPLIT (forward only) -- out is stored in the pre-split form of CLIPK_A_SPLIT
 * (per 8 consecutive columns 16 B of hi parts, then 16 B of lo parts, of the fp32 o the call
 * stores without the flag: bitwise the parts a split GEMM forms from it), for out_proj's A. Valid
 * only together with CLIPK_PREFIX_SPLIT and ldo % 8 == 0, otherwise CLIPK_EINVAL; the backward
 * rejects the flag (CLIPK_EINVAL): no kernel reads such an o as fp32 values. lse is unchanged. */
enum { CLIPK_PREFIX_CLS_GROUP0 = 1, CLIPK_PREFIX_SPLIT = 2, CLIPK_PREFIX_OUT_SPLIT = 4 };
int clipk_attention_prefix_fwd_ex(int dtype, int G, int P, int R, int ntiles, const int* tiles,
                                  const int* row_first, int heads, const void* qkv, int ldqkv, void* out,
                                  int ldo, float* lse, int flags, void* stream);
int clipk_attention_prefix_bwd_ex(int dtype, int grad_dtype, int G, int P, int R, int ntiles,
                                  const int* tiles, const int* row_first, int heads, const void* qkv,
                                  int ldqkv, const void* ofwd, int ldof, const void* dout, int lddo,
                                  const float* lse, void* dqkv, int lddqkv, void* ws, size_t ws_bytes,
                                  int flags, void* stream);

/* Patch extraction: img fp32 [B,3,R,R] -> out [B*G*G, Kp] (out_dtype), K index c*p*p+ky*p+kx,
 * zero padded to Kp >= 3*p*p. */
int clipk_im2col(int out_dtype, int B, int res, int patch, int Kp, const float* img, void* out,
                 void* stream);

/* x[b*L + t] = ln_pre( (t==0 ? cls : patch[b*(L-1) + t-1]) + pos[t] ), L = G*G+1, f32 out. */
int clipk_vit_embed_ln(int B, int L, int width, const float* patch, const float* cls,
                       const float* pos, const float* gamma, const float* beta, float* x,
                       void* stream);

/* Prompt assembly (+ positional embedding) for nseq = B*C sequences of length L:
 *   s = b*C + c;  m = src_map[c*L + t]
 *   x0[s*L+t] = (m >= 0 ? emb[(c*77 + m)*W] : ctx[b*ctx_sb + c*ctx_sc + (-1-m)*W] + bias[b*W]) + pos[t*W]
 * bias may be NULL (CoOp). */
int clipk_prompt_assemble(int B, int C, int L, int W, const int* src_map, const float* emb,
                          const float* ctx, long ctx_sb, long ctx_sc, const float* bias,
                          const float* pos, float* x0, void* stream);

/* d ctx_shifted: dctx[b*out_sb + c*out_sc + k*W + w] = sum over c' in class group of
 *   dx0[((b*C + c')*L + pos_of(c',k))*W + w]   where pos_of from ctx_pos[c'*n_ctx + k].
 * csc != 0: one output per class (no sum over c). Deterministic fixed-order sums. */
int clipk_ctx_grad(int B, int C, int L, int W, int n_ctx, int csc, const int* ctx_pos,
                   const float* dx0, float* dctx, void* stream);

/* Packed-prompt assembly: x0[g*R + r] = token(c,t) (+ctx slot + bias[g]) + pos[t] with
 * c*L + t = row_tab[r] and the src_map convention above (ctx offset g*ctx_sg + c*ctx_sc). */
int clipk_prompt_assemble_rows(int G, int R, int C, int L, int W, const int* row_tab,
                               const int* src_map, const float* emb, const float* ctx, long ctx_sg,
                               long ctx_sc, const float* bias, const float* pos, float* x0,
                               void* stream);
/* dctx[(g*n_ctx + k)*W + w] = sum_{i in [slot_ptr[k], slot_ptr[k+1])} dx0[(g*R + slot_rows[i])*W + w]. */
int clipk_ctx_grad_rows(int G, int R, int W, int n_ctx, const int* slot_ptr, const int* slot_rows,
                        const float* dx0, float* dctx, void* stream);

/* CoCoOp's two prompt-parameter gradients of packed prompts in one launch (PromptAssembleFn
 * backward, cocoop.py:189-197 ctx_shifted = ctx + bias): with d(g, k) = the clipk_ctx_grad_rows
 * sum of slot k's rows of group g, dctx[k*W + w] = sum_g d(g, k)[w] (g order) and, when dbias is
 * given, dbias[g*W + w] = sum_k d(g, k)[w] (k order). Replaces the per-(g, k) output + two sums. */
int clipk_ctx_bias_grad_rows(int G, int R, int W, int n_ctx, const int* slot_ptr, const int* slot_rows,
                             const float* dx0, float* dctx, float* dbias, void* stream);

/* logits[b,c] = scale * <imf[b], txt[row]> / |txt[row]| / |imf[b]|,
 * row = per_image ? b*C + c : c.  tnorm[row] (optional out) = |txt[row]|. */
int clipk_cosine_logits_fwd(int B, int C, int E, int per_image, float scale, const float* imf,
                            const float* txt, float* logits, float* inv_tnorm, float* inv_inorm,
                            void* stream);
/* d txt[row] from dlogits (image side has no grad: frozen encoder). */
int clipk_cosine_logits_bwd(int B, int C, int E, int per_image, float scale, const float* imf,
                            const float* txt, const float* inv_tnorm, const float* inv_inorm,
                            const float* dlogits, float* dtxt, void* stream);

/* Row-wise CE / focal (gamma) loss with optional per-class alpha; writes per-row loss and
 * dlogits = d(mean loss)/dlogits * grad_scale. focal with gamma < 0 (or NaN): CLIPK_EINVAL, here and
 * in clipk_ce_loss_reduce / clipk_ce_loss_mix. A row whose label probability rounds to 1 has loss and
 * dlogits exactly 0 for every gamma > 0 (the limit; csrc/common.h focal_terms). */
int clipk_ce_loss(int B, int C, const float* logits, const int64_t* labels, const float* alpha,
                  float gamma, int focal, float grad_scale, float* row_loss, float* dlogits,
                  void* stream);

/* clipk_ce_loss with the batch reduction in the same launch (one block): reduction 1 = mean,
 * 2 = sum of the row losses (summed in row order), into loss[0]; row_loss [B] is still written.
 * Replaces the separate mean / sum launch after clipk_ce_loss (coop.py:158-163 reductions). */
int clipk_ce_loss_reduce(int B, int C, const float* logits, const int64_t* labels, const float* alpha,
                         float gamma, int focal, float grad_scale, int reduction, float* row_loss,
                         float* loss, float* dlogits, void* stream);

/* Mixup (mixup_data / mixup_criterion, independentVL.py:435-460; csrc/mixup.hip).
 *
 * clipk_mixup_images: out[b, i] = w0 * x[b, i] + w1 * x[p, i], p = perm[b], for fp32 x / out
 * [B, n_per] (contiguous) and a device array perm [B]. With labels and y_b (int64 [B], both or
 * neither) the same launch writes y_b[b] = labels[p]. A perm entry outside [0, B) is never
 * dereferenced: that row takes p = b. The two products are rounded to fp32 separately and then
 * added (no FMA contraction): with w0 = (float)lam and w1 = (float)(1.0 - lam) formed in double on
 * the host the result is torch's lam * x + (1 - lam) * x[perm] bit for bit. 16-byte accesses when
 * n_per % 4 == 0 and x / out are 16-byte aligned, one float at a time otherwise. B == 0: CLIPK_OK,
 * nothing launched. CLIPK_ESHAPE: B < 0 or n_per <= 0. CLIPK_EINVAL: x, perm or out null, only
 * one of labels / y_b given, or out overlapping x (rows are read while others are written). */
int clipk_mixup_images(int B, long n_per, const float* x, const int* perm, const int64_t* labels,
                       int64_t* y_b, float w0, float w1, float* out, void* stream);

/* clipk_ce_loss_reduce for a mixed batch: one launch, one max and one sum-of-exponentials pass per
 * row shared by the two targets y_a, y_b (int64 [B]). With L the CE / focal row loss of
 * clipk_ce_loss (the same arithmetic) and red = the mean (the sum in row order times 1 / B,
 * reduction 1) or the sum (reduction 2):
 *   row_loss [2B] = L(logits, y_a) then L(logits, y_b),
 *   loss[0] = lam * red(row_loss[:B]) + (1 - lam) * red(row_loss[B:]),
 *   dlogits[b, c] = grad_scale * (lam * w_a (p_c - [c == y_a]) + (1 - lam) * w_b (p_c - [c == y_b]))
 * with p = softmax(logits[b]) and w_a, w_b = 1 (CE) or the focal weight of the row's target; a row
 * with y_a == y_b gets both terms on one column. dlogits NULL: forward only. A label outside
 * [0, C) is not dereferenced: that row's loss (and gradient) is NaN. No atomics, fixed summation
 * order: bitwise reproducible. Error codes as clipk_ce_loss_reduce (CLIPK_EINVAL: logits, y_a,
 * y_b, row_loss or loss null, reduction not 1 / 2; CLIPK_ESHAPE: B <= 0 or C <= 0). */
int clipk_ce_loss_mix(int B, int C, const float* logits, const int64_t* y_a, const int64_t* y_b,
                      float lam, const float* alpha, float gamma, int focal, float grad_scale,
                      int reduction, float* row_loss, float* loss, float* dlogits, void* stream);

/* NT-Xent (SimCLR) loss of two views a, b (fp32 [n, D], contiguous), forward and gradient:
 * LogitsNTXentLoss on the two views' logits (coop.py:72-123) and ImageNTXentLoss on their image
 * features (independentVL.py:73-112). With N = 2n, rows x_0..x_{N-1} = the rows of a then of b and
 * p(i) = (i + n) mod N:  z_i = x_i / max(|x_i|, 1e-12),  s_ij = z_i . z_j / temperature,
 *   loss[0] = (1/N) sum_i ( log sum_{j != i} exp(s_ij) - s_{i,p(i)} ),
 * da / db [n, D] = grad_scale * d loss / d a, b; both NULL: forward only, no gradient work is
 * launched. fp32 products and sums throughout, every sum in a fixed order (bitwise reproducible,
 * no atomics); 3 launches either way (csrc/ntxent.hip). n = 1 gives loss 0 and zero gradients.
 * ws: caller workspace of clipk_ntxent_ws_bytes(n, D) bytes (0 for a shape out of range); no
 * allocation or synchronisation inside. Any D >= 1, 1 <= n <= 512 (else CLIPK_ESHAPE);
 * CLIPK_EINVAL: a, b, loss or ws null, only one of da / db given, temperature <= 0. */
size_t clipk_ntxent_ws_bytes(int n, int D);
int clipk_ntxent_loss(int n, int D, const float* a, const float* b, float temperature,
                      float grad_scale, float* loss, float* da, float* db,
                      void* ws, void* stream);

/* PromptSRC head (promptsrc.py:171-213, 296-323; csrc/srchead.hip): the whole objective and its
 * gradients with respect to the raw (un-normalised) prompted features, all fp32 and contiguous.
 * With n(x) = x / max(|x|, 1e-12) (F.normalize), u_b = n(img_b), t_c = n(txt_c), z_b = n(zs_img_b),
 * s = scale u t^T, q = scale z fixed_q^T and ls, lq the row log-softmaxes of s and q:
 *   ce       = mean_b L(s_b, labels_b), L the CE / focal row loss of clipk_ce_loss (alpha, gamma,
 *              focal: the same arithmetic),
 *   kl       = w_logits / (B C) sum_{b,c} exp(lq) (lq - ls),
 *   l1_text  = w_text / (C E) sum |t - fixed_n|,     l1_image = w_image / (B E) sum |u - z|,
 *   loss[0..4] = total (the sum of the four), ce, kl, l1_text, l1_image.
 * fixed_n: the frozen text features, L2-normalised; fixed_q: the copy the zero-shot logits use
 * (fixed_n rounded to fp16 values, promptsrc.py:204). logits [B,C] (optional): s.
 * With G = d total / d s = (CE / focal gradient) + w_logits / (B C) (softmax(s) - softmax(q)),
 *   g_u = scale G t + w_image / (B E) sign(u - z),  g_t = scale G^T u + w_text / (C E) sign(t - fixed_n)
 * (sign(0) = 0) and d x = (g - (g . n) n) / |x| through the normalisation,
 *   d_img [B,E], d_txt [C,E] = grad_scale * d total / d img, txt;
 * both NULL: forward only, no gradient work is launched. fp32 products and sums throughout (no
 * MFMA), each log-sum-exp kept as (row max, log of the sum), every sum in a fixed order (bitwise
 * reproducible, no atomics); 4 launches with gradients, 3 without. C = 1 gives ce == 0 and kl == 0
 * exactly. A label outside [0, C) is never dereferenced: ce (and the total, and that row's
 * gradient) is NaN.
 * ws: caller workspace of clipk_src_head_ws_bytes(B, C, E) bytes (0 for a shape out of range); no
 * allocation or synchronisation inside. Any C >= 1 and E >= 1, 1 <= B <= 128 (else CLIPK_ESHAPE).
 * CLIPK_EINVAL: img, txt, zs_img, fixed_n, fixed_q, labels, loss or ws null, only one of d_img /
 * d_txt given, scale <= 0, focal with gamma < 0. */
size_t clipk_src_head_ws_bytes(int B, int C, int E);
int clipk_src_head(int B, int C, int E, const float* img, const float* txt, const float* zs_img,
                   const float* fixed_n, const float* fixed_q, const int64_t* labels,
                   const float* alpha, float gamma, int focal, float scale, float w_text,
                   float w_image, float w_logits, float grad_scale, float* loss, float* logits,
                   float* d_img, float* d_txt, void* ws, void* stream);

/* Linear-probe head (csrc/probe.hip): nn.Linear on frozen image features, CE / focal, and the
 * gradients of the classifier, all fp32 and contiguous: feat [B,E], w [C,E], bias [C] or NULL,
 * alpha [C] or NULL.
 *   u_b     = normalize ? feat_b / max(|feat_b|, 1e-12) (F.normalize) : feat_b,
 *   s[b,c]  = scale <u_b, w_c> + (bias ? bias[c] : 0);  logits [B,C] (optional) receives s,
 *   loss[0] = (1/B) sum_b L(s_b, labels_b), L the CE / focal row loss of clipk_ce_loss (alpha, gamma,
 *             focal: the same arithmetic).
 * With G = d loss / d s = wgt_b / B (softmax(s_b) - onehot(labels_b)) (wgt_b = 1 for CE, the focal
 * weight of the row otherwise) and d_w given,
 *   d_w [C,E]  = grad_scale * scale * sum_b G[b,c] u[b,e],   d_bias [C] = grad_scale * sum_b G[b,c];
 * nothing goes to feat (the encoder is frozen). d_bias must be given exactly when d_w and bias both
 * are. d_w NULL: forward only, no gradient work is launched. labels NULL: scoring only -- logits
 * (then required) is written and nothing else; loss, d_w and d_bias must be NULL, ws is not used and
 * may be NULL.
 * fp32 products and sums throughout (fp32 VALU FMA chains, no MFMA: DESIGN.md, "Probe head kernel"),
 * the log-sum-exp kept as (row max, log of the sum), every sum in an order fixed by (B, C, E)
 * (bitwise reproducible, no atomics). 3 launches with gradients (logits; row softmax, loss and G;
 * d_w / d_bias and the loss sum), 2 forward only, 1 scoring only. C = 1 gives loss == 0, d_w == 0
 * and d_bias == 0 exactly. A label outside [0, C) is never dereferenced: the loss (and that row's
 * gradient) is NaN. 16-byte loads when E % 4 == 0 and feat / w are 16-byte aligned, one float at a
 * time otherwise.
 * ws: caller workspace of clipk_probe_head_ws_bytes(B, C, E) bytes (0 for a shape out of range),
 * 16-byte aligned; no allocation or synchronisation inside. Any C >= 1 and E >= 1, 1 <= B <= 512
 * (else CLIPK_ESHAPE). CLIPK_EINVAL: feat or w null; with labels: loss or ws null, the d_w / d_bias /
 * bias rule broken, focal with gamma < 0; without labels: logits null or one of loss, d_w, d_bias
 * given; scale <= 0. Checked on the host before any launch. */
size_t clipk_probe_head_ws_bytes(int B, int C, int E);
int clipk_probe_head(int B, int C, int E, const float* feat, const float* w, const float* bias,
                     const int64_t* labels, const float* alpha, float gamma, int focal,
                     int normalize, float scale, float grad_scale,
                     float* loss, float* logits, float* d_w, float* d_bias,
                     void* ws, void* stream);

/* CoCoOp Meta-Net: h = relu(x W1^T + b1); y = h W2^T + b2. x [B,V], W1 [Hd,V], W2 [Wd,Hd].
 * The CLIP widths (V % 256 == 0, V <= 1024, Hd <= 64, x / W1 16-B aligned) take the
 * many-block form; other shapes one block per image. */
int clipk_meta_net_fwd(int B, int V, int Hd, int Wd, const float* x, const float* w1,
                       const float* b1, const float* w2, const float* b2, float* h, float* y,
                       void* stream);
/* clipk_meta_net_fwd on the L2-normalised rows of x: xn [B,V] = x / |x| (written; cocoop.py:238
 * imf / imf.norm(dim=-1)), then the Meta-Net on xn -- the normalisation's two launches folded in. */
int clipk_meta_net_fwd_norm(int B, int V, int Hd, int Wd, const float* x, const float* w1,
                            const float* b1, const float* w2, const float* b2, float* xn, float* h,
                            float* y, void* stream);
/* grads of W1,b1,W2,b2 from dy (x has no grad). dh_ws: caller scratch of B*Hd floats. */
int clipk_meta_net_bwd(int B, int V, int Hd, int Wd, const float* x, const float* h,
                       const float* w2, const float* dy, float* dw1, float* db1, float* dw2,
                       float* db2, float* dh_ws, void* stream);

/* p -= lr * (buf = momentum*buf + (g + wd*p)); first step (has_buf==0): buf = g + wd*p. */
int clipk_sgd_step(long n, float* p, const float* g, float* buf, float lr, float momentum,
                   float weight_decay, int has_buf, void* stream);
/* clipk_sgd_step over up to 16 tensors of one param group in one launch (p[k], g[k], buf[k] of
 * n[k] floats, has_buf[k] per tensor; host arrays): the same per-element update. */
int clipk_sgd_step_multi(int count, float* const* p, const float* const* g, float* const* buf,
                         const long* n, const int* has_buf, float lr, float momentum,
                         float weight_decay, void* stream);

/* clipk_sgd_step_multi on grad_scale * g (e.g. 1 / world after a SUM all-reduce: the average
 * folded into the update instead of a division launch; 1.0 is bitwise clipk_sgd_step_multi). */
int clipk_sgd_step_multi_scaled(int count, float* const* p, const float* const* g, float* const* buf,
                                const long* n, const int* has_buf, float lr, float momentum,
                                float weight_decay, float grad_scale, void* stream);
/* clipk_sgd_step_multi_scaled skipped entirely (p, buf untouched) when guard[0] & mask != 0, read on
 * the device: the PREC fp32s trainer queues the step without waiting for its backward's overflow
 * flag (clipk_encoder_set_status bit 2) and re-runs an overflowed step later. */
int clipk_sgd_step_multi_if(int count, float* const* p, const float* const* g, float* const* buf,
                            const long* n, const int* has_buf, float lr, float momentum,
                            float weight_decay, float grad_scale, const int* guard, int mask, void* stream);

/* clipk_adam_step_multi modes */
enum { CLIPK_ADAM_ADAM = 0, CLIPK_ADAM_ADAMW = 1, CLIPK_ADAM_AMSGRAD = 2 };
/* torch.optim.Adam / AdamW step (non-capturable single-tensor semantics) over up to 16 tensors of
 * one param group in one launch: p[k], g[k], m[k] (exp_avg), v[k] (exp_avg_sq) and, for
 * CLIPK_ADAM_AMSGRAD, vmax[k] (max_exp_avg_sq; vmax may be NULL otherwise) of n[k] floats; host
 * arrays of device pointers. With g' = grad_scale * g (rounded on its own; 1.0 is bitwise the
 * unscaled update):
 *   ADAM / AMSGRAD  g' += wd * p                      ADAMW  p *= 1 - lr * wd
 *   m = beta1 m + (1 - beta1) g'      v = beta2 v + (1 - beta2) g'^2      [vmax = max(vmax, v)]
 *   p -= lr / (1 - beta1^t) * m / (sqrt(v or vmax) / sqrt(1 - beta2^t) + eps)
 * 1 - beta^t is formed in double on the device and the step size rounded to fp32.
 * The step count is device state, per tensor: step[k] points at two int32 (both 0 for fresh
 * state). The launch reads t - 1 = step[k][parity[k]] and writes t to step[k][parity[k] ^ 1]; the
 * caller flips parity[k] (0 / 1) after every call that names the tensor, so the count of the
 * last call is step[k][next parity].
 * guard (may be NULL): when guard[0] & mask != 0, read on the device, the whole update is skipped
 * -- p, m, v, vmax untouched and the count carried over unchanged (the parity still flips).
 * CLIPK_EINVAL: count outside 1..16, a null pointer, a parity other than 0 / 1, mode out of
 * range, beta outside [0, 1), eps, lr or weight_decay < 0; CLIPK_ESHAPE: n[k] < 0. */
int clipk_adam_step_multi(int count, float* const* p, const float* const* g, float* const* m,
                          float* const* v, float* const* vmax, const long* n, int* const* step,
                          const int* parity, double lr, double beta1, double beta2, double eps,
                          double weight_decay, int mode, float grad_scale, const int* guard, int mask,
                          void* stream);
/* Status word hand-off (PREC fp32s overflow flags, clipk_encoder_set_status): host_word[0] =
 * flags[0], then flags[0] = 0, in one stream-ordered launch; host_word is host-visible memory
 * (pinned). The caller synchronises the stream (or an event after it) before reading it. */
int clipk_status_take(int* flags, int* host_word, void* stream);

/* Row gather / scatter: dst row (dst_rows ? dst_rows[i] : i) = src row (src_rows ? src_rows[i] : i)
 * for i < n; rows of row_bytes (multiple of 16) bytes, 16-B aligned. The text encoder's last
 * layer runs on the EOT rows only (the output is read there alone; exact) and moves rows
 * between the compact and the full layouts with it. */
int clipk_rows_copy(int row_bytes, int n, const void* src, const int* src_rows, void* dst,
                    const int* dst_rows, void* stream);

/* Elementwise cast fp32 -> dtype. */
int clipk_cast(int out_dtype, long n, const float* x, void* y, void* stream);

/* ---------------------------------------------------------------- encoders */
typedef struct clipk_encoder clipk_encoder;

/* Per-layer weight table order (n_per_layer = 16):
 *   0 ln1_w f32, 1 ln1_b f32, 2 in_w [3W,W] act, 3 in_b f32[3W], 4 out_w [W,W] act, 5 out_b,
 *   6 ln2_w, 7 ln2_b, 8 fc_w [4W,W] act, 9 fc_b f32[4W], 10 proj_w [W,4W] act, 11 proj_b,
 *   12 in_wT [W,3W] grad, 13 out_wT [W,W] grad, 14 fc_wT [W,4W] grad, 15 proj_wT [4W,W] grad
 * (12..15 may be NULL for a forward-only encoder). Head: lnf_w, lnf_b (f32), projT [E,W] act,
 * proj_grad [W,E] grad (NULL if forward-only).
 * act_dtype: forward GEMM operand type; grad_dtype: backward GEMM operand type. */
int clipk_encoder_create(int width, int layers, int heads, int embed, int act_dtype,
                         int grad_dtype, const void* const* layer_ptrs, const void* const* head_ptrs,
                         clipk_encoder** out);
void clipk_encoder_destroy(clipk_encoder* enc);

/* Deep prompts of an encoder (IVLP / MaPLe / PromptSRC, model.py:191-331): before layer l in
 * 1..n_deep the rows `rows` ([n_ctx][n_per], see clipk_rows_inject) of the residual stream
 * are replaced by prompts[l-1] ([n_deep][n_ctx][width] fp32, values as given: the trainers
 * round them through fp16 as the reference's .half() does); the backward writes the prompts'
 * gradients into grads[l-1] (when grads != NULL) and stops them there. Text: rows 1..n_ctx of
 * every sequence (packed layout: of every group); ViT: the last n_vpt rows of every image.
 * The pointers must stay valid for the calls that follow; n_deep = 0 clears. */
int clipk_encoder_set_deep_prompts(clipk_encoder* e, int n_deep, int n_ctx, int n_per, const int* rows,
                                   const float* prompts, float* grads);

/* Input-row mode of the next text-encoder calls on the shared-prefix packed layout
 * (clipk_text_{forward,backward}_packed). mode 0: every row of x0 is an independent input (the
 * reference's TextEncoder contract, coop.py:195-205). mode 1: only the P prefix rows of each
 * group carry per-group values -- the context slots of CoOp / CoCoOp with class position "end"
 * (coop.py:259-270; cocoop.py:173-198, pi_b added to ctx only) -- so the class rows of x0 are
 * identical in every group: layer 0's LN1 and qkv projection run once for them (group 0) and
 * are copied to the other groups, and the backward forms dx0 on the prefix rows only (the
 * rows clipk_ctx_grad_rows reads; the class rows of dx0 are left unspecified). Exact. Forward
 * and backward of one call must use the same mode. */
int clipk_encoder_set_input_rows(clipk_encoder* e, int mode);

/* LayerNorm fold of a 16-bit text encoder (see clipk_gemm_ln): fold_ptrs = 6 per layer,
 * {W_in' [3W, W] act dtype, s_in [3W] fp32, c_in [3W] fp32, W_fc' [4W, W], s_fc [4W], c_fc [4W]}
 * built from the layer's ln_1 / ln_2 and in_proj / c_fc weights. When set, layers >= 1 take
 * ln_1 from the previous layer's c_proj epilogue statistics and every layer takes ln_2 from its
 * out_proj epilogue (layer 0's ln_1 and ln_final stay LayerNorm passes; not used with deep
 * prompts or an fp32 encoder; a PREC fp32s encoder (clipk_encoder_set_split first) takes W_in' /
 * W_fc' split-packed). The saved mean / rstd are the same quantities the LayerNorm pass
 * writes, so the backward is unchanged. fold_ptrs == NULL clears. Pointers must stay valid. A ViT
 * handle (clipk_vision_create) takes the same table for its ln_1 / ln_2: its forward with a
 * 16-bit act dtype (clipk_vit_forward) runs the residual stream in that dtype through the text
 * encoder's layer loop and folds them the same way. */
int clipk_encoder_set_ln_fold(clipk_encoder* e, const void* const* fold_ptrs);

/* PREC fp32s on an fp32 encoder (act and grad dtype CLIPK_F32): on = 1 declares every GEMM weight
 * of the handle's tables (layer weights 2, 4, 8, 10 and their transposes 12-15; text head 2-3,
 * ViT head 4-5 and the prompted backward's proj) packed by clipk_split_pack, and runs every GEMM
 * of its calls as CLIPK_F32S (the fp32-class split-fp16 MFMA product). LayerNorm, attention and
 * the residual stream stay fp32. The text backward then runs on s * dtxt with s a power of two
 * from max |dtxt| (exact, undone on dx0 and the deep-prompt gradients), so the gradient operands
 * sit in fp16's normal range. Reference semantics: PromptSRC/clip/model.py:699 (fp32 model).
 * on = 2: those weights are fp16-valued (clipk_split_lo_zero returned 1 for each; the released
 * CLIP checkpoints) and the tables hold their COMPACT form (clipk_split_hi16) instead of the packed
 * one: every GEMM runs CLIPK_F32S16, 2 MFMAs per product, the same results as mode 1.
 * With a LayerNorm fold (clipk_encoder_set_ln_fold after this call) the fold tables then hold W
 * itself (compact) instead of W' = W diag(gamma), s = rowsums of W diag(gamma) over the packed
 * values / 64, and the fold GEMMs apply the layer's LayerNorm weight to A (clipk_gemm_ln_gamma).
 * The mode describes the tables' format, so it is fixed once set: a second call with another mode,
 * or any call after clipk_encoder_set_ln_fold, returns CLIPK_EINVAL. */
int clipk_encoder_set_split(clipk_encoder* e, int on);
/* The split backward's scale target t (default 7): s puts max |s dtxt| in [2^(t-1), 2^t). A lower
 * target leaves more headroom below fp16's 65504 for gradient growth through the layers, at
 * fewer significant bits for the smallest gradients. -24 <= t <= 30 (t > 16 overflows by design:
 * a test of the overflow status). */
int clipk_encoder_set_split_target(clipk_encoder* e, int target);
/* Overflow status of a PREC fp32s (split) encoder's calls: status = a device int the encoder
 * ORs flags into -- 1 when a text / ViT forward produced a non-finite feature, 2 when a backward's
 * returned gradients (dx0, deep-prompt and visual-prompt gradients) hold a non-finite value (the
 * split operands' fp16 range was exceeded: an activation or gradient past 65504). The caller zeroes
 * it and reads it when it synchronises (fsp_amd/clip/model.py re-runs an overflowed backward at a
 * lower scale target). NULL detaches. The pointer must stay valid for the calls that follow. */
int clipk_encoder_set_status(clipk_encoder* e, int* status);

/* LoRA on attn.in_proj_weight (this package's LoRA trainer; CLIP-LoRA's q / k / v adapters):
 *   W'_p = W0_p + scale * B_p A_p  for the projections p (bit 0 q, 1 k, 2 v) of proj_mask, in the
 *   layers of layer_mask (bit l); A_p [rank, W], B_p [W, rank] fp32, 1 <= rank <= 16, W % 64 == 0.
 * LoRA is linear, so an encoder whose tables hold W' (entries 2 and 12) runs LoRA's forward and its
 * input-grad backward unchanged; what is new is the merge and the adapters' own gradient.
 *
 * clipk_lora_merge: one launch for all `layers` (<= 32) of an encoder. w0[l] fp32 [3W, W] (host
 * array of device pointers, as out / outT); A [layers][3][rank][W], B [layers][3][W][rank].
 * out[l] = W' [3W, W] in act_dtype, outT[l] = W'^T [W, 3W] in grad_dtype (outT NULL: none), both
 * rounded once from the same fp32 value  fma(scale, acc, W0[n, k]),  acc = 0, then
 * acc = fma(B[n, j], A[j, k], acc) for j ascending. Projections and layers outside the masks: W0.
 * Output dtypes CLIPK_F32 / F16 / BF16 (PREC fp32s: merge to fp32, then clipk_split_pack).
 *
 * clipk_lora_wgrad: one layer's dA [3][rank][W], dB [3][W][rank] (fp32, overwritten; zeros for the
 * projections outside proj_mask) from the layer input X [rows, W] (x_dtype), its LayerNorm
 * statistics mean / rstd [rows], the LayerNorm's gamma / beta and dqkv [rows, 3W] (g_dtype):
 *   xn = (X - mean) rstd gamma + beta    P_p = xn A_p^T    dU_p = scale dY_p B_p
 *   dB_p = scale dY_p^T P_p              dA_p = dU_p^T xn            (dY_p: dqkv's p slice)
 * fp32 accumulation in an order fixed by the shapes (bitwise reproducible), three launches.
 * CLIPK_EINVAL: rank outside 1..16, W % 64 != 0, a null or misaligned (16 B) pointer.
 *
 * clipk_encoder_set_lora: declares the handle's in_proj tables merged as above; its backwards
 * (clipk_text_backward, clipk_vit_backward_prompted with n_vpt = 0) then also write
 * dA [layers][3][rank][W] and dB [layers][3][W][rank] (zeros for layers outside layer_mask; with
 * PREC fp32s unscaled with dx0 and covered by status flag 2). dA = dB = NULL: no gradients.
 * Query the backward workspace size after this call. The pointers must stay valid; rank = 0
 * clears. CLIPK_EINVAL with a LayerNorm fold or deep prompts set (and from those setters while
 * LoRA is set), and from the packed text entry points and prompted ViT calls with n_vpt > 0. */
int clipk_lora_merge(int W, int layers, int rank, int proj_mask, unsigned layer_mask, float scale,
                     int act_dtype, int grad_dtype, const float* const* w0, const float* A, const float* B,
                     void* const* out, void* const* outT, void* stream);
size_t clipk_lora_wgrad_ws_bytes(int rows, int W, int rank);
int clipk_lora_wgrad(int x_dtype, int g_dtype, int rows, int W, int rank, int proj_mask, float scale,
                     const void* X, const float* mean, const float* rstd, const float* gamma,
                     const float* beta, const void* dqkv, const float* A, const float* B, float* dA,
                     float* dB, void* ws, size_t ws_bytes, void* stream);
int clipk_encoder_set_lora(clipk_encoder* e, int rank, int proj_mask, unsigned layer_mask, float scale,
                           const float* A, const float* B, float* dA, float* dB);

/* ViT with visual prompts, forward with saved activations and input-grad backward (the
 * prompted VisionTransformer of IVLP / PromptSRC, model.py:401-431, and MaPLe, 434-485):
 * n_vpt prompt rows (vpt [n_vpt, width] fp32) appended after the image tokens before ln_pre,
 * deep prompts per clipk_encoder_set_deep_prompts, feat [B, E] fp32 from ln_post(CLS) @ proj.
 * saved == NULL: inference. The backward needs the encoder created with its transposed
 * layer weights (layer_ptrs 12..15) and proj_bwd = proj [width, E] in the grad dtype; it
 * writes d vpt [n_vpt, width] fp32 (summed over the images) and the deep prompts' gradients.
 * One workspace (clipk_vit_prompted_ws_bytes) serves both calls. */
size_t clipk_vit_prompted_saved_bytes(const clipk_encoder* e, int B, int n_vpt);
size_t clipk_vit_prompted_ws_bytes(const clipk_encoder* e, int B, int n_vpt);
int clipk_vit_forward_prompted(const clipk_encoder* e, int B, const float* img, int n_vpt, const float* vpt,
                               float* feat, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes,
                               void* stream);
int clipk_vit_backward_prompted(const clipk_encoder* e, int B, int n_vpt, const float* vpt, const void* proj_bwd,
                                const float* dfeat, const void* saved, size_t saved_bytes, float* dvpt, void* ws,
                                size_t ws_bytes, void* stream);

/* Text encoder forward over nseq sequences of length L (x0 fp32 [nseq*L, W], positional
 * embedding already added). eot_rows[s] = s*L + EOT position of sequence s (int32, device).
 * txt fp32 [nseq, E].
 * If save != 0 the activations needed by clipk_text_backward stay in `saved`. */
size_t clipk_text_saved_bytes(const clipk_encoder* enc, int nseq, int L);
size_t clipk_text_ws_bytes(const clipk_encoder* enc, int nseq, int L);
int clipk_text_forward(const clipk_encoder* enc, int nseq, int L, const float* x0, const int* eot_rows,
                       float* txt, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes,
                       void* stream);
size_t clipk_text_bwd_ws_bytes(const clipk_encoder* enc, int nseq, int L);
int clipk_text_backward(const clipk_encoder* enc, int nseq, int L, const int* eot_rows,
                        const float* dtxt, const void* saved, size_t saved_bytes, float* dx0,
                        void* ws, size_t ws_bytes, void* stream);

/* Shared-prefix packed variant (see clipk_attention_prefix_fwd): G groups of R rows,
 * C sequences per group, x0 fp32 [G*R, W]; eot_rows[g*C + c] = absolute EOT row;
 * txt fp32 [G*C, E]. Exact: rows after a sequence's EOT and duplicated causal prefixes
 * never influence the EOT features. */
size_t clipk_text_packed_saved_bytes(const clipk_encoder* enc, int G, int C, int R);
size_t clipk_text_packed_ws_bytes(const clipk_encoder* enc, int G, int C, int R);
size_t clipk_text_packed_bwd_ws_bytes(const clipk_encoder* enc, int G, int C, int R, int ntiles);
int clipk_text_forward_packed(const clipk_encoder* enc, int G, int C, int P, int R, int ntiles,
                              const int* tiles, const int* row_first, const float* x0,
                              const int* eot_rows, float* txt, void* saved, size_t saved_bytes,
                              void* ws, size_t ws_bytes, void* stream);
int clipk_text_backward_packed(const clipk_encoder* enc, int G, int C, int P, int R, int ntiles,
                               const int* tiles, const int* row_first, const int* eot_rows,
                               const float* dtxt, const void* saved, size_t saved_bytes, float* dx0,
                               void* ws, size_t ws_bytes, void* stream);

/* Vision transformer forward (frozen, no grad): img fp32 [B,3,R,R] -> feat fp32 [B,E]. With a
 * 16-bit act dtype the residual stream is kept in that dtype (CLIP's half semantics, as the text
 * encoder's; env CLIPK_VIT_RES16=0: fp32), ln_1 / ln_2 are folded when set
 * (clipk_encoder_set_ln_fold) and the last layer's post-attention half runs on the CLS rows.
 * Head table for a vision encoder: ln_pre_w, ln_pre_b, ln_post_w, ln_post_b (f32),
 * projT [E,D] act, conv_w [D,Kp] act, class_emb f32[D], pos f32[L,D]. */
int clipk_vision_create(int width, int layers, int heads, int embed, int res, int patch,
                        int act_dtype, const void* const* layer_ptrs,
                        const void* const* head_ptrs, clipk_encoder** out);
size_t clipk_vit_ws_bytes(const clipk_encoder* enc, int B);
int clipk_vit_forward(const clipk_encoder* enc, int B, const float* img, float* feat, void* ws,
                      size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- ModifiedResNet (RN50 / RN101)
 * CLIP's ResNet image tower (PromptSRC/clip/model.py:10-150), frozen and forward-only. Activations
 * are NHWC in the act dtype (CLIPK_F32 / CLIPK_F16 / CLIPK_BF16), every pointer 16-B aligned.
 * Every violation below returns CLIPK_EINVAL before any launch. No atomics, no split-K: two
 * calls agree bitwise. */
enum { CLIPK_CONV_RES = 1, CLIPK_CONV_RELU = 2, CLIPK_CONV_OUT_F32 = 4 };
/* Implicit-GEMM convolution on the MFMA (16-bit: mfma_f32_16x16x32, fp32: mfma_f32_16x16x4f32;
 * fp32 accumulation), stride 1, pad ksize / 2, ksize 1 or 3, Cin % 32 == 0, Cout % 32 == 0, any
 * M = B H W. x [B,H,W,Cin], w [Cout, ksize^2 Cin] (k = tap * Cin + c, tap = ky * ksize + kx), both
 * dtype; out [B,H,W,Cout] = max(acc * scale[n] + shift[n] + res, 0) in fp32, rounded once (scale /
 * shift fp32 [Cout], the frozen BatchNorm's; null: 1 / 0). CLIPK_CONV_RES adds res (dtype, the
 * shape of out), CLIPK_CONV_RELU clamps, CLIPK_CONV_OUT_F32 stores out as fp32. A tap outside the
 * image contributes zero and is never read: its index is clamped into the image and zero is
 * selected. */
int clipk_conv2d_nhwc(int dtype, int flags, int B, int H, int W, int Cin, int Cout, int ksize,
                      const void* x, const void* w, const float* scale, const float* shift,
                      const void* res, void* out, void* stream);
/* The stem's conv1 (3 -> Cout, 3x3, stride 2, pad 1) as a gather for the 1x1 path: img fp32
 * [B,3,R,R] -> out [B (R/2)^2, 32] (out_dtype), k = (ky * 3 + kx) * 3 + c, zero for k >= 27. R even. */
int clipk_im2col_3x3s2(int out_dtype, int B, int res, const float* img, void* out, void* stream);
/* AvgPool2d(2) on NHWC: the four values summed in fp32, times 0.25, rounded once. H, W even,
 * C % 8 == 0. */
int clipk_avgpool2_nhwc(int dtype, int B, int H, int W, int C, const void* x, void* out, void* stream);
/* AttentionPool2d: x [B, HW, C] (dtype) -> feat fp32 [B, E]. The mean token (fp32 sum) is
 * prepended, pos fp32 [HW + 1, C] added, and one multi-head attention runs with the mean token as
 * the only query: q = q_w tok0 + q_b scaled by 64^-0.5, k | v = kv_w tok + kv_b for every token
 * (kv_w [2C, C]: k_proj over v_proj), fp32 softmax, feat = c_w o + c_b. Weights [out, in] in dtype,
 * biases fp32. C == 64 heads, HW + 1 <= 256, E % 32 == 0; ws 16-B aligned, at least
 * clipk_attnpool_ws_bytes (else CLIPK_EWORKSPACE). */
size_t clipk_attnpool_ws_bytes(int dtype, int B, int HW, int C);
int clipk_attnpool(int dtype, int B, int HW, int C, int heads, int E, const void* x, const float* pos,
                   const void* q_w, const float* q_b, const void* kv_w, const float* kv_b,
                   const void* c_w, const float* c_b, float* feat, void* ws, size_t ws_bytes,
                   void* stream);
/* The whole tower: img fp32 [B,3,R,R] -> feat fp32 [B, embed]. width = layer1's planes (64),
 * blocks = the four block counts, res % 32 == 0. Weights are not owned. ptrs, in order:
 *   stem: conv1 w [width/2, 32] (clipk_im2col_3x3s2's k order), scale, shift; conv2 w, scale,
 *         shift; conv3 w, scale, shift;
 *   per block: conv1 w, scale, shift, conv2 w, scale, shift, conv3 w, scale, shift, downsample w,
 *         scale, shift (three nulls where the block has none);
 *   attnpool: pos, q_w, q_b, kv_w, kv_b, c_w, c_b
 * -- n_ptrs = 9 + 12 * (number of blocks) + 7. Convolution weights in act_dtype, repacked to
 * clipk_conv2d_nhwc's [Cout, ksize^2 Cin]; scale = bn.weight / sqrt(running_var + 1e-5), shift =
 * bn.bias - running_mean * scale, fp32. */
typedef struct clipk_resnet clipk_resnet;
int clipk_resnet_create(int width, const int* blocks, int embed, int res, int act_dtype,
                        const void* const* ptrs, int n_ptrs, clipk_resnet** out);
void clipk_resnet_destroy(clipk_resnet* h);
size_t clipk_resnet_ws_bytes(const clipk_resnet* h, int B);
int clipk_resnet_forward(const clipk_resnet* h, int B, const float* img, float* feat, void* ws,
                         size_t ws_bytes, void* stream);

/* Per-kernel-class timing with hipEvents on the launch stream (bench.py roofline). */
enum { CLIPK_PROF_NONE = 0, CLIPK_PROF_GEMM_FC = 1, CLIPK_PROF_GEMM_ALL = 2, CLIPK_PROF_ATTN = 3,
       CLIPK_PROF_LN = 4, CLIPK_PROF_GEMM_DGELU = 5 };
/* GEMM_FC = text c_fc forward GEMMs; GEMM_DGELU = text c_proj input-grad GEMMs with the fused
 * QuickGELU' epilogue; GEMM_ALL = every text GEMM; ATTN = text attention fwd+bwd. */
int clipk_prof_enable(int kind);
int clipk_prof_read(double* total_ms, long* count, double* flops_or_bytes);

/* Per-launch-site timing (bench.py's per-kernel roofline table): when on, every named launch
 * site of the encoders ("text.qkv_fwd", "text.attn_bwd", "text.ln_fwd", "vit.fc_fwd", ...) is
 * bracketed by hipEvents on its launch stream, with its algorithmic FLOPs and HBM bytes.
 * clipk_prof_sites_read fills up to max_sites rows (names: CLIPK_PROF_NAME_LEN chars each,
 * NUL-terminated) summed since the last read / enable, sets *n_sites, and resets. */
enum { CLIPK_PROF_NAME_LEN = 32 };
int clipk_prof_sites_enable(int on);
int clipk_prof_sites_read(int max_sites, char* names, double* total_ms, long* count, double* flops,
                          double* bytes, int* n_sites);

#ifdef __cplusplus
}
#endif
#endif /* CLIPK_H */
