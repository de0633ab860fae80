/*
 * lemon_hip.h -- C ABI of liblemon_hip.so, the MI355X (gfx950) implementation of
 * LEMoN's kNN + multimodal-neighbour scoring hot path.
 *
 * The reference (MLforHealth/LEMoN, 100% Python) has no FFI layer; the seam this
 * library replaces is the object protocol run_lemon.py uses.  Each entry point
 * cites the reference call site it stands in for (paths relative to the
 * reference root).  INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *   - every pointer named *_dev is a DEVICE pointer (hipMalloc / torch data_ptr());
 *     all matrices are row-major, float32 unless stated, int64 labels like faiss;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every
 *     call only enqueues work on that stream (no host synchronisation) unless its
 *     comment says otherwise;
 *   - return value: 0 = ok, <0 = error (LEMON_E_*); lemon_last_error() returns a
 *     thread-local description of the last failure;
 *   - row alignment: the query and embedding rows handed to lemon_index_search, lemon_neighbors and lemon_discrepancy
 *     must start on a 16-byte boundary when d % 4 == 0 (kernels behind the search read such rows 16 bytes at a time);
 *     a pointer that does not is refused with LEMON_E_INVALID before anything is launched.  With d % 4 != 0 any float
 *     pointer is accepted.  The row-wise helpers (lemon_normalize_rows, lemon_paired_distance, lemon_paired_metric)
 *     take any float pointer at every d;
 *   - caller owns every output buffer; the library owns only what is inside a
 *     lemon_index handle; one handle per thread.  The ONLY process-wide state is
 *     lemon_linear_f32's hipBLASLt handle + workspace + solution cache (one set per
 *     device, mutex-guarded; see its comment) and the thread-local error string.
 *   - numeric contract ("chain" numerics): dot(a,b) is the float32 fmaf chain in
 *     ascending k starting from +0 (bit-for-bit what v_mfma_f32_32x32x2_f32
 *     accumulates); ties in every top-k are broken towards the lower index.
 */
#ifndef LEMON_HIP_H
#define LEMON_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LEMON_METRIC_IP 0 /* faiss.IndexFlatIP, --dist_type cosine    (run_lemon.py:166-169) */
#define LEMON_METRIC_L2 1 /* faiss.IndexFlatL2, --dist_type euclidean (run_lemon.py:170-173) */

#define LEMON_OK 0
#define LEMON_E_INVALID (-1) /* bad argument (null pointer, d mismatch, k out of range) */
#define LEMON_E_HIP (-2)     /* a HIP runtime call failed; see lemon_last_error()        */
#define LEMON_E_NOMEM (-3)   /* device allocation failed                                 */

#define LEMON_MAX_K 64 /* k + (sname == 'train') <= 64 in lemon_neighbors / one scan pass; the reference grid tops out at 50+1 (experiments.py:86) */
#define LEMON_MAX_K_DEEP 2048 /* lemon_index_search accepts deeper lists (faiss has no limit): passes of LEMON_MAX_K */

/* search algorithm selector for lemon_index_set_algo() */
#define LEMON_ALGO_AUTO 0
#define LEMON_ALGO_F32_MFMA 1   /* exact fp32 MFMA scan (v_mfma_f32_32x32x2_f32)                       */
#define LEMON_ALGO_BF16_FILTER 2 /* 16-bit MFMA filter with a rigorous error band + exact fp32 re-rank; */
                                 /* returns bit-identical results to LEMON_ALGO_F32_MFMA.  The filter   */
                                 /* operands are fp16 copies since round 3 (bf16 before: name kept)     */
#define LEMON_ALGO_F16_FILTER LEMON_ALGO_BF16_FILTER

typedef struct lemon_index lemon_index_t;

const char *lemon_last_error(void);
/* library / device facts, for logs: returns 0 and fills what it can */
int lemon_version(int *major, int *minor);

/* ---- row-wise helpers ------------------------------------------------------------ */

/* lib/utils/utils.py:39-40 normalize_vectors == F.normalize(p=2, dim=1, eps=1e-12);
 * call sites run_lemon.py:163-164,230-233.  y_dev may alias x_dev. */
int lemon_normalize_rows(const float *x_dev, int64_t n, int d, float *y_dev, void *stream);

/* run_lemon.py:169 (IP: 1 - <a_i,b_i>), :173 (L2: sum_k (a_ik-b_ik)^2) -> dists_tr;
 * run_lemon.py:250-253 -> d_1.  out_dev [n]. */
int lemon_paired_distance(int metric, const float *a_dev, const float *b_dev, int64_t n, int d,
                          float *out_dev, void *stream);

/* DistanceEvaluator.our_metric, lib/metrics/distance_metrics.py:48-73 (used by
 * lib/baselines/run_clip_sim.py:235-248): paired distance of row i of a and row i of b WITHOUT
 * assuming normalised inputs.  kind 0: cosine 1 - <a,b>/(|a||b|); 1: euclidean (NOT squared);
 * 2: manhattan.  The reference takes the diagonal of the full n x n pairwise matrix.  Sums run in float64 and the result is
 * rounded once to float32 (sklearn's euclidean and manhattan distances are float64 values); a row of norm zero has cosine
 * similarity 0 to everything, hence distance exactly 1, as sklearn.metrics.pairwise.cosine_similarity gives. */
int lemon_paired_metric(int kind, const float *a_dev, const float *b_dev, int64_t n, int d,
                        float *out_dev, void *stream);

/* --normalize_d1, run_lemon.py:244-248: d1[i] = softmax_c(dist(img_i, cls_txt_c))[noisy_label[i]].
 * cls_txt_dev [C,d] (run_lemon.py:180-190), noisy_label_dev [n] int32.  0 < C <= 1024, anything else is refused with
 * LEMON_E_INVALID and d1_dev is not written.  The labels live on the device and are NOT checked: a label outside [0, C)
 * matches no class and gives d1 = 0 (the reference raises IndexError for a label >= C and wraps a negative one round).  A
 * caller that cannot vouch for its labels checks them on the host first, as lemon_amd.ops.d1_normalized does. */
int lemon_d1_normalized(int metric, const float *q_img_dev, int64_t n, int d,
                        const float *cls_txt_dev, int C, const int32_t *noisy_label_dev,
                        float *d1_dev, void *stream);

/* Zero-shot "CLIP logits" baseline, lib/baselines/train_zero_shot_clip_baseline.py:207-224: per image,
 * conf[i] = softmax_c(1 - dist(cls_txt_c, img_i))[noisy_label[i]] with dist = DistanceEvaluator.our_metric
 * (lib/metrics/distance_metrics.py:48-73) on UN-normalised embeddings: kind 0 = 1 - cosine similarity,
 * 1 = euclidean (not squared), 2 = manhattan.  img_dev [n,d], cls_txt_dev [C,d], 0 < C <= 1024 (anything else: LEMON_E_INVALID,
 * conf_dev not written).  Distances, softmax and quotient are computed in float64 and rounded once to float32.  A zero image
 * or class row has cosine distance 1 (similarity 0, as sklearn gives), never NaN.  Labels are not checked, as in
 * lemon_d1_normalized: one outside [0, C) gives conf = 0; lemon_amd.baselines.clip_logits_confidence checks on the host. */
int lemon_class_confidence(int kind, const float *img_dev, int64_t n, int d, const float *cls_txt_dev, int C,
                           const int32_t *noisy_label_dev, float *conf_dev, void *stream);

/* generic_transform (lib/datasets/utils.py:159-170: Resize(224, BICUBIC) -> CenterCrop(224) -> ToTensor ->
 * Normalize) for a batch of equally sized uint8 HWC images, bit-identical to PIL + torch: the two integer
 * resampling passes of PIL (22-bit fixed-point taps, horizontal then vertical, clip8) and (v/255-mean)/std.
 * img_dev [batch, in_h, in_w, 3] uint8; kk_*_dev [out_size, ks_*] int32 taps and bnd_*_dev [out_size, 2]
 * (first input index, tap count) for the out_size CROPPED output columns / rows (built on the host:
 * lemon_amd/data.py::pil_bicubic_tables); rows_per_block output rows per workgroup, max_rows_per_block
 * = the largest number of input rows one block's vertical windows span (x out_size x 3 bytes <= 64 KB);
 * mean3_host/std3_host: 3 floats each (host memory); out_dev [batch, 3, out_size, out_size] float32 when
 * patch == 0, else patch-major [batch, (out_size/patch)^2, 3*patch*patch] -- the rows the ViT patch
 * embedding (a stride == kernel convolution, HF CLIPVisionEmbeddings / chexzero_clip.py:226-238) multiplies,
 * so that it becomes one lemon_linear_f32 GEMM with no im2col pass. */
int lemon_preprocess_u8(const uint8_t *img_dev, int64_t batch, int in_h, int in_w, const int32_t *kk_h_dev,
                        const int32_t *bnd_h_dev, int ks_h, const int32_t *kk_v_dev, const int32_t *bnd_v_dev,
                        int ks_v, int out_size, int max_rows_per_block, int rows_per_block,
                        const float *mean3_host, const float *std3_host, int patch, float *out_dev, void *stream);
/* The same transform with the patch rows written as the tile-major fp16 split operand of lemon_linear_f16x3t (rows = batch *
 * (out_size / patch)^2 padded to 128, k = 3 patch^2; patch % 4 == 0, 3 patch^2 % 16 == 0): the patch embedding then runs in the
 * hand-written GEMM straight from this kernel's output -- no fp32 pixel tensor, no split pass.  Values are exactly the fp16 split
 * (split3.hpp) of what lemon_preprocess_u8 writes. */
int lemon_preprocess_u8_f16x3t(const uint8_t *img_dev, int64_t batch, int in_h, int in_w, const int32_t *kk_h_dev,
                               const int32_t *bnd_h_dev, int ks_h, const int32_t *kk_v_dev, const int32_t *bnd_v_dev,
                               int ks_v, int out_size, int max_rows_per_block, int rows_per_block,
                               const float *mean3_host, const float *std3_host, int patch, uint16_t *outt_dev, void *stream);
/* generic_transform for a RAGGED batch: images of different (H, W), as the file datasets deliver them (the reference decodes and
 * transforms them one by one in 8 forked DataLoader workers: run_lemon.py:129-131,199-201, lib/datasets/dataloader.py:167-198,
 * transform lib/datasets/utils.py:163-170).  Same arithmetic and bits as lemon_preprocess_u8 per image.
 * data_dev: packed uint8 HWC images, data_bytes long.  aux_dev (int64): [batch, 4] descriptors (byte offset into data_dev, H, W, plan index),
 * then [batch + 1] first horizontal-pass block of each image (h_blocks = the last entry), [batch + 1] first vertical-pass
 * block (v_blocks = the last entry), [batch] byte offset of each image's horizontally resampled rows in work_dev.
 * plans_dev (int32): 16 per distinct input shape: H, W, offsets into taps_dev of kk_h, bnd_h, kk_v, bnd_v (the CROPPED PIL
 * tables of lemon_preprocess_u8), ks_h, ks_v, R (output rows per vertical block, R (2 + ks_v) <= 4096), vertical blocks,
 * first input row of the crop window, its input row count, horizontal blocks (16 input rows each), 3 unused.
 * work_dev: >= sum over images of rows x out_size x 3 bytes (4-byte aligned).  Output at batch position i: operand == 0 ->
 * out_dev float32 NCHW (patch == 0) or patch-major (patch > 0) as lemon_preprocess_u8; operand != 0 -> the tile-major fp16
 * split operand of lemon_preprocess_u8_f16x3t (rows = batch (out_size/patch)^2 padded to 128).  Any input size whose vertical
 * window has at most 4 094 taps (R = 1): a short side up to ~1 020 x out_size (229 000 px for 224).  An image whose plan does
 * not match its descriptor, or that does not lie inside data_bytes, is not read and its outputs are NaN. */
int lemon_preprocess_ragged(const uint8_t *data_dev, int64_t data_bytes, int64_t batch, const int64_t *aux_dev, int64_t h_blocks, int64_t v_blocks,
                            const int32_t *plans_dev, const int32_t *taps_dev, uint8_t *work_dev, int out_size,
                            const float *mean3_host, const float *std3_host, int patch, int operand, void *out_dev, void *stream);

/* Multi-head self-attention of the CLIP towers, fused to one pass: the attention inside
 * encode_image / encode_text (lib/models/downstream_models.py:37-41 -> HF CLIPAttention; in-tree twin
 * lib/models/chexzero_clip.py:191-212 with the causal mask of :348-354 for text).
 * qkv_dev [batch, seq_len, 3, heads, head_dim] float32 = the fused q/k/v projection output;
 * out_dev [batch, seq_len, heads*head_dim] = softmax(q k^T / sqrt(head_dim) [+ causal]) v with heads
 * concatenated, ready for the output projection.  head_dim must be 64 (72 .. 128 behind lemon_attention_set_head_dims), seq_len <= LEMON_ATTENTION_MAX_SEQ.
 * seq_len <= 288: one workgroup per (batch, head), K and V of the head staged in LDS once.  Beyond 288 (the 577 tokens of
 * ViT-L/14@336, 1025 at 448 px, long text contexts): the streaming kernels -- query tiles dealt to several workgroups per
 * (batch, head), the keys passing through LDS in blocks of 128 -- with the same arithmetic per key tile, in every output form.
 * Arithmetic (all lemon_attention_* entry points): by default the two products run as SPLIT products on the fp16 matrix cores
 * -- q, k, v and the probabilities are carried as fp16 pairs (hi = f16(v), lo = the remainder: 22 bits + sign, fp32
 * accumulate; error vs float64 at the level of the all-fp32 form).  RANGE: |q|, |k|, |v| must stay below 65 520, beyond that
 * the fp16 parts are inf and the result NaN (loud, not wrong); PRECISION: the short kernels (seq_len <= 64) scale lo by 2^11
 * (full relative precision), the general kernel stores lo unscaled (absolute precision 2^-25: values below 2^-3 keep less than
 * 22 bits, still >= 2^-25 absolute).  lemon_attention_set_f16(0) switches the CALLING THREAD to v_mfma_f32_32x32x2_f32 for both
 * products (no range limit, the fp32 GEMM modes select it; returns the thread's previous setting); $LEMON_ATTN_F16=0 starts
 * every thread there. */
int lemon_attention_f32(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                        int causal, float *out_dev, void *stream);
#define LEMON_ATTENTION_MAX_SEQ 4096
int lemon_attention_set_f16(int on);
/* Sequences LONGER than seq_len go to the streaming kernels, for the calling thread: default 288 (what the one-workgroup
 * kernels hold), accepted 64 .. 288 (anything else: LEMON_E_INVALID, nothing changes); returns the previous value.  The two
 * families give the same bits; the switch exists for the test of that and for A/B timing. */
int lemon_attention_set_stream_min(int seq_len);
/* Head dims other than 64, for the calling thread (opt-in; $LEMON_ATTN_HEAD_DIMS = 1 or 2 starts every thread there, default 0):
 *   0  head_dim must be 64: every lemon_attention_* entry point refuses anything else and writes nothing;
 *   1  head_dim a multiple of 8 in 72 .. 128 (ViT-H/14: 80, g/14: 88, bigG/14: 104) is accepted by all four entry points and
 *      runs one streaming kernel for every seq_len <= LEMON_ATTENTION_MAX_SEQ -- fp32 arithmetic (v_mfma_f32_32x32x2_f32)
 *      under BOTH selections of lemon_attention_set_f16, no input range limit; 64 * 3 * heads * head_dim * 4 < 2^32.  The
 *      split and tile-major output forms have heads*head_dim columns.  head_dim 64 keeps its kernels and their bits;
 *   2  as 1, and head_dim 64 runs that kernel too (bit-identical to the fp32-arithmetic kernels; for the test of that and
 *      for A/B timing).
 * Any other mode: LEMON_E_INVALID, nothing changes.  Returns the previous mode. */
int lemon_attention_set_head_dims(int mode);
/* The calling thread's current mode. */
int lemon_attention_get_head_dims(void);
/* The kernel instantiation the calling thread's last lemon_attention_* call launched, as csrc/attention_plan.hpp names it (e.g.
 * "k_attention_hd64_short<1, 2, true>"); "" before any launch; a refused call and one with batch == 0 leave it as it was.  Host
 * state only.  For tests and tools. */
const char *lemon_attention_last_kernel(void);
/* The same attention with the result written as the 3-way bf16 split activation operand of lemon_linear_bf16x6 (below):
 * out6_dev [batch*seq_len, 6*heads*64] bf16, 16-byte aligned.  The fp32 result is split at the store, not recomputed. */
int lemon_attention_split3(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                           int causal, uint16_t *out6_dev, void *stream);
/* Bidirectional attention with a key length PER SEQUENCE: the padding mask of a BERT text tower whose captions are padded
 * behind their last token (HF BertSelfAttention called with attention_mask = ids != pad, behind lib/models/utils.py:72-78).
 * The four entry points take the arguments of their plain siblings without `causal`, and lengths_dev [batch] int32 on the
 * device; n_b = clamp(lengths[b], 1, seq_len), clamped on the device.
 *   rows t <  n_b of sequence b: attention of query t over keys 0 .. n_b - 1 only;
 *   rows n_b <= t < seq_len:     zeros (hi and lo parts 0 in the split forms; the tile-major form's padded tile rows are not
 *                                written, as in the plain call);
 *   qkv rows t >= n_b are never loaded: NaN, Inf or values beyond the fp16 range there reach no output row t < n_b.
 * head_dim 64 (in every lemon_attention_set_head_dims mode) and 1 <= seq_len <= 288; both arithmetic selections of
 * lemon_attention_set_f16; heads < 19 418.  Anything else: LEMON_E_INVALID, nothing is written.  lengths_dev == NULL: the plain
 * entry point with causal = 0.  Kernel layout, tile walk and summation order are the plain kernels' at the same seq_len: with
 * lengths[b] = seq_len the bits are the plain call's, and a row t < n_b has the bits of the plain call on qkv[b, :n_b] wherever
 * ceil(n_b / 32) = ceil(seq_len / 32).  A key tile or a wave of queries entirely beyond n_b skips its products. */
int lemon_attention_f32_varlen(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                               const int32_t *lengths_dev, float *out_dev, void *stream);
int lemon_attention_split3_varlen(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                                  const int32_t *lengths_dev, uint16_t *out6_dev, void *stream);

/* LayerNorm over the last dimension, float32: y = (x - mean) / sqrt(var + eps) * weight + bias (biased variance, like
 * torch.nn.LayerNorm) -- layer_norm1/2, pre_layrnorm, post_layernorm, final_layer_norm of the towers behind
 * encode_image / encode_text (lib/models/downstream_models.py:37-41; in-tree twin lib/models/chexzero_clip.py:177-183).
 * x_dev, y_dev [rows, width] (y_dev may alias x_dev), width a multiple of 4 and <= 2048, pointers 16-byte aligned. */
int lemon_layernorm_f32(const float *x_dev, const float *weight_dev, const float *bias_dev, float eps, int64_t rows,
                        int width, float *y_dev, void *stream);

/* Token assembly of the towers, one pass each instead of torch's cat / gather + add (+ LayerNorm):
 *   vision (HF CLIPVisionEmbeddings + pre_layrnorm; lib/models/chexzero_clip.py:243-249):
 *     y[b,0] = LN(cls + pos[0]),  y[b,1+p] = LN(patches[b,p] + pos[1+p]);  patches_dev [batch, n_tokens-1, width] is the
 *     patch-embedding GEMM's output, y_dev [batch, n_tokens, width]; ln_weight_dev = ln_bias_dev = NULL: no LayerNorm (timm's
 *     VisionTransformer._pos_embed has none: norm_pre is the identity in BiomedCLIP's vit_base_patch16_224);
 *   text (token + position embedding, chexzero_clip.py:363-365): y[b,t] = tok_emb[ids[b,t]] + pos[t] for t < seq_len;
 *     ids_dev int64 with row pitch ids_pitch >= seq_len (the caller's [batch, context] id matrix, truncated in place; columns
 *     from seq_len on are never read).  An id outside [0, vocab) is CLAMPED to the nearest valid row (id < 0 -> row 0,
 *     id >= vocab -> row vocab - 1), so that no id can make the lookup leave tok_emb_dev; torch's embedding raises instead.
 *   width a multiple of 4 (vision: <= 2048, n_tokens >= 2, LayerNorm weight and bias both given or both NULL); every pointer
 *   16-byte aligned (float4 accesses); a refused call (LEMON_E_INVALID) writes nothing. */
int lemon_vision_tokens_ln(const float *patches_dev, const float *cls_dev, const float *pos_dev,
                           const float *ln_weight_dev, const float *ln_bias_dev, float eps, int64_t batch,
                           int n_tokens, int width, float *y_dev, void *stream);
int lemon_text_tokens(const int64_t *ids_dev, int64_t ids_pitch, const float *tok_emb_dev, const float *pos_dev,
                      int64_t batch, int seq_len, int width, int vocab, float *y_dev, void *stream);

/* Linear layer of the CLIP towers with its element-wise tail fused into the GEMM:
 *   y[m,n] = act(alpha x[m,k] W[n,k]^T + bias[n]) (+ residual[m,n])         float32, row-major
 * (nn.Linear inside HF CLIPEncoderLayer / lib/models/chexzero_clip.py:191-212, driven by
 * lib/models/downstream_models.py:30-41).  The GEMM runs on hipBLASLt; act = LEMON_ACT_SILU
 * (u*sigmoid(u)) and the residual add ride in its epilogue.  QuickGELU z*sigmoid(1.702z)
 * (chexzero_clip.py:186-188) is silu(1.702 z)/1.702: call with alpha = 1.702 and a bias scaled by 1.702,
 * and give the consuming GEMM alpha = 1/1.702 (lemon_amd/clip.py does).  bias_dev / residual_dev may
 * be NULL; residual_dev may alias y_dev; activation and residual cannot be combined.
 * Solution choice per (m,n,k,epilogue,residual) key -- reproducible by default: a key supplied by
 * lemon_linear_load_tuned() uses the recorded hipBLASLt solution index (checked once per process, on first
 * use and on the caller's operands, against the library's first-ranked solution: one extra GEMM, one stream
 * synchronisation; dropped if it disagrees); every other key uses the library's first-ranked supported
 * solution (no timing, no allocation, no synchronisation; identical in every process).  Only after
 * lemon_linear_set_tuning(1) (or LEMON_LINEAR_TUNE=1) is an unknown key benchmarked over all solutions
 * (synchronises; bounded by LEMON_LINEAR_TUNE_MS, default 6000): that is the offline tuner's mode
 * (tools/tune_gemms.py), never the inference path's. */
#define LEMON_ACT_NONE 0
#define LEMON_ACT_SILU 1
/* the exact GELU u/2 (1 + erf(u / sqrt 2)) of the towers of open_clip's BiomedCLIP (lib/models/utils.py:72-78: timm
 * vit_base_patch16_224 blocks and the PubMedBERT layers both use nn.GELU).  In the library GEMMs it runs as one in-place pass
 * behind the bias epilogue (hipBLASLt's own GELU epilogue is the tanh approximation); in lemon_linear_f16x3t(_ln) it rides in
 * the operand epilogue like SiLU. */
#define LEMON_ACT_GELU 2
int lemon_linear_f32(const float *x_dev, const float *w_dev, const float *bias_dev, const float *residual_dev,
                     int64_t m, int n, int k, float alpha, int act, float *y_dev, void *stream);

/* The same nn.Linear (same reference call sites, same epilogues, same fp32 result type) with the products on the bf16
 * matrix cores at fp32-equivalent accuracy: every fp32 operand value v is split EXACTLY into three bf16 parts
 * (hi = bf16(v), mid = bf16(v - hi), lo = bf16(v - hi - mid): 24 significant bits) and the six cross products of order
 * <= 2 are summed by ONE bf16 GEMM with fp32 accumulation over a 6k-long k axis:
 *     x6_dev [m, 6k] rows = [hi | hi | mid | hi | mid | lo]   (lemon_layernorm_split3, or lemon_split3_f32 with weight = 0)
 *     w6_dev [n, 6k] rows = [hi | mid | hi | lo | mid | hi]   (lemon_split3_f32 with weight = 1; once per weight)
 * k6 = 6k.  The dropped products are O(2^-24) of the result; what the GEMM delivers is bounded by its fp32 accumulation, like
 * the fp32 GEMM's own result (max error vs float64, relative to the largest output, 1.3-2.1e-6 at the ViT-B/32 tower shapes;
 * fp32 GEMM 1.0-2.1e-6 -- tools/split_gemm_probe.py).  y_dev / bias_dev / residual_dev are float32. */
int lemon_linear_bf16x6(const uint16_t *x6_dev, const uint16_t *w6_dev, const float *bias_dev, const float *residual_dev,
                        int64_t m, int n, int k6, float alpha, int act, float *y_dev, void *stream);
/* 3-way bf16 split of a row-major float32 matrix [rows, k] (k a multiple of 4) into lemon_linear_bf16x6's operand rows
 * y6_dev [rows, 6k] bf16; weight = 0: activation layout, 1: weight layout. */
int lemon_split3_f32(const float *x_dev, int64_t rows, int k, int weight, uint16_t *y6_dev, void *stream);
/* lemon_layernorm_f32 whose result is written as the split activation operand y6_dev [rows, 6 width] bf16 (one pass). */
int lemon_layernorm_split3(const float *x_dev, const float *weight_dev, const float *bias_dev, float eps, int64_t rows,
                           int width, uint16_t *y6_dev, void *stream);
/* The same nn.Linear once more, with HALF the matrix work of lemon_linear_bf16x6: every fp32 operand value v is split into
 * two fp16 parts, hi = f16(v) and lo = v - hi (exact in fp32; kept as f16(lo * 2^11): 11 + 11 significant bits and lo's sign,
 * |v - hi - lo| <= 2^-23 |v|), and ONE fp16 GEMM with fp32 accumulation over a 3k-long k axis sums hi.hi + hi.lo + lo.hi:
 *     x3_dev [m, 3k] rows = [hi | hi | lo 2^11]            (lemon_layernorm_f16x3 / lemon_attention_f16x3 / lemon_split_f16x3)
 *     w3_dev [n, 3k] rows = [hi | lo | hi 2^-11] of w * wscale   (lemon_split_f16x3 with weight = 1; once per weight)
 * wscale is a power of two chosen by the caller so that max |w| * wscale lies in [2^14, 2^15) (lo and hi 2^-11 of every
 * weight that matters are then fp16 normals); the caller passes alpha / wscale as `alpha`.  k3 = 3k.  The dropped lo.lo
 * product is <= 2^-22 (typically 2^-26) of a product: against float64 the result is as accurate as the fp32 GEMM's
 * (tools/split_gemm_probe.py).  Operand values with |v| >= 65 520 (beyond fp16) turn the outputs they reach into NaN. */
int lemon_linear_f16x3(const uint16_t *x3_dev, const uint16_t *w3_dev, const float *bias_dev, const float *residual_dev,
                       int64_t m, int n, int k3, float alpha, int act, float *y_dev, void *stream);
/* 2-way fp16 split of a row-major float32 matrix [rows, k] (k a multiple of 4) into lemon_linear_f16x3's operand rows
 * y3_dev [rows, 3k] fp16; weight = 0: activation layout (wscale ignored), 1: weight layout of x * wscale (a power of two). */
int lemon_split_f16x3(const float *x_dev, int64_t rows, int k, int weight, float wscale, uint16_t *y3_dev, void *stream);
/* lemon_layernorm_f32 / lemon_attention_f32 whose result is written as the fp16 split activation operand (one pass):
 * y3_dev [rows, 3 width], out3_dev [batch*seq_len, 3*heads*64], 16-byte aligned. */
int lemon_layernorm_f16x3(const float *x_dev, const float *weight_dev, const float *bias_dev, float eps, int64_t rows,
                          int width, uint16_t *y3_dev, void *stream);
int lemon_attention_f16x3(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                          int causal, uint16_t *out3_dev, void *stream);
int lemon_attention_f16x3_varlen(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                                 const int32_t *lengths_dev, uint16_t *out3_dev, void *stream);   /* see lemon_attention_f32_varlen */
/* The MLP of a transformer block (fc1 -> QuickGELU -> fc2; lib/models/downstream_models.py:37-41 via HF CLIPMLP, in-tree twin
 * lib/models/chexzero_clip.py:171-183) with the arithmetic of lemon_linear_f16x3 in a HAND-WRITTEN gfx950 kernel whose operands
 * are tile-major in MFMA fragment order:
 *     activation operand at_dev: ceil(m / 128) * 128 rows x k, halves [row tile of 128][k / 16][hi, lo 2^11][row block of 32]
 *                                [k half][row in block][8 k]  (4 bytes per element; rows >= m need not be initialised)
 *     weight operand wt_dev:     n rows x k of w * wscale, the same with 256-row tiles and parts hi, lo   (lemon_pack_weight_f16x3t)
 * lemon_layernorm_f16x3t writes the activation operand (the LayerNorm in front of fc1); lemon_linear_f16x3t computes
 *     act = LEMON_ACT_NONE, out_operand = 0:  out_dev fp32 [m, n] = alpha * x W^T + bias (+ residual)          (fc2)
 *     act = LEMON_ACT_SILU, out_operand = 1:  out_dev = the activation operand (k' = n) of silu(alpha * x W^T + bias)   (fc1:
 *         the [m, n] fp32 tensor and the split pass over it never exist)
 *     act = LEMON_ACT_GELU, out_operand = 1:  the same with the exact GELU (BiomedCLIP's towers)
 * with n a multiple of 256 and k a multiple of 16; the caller folds 1 / wscale into alpha.  Results are independent of a row's
 * position in the batch (fixed k order, no split-k).  lemon_unpack_act_f16x3t turns an activation operand back into fp32
 * (hi + lo 2^-11; tests). */
int lemon_pack_weight_f16x3t(const float *w_dev, int n, int k, float wscale, uint16_t *wt_dev, void *stream);
int lemon_layernorm_f16x3t(const float *x_dev, const float *weight_dev, const float *bias_dev, float eps, int64_t rows,
                           int width, uint16_t *yt_dev, void *stream);
int lemon_linear_f16x3t(const uint16_t *at_dev, const uint16_t *wt_dev, const float *bias_dev, const float *residual_dev,
                        int64_t m, int n, int k, float alpha, int act, int out_operand, void *out_dev, void *stream);
int lemon_unpack_act_f16x3t(const uint16_t *at_dev, int64_t rows, int k, float *y_dev, void *stream);
/* LayerNorm folded into the hand-written GEMMs (HF CLIPEncoderLayer.layer_norm1 / layer_norm2 in front of q/k/v_proj and
 * mlp.fc1; in-tree twin lib/models/chexzero_clip.py:171-183: ln_1, ln_2).  LN(x) W^T + b = rstd (x W'^T - mean c) + b' with
 * W' = W diag(gamma), c = W' 1, b' = b + W beta, so the GEMM behind a LayerNorm takes the RAW residual stream as its operand:
 *   lemon_linear_f16x3t_ln(..., row_aff_dev, colsum_dev, NULL, NULL):  out = act(row_aff[m].x * (alpha x W'^T) + row_aff[m].y *
 *       colsum[n] + bias[n]) (+ residual) with row_aff [m, 2] = (rstd, -mean rstd) and colsum [n] = alpha * sum_k W'[n, k]
 *       (of the PACKED weight: hi + lo), bias = b'
 *   lemon_linear_f16x3t_ln(..., NULL, NULL, emit_t_dev, emit_stats_dev) (act none, fp32 out):  the fp32 result is ALSO written as
 *       the tile-major activation operand emit_t_dev (ceil(m / 128) * 128 rows x n) and emit_stats_dev [m, n / 128, 2] receives
 *       per row and 128-column group (mean, sum of squared deviations); lemon_ln_finalize merges them into row_aff
 *   lemon_rowstats_f16x3t: operand + row_aff of a tensor no GEMM produced (a tower's first block)
 * k must be a multiple of 32.  With all four extra pointers NULL the call is lemon_linear_f16x3t.
 * Accuracy contract: the fold's rounding error is the un-folded GEMM's times sqrt(1 + mean^2 / var) of the row, so rows with
 * |mean| rstd > 8 (LEMON_LN_FOLD_MAX_SHIFT) get row_aff = (NaN, NaN) from lemon_ln_finalize / lemon_rowstats_f16x3t: their
 * output rows come out non-finite and the caller must redo them without the fold (lemon_amd.pipeline.Embedder re-embeds the
 * micro-batch with LayerNorm kernels). */
int lemon_linear_f16x3t_ln(const uint16_t *at_dev, const uint16_t *wt_dev, const float *bias_dev, const float *residual_dev,
                           int64_t m, int n, int k, float alpha, int act, int out_operand, void *out_dev, const float *row_aff_dev,
                           const float *colsum_dev, uint16_t *emit_t_dev, float *emit_stats_dev, void *stream);
/* The producing GEMM of a block chain (HF CLIPEncoderLayer: self_attn.out_proj and mlp.fc2 with their residual adds;
 * lib/models/chexzero_clip.py:191-212) in its leanest form -- lemon_linear_f16x3t_ln's emit side with two options:
 *   residual_t_dev  the residual as the tile-major activation operand [m, n] an emitting GEMM in front left (x = hi + lo 2^-11:
 *                   22 significant bits -- one more rounding of the size the split products make anyway) instead of residual_dev
 *                   (fp32 [m, n]); at most one of the two may be given
 *   out_dev = NULL  no fp32 result: every consumer reads emit_t_dev (the next GEMM as its operand, the one behind it as its
 *                   residual) -- the output projection then writes 6 instead of 10 bytes per element
 * emit_t_dev / emit_stats_dev as in lemon_linear_f16x3t_ln (both required); act none; k a multiple of 32. */
int lemon_linear_f16x3t_chain(const uint16_t *at_dev, const uint16_t *wt_dev, const float *bias_dev, const float *residual_dev,
                              const uint16_t *residual_t_dev, int64_t m, int n, int k, float alpha, float *out_dev,
                              uint16_t *emit_t_dev, float *emit_stats_dev, void *stream);
int lemon_ln_finalize(const float *partials_dev, int64_t rows, int width, float eps, float *row_aff_dev, void *stream);
int lemon_rowstats_f16x3t(const float *x_dev, float eps, int64_t rows, int width, uint16_t *yt_dev, float *row_aff_dev, void *stream);
/* Timing of the hand-written GEMM (no reference counterpart; bench.py's roofline object): while profiling is on every
 * lemon_linear_f16x3t launch of this process is bracketed by HIP events on its launch stream (a pool that grows with the
 * launches between two reads; a launch that cannot get its events fails with LEMON_E_HIP, none is silently left out).
 * profile_read waits for the recorded events, returns the number
 * of bracketed launches, their summed durations and their summed arithmetic (2 m n 3k: the three fp16 products the kernel
 * executes per fp32 product), and rewinds the pool. */
int lemon_linear_f16x3t_set_profiling(int on);
/* The matrix instruction of lemon_linear_f16x3t: 16 = v_mfma_f32_16x16x32_f16 (default wherever k is a multiple of 32), 32 =
 * v_mfma_f32_32x32x16_f16 (always used for the other k), 0 = back to the default ($LEMON_GEMM_MFMA).  Same arithmetic, another
 * summation order inside a k32 step; process-wide, for A/B runs and tests.  Returns the previous setting (>= 0) or an error. */
int lemon_linear_f16x3t_set_mfma(int shape);
int lemon_linear_f16x3t_profile_read(int64_t *launches, double *kernel_ms, double *flops);
/* The kernel instantiation the calling thread's last lemon_linear_f16x3t / _ln / _chain call launched, as
 * csrc/gemm_f16x3_plan.hpp names it (e.g. "k_gemm_f16x3t16<0, false, true, 2>"); "" before any launch.  For tests and tools. */
const char *lemon_linear_f16x3t_last_kernel(void);
/* lemon_attention_f32 whose result is written as that activation operand (rows = batch*seq_len, k = heads*64): the output
 * projection then runs in the hand-written GEMM too (with QKV: all four GEMMs of a block). */
int lemon_attention_f16x3t(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                           int causal, uint16_t *outt_dev, void *stream);
int lemon_attention_f16x3t_varlen(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                                  const int32_t *lengths_dev, uint16_t *outt_dev, void *stream);  /* see lemon_attention_f32_varlen */
/* Recorded solution choices: a "# lemon_linear hipblaslt=<version> arch=<gfx name>" stamp line followed by
 * "m,n,k,epilogue,residual,index,usec" lines.  load returns the number of keys taken -- 0 when the stamp
 * does not match this process's hipBLASLt version / device arch (the file is then ignored) -- and dump the
 * number written (<0 on error).  lemon_linear_stamp reports the stamp of the current device. */
int lemon_linear_load_tuned(const char *path);
int lemon_linear_dump_tuned(const char *path);
int lemon_linear_set_tuning(int enabled);
int lemon_linear_stamp(int *hipblaslt_version, char *arch, int arch_len);

/* ---- flat index (faiss.IndexFlatIP / IndexFlatL2 as used by run_lemon.py) ---------- */

/* faiss.IndexFlatIP(d) / faiss.IndexFlatL2(d): run_lemon.py:167-168,171-172;
 * lib/baselines/discrepancy_baseline.py:150-155.  Binds to the current HIP device. */
int lemon_index_create(int metric, int d, lemon_index_t **out);
int lemon_index_free(lemon_index_t *idx);

/* index.add(x): run_lemon.py:175-176.  Copies x (like faiss) and builds the kernel-side
 * layouts; may be called repeatedly (appends).  Allocates device memory: NOT capturable
 * in a hipGraph, and it synchronises `stream` when it has to grow its storage. */
int lemon_index_add(lemon_index_t *idx, const float *x_dev, int64_t n, void *stream);

int64_t lemon_index_ntotal(const lemon_index_t *idx); /* faiss index.ntotal */
int lemon_index_dim(const lemon_index_t *idx);        /* faiss index.d      */
/* device pointer to the stored row-major copy [ntotal, d] (valid until the next add/free) */
const float *lemon_index_data(const lemon_index_t *idx);

/* index.search(x, k): run_lemon.py:235-236; lib/baselines/discrepancy_baseline.py:166,209.
 * D_dev [nq,k] float32 and I_dev [nq,k] int64, best first (IP: descending inner product;
 * L2: ascending SQUARED distance max(0, |q|^2+|x|^2-2<q,x>)).  Slots beyond ntotal get
 * I=-1 and D=-FLT_MAX (IP) / +FLT_MAX (L2).  1 <= k <= LEMON_MAX_K_DEEP (2048; faiss itself has no limit): up to
 * LEMON_MAX_K (64) one scan pass; deeper lists are produced LEMON_MAX_K at a time by key-bounded passes of the exact
 * fp32 scan (each pass admits only rows ranked behind the previous pass's last result: same order, same tie rule).
 * Non-finite scores follow faiss, whose heaps start at -/+FLT_MAX: a row whose inner product is NaN or -inf, or whose
 * L2 distance is +inf, is never returned (a list left with fewer than k rows ends in padding, as beyond ntotal); +inf inner products rank first,
 * ties by ascending index; the L2 expression above is taken literally, so a NaN inside it gives distance 0.
 * Grows an internal workspace on first use of a larger (nq,k): that first call is not
 * graph-capturable; later calls with nq,k no larger only enqueue kernels.  With LEMON_ALGO_AUTO
 * (default) the first LARGE search (ntotal >= 65536, nq*ntotal >= 8e9, d <= 768 -- d <= 1280 once
 * lemon_index_set_wide_filter(idx, 1) has switched the wide filter kernel on) after an add()
 * runs a small probe search and synchronises the stream once to choose between the two scans.
 * q_dev: 16-byte aligned when d % 4 == 0 (see "row alignment" above), else LEMON_E_INVALID. */
int lemon_index_search(lemon_index_t *idx, const float *q_dev, int64_t nq, int k,
                       float *D_dev, int64_t *I_dev, void *stream);
int lemon_index_set_algo(lemon_index_t *idx, int algo);
/* index.search(x, k) on embeddings wider than 768 (run_lemon.py:235-236 with a ViT-H/14, g/14 or bigG/14 tower: d = 1024 /
 * 1280): enabled != 0 lets LEMON_ALGO_BF16_FILTER serve 768 < d <= 1280 with a register-resident fp16 filter kernel (16-bit
 * copies at column pitch 1024 / 1280) and raises LEMON_ALGO_AUTO's width limit from 768 to 1280; results stay bit-identical to
 * LEMON_ALGO_F32_MFMA.  Off by default (LEMON_WIDE_FILTER=1 turns it on process-wide): with it off every call takes the path
 * it took before.  Toggling it on an index whose 16-bit copy exists at the other pitch rebuilds that copy at the next filter
 * search (one stream synchronisation). */
int lemon_index_set_wide_filter(lemon_index_t *idx, int enabled);
/* Which scan kernel served the last index.search (run_lemon.py:235-236) -- the family name of its dominant kernel, a static
 * string: "scan_f32" (LEMON_ALGO_F32_MFMA), or for LEMON_ALGO_BF16_FILTER "scan_bf16" (streaming), "qs", "qs2", "qs4"
 * (Q-stationary, d <= 768) or "qsw" (Q-stationary, 768 < d <= 1280 with the wide filter on); "" before any search.
 * lemon_search_info_t cannot tell "qsw" from "scan_bf16": both run 128-query panels. */
const char *lemon_index_last_scan_kernel(const lemon_index_t *idx);
/* Query de-duplication (on by default; LEMON_QUERY_DEDUP=0 disables it process-wide): from 1024 queries on, the rows of
 * q are grouped by content (64-bit hash + stable sort + full bitwise comparison) and, when at most half of them are
 * distinct, the search runs once per distinct row and its (D, I) lists are copied to every member -- exact, because a
 * query's result does not depend on the other queries.  Classification datasets make the text-side search of
 * run_lemon.py:236 a C-query problem this way.  Costs one stream synchronisation per search call of >= 1024
 * queries (the group count is read back to size the reduced search) -- the one exception to "later calls only enqueue
 * kernels" above; lemon_index_set_query_dedup(idx, 0) restores it.  lemon_neighbors applies de-duplication to its TEXT
 * index only (image queries of the LEMoN loop are distinct), so its image-side search never synchronises. */
int lemon_index_set_query_dedup(lemon_index_t *idx, int enabled);

/* last search's dominant-kernel launch statistics (for bench/roofline bookkeeping) */
typedef struct {
    int algo;            /* LEMON_ALGO_* actually used                       */
    int grid, block;     /* launch geometry of the scan kernel               */
    int query_panel;     /* query rows per workgroup (B of the scan model)   */
    int db_splits;       /* how many workgroups share one query panel        */
    int64_t nq, n;       /* the call's nq (also when duplicate queries were folded: see nq_distinct) and ntotal */
    int d, k;
    int64_t nq_distinct; /* query rows actually searched (== the call's nq unless duplicates were folded) */
} lemon_search_info_t;
int lemon_index_last_search_info(const lemon_index_t *idx, lemon_search_info_t *out);

/* Optional in-library timing of the scan kernel (the dominant kernel of search): when enabled,
 * every scan launch is bracketed by hipEvents recorded on the launch stream.
 * lemon_index_profile_read synchronises those events (host sync!) and returns, summed since the
 * last reset: launches, kernel milliseconds, algorithmic flops (2*nq*n*d) and algorithmic HBM bytes
 * of the scan model (4*d*(nq + ceil(nq/B)*n) + 12*k*nq with B = query_panel); then
 * resets the counters.  Any output pointer may be NULL. */
int lemon_index_set_profiling(lemon_index_t *idx, int enabled);
int lemon_index_profile_read(lemon_index_t *idx, int64_t *launches, double *kernel_ms,
                             double *algo_flops, double *algo_bytes);

/* Host-only view of how the exact scan (LEMON_ALGO_F32_MFMA) decomposes `panels` query panels (128 queries each) x
 * `n_tiles` database tiles (128 rows each) over its workgroups: for tests and tools, no device is touched (the plan is that
 * of a device of 256 CUs, under the LEMON_XCDS / LEMON_SEG_COST of the environment at the time of the call).
 *   seg_begin [*grid + 1]  first segment of every workgroup (cap_wgs + 1 ints of room)
 *   pieces    [panels]     pieces the panel is scanned in (what the merge combines)
 *   segs      [4 * *n_segs] (panel, first tile, tiles, piece number inside the panel) per segment (cap_segs segments of room)
 * Returns LEMON_E_ARG when an output does not fit. */
int lemon_debug_scan_plan(int panels, int n_tiles, int *grid, int *splits, int *seg_begin, int cap_wgs,
                          int *pieces, int *segs, int cap_segs, int *n_segs);

/* ---- multimodal neighbours (the per-sample loop run_lemon.py:238-307) ------------- */

/*
 * One call = one split of the reference's scoring loop.
 *   idx_img / idx_txt : indices over the normalised DB image / text embeddings (same
 *                       ntotal, d and metric); dists_tr_dev [ntotal] (run_lemon.py:169/173)
 *   q_img_dev, q_txt_dev [nq,d] normalised query embeddings (run_lemon.py:230-233)
 *   drop_self : 1 on the train split -- search k+1 (:235-236) then drop result[0] where
 *               in_db_dev[i] != 0 else result[-1] (:257-263,277-283); in_db_dev [nq] u8,
 *               may be NULL (= all ones) and is ignored when drop_self == 0
 *   discrete  : --use_discrete_for_text (:266-267): dists_n = 1 - [tr_label_id[I_n] == q_label_id]
 *               (int32 ids of the prompt strings; may be NULL when discrete == 0)
 * Outputs, caller-allocated: d1 [nq]; D_n, dists_n, dists_tr_n, D_m, dists_m, dists_tr_m [nq,k]
 * float32 with the sign convention of :269-270,285-286; I_n, I_m [nq,k] int64 (may be NULL).
 * Neighbours that do not exist (ntotal < k+drop_self) give I=-1 and NaN distances.
 * Limit: k + drop_self <= LEMON_MAX_K (64), i.e. k <= 63 on the train split -- the faiss contract behind :235-236 has no
 * such limit, but the loop's per-sample record is built from ONE scan pass here; the reference's own grids stop at
 * k = 50 (+1) (experiments.py:86), and deeper lists are available from lemon_index_search (k <= 2048).  Larger k is
 * refused with LEMON_E_INVALID, never truncated.  De-duplication of identical query rows is applied to idx_txt only.
 * q_img_dev, q_txt_dev: 16-byte aligned when d % 4 == 0 (see "row alignment" above), else LEMON_E_INVALID and no output
 * is written.
 */
int lemon_neighbors(lemon_index_t *idx_img, lemon_index_t *idx_txt, const float *dists_tr_dev,
                    const float *q_img_dev, const float *q_txt_dev, int64_t nq, int k,
                    int drop_self, const uint8_t *in_db_dev, int discrete,
                    const int32_t *tr_label_id_dev, const int32_t *q_label_id_dev,
                    float *d1_dev, float *D_n_dev, float *dists_n_dev, float *dists_tr_n_dev,
                    int64_t *I_n_dev, float *D_m_dev, float *dists_m_dev, float *dists_tr_m_dev,
                    int64_t *I_m_dev, void *stream);

/* ---- metric sweep: the euclidean lists of the reference's grid from the cosine scan (experiments.py crosses dist_type with
 * everything; DESIGN.md section 4, "Metric sweep") ------------------------------------------------------------------------
 *
 * lemon_index_l2_from_ip: the k list IndexFlatL2.search would return for the rows of q_dev over the rows of `idx`, an
 * IndexFlatIP, derived from that index's own search output D_ip_dev / I_ip_dev [nq, kd] (kd >= k, best first, padding I = -1
 * at the end) without another scan: D = max(0, fmaf(-2, s, dot(q,q) + dot(x,x))), the numeric contract's own expression on
 * the list's scores, the stored row norms and one chain per query; the first k by (D ascending, id ascending) go to
 * D_l2_dev / I_l2_dev [nq, k] (slots beyond the DB: I = -1, D = +FLT_MAX).  cert_dev, uint8 [nq]: 1 where the row is PROVEN
 * to equal the L2 search bit for bit -- the list holds the whole DB, or D of slot k-1 is strictly below the bound
 * max(0, fmaf(-2, s_{kd-1}, dot(q,q) + min_x dot(x,x))) that no row outside the list can undercut (fp32 add, fmaf and max
 * are monotone: csrc/l2_from_ip_core.hpp); 0 where it is not, where dot(q,q), a listed score or any stored norm is not finite,
 * or where an id is not a row of the index.  A row with cert 0 is still written but must be searched with an IndexFlatL2.
 * Refused with LEMON_E_INVALID, nothing written: a null pointer, an index that is not IP, k < 1, k > kd, kd > LEMON_MAX_K,
 * q_dev not 16-byte aligned when d % 4 == 0.  The smallest stored norm is reduced on the device once per index content
 * (the first call after an add) and kept; dot(q,q) lives in the index's neighbour workspace, which the first larger call
 * grows (one stream synchronisation and a device allocation) and later calls only reuse.
 * lemon_l2_from_ip_host: the same header with the lanes looped, on host pointers, for the tests: qq [nq], xx [n] and xx_min
 * are brought by the caller (xx_min: NaN when any norm is not finite). */
int lemon_index_l2_from_ip(lemon_index_t *idx, const float *q_dev, int64_t nq, const float *D_ip_dev, const int64_t *I_ip_dev,
                           int kd, int k, float *D_l2_dev, int64_t *I_l2_dev, uint8_t *cert_dev, void *stream);
int lemon_l2_from_ip_host(const float *qq, const float *xx, int64_t n, float xx_min, const float *D_ip, const int64_t *I_ip,
                          int64_t nq, int kd, int k, float *D_l2, int64_t *I_l2, uint8_t *cert);

/* lemon_neighbors for both metrics from one search a side.  idx_img / idx_txt: IndexFlatIP over the normalised DB rows;
 * dists_tr_ip_dev / dists_tr_l2_dev [ntotal]: run_lemon.py:169 and :173.  Each side is searched once at
 * kd = min(LEMON_MAX_K, k + drop_self + margin), margin >= 0.  The first set of outputs is what lemon_neighbors writes for an
 * IP pair (an exact list is a prefix of every deeper one); the second set (*_l2_dev) is what it writes for an L2 pair WHERE
 * cert_n_dev[i] and cert_m_dev[i] (uint8 [nq], the certificate of lemon_index_l2_from_ip at depth k + drop_self on the image
 * and the text side) are both 1: record row i of the second set reads the derived lists, and a side whose certificate is 0
 * may differ from the L2 search, so such rows must be replaced by lemon_neighbors on an IndexFlatL2 pair.  Every other
 * argument, limit and refusal as lemon_neighbors; I_* may be NULL; de-duplication on the text side only. */
int lemon_neighbors_metrics(lemon_index_t *idx_img, lemon_index_t *idx_txt, const float *dists_tr_ip_dev,
                            const float *dists_tr_l2_dev, const float *q_img_dev, const float *q_txt_dev, int64_t nq, int k,
                            int drop_self, const uint8_t *in_db_dev, int discrete, const int32_t *tr_label_id_dev,
                            const int32_t *q_label_id_dev, int margin,
                            float *d1_dev, float *D_n_dev, float *dists_n_dev, float *dists_tr_n_dev, int64_t *I_n_dev,
                            float *D_m_dev, float *dists_m_dev, float *dists_tr_m_dev, int64_t *I_m_dev,
                            float *d1_l2_dev, float *D_n_l2_dev, float *dists_n_l2_dev, float *dists_tr_n_l2_dev,
                            int64_t *I_n_l2_dev, float *D_m_l2_dev, float *dists_m_l2_dev, float *dists_tr_m_l2_dev,
                            int64_t *I_m_l2_dev, uint8_t *cert_n_dev, uint8_t *cert_m_dev, void *stream);

/* Discrepancy baselines, lib/baselines/discrepancy_baseline.py:164-242 (next-row scope).
 * method 0 = dis_x / dis_y: mean cosine distance between the query's embedding qv_dev [nq,d] and the
 * second-order neighbours (through the DB's own text kNN cache of k+1, self removed by index, :165-169)
 * of its k (+1 on train, not dropped) text neighbours; method 1 = div_x / div_y: sum of pairwise cosine
 * distances inside the neighbour set divided by k^2.  E_tr_dev [ntotal,d] are the DB embeddings of the
 * scored modality (x: image, y: text); neighbours always come from idx_txt (:209).  out_dev [nq].
 * E_tr_dev, qv_dev, q_txt_dev: 16-byte aligned when d % 4 == 0 (see "row alignment" above), else LEMON_E_INVALID. */
int lemon_discrepancy(int method, lemon_index_t *idx_txt, const float *E_tr_dev, const float *qv_dev,
                      const float *q_txt_dev, int64_t nq, int k, int is_train, float *out_dev, void *stream);

/* The database's own text neighbours for the dis_* scores, lib/baselines/discrepancy_baseline.py:165-169 (the cache the
 * reference builds once per run; experiments.py:141-177 runs it once per grid point): the top-kc list of every row of idx_txt
 * among the rows of idx_txt, self included, into Ic_dev, int64 [ntotal, kc], owned by the caller.  2 <= kc <= LEMON_MAX_K.
 * Nothing is kept on the index: a cache belongs to the ntotal it was built at, and lemon_discrepancy_ks checks that count.
 * May grow the index's neighbour workspace on first use (one stream synchronisation and a device allocation), as
 * lemon_discrepancy does. */
int lemon_discrepancy_cache(lemon_index_t *idx_txt, int kc, int64_t *Ic_dev, void *stream);

/* lemon_discrepancy for every method and a list of knn_k in one call, lib/baselines/discrepancy_baseline.py:164-242 on the grid
 * of experiments.py:141-177 (four methods x eight knn_k per dataset and seed).  out_dev is float32 [4][n_ks][nq] in the order
 * dis_x, dis_y, div_x, div_y; out[m][t][i] has the bits lemon_discrepancy(method m, k = ks[t]) writes for query i, NaN
 * included.  methods: bit 0 dis_x, bit 1 dis_y, bit 2 div_x, bit 3 div_y (at least one); a method that is not selected leaves
 * its rows of out_dev untouched.  ks: HOST int32, strictly ascending, 1 <= ks[0], ks[n_ks-1] + 1 <= LEMON_MAX_K.
 * E_img_tr_dev / E_txt_tr_dev [ntotal,d]: the DB embeddings (either may be NULL when no method reads it: x image, y text);
 * q_img_dev may be NULL unless dis_x is selected.  Ic_dev [cache_rows, kc]: what lemon_discrepancy_cache wrote, kc >=
 * ks[n_ks-1] + 1 (a wider cache serves: an exact list is a prefix of every deeper one); NULL is allowed when no dis_* bit is
 * set.  cache_rows must equal the index's ntotal (a cache built before an add is refused), else LEMON_E_INVALID.
 * One text search of the queries at ks[n_ks-1] + is_train; each query's pair distances are computed once at that depth and
 * every k sums its prefix of them in lemon_discrepancy's order.  Row alignment and every other refusal as lemon_discrepancy
 * (an empty index is refused as well); a refused call writes nothing.  nq < 2^31.  May grow the index's neighbour workspace on
 * first use (one stream synchronisation and a device allocation), as lemon_discrepancy does.
 * lemon_discrepancy_ks_host: the summation header compiled for the host (the 64 lanes looped) for ONE method (0 dis, 1 div) and
 * one modality, on host pointers and on neighbour lists the caller brings instead of an index: E [n,d], qv [nq,d] (dis only),
 * Im [nq, ks[n_ks-1] + is_train], Ic [n, kc] (dis only); out [n_ks][nq].  Row ids >= n are refused. */
int lemon_discrepancy_ks(lemon_index_t *idx_txt, const float *E_img_tr_dev, const float *E_txt_tr_dev,
                         const float *q_img_dev, const float *q_txt_dev, int64_t nq, const int32_t *ks, int n_ks,
                         int is_train, int methods, const int64_t *Ic_dev, int64_t cache_rows, int kc, float *out_dev,
                         void *stream);
int lemon_discrepancy_ks_host(int method, const float *E, int64_t n, int d, const float *qv, const int64_t *Im, int64_t nq,
                              const int64_t *Ic, int kc, const int32_t *ks, int n_ks, int is_train, float *out);

/* lib/metrics/utils.py:47-82 calc_scores_given_hparams_vectorized (== loop twin :21-45):
 * score = d_1 + beta*mean_j[e^{-tau_1_n D_n} e^{-tau_2_n dists_tr_n} dists_n] + gamma*(same for m).
 * hp = {beta, gamma, tau_1_n, tau_2_n, tau_1_m, tau_2_m} (host doubles, passed by value in the
 * launch).  score_dev [n] float64; d_n_dev / d_m_dev [n] float64 or NULL. */
int lemon_score(const float *d1_dev, const float *D_n_dev, const float *dists_tr_n_dev,
                const float *dists_n_dev, const float *D_m_dev, const float *dists_tr_m_dev,
                const float *dists_m_dev, int64_t n, int k, const double hp[6],
                double *score_dev, double *d_n_dev, double *d_m_dev, void *stream);

/* The hyper-parameter grid of run_lemon.py:319-384 as one batch: for each of G rows of hp_dev
 * [G,6] = (beta, gamma, tau_1_n, tau_2_n, tau_1_m, tau_2_m) the scores of lemon_score (same float64
 * arithmetic) and optimize_f1_efficient (lib/metrics/utils.py:286-296: scipy fminbound on -F1(y, score >= t),
 * xtol, maxfun) -> f1_dev[G], thres_dev[G] (float64), bit-identical to evaluating the grid points one by one
 * on the host.  y_dev [n] uint8 (is_mislabel); scores_ws_dev: caller-provided [G, n] float64 workspace;
 * G <= 65535.  A grid point whose scores are not all finite gets f1 = 0, thres = NaN. */
int lemon_grid_f1(const float *d1_dev, const float *D_n_dev, const float *dists_tr_n_dev, const float *dists_n_dev,
                  const float *D_m_dev, const float *dists_tr_m_dev, const float *dists_m_dev,
                  const uint8_t *y_dev, int64_t n, int k, const double *hp_dev, int G, double xtol, int maxfun,
                  double *scores_ws_dev, double *f1_dev, double *thres_dev, void *stream);

/* lemon_grid_f1 for several knn_k from ONE record: the six neighbour arrays are [n, kmax] (row pitch kmax) and for every
 * k in ks[K] (host ints, strictly ascending, 1 <= ks[0], ks[K-1] <= kmax <= LEMON_MAX_K, 1 <= K <= LEMON_KSWEEP_MAX_KS) the
 * outputs are what lemon_grid_f1 returns on the contiguous [n, k] prefix of the record, bit for bit: f1_dev, thres_dev [K, G]
 * float64 and, when scores_dev is not NULL, the scores [K, G, n] float64.  hp [G, 6] is a HOST pointer (as in lemon_score);
 * rows are arbitrary -- the neighbour terms are computed once per distinct (tau_1, tau_2) bit pattern of a side and once per
 * sample for all ks (an exact top-k list is a prefix of every deeper one and the score sum runs in column order).
 * ws_dev: caller-provided device workspace of at least lemon_grid_f1_ks_workspace_bytes(n, K, G, hp) bytes (ws_bytes says how
 * many there are), 8-byte aligned; nothing is allocated on the device.  The call waits for the stream once, when the row
 * tables have been handed to it.  G <= 65535.  Anything out of contract is refused with LEMON_E_INVALID and nothing is
 * written.  lemon_grid_f1_ks_workspace_bytes returns -1 for arguments out of contract. */
#define LEMON_KSWEEP_MAX_KS 16
int64_t lemon_grid_f1_ks_workspace_bytes(int64_t n, int K, int G, const double *hp);
int lemon_grid_f1_ks(const float *d1_dev, const float *D_n_dev, const float *dists_tr_n_dev, const float *dists_n_dev,
                     const float *D_m_dev, const float *dists_tr_m_dev, const float *dists_m_dev,
                     const uint8_t *y_dev, int64_t n, int kmax, const int *ks, int K, const double *hp, int G,
                     double xtol, int maxfun, void *ws_dev, int64_t ws_bytes, double *scores_dev, double *f1_dev,
                     double *thres_dev, void *stream);

/* The local searches in front of the grid (lib/metrics/utils.py:143-158: scipy.optimize.minimize with Powell and Nelder-Mead
 * from every start point, options={}) as ONE launch: S searches, one workgroup each, no host synchronisation inside a search.
 * The record is lemon_grid_f1_ks's: d1 [n], six neighbour arrays [n, kmax] (row pitch kmax), y [n] uint8 (is_mislabel).
 * x0 [S, 6] float64 start points in the order (beta, gamma, tau_1_n, tau_2_n, tau_1_m, tau_2_m); spec [S, 4] int32 =
 * (method, k with 1 <= k <= kmax: the search sees the [n, k] prefix of the record, force_zero mask, force_one mask; bit i of a
 * mask = hyper-parameter i, zeros are applied first as metrics.unpack_vector does; the optimiser keeps moving a forced
 * coordinate, the objective ignores it).  The objective is maximize_metric's: 0.0 when a score is not finite, else -F1 at the
 * threshold of optimize_f1_efficient (fminbound, xtol 1e-8, maxfun 500), scores with lemon_score's arithmetic.  The optimisers
 * restate scipy 1.15 in IEEE double (csrc/hparam_search_core.hpp): out[s] = (x, fun, nfev, nit, status) of
 * scipy.optimize.minimize on that objective, bit for bit; status is scipy's (0 ok, 1 maxfev, 2 maxiter, 3 NaN), or 5 where
 * scipy's bracket() would raise at its iteration limit.  Nelder-Mead orders tied vertices as np.argsort does on x86-64 with
 * AVX-512 (an 8-lane network, not a stable sort).
 * lemon_hparam_search: every pointer is a device pointer; ws: lemon_hparam_search_workspace_bytes(n, S) bytes, 8-byte
 * aligned, used when the score row of a search (8 n bytes, beside n bytes of labels) does not fit into 48 KB of LDS.  The call
 * waits for the stream once, to check spec before anything is launched.  Refused with LEMON_E_INVALID, nothing written: a null
 * pointer, n <= 0, k outside [1, kmax], an unknown method, a mask beyond six bits, a short workspace, S > 65535.
 * lemon_hparam_search_host / lemon_hparam_objective_host: the same header compiled for the host (threads looped, libm's
 * exp), host pointers; for the tests, no product path calls them.  The objective returns NaN for arguments out of contract.
 * lemon_hparam_search_set_test_knobs: test-only.  force_workspace != 0 keeps the score rows out of LDS; the four caps
 * (Nelder-Mead maxiter / maxfev, Powell maxiter / maxfev; <= 0 = scipy's defaults 1200, 1200, 6000, 6000) apply to both
 * forms.  Recorded time (tools/hparam_search_time.py): 64 searches at n = 5 000, kmax = 50 in 0.42 s. */
#define LEMON_SEARCH_NELDER_MEAD 0
#define LEMON_SEARCH_POWELL 1
typedef struct LemonSearchResult { double x[6]; double fun; int32_t nfev, nit, status, pad; } LemonSearchResult;
int64_t lemon_hparam_search_workspace_bytes(int64_t n, int S); /* < 0: LEMON_E_* */
int lemon_hparam_search(const float *d1, const float *D_n, const float *dists_tr_n, const float *dists_n,
                        const float *D_m, const float *dists_tr_m, const float *dists_m, const uint8_t *y,
                        int64_t n, int kmax, int S, const double *x0, const int32_t *spec,
                        void *ws, int64_t ws_bytes, LemonSearchResult *out, void *stream);
int lemon_hparam_search_host(const float *d1, const float *D_n, const float *dists_tr_n, const float *dists_n,
                             const float *D_m, const float *dists_tr_m, const float *dists_m, const uint8_t *y,
                             int64_t n, int kmax, int S, const double *x0, const int32_t *spec,
                             void *ws, int64_t ws_bytes, LemonSearchResult *out);
double lemon_hparam_objective_host(const float *d1, const float *D_n, const float *dists_tr_n, const float *dists_n,
                                   const float *D_m, const float *dists_tr_m, const float *dists_m, const uint8_t *y,
                                   int64_t n, int kmax, int k, int force_zero, int force_one, const double *x);
int lemon_hparam_search_set_test_knobs(int force_workspace, int nm_maxiter, int nm_maxfun, int powell_maxiter,
                                       int powell_maxfun);

/* The LBFGS polish of maximize_metric (lib/metrics/utils.py:160-176: torch_minimize :129-141 on the SoftMargin proxy
 * :121-127,148-149) as ONE launch: S polishes on one record, one workgroup each.  The record and y as in lemon_hparam_search.
 * x0 [S, 6] double: the start points; spec int32 [S, 3]: (k, force_zero, force_one) with 1 <= k <= kmax (the polish sees
 * the [n, k] prefix) and the six-bit force masks of lemon_hparam_search.  outer_steps: optimizer.step calls, 1 .. 20 (the
 * reference's is 20).  The proxy is loss = mean_i log1p(exp(-t_i s_i)), t = 2 y - 1, s = the score with ONE exp per element,
 * exp(-(tau_1 D + tau_2 tr)), in float64 on the float32 record, with its gradient in the same pass; exp and log1p are restated
 * with explicit fma and every sum has a fixed order (csrc/lbfgs_core.hpp), so the result is a function of the record alone and
 * the device and the host twin agree bit for bit.  It is not bit-compatible with torch's float32-promoted two-exp expression;
 * the candidate is scored exactly afterwards, as the reference does.  The optimiser restates torch.optim.LBFGS (torch 2.10:
 * lr 0.1, max_iter 20, max_eval 25, history 100, strong_wolfe) with the state kept over the outer steps.  Nothing is clamped:
 * an overflow becomes inf or NaN as in torch and flows to the result; out[s].status is 1 where x or loss is not finite, else 0.
 * lemon_lbfgs_polish: every pointer is a device pointer; the call waits for the stream once, to check spec before anything
 * is launched.  Refused with LEMON_E_INVALID, nothing written: a null pointer, n <= 0, k outside [1, kmax], a mask beyond six
 * bits, S > 65535, outer_steps outside [1, 20].
 * lemon_lbfgs_polish_host / lemon_lbfgs_proxy_host: the same header compiled for the host (threads looped, the same
 * reduction order), host pointers; for the tests, no product path calls them.  The proxy returns the loss and writes grad[6];
 * NaN for arguments out of contract.  lemon_lbfgs_math_host: test-only, the restated exp (fn 0) / log1p (fn 1) on count
 * host doubles. */
typedef struct LemonPolishResult { double x[6]; double loss; int32_t nfev, nit, status, pad; } LemonPolishResult;
int lemon_lbfgs_polish(const float *d1, const float *D_n, const float *dists_tr_n, const float *dists_n,
                       const float *D_m, const float *dists_tr_m, const float *dists_m, const uint8_t *y,
                       int64_t n, int kmax, int S, const double *x0, const int32_t *spec, int outer_steps,
                       LemonPolishResult *out, void *stream);
int lemon_lbfgs_polish_host(const float *d1, const float *D_n, const float *dists_tr_n, const float *dists_n,
                            const float *D_m, const float *dists_tr_m, const float *dists_m, const uint8_t *y,
                            int64_t n, int kmax, int S, const double *x0, const int32_t *spec, int outer_steps,
                            LemonPolishResult *out);
double lemon_lbfgs_proxy_host(const float *d1, const float *D_n, const float *dists_tr_n, const float *dists_n,
                              const float *D_m, const float *dists_tr_m, const float *dists_m, const uint8_t *y,
                              int64_t n, int kmax, int k, int force_zero, int force_one, const double *x, double *grad);
int lemon_lbfgs_math_host(int fn, const double *x, int64_t count, double *out);

/* metrics.eval_metrics (lib/metrics/utils.py:273-441: optimize_f1 :273-284, f1_with_pred_prev_constraint(2) :298-322,
 * f1_with_local_minima_finder :327-349, the counts of binary_metrics :351-405, prob_metrics :408-412, eval_metrics :414-441)
 * for every split of a run as ONE launch sequence.  score [total] float64 and y [total] uint8 (non-zero = mislabelled) hold S
 * segments side by side; segs [S] says where: rows offset .. offset + n of both arrays, n >= 1, segments disjoint and inside
 * [0, total), total < 2^31.  thres_from = -1: a FREE segment -- its three thresholds are found on its own rows with
 * `prevalence` (F1_optimal: the 100-candidate sweep, the last candidate at the maximum; F1_prev: scipy's bisect on the
 * predicted prevalence, the squared-gap fminbound where bisect raises; F1_heuristic: the median local minimum of the Gaussian
 * KDE on 1 000 grid points, else the median of >= 2 maxima, else np.mean in numpy's summation order).  thres_from = t >= 0:
 * the segment is counted at the thresholds of the free segment t (before or behind it) and its record repeats them: the
 * val -> train / val / test pattern of a run is one free and one fixed segment per split.
 * out[s]: AUROC exact from integer pair counts over groups of equal scores, correctly rounded once; AUPRC = sum over groups
 * (pos_g / P) precision_g in a fixed order; (TP, FP, FN, TN) at each threshold; status 0 ok, 1 a non-finite score, 2 one class
 * only, 3 a free segment with fewer than two rows, 4 a free segment whose variance is zero (where scipy's Cholesky raises),
 * 5 a fixed segment whose free segment has a status -- the first that applies, in the order the host path raises; a status
 * concerns its own segment only (5 follows its source), and the fields of a record with a status are not meaningful.
 * kde_branch 1 median of > 1 minima, 2 the one minimum, 3 median of maxima, 4 np.mean; bisect_fallback 1 where fminbound
 * served F1_prev.  The arithmetic is csrc/eval_metrics_core.hpp: thresholds and counts equal the host path by their bits (the
 * KDE's where scipy's density separates neighbouring grid points), the device and the host twin agree bit for bit.
 * lemon_eval_metrics: every pointer is a device pointer; ws: lemon_eval_metrics_workspace_bytes(total, S, S_free) bytes with
 * S_free >= the number of free segments (for S > 1 the size comes from hipcub's segmented sort, which needs a HIP device:
 * LEMON_E_HIP without one), 256-byte aligned; nothing is allocated, every launch goes to `stream`; the call
 * waits for the stream once, to check segs before anything is launched.  Refused with LEMON_E_INVALID, nothing written: a
 * null pointer, S outside [1, 65535], total outside [1, 2^31), a segment with offset < 0 or n < 1, one that passes `total` or
 * overlaps another, a thres_from that is neither -1 nor the index of a free segment, a short or misaligned workspace.
 * lemon_eval_metrics_host: the same header with the lanes looped on the host, host pointers, std::stable_sort; for the
 * tests, no product path calls it.  lemon_eval_metrics_kde_host: test-only, the KDE of one free segment of n >= 2 host rows as
 * the twin evaluates it: grid [1000] and dens [1000]; LEMON_E_INVALID for a null pointer, n < 2, a non-finite score or zero
 * variance. */
#define LEMON_EVAL_OK 0
#define LEMON_EVAL_NONFINITE 1
#define LEMON_EVAL_ONE_CLASS 2
#define LEMON_EVAL_FEW_ROWS 3
#define LEMON_EVAL_ZERO_VARIANCE 4
#define LEMON_EVAL_SOURCE 5
typedef struct LemonEvalSegment { int64_t offset, n; double prevalence; int32_t thres_from, pad; } LemonEvalSegment;
typedef struct LemonEvalRecord {
    double auroc, auprc, thres[3];
    int64_t counts[3][4];
    int32_t status, kde_branch, bisect_fallback, pad;
} LemonEvalRecord;
int64_t lemon_eval_metrics_workspace_bytes(int64_t total, int S, int S_free); /* < 0: LEMON_E_* */
int lemon_eval_metrics(const double *score, const uint8_t *y, int64_t total, const LemonEvalSegment *segs, int S,
                       void *ws, int64_t ws_bytes, LemonEvalRecord *out, void *stream);
int lemon_eval_metrics_host(const double *score, const uint8_t *y, int64_t total, const LemonEvalSegment *segs, int S,
                            LemonEvalRecord *out);
int lemon_eval_metrics_kde_host(const double *score, int64_t n, double *grid, double *dens);

/* ---- k-means on caption embeddings + the deep-kNN label score ------------------------ */

/* FaissKMeans.predict = index.search(x, 1) (lib/datasets/clustering.py:38-41) and the assignment step of faiss.Kmeans.train
 * (:28-36): nearest centroid of every row of x_dev [n, d] among c_dev [C, d], squared L2 with the exact key of the numeric
 * contract max(0, fma(-2, <x,c>, |x|^2 + |c|^2)) (chain norms), ties to the lower index.  assign_dev int32 [n] and dist_dev
 * float32 [n] (may be NULL) equal, bit for bit, lemon_index_search(IndexFlatL2 over c, x, 1).  A dedicated kernel: no
 * workspace, no candidate lists.  1 <= C <= 16384; d a multiple of 4, 4 <= d <= 1024; x_dev and c_dev 16-byte aligned;
 * anything else is refused with LEMON_E_INVALID, never truncated. */
int lemon_kmeans_assign(const float *x_dev, int64_t n, int d, const float *c_dev, int C, int32_t *assign_dev, float *dist_dev,
                        void *stream);
/* The centroid step of faiss.Kmeans.train (clustering.py:28-36): c_dev [C, d] (in/out) = mean of the points assigned to each
 * cluster, summed in float64 in ascending point order (stable radix sort of the ids by cluster, then one serial sum per
 * cluster and coordinate: no floating-point atomics, the same bits on every run and every launch geometry) and rounded
 * once to float32; a cluster without points keeps its centroid.  count_dev int64 [C]; obj_dev double [1] (may be NULL) =
 * sum of dist_dev in float64, in a fixed order.  ws_dev: lemon_kmeans_workspace_bytes(n, d, C) bytes, 256-byte aligned. */
int lemon_kmeans_update(const float *x_dev, int64_t n, int d, const int32_t *assign_dev, const float *dist_dev, int C,
                        float *c_dev, int64_t *count_dev, double *obj_dev, void *ws_dev, int64_t ws_bytes, void *stream);
/* Empty clusters (faiss split_clusters inside Kmeans.train): for each empty cluster in ascending index the currently largest
 * cluster (ties: lower index) is the donor; the empty one takes a copy of the donor's centroid with even coordinates
 * x (1 + eps) and odd ones x (1 - eps), the donor the other way round, eps = 1/1024; the empty one gets floor(count / 2) of
 * the donor's count.  faiss draws the donor at random in proportion to its size: its RNG stream is not pinned here (faiss is
 * not available to this project's tests), the rule is otherwise faiss's. */
int lemon_kmeans_split(float *c_dev, int d, int C, int64_t *count_dev, void *stream);
/* faiss.Kmeans(d, C, niter).train(x) for ONE redo from the initial centroids in c_dev (clustering.py:28-36): enqueues niter x
 * (assign, update, split) and a last assign against the final centroids, with no host synchronisation.  obj_hist_dev double
 * [niter]: the objective of every iteration; count_dev: the last update's (after its split); assign_dev int32 [n]: the
 * final assignment.  n >= C.  Early stop on the device: after an iteration that changes no assignment and leaves no
 * cluster empty (a fixed point: the remaining iterations could not change anything) a device flag makes the kernels of the
 * remaining iterations return at once and obj_hist is filled with the last value; the host never reads the flag.
 * LEMON_KMEANS_EARLY_STOP=0 runs every iteration in full (same result). */
int lemon_kmeans_train(const float *x_dev, int64_t n, int d, int C, int niter, float *c_dev, double *obj_hist_dev,
                       int64_t *count_dev, int32_t *assign_dev, void *ws_dev, int64_t ws_bytes, void *stream);
int64_t lemon_kmeans_workspace_bytes(int64_t n, int d, int C); /* < 0: LEMON_E_* */
/* The deep-kNN score of lib/baselines/run_deepknn.py on the labels lib/datasets/dataloader.py:190-192 hands out: the
 * fraction of a query's k kept neighbours whose label differs from the query's.  I_dev int64 [nq, kk] from
 * lemon_index_search; drop_self as in lemon_neighbors (run_lemon.py:257-263: searched kk >= k + 1, drop result[0] where
 * in_db_dev[i] != 0 (NULL = all), else result[-1]); db_label_dev int32 [ntotal]; a slot with I outside [0, ntotal) counts as
 * disagreeing, a query label of -1 matches nothing.  out_dev float32 [nq]. */
int lemon_knn_label_disagreement(const int64_t *I_dev, int64_t nq, int kk, int k, int drop_self, const uint8_t *in_db_dev,
                                 const int32_t *db_label_dev, int64_t ntotal, const int32_t *q_label_dev, float *out_dev,
                                 void *stream);

/* ---- baseline JPEG files decoded on the GPU (the reference decodes every file with PIL, `Image.open(p).convert("RGB")`, in its
 * DataLoader workers: lib/datasets/dataloader.py:167-198, run_lemon.py:129-131,199-201).  The decode is split: the serial
 * Huffman pass runs on the host (lemon_jpeg_entropy), the data-parallel rest on the device (lemon_jpeg_decode); the pixels are
 * bit for bit PIL's (libjpeg-turbo: JDCT_ISLOW, fancy upsampling).  The three host functions are also exported by
 * liblemon_jpeg_host.so, which links no HIP runtime (the decode workers load that one). */
typedef struct LemonJpegInfo {
    int32_t status;                   /* 0 = accepted; > 0 = declined, decode with PIL (codes: csrc/jpeg_entropy.hpp) */
    int32_t width, height, components;
    int32_t hs, vs;                   /* sampling factors of component 0: 1x1, 2x1 or 2x2 (1x1 with one component) */
    int32_t mcus_x, mcus_y;
    int32_t max_abs;                  /* largest |coefficient * quantiser| of the image */
    int32_t exact_blocks;             /* blocks whose envelope check needed the exact form */
    int64_t blocks;                   /* 8x8 blocks of all components over the MCU-padded grid */
    int64_t record_bytes;             /* 384 + 128 * blocks */
    uint16_t quant[3][64];            /* per component, natural order */
} LemonJpegInfo;
/* Header pass of lib/datasets/dataloader.py:167-198's decode: geometry, quantisers and record size of the file in data[0, n), or
 * the reason it is declined (progressive, arithmetic, 12-bit, several scans, 16-bit tables, other sampling, 4 components, Adobe
 * marker, non-YCbCr component ids, a zero dimension, anything malformed).  Returns info->status.  Host only, no GPU. */
int lemon_jpeg_info(const uint8_t *data, int64_t n, LemonJpegInfo *info);
/* The whole host pass for the same call site (lib/datasets/dataloader.py:167-198; run_lemon.py:129-131,199-201 run it in 8
 * workers): header + Huffman decoding into `record` (info->record_bytes <= record_cap bytes: uint16 quant[3][64], then int16
 * coefficient blocks, component 0 [block row][block col][64] natural order, then components 1 and 2).  Also declines a bit
 * stream that ends early or runs past its last MCU and an image with a block outside the arithmetic envelope
 * (csrc/jpeg_entropy.hpp).  Every read of `data` is bounds-checked.  Returns info->status.  Host only, no GPU. */
int lemon_jpeg_entropy(const uint8_t *data, int64_t n, uint8_t *record, int64_t record_cap, LemonJpegInfo *info);
/* The device arithmetic of lemon_jpeg_decode run on the host (csrc/jpeg_core.hpp): record -> uint8 RGB [h, w, 3].  Test support
 * for lib/datasets/dataloader.py:167-198's pixels on a machine without a GPU; no product path calls it.  0 = ok. */
int lemon_jpeg_reconstruct_host(const uint8_t *record, int64_t record_bytes, int32_t w, int32_t h, int32_t ncomp, int32_t hs,
                                int32_t vs, uint8_t *rgb);
/* Device half for a batch (lib/datasets/dataloader.py:167-198 per image; run_lemon.py:129-131,199-201 per loader batch):
 * rec_dev holds the records (rec_bytes long, 16-byte aligned).  aux_dev (int64): [batch, 8] descriptors (record offset -- a
 * multiple of 16 --, output offset, width, height, components, hs, vs, work offset -- a multiple of 16), then [batch + 1] first
 * inverse-DCT workgroup of each image (32 blocks per workgroup; idct_blocks = the last entry), then [batch + 1] first colour
 * workgroup (1024 pixel slots of 4 pixels per row-quad, i.e. ceil(h * ceil(w / 4) / 256) per image; rgb_blocks = the last entry).
 * Two launches: dequantise + inverse DCT into uint8 component planes in work_dev (64 bytes per block), then chroma upsampling,
 * YCbCr -> RGB and the crop to w x h, written as packed uint8 RGB [h, w, 3] at each image's output offset in out_dev -- the
 * layout lemon_preprocess_ragged reads.  An image whose record, planes or pixels would not lie inside rec_bytes / work_bytes /
 * out_bytes is neither read nor written. */
int lemon_jpeg_decode(const uint8_t *rec_dev, int64_t rec_bytes, int64_t batch, const int64_t *aux_dev, int64_t idct_blocks,
                      int64_t rgb_blocks, uint8_t *work_dev, int64_t work_bytes, uint8_t *out_dev, int64_t out_bytes, void *stream);

/* ---- the Huffman pass on the device: files cross PCIe compressed.  The decode workers of lib/datasets/dataloader.py:167-198's
 * call site then only read the file, parse its markers and strip the byte stuffing (lemon_jpeg_pack); the device decodes the
 * entropy-coded segment in parallel WITHIN every image (lemon_jpeg_entropy_device; scheme and packet: csrc/jpeg_par.hpp) into the
 * records lemon_jpeg_decode reads, bit for bit what lemon_jpeg_entropy writes.  lemon_jpeg_pack and lemon_jpeg_entropy_par_host
 * are also exported by liblemon_jpeg_host.so. */
#define LEMON_JPEG_SYNC 16                /* status: the lanes' states had not settled under the round cap; decode with PIL */
#define LEMON_JPEG_PACKET_BOUND 2752      /* packet_cap = n + n / 8192 + this always suffices (n + this without restart markers) */
#define LEMON_JPEG_SUBSEQ_MIN 16          /* smallest subseq_bytes; a multiple of 4 up to 4096 */
#define LEMON_JPEG_PAR_GROUP 256          /* lanes per workgroup */
/* Host, no GPU (lib/datasets/dataloader.py:167-198, in the workers): runs lemon_jpeg_info's header pass -- and declines exactly
 * what it declines --, then writes the scan packet into packet[0, packet_cap): geometry, quantisers, the Huffman table
 * specifications and selectors, the restart interval, the entropy-coded segment with FF 00 -> FF and the restart markers
 * removed, and the byte count of every restart interval.  While copying it verifies the marker structure (fill bytes, RSTn
 * exactly where expected counting modulo 8, EOI after the last interval, no other marker): a violation is LEMON_JPEG_STREAM.
 * Every read is bounds-checked.  *packet_bytes receives the packet's size (a multiple of 16).  Returns info->status. */
int lemon_jpeg_pack(const uint8_t *data, int64_t n, uint8_t *packet, int64_t packet_cap, LemonJpegInfo *info, int64_t *packet_bytes);
/* Device Huffman pass for a batch (lib/datasets/dataloader.py:167-198 per image; run_lemon.py:129-131,199-201 per loader batch).
 * packets_dev[0, packets_bytes) holds the packets, rec_dev[0, rec_bytes) receives the records (both 16-byte aligned).  desc_dev
 * (int64 [batch, 8]): packet offset and bytes, record offset (multiples of 16), restart intervals of the packet, first workgroup,
 * first interval slot, workgroups, 0 -- where an image with scan_bytes of entropy-coded data in `intervals` intervals is given
 * ceil((ceil(scan_bytes / subseq) + intervals) / 256) workgroups; total_groups and total_intervals are the sums.  subseq_bytes:
 * bytes per lane, 0 = the default (256).  status_dev int32 [batch]: 0, a LemonJpegStatus code, LEMON_JPEG_SYNC, or
 * LEMON_JPEG_BUFFER for an image whose packet, record or workspace share would leave its buffer (neither read nor written).
 * ws_dev: lemon_jpeg_entropy_workspace_bytes(batch, total_groups, total_intervals) bytes, 16-byte aligned.  A declined image's
 * record is unspecified. */
int lemon_jpeg_entropy_device(const uint8_t *packets_dev, int64_t packets_bytes, int64_t batch, const int64_t *desc_dev,
                              int64_t total_groups, int64_t total_intervals, int32_t subseq_bytes, uint8_t *rec_dev,
                              int64_t rec_bytes, int32_t *status_dev, void *ws_dev, int64_t ws_bytes, void *stream);
int64_t lemon_jpeg_entropy_workspace_bytes(int64_t batch, int64_t total_groups, int64_t total_intervals); /* < 0: LEMON_E_* */
/* lemon_jpeg_entropy_device's algorithm with the lanes looped on the host -- the same functions, workgroups and rounds, so the
 * same record and the same status.  Test support for lib/datasets/dataloader.py:167-198's decode where there is no GPU; no
 * product path calls it.  Returns 0 unless an argument is invalid; *status as status_dev above. */
int lemon_jpeg_entropy_par_host(const uint8_t *packet, int64_t packet_bytes, int32_t subseq_bytes, uint8_t *record,
                                int64_t record_cap, int32_t *status);

/* ---- progressive JPEG files (SOF2) on the same path, opt-in: lib/datasets/dataloader.py:167-198 decodes them with PIL like any
 * other file, and web-scraped caption sets hold many.  A progressive file ends in the same coefficient record as a baseline one,
 * so lemon_jpeg_decode and lemon_jpeg_reconstruct_host read it unchanged; only the Huffman pass differs: several scans, each
 * with its own tables and restart interval (csrc/jpeg_prog.hpp, csrc/jpeg_prog_par.hpp).  lemon_jpeg_info, lemon_jpeg_entropy and
 * lemon_jpeg_pack keep declining SOF2; these accept SOF2 only (a baseline file: status 3).  The host functions are also exported
 * by liblemon_jpeg_host.so. */
#define LEMON_JPEG_PROGRESSION 17         /* status: at EOI not every coefficient was sent down to bit 0 (libjpeg would smooth) */
#define LEMON_JPEG_PROG_PACKET_BOUND 5424 /* packet_cap = n + 2 * (n / 3) + this always suffices (csrc/jpeg_prog_par.hpp) */
#define LEMON_JPEG_PROG_ITEM 16           /* restart intervals of one scan that one wave decodes */
/* Header pass of lib/datasets/dataloader.py:167-198's decode for a progressive file: markers up to the first SOS -> geometry and
 * record size, or the reason it is declined.  Returns info->status.  Host only, no GPU. */
int lemon_jpeg_prog_info(const uint8_t *data, int64_t n, LemonJpegInfo *info);
/* The whole host pass for the same call site (lib/datasets/dataloader.py:167-198): all markers and all scans of a progressive
 * file into `record` (the record of lemon_jpeg_entropy).  Declines whatever libjpeg would warn about and every file whose
 * progression is incomplete at EOI (LEMON_JPEG_PROGRESSION), see csrc/jpeg_prog.hpp; max_abs and exact_blocks as
 * lemon_jpeg_entropy.  Every read of `data` is bounds-checked.  Returns info->status.  Host only, no GPU. */
int lemon_jpeg_prog_entropy(const uint8_t *data, int64_t n, uint8_t *record, int64_t record_cap, LemonJpegInfo *info);
/* Host, no GPU (lib/datasets/dataloader.py:167-198, in the workers): all header and marker-structure checks of
 * lemon_jpeg_prog_entropy -- it declines exactly what those decline --, then the packet of csrc/jpeg_prog_par.hpp into
 * packet[0, packet_cap): geometry, quantisers, the scan table, the Huffman specifications the scans use and every scan's
 * entropy-coded bytes with FF 00 -> FF and restart markers removed.  *packet_bytes receives its size (a multiple of 16); its head
 * holds the scan, item and level counts that lemon_jpeg_prog_entropy_device's caller needs (int32 at bytes 24, 32, 36). */
int lemon_jpeg_prog_pack(const uint8_t *data, int64_t n, uint8_t *packet, int64_t packet_cap, LemonJpegInfo *info,
                         int64_t *packet_bytes);
/* Device Huffman pass for a batch of progressive packets (lib/datasets/dataloader.py:167-198 per image;
 * run_lemon.py:129-131,199-201 per loader batch).  packets_dev / rec_dev as lemon_jpeg_entropy_device.  desc_dev (int64
 * [batch, 8]): packet offset and bytes, record offset (multiples of 16), first item slot, items of the packet (its head), 0, 0, 0;
 * total_items is the sum, levels the largest level count of the packets' heads.  One wave decodes one item -- a scan's
 * LEMON_JPEG_PROG_ITEM consecutive restart intervals --, one launch per level.  status_dev int32 [batch]: 0, a LemonJpegStatus
 * code, or LEMON_JPEG_BUFFER for an image whose packet, record or item share would leave its buffer or whose scan table is
 * inconsistent (neither read further nor written).  ws_dev: lemon_jpeg_prog_entropy_workspace_bytes(batch, total_items, levels)
 * bytes, 16-byte aligned.  A declined image's record is unspecified. */
int lemon_jpeg_prog_entropy_device(const uint8_t *packets_dev, int64_t packets_bytes, int64_t batch, const int64_t *desc_dev,
                                   int64_t total_items, int32_t levels, uint8_t *rec_dev, int64_t rec_bytes, int32_t *status_dev,
                                   void *ws_dev, int64_t ws_bytes, void *stream);
int64_t lemon_jpeg_prog_entropy_workspace_bytes(int64_t batch, int64_t total_items, int32_t levels); /* < 0: LEMON_E_* */
/* lemon_jpeg_prog_entropy_device's algorithm with the waves looped on the host -- the same items, levels and step functions, so
 * the same record and status.  Test support for lib/datasets/dataloader.py:167-198's decode where there is no GPU; no product
 * path calls it.  Returns 0 unless an argument is invalid. */
int lemon_jpeg_prog_entropy_par_host(const uint8_t *packet, int64_t packet_bytes, uint8_t *record, int64_t record_cap,
                                     int32_t *status);

/* ---- PNG files on the same path, opt-in (LEMON_PNG=gpu).  lib/datasets/dataloader.py:177-184 opens a frame's down-sampled PNG
 * with `Image.open(p).convert("RGB")` for mimiccxr_caption, and lib/datasets/dataloader.py:167-198 any PNG of a file dataset.  The
 * decode is split: chunk parsing (lemon_png_info, lemon_png_idat) and the zlib inflate (Python's zlib, lemon_amd/png_host.py) run
 * in the workers; unfiltering and the expansion to RGB run on the device (lemon_png_decode).  Between them lies the record
 * (csrc/png_core.hpp): 256 x 4 palette bytes (R, G, B, 0), then the filtered scanlines as inflated, each behind its filter-type
 * byte.  The host functions are also exported by liblemon_jpeg_host.so. */
#define LEMON_PNG_FILTER 13               /* device verdict: a filter-type byte above 4 (PIL raises); RGB region unspecified */
#define LEMON_PNG_INDEX 14                /* device verdict: a palette index at or above the PLTE count; RGB region unspecified */
typedef struct LemonPngInfo {
    int32_t status;                   /* 0 = accepted so far; > 0 = declined, decode with PIL (LemonPngStatus, csrc/png_core.hpp) */
    int32_t width, height;
    int32_t colour_type;              /* 0 grey, 2 RGB, 3 palette, 4 grey + alpha, 6 RGBA */
    int32_t channels;                 /* bytes per pixel: 1, 3, 1, 2, 4 */
    int32_t plte_count;               /* PLTE entries of a palette file, else 0 */
    int32_t idat_spans;               /* IDAT chunks */
    int32_t pad;
    int64_t stride;                   /* width * channels */
    int64_t record_bytes;             /* 1024 + height * (stride + 1) */
    int64_t idat_bytes;               /* total IDAT payload */
    int64_t idat_offset;              /* file offset of the first IDAT payload (the whole stream when idat_spans == 1) */
    int64_t plte_offset;              /* file offset of the PLTE payload of a palette file, else -1 */
} LemonPngInfo;
/* Chunk walk of lib/datasets/dataloader.py:177-184's file: every read bounds-checked, every chunk's CRC-32 verified.  Accepts
 * 8-bit samples of colour type 0, 2, 3, 4 or 6, not interlaced, consecutive IDAT chunks, IEND present, no acTL; everything
 * else is declined with its own status.  Returns info->status.  Host only, no GPU. */
int lemon_png_info(const uint8_t *data, int64_t n, LemonPngInfo *info);
/* The same walk, copying the concatenated IDAT payload (the zlib stream) into out[0, cap).  Returns the bytes copied, or
 * -status for a declined file or a buffer that is too small.  Host only, no GPU. */
int64_t lemon_png_idat(const uint8_t *data, int64_t n, uint8_t *out, int64_t cap);
/* Device half for a batch (lib/datasets/dataloader.py:184 per image): rec_dev holds the records (rec_bytes long, 16-byte
 * aligned).  aux_dev (int64 [batch, 8]): record offset (a multiple of 16), height, width, colour type, PLTE count, output
 * offset, work offset (a multiple of 16), 0.  One workgroup of one wave per image: bands of 64 rows in order, inside a band a
 * diagonal wavefront (lane = row, one pixel behind the lane above; csrc/png_core.hpp), the filtered bytes and the RGB bytes
 * staged through LDS in aligned 16-byte pieces.  Writes packed uint8 RGB [h, w, 3] at each image's output offset in out_dev (grey
 * replicated, alpha dropped, palette looked up) -- the layout lemon_preprocess_ragged reads -- and status_dev int32 [batch]: 0,
 * LEMON_PNG_FILTER, LEMON_PNG_INDEX, or LEMON_PNG_BUFFER (11) for an image whose record, pixels or work share would leave
 * rec_bytes / out_bytes / work_bytes (neither read nor written).  No verdict aborts the launch.  work_dev: each image owns
 * lemon_png_decode_workspace_bytes(1, width) bytes at its work offset. */
int lemon_png_decode(const uint8_t *rec_dev, int64_t rec_bytes, int64_t batch, const int64_t *aux_dev, uint8_t *work_dev,
                     int64_t work_bytes, uint8_t *out_dev, int64_t out_bytes, int32_t *status_dev, void *stream);
/* 16 * batch + 4 * total_width rounded so that every image's share (4 * width rounded up to 16) fits; < 0: LEMON_E_* */
int64_t lemon_png_decode_workspace_bytes(int64_t batch, int64_t total_width);
/* lemon_png_decode's schedule with the lanes looped on the host -- the same step functions, so the same pixels and status.  Test
 * support for lib/datasets/dataloader.py:184's pixels where there is no GPU, and the fuzzer's target; no product path calls it.
 * Returns 0 unless an argument is invalid. */
int lemon_png_decode_host(const uint8_t *record, int64_t record_bytes, int32_t h, int32_t w, int32_t colour_type,
                          int32_t plte_count, uint8_t *rgb, int32_t *status);
/* The inflate on the device too, opt-in (LEMON_PNG=device): the workers hand over lib/datasets/dataloader.py:177-184's file as
 * its palette and its concatenated IDAT payload, still compressed, and the record is written here.  z_dev holds the zlib
 * streams (z_bytes long); aux_dev (int64 [batch, 4]): stream offset, stream length, offset of the scanlines in rec_dev (record
 * offset + 1024), and want = height * (stride + 1).  One workgroup of one wave per image (csrc/png_inflate_core.hpp): lane 0
 * walks the codes into queues of 64 tokens, the wave stages the input, builds the tables of a dynamic block, places the tokens
 * (matches read a 32 KiB window in LDS), copies stored blocks, writes the window through in aligned 16-byte pieces and sums the
 * Adler-32.  status_dev int32 [batch]: 0 for a stream that is RFC 1950 / 1951 with CM = 8, CINFO <= 7, FDICT clear, yields
 * exactly `want` bytes, ends with its final block and a matching Adler-32 and has no byte behind it -- the rule
 * lemon_amd/png_host.py::fill_record applies with zlib; LEMON_PNG_STREAM (12) otherwise (its rows are unspecified, decode the
 * file with PIL); LEMON_PNG_BUFFER (11) for an image whose stream or rows would leave z_bytes / rec_bytes (neither read nor
 * written).  No status aborts the launch.  lemon_png_decode runs next on the same stream over the same rec_dev with a status
 * array of its own; the caller takes the first non-zero of the two. */
int lemon_png_inflate(const uint8_t *z_dev, int64_t z_bytes, int64_t batch, const int64_t *aux_dev, uint8_t *rec_dev,
                      int64_t rec_bytes, int32_t *status_dev, void *stream);
/* lemon_png_inflate's schedule with the lanes looped on the host -- the same code, so the same bytes and status (0 or
 * LEMON_PNG_STREAM).  Test support for lib/datasets/dataloader.py:177-184's decode where there is no GPU; no product path calls
 * it.  Also exported by liblemon_jpeg_host.so.  Returns 0 unless an argument is invalid. */
int lemon_png_inflate_host(const uint8_t *z, int64_t n, uint8_t *rows, int64_t want, int32_t *status);

/* ---- caption tokenizers on the device, opt-in (LEMON_TOKENIZE=device): the captions cross PCIe as raw bytes and the id matrix is
 * written where the text tower reads it.  Two vocabularies: the CLIP byte-pair encoding and BERT WordPiece.  The device serves
 * the rows inside an envelope -- every byte one of {9, 10, 13, 32 .. 126}, no '&', no "<|", for WordPiece no whitespace-delimited
 * word equal to [PAD] [UNK] [CLS] [SEP] [MASK] -- on which text cleaning reduces to whitespace collapse and ASCII lower-casing
 * (csrc/tokenize_core.hpp).  Every other row gets one of the status codes below, is written as all pad_id with length 0, and is
 * the caller's to tokenise (lemon_amd/tokenizer.py: device_form); nothing here falls back and nothing is truncated silently. */
#define LEMON_TOK_NON_ASCII 1 /* a byte outside {9, 10, 13, 32 .. 126}                                                    */
#define LEMON_TOK_AMPERSAND 2 /* an '&': html.unescape may rewrite the text                                               */
#define LEMON_TOK_SPECIAL 3   /* "<|" (CLIP's special tokens), or a reserved [XXX] word of WordPiece                      */
#define LEMON_TOK_TOO_LONG 4  /* more than LEMON_TOKENIZE_MAX_BYTES bytes                                                 */
#define LEMON_TOK_WORD 5      /* a word, among those that can reach the row, of more than LEMON_TOKENIZE_MAX_WORD symbols
                                 (CLIP: bytes of the token; WordPiece: pieces of the word)                                */
#define LEMON_TOK_BUFFER 6    /* the row's offsets are not ordered or leave text_bytes: the row was not read             */
/* a row with several reasons reports LEMON_TOK_BUFFER, else LEMON_TOK_TOO_LONG, else the lowest of codes 1 .. 3 */
#define LEMON_TOKENIZE_MAX_BYTES 4096
#define LEMON_TOKENIZE_MAX_WORD 64
#define LEMON_TOKENIZE_MAX_CTX 1024
typedef struct lemon_tokenizer lemon_tokenizer_t;
/* The merges table of lib/models/simple_tokenizer.py:86-104 (SimpleTokenizer.__init__) by id: merge m joins the symbols with ids
 * left[m] and right[m] at rank[m] (lower = earlier) into the symbol with id merged[m]; the caller leaves out merges whose parts
 * or result have no id.  All ids < 65535.  The pairs go into a hash table keyed by (left, right), compared exactly, of load
 * factor <= 0.5 and probe sequences <= 64.  LEMON_E_INVALID: an id out of range, one pair given two meanings, no such table.
 * Host only, no GPU: the table is uploaded by the first lemon_tokenize, to the device current then. */
int lemon_tokenizer_create_bpe(const int32_t *left, const int32_t *right, const int32_t *rank, const int32_t *merged, int64_t n_merges,
                               int32_t sot_id, int32_t eot_id, lemon_tokenizer_t **out);
/* The vocabulary of lib/models/utils.py:72-78's tokenizer (open_clip's HFTokenizer around BERT WordPiece): token v is the bytes
 * blob[offsets[v], offsets[v + 1]) with id ids[v] < 65535.  A lookup hashes the piece and then compares it with the stored bytes,
 * so a collision cannot change an id.  lower_case and max_chars as BertTokenizer's do_lower_case and max_input_chars_per_word.
 * home_buckets: 0; a power of two restricts the home slots to that many (test hook: 2 forces collisions).  Host only, no GPU. */
int lemon_tokenizer_create_wordpiece(const uint8_t *blob, const int64_t *offsets, const int32_t *ids, int64_t n_tokens, int32_t cls_id,
                                     int32_t sep_id, int32_t unk_id, int lower_case, int max_chars, int home_buckets,
                                     lemon_tokenizer_t **out);
int lemon_tokenizer_free(lemon_tokenizer_t *tok);
/* slots and entries of the hash table and its longest probe sequence */
int lemon_tokenizer_table_info(const lemon_tokenizer_t *tok, int64_t *slots, int64_t *entries, int *max_probe);
/* The tokenizer calls of the hot path for a batch -- lib/models/chexzero_clip.py:481-493 (tokenize: pad_id 0), run_lemon.py:140-154
 * (the HF call with padding="max_length", truncation=True: pad_id = the end-of-text id) and lib/models/utils.py:72-78 (pad_id =
 * [PAD]).  Row r is text_dev[offsets_dev[r], offsets_dev[r + 1]) (offsets_dev: n + 1 entries).  ids_dev [n, ctx] int64: first
 * token, word ids, last token, pad_id; a row with more than ctx - 2 word ids keeps the first ctx - 2 and ends in the last token.
 * length_dev [n]: tokens before the padding.  status_dev [n]: 0 or a LEMON_TOK_* code.  2 <= ctx <= LEMON_TOKENIZE_MAX_CTX.  One
 * launch on `stream`, no synchronisation (the first call of a tokenizer uploads its table, synchronously); a wave per row, every
 * loop bounded: merge rounds by the symbols of a word, probes by the table's longest sequence. */
int lemon_tokenize(lemon_tokenizer_t *tok, const uint8_t *text_dev, int64_t text_bytes, const int64_t *offsets_dev, int64_t n, int ctx,
                   int32_t pad_id, int64_t *ids_dev, int32_t *length_dev, uint8_t *status_dev, void *stream);
/* lemon_tokenize's algorithm with the lanes looped on the host, on host pointers: the same functions, chunks and word groups, so
 * the same ids, lengths and statuses.  Test support for the same call sites where there is no GPU; no product path calls it. */
int lemon_tokenize_host(const lemon_tokenizer_t *tok, const uint8_t *text, int64_t text_bytes, const int64_t *offsets, int64_t n, int ctx,
                        int32_t pad_id, int64_t *ids, int32_t *length, uint8_t *status);

#ifdef __cplusplus
}
#endif
#endif /* LEMON_HIP_H */
