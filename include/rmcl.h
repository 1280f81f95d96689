/* rmcl.h - C ABI of librmcl_hip.so: the MI355X (gfx950) hot path of the RMCL training step.
 *
 * The reference (stanFurrer/Robust-Multimodal-Contrastive-Learning) is 100 % Python and has no
 * FFI; its boundary for this path is the Python protocol `vilt.modules.ViLTransformerSS`
 * (vilt/modules/vilt_module.py:20-507) + the free functions in vilt/modules/objectives.py and
 * attack/pgd_attack_vilt.py.  This header is the C boundary a maintainer binds underneath that
 * protocol (ctypes stub: INTEGRATION.md).  Each entry point names the reference code it replaces.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless noted; no entry point allocates, frees or synchronises;
 *    work is enqueued on `stream` (a hipStream_t passed as void*); the caller keeps buffers alive
 *    until the stream has drained.
 *  - return value: 0 on success, otherwise a hipError_t value or -1 (argument check);
 *    rmcl_last_error() returns the message (thread-local, host string).
 *  - dtype codes: RMCL_F32 = 0, RMCL_BF16 = 1 (raw bfloat16 bits in uint16_t).
 *  - "arena": all parameters of one encoder live in ONE flat fp32 buffer whose element offsets are
 *    given by rmcl_param_layout(); the optional low-precision shadow arena has the same offsets.
 */
#ifndef RMCL_H
#define RMCL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define RMCL_F32 0
#define RMCL_BF16 1

#define RMCL_MODE_INFER 0 /* no activations kept (momentum encoder, clean query) */
#define RMCL_MODE_DATA 1  /* keep what the data-gradient (PGD) backward needs     */
#define RMCL_MODE_FULL 2  /* keep what the weight-gradient backward needs too     */
/* OR-ed into the mode of rmcl_encoder_forward: the caller will read ONLY row 0 (the cls token) of every sample of xn - what
 * the pooler does (heads.py:17) in the contrastive objectives.  Everything behind the last block's attention is row-wise
 * (proj, LayerNorm 2, the MLP, the final LayerNorm), so it then runs on B rows instead of B * N; the other rows of xn are
 * left unwritten.  The matching rmcl_encoder_backward must be called with cls_only = 2 (dxn = the [B, D] gradient of those
 * rows): it back-propagates the compact tail and reduces the last layer's fc2 / fc1 / proj weight gradients over B rows.
 * Requires dropout off and B <= 1024.  Results equal the dense pass on the cls rows up to fp32 summation order (the tail
 * uses the fp32 master weights).                                                                                     */
#define RMCL_MODE_CLS_TAIL 16
/* OR-ed into the mode of rmcl_encoder_forward, rmcl_encoder_forward_rank and rmcl_encoder_backward (and accepted by rmcl_stash_bytes):
 * with dtype bf16, exact = 0 and N = L + 1 + P > 256 every layer's attention runs the streaming kernels (rmcl_attention_stream_fwd / _bwd
 * below) instead of the unfused score / probability matrices; the layer's `probs` stash then holds the log-sum-exp.  In every other
 * case (fp32, exact, N <= 256) the bit changes nothing.  A forward and the backward that reads its stash must agree on the bit: the
 * library remembers (host side, by address) what the last forward left in each of the 64 most recent stashes, and a backward whose
 * setting differs from it returns -1.                                                                                         */
#define RMCL_MODE_STREAM_ATTN 32

typedef struct rmcl_dims {
  int B;        /* samples in this pass                                              */
  int L;        /* text tokens per sample (max_text_len, 40)                         */
  int P;        /* image patches per sample ((384/32)^2 = 144)                       */
  int D;        /* hidden size 768                                                   */
  int H;        /* heads 12 (head dim D/H must be 64)                                */
  int layers;   /* 12                                                                */
  int mlp;      /* 3072                                                              */
  int patch_k;  /* 3*32*32 = 3072 (K of the patch-embedding GEMM)                    */
  int proj;     /* MoCo projection dim 128                                           */
  int vocab;    /* 30522                                                             */
  int dtype;    /* RMCL_F32 or RMCL_BF16: operand type of the encoder GEMMs          */
  int exact;    /* 1: force the exact-f32 matrix-core GEMM (bf16 operands widened)   */
  int Pp;       /* patches of the position table ((image_size/patch)^2 = 144); 0 = P. Differs from P for zero-padded
                   batches of smaller images, where P = selected patches per sample (rmcl_ragged)                  */
  int n_types;  /* rows of token_type_embeddings: 0 or 2 = the pre-training table; 3 = NLVR2 (vilt_module.py:193-231: rows
                   [old0, old1, old1] after the resize).  Only 3 changes the arena layout (3 D elements for vtype)          */
  int img_type; /* token-type row added to every image token (vilt_module.py:315-321 image_token_type_idx): 0 or 1 = row 1;
                   2 = row 2 (n_types 3); -1 = per PAIR (n_types 3, B even): sample b gets row 1 + (b & 1) - the NLVR2 pair
                   pass with image_0[i] at sample 2i and image_1[i] at 2i + 1.  In FULL mode the token-type gradient of
                   the image tokens lands in the row(s) used                                                                 */
} rmcl_dims;

/* Zero-padded batch of smaller images (VisionTransformer.visual_embed, vision_transformer.py:559-677): `patches` then
 * holds the P SELECTED patches of every sample (rmcl_patch_select + rmcl_im2patch_sel; pad slots are zero rows, which the
 * key mask drops like the reference's), and the position embedding of a sample is the G0 x G0 table resized to its (h, w).
 * All arrays are device pointers owned by the caller.                                                              */
typedef struct rmcl_ragged {
  const int32_t* sel;      /* [B, sel_ld] flat patch index (row * gw + col) of every selected slot                   */
  const int32_t* counts;   /* [B] valid slots per sample (slots >= counts[b] are pads)                              */
  const int32_t* hw;       /* [B, 2] valid patch rows / columns of every sample (x_h, x_w)                           */
  int sel_ld;              /* row pitch of sel                                                                        */
  int gw;                  /* patch columns of the padded batch (Wmax / patch)                                       */
  int G0;                  /* side of the position table (12)                                                         */
  float* pos_tok;          /* scratch [B, P+1, D] f32: resized position rows (forward writes, every pass)            */
  float* dpos_tok;         /* scratch [B, P+1, D] f32: their gradient (backward, mode FULL)                          */
} rmcl_ragged;

/* LayerNorm folded into the GEMM that consumes it (forward passes that keep no LayerNorm output: INFER and DATA mode, bf16,
 * dropout off): y = LN(x) W^T + b = rstd * (bf16(x) W'^T - mean * s) + c.  rmcl_ln_fold derives, from an fp32 arena,
 *   wf [layers][3D + mlp][D] bf16 : W' = W * gamma for qkv (norm1) then fc1 (norm2)
 *   sc [layers][2][3D + mlp] f32  : s = row sums of W', c = W beta + bias
 * and must be re-run whenever that arena changes (optimizer step, momentum update, checkpoint load).  Passing the pair to
 * rmcl_encoder_forward removes the 2 LayerNorm launches per layer (the producer GEMMs emit the bf16 copy of the residual
 * stream and per-row partial sums in their epilogues); NULL keeps the separate LayerNorm kernels.  The fold is taken only where
 * all four GEMMs of a layer run on the bf16 192-row tile kernels: D % 192 == 0 and a routing that sends them there (automatic at the
 * step's shapes, rmcl_tune_set key 0 = 60 at any).  Every other pass given the pair runs the separate LayerNorm kernels, bit for bit
 * the pass without it: for such an encoder (D % 192 != 0) building the pair with rmcl_ln_fold is wasted work.             */
typedef struct rmcl_fold {
  const void* wf;
  const float* sc;
} rmcl_fold;
int64_t rmcl_ln_fold_elems(const rmcl_dims* d, int which);   /* which = 0: elements of wf (bf16), 1: elements of sc (f32) */
int rmcl_ln_fold(const rmcl_dims* d, const float* params32, void* wf, float* sc, void* stream);

/* Transposed bf16 shadows of qkv / proj / fc1 / fc2 of every layer (same offsets as params_lp, each matrix stored
 * [in][out]): optional operand of rmcl_encoder_backward - the data-gradient GEMMs then read k-contiguous rows.  Re-run after
 * every change of params_lp.                                                                                         */
int rmcl_weight_transpose_bf16(const rmcl_dims* d, const void* params_lp, void* params_lpT, void* stream);

/* The two GEMM forms of the fold as single operators (the encoder pass uses them internally; exported for tests / reuse).
 * rmcl_linear_rowstat: out[M,N] f32 = A[M,K] W[N,K]^T + bias + residual, plus out_bf16 (same values) and, per row, 4 partial
 *   (sum, sum of squares) per 192 output columns: part[M][4*N/192][2].  N % 192 == 0; 192-row-tile shapes only.
 * rmcl_linear_lnfold: out[M,N] bf16 = act( rstd_m * (xb[M,K] wf[N,K]^T - mean_m * s_n) + c_n ), mean / rstd from `part`
 *   ([M][nparts][2], sums over K_ln = 768... columns); preact (optional, bf16) receives the value before the GELU.
 * Both return an error when the shape would not run on the 192-row tile kernels (no fallback).                      */
int rmcl_linear_rowstat(const void* A, const void* W, const float* bias, const float* residual, float* out, void* out_bf16, float* part,
                        int M, int N, int K, void* stream);
int rmcl_linear_lnfold(const void* xb, const void* wf, const float* s, const float* c, const float* part, int nparts, void* out,
                       void* preact, int M, int N, int K, int gelu, float eps, float* mean, float* rstd, void* stream);
/* The SHIFT-ROBUST pair (round 4; what the encoder passes run).  LayerNorm is shift-invariant, LN(x) = LN(x - c) for any per-row c:
 * with `center` [M] the producer stores out_bf16 = bf16(out - c_m) and the partial sums of (out - c_m), so the bf16 operand's rounding
 * follows the row's spread instead of its offset (a trained checkpoint's residual stream is not zero-mean; reference norms:
 * vision_transformer.py:351,362); the consumer's arithmetic is unchanged and it adds c_m back to the `mean` it writes.  The encoder
 * uses c = the row mean of the row's previous LayerNorm, which already sits in the stash.  center = NULL: the two functions above.  */
int rmcl_linear_rowstat_c(const void* A, const void* W, const float* bias, const float* residual, const float* center, float* out,
                          void* out_bf16, float* part, int M, int N, int K, void* stream);
int rmcl_linear_lnfold_c(const void* xb, const void* wf, const float* s, const float* c, const float* part, int nparts, const float* center,
                         void* out, void* preact, int M, int N, int K, int gelu, float eps, float* mean, float* rstd, void* stream);

/* PROTOTYPE (round 4): up to four bf16 GEMMs out[M,N_i] = epi(A_i[M,K_i] W_i[N_i,K_i]^T ...) of one activation row tile chained inside
 * ONE launch - the row-wise part of an encoder layer between two attention calls (reference op chain: vision_transformer.py:279-285
 * Mlp, :330-331 proj, :371-375 Block).  Stage i + 1 reads what stage i wrote (its A / residual pointers name stage i's outputs); groups
 * of four workgroups on one XCD carry a 191-row tile through all stages and synchronise through `tickets` (4 * 64 + 1 uint32, zeroed
 * once by the caller; `epoch` = 1, 2, 3, ... counts the launches made with that buffer).  epi: EPI_BIAS [| EPI_GELU | EPI_SAVE_PREACT]
 * (bf16 output), EPI_BIAS | EPI_RESIDUAL | EPI_ROWSTAT (fp32 output + bf16 copy `out2` + row partials `part`), EPI_LNFOLD (as
 * rmcl_linear_lnfold_c).  flags bit 0: placement-independent hand-off (agent-scope release per stage); 0 relies on the four blocks
 * b, b + 8, b + 16, b + 24 sharing an XCD - check with `xcc` ([grid] int32, optional).  stamps: optional [4][4] int64 wall-clock stamps of
 * block `stamp_wg`.  Measured against separate launches in tools/chain_bench.py; not used by the encoder passes.   */
typedef struct rmcl_chain_stage {
  const void* A; const void* W; const float* bias; const float* residual; void* out; void* out2; float* part; const float* center;
  const float* ln_s; const float* ln_c; float* mean; float* rstd;
  int N, K, epi, nparts; float ln_eps;
} rmcl_chain_stage;
int rmcl_gemm_chain(const rmcl_chain_stage* stages, int n, int M, uint32_t* tickets, uint32_t epoch, int flags, int32_t* xcc, int64_t* stamps,
                    int stamp_wg, void* stream);

/* EXPERIMENT (round 4, tools/l2_prefetch_bench.py): an L2 prefetch agent beside a 192-row-tile GEMM C[M,N] = A[M,K] W[N,K]^T - `wgs`
 * single-wave workgroups, of which the first `per_xcd` to arrive on each XCD (hardware XCC_ID; `counter`: 8 int32 zeroed by the caller) pull
 * one dword of every 128-byte line of the k-tiles the XCD's GEMM workgroups are about to stream (A rows of its row panels: tile ids
 * xcd * tiles_per_xcd ..., `col_tiles` column tiles per row panel; all nB rows of W), `lead` k-tiles ahead of a clock-paced schedule of
 * `tick` 10-ns ticks per k-tile.  Nothing is written but `stamps` ([8][2] int64 start / end wall clock, optional).  Not used by the
 * encoder passes; DESIGN.md section 3 records what it measured.                                                                        */
int rmcl_l2_prefetch_experiment(const void* A, int64_t lda_bytes, int M, int rows_per_tile, int tiles_per_xcd, int col_tiles, const void* W,
                                int64_t ldw_bytes, int nB, int nk, int tick, int lead, int per_xcd, int wgs, int* counter, int64_t* stamps,
                                void* stream);

/* Element offsets into a parameter arena.  Names follow the reference state dict. */
typedef struct rmcl_layout {
  int64_t word, pos, btype, eln_w, eln_b;      /* text_embeddings.{word,position,token_type}_embeddings, LayerNorm */
  int64_t vtype;                               /* token_type_embeddings.weight [2,D] ([3,D] when n_types == 3)     */
  int64_t cls, pos_img, patch_w, patch_b;      /* transformer.{cls_token,pos_embed,patch_embed.proj.*}             */
  int64_t layer0, layer_stride;                /* transformer.blocks.<i> base = layer0 + i*layer_stride            */
  int64_t ln1_w, ln1_b, qkv_w, qkv_b, proj_w, proj_b, ln2_w, ln2_b, fc1_w, fc1_b, fc2_w, fc2_b; /* rel. to block */
  int64_t norm_w, norm_b;                      /* transformer.norm                                                 */
  int64_t mh0_w, mh0_b, mh1_w, mh1_b, mh3_w;   /* moco_head.projector.{0,1,3}                                      */
  int64_t ema_end;                             /* [0, ema_end) is the range the momentum update covers             */
  int64_t pool_w, pool_b;                      /* pooler.dense (query side only; vilt_module.py:405)               */
  int64_t itm_w, itm_b;                        /* itm_score.fc                                                     */
  int64_t total;
} rmcl_layout;

const char* rmcl_last_error(void);
int rmcl_version(void);

/* In-stream timing of one class of GEMM launches (tag mask: csrc/gemm.h GEMM_TAG_*) with hipEvents
 * recorded around each launch on the launch stream; used by bench.py for the roofline object.
 * rmcl_prof_end synchronises the recorded events and returns total ms, launches and algorithmic FLOPs. */
/* Tuning knobs (developer use).  key 0: bf16 GEMM tile/pipeline configuration (-1 = automatic).
 * key 1: number of CUs the persistent activation GEMMs leave to other kernels (default 8, so that RCCL's
 * channel workgroups and small side-stream kernels do not displace GEMM workgroups - at M = 64*185 the 62 x {4,12,16} tiles
 * are whole multiples of a 248-workgroup grid, so this costs nothing).
 * Further keys (csrc/api.cpp rmcl_tune_set has the list): 2 two-kernel attention backward, 3 per-GEMM weight gradients, 4 waves of the attention
 * forward, 5 InfoNCE form, 6 skinny-GEMM form (below), 7 gemm_dp stagger, 8 / 9 attention-backward experiments, 10 chains sharing the chip (half-batch
 * lanes), 11 (round 4) 0 = the UNCENTRED LayerNorm fold of round 2, 12 / 13 (round 4) stash prefetch of the backward: buffer mask / touch
 * workgroups - measured negative, 0 by default, 14 residual GEMMs: 0 = the fp32 residual through registers only, 15 the MLP pre-activation
 * stash: 1 (default) = in tile order wherever both GEMMs that touch it run on the 192x384 kernel (EPI_PREACT_TILED below), 0 = row-major
 * in every pass (A/B runs, bit-comparison tests).  These are process-global: callers that change one around a region restore it in a finally
 * block (attack/pgd_attack_vilt.py, vilt/modules/objectives.py).
 * key 6, the skinny fp32 GEMMs (M <= 1024 rows, csrc/gemm_exact.hip): 0 = the row-split kernel only; 1 = the k-split kernel wherever
 * K % 64 == 0 and K >= 128; -1 (default) or 2 = for N < 4096 the STREAMING k-split kernel - the same arithmetic bit for bit, with the weight
 * loads of a wave's whole K chunk issued before its first MFMA and 1, 2 or 4 row tiles per workgroup, chosen from M and from the share of
 * key 10 - and the k-split kernel's 32-column form for N >= 4096.  1 is the A/B arm and the bitwise reference of the default.              */
int rmcl_tune_set(int key, int value);

/* Optional second HIP stream: the weight-gradient GEMMs of rmcl_encoder_backward (mode FULL, bf16) then run
 * concurrently with the data-gradient chain, fork/joined with events on `stream`.  NULL disables it.     */
/* Data-parallel overlap: make `stream` wait until the gradients of encoder layer `layer` written by the most recently
 * enqueued weight-gradient backward (rmcl_encoder_backward, full mode) are complete - the bucket of that layer can then be
 * all-reduced while the backward of the layers below is still running (replaces DistributedDataParallel's bucket hooks,
 * run.py:96 / pytorch_lightning ddp).  Layers finish in the order layers-1 .. 0.                                        */
int rmcl_grad_ready_wait(int layer, void* stream);
int rmcl_set_side_stream(void* stream);
/* Stream of the stash prefetch (round 4, rmcl_tune_set(12, mask) != 0): rmcl_encoder_backward touches layer l - 1's cold stash buffers into
 * the Infinity Cache from a few workgroups on this stream while layer l's backward chain runs.  NULL / never set: no prefetch.            */
int rmcl_set_prefetch_stream(void* stream);

/* Test hook: x[i] *= dropout_mask(site seed of (drop_seed, layer, site), i), i < n (x pre-filled with ones gives the mask).
 * sites: 0 proj, 1 mlp hidden, 2 fc2, 3 text embeddings, 4 image embeddings (layer 0 for the last two).   */
int rmcl_dropout_mask_apply(float* x, int64_t n, uint32_t drop_seed, int layer, int site, float drop_p, void* stream);

int rmcl_prof_begin(int tag_mask, int max_launches);
int rmcl_prof_end(double* ms_total, int64_t* launches, double* flops_total);

void rmcl_param_layout(const rmcl_dims* d, rmcl_layout* out);
int64_t rmcl_stash_bytes(const rmcl_dims* d, int mode);
int64_t rmcl_workspace_bytes(const rmcl_dims* d);
int64_t rmcl_heads_stash_bytes(const rmcl_dims* d);

/* ---- path-level entry points --------------------------------------------------------------- */

/* image [B,3,Hh,Ww] f32 -> patch rows [B*(Hh/ps)*(Ww/ps), 3*ps*ps] f32 (to_image=0) or back (1).
 * GEMM view of PatchEmbed's Conv2d (vilt/modules/vision_transformer.py:397-409).                */
int rmcl_im2patch_f32(const float* img, float* patches, int B, int C, int Hh, int Ww, int ps, int to_image, void* stream);

/* Patch geometry of a zero-padded batch [B,C,Hh,Ww] (vision_transformer.py:563-567,605-651): per sample the selection list
 * sel[b, :] (valid patches row-major, then the first non-valid patch repeated; pitch (Hh/ps)*(Ww/ps)), counts[b] valid
 * patches and hw[b] = (x_h, x_w).  The caller picks n = min(max counts, max_image_len) and, for a sample with MORE than n
 * valid patches, overwrites its row with a random subset like the reference's multinomial draw.                      */
int rmcl_patch_select(const float* img, int B, int C, int Hh, int Ww, int ps, int32_t* sel, int32_t* counts, int32_t* hw, void* stream);
/* image <-> compact rows [B*n, C*ps*ps] of the selected patches (pad slots: zero rows / not written back; to_image=1 zeroes
 * the image first).                                                                                                  */
int rmcl_im2patch_sel(float* img, float* patches, const int32_t* sel, const int32_t* counts, int sel_ld, int B, int n, int C, int Hh,
                      int Ww, int ps, int to_image, void* stream);
/* Feed path (row f3): a decoded batch as BYTES - uint8 [B, Hmax, Wmax, 3] (HWC, every sample in its top-left corner, sizes[b] = its
 * (h, w), multiples of 32) -> normalised fp32 patch rows [B*n, 3*32*32]: ToTensor + Normalize(.5, .5) (transforms/pixelbert.py:9-17)
 * through the 256-entry table `lut`, the exact zeros of the collate padding (datasets/base_dataset.py:192-206) outside a sample,
 * and the patch cut of rmcl_im2patch_f32 / rmcl_im2patch_sel, in one pass.  sel / counts: selection of rmcl_patch_select (NULL, NULL:
 * the whole grid in row-major order, n = grid size).                                                                              */
int rmcl_image_u8_to_patches(const uint8_t* img, const int32_t* sizes, const int32_t* sel, const int32_t* counts, int sel_ld, int B, int n,
                             int Hmax, int Wmax, int patch_size, const float* lut, float* patches, void* stream);

/* MinMaxResize on the device (reference: vilt/transforms/utils.py:5-26 -> PIL Image.resize(size, BICUBIC), called from
 * transforms/pixelbert.py:9-18 in every loader worker).  src: decoded bytes of a batch, uint8 [B, Hs, Ws, 3], every sample in its top-left
 * corner, src_sizes [B,2] = (h, w) per sample; dst: uint8 [B, Hd, Wd, 3] with dst_sizes [B,2] (multiples of 32: min_max_resize_size), zero
 * outside a sample - exactly the batch rmcl_image_u8_to_patches takes; tmp: uint8 [B, Hs, Wd, 3] scratch.  The integer tables are PIL's
 * (Pillow src/libImaging/Resample.c precompute_coeffs / normalize_coeffs_8bpc, built by vilt/transforms/resample.py): hbounds [B, Wd, 2] =
 * (first source column, taps) and hk [B, Wd, ksh] = 22-bit fixed-point weights per output column, vbounds [B, Hd, 2] / vk [B, Hd, ksv]
 * per output row.  Integer arithmetic throughout: the output bytes equal PIL's (tests/test_feed_gpu.py).                                  */
int rmcl_image_resize_u8(const uint8_t* src, const int32_t* src_sizes, int B, int Hs, int Ws, const int32_t* dst_sizes, int Hd, int Wd,
                         const int32_t* hbounds, const int32_t* hk, int ksh, const int32_t* vbounds, const int32_t* vk, int ksv, uint8_t* tmp,
                         uint8_t* dst, void* stream);

/* RandAugment on the device (reference: vilt/transforms/randaug.py RandAugment(2, 9), inserted in front of MinMaxResize by
 * transforms/pixelbert.py:20-30 and run with PIL in every loader worker).  src: decoded bytes of a batch, uint8 [B, Hs, Ws, 3], every sample
 * in its top-left corner, sizes [B,2] = (h, w) per sample - the batch rmcl_image_resize_u8 takes, which this call precedes.  Sample b runs
 * the n_ops operations ops[b, 0 .. n_ops) in turn, each on its own h x w rectangle (histogram, mean, rotation centre, borders); dst: uint8
 * [B, Hs, Ws, 3], zero outside a sample; tmp: same-sized scratch (the stages ping-pong src -> tmp -> dst); scratch: rmcl_randaug_scratch_bytes
 * bytes.  The op codes are the positions in the reference's augment_list().  params[b, s, :]: for Rotate, ShearX, ShearY and the translations
 * the six coefficients (a, b, c, d, e, f) of PIL's affine transform - output (x, y) reads source (a x + b y + c, d x + e y + f); Rotate's as
 * Image.rotate computes them in Python doubles -, for the other ops params[b, s, 0] = factor / threshold / bits / addition
 * (vilt/transforms/randaug.py plan_params).  The arithmetic is PIL's (16.16 fixed point, doubles, or unfused C float, as PIL has it): the
 * output bytes equal PIL's (tests/test_randaug_gpu.py).
 * ops and params are HOST arrays - the argument check reads the op codes -, copied to the device on `stream`: like every buffer they stay
 * alive until the stream has drained.  Returns -1 before any launch for a NULL operand, dst or tmp overlapping src (or each other), an op
 * code outside 0..13 or n_ops outside 1..RMCL_RA_MAX_OPS.                                                                              */
#define RMCL_RA_AUTOCONTRAST 0
#define RMCL_RA_EQUALIZE 1
#define RMCL_RA_ROTATE 2
#define RMCL_RA_POSTERIZE 3
#define RMCL_RA_SOLARIZE 4
#define RMCL_RA_SOLARIZE_ADD 5
#define RMCL_RA_COLOR 6
#define RMCL_RA_CONTRAST 7
#define RMCL_RA_BRIGHTNESS 8
#define RMCL_RA_SHARPNESS 9
#define RMCL_RA_SHEAR_X 10
#define RMCL_RA_SHEAR_Y 11
#define RMCL_RA_TRANSLATE_X 12
#define RMCL_RA_TRANSLATE_Y 13
#define RMCL_RA_MAX_OPS 8
int64_t rmcl_randaug_scratch_bytes(int B, int n_ops);
int rmcl_randaug_u8(const uint8_t* src, const int32_t* sizes, int B, int Hs, int Ws, const int32_t* ops, const double* params, int n_ops,
                    uint8_t* tmp, void* scratch, uint8_t* dst, void* stream);

/* Owner-side sum of a direct reduce-scatter over the xGMI links (replaces the reduction DDP's all-reduce performs inside the
 * collective, run.py:96): pieces [n_pieces][piece_elems] of `dtype` (F32 or BF16), this rank's slice as every rank sent
 * it; out32 = their sum (fp32 accumulation, rank order); out_wire (may be NULL) = the sum rounded to `dtype`, the operand
 * of the all-gather that follows.  piece_elems % 4 == 0.                                                            */
int rmcl_shard_sum(const void* pieces, int dtype, int n_pieces, int64_t piece_elems, float* out32, void* out_wire, void* stream);

/* out[dtype] = a + d1 + d2 (d1/d2 may be NULL): `img_init + img_delta` (attack/pgd_attack_vilt.py:144)
 * and the attacked view of objectives.py:176, fused with the cast to the GEMM operand type.      */
int rmcl_add_cast_f32(const float* a, const float* d1, const float* d2, void* out, int dtype, int64_t n, void* stream);

/* ---- Barlow-Twins variant ---------------------------------------------------------------------------
 * BarlowTwinsHead (vilt/modules/heads.py:88-107; built with [8192, 8192], 8192 at vilt_module.py:115): Linear(D,H1) -
 * BatchNorm1d - ReLU - Linear(H1,H2) - BatchNorm1d - ReLU - Linear(H2,H3) (no biases), then BatchNorm1d(H3, affine=False).
 * w1..w3, g1/b1, g2/b2: element offsets of the weights and the BatchNorm gamma/beta in ONE fp32 arena (parameters and, at
 * the same offsets, gradients).  All head arithmetic is fp32.                                                          */
typedef struct rmcl_bt_head {
  int32_t D, H1, H2, H3;
  int64_t w1, g1, b1, w2, g2, b2, w3;
} rmcl_bt_head;
int64_t rmcl_bt_stash_floats(const rmcl_bt_head* h, int B);
/* z [B,H3] = head(cls_feats [B,D]).  training != 0: batch statistics (and, when `running` is given, the running estimates
 * [mean1,var1,mean2,var2,mean3,var3] are updated with `momentum`, unbiased variance - nn.BatchNorm1d); training == 0:
 * normalise with `running`.  `stash` (rmcl_bt_stash_floats) keeps what rmcl_bt_head_backward needs.                  */
int rmcl_bt_head_forward(const rmcl_bt_head* h, const float* params, const float* cls_feats, int B, int training, float* running,
                         float momentum, float* stash, float* z, void* stream);
/* dcls [B,D] = d loss / d cls_feats given dz [B,H3]; G != NULL: weight / gamma / beta gradients are ACCUMULATED into G at the
 * head's offsets (NULL: data gradient only - the PGD inner loop, attack/pgd_attack_vilt.py:205-222).                     */
int rmcl_bt_head_backward(const rmcl_bt_head* h, const float* params, float* stash, const float* dz, int B, int training, float* G,
                          float* dcls, void* stream);
/* Cross-correlation loss of compute_barlowtwins_contrastive (vilt/modules/objectives.py:476-484, PGD form
 * attack/pgd_attack_vilt.py:219-224), in three steps so the caller can all-reduce c between the first two (:480):
 *   rmcl_bt_corr: c [N,N] = zq^T zk * inv_bs;
 *   rmcl_bt_loss: loss2 = (sum_i (c_ii - 1)^2, sum_{i != j} c_ij^2) and, IN PLACE, c <- grad_scale * d(on + lambda off)/dc;
 *                 ws: rmcl_bt_loss_ws_floats(N) floats;
 *   rmcl_bt_dz:   dzq [B,N] = zk G^T * inv_bs with G the matrix rmcl_bt_loss left in c.                                */
int rmcl_bt_corr(const float* zq, const float* zk, int B, int N, float inv_bs, float* c, void* stream);
int64_t rmcl_bt_loss_ws_floats(int N);
int rmcl_bt_loss(float* c, int N, float lambda, float grad_scale, float* ws, float* loss2, void* stream);
int rmcl_bt_dz(const float* zk, const float* G, int B, int N, float inv_bs, float* dzq, void* stream);
/* rows [B,3] = (||q_b - k_b||, cosine(q_b, k_b) eps 1e-6, q_b . k_b): the distance logs of objectives.py:496-498 */
int rmcl_bt_pair_metrics(const float* q, const float* k, int B, int N, float* rows, void* stream);

/* ---- VQAv2 fine-tuning head ------------------------------------------------------------------------------------------
 * vqa_classifier (vilt_module.py:164-172): Linear(D,H) - LayerNorm(H, eps 1e-5) - GELU (exact erf) - Linear(H,N), H = 2D,
 * N = vqav2_label_size (3129).  w0 [H,D], b0 [H], g1 / b1 [H] (LayerNorm), w3 [N,H], b3 [N]: element offsets in ONE fp32 arena
 * (parameters and, at the same offsets, gradients).  The arena keeps ldl rows for w3: rows N..ldl-1 are zero padding.
 * ldl: pitch of the logits / dz rows, a multiple of 64 >= N (3136).  D % 16 == 0, H in {512, 768, 1024, 1536, 2048}, N <= 4096,
 * 1 <= B <= 256.  All head arithmetic is fp32; nothing uses float atomics (two identical calls give identical bits). */
typedef struct rmcl_vqa_head {
  int32_t D, H, N, ldl;
  int64_t w0, b0, g1, b1, w3, b3;
} rmcl_vqa_head;
int64_t rmcl_vqa_stash_floats(const rmcl_vqa_head* h, int B);
/* logits [B, ldl] (columns N..ldl-1 not written) = vqa_classifier(cls [B,D]); `stash` (rmcl_vqa_stash_floats) keeps what
 * rmcl_vqa_head_backward needs (a copy of cls, the pre-LayerNorm rows, the GELU output, the row statistics).            */
int rmcl_vqa_head_forward(const rmcl_vqa_head* h, const float* params, const float* cls, int B, float* stash, float* logits, void* stream);
/* Soft-target BCE of compute_vqa (objectives.py:871-884) on logits [B, ldl] with SPARSE targets: labels [B,A] int32 (-1 = pad),
 * scores [B,A]; target[b, labels[b,a]] = scores[b,a] in list order (a repeated label keeps its last score).  Per row:
 * rows[b] = (sum_c max(z,0) - z t + log1p(exp(-|z|)), t[argmax]), argmax[b] = first maximum over the N classes.
 * loss2 = (sum_b rows[b][0] / B, sum_b rows[b][1] / B): BCE mean x N (the reference's loss) and VQAScore / B.
 * dz != NULL: dz [B, ldl] = grad_scale s (sigmoid(z) - t) / B, pad columns 0, s = *grad_scale_dev (a device scalar: the
 * incoming gradient of the loss inside a backward, read on the device) or 1 when grad_scale_dev is NULL.  dz == NULL: evaluation. */
int rmcl_vqa_bce(const float* logits, int ldl, const int32_t* labels, const float* scores, int A, int B, int N, float grad_scale,
                 const float* grad_scale_dev, float* dz, float* rows, int32_t* argmax, float* loss2, void* stream);
/* out [B, ldo] (N columns written): the dense target matrix of the same label / score tables. */
int rmcl_vqa_targets_dense(const int32_t* labels, const float* scores, int A, int B, int N, float* out, int ldo, void* stream);
/* dcls [B,D] = d loss / d cls given dz [B, ldl]; G != NULL: weight / bias / LayerNorm gradients are ACCUMULATED into G at the head's
 * offsets (NULL: data gradient only - the PGD inner loop, attack/pgd_attack_vilt.py:448-466).                          */
int rmcl_vqa_head_backward(const rmcl_vqa_head* h, const float* params, float* stash, const float* dz, int B, float* G, float* dcls,
                           void* stream);

/* ---- NLVR2 fine-tuning ------------------------------------------------------------------------------------------------
 * nlvr2_classifier (vilt_module.py:193-200): Linear(2D,2D) - LayerNorm(2D) - GELU - Linear(2D,2) is the VQA head above with
 * D = H = 2 * hidden, N = 2, ldl = 64 (rmcl_vqa_head_forward / _backward on an rmcl_vqa_head describing it).  Its input is the
 * pair pass's pooled cls [2B, hidden] read as [B, 2 hidden] (image_0's cls, then image_1's: sample 2i / 2i + 1).
 * Hard-label softmax cross-entropy of compute_nlvr2 / compute_nlvr2_attack / PGDAttack_nlvr2 (objectives.py:898-1060,
 * pgd_attack_vilt.py:285-300) on logits [B, ldl] (N columns used), labels [B] int32 in [0, N) (the kernel clamps a label outside into
 * [0, N): callers validate on the host).  One wave per row, one workgroup, no float atomics: two identical
 * calls give identical bits.  Outputs:
 *   rows [B]      per-row loss  lse(z) - z[label]
 *   argmax [B]    first maximum of the row
 *   stats [3]     (mean loss, rows with argmax == label, rows whose argmax differs from logits_ref's - 0 when logits_ref is NULL)
 *   dz (optional) [B, ldl] = grad_scale * s * (softmax(z) - onehot) / B, pad columns 0, s = *grad_scale_dev or 1 when NULL.
 * logits_ref (optional): a second logits buffer [B, ld_ref] - the changed-argmax count of change_rate_cross (my_metrics.py:30-45).
 * 1 <= N <= 64, N <= ldl, 1 <= B <= 65536.                                                                                 */
int rmcl_nlvr2_ce(const float* logits, int ldl, const int32_t* labels, int B, int N, float grad_scale, const float* grad_scale_dev,
                  float* dz, float* rows, int32_t* argmax, const float* logits_ref, int ld_ref, float* stats, void* stream);

/* ---- Masked language modelling (task_mlm_itm) ---------------------------------------------------------------------------
 * mlm_score (heads.py:183-195, vilt_module.py:56): transform = Linear(D,D) - GELU (exact erf) - LayerNorm(D, eps 1e-12), then
 * decoder = Linear(D, V, no bias) + bias [V]; loss = cross_entropy over the rows whose label is not -100 (objectives.py:604-630).
 * tw [D,D], tb [D], lg / lb [D] (LayerNorm), dw [V,D] (decoder.weight, NOT tied to the word embeddings), db [V] (mlm_score.bias):
 * element offsets in ONE fp32 arena (parameters and, at the same offsets, gradients).  D in {256, 768}.
 * The training path runs on the COMPACTED rows with a label and never holds a [rows, V] logits tensor; `rows` below is the launch
 * extent of the compacted buffers: a multiple of 128 that is >= the number n of rows with a label (n itself stays on the device).
 * dtype: operand type of the decoder products - RMCL_BF16 (h in bf16, W = the bf16 shadow arena params_lp at the same offset) or
 * RMCL_F32 (fp32 operands, params_lp may be NULL); accumulation and the softmax statistics are fp32; the transform is exact fp32.
 * Nothing here uses float atomics: every output has one owner and a fixed summation order (two identical calls: identical bits). */
typedef struct rmcl_mlm_head {
  int32_t D, V;
  int64_t tw, tb, lg, lb, dw, db;
} rmcl_mlm_head;
/* floats of the workspace `ws` shared by forward / backward / logits for this launch extent (monotone in rows) */
int64_t rmcl_mlm_ws_floats(const rmcl_mlm_head* h, int rows);
/* labels [M = B L] int64 -> idx [M] int32: row b * N + l of xn [B N, D] for the j-th position (ascending) whose label lies in [0, V);
 * lab [M] its label; count [1] = n.  Entries behind n: idx -1, lab -100.  Any other label (-100, or outside [0, V): callers validate
 * on the host) is skipped.  all_rows = 1: every position is listed (the dense-logits pass), lab keeps -100 where there is no label. */
int rmcl_mlm_compact(const int64_t* labels, int M, int L, int N, int V, int all_rows, int32_t* idx, int32_t* lab, int32_t* count, void* stream);
/* WT [D, ldv] in `dtype` = decoder.weight^T of the fp32 masters, ldv = V rounded up to 128 (pad columns zero): the operand of dh = dz W */
int rmcl_mlm_weight_transpose(const rmcl_mlm_head* h, const float* params, void* WT, int dtype, void* stream);
/* gather xn[idx] -> transform -> fused decoder + cross-entropy.  Per compacted row r < n: lse[r], rowloss[r] = lse - z[label], argmax[r]
 * (first maximum); rows >= n: 0 / 0 / -1.  stats [3] = (sum rowloss / n, rows with argmax == label, n); n = 0 gives a NaN loss like
 * F.cross_entropy over an all-ignored batch.  `ws` keeps what the backward / the logits writer need. */
int rmcl_mlm_forward(const rmcl_mlm_head* h, const float* params, const void* params_lp, int dtype, const float* xn, const int32_t* idx,
                     const int32_t* lab, const int32_t* count, int rows, float* ws, float* lse, float* rowloss, int32_t* argmax, float* stats,
                     void* stream);
/* dz = grad_scale s (softmax(z) - onehot) / n recomputed from ws and lse (s = *grad_scale_dev, the incoming gradient read on the device,
 * or 1 when NULL); G != NULL: every head gradient is ACCUMULATED into G at the head's offsets; dxn != NULL: the gradient of the gathered
 * rows is stored to dxn[idx[r]] (dxn [B N, D] zero-filled by the caller).  n = 0 leaves G's decoder slots and dxn untouched. */
int rmcl_mlm_backward(const rmcl_mlm_head* h, const float* params, const void* params_lp, const void* WT, int dtype, const int32_t* idx,
                      const int32_t* lab, const int32_t* count, int rows, float* ws, const float* lse, float grad_scale,
                      const float* grad_scale_dev, float* G, float* dxn, void* stream);
/* logits [rows_out, ldl] (V columns written) of the first rows_out compacted rows of the last rmcl_mlm_forward on `ws` */
int rmcl_mlm_logits(const rmcl_mlm_head* h, const float* params, const void* params_lp, int dtype, float* ws, int rows, int rows_out,
                    float* logits, int64_t ldl, void* stream);

/* ---- Masked patch prediction (task_mlm_itm_mpp) ----------------------------------------------------------------------------
 * VisionTransformer.mask_tokens (vision_transformer.py:525-557), MPPHead (heads.py:198-207) and compute_mpp (objectives.py:632-665):
 * mpp_score = Linear(D,D) - GELU (exact erf) - LayerNorm(D, eps 1e-12) - Linear(D, 768) + bias; the 768 logits are 3 channels x 256
 * intensity classes; loss = cross_entropy(logits.view(-1, 256), labels.view(-1), ignore_index -100), the mean over the labelled
 * (row, channel) pairs.  mt [D] (transformer.mask_token), tw [D,D], tb [D], lg / lb [D] (LayerNorm), dw [768,D], db [768]: element
 * offsets in ONE fp32 arena (parameters and, at the same offsets, gradients).  D in {256, 768}.  `rows`, dtype and the no-atomics rule
 * are those of the MLM head above: the head runs on the COMPACTED masked image rows, n stays on the device.                        */
typedef struct rmcl_mpp_head {
  int32_t D, reserved;
  int64_t mt, tw, tb, lg, lb, dw, db;
} rmcl_mpp_head;
/* floats of the workspace `ws` shared by forward / backward / logits for this launch extent (monotone in rows) */
int64_t rmcl_mpp_ws_floats(const rmcl_mpp_head* h, int rows);
/* labels [B, P, 3] int32 of the float image img [B, 3, H, W] (H, W multiples of the 32-pixel patch): per patch and channel
 * trunc(((sum of img * 0.5 + 0.5 over the patch) * (1 / 1024)) * 255), fp32.  sel = NULL: the whole grid, P = (H / 32) (W / 32), slot j =
 * patch j; else the selected slots of an rmcl_ragged selection (sel [B, sel_ld], counts [B], gw = W / 32): slot j < counts[b] reads patch
 * sel[b, j], every other slot gets -100 in all three channels.                                                                   */
int rmcl_mpp_labels(const float* img, int B, int H, int W, const int32_t* sel, const int32_t* counts, int sel_ld, int gw, int P,
                    int32_t* labels, void* stream);
/* The same labels from the byte feed: img uint8 [B, Hmax, Wmax, 3] (HWC, every sample in its top-left corner), sizes [B, 2] = (h, w),
 * multiples of 32, lut [256] = normalize_lut() - exactly the batch rmcl_image_u8_to_patches takes.  sel / counts / sel_ld / gw / P and the
 * layout of labels as in rmcl_mpp_labels (dense form: sel = NULL, P = (Hmax / 32) (Wmax / 32)).  The labels equal, integer for integer,
 * what rmcl_mpp_labels writes for the float batch of the same bytes (Uint8Batch.float_image()): a pixel outside its sample counts as
 * that batch's zero, 0 * 0.5 + 0.5 (not lut[0]), so a fully padded patch of the dense form has the label 127.  img 4-byte aligned. */
int rmcl_mpp_labels_u8(const uint8_t* img, const int32_t* sizes, int B, int Hmax, int Wmax, const float* lut, const int32_t* sel,
                       const int32_t* counts, int sel_ld, int gw, int P, int32_t* labels, void* stream);
/* labels [B, P, 3], masked [B, P] int32 -> idx [cap]: row b * N + L + 1 + j of xn [B N, D] for every masked valid slot (ascending) whose
 * three labels lie in [0, 256); lab [cap, 3] its labels; count [2]: count[0] = n, count[1] = the label entries outside [0, 256) of masked
 * valid slots (such a slot is skipped; callers turn a non-zero count[1] into an error).  A masked pad slot (labels -100) is ignored.
 * Entries behind n: idx -1, lab -100.  all_rows = 1 (the dense-logits pass): every image row b * N + L + t, t = 0 .. P, is listed (the
 * cls row first) and lab keeps -100 wherever the compacted form lists nothing.  cap >= B * (P + all_rows).                         */
int rmcl_mpp_compact(const int32_t* labels, const int32_t* masked, int B, int P, int L, int N, int all_rows, int cap, int32_t* idx, int32_t* lab,
                     int32_t* count, void* stream);
/* gather xn[idx] -> transform -> decoder -> three 256-way cross-entropies per row.  Per listed row r < n: lse [rows, 3], argmax [rows, 3]
 * (first maximum), rowloss [rows] = the sum over its labelled channels of lse - z[label]; rows >= n: 0 / -1 / 0.
 * stats [3] = (sum rowloss / pairs, pairs with argmax == label, pairs), pairs = 3 n on the compacted path; n = 0 gives a NaN loss like
 * F.cross_entropy over an all-ignored batch.  `ws` keeps what the backward / the logits writer need (the dense [rows, 768] logits). */
int rmcl_mpp_forward(const rmcl_mpp_head* h, const float* params, const void* params_lp, int dtype, const float* xn, const int32_t* idx,
                     const int32_t* lab, const int32_t* count, int rows, float* ws, float* lse, float* rowloss, int32_t* argmax, float* stats,
                     void* stream);
/* dz = grad_scale s (softmax(z) - onehot) / (3 n) (s = *grad_scale_dev, read on the device, or 1 when NULL), after a forward on the
 * compacted rows; G != NULL: the six head gradients are ACCUMULATED into G at the head's offsets; dxn != NULL: the gradient of the
 * gathered rows is stored to dxn[idx[r]] (dxn [B N, D] zero-filled by the caller).  n = 0: dz = 0, nothing changes.                */
int rmcl_mpp_backward(const rmcl_mpp_head* h, const float* params, const void* params_lp, int dtype, const int32_t* idx, const int32_t* lab,
                      const int32_t* count, int rows, float* ws, const float* lse, float grad_scale, const float* grad_scale_dev, float* G,
                      float* dxn, void* stream);
/* logits [rows_out, 768] of the first rows_out listed rows of the last rmcl_mpp_forward on `ws` */
int rmcl_mpp_logits(const rmcl_mpp_head* h, float* ws, int rows, int rows_out, float* logits, void* stream);

/* ---- Text attack on the fine-tuning tasks (GreedyAttack_vqa / GreedyAttack_nlvr2) ------------------------------------------
 * get_important_scores (attack/greedy_attack_vilt.py:221-228) on the device: the L1 norm over the hidden columns of the MEAN saliency
 * gradient over a word's sub-word tokens,
 *   out[b, w] = sum_d | (1 / len) * sum_{t = start .. start + len - 1} g[row0 + b * row_step, t, d] |
 * g [R, L, D] f32: the `dtext` buffer rmcl_encoder_backward fills, R >= row0 + (B - 1) * row_step + 1 sequences (row0 = 1, row_step = 2:
 * the image_1 sequences of an NLVR2 pair pass).  spans [B, W, 2] int32 = (first token position, token count) per word; positions count
 * [CLS] as 0.  A count <= 0 marks a padding entry: it writes 0.  A span that leaves [0, L) is cut to the tokens inside (nothing is read
 * out of bounds; the divisor stays the stated count).  out [B, W] f32.  fp32 accumulation, tokens summed in ascending order, one wave
 * per output, no float atomics, no scratch: two identical calls give identical bits.
 * 1 <= B <= 65536, 1 <= W <= 4096, 1 <= L <= 4096, 4 <= D <= 8192 with D % 4 == 0, row0 >= 0, row_step >= 1.                      */
int rmcl_word_saliency(const float* g, const int32_t* spans, float* out, int B, int W, int L, int D, int row0, int row_step, void* stream);

/* ---- Row top-k (the prediction API: masked-token candidates, VQA answers, retrieval lists) ---------------------------------
 * For every row of the row-major fp32 matrix x [R, C] with pitch ld >= C (in elements): the k largest entries in descending order into
 * idx [R, k] (column, int32) and val [R, k] (the selected inputs, bit for bit).
 *   order   larger value first; equal values go to the smaller column; -inf is an ordinary value that sorts last; a NaN is never
 *           selected.  A row with fewer than k selectable columns fills the remaining slots with idx -1, val -inf, prob 0.
 *   mode    RMCL_TOPK_RAW      prob is not written.
 *           RMCL_TOPK_SOFTMAX  prob = exp(val - lse_row), lse_row the log-sum-exp of the row's selectable columns, formed in the same
 *                              launch with a running maximum in fp32 and a fixed order (entries of +-80 in one row do not overflow);
 *                              written to lse [R] when that pointer is given.  A row without a finite column has lse -inf; a selected
 *                              -inf column has prob 0.
 *           RMCL_TOPK_SIGMOID  prob = 1 / (1 + exp(-val)).
 *           prob [R, k] may be NULL in every mode; lse is written in SOFTMAX mode only.
 * Any ld >= C and any 4-byte aligned x are accepted: 16-byte loads are taken from the first 16-byte boundary of each row, the ragged head
 * and tail are read column by column, and nothing outside [row, row + C) is read.  One workgroup per row, one owner per output, no
 * atomics, no scratch, no workspace: two calls on the same input give the same bytes.  R == 0 returns 0 without a launch.  Returns -1
 * before any launch for a NULL x / idx / val, an unknown mode, C < 1, ld < C, k outside 1 .. min(C, RMCL_TOPK_MAX), R < 0 or a
 * misaligned x.                                                                                                                       */
#define RMCL_TOPK_MAX 32
#define RMCL_TOPK_RAW 0
#define RMCL_TOPK_SOFTMAX 1
#define RMCL_TOPK_SIGMOID 2
int rmcl_rows_topk(const float* x, int64_t ld, int R, int C, int k, int mode, int32_t* idx, float* val, float* prob, float* lse, void* stream);

/* ---- Word-patch alignment maps (the prediction API: the heat map of the reference's demo.py:86-151) --------------------------
 * rmcl_ipot_plan_f32: IPOT (objectives.py:46-76 with k = 1) shaped for long runs (the demo's 1000 iterations).  Inputs and output
 * are those of rmcl_ipot_f32: cost [B, Lt, ld] f32 as rmcl_wpa_cost_finish leaves it (ld >= Li), txt_valid [B, Lt] / img_valid [B, Li]
 * int32, T [B, Li, Lt] like the reference's ipot().  Every joint-pad position of T is exactly zero; a sample without a valid text
 * token or without a valid image slot gets T = 0.  One 256-thread workgroup per sample, the plan in registers (thread n owns row n,
 * and row n + 256 when Li > 256), two barriers per iteration, no atomics, no scratch, no workspace, a fixed summation order
 * (csrc/align.hip; tests/align_ref.py restates it): two calls give the same bytes.  T <- (delta * (A * T)) * sigma.
 * Returns -1 before any launch, with a message naming the limit, unless 1 <= Lt <= RMCL_IPOT_PLAN_MAX_LT,
 * 1 <= Li <= RMCL_IPOT_PLAN_MAX_LI, 1 <= iters <= RMCL_IPOT_PLAN_MAX_ITERS and beta > 0.  B == 0 returns 0 without a launch.      */
#define RMCL_IPOT_PLAN_MAX_LT 40
#define RMCL_IPOT_PLAN_MAX_LI 512
#define RMCL_IPOT_PLAN_MAX_ITERS 10000
int rmcl_ipot_plan_f32(const float* cost, const int32_t* txt_valid, const int32_t* img_valid, float* T, int B, int Lt, int Li, int ld,
                       float beta, int iters, void* stream);
/* rmcl_align_heat: a plan T [B, Li, Lt] to patch grids, heat maps and alpha bytes.  patch_index [B, Li - 1] int32: the grid cell
 * h * W + w of image slot 1 + i (slot 0, the image cls row, is dropped); an entry outside [0, H W) writes nothing, and the entries
 * inside it must be distinct per sample.
 *   grid [B, Lt, H, W] f32   T[b, 1 + i, m] at cell patch_index[b, i]; every other cell 0.
 *   heat [B, Lt, H, W] f32   the demo's arithmetic over the whole grid: z = (grid - mean) / std (unbiased), clip(z, 1, 3),
 *                            (c - min) / (max - min).  Mean, variance and extrema are accumulated in fp64 from the fp32 cells in a
 *                            fixed order; heat is rounded to fp32 once.
 *   flat [B, Lt] int32       1 where the demo would divide by zero: txt_valid[b, m] == 0, H W < 2, std == 0, or all clipped values
 *                            equal.  Such a position has heat = 0 (a deviation from the demo, which produces NaN there).
 *   alpha [B, Hout, Wout] uint8 (may be NULL; then token / tables are not read)   for position m = token[b] of sample b:
 *                            uint8(heat * 255) - the fp32 product, truncated like np.uint8 - of cell (tables[y], tables[Hout + x]):
 *                            tables [Hout + Wout] int32 are PIL's NEAREST source indices of the rows, then of the columns (entries are
 *                            clamped to the grid).  alpha[b] is written only when 0 <= token[b] < Lt.
 * One workgroup per (sample, position), one owner per output, no atomics, no scratch.  Returns -1 before any launch for a NULL
 * operand, B outside 0 .. 65535, Lt < 1, Li < 1, H W outside 1 .. RMCL_ALIGN_MAX_CELLS or an alpha extent outside 1 .. 16384.     */
#define RMCL_ALIGN_MAX_CELLS 4096
int rmcl_align_heat(const float* T, const int32_t* patch_index, const int32_t* txt_valid, int B, int Lt, int Li, int H, int W, float* grid,
                    float* heat, int32_t* flat, const int32_t* token, const int32_t* tables, int Hout, int Wout, uint8_t* alpha,
                    void* stream);

/* One joint text+image encoder forward up to transformer.norm: replaces ViLTransformerSS.infer /
 * infer_k (vilt_module.py:275-418) minus the pooler.  params32: fp32 arena; params_lp: bf16
 * shadow arena (NULL when dtype is F32).  text_ids/text_mask [B,L] int64; patches [B*P,patch_k]
 * in `dtype`; co_mask out [B,N] int32 (N = L+1+P); xn out [B*N, D] f32.
 * drop_p > 0 enables the reference's dropout sites (BertEmbeddings dropout, pos_drop, proj_drop, both Mlp
 * drops; vision_transformer.py:279-285,330-331,667) with a counter-based RNG: masks are a pure function
 * of (drop_seed, site, element), so the backward, given the same seed, regenerates them.
 * ragged: NULL for full-size images (dense fixed-order patches), else the selection of a zero-padded batch.  */
int rmcl_encoder_forward(const rmcl_dims* d, int mode, const float* params32, const void* params_lp,
                         const int64_t* text_ids, const int64_t* text_mask, const void* patches,
                         int32_t* co_mask, void* stash, void* workspace, float* xn,
                         uint32_t drop_seed, float drop_p, const rmcl_ragged* ragged, const rmcl_fold* fold, void* stream);

/* rmcl_encoder_forward with the mask-token substitution of masked patch prediction: replaced [B, P] int32; where replaced[b, j] != 0 the
 * patch-projection output (bias included) of slot j is replaced by the mask token params32[mask_token_off .. + D) BEFORE the position
 * rows and the token type are added (vision_transformer.py:602-603).  Every mode; RMCL_MODE_CLS_TAIL is refused (the loss reads the
 * image rows).  replaced = NULL (or all zero): rmcl_encoder_forward, bit for bit.                                                 */
int rmcl_encoder_forward_mpp(const rmcl_dims* d, int mode, const float* params32, const void* params_lp,
                             const int64_t* text_ids, const int64_t* text_mask, const void* patches,
                             int32_t* co_mask, void* stash, void* workspace, float* xn,
                             uint32_t drop_seed, float drop_p, const rmcl_ragged* ragged, const rmcl_fold* fold,
                             const int32_t* replaced, int64_t mask_token_off, void* stream);

/* ---- Image-text retrieval (IRTR) ---------------------------------------------------------------------------------------
 * The image side of VisionTransformer.visual_embed (vision_transformer.py:559-677, mask_it = False) for the patch rows of
 * rmcl_encoder_forward: patch GEMM + (resized) position rows + cls token, WITHOUT the token-type row (the reference adds it in infer,
 * vilt_module.py:315-321).  out [B, 1 + P, D] f32, masks [B, 1 + P] int32 (cls 1, then the patch mask rmcl_encoder_forward derives).
 * workspace: rmcl_workspace_bytes(d).  ragged as for rmcl_encoder_forward (dpos_tok is not used).                             */
int rmcl_visual_embed(const rmcl_dims* d, const float* params32, const void* params_lp, const void* patches, const rmcl_ragged* ragged,
                      void* workspace, float* out, int32_t* masks, void* stream);

/* rmcl_visual_embed with the mask-token substitution of rmcl_encoder_forward_mpp (visual_embed(mask_it=True)): replaced [B, P] int32 */
int rmcl_visual_embed_mpp(const rmcl_dims* d, const float* params32, const void* params_lp, const void* patches, const rmcl_ragged* ragged,
                          void* workspace, float* out, int32_t* masks, const int32_t* replaced, int64_t mask_token_off, void* stream);

/* The image tokens of a rank pass come from a device-resident cache of rmcl_visual_embed outputs instead of pixels
 * (compute_irtr_recall, objectives.py:1226-1346: every image against every caption).  embeds [n_img, ld_tok, D] f32 and
 * masks [n_img, ld_tok] int32 hold one image per slot (rows behind an image's own tokens: zeros, mask 0); img_of [B] int32 names the
 * slot of every sequence of the pass, so one pass holds ANY set of (image, caption) pairs.                                      */
typedef struct rmcl_rank_src {
  const float* embeds;
  const int32_t* masks;
  const int32_t* img_of;
  int32_t n_img;
  int32_t ld_tok;           /* token rows per cache slot, >= 1 + d->P */
} rmcl_rank_src;
/* rmcl_encoder_forward in INFER mode (RMCL_MODE_CLS_TAIL may be OR-ed in) whose sequence b is text b + the first 1 + d->P cached token
 * rows of image img_of[b] + token-type row 1; co_mask [B, N] = text mask | cached image mask.  No dropout, no stash.  A sequence whose
 * img_of is outside [0, n_img) gets zero image rows and a zero image mask.                                                      */
int rmcl_encoder_forward_rank(const rmcl_dims* d, int mode, const float* params32, const void* params_lp, const int64_t* text_ids,
                              const int64_t* text_mask, const rmcl_rank_src* src, int32_t* co_mask, void* workspace, float* xn,
                              const rmcl_fold* fold, void* stream);
/* rank_output (vilt_module.py:233-239: Linear(D, 1) whose weight / bias are row 1 of itm_score.fc): scores[o] = cls[i] . w + b with
 * o = out_index[i] (int32, e.g. img * n_txt + txt of the recall score matrix) or i when out_index is NULL.  cls rows have pitch ld_cls;
 * scores holds out_n floats and an index outside [0, out_n) is dropped.  One wave per sequence.                                 */
int rmcl_irtr_score(const float* cls, int64_t ld_cls, const float* w, const float* bias, int S, int D, float* scores,
                    const int32_t* out_index, int64_t out_n, void* stream);
/* compute_irtr's loss (objectives.py:1211-1214): cross-entropy against answer 0 over each of the B groups of R consecutive scores
 * (the true caption first, then draw_false_text false ones; R <= 64).  stats [2] = (mean loss, groups whose first maximum is score 0);
 * rows [B] (optional) per-group loss; dscore [B * R] (optional) = grad_scale * s * (softmax - onehot_0) / B with s = *grad_scale_dev or 1.
 * One workgroup, fixed reduction order, no float atomics.                                                                       */
int rmcl_irtr_ce(const float* scores, int B, int R, float grad_scale, const float* grad_scale_dev, float* dscore, float* rows, float* stats,
                 void* stream);
/* dcls [S, D] = dscore[i] * w;  dw [D] += sum_i dscore[i] * cls[i, :] (i ascending);  db [1] += sum_i dscore[i].  dw / db may be NULL
 * (data gradient only).  No float atomics.                                                                                      */
int rmcl_irtr_bwd(const float* dscore, const float* cls, int64_t ld_cls, const float* w, int S, int D, float* dcls, float* dw, float* db,
                  void* stream);

/* Backward of the above.  dxn: gradient wrt xn, [B*N,D] f32, or [B,D] (row 0 of every sample)
 * when cls_only=1; cls_only=2: the same [B,D] gradient for a stash whose forward ran with RMCL_MODE_CLS_TAIL (compact last
 * layer).  dpatches (optional) receives d loss/d patches [B*P,patch_k] in `dtype`
 * (the PGD data gradient, attack/pgd_attack_vilt.py:160-162).  dtext (optional) receives d loss/d
 * word-embedding output [B*L, D] f32 (the text-attack saliency, greedy_attack_vilt.py:414-452).
 * grads32 (mode FULL): gradient
 * arena, accumulated into (+=), same layout as the parameter arena.  params_lpT (optional, bf16 mode): transposed
 * weight shadows from rmcl_weight_transpose_bf16.                                                 */
int rmcl_encoder_backward(const rmcl_dims* d, int mode, const float* params32, const void* params_lp,
                          const int64_t* text_ids, const void* patches, const int32_t* co_mask,
                          void* stash, void* workspace, const float* dxn, int cls_only,
                          void* dpatches, float* dtext, float* grads32, uint32_t drop_seed, float drop_p,
                          const rmcl_ragged* ragged, const void* params_lpT, void* stream);

/* rmcl_encoder_backward (full-row dxn: cls_only = 0) of a pass run by rmcl_encoder_forward_mpp with the same `replaced`: the gradient
 * arriving at the patch-embedding rows of replaced patches (image-token dropout mask applied, fp32, rows ascending) is ACCUMULATED into
 * grads32[mask_token_off .. + D) in FULL mode, and those rows are zeroed before dpatches, the patch-weight and the patch-bias gradients
 * read them: a replaced patch contributes nothing to patch_embed.proj.  replaced = NULL: rmcl_encoder_backward, bit for bit.        */
int rmcl_encoder_backward_mpp(const rmcl_dims* d, int mode, const float* params32, const void* params_lp,
                              const int64_t* text_ids, const void* patches, const int32_t* co_mask,
                              void* stash, void* workspace, const float* dxn,
                              void* dpatches, float* dtext, float* grads32, uint32_t drop_seed, float drop_p,
                              const rmcl_ragged* ragged, const void* params_lpT,
                              const int32_t* replaced, int64_t mask_token_off, void* stream);

/* Pooler + MoCo head + L2 normalise (vilt/modules/heads.py:10-20,129-143; objectives.py:264-269).
 * pool32: arena that owns the pooler (always the query arena); head32: arena that owns the
 * moco head (query or momentum).  Outputs cls_feats [B,D] and q [B,proj] (f32).                  */
int rmcl_heads_forward(const rmcl_dims* d, const float* pool32, const float* head32, const float* xn,
                       void* hstash, float* cls_feats, float* q, void* stream);
/* The same with flags.  RMCL_HEADS_NO_WGRAD: the matching rmcl_heads_backward will be called with grads32 = NULL (key pass, PGD
 * and text-attack passes: data gradients only) - the pooler input is then not stashed and one launch less is issued.  The library
 * remembers (on the host) which stash buffers last saw such a forward: rmcl_heads_backward on one of them with grads32 != NULL
 * returns -1 instead of forming the pooler weight gradient from a stale input.  The record is per stash address, is updated when
 * the call is made (not when the enqueued work executes) and is never dropped: only a later forward without the flag on the same
 * address clears it.                                                                                                         */
#define RMCL_HEADS_NO_WGRAD 1
int rmcl_heads_forward2(const rmcl_dims* d, const float* pool32, const float* head32, const float* xn,
                        void* hstash, float* cls_feats, float* q, int flags, void* stream);
/* dq [B,proj] (may be NULL) and dcls_extra [B,D] (may be NULL, e.g. from the ITM head) -> dcls [B,D];
 * grads32 (may be NULL) accumulates pooler and moco-head weight gradients.                       */
int rmcl_heads_backward(const rmcl_dims* d, const float* pool32, const float* head32, void* hstash,
                        const float* dq, const float* dcls_extra, float* dcls, float* grads32, void* workspace, void* stream);

/* Fused InfoNCE forward + dq + queue metrics (objectives.py:328-351, pgd_attack_vilt.py:152-158).
 * rows_out [B,10]: loss_i, argmax, l_pos, pos_dist, pos_cos, pos_dot, neg_dist, neg_cos, neg_dot, lse.
 * loss_sum (optional, 1 float, += mean loss).  workspace: rmcl_infonce_ws_bytes(B,Kq) bytes.      */
int64_t rmcl_infonce_ws_bytes(int B, int64_t Kq);
int rmcl_infonce_f32(const float* q, const float* k, const float* queue, int B, int proj, int64_t Kq, float temperature,
                     float grad_scale, float* dq, float* rows_out, float* loss_sum, void* workspace, void* stream);
/* The same pass for the bf16 engine: logits and dq on the bf16 matrix cores with SPLIT operands (x = bf16(x) + bf16(x - bf16(x)),
 * three products per pair: 2^-16 relative per product, fp32 softmax / accumulation) - the fp32 queue is read as it is.
 * with_metrics = 0 (the PGD passes consume dq only): rows_out[6..8] (queue-distance means) are written as 0, whichever kernel runs.
 * At Kq % 256 == 128, and under rmcl_tune_set key 5 = 0, this entry runs the exact-f32 kernel of rmcl_infonce_f32 (no split products). */
int rmcl_infonce_split_bf16(const float* q, const float* k, const float* queue, int B, int proj, int64_t Kq, float temperature,
                            float grad_scale, float* dq, float* rows_out, float* loss_sum, void* workspace, int with_metrics,
                            void* stream);

/* PGD ascent step in patch layout (attack/pgd_attack_vilt.py:162-173).  amax_scratch: 64 * B uint32 (per-block partial maxima of
 * |grad| per sample; need not be cleared).                                                          */
int rmcl_pgd_step(const void* grad, int dtype, float* delta, uint32_t* amax_scratch, int B, int64_t per_sample,
                  float lr, float eps, void* stream);
/* The same step fused with the loop's next operand (attack/pgd_attack_vilt.py:144,162-173): delta is updated in place and, when
 * `operand` is given, operand = cast(base + delta_new) - the next encoder forward's patch rows - in the same pass.
 * RMCL_PGD_DELTA_ZERO: the incoming delta is the all-zero delta_0 and is not read (the buffer need not be cleared).
 * RMCL_PGD_SUM_PREV: operand = cast((base + delta_old) + delta_new): the attacked view img + delta_{K-1} + delta_K that
 * objectives.py:176 builds on the batch image pgd_attack left behind.  base: the clean patch rows (fp32).                 */
#define RMCL_PGD_DELTA_ZERO 1
#define RMCL_PGD_SUM_PREV 2
int rmcl_pgd_step_fused(const void* grad, int dtype, float* delta, uint32_t* amax_scratch, int B, int64_t per_sample, float lr,
                        float eps, const float* base, void* operand, int operand_dtype, int flags, void* stream);
/* ---- PGD threat models (csrc/pgd_ball.hip) ------------------------------------------------------------------------------------
 * Configurable forms of the step above, in the same patch layout: B samples of per_sample fp32 delta elements (per_sample % 4 == 0).
 * valid (int32 [B], optional): the number of LEADING elements of each sample that belong to real patches (RaggedGeometry.counts[b] *
 * patch_k); NULL: all of them.  Elements at or beyond valid[b] are pad slots: they always get delta = 0 and operand = cast(base), and
 * they take part in no maximum and no norm.
 * scratch: rmcl_pgd_ball_scratch_bytes(B) bytes, 8-byte aligned, need not be cleared: per-block partials (at most 64 per sample and
 * statistic; slots beyond a launch's block count are neither written nor read).  Sums of squares are accumulated in double in a fixed
 * order and nothing is accumulated atomically: a repeated call writes the same bytes.
 *
 * rmcl_pgd_step_ball: one ascent step, the projection and the next forward's operand.  Per sample, g = grad on the valid elements:
 *   direction d   RMCL_PGD_DIR_NORMALISED  g / max(max|g|, 1e-8)   (the reference's, the arithmetic of rmcl_pgd_step_fused)
 *                 RMCL_PGD_DIR_SIGN        sign(g), sign(0) = 0
 *                 RMCL_PGD_DIR_L2          g / max(||g||_2, 1e-12)
 *   t = delta_old + lr d                   (flag RMCL_PGD_DELTA_ZERO: delta_old = 0, the buffer is not read)
 *   projection t' RMCL_PGD_BALL_LINF       clamp(t, +-eps)
 *                 RMCL_PGD_BALL_L2         t min(1, eps / ||t||_2)
 *                 eps <= 0                 none
 *   box, when lo < hi:   x = clamp(base + t', lo, hi), delta_new = x - base, operand = cast(x)
 *   without a box:       delta_new = t', operand = cast(base + t')
 * The box runs AFTER the ball: where base lies inside [lo, hi] (the pixelbert normalisation gives [-1, 1] on every valid element)
 * clamping base + t' moves each element towards base, |delta_new| <= |t'| element by element, so the result stays inside either ball.
 * The kernel does not check base.  There is no SUM_PREV form: a configured threat model is evaluated on img + delta_K.
 * base is required with an operand or a box; operand is optional.  The L2 ball takes one more pass over grad and delta (the norm of t).
 *
 * rmcl_pgd_random_start: delta_0 and the first operand.  With h = rmcl_rng_hash(rmcl_rng_hash(seed, sample0 + b), i) (csrc/rmcl_common.h)
 * for element i of sample b, u = (h >> 8) 2^-24 and v = 2u - 1:  L-inf: delta = eps v;  L2: delta = eps v / ||v||_2 over the valid
 * elements - a point ON the sphere: the radius draw U^(1/n) of a uniform point of the ball is left out, since in n >= 3072 dimensions
 * P(radius <= 0.99 eps) = 0.99^n < 4e-14.  The box is applied as above.  sample0: global index of the call's first sample, so a
 * half-batch lane draws what the whole batch would; a restart number is mixed into seed by the caller.
 *
 * rmcl_pgd_keep_worst: the per-sample worst case over restarts, decided on the device.  score_new[j * score_stride] is decision j's
 * score after restart `restart`; decision j owns the rows_per_decision (1 or 2: NLVR2's pair pass) consecutive sample rows
 * j * G .. j * G + G - 1 of delta / operand.  It takes the new result iff restart == 0 or score_new > best_score[j] (strict; a NaN
 * never takes except at restart 0): its delta (and operand) rows are copied into best_delta (best_operand) and best_score / best_restart
 * are updated; every other row and score is left untouched.                                                                        */
#define RMCL_PGD_DIR_NORMALISED 0
#define RMCL_PGD_DIR_SIGN 1
#define RMCL_PGD_DIR_L2 2
#define RMCL_PGD_BALL_LINF 0
#define RMCL_PGD_BALL_L2 1
int64_t rmcl_pgd_ball_scratch_bytes(int B);
int rmcl_pgd_step_ball(const void* grad, int dtype, float* delta, void* scratch, const int32_t* valid, int B, int64_t per_sample,
                       float lr, float eps, int direction, int ball, float lo, float hi, const float* base, void* operand,
                       int operand_dtype, int flags, void* stream);
int rmcl_pgd_random_start(float* delta, void* scratch, const int32_t* valid, int B, int64_t per_sample, int sample0, uint32_t seed,
                          float eps, int ball, float lo, float hi, const float* base, void* operand, int operand_dtype, void* stream);
int rmcl_pgd_keep_worst(const float* score_new, int64_t score_stride, float* best_score, int32_t* best_restart, int restart, int D,
                        int rows_per_decision, const float* delta, float* best_delta, const void* operand, void* best_operand,
                        int operand_dtype, int64_t per_sample, void* stream);
/* sum over (row, pixel) of the channel-wise L2 norm of delta (objectives.py:184); out += sum     */
int rmcl_delta_channel_norm(const float* delta, float* out, int64_t rows, int C, int pp, void* stream);

/* Momentum update k = m*k + (1-m)*q over n arena elements (objectives.py:219-224,257-260);
 * k_lp (optional) refreshed bf16 shadow.                                                         */
int rmcl_ema_f32(float* k, const float* q, void* k_lp, float m, int64_t n, void* stream);
/* queue[:, ptr:ptr+n] = keys^T (objectives.py:244-246); queue [proj,Kq] f32, keys [n,proj] f32.  */
int rmcl_enqueue_f32(float* queue, const float* keys, int n, int proj, int64_t Kq, int64_t ptr, void* stream);
/* f32 -> dtype cast of n elements (bf16 weight shadow refresh).                                  */
int rmcl_cast_f32(const float* in, void* out, int dtype, int64_t n, void* stream);

/* Fused AdamW over flat arenas ("next" row f1; vilt/modules/vilt_utils.py:395-398, HF AdamW).    */
int rmcl_adamw_f32(float* p, const float* g, float* m, float* v, void* p_lp, const int64_t* seg_end,
                   const float* seg_lr_mult, const float* seg_wd, int nseg, float lr, float beta1, float beta2,
                   float eps, int step, float grad_scale, int64_t n, void* stream);

/* Guarded optimizer step (Lightning's precision=16 GradScaler skip and gradient_clip_val, run.py:92-112): the decision to skip or
 * clip a step is taken on the device and handed to the AdamW through this block of DEVICE memory, so a step costs no host round
 * trip.  48 bytes, 8-byte aligned; the host reads it only when asked (counters, norm).  Zero-fill it before the first step.
 *   offset  0  double  sumsq       sum of g^2 over the FINITE elements of the last statistics pass (unscaled gradient)
 *   offset  8  int64   nonfinite   elements of that pass whose exponent bits are all ones (NaN, +inf, -inf)
 *   offset 16  float   norm        (float)(grad_scale * sqrt(sumsq))
 *   offset 20  float   clip_coef   max_norm > 0 ? min(1, max_norm / (norm + 1e-6f)) : 1      (torch.nn.utils.clip_grad_norm_)
 *   offset 24  int32   skip        nonfinite > 0: the guarded AdamW that follows writes nothing
 *   offset 28  int32   applied     AdamW steps actually applied so far (the step number of the bias corrections)
 *   offset 32  int32   skipped     steps dropped so far
 *   offset 36  float   bc1         1 - beta1^applied          (double arithmetic, rounded once)
 *   offset 40  float   bc2s        sqrt(1 - beta2^applied)
 *   offset 44  int32   reserved                                                                                          */
typedef struct rmcl_step_ctl {
  double sumsq;
  int64_t nonfinite;
  float norm, clip_coef;
  int32_t skip, applied, skipped;
  float bc1, bc2s;
  int32_t reserved;
} rmcl_step_ctl;
/* One pass over the n fp32 gradients (n > 0, n % 4 == 0): per-block (sum of squares in double, non-finite count) pairs into `ws`
 * (rmcl_grad_stats_ws_bytes(n) bytes, every byte of it written), then one block adds them in a fixed order and writes the decision
 * into ctl: sumsq, nonfinite, norm, clip_coef, skip; not skipping, applied += 1 and bc1 / bc2s of that step; skipping, skipped += 1.
 * No atomics: the same input gives the same bytes of ws and ctl on every call.                                           */
int64_t rmcl_grad_stats_ws_bytes(int64_t n);
int rmcl_grad_stats_f32(const float* g, int64_t n, float grad_scale, float max_norm, float beta1, float beta2, void* ws,
                        rmcl_step_ctl* ctl, void* stream);
/* rmcl_adamw_f32 with skip, clip_coef, bc1 and bc2s read from ctl on the device: skip set, no byte of p, m, v or p_lp is written;
 * otherwise the gradient is g * grad_scale * clip_coef and the rest (segments, weight decay, bf16 shadow) is rmcl_adamw_f32's.   */
int rmcl_adamw_guarded_f32(float* p, const float* g, float* m, float* v, void* p_lp, const int64_t* seg_end,
                           const float* seg_lr_mult, const float* seg_wd, int nseg, float lr, float beta1, float beta2,
                           float eps, float grad_scale, const rmcl_step_ctl* ctl, int64_t n, void* stream);

/* Adam and SGD over the same flat arenas (vilt/modules/vilt_utils.py:399-402: torch.optim.Adam(groups, lr) and
 * torch.optim.SGD(groups, lr, momentum=0.9)), with rmcl_adamw_f32's segment tables, grad_scale and optional bf16 shadow p_lp.
 * All arithmetic in fp32, per element, in this order (slr = lr * seg_lr_mult[s], wd = seg_wd[s] of the element's segment s):
 *   gj = g * grad_scale                      guarded form: gj = (g * grad_scale) * clip_coef
 *   if wd > 0: gj = gj + wd * p              torch's coupled L2 decay, on the OLD p
 *   RMCL_OPTIM_ADAM  (torch.optim.Adam, amsgrad off; the reference's defaults: betas (0.9, 0.999), eps 1e-8)
 *     m = b1 * m + (1 - b1) * gj
 *     v = b2 * v + (1 - b2) * gj * gj
 *     p = p - ((slr / bc1) * m) / (sqrt(v) / bc2s + eps)        bc1 = 1 - b1^t, bc2s = sqrt(1 - b2^t), each computed in double and
 *                                                               rounded once; eps is added AFTER the division by bc2s (rmcl_adamw_f32,
 *                                                               HF AdamW, adds it before)
 *   RMCL_OPTIM_SGD   (torch.optim.SGD with momentum, dampening 0, nesterov off; beta1 IS the momentum, beta2 and eps are ignored)
 *     m = b1 * m + gj                                           (m zero-filled before the first step gives torch's buf = gj)
 *     p = p - slr * m
 *     v must be NULL: SGD keeps no second moment.
 * ctl == NULL: the plain form, t = step (>= 1).  ctl != NULL: the guarded form, `step` is ignored; ctl->skip set, no byte of p, m, v
 * or p_lp is written; otherwise clip_coef and, for Adam, bc1 / bc2s are read from ctl as rmcl_grad_stats_f32 (called with Adam's betas)
 * left them.  With clip_coef == 1 the guarded form gives the plain form's bits.  n > 0, n % 4 == 0, nseg > 0.              */
#define RMCL_OPTIM_ADAM 1
#define RMCL_OPTIM_SGD 2
int rmcl_optim_step_f32(int rule, float* p, const float* g, float* m, float* v, void* p_lp, const int64_t* seg_end,
                        const float* seg_lr_mult, const float* seg_wd, int nseg, float lr, float beta1, float beta2, float eps,
                        int step, float grad_scale, const rmcl_step_ctl* ctl, int64_t n, void* stream);

/* Epoch metrics on the device (vilt/gadgets/my_metrics.py: Accuracy, VQAScore, Scalar, change_rate - each a (sum, count) pair that is
 * divided at the end of the epoch).  `table` is double[n_slots][2], slot s = (table[2 s], table[2 s + 1]) = (sum, count).  One call adds up
 * to RMCL_METRIC_MAX_OPS ops, carried BY VALUE in the kernel arguments (nothing is uploaded); one workgroup of 256 threads per op, the
 * workgroups of a call run concurrently, so the slot ranges of a call's ops must not overlap.  Stream order serialises calls.
 *
 * A row kind reads `rows` rows and takes an optional `group` table, int32 [rows]: row r belongs to group group[r] when that lies in
 * [0, n_groups), and is left out otherwise; without a table every row is in group 0.  Group g adds into slot `slot + g`; an op owns the
 * slots [slot, slot + n_groups), 1 <= n_groups <= 4 (SCALAR and PAIR use `slot` alone).  n_g = rows of group g.
 *   SCALAR        sum += scale * x,  x = ((const float*)a)[0] or `imm` when a is NULL;  count += 1                   (Scalar.update)
 *                 optional gate b: nothing when ((const float*)b)[0] == 0 (the loss of a batch without a labelled row, which is NaN)
 *   PAIR          sum += ((const float*)a)[0], count += ((const float*)b)[0];  nothing when that count is 0         (MLM / MPP stats[1], [2])
 *   ROWSUM        sum += sum_{r in g} x[r * stride], count += n_g;  nothing when n_g == 0;  x = (const float*)a      (VQAScore.update)
 *   ROWMEAN       sum += (sum_{r in g} x[r * stride]) / n_g, count += 1;  nothing when n_g == 0                      (Scalar of a split's mean loss)
 *   MATCH         a, b int32 [rows]; over the rows of g with b[r] != ignore_index: sum += #(a[r] == b[r]), count += #rows; nothing when no
 *                 row qualifies.  RMCL_METRIC_INVERT: sum += #(a[r] != b[r]) over ALL rows of g, ignore_index is not read
 *                                                                                                                 (Accuracy.update, change_rate.update)
 *   ARGMAX_MATCH  MATCH with a[r] = index of the FIRST maximum of row r of the fp32 logits a = [rows, pitch], columns 0 .. ncols - 1
 *                 (1 <= ncols <= pitch; the pad columns are not read); one wave per row; a row of -inf gives index 0.
 * Counts stay integers until the one addition into the table; sums are in double in a fixed order (a thread's strided partial, a butterfly
 * over the wave, the four waves in wave order), no float or double atomics: from the same table bytes and the same inputs a call leaves the
 * same bytes.  rows == 0 is legal and writes nothing.  Inputs are finite: a NaN among the logits or the addends is the caller's problem, as
 * for the heads' own argmax.  Returns -1, with nothing launched and the table untouched, for: n_ops outside 1 .. 8, a NULL table or required
 * pointer, an unknown kind or flag, n_groups outside 1 .. 4, a slot range outside [0, n_slots), rows < 0, stride < 1, ncols < 1 or
 * ncols > pitch, or two ops of the call whose slot ranges overlap.                                                                      */
#define RMCL_METRIC_SCALAR 0
#define RMCL_METRIC_PAIR 1
#define RMCL_METRIC_ROWSUM 2
#define RMCL_METRIC_ROWMEAN 3
#define RMCL_METRIC_MATCH 4
#define RMCL_METRIC_ARGMAX_MATCH 5
#define RMCL_METRIC_INVERT 1
#define RMCL_METRIC_MAX_OPS 8
#define RMCL_METRIC_MAX_GROUPS 4
typedef struct {
  int32_t kind, slot, n_groups, flags;
  int32_t rows, stride, ncols, pitch;
  int32_t ignore_index;
  float scale, imm;
  int32_t reserved;
  const void* a;
  const void* b;
  const int32_t* group;
} rmcl_metric_op;
typedef struct {
  int32_t n_ops, reserved;
  rmcl_metric_op op[RMCL_METRIC_MAX_OPS];
} rmcl_metric_ops;
int rmcl_metrics_update(double* table, int n_slots, const rmcl_metric_ops* ops, void* stream);

/* ITM + word-patch alignment (objectives.py:24-76,714-787).  cost / dsim are [B, Lt, ld] f32 with
 * ld >= Li a multiple of 4 (GEMM operand pitch); T is [B, Li, Lt] like the reference's ipot().      */
int rmcl_gemm_batched(const void* A, const void* B, void* C, int M, int N, int K, int64_t lda, int64_t ldb, int ldc, float alpha,
                      int nbatch, int64_t strideA, int64_t strideB, int64_t strideC, int dt_in, int dt_out, int a_kc, int b_kc,
                      void* stream);
int rmcl_l2norm_rows_fwd(const float* x, float* y, float* norms, int rows, int D, float eps, void* stream);   /* cost_matrix_cosine :31-32 */
int rmcl_l2norm_rows_bwd(const float* dy, const float* y, const float* norms, float* dx, int rows, int D, void* stream);
int rmcl_wpa_cost_finish(float* cost, const int32_t* txt_valid, const int32_t* img_valid, int B, int Lt, int Li, int ld, void* stream);
int rmcl_ipot_f32(const float* cost, const int32_t* txt_valid, const int32_t* img_valid, float* T, int B, int Lt, int Li,
                  int ld, float beta, int iters, void* stream);
/* dist[b] = trace(cost_b @ T_b) (objectives.py:761); dsim = -w[b] * T^T = d(sum_b w_b dist_b)/d(cosine sim)  */
int rmcl_wpa_distance(const float* cost, const float* T, const float* w, float* dist, float* dsim, int B, int Lt, int Li, int ld,
                      void* stream);
/* ITMHead + 2-class CE (heads.py:173-180, objectives.py:764-765): logits, mean loss (+=), dlogits = grad_scale*(softmax-onehot) */
int rmcl_itm_fwd(const float* cls, const float* W, const float* bias, const int32_t* labels, float* logits, float* dlogits,
                 float* loss_sum, int B, int D, float grad_scale, void* stream);
int rmcl_itm_bwd(const float* dlogits, const float* cls, const float* W, float* dcls, float* dW, float* db, int B, int D,
                 float scale, void* stream);

/* ---- kernel-level entry points (unit parity tests) ----------------------------------------- */
/* C = epilogue(alpha * op(A) op(B)); layout kinds and epilogue flags: csrc/gemm.h.
 * EPI_PREACT_TILED (16384), with bf16 output, b_kc = 1 and a shape the 192x384 kernel takes (rmcl_gemm_route = 2) - anything else is an
 * error, never a row-major fallback: the pre-activation of an MLP in TILE ORDER.  With EPI_GELU | EPI_SAVE_PREACT, C2 is not [M][ldc] but
 * one block of 192 x 384 bf16 (147 456 bytes) per output tile, blocks ordered by (row tile, column tile), inside a block the order in
 * which the kernel's accumulator registers hold the tile (csrc/gemm.h rmcl_preact_tiled_off); with EPI_DGELU (no bias), aux is such a
 * buffer and ld_aux stays the logical row length.  Size in elements: ceil(M / 192) * (N / 384) * 192 * 384 - the rows padded to whole
 * blocks; rows of a block behind the tile's live rows hold anything.  Only a GEMM of the same M and N reads what another wrote.
 * (rmcl_encoder_forward keeps rmcl_stash_bytes as it was: a layer's tiled buffer begins in the tail of the layer's `probs` slot, free under
 * the fused / streamed attention every tiled pass runs, and ends with the `u` slot.)
 * rmcl_linear_lnfold(_c): bit 1 of `gelu` asks for the tiled `preact`.                                                           */
int rmcl_gemm(const void* A, const void* B, void* C, void* C2, const float* bias, const void* aux, int M, int N, int K,
              int64_t lda, int64_t ldb, int ldc, int ld_aux, float alpha, int epi, int splitk, int dt_in, int dt_out,
              int a_kc, int b_kc, int exact, void* stream);
/* Skinny fp32 GEMM whose A operand is bf16 rows read in place: C[M, N] = epilogue(A[M, K] W[N, K]^T) with A bf16 at row stride lda (in
 * bf16 elements, lda % 4 == 0), W / bias / aux / C / C2 fp32, epi of csrc/gemm.h.  Widening bf16 is exact: the result has the bits of
 * rmcl_rows_gather_f32 followed by rmcl_gemm on the fp32 rows.  Runs on the streaming skinny kernel only (M <= 1024, K % 64 == 0,
 * 128 <= K < 2048, N < 4096, rmcl_tune_set key 6 at -1 or 2); anything else is an error, never a converted copy.                      */
int rmcl_gemm_rows_bf16(const void* A, const float* W, float* C, float* C2, const float* bias, const float* aux, int M, int N, int K,
                        int64_t lda, int ldc, int ld_aux, int epi, void* stream);
/* out[r, :] = f32(in[(r * stride + off) * D ...]) for r < R: rows of a [., D] tensor of `dtype` gathered at a row stride into compact fp32. */
int rmcl_rows_gather_f32(const void* in, int dtype, float* out, int R, int D, int64_t stride, int64_t off, void* stream);
/* Kernel family the bf16 fast path gives a GEMM of this shape / epilogue / layout to under the current tuning: 0 = 128x128 tiles,
 * 1 = 192x192 one workgroup per CU (gemm_st.hip), 2 = 192x384 (gemm_sw.hip), 3 = 192x192x32 two workgroups per CU (gemm_dp.hip),
 * 4 / 5 = 256x256.  Lets a parity test state WHICH kernels it compared with the oracle.  The answer 0 holds for a GEMM the 128x128
 * kernel can take (N % 128 == 0, K % 64 == 0, bf16 operands): rmcl_gemm runs any other such GEMM on the exact kernels.              */
int rmcl_gemm_route(int M, int N, int K, int epi, int dt_out, int a_kc, int b_kc);
/* rmcl_gemm with bf16 operands stored K-BLOCKED, [K/32][rows][32] (kblk bit 0: A, bit 1: B): the layout the two-workgroups-per-CU
 * kernel (csrc/gemm_dp.hip) streams as whole 128-byte lines; A [M,K] x B [N,K]^T only; fails when no kernel takes the layout  */
int rmcl_gemm_kblk(const void* A, const void* B, void* C, void* C2, const float* bias, const void* aux, int M, int N, int K,
                   int ldc, int ld_aux, int epi, int dt_out, int kblk, void* stream);
int rmcl_layernorm_fwd(const float* x, const float* w, const float* b, float eps, void* y, int dt_out, float* mean,
                       float* rstd, int M, int D, int relu, void* stream);
int rmcl_layernorm_bwd(const void* dy, int dt_dy, const float* x, const float* mean, const float* rstd, const float* w,
                       const float* b, float* dx, int add, float* dgamma, float* dbeta, int M, int D, int relu, void* stream);
/* Masked multi-head self-attention on a packed qkv [B*N, 3*H*64] (Attention.forward,
 * vision_transformer.py:309-332), 1 <= N <= 512 (checked before anything is written).  out [B*N, H*64]; probs (stash), scores
 * and dscores (scratch) hold rmcl_attention_scratch_elems(B, H, N) ELEMENTS of their type each (probs, dscores: dtype; scores: fp32):
 * max(B*H*N*ldp, 2*B*H*NKP) with ldp = N rounded up to 8 and NKP = 64 / 128 / 192 / 256 for N <= 64 / 128 / 192 / 256.  With dtype
 * bf16, exact=0 and N <= 256 the fused flash-style kernels run: `probs` then holds only the per-row log-sum-exp, fp32 [B, H, NKP],
 * and the two-kernel backward keeps its delta, as many floats, in `scores` - the second term of the size, which is the larger one for
 * N <= 8.  Every other case materialises the [B, H, N, ldp] scores and probabilities (batched GEMM + softmax kernels).            */
int64_t rmcl_attention_scratch_elems(int B, int H, int N);
int rmcl_attention_fwd(const void* qkv, const int32_t* mask, void* out, void* probs, float* scores, int B, int N, int H,
                       int dtype, int exact, void* stream);
/* `out`: the forward's output (same buffer rmcl_attention_fwd wrote) - with it the bf16 path runs ONE backward kernel
 * (delta = rowsum(dO * O)); NULL selects the two-kernel form that recomputes delta from P and dP.                 */
int rmcl_attention_bwd(const void* qkv, const int32_t* mask, const void* probs, const void* dout, const void* out, void* dqkv,
                       float* scores, void* dscores, int B, int N, int H, int dtype, int exact, void* stream);
/* The same attention for bf16 storage at every 1 <= N <= 512 WITHOUT the [B, H, N, ldp] matrices: keys and values (backward: queries and
 * dO too) stream through LDS in blocks of 64 rows, online softmax in fp32 (csrc/attention_stream.hip).  Arguments as above without
 * dtype / exact; the buffers keep the sizes above.  The forward writes `out` and the per-row log-sum-exp, fp32 [B, H, NKP], into `probs`
 * (NKP = N rounded up to 64; rmcl_attention_stream_stat_elems = B * H * NKP floats, which rmcl_attention_scratch_elems bf16 elements always
 * hold); `scores` is not touched.  The backward recomputes P from that log-sum-exp, takes delta = rowsum(dO * O) from `out` (required),
 * keeps it in `scores` (as many floats) and writes dqkv; `dscores` is not touched.  dK / dV rows of masked keys are exactly zero, no
 * float atomics, identical bits run to run.  N outside 1..512 or a NULL argument returns -1 before anything is written.
 * rmcl_encoder_forward / _backward route their attention here when RMCL_MODE_STREAM_ATTN is set (above).                          */
int64_t rmcl_attention_stream_stat_elems(int B, int H, int N);
int rmcl_attention_stream_fwd(const void* qkv, const int32_t* mask, void* out, void* probs, float* scores, int B, int N, int H, void* stream);
int rmcl_attention_stream_bwd(const void* qkv, const int32_t* mask, const void* probs, const void* dout, const void* out, void* dqkv,
                              float* scores, void* dscores, int B, int N, int H, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RMCL_H */
