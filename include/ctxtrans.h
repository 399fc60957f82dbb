/*
 * ctxtrans.h -- C ABI of libctxtrans.so: the context-translation encoder/decoder
 * ("translator") of imitation_from_observation as hand-written HIP kernels for gfx950.
 *
 * The reference has no FFI for this path; its boundary is the TensorFlow feed/fetch contract used
 * at four call sites plus Saver.restore/save.  Every entry point below replaces one of them
 * (paths relative to the reference root):
 *
 *   ctx_create            Model().build(placeholder)            rllab/sampler/base.py:134-138,
 *                                                               scripts/train_script.py:118-121
 *   ctx_param_* / set / get   tf.train.Saver var list, restore/save   base.py:144-145,
 *                                                               train_script.py:133,181
 *   ctx_init_params       tf.global_variables_initializer       train_script.py:129
 *   ctx_translate         sess.run([translated_z, out], {image:[src,[ctx]*B,[ctx]*B]})
 *                                                               base.py:216-218
 *   ctx_encode            sess.run([input_z, image_trans], ...) base.py:234-235
 *   ctx_train_step        sess.run([optimizer, loss, simloss, recon1, recon2], ...)
 *                                                               train_script.py:163,167
 *   ctx_eval              sess.run([loss, simloss, recon1, recon2, out, out2], ...)
 *                                                               train_script.py:176,192-193
 *   ctx_dev_*             the same train step split into device-resident phases so a host can put
 *                         an RCCL gradient all-reduce between backward and Adam (new: the
 *                         reference has no multi-GPU path)
 *   ctx_dp_*              that all-reduce itself, on RCCL, behind this ABI (no torch needed)
 *   ctx_dev_forward_vjp / ctx_dev_backward_vjp / ctx_params_written
 *                         the translator as a differentiable function of its parameters and frames, for a
 *                         caller's own loss or a torch.autograd graph (new: the reference has no equivalent)
 *
 * Conventions: every function returns 0 on success or a negative CTX_E_* code; the message is
 * available from ctx_last_error().  No C++ exception crosses the ABI.  Host buffers are caller
 * owned and only touched during the call.  Layouts are the reference's: frames NHWC uint8 / f32,
 * parameters flat f32 in ctx_param_info order (TF variable names and shapes).  A handle is bound
 * to one device and is thread-compatible, not thread-safe (one caller at a time, like the single
 * tf.Session user).  There is NO CPU fallback: without a usable gfx950 device ctx_create fails.
 */
#ifndef CTXTRANS_H
#define CTXTRANS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTX_ABI_VERSION 4   /* 2: ctx_config carries strides / kernels / filters / keep_prob / loss_mode; 3: per-handle options,
                               ctx_dp_train_step_sampled / ctx_dp_eval_sampled, ctx_prof_entry.useful_frac; 4: ctx_dev_frames;
                               still 4 (additions only): ctx_vjp_args, ctx_dev_forward_vjp, ctx_dev_backward_vjp, ctx_params_written;
                               CTX_CNN_AVGPOOL_VALID / CTX_CNN_CONV_LINEAR, ctx_cnn_stats_*, ctx_cnn_reward_*; ctx_nn_err,
                               ctx_dp_nn_err, ctx_cnn_demos_upload, ctx_cnn_forward_sampled_dev; ctx_reward_costs_dev, ctx_reward_cache_*,
                               ctx_reward_get_cache, ctx_reward_stats, option reward_split; ctx_resize_*; the device-uint8 forms
                               ctx_resize_u8_dev / _v, ctx_cnn_*_dev_u8, ctx_disc_stream / _data_begin / _reward_paths_dev;
                               ctx_reconstruct / _f32 / _dev, ctx_reward_costs_recon / _dev;
                               ctx_set_grad_guard, ctx_grad_norm, ctx_grad_guard_stats; ctx_accum_* / ctx_dp_accum_*;
                               ctx_ema_*, ctx_get_ema, ctx_set_ema; ctx_tensor_stat, ctx_tensor_stats_* */

enum {
    CTX_OK = 0,
    CTX_E_INVALID = -1,   /* bad argument / unsupported configuration */
    CTX_E_DEVICE = -2,    /* HIP runtime error (no device, launch failure, ...) */
    CTX_E_NOMEM = -3,     /* device allocation failed */
    CTX_E_STATE = -4      /* call sequence error (e.g. adam before backward) */
};

enum {
    CTX_VARIANT_SKIPNEW = 0, /* ContextSkipNew, gym/envs/mujoco/arm_shaping.py:1260-1354 */
    CTX_VARIANT_INCEPTION2 = 2, /* ContextAEInception2(strides, kernels, filters), arm_shaping.py:1786-1894 (mode
                                   'oursinception').  ctx_config.strides / kernels / filters are the constructor's lists
                                   (:1787-1803: s1..s4, k1..k4, f1..f4; the decoder mirrors them); all-zero lists mean the
                                   sampler's instantiation strides [1,2,1,2], kernels [3,3,3,3], filters [16d,16d,8d,8d]
                                   (d = df_dim = 64: rllab/sampler/base.py:126).  Strides 1 | 2, kernels 1..5 (k x k),
                                   filters multiples of 32.  Inputs are Inception-v3 Mixed_7c FEATURE MAPS, f32
                                   [B, H, W, C] with C a multiple of 32 (2048; H = W = 2 for 125x125 frames, 8 for
                                   299x299); out = decode + tgtctx.  The uint8 entry points are refused: use *_f32. */
    CTX_VARIANT_REAL = 1     /* ContextAEReal, arm_shaping.py:1599-1684 (sampler names 'real', 'sweep'): shared
                                encoder, filters 32/16/16/8, strides 1/2/1/2; H, W multiples of 4, featsize (100)
                                a multiple of 4, df_dim ignored, keep_prob = 1 */
};

/* Arithmetic of the convolutions / linear layers (everything else -- epilogues, losses, reductions, Adam,
 * parameters, activations in HBM -- is f32 in every mode):
 *   CTX_PREC_F32     v_mfma_f32_32x32x2_f32: bitwise an fmaf chain.
 *   CTX_PREC_BF16X3  every f32 operand is split on the fly into bf16 hi + bf16 lo and a*b is evaluated as
 *                    hi*hi + hi*lo + lo*hi on the bf16 matrix cores with f32 accumulation: ~2^-16 relative error
 *                    per product, inside the 1e-3 budget of the path, at 16/3 the f32 matrix rate.
 *   CTX_PREC_FP16X3  the same three terms with fp16 hi + fp16 lo of x * 2^6 on the fp16 matrix cores (same rate), the
 *                    f32 accumulators rescaled by 2^-12: fp16's 11-bit significand makes the dropped lo*lo term
 *                    ~2^-22, so outputs and gradients are level with CTX_PREC_F32 (1e-6) -- inside a window of
 *                    operand magnitudes (operands = activations, weights, gradients: whatever a convolution or
 *                    linear layer multiplies).  Range contract:
 *                      small  f32-grade for |x| from about 1e-3 up to 1023.  Below, the error degrades gradually:
 *                             the absolute floor per operand is about 2^-24 / 64 (fp16's smallest subnormal over
 *                             the operand scale), e.g. relative 3e-6 for operands ~1e-4, 3e-4 for ~1e-6.
 *                      large  an operand with |x| * 64 >= 65520 (|x| >= 1023.75) becomes +-inf in its hi term: the
 *                             product is non-finite and the inf / NaN reaches the scalars or features of that
 *                             call.  A large operand never yields a wrong finite number.
 *                      after  such a call (here and in CTX_PREC_FP16X3D below, and in any mode after an inf / NaN in a frame)
 *                             the handle stays usable for INFERENCE calls, which change no state.  A TRAINING step
 *                             carries the non-finite gradient through Adam into every parameter and both moment
 *                             arenas -- unless ctx_set_grad_guard(skip_nonfinite) is set, under which that step
 *                             leaves parameters and moments untouched and the handle stays usable.
 *                    The scale 2^6 is fixed (CTX_PREC_FP16X3D is the form with per-operand scales).
 *   CTX_PREC_FP16X3D the three fp16 terms of CTX_PREC_FP16X3 with a power-of-two scale PER OPERAND of each product launch:
 *                    x * 2^e with e = 14 - floor(log2(largest |x| of that operand)), taken on the device in front of
 *                    the product (one extra read of both operands, one small launch; no host synchronisation, and a
 *                    replayed graph follows the data); the accumulators are rescaled by 2^-e_a and 2^-e_b, each an
 *                    exact multiply.  The largest entry of every operand lands in [2^14, 2^15).  Range contract:
 *                      f32-grade (level with CTX_PREC_F32, 1e-6) for operands of ANY finite magnitude: there is no
 *                             window to audit.  e is clamped to [-126, 126] so that 2^e and 2^-e are normal f32
 *                             values; the clamp binds only below a largest magnitude of 2^-112 (1.9e-34), where e
 *                             stays 126 and entries lose accuracy gradually as they approach the f32 subnormals.
 *                      inside one operand, entries below 2^-25 of its largest magnitude meet the fp16 subnormal floor
 *                             (absolute error 2^-39 of the largest entry per term: far below the f32 rounding of the
 *                             entries that dominate the sum).  One exponent per operand tensor; [decoder | skip]
 *                             operands share one.
 *                      zero   an all-zero operand takes e = 0: the product is exactly zero.
 *                      inf / NaN in an operand makes its scale NaN: every output of that launch is non-finite --
 *                             never a wrong finite number.
 *                    Exact f32 in every mode (inside every mode's contract; they are no operands of a split product): the 3-channel
 *                    family (c3conv, c3wgrad, convt3, convt3m: every layer that reads or writes the 3-channel frames) and the
 *                    filter gradients of the narrow direct path (dconv_wgrad_kernel / c3wgrad: their K is the pixel index and
 *                    their fragments are scalar LDS reads, so the split form of the forward kernel does not carry over).
 *                    ContextAEReal (CTX_VARIANT_REAL, W a multiple of 64) in a split mode, per launch:
 *                      split   h1..h3_conv forward, d_h1..d_h3 forward and the input gradients of all six (8 .. 32 input
 *                              channels): the split form of dconv_fwd_kernel (option dconv bit 16; fp16x3d: the scale of
 *                              [decoder | skip] is one exponent over both tensors, the filter's is taken per launch), and
 *                              every fully connected layer (implicit GEMM).
 *                      exact   h0_conv forward, d_h4 forward, d_h4's input gradient, the frame gradients of a VJP, and all
 *                              eight filter gradients.  With bit 16 cleared also the six layers above (the f32 direct kernel).
 *                      Option dconv bit 8 cleared (or W not a multiple of 64): every launch but the 3-channel ones is a
 *                      split implicit GEMM on channel-padded tensors, as before the narrow path existed for these modes.
 * Additions to the enum only: CTX_ABI_VERSION and the ctx_config layout are those of ABI 4. */
enum { CTX_PREC_F32 = 0, CTX_PREC_BF16X3 = 1, CTX_PREC_FP16X3 = 2, CTX_PREC_FP16X3D = 3 };

typedef struct ctx_config {
    int32_t variant;    /* CTX_VARIANT_* */
    int32_t H, W, C;    /* frame size; H, W multiples of 16 (arm_shaping.py:1314-1319); C == 3 */
    int32_t df_dim;     /* encoder/decoder base width (df_dim == gf_dim == 64 in the reference);
                           multiple of 32 */
    int32_t featsize;   /* 1024 in the reference (arm_shaping.py:1277); multiple of 32 */
    int32_t max_batch;  /* largest B any later call will pass */
    int32_t precision;  /* CTX_PREC_*: arithmetic of the matrix contractions (0 = exact f32, the default) */
    /* ---- ABI 2 (zero-initialise for the defaults) ---- */
    int32_t strides[4]; /* CTX_VARIANT_INCEPTION2: s1..s4 of the constructor (0,0,0,0 = 1,2,1,2) */
    int32_t kernels[4]; /*                          k1..k4 (0 = 3) */
    int32_t filters[4]; /*                          f1..f4 (0 = 16d,16d,8d,8d) */
    float keep_prob;    /* CTX_VARIANT_REAL: tf.nn.dropout keep probability of the TRAINING graph (arm_shaping.py:1637-1661; the
                           module-level default is 1.0, :1476; ablations_code/ablations.py:544 feeds 0.5).  0 or 1 = no dropout.
                           Inference fetches (ctx_translate / ctx_encode) and ctx_eval never drop (keep_prob = 1 is what the
                           sampler's graph has). */
    int32_t loss_terms; /* CTX_LOSS_* bits: which terms make up `loss`, i.e. what Adam minimises (0 = all three) */
} ctx_config;

/* `loss` of the training graph.  The reference's trainer minimises recon1 + recon2 + simloss (arm_shaping.py:1354); its ablation
 * script switches terms off (ablations_code/ablations.py:175-182, 278-285):  "None" = all (7),  "L2" = recon1 + recon2 (3),
 * "L2L3" = recon1 (1),  "L1" = recon2 + simloss (6).  All four scalars are reported whatever the mask. */
enum { CTX_LOSS_RECON1 = 1, CTX_LOSS_RECON2 = 2, CTX_LOSS_SIM = 4 };

typedef struct ctx_handle ctx_handle;

/* ---- lifetime ------------------------------------------------------------------------------ */
int ctx_abi_version(void);
/* Allocates everything on `device` with hipMalloc and creates a private stream. */
int ctx_create(const ctx_config* cfg, int device, ctx_handle** out);
/* Same, on caller-owned resources: `stream` is a hipStream_t (NULL = private stream), `arena` is
 * device memory of ctx_arena_bytes(cfg) bytes laid out [params | grads | adam_m | adam_v], each
 * ctx_param_total floats (NULL = allocate).  Lets a host framework own the gradient buffer it
 * hands to its collective library. */
int ctx_create_ex(const ctx_config* cfg, int device, void* stream, void* arena, ctx_handle** out);
void ctx_destroy(ctx_handle* h);
/* Message of the last failed call on `h` (or of the last failed ctx_create when h == NULL). */
const char* ctx_last_error(const ctx_handle* h);

/* ---- tuning switches, per handle ---------------------------------------------------------------
 * Every switch is an int.  A handle starts from the built-in defaults overridden by the environment variables CTX_<NAME> (upper
 * case) as they stand at ctx_create; ctx_set_option changes it for that handle only (two handles of one process may differ).
 * Names (ctx_option_count / ctx_option_name enumerate them):
 *   overlap     -1   1 = the step runs on three stream lanes (conv_context chain; filter / bias gradients beside the dx chain); 0 = one stream;
 *                    -1 = decided at create (off for the table-driven translators on maps under 64 positions) and reads back as 0 / 1
 *   graphs       1   the inference fetches at B <= 64 replay captured hipGraphs
 *   graph_lanes  1   ... with the stream lanes captured as graph branches (translate: the two encoders run side by side)
 *   posmajor     1   position-major convolutions (only the taps inside the grid) from 64 images up
 *   xcd_swizzle  7   bits: contiguous runs of work per XCD for 1 the position-major conv, 2 the transposed conv, 4 the filter gradient
 *   balance      9   bits: problem order of the position-major conv: 1 load-balanced runs on grids of <= 16 positions, 2 on larger grids,
 *                    8 Z-order (2-D compact) runs on larger grids instead (wins over 2); 4 load-balanced taps in the filter gradient
 *   wconvt      31   bits: 1 LDS-resident transposed conv, 2 / 4 row blocks on 4x4 / 8x8 grids, 8 column-uniform waves (4x4),
 *                    16 inference launches of <= 32 images as one product + a gather
 *   direct3     31   bits: 1 3-channel layers on the direct kernels, 2 c3conv, 4 c3wgrad, 8 d_h4 forward in one pass, 16 d_h4 forward on the
 *                    matrix cores at >= 128 images (convt3m.hip)  [fixed at create]
 *   dconv       59   bits: 1 ContextAEReal in f32 on the narrow-channel direct kernels, 2 the K-sliced LDS-DMA forward kernel (4: its four-class
 *                    launches too), 8 ContextAEReal in a split mode takes the narrow path (cleared: channel-padded implicit GEMM, 3 x the step),
 *                    16 its forward-type launches with >= 8 input channels use the split arithmetic (cleared: the exact-f32 direct kernel).
 *                    32 (in the default only) = bit 16 by mode: at create it is dropped, and with it bit 16 for CTX_PREC_FP16X3D handles
 *                    (measured slower there: profiles/precision_modes.txt), so a handle reads back 27 or 11; a stated value without bit 32
 *                    (CTX_DCONV=27) holds in every mode     [fixed at create]
 *   rchain       1   ContextAEReal's FC middle in three launches
 *   early_adam   1   Adam's slices beside the remaining backward in the fused ContextSkipNew steps (bit-identical; -0.06 ms)
 *   cnn_lanes   -1   Inception front end: branch lanes; -1 = in the split-bf16 mode only      (ctx_cnn handles: environment at create) [fixed at create]
 *   cnn_dconv    1   Inception front end (f32): layers of <= 32 input and output channels on the direct kernels (dconv.h); 0 = implicit GEMM  [fixed at create]
 *   cnn_stem4    1   Inception front end: the 3-channel first conv on the 4-channel gather    (ctx_cnn handles: environment at create) [fixed at create]
 *   trace_launch 0   one stderr line per distinct launch, `family | key value ...` (diagnostics, and how tests/test_gpu_ragged_routes.py and
 *                    tests/test_gpu_fp16x3d_ranges.py see which kernel a layer ran).  Families:
 *                      igemm          M N nprob chunks tile tiles nsplit swz  [loader A x loader B]   (gemm_launch.h: launch_igemm)
 *                      wconvt         form wc|wr, HS WS, NB (wc) or PB (wr), XS, ks, nimg, imgt = images per tile, c1 c2 nmod2 ca, blocks
 *                      convt3         form valu (S P NT TW ... ntiles grid nimg) or mfma (S KQH ... grid rounds nimg): d_h4's forward
 *                      c3conv         S NB TWB hin win ntiles grid nimg;   c3wgrad  S NB TWB two nmod2 hs ws ntiles nbl ngroups nimg
 *                      convt_product  M N cb ca (the starved inference route; its product is an igemm line as well)
 *                      dconv          CI N S span ncls taps hin win hlog wlog nimg fmt, then the tile choice: kernel fwd (TH TW MI NB occ slices) or
 *                                     fwd2 (TH TW MI NSL NB2 occ slices), tiles_y tiles_x ntiles grid   (dconv.hip: dconv_launch / dconv_launch2)
 *                      dconv_wgrad    CA CB CAK NB S TH TW two nmod2 hs ws tiles_y tiles_x ntiles nblk slices nimg
 *                    One set of seen lines per process; the other launchers (rchain.hip, elementwise) print nothing.
 *   adam_prio    2   HIP priority of the early-Adam stream (1 low: its own hardware queue; 0 normal; -1 high; 2 = low for exact-f32 handles,
 *                    normal for split-bf16 ones, reads back resolved)  [fixed at create]
 *   reward_split -1  the reward hook's image term (ctx_reward_costs / ctx_reward_costs_dev): -1 = the split kernel for frames of >= 32768
 *                    elements, 0 = always one block per frame, 1 = always split (frames of a multiple of 4 elements; measurements)
 * Results never depend on a switch beyond f32 summation order -- tested value by value (tests/test_gpu_options.py, against the default
 * switches on the bench's launch shapes; the defaults themselves are what every oracle suite runs):
 *   ContextSkipNew 64x64 B = 256:  overlap 0 | posmajor 0 | xcd_swizzle 0 1 2 3 4 5 6 | balance 0 1 2 3 4 5 8 13 | wconvt 0 1 3 5 7 15 23 29 |
 *                                  direct3 0 1 3 5 7 9 15 23 | early_adam 0 | adam_prio -1 0 1;  graph_lanes 0 1 and early_adam 0 1 also in
 *                                  tests/test_gpu_parity.py against the oracle
 *   ContextAEReal 36x64 B = 64:    overlap 0 1 | dconv 0 1 5 7 | rchain 0 | direct3 0 15 | posmajor 0;  dconv 3 11 27 in the three split modes against
 *                                  the oracle (tests/test_gpu_real_split.py: bits 8 and 16 choose kernels with different ARITHMETIC, each within its mode's bars)
 * Combinations of two non-default switches are not enumerated; cnn_* (front end) and graphs 0 run in their own suites' defaults only.
 * Not options: CTX_DEBUG_POISON=1 (debugging aid: every device
 * buffer a handle allocates is filled with 0xFF bytes -- float NaN -- so that a read of never-written memory shows on every run),
 * CTX_RCCL_LIB (path of the librccl to dlopen, read by the
 * first ctx_dp_* call of the process). */
int ctx_option_count(void);
const char* ctx_option_name(int index);                               /* NULL past the end */
int ctx_get_option(const ctx_handle* h, const char* name, int* value);
int ctx_set_option(ctx_handle* h, const char* name, int value);       /* CTX_E_INVALID: unknown name; CTX_E_STATE: fixed at create */

/* ---- parameter inventory (TF variable names) ------------------------------------------------ */
int64_t ctx_param_total_for(const ctx_config* cfg); /* number of f32 parameters, <0 on error */
int64_t ctx_arena_bytes(const ctx_config* cfg);     /* 4 * 4 * ctx_param_total_for */
int64_t ctx_param_total(const ctx_handle* h);
int ctx_param_count(const ctx_handle* h);           /* number of tensors */
/* name: e.g. "conv/h0_conv/w"; shape: up to 4 dims, unused = 1; offset: in floats into the arena */
int ctx_param_info(const ctx_handle* h, int index, const char** name, int* ndim, int64_t shape[4],
                   int64_t* offset);
int ctx_set_params(ctx_handle* h, const float* flat, size_t n);
int ctx_get_params(ctx_handle* h, float* flat, size_t n);
int ctx_get_grads(ctx_handle* h, float* flat, size_t n); /* gradient of the last backward */
/* Adam slots + step counter (Saver saves them too, train_script.py:133). */
int ctx_set_adam_state(ctx_handle* h, const float* m, const float* v, size_t n, int64_t step);
int ctx_get_adam_state(ctx_handle* h, float* m, float* v, size_t n, int64_t* step);
/* conv w: truncated normal(0.02); deconv w, FC Matrix: normal(0.02); biases 0
 * (arm_shaping.py:25-29, 52-55, 67-68, 79).  Also zeroes the Adam state. */
int ctx_init_params(ctx_handle* h, uint64_t seed);

/* ---- inference: the rllab reward hook's two fetches ------------------------------------------ */
/* translate(obs_src, obs_tgt0) -> (pred_frame, feat).
 * src  [B,H,W,3] uint8; ctx0 [H,W,3] uint8 (ctx_batched == 0, broadcast to B like base.py's
 * [context]*batch_size) or [B,H,W,3] (ctx_batched != 0).
 * pred [B,H,W,3] f32 = model.out; feat [B,featsize] f32 = model.translated_z.  Either may be NULL. */
int ctx_translate(ctx_handle* h, const uint8_t* src, const uint8_t* ctx0, int ctx_batched, int B,
                  float* pred, float* feat);
/* frames [B,H,W,3] uint8 -> feat [B,featsize] = model.input_z; frames_f32 (nullable) [B,H,W,3] =
 * image_trans[0] = (x/255 - 0.5)*2 -- the device's bits either way: up to 2^20 elements (the hook's batch of 25 and a few paths) they are written
 * by the host from the 256-entry table of the same three f32 operations while the device encodes (no download), beyond that copied back. */
int ctx_encode(ctx_handle* h, const uint8_t* frames, int B, float* feat, float* frames_f32);
/* The same two fetches on float inputs [B,H,W,C]: frames already scaled to [-1,1], or -- for
 * CTX_VARIANT_INCEPTION2, where image_trans IS the feature tensor (base.py:127-132) -- Mixed_7c feature maps. */
int ctx_translate_f32(ctx_handle* h, const float* src, const float* ctx0, int ctx_batched, int B,
                      float* pred, float* feat);
int ctx_encode_f32(ctx_handle* h, const float* frames, int B, float* feat);
/* ... and with the inputs already in DEVICE memory (d_*: f32 [B,H,W,C]; d_ctx0 [H,W,C] or, ctx_batched != 0, [B,H,W,C]), e.g. the
 * output buffer of ctx_cnn_forward_u8_dev on the same stream: mode 'oursinception' without a host round trip of the feature maps
 * (base.py:121-132, 216-218, 234-235).  pred / feat are HOST buffers (nullable). */
int ctx_translate_dev(ctx_handle* h, const float* d_src, const float* d_ctx0, int ctx_batched, int B, float* pred, float* feat);
int ctx_encode_dev(ctx_handle* h, const float* d_frames, int B, float* feat);

/* The per-path cost of the reward hook computed where the frames already are (base.py:232-249), several paths per call:
 * ctx_reward_set_cache keeps, per viewpoint vp, the demo cache  means [bs, featsize] (= self.means[vp]) and  imgs [bs,H,W,3]
 * (= self.imgs[vp])  on the device;  ctx_reward_costs encodes  frames [npaths*bs,H,W,3] uint8 (npaths rollouts of bs rendered
 * frames) and returns  costs[p*bs + j] = sum((means[j] - input_z[p,j])^2) + scale * sum((imgs[j] - image_trans[0][p,j])^2)
 * (ablation 0 = "None"; 1 = "nofeat": image term only; 2 = "noimage": feature term only).  Only npaths*bs floats come back
 * over PCIe instead of the preprocessed frames (49 MB at 40 paths). */
int ctx_reward_set_cache(ctx_handle* h, int vp, const float* means, const float* imgs, int bs);
int ctx_reward_costs(ctx_handle* h, int vp, const uint8_t* frames, int npaths, float scale, int ablation, float* costs);
/* For CTX_VARIANT_INCEPTION2 -- mode 'oursinception', where image_trans IS the feature tensor (base.py:132) -- ctx_reward_set_cache
 * takes  imgs [bs,H,W,C]  feature maps; ctx_reward_costs (uint8 frames) is refused there like the other uint8 entries.
 * ctx_reward_costs_dev: the same cost on frames that are ALREADY on the device:  d_frames  f32 [npaths*bs,H,W,C] -- frames in [-1,1]
 * for the pixel variants, Mixed_7c maps for CTX_VARIANT_INCEPTION2 (e.g. the output buffer of ctx_cnn_forward_u8_dev on the same
 * stream).  The `conv` encoder runs on a copy in the handle's own slot (not for ablation 1; no copy when d_frames is that slot,
 * ctx_dev_frames), the image term reads d_frames where they are; npaths*bs floats come back.  Stream contract of ctx_encode_dev:
 * d_frames must be complete in the handle's stream order; the call returns after the stream has drained.
 * Frames of >= 32768 elements (8x8x2048 maps at 299 x 299: 131072) take a split cost kernel -- one block per (frame, 8192-element
 * slice), the slices then added in order; smaller frames the one-block-per-frame kernel, in both entries. */
int ctx_reward_costs_dev(ctx_handle* h, int vp, const float* d_frames, int npaths, float scale, int ablation, float* costs);

/* The 'recon' ablation (launchers' ours_recon: ablation_type='recon'; base.py:250-252).  Its cost reads `image_recon`, which the reference
 * never assigns; its trainer and the commented lines base.py:238-241 say what it was: model.out2 of the per-path feed
 * [curimgs, [curimgs[0]]*bs, curimgs] -- the path's own frames through the `conv` encoder, decoded with the skips of the path's first
 * frame.
 * ctx_reconstruct*: out2 / input_z of the feed [frames, ctx, frames] (base.py:234-235 with the model's out2 fetched):
 *   frames [B,H,W,C]; nctx >= 1 divides B; row r uses context r / (B/nctx); ctx0 [nctx,H,W,C], or NULL = the first frame of each group
 *   ([curimgs[0]]*bs).  recon [B,H,W,C], feat [B,featsize]; either nullable.  Each context is encoded once; the translate MLP and
 *   decoder pass 1 do not run.  _f32: frames in [-1,1] / feature maps on the host; _dev: on the device (stream contract of
 *   ctx_encode_dev); results are HOST buffers.  The uint8 entry is refused for CTX_VARIANT_INCEPTION2 like the others.
 *   B % nctx != 0 or nctx outside [1, B]: CTX_E_INVALID.
 * ctx_reward_costs_recon*: costs[p*bs+j] = sum((means[j]-input_z[p,j])^2) + scale*sum((out2[p,j]-image_trans[0][p,j])^2), context =
 *   frame 0 of path p; only npaths*bs floats come back.  The feature term needs the viewpoint's demo cache (means): CTX_E_STATE before
 *   one exists.  One block per frame, or -- frames of >= 32768 elements, option reward_split as for ctx_reward_costs -- the split form;
 *   counted by ctx_reward_stats like any other cost call. */
int ctx_reconstruct(ctx_handle* h, const uint8_t* frames, const uint8_t* ctx0, int nctx, int B, float* recon, float* feat);
int ctx_reconstruct_f32(ctx_handle* h, const float* frames, const float* ctx0, int nctx, int B, float* recon, float* feat);
int ctx_reconstruct_dev(ctx_handle* h, const float* d_frames, const float* d_ctx0, int nctx, int B, float* recon, float* feat);
int ctx_reward_costs_recon(ctx_handle* h, int vp, const uint8_t* frames, int npaths, float scale, float* costs);
int ctx_reward_costs_recon_dev(ctx_handle* h, int vp, const float* d_frames, int npaths, float scale, float* costs);

/* The demo cache built on the device (base.py:195-223: translate every demo video into the rollout's context, np.mean over the
 * videos of translated_z and out) -- neither the translated frames / maps nor the finished cache cross PCIe:
 *   ctx_reward_cache_begin(h, vp, bs)      zeroed float64 sums [bs, featsize] and [bs, H*W*C] for viewpoint vp; again = reset.
 *                                          CTX_E_INVALID when vp already holds a cache of another bs.
 *   ctx_reward_cache_add_dev(h, vp, d_src, d_ctx0, nvideos)
 *                                          d_src f32 [nvideos*bs,H,W,C] and ONE context d_ctx0 [H,W,C] on the device (`[context] *
 *                                          batch_size`, base.py:217-218): one translate of nvideos*bs rows (<= max_batch), then
 *                                          sums[j] += translated_z / out of row v*bs + j, v = 0 .. nvideos-1 in order (float64).
 *   ctx_reward_cache_add(h, vp, src, ctx0, nvideos)   the same from host uint8 frames (pixel variants).
 *   ctx_reward_cache_finish(h, vp, nvideos_total, distributed)
 *                                          cache = f32(sums / nvideos_total), rounded once (np.mean(tfeats, axis=0), :221-222), written
 *                                          into the viewpoint's cache -- what ctx_reward_set_cache would have received.
 *                                          distributed != 0 (handle inside a ctx_dp_init group, else CTX_E_STATE; collective): the
 *                                          sums are first SUM-all-reduced in place over the ranks (ncclDouble), each rank having
 *                                          added its shard of the videos.  Ends the accumulation: add / finish need a new begin.
 *   ctx_reward_get_cache(h, vp, means, imgs)   host copies of the cache [bs, featsize] / [bs,H,W,C] (either nullable).
 * add / finish before begin: CTX_E_STATE.
 * ctx_reward_stats: counters of this handle's ctx_reward_* calls since create (tests read the PCIe property from them):
 *   [CTX_REWARD_STAT_D2H_BYTES] bytes of device-to-host copies issued, [.._COST_CALLS] cost calls, [.._SPLIT_LAUNCHES] /
 *   [.._PLAIN_LAUNCHES] cost calls that took the split / the one-block-per-frame kernel. */
#define CTX_REWARD_STAT_D2H_BYTES 0
#define CTX_REWARD_STAT_COST_CALLS 1
#define CTX_REWARD_STAT_SPLIT_LAUNCHES 2
#define CTX_REWARD_STAT_PLAIN_LAUNCHES 3
#define CTX_REWARD_NSTATS 4
int ctx_reward_cache_begin(ctx_handle* h, int vp, int bs);
int ctx_reward_cache_add_dev(ctx_handle* h, int vp, const float* d_src, const float* d_ctx0, int nvideos);
int ctx_reward_cache_add(ctx_handle* h, int vp, const uint8_t* src, const uint8_t* ctx0, int nvideos);
int ctx_reward_cache_finish(ctx_handle* h, int vp, int64_t nvideos_total, int distributed);
int ctx_reward_get_cache(ctx_handle* h, int vp, float* means, float* imgs);
int ctx_reward_stats(const ctx_handle* h, int64_t stats[CTX_REWARD_NSTATS]);

/* ---- training --------------------------------------------------------------------------------- */
/* src/ctx/tgt [B,H,W,3] f32 in [-1,1] (tfinput[0], [1], [2]).  scalars = {loss, simloss, recon1,
 * recon2} of the forward pass before the update.  Adam: TF defaults b1 .9, b2 .999, eps 1e-8. */
int ctx_train_step(ctx_handle* h, const float* src, const float* ctx, const float* tgt, int B,
                   float lr, float scalars[4]);
/* CTX_VARIANT_REAL with 0 < keep_prob < 1: seed of the dropout masks of the training entry points (ctx_train_step*,
 * ctx_dev_forward_backward, ctx_dp_train_step).  The factor of element e at dropout site s in the step that follows `t` Adam updates
 * is  (hash32(seed, t, s, e) < keep_prob * 2^32) / keep_prob  -- a counter-based hash (csrc/kernels.hip: drop_hash) that
 * oracle/ctx_oracle_real.py restates, so a step can be checked with the masks it used.  Default seed 0.  (TensorFlow's own random
 * stream is not reproducible from outside; tf.nn.dropout's arithmetic x * mask / keep_prob is.)  After ctx_dp_init rank r hashes with
 * seed ^ (0x9E3779B9 * r), so the shards of a data-parallel batch draw different masks (rank 0 keeps the single-device masks). */
int ctx_set_dropout_seed(ctx_handle* h, uint64_t seed);
/* Same on uint8 frames, preprocessed on device with (x/255 - 0.5)*2. */
int ctx_train_step_u8(ctx_handle* h, const uint8_t* src, const uint8_t* ctx, const uint8_t* tgt,
                      int B, float lr, float scalars[4]);
/* The trainer's input pipeline on device (scripts/train_script.py:144-159).  ctx_demos_upload keeps the demo
 * tensor vdata[T][N][H][W][3] (uint8 frames, T frames of N videos) resident in HBM; ctx_train_step_sampled
 * builds the batch  src[b] = vdata[b % T][choicesrc[b]], tgt[b] = vdata[b % T][choicetgt[b]],
 * ctx[b] = vdata[0][choicetgt[b]]  with the trainer's x/127.5 - 1 scaling and runs one train step.  The two
 * index arrays are what `np.random.choice(ntrain, batch_size)` returns (:154-155). */
int ctx_demos_upload(ctx_handle* h, const uint8_t* vdata, int T, int N);
int ctx_train_step_sampled(ctx_handle* h, const int32_t* choicesrc, const int32_t* choicetgt, int B,
                           float lr, float scalars[4]);
/* The validation batch of the trainer (train_script.py:169-176) from the resident demo tensor: the same gather as
 * ctx_train_step_sampled, forward + losses, no update.  out / out2 (nullable) [B,H,W,3]. */
int ctx_eval_sampled(ctx_handle* h, const int32_t* choicesrc, const int32_t* choicetgt, int B, float scalars[4],
                     float* out, float* out2);
/* Host copies of model.out / model.out2 [B,H,W,3] of the last training-mode forward and of the tgt frames it was fed
 * (tfinput[2]) -- what the trainer's `nn_err` fetch reads next to the optimizer (train_script.py:148,163).  Any may be NULL. */
int ctx_last_outputs(ctx_handle* h, float* out, float* out2, float* tgt);
/* The trainer's nn_err (train_script.py:148) of the last training-mode forward, computed where the maps are: rows of model.out against
 * the tgt slot it was fed,  *err = sum_b | argmin_i mean((tgt_i - out_b)^2) - ((j0 + b) % nlen) |  with the distances accumulated in
 * f64 and the FIRST index of least distance on ties (np.argmin).  j0: the first global row of these outputs (a data-parallel shard's
 * share).  Any variant (npi = H*W*C a multiple of 4).  Synchronous. */
int ctx_nn_err(ctx_handle* h, int nlen, int j0, int64_t* err);
/* Forward + losses only.  out / out2 (nullable) [B,H,W,3]. */
int ctx_eval(ctx_handle* h, const float* src, const float* ctx, const float* tgt, int B,
             float scalars[4], float* out, float* out2);

/* ---- device-resident phases (benchmarks, data parallel) -------------------------------------- */
/* d_* are DEVICE pointers [B,H,W,3] f32.  Enqueues forward + backward on the handle's stream and
 * returns without synchronising.  sim_batch: batch in the simloss mean's denominator (0 = B); a
 * data-parallel shard passes the GLOBAL batch so a SUM all-reduce of the gradient arena equals the
 * full-batch gradient. */
int ctx_dev_forward_backward(ctx_handle* h, const float* d_src, const float* d_ctx,
                             const float* d_tgt, int B, int sim_batch);
/* The handle's own frame buffer for a batch of B: the device entry points (ctx_dev_*, ctx_dp_train_step) copy the caller's three
 * tensors into it (3 B frames device-to-device per step) -- unless a pointer passed to them IS the one returned here, i.e. the caller
 * (a device-side sampler, a front end) wrote that slot in place.  The pointers depend on B (slots are packed [tgt | src | ctx]). */
int ctx_dev_frames(ctx_handle* h, int B, float** d_src, float** d_ctx, float** d_tgt);
int ctx_dev_forward(ctx_handle* h, const float* d_src, const float* d_ctx, const float* d_tgt,
                    int B);
/* One whole training step on device-resident frames: forward + backward + Adam (train_script.py:163's
 * sess.run([..., optim]) without the host copies), enqueued on the handle's stream, no synchronisation.
 * Same result, bit for bit, as ctx_dev_forward_backward(sim_batch = 0) followed by ctx_dev_adam(lr).  With
 * option "early_adam" set, Adam's update of a parameter slice is enqueued beside the remaining
 * backward as soon as that slice's gradients are final and its parameters are no longer read (on by default:
 * -0.06 ms of 13.1 on MI355X; bit-identical either way).  The host-fed steps (ctx_train_step, _u8, _sampled)
 * go through the same code. */
int ctx_dev_train_step(ctx_handle* h, const float* d_src, const float* d_ctx, const float* d_tgt, int B,
                       float lr);
/* Fused multi-tensor Adam over the whole arena with the gradients currently in the grad arena. */
/* Data-parallel overlap (new; the reference is single-device).  When set, ctx_dev_forward_backward calls fn(user, 0, first,
 * count) on the calling thread as soon as gradients [first, first + count) of the gradient arena -- translate/ and deconv/,
 * the tail of the arena -- are complete in the handle's stream order; the caller starts their all-reduce there (ordered
 * after the handle's stream) while the encoders' backward is still being enqueued, and reduces [0, first) after the call
 * returns.  fn == NULL clears it. */
typedef void (*ctx_bucket_fn)(void* user, int bucket, int64_t first, int64_t count);
int ctx_set_grad_bucket_callback(ctx_handle* h, ctx_bucket_fn fn, void* user);
int ctx_dev_adam(ctx_handle* h, float lr);
/* ---- guarded Adam: gradient norm, clip-by-global-norm, skip of a non-finite step, all on the device ----
 * With a guard set, every Adam update of this handle (ctx_train_step*, ctx_dev_train_step, ctx_dev_adam, ctx_dp_train_step*) is
 * preceded by one more pass over the gradient arena on the same stream: sum of g^2 in f64 over every float the backward writes
 * (the square of an f32 is exact in f64 and a finite f32 gradient cannot overflow the f64 sum: the sum is non-finite if and only if
 * some gradient element is), summed in a fixed order that depends on neither the device nor the batch.  From it, on the device:
 *   norm    = sqrt(sum)
 *   factor  = 1 exactly when clip_norm == 0 or norm <= clip_norm (such a step is bit-identical to the unguarded one), else
 *             (float)(clip_norm / norm) with the division in f64: tf.clip_by_global_norm's  g * clip / max(norm, clip)
 *   apply   = 0 if skip_nonfinite is set and the sum is non-finite, else 1.  With skip_nonfinite clear a non-finite sum gives
 *             factor = 1, apply = 1: the unguarded behaviour, poison included.
 * Adam then reads factor and apply from device memory: apply == 0 reads and writes nothing -- parameters, m and v stay as they were;
 * otherwise it updates with g * factor.  Nothing returns to the host: a guarded ctx_dev_train_step stays asynchronous.
 *   - The factor exists only after the last gradient is written, so under a guard the early Adam slices are not used, whatever option
 *     "early_adam" says (its value is not changed).
 *   - The step counter behind the bias correction (and the dropout mask step) is host state and advances on a SKIPPED step too: the
 *     host cannot know of the skip without synchronising.  steps_skipped is the correction for a caller that wants the number of
 *     applied steps; the scalars of a skipped step are non-finite.
 *   - Data parallel: the norm is taken on the all-reduced gradient, so every rank computes the same norm, factor and skip decision
 *     (no extra collective) and replicas stay bit-identical; one rank's NaN makes all ranks skip.
 * clip_norm == 0: no clipping; clip_norm == 0 and skip_nonfinite == 0: no guard (the default; no extra launch).  NaN or negative
 * clip_norm: CTX_E_INVALID.  Setting a guard resets the counters. */
int ctx_set_grad_guard(ctx_handle* h, float clip_norm, int skip_nonfinite);
/* The global norm of the gradients now in the gradient arena, whether a guard is set or not (the guard's statistics are not touched).
 * CTX_E_STATE before any backward.  Synchronises the stream. */
int ctx_grad_norm(ctx_handle* h, double* norm);
/* norm and factor of the last guarded step and the counts of skipped / clipped steps since ctx_set_grad_guard (zeros before the
 * first).  Synchronises the stream.  Any pointer may be NULL. */
int ctx_grad_guard_stats(ctx_handle* h, double* last_norm, float* last_factor, int64_t* steps_skipped, int64_t* steps_clipped);
/* ---- training a subset of the parameters: one learning-rate scale per tensor (the trainer's var_list, train_script.py:126-128) ----
 * scale[i] multiplies lr for tensor i of ctx_param_info (n == ctx_param_count(h)); 0 = frozen.  scale == NULL (n ignored) or every
 * scale 1 = no mask, the default: every launch is then the one of a handle that never called this.  CTX_E_INVALID: NULL handle, wrong
 * n, a negative or non-finite scale.  The mask is handle state; checkpoints do not hold it.  It covers every Adam update of the handle
 * (ctx_train_step*, ctx_dev_train_step, ctx_dev_adam, ctx_dp_train_step*), in ONE launch per step whatever the mask:
 *   - scaled tensor: today's Adam at lr_i = lr * scale[i], the product taken in f32 and lr_t formed from lr_i as it is from lr --
 *     bit for bit the update of an unmasked handle stepped at (float)(lr * scale[i]) from the same state and gradient.
 *   - frozen tensor: parameter, m and v keep every bit; no kernel of the update touches their memory.  The step counter is global and
 *     advances: a tensor unfrozen later continues from its stale moments with the current bias correction (a TensorFlow graph with a
 *     fixed var_list cannot unfreeze at all).
 *   - guard (ctx_set_grad_guard, ctx_grad_norm): the norm, and with it the clip factor and the skip decision, is taken over the
 *     trainable tensors only -- a NaN in a gradient no trainable tensor uses does not skip the step.
 *   - ctx_get_grads returns exact zeros for a frozen tensor.  What ctx_dev_grads points at inside a frozen tensor's range is
 *     UNSPECIFIED: a plain backward (ctx_dev_forward_backward, the fused steps, ctx_profile_step) leaves out every launch whose
 *     results reach no trainable tensor's gradient -- filter / bias gradients of frozen tensors, input-gradient chains that end in
 *     frozen tensors only -- so that range may hold an older step's values.  The launches that do run are the unmasked step's and the
 *     trainable gradients are bit-identical.
 *   - under a mask the early Adam slices are not used, as under a guard.
 *   - data parallel (ctx_dp_train_step*, a handle after ctx_dp_init) and under ctx_set_grad_bucket_callback the backward stays whole
 *     and the buckets are unchanged; the mask applies to Adam and to the norm of the reduced gradient.
 *   - ctx_dev_backward_vjp ignores the mask: frame and code gradients need the whole chain. */
int ctx_set_param_lr_scale(ctx_handle* h, const float* scale, int n);
int ctx_get_param_lr_scale(const ctx_handle* h, float* scale, int n);
/* ---- decoupled weight decay: one rate per tensor (Loshchilov & Hutter's AdamW, torch.optim.AdamW) ----
 * decay[i] = lambda of tensor i of ctx_param_info (n == ctx_param_count(h)).  decay == NULL (n ignored) or every rate 0 = off, the
 * default: every launch is then the one of a handle that never called this.  CTX_E_INVALID: NULL handle, wrong n, a negative or
 * non-finite rate.  Like ctx_set_param_lr_scale it never answers CTX_E_STATE: the rates only take effect at the next Adam update, also
 * when set inside an open accumulation or while the averaged weights are swapped in.  The rates are handle state; checkpoints do not hold them.
 * They cover every Adam update of the handle (ctx_train_step*, ctx_dev_train_step, ctx_dev_adam, ctx_accum_adam, ctx_dp_train_step*),
 * in ONE launch per step, inside the Adam pass -- no further traffic.  Per element, with lr_i = (float)(lr * scale[i]) and
 * d = (float)(lr_i * decay[i]), both products taken in f32:
 *     m' = b1 m + (1 - b1) g ;  v' = b2 v + (1 - b2) g g          (as without; g already times the clip factor under a guard)
 *     q  = d != 0 ? fmaf(-d, p, p) : p                             (ONE rounding)
 *     p' = q - lr_t m' / (sqrt(v') + eps)                          (lr_t: the bias-corrected rate formed from lr_i, as without)
 *   - d is formed from the RAW rate lr_i, not from lr_t (torch's convention), so the decay follows a learning-rate schedule by
 *     itself.  It acts on the parameter as it was before the step; it is not part of the gradient, so it enters neither m nor v.
 *     (Coupled L2, lambda p added to g, is NOT offered.)
 *   - a tensor at decay 0 inside a decayed step is updated bit for bit as on a handle without decay, -0 and non-finite values
 *     included; m and v of EVERY tensor are those of the undecayed step.
 *   - guard (ctx_set_grad_guard): the clip factor scales g only, never the decay; norm, factor and skip decision are bit for bit the
 *     undecayed handle's.  A step the guard skips does not decay.
 *   - mask (ctx_set_param_lr_scale): a scaled tensor decays at lr_i -- bit for bit the update of an unmasked handle stepped at
 *     (float)(lr * scale[i]) with the same lambda.  A frozen tensor is not decayed and keeps every bit of p, m and v, whatever its
 *     lambda.  Decay alone does NOT make a handle masked: the backward stays whole, the guard's norm, the accumulation and the average
 *     keep their dense extent and ctx_get_grads is unchanged.
 *   - the early Adam slices are not used, as under a guard or a mask (the value of option "early_adam" is not changed).
 *   - accumulation (ctx_accum_*): one decay per UPDATE, not per micro-batch.  Average (ctx_ema_*): follows the decayed parameters.
 *   - statistics (ctx_tensor_stats_*): unchanged; u stays the Adam term lr_t m / (sqrt(v) + eps).  The decay's own step is d |p|.
 *   - data parallel: every rank must set the same rates, as with the mask; the update is deterministic, replicas stay bit-identical.
 *   - channel pads and the floats between two tensors are exact zeros and stay exact zeros (fmaf(-d, 0, 0) = +0).
 *   - ctx_dev_forward_vjp / ctx_dev_backward_vjp ignore the rates: they compute gradients, not updates. */
int ctx_set_param_weight_decay(ctx_handle* h, const float* decay, int n);
int ctx_get_param_weight_decay(const ctx_handle* h, float* decay, int n);
/* Synchronises and copies {loss, simloss, recon1, recon2} of the last forward. */
int ctx_dev_scalars(ctx_handle* h, float scalars[4]);
/* Device pointer to the parameters (flat, ctx_param_info order).  WRITABLE: a caller may update the weights through it (its own
 * optimiser, a torch-side broadcast) on ctx_stream(h) or after ctx_sync(h).  The library cannot see such writes, so from the first call
 * on it stops trusting filters it packed earlier for the direct kernels (ContextAEReal / the front end): they are re-packed in front of
 * every launch, and inference graphs captured before the call are dropped.  Handles that never call it keep the packed-filter cache. */
void* ctx_dev_params(ctx_handle* h);
void* ctx_dev_grads(ctx_handle* h);      /* (inside a frozen tensor's range the contents are unspecified: ctx_set_param_lr_scale) */
void* ctx_dev_scalar_buf(ctx_handle* h); /* device f32[4] written by the last forward */
void* ctx_stream(ctx_handle* h);         /* hipStream_t the kernels are enqueued on */
int ctx_sync(ctx_handle* h);
/* Device outputs of the last forward (valid until the next call): model.out / out2 [B,H,W,3],
 * input_z / translated_z [B,featsize]. */
int ctx_dev_outputs(ctx_handle* h, const float** out, const float** out2, const float** input_z,
                    const float** translated_z);
/* Host copies of model.input_z / model.translated_z [B, featsize] (arm_shaping.py:1298, :1312) of the last training-mode
 * forward (ctx_eval / ctx_train_step* / ctx_dev_forward*), i.e. sess.run([..., input_z, translated_z], feed) next to the
 * losses; rows are de-padded (the device keeps them at a stride of featsize rounded up to 32 for CTX_VARIANT_REAL).
 * Either pointer may be NULL; *B (nullable) receives the batch of that forward. */
int ctx_last_codes(ctx_handle* h, float* input_z, float* translated_z, int* B);

/* ---- vector-Jacobian products: the translator under a caller's loss (new: the reference has no equivalent) ---------
 * ctx_dev_forward_vjp runs the training-mode forward of ctx_dev_forward (frames, outputs and scalars alike) and keeps its
 * activations for ONE later ctx_dev_backward_vjp, identified by *token.  dropout != 0 applies the training graph's dropout masks
 * (CTX_VARIANT_REAL with keep_prob < 1; ignored otherwise); drop_step is the `t` of the mask hash (ctx_set_dropout_seed), -1 = the
 * handle's Adam step count, i.e. the masks ctx_dev_forward_backward would draw.  Asynchronous on the handle's stream. */
int ctx_dev_forward_vjp(ctx_handle* h, const float* d_src, const float* d_ctx, const float* d_tgt, int B, int dropout,
                        int64_t drop_step, uint64_t* token);
/* Cotangents of a VJP.  All pointers are DEVICE pointers and may be NULL: an input NULL means a zero cotangent, an output NULL
 * skips that frame gradient's launches.  d_out / d_out2 and the frame gradients are [B,H,W,C]; d_input_z / d_translated_z are
 * dense [B, featsize] (the library handles the padded row stride of CTX_VARIANT_REAL).  loss_weight is the cotangent of the
 * scalar `loss` (the handle's loss_terms); sim_batch as in ctx_dev_forward_backward (0 = B). */
typedef struct ctx_vjp_args {
    const float* d_out;
    const float* d_out2;
    const float* d_input_z;
    const float* d_translated_z;
    float loss_weight;
    int sim_batch;
    float* d_src_frames;
    float* d_ctx_frames;
    float* d_tgt_frames;
} ctx_vjp_args;
/* The backward of the forward `token` names, seeded with  d out = loss_weight * d loss / d out + [d_out ; d_out2]  and
 * d translated_z = loss_weight * d loss / d translated_z + d_translated_z  (d_input_z joins the gradient of input_z).  Parameter
 * gradients OVERWRITE the gradient arena (ctx_dev_grads) as ctx_dev_forward_backward's do; frame gradients go to the caller's
 * buffers.  No Adam, no bucket callback, no host synchronisation.  With loss_weight = 1 and no cotangents the gradient arena is
 * bit-identical to ctx_dev_forward_backward's.  A token is good for ONE backward: any later forward or backward (this call
 * included -- a second VJP on the same token, torch's retain_graph) overwrites the activations and returns CTX_E_STATE. */
int ctx_dev_backward_vjp(ctx_handle* h, uint64_t token, const ctx_vjp_args* a);
/* The caller has changed parameters through ctx_dev_params: packed filters of the direct kernels and captured inference graphs
 * made from the old values are dropped (re-packed / re-captured at their next use).  Cheap: call it after every external update. */
int ctx_params_written(ctx_handle* h);

/* ---- data parallel over RCCL (new: the reference is single-device) ------------------------------
 * One process per GPU, each with a full replica + Adam state; per step: local forward/backward on the rank's shard with
 * the simloss mean taken over the GLOBAL batch -> SUM all-reduce of the flat f32 gradient arena over xGMI -> identical
 * local Adam.  librccl is loaded at run time on the first ctx_dp_* call (CTX_RCCL_LIB overrides the search; a process
 * that already holds a librccl.so.1 -- PyTorch's -- shares it).
 *   ctx_dp_unique_id      rank 0 makes the rendezvous blob (an ncclUniqueId); the host ships it to the other ranks
 *   ctx_dp_init           collective: creates the communicator on the handle's device, then broadcasts rank 0's parameters
 *                         and Adam slots so the replicas start identical
 *   ctx_dp_allreduce_grads  the exchange step alone: in-place SUM all-reduce of the gradient arena, stream-ordered between
 *                         ctx_dev_forward_backward(sim_batch = B * world) and ctx_dev_adam (asynchronous)
 *   ctx_dp_train_step     the whole step with the bucketed schedule: the translate/deconv gradients, then each encoder's
 *                         h4_lin / hz_lin slice, are reduced on a second stream while the encoders' backward still runs;
 *                         only the encoders' conv filters (18 % of the arena) go after it; then Adam.  scalars (nullable) =
 *                         GLOBAL {loss, simloss, recon1, recon2} (one more 16-byte all-reduce and a sync).  d_* are DEVICE
 *                         pointers [B,H,W,3] f32 -- for CTX_VARIANT_INCEPTION2 handles the Mixed_7c maps [B,h,w,C] f32, e.g.
 *                         the three slices of ctx_cnn_forward_sampled_dev's output; every rank passes the same B.
 *   ctx_dp_scalars        global scalars of the last forward (collective) */
#define CTX_DP_UNIQUE_ID_BYTES 128
int ctx_dp_unique_id(uint8_t id[CTX_DP_UNIQUE_ID_BYTES]);
int ctx_dp_init(ctx_handle* h, const uint8_t id[CTX_DP_UNIQUE_ID_BYTES], int rank, int world);
int ctx_dp_world(const ctx_handle* h, int* rank, int* world);   /* (rank 0, world 0) before ctx_dp_init */
int ctx_dp_allreduce_grads(ctx_handle* h);
int ctx_dp_train_step(ctx_handle* h, const float* d_src, const float* d_ctx, const float* d_tgt, int B, float lr,
                      float scalars[4]);
int ctx_dp_scalars(ctx_handle* h, float scalars[4]);
/* The trainer's loop on N GPUs without a host gather (scripts/train_script.py:153-167 + SURVEY.md 8e / 8f-3): every rank holds the
 * whole demo tensor in HBM (ctx_demos_upload) and is handed the SAME global index arrays choicesrc / choicetgt [B_global]
 * (np.random.choice(ntrain, batch_size) twice, :154-155; B_global a multiple of the world size, B_global / world <= max_batch).
 * Rank r gathers rows b in [r B/world, (r+1) B/world) of the global batch on the device -- src[b] = vdata[b % T][choicesrc[b]],
 * tgt[b] = vdata[b % T][choicetgt[b]], ctx[b] = vdata[0][choicetgt[b]], b the GLOBAL row -- and runs ctx_dp_train_step's bucketed
 * schedule on them: N ranks leave the parameters a single handle's ctx_train_step_sampled leaves on the same arrays (up to f32
 * summation order).  scalars (nullable): the GLOBAL {loss, simloss, recon1, recon2}.
 * ctx_dp_eval_sampled: the validation fetch (:169-176) sharded the same way -- forward + losses on this rank's rows, GLOBAL scalars
 * (collective: every rank must call it), out / out2 (nullable) = THIS RANK's rows [B_global / world, H, W, 3]. */
int ctx_dp_train_step_sampled(ctx_handle* h, const int32_t* choicesrc, const int32_t* choicetgt, int B_global, float lr,
                              float scalars[4]);
int ctx_dp_eval_sampled(ctx_handle* h, const int32_t* choicesrc, const int32_t* choicetgt, int B_global, float scalars[4], float* out,
                        float* out2);
/* In-place SUM over the ranks of a HOST buffer of doubles (synchronous; through a device staging buffer and ncclAllReduce
 * on the handle's collective stream).  For the sharded demo cache of the reward hook (sampler/base.py:195-223 builds it on
 * one device; reward.py shards the demo videos rank::world and adds the partial feature / frame sums): the group that
 * ctx_dp_init made serves it, no second communication library in the sampler process. */
int ctx_dp_allreduce_host_f64(ctx_handle* h, double* buf, size_t n);
/* ctx_nn_err of the GLOBAL batch (collective: every rank must call it, after the same training-mode forward on its shard): every rank's
 * outputs against the tgt rows of ALL ranks.  The tgt slots are all-gathered as a SUM all-reduce of a zero-filled [B_global, npi] buffer
 * in which each rank wrote its own rows (exact: one non-zero contributor per element), rank r's share is taken with j0 = r * B, and
 * the shares are summed.  *err is the same on every rank. */
int ctx_dp_nn_err(ctx_handle* h, int nlen, int64_t* err);

/* ---- gradient accumulation: ONE Adam step from several micro-batches (new: the reference steps on what one feed carries) ----------
 * A step whose batch is larger than max_batch.  A data-parallel step is a sum of shard gradients with the simloss mean over the
 * global batch; the same arithmetic in micro-batches on one handle:
 *   ctx_accum_begin(h, total)                      opens an accumulation of `total` triples (resets the rows seen, the scalar sums and
 *                                                  the micro-batch ordinal); total = 0 cancels an open one.  Under ctx_dp_init `total`
 *                                                  is the GLOBAL batch over all ranks (a multiple of the world size) and this handle
 *                                                  adds total / world rows.  The first call allocates the accumulator, one more
 *                                                  buffer of the parameters' size BESIDE the arena (caller-supplied arenas and
 *                                                  ctx_arena_bytes are unchanged); it is freed with the handle.
 *   ctx_accum_dev_forward_backward(h, s, c, t, B)  one micro-batch, B <= max_batch, sizes may differ: the training-mode forward and
 *                                                  the backward of ctx_dev_forward_backward(sim_batch = total) -- pruned under a mask
 *                                                  as a plain backward is, no bucket callback -- and its gradient joins the sum.
 *                                                  CTX_E_STATE when the rows seen would exceed the handle's share.  Asynchronous.
 *   ctx_accum_adam(h, lr, scalars)                 CTX_E_STATE unless every row has been seen.  Writes the sum into the gradient arena
 *                                                  and runs the Adam update of ctx_dev_adam on it; the step count advances by ONE and
 *                                                  the accumulation is closed.  scalars (nullable; non-NULL synchronises): {loss,
 *                                                  simloss, recon1, recon2} of the whole batch -- recon sums add, simloss is the
 *                                                  mean weighted by rows / total, loss is formed from the handle's loss_terms; they
 *                                                  are also what ctx_dev_scalars returns afterwards.
 *   ctx_dp_accum_adam(h, lr, scalars)              the same on a handle after ctx_dp_init, with ONE SUM all-reduce of the gradient
 *                                                  arena between the sum and Adam (collective); scalars: the GLOBAL ones.
 *   ctx_accum_state(h, &rows_seen, &total)         rows this handle has added and the announced total (0 = none open).
 * The sum: the gradient arena ends up holding ((g1 + g2) + ...) + gk, g_j the gradient ctx_dev_forward_backward(sim_batch = total)
 * gives for micro-batch j -- one plain f32 add per element and micro-batch in that order, the same bits on every run.  The last
 * micro-batch's gradient is not copied: it waits in the gradient arena, where ctx_accum_adam adds the sum of the others to it, so
 * nothing may overwrite the gradient arena between the last micro-batch and ctx_accum_adam.  An accumulation of ONE micro-batch is
 * ctx_dev_forward_backward + ctx_dev_adam bit for bit and launch for launch.  Afterwards ctx_get_grads / ctx_grad_norm see the
 * gradient Adam consumed.
 *   - guard (ctx_set_grad_guard): the norm, the clip and the non-finite skip act on the SUM; one NaN micro-batch skips the whole step
 *     and leaves parameters and moments untouched.
 *   - mask (ctx_set_param_lr_scale): the sum runs over the trainable tensors only; frozen floats of the accumulator and of the
 *     gradient arena are neither read nor written.
 *   - dropout (CTX_VARIANT_REAL, keep_prob < 1): the Adam step count does not move between micro-batches, so micro-batch j mixes its
 *     ordinal j into the mask seed (as a data-parallel rank is mixed in); j = 0 leaves the seed alone.  Later micro-batches draw
 *     masks of their own -- a host loop over ctx_dev_forward_backward would draw the SAME masks k times.
 *   - while an accumulation is open every other Adam update (ctx_dev_adam, ctx_train_step*, ctx_dev_train_step, ctx_dp_train_step*,
 *     ctx_profile_step) returns CTX_E_STATE; inference, ctx_eval* and the VJP calls stay allowed (a VJP backward overwrites the
 *     gradient arena: not behind the last micro-batch).
 * The trainer's entry: ctx_accum_train_step_sampled is ctx_train_step_sampled on a batch of B_total rows in micro-batches of micro_B
 * (<= max_batch; the last may be short).  Indices are checked over all B_total rows first; micro-batch j gathers rows [j micro_B, ...)
 * with t = b % T taken on the row b of the WHOLE batch, so the frames are those of one B_total-row gather.  nn_err (nullable; nlen > 0):
 * the trainer's nn_err of the whole batch -- every micro-batch's outputs against the tgt rows of ALL B_total rows -- summed on the
 * device.  ctx_dp_accum_train_step_sampled: rank r takes rows [r B_total / world, ...) of the same global arrays in micro-batches,
 * one all-reduce per step; scalars and nn_err are global and the same on every rank (collective: every rank must call it).
 * Synchronous like ctx_train_step_sampled. */
int ctx_accum_begin(ctx_handle* h, int total_batch);
int ctx_accum_dev_forward_backward(ctx_handle* h, const float* d_src, const float* d_ctx, const float* d_tgt, int B);
int ctx_accum_adam(ctx_handle* h, float lr, float scalars[4]);
int ctx_dp_accum_adam(ctx_handle* h, float lr, float scalars[4]);
int ctx_accum_state(const ctx_handle* h, int* rows_seen, int* total_batch);
int ctx_accum_train_step_sampled(ctx_handle* h, const int32_t* choicesrc, const int32_t* choicetgt, int B_total, int micro_B, float lr,
                                 float scalars[4], int nlen, int64_t* nn_err);
int ctx_dp_accum_train_step_sampled(ctx_handle* h, const int32_t* choicesrc, const int32_t* choicetgt, int B_total, int micro_B,
                                    float lr, float scalars[4], int nlen, int64_t* nn_err);

/* ---- exponential moving average of the parameters, kept on the device (new here; tf.train.ExponentialMovingAverage) ---------------
 * An averaged copy ("shadow") of the parameters beside the arena, updated by ONE launch behind every Adam update of the handle --
 * ctx_train_step*, ctx_dev_train_step, ctx_dev_adam, ctx_dp_train_step*, ctx_accum_adam / ctx_dp_accum_adam and the accumulated
 * sampled steps (once per Adam update, not per micro-batch).  Off by default: a handle that never enables it runs exactly the
 * launches of one that has never heard of it.
 *   ctx_ema_enable(h, decay, warmup)   decay in [0, 1], else (NaN included) CTX_E_INVALID.  The first call allocates the shadow -- one
 *                                      buffer of the parameters' size, the library's own also beside a caller-supplied arena
 *                                      (ctx_arena_bytes is unchanged) -- and sets it to the parameters; a later call changes only
 *                                      decay and warmup.
 *   ctx_ema_disable(h)                 frees the shadow; the handle then behaves as if it had never been enabled.
 *   ctx_ema_reset(h)                   shadow = parameters, update count = 0.
 *   ctx_ema_update(h)                  one update from the parameters as they are now, for callers whose optimiser lives outside the
 *                                      library (they write through ctx_dev_params and call ctx_params_written): honours the mask,
 *                                      ignores the guard.  Asynchronous.
 *   ctx_ema_swap(h)                    exchanges parameters and shadow on the device (two swaps restore every bit), so that every
 *                                      inference entry runs on the averaged weights; packed filters and captured graphs follow as
 *                                      after any parameter change.  CTX_E_STATE while an accumulation is open.  Asynchronous.
 *   ctx_ema_state(h, &enabled, &swapped, &decay, &updates)   every out-pointer nullable; works on a handle without a shadow.
 *   ctx_get_ema(h, out, n, &updates) / ctx_set_ema(h, in, n, updates)   the shadow in the flat order and length of ctx_get_params /
 *                                      ctx_set_params, and the update count (nullable on get; < 0 on set: CTX_E_INVALID).
 * The update: e = fmaf(c, p - e, e) per element with c = (float)(1 - d_t), d_t formed in double: update number t, counted from 0,
 * runs at d_t = decay, or with warmup != 0 at min(decay, (1 + t) / (10 + t)).  e == p stays e exactly and decay = 1 leaves e exactly.
 * The count moves on the host with every update ISSUED -- also for a step the guard then skips on the device, as the Adam step
 * count does.
 *   - guard (ctx_set_grad_guard): a step skipped for a non-finite gradient leaves the shadow untouched as well (the count moves).
 *   - mask (ctx_set_param_lr_scale): the update runs over the trainable tensors only; a frozen tensor's shadow keeps every bit.
 *   - reset rule: the shadow is set to the new parameters and the count to 0 when ALL parameters are replaced from outside a step:
 *     ctx_set_params, ctx_init_params and the broadcast of ctx_dp_init.  ctx_params_written does NOT reset.
 *   - while swapped, every entry that writes parameters or shadow returns CTX_E_STATE: the training steps, ctx_dev_adam, ctx_accum_begin
 *     and with it every accumulation entry, ctx_profile_step, ctx_set_params, ctx_init_params, ctx_dp_init and the entries of this
 *     section other than ctx_ema_swap and ctx_ema_state.  Inference, ctx_eval*, ctx_get_params (which then returns the averaged
 *     weights) and the VJP calls stay allowed.
 * Every entry but ctx_ema_enable and ctx_ema_state returns CTX_E_STATE on a handle without a shadow; a NULL handle is CTX_E_INVALID
 * and nothing is written through the out-pointers. */
int ctx_ema_enable(ctx_handle* h, float decay, int warmup);
int ctx_ema_disable(ctx_handle* h);
int ctx_ema_reset(ctx_handle* h);
int ctx_ema_update(ctx_handle* h);
int ctx_ema_swap(ctx_handle* h);
int ctx_ema_state(ctx_handle* h, int* enabled, int* swapped, float* decay, int64_t* updates);
int ctx_get_ema(ctx_handle* h, float* out, int64_t n, int64_t* updates);
int ctx_set_ema(ctx_handle* h, const float* in, int64_t n, int64_t updates);

/* ---- per-tensor gradient, parameter and update statistics, taken on the device (new here) --------------------------------------------
 * One row per tensor of ctx_param_info, in its order, from a deterministic two-stage f64 reduction over the arena:
 * the sums of squares of gradient g, parameter p and Adam update u = lr_t m / (sqrtf(v) + eps) in f64, their largest magnitudes in
 * f32 -- all over the FINITE elements only -- and the counts of non-finite elements of g and of p.  The bits of a row depend neither
 * on the device nor on which other tensors are frozen.  Off by default: a handle that never enables it runs exactly the launches of
 * one that has never heard of it.
 *   ctx_tensor_stats_enable(h, every)   every >= 1, else CTX_E_INVALID.  From here on every `every`-th Adam update of the handle (the
 *                                       updates listed for ctx_ema_* above; counted by the Adam step count) is followed by one
 *                                       table: two launches behind the update and behind the average's, nothing synchronised.  g is
 *                                       the gradient that update consumed (reduced on a ctx_dp_* step, the folded sum under an
 *                                       accumulation), p the parameters and u the update as the step left them.  A step the guard
 *                                       skipped has u exactly 0 and reports applied = 0.  Allocates the library's own buffers
 *                                       (ctx_arena_bytes is unchanged); a later call changes only the period.
 *   ctx_tensor_stats_disable(h)         stops the automatic form and frees the buffers and the table taken; a handle without them
 *                                       is left as it is (CTX_OK).
 *   ctx_tensor_stats_compute(h, what)   a table of the arena as it stands, what = CTX_TSTAT_PARAMS | CTX_TSTAT_GRADS (anything else,
 *                                       or 0: CTX_E_INVALID): fields not asked for are zero, so are the u fields, has_update is 0 and
 *                                       applied 1.  CTX_TSTAT_GRADS before any backward: CTX_E_STATE.  Reads only, so it is allowed
 *                                       while the averaged weights are swapped in -- p is then the AVERAGE (the arena holds it) --
 *                                       and while an accumulation is open -- g is then the LAST micro-batch's gradient alone, the
 *                                       sum of the earlier ones lies beside the arena.  Works without ctx_tensor_stats_enable.
 *                                       Asynchronous.
 *   ctx_tensor_stats_get(h, rows, cap, &n, &adam_step, &applied, &has_update)   synchronises and copies the last table taken: n =
 *                                       ctx_param_count rows (cap < n: CTX_E_INVALID), the Adam step count it was taken at, whether
 *                                       that step was applied (0: the guard skipped it) and whether the u fields were computed.
 *                                       Every out-pointer but rows is nullable.  CTX_E_STATE when no table has been taken yet.
 *   - mask (ctx_set_param_lr_scale): a frozen tensor's gradient and moments are NOT read (a pruned backward never wrote that
 *     gradient): its g and u fields are zero and flag bit 0 is clear; its p fields are filled.  u uses the tensor's own lr_t.
 *   - floats between two tensors and past the end of the last one are never read.
 * A NULL handle is CTX_E_INVALID and nothing is written through the out-pointers. */
typedef struct ctx_tensor_stat {
    double g_sumsq, p_sumsq, u_sumsq;
    float g_absmax, p_absmax, u_absmax;
    uint32_t g_nonfinite, p_nonfinite;
    uint32_t flags;       /* CTX_TSTAT_F_* */
} ctx_tensor_stat;        /* 48 bytes */
enum { CTX_TSTAT_PARAMS = 1, CTX_TSTAT_GRADS = 2 };
enum {
    CTX_TSTAT_F_TRAINABLE = 1,   /* bit 0: the tensor is trainable -- its g and u fields are valid (where the table took them) */
    CTX_TSTAT_F_GRADS = 2,       /* the table took gradients and this tensor's were read */
    CTX_TSTAT_F_UPDATE = 4,      /* ... the update, from this tensor's moments */
    CTX_TSTAT_F_PARAMS = 8       /* the table took parameters */
};
int ctx_tensor_stats_enable(ctx_handle* h, int every);
int ctx_tensor_stats_disable(ctx_handle* h);
int ctx_tensor_stats_compute(ctx_handle* h, int what);
int ctx_tensor_stats_get(ctx_handle* h, ctx_tensor_stat* rows, int cap, int* n, int64_t* adam_step, int* applied, int* has_update);

/* ---- measurement ------------------------------------------------------------------------------ */
/* One entry per launch group of a train step (a layer's forward, input gradient, filter gradient,
 * bias gradient, the losses, Adam): HIP-event time on the handle's stream, averaged over `iters`
 * full steps, plus the group's algorithmic FLOPs (2 per multiply-add, all 25 taps), the share of them that
 * is not a product with SAME padding (useful_frac) and the kernel that executes it.  bench.py derives its
 * `roofline` block from this. */
typedef struct ctx_prof_entry {
    char name[56];
    char kernel[40];
    double flops;       /* 2 per multiply-add, every tap of a SAME-padded layer counted (SURVEY.md 8d's convention) */
    float ms;
    float useful_frac;  /* share of `flops` whose product meets data on both sides: (valid (position, tap) pairs) / (all) of the
                           layer -- (5n-3)^2 / (5n)^2 for a 5x5 stride-2 layer with an n x n small grid; 1 for linear layers.
                           flops * useful_frac is what a kernel that never multiplies padding zeros has to do. */
} ctx_prof_entry;
int ctx_profile_step(ctx_handle* h, const float* d_src, const float* d_ctx, const float* d_tgt, int B,
                     float lr, int iters, ctx_prof_entry* entries, int max_entries, int* n_entries);

/* ---- test hook ------------------------------------------------------------------------------- */
/* Copies n floats of a named internal activation / gradient buffer to the host (bring-up and
 * parity tests only; names are listed in csrc/ctx_abi.cpp: ctx_debug_read). */
int ctx_debug_read(ctx_handle* h, const char* name, float* host, size_t n);

/* ---- frozen conv-net front end (mode 'oursinception') --------------------------------------------
 * Replaces the reference's  inception_v3.inception_v3(images, is_training=False)[1]['Mixed_7c']
 * (rllab/sampler/base.py:122-127, scripts/train_script.py:104-111; nets/inception_v3.py:93-416).  The graph is
 * handed over as an op list by the host (imitation_from_observation_amd/inception_frontend.py builds it from the
 * reference's layer table); this library executes it.  Activations are NHWC, channel counts rounded up to 32.
 *   CONV     slim.conv2d: kh x kw (kh*kw <= 25) conv, stride 1|2, TF 'SAME' or 'VALID', with the batch norm folded by the
 *            host into the filter  w' = w / sqrt(var + 0.001)  and a bias  b' = beta - mean / sqrt(var + 0.001),  then ReLU;
 *            filter [kh][kw][src channels (padded)][cout] at w_off, bias [cout] at b_off (floats into the blob);
 *            output written to channels [dst_ch0, dst_ch0 + cout) of buffer dst (tf.concat = adjacent slices).
 *   MAXPOOL  3x3 stride 2 VALID.     AVGPOOL  3x3 stride 1 SAME, mean over the taps inside the image.
 *   AVGPOOL_VALID  kh x kw stride `stride` VALID, mean over the kh*kw taps: the classifier head's
 *            slim.avg_pool2d(Mixed_7c, [min(h,8), min(w,8)], padding='VALID') = PreLogits (nets/inception_v3.py:510-515).
 *   CONV_LINEAR    a CONV with bias and NO ReLU (slim.conv2d(..., activation_fn=None, normalizer_fn=None)): Logits = the 1x1
 *            Conv2d_1c_1x1 on PreLogits (:518-519), 1001 classes padded to cout 1024 with zero filter columns and bias.
 *            (ABI 4, additions only: kinds 3 and 4.)
 * Buffer 0 is the frame buffer (h, w, 32: channels 0..2 hold the frame); the LAST buffer is the output.
 * Every buffer is written once per pass (by one op, or by several ops into disjoint channel slices). */
enum { CTX_CNN_CONV = 0, CTX_CNN_MAXPOOL = 1, CTX_CNN_AVGPOOL = 2, CTX_CNN_AVGPOOL_VALID = 3, CTX_CNN_CONV_LINEAR = 4 };
typedef struct ctx_cnn_buf { int32_t h, w, c; } ctx_cnn_buf;
typedef struct ctx_cnn_op {
    int32_t kind, src, dst, dst_ch0;
    int32_t kh, kw, stride, same;     /* CONV / CONV_LINEAR (same: 1 = 'SAME', 0 = 'VALID') and AVGPOOL_VALID (kh, kw, stride) */
    int32_t cout;
    int32_t lane;                     /* 0..3: ops of different lanes may run concurrently (the branches of an Inception block);
                                         the library orders every op after the writers of its src buffer */
    int64_t w_off, b_off;
    /* ---- ABI 2 (zero-initialise for the plain forms) ----
     * src_c != 0: the conv reads channels [src_ch0, src_ch0 + src_c) of buffer src (multiples of 32) instead of all of them: the
     *   filter is then [kh][kw][src_c][cout].
     * nsplit != 0 (CONV): a MERGED conv of sibling branches that read the same tensor (the 1x1 heads of an Inception block,
     *   nets/inception_v3.py:140-213, 236-364, 389-416) -- one GEMM with the filters side by side along cout: output columns
     *   [0, nsplit) go to (dst, dst_ch0), columns [nsplit, cout) to (dst2, dst2_ch0). */
    int32_t src_ch0, src_c;
    int32_t nsplit, dst2, dst2_ch0, reserved;
} ctx_cnn_op;
typedef struct ctx_cnn ctx_cnn;
int ctx_cnn_create(const ctx_cnn_buf* bufs, int nbufs, const ctx_cnn_op* ops, int nops, int64_t weight_floats,
                   int max_images, int precision, int device, void* stream, ctx_cnn** out);
void ctx_cnn_destroy(ctx_cnn* h);
const char* ctx_cnn_last_error(const ctx_cnn* h);          /* h == NULL: last creation error of this thread */
int ctx_cnn_set_weights(ctx_cnn* h, const float* blob, size_t n);
/* frames: host uint8 [n,H,W,3], preprocessed like base.py:116-119; out: host f32 [n,h,w,c] of the last buffer.
 * n may exceed max_images (processed in chunks). */
int ctx_cnn_forward_u8(ctx_cnn* h, const uint8_t* frames, int n, float* out);
/* frames: host uint8 [n,H,W,3], n <= max_images; *d_out: DEVICE pointer of the last buffer [n,h,w,c] (valid until the next
 * forward).  Asynchronous on the handle's stream: `frames` must stay untouched until the stream has passed the upload. */
int ctx_cnn_forward_u8_dev(ctx_cnn* h, const uint8_t* frames, int n, const float** d_out);
/* d_frames: DEVICE f32 [n,H,W,3] in [-1,1], n <= max_images; *d_out: device pointer of the last buffer.
 * Asynchronous on the handle's stream (ctx_cnn_stream / ctx_cnn_sync). */
int ctx_cnn_forward_dev(ctx_cnn* h, const float* d_frames, int n, const float** d_out);
/* d_frames: DEVICE uint8 [n,H,W,3] at the front end's size (e.g. what ctx_resize_u8_dev left on ctx_cnn_stream(h)), n <= max_images:
 * ctx_cnn_forward_u8_dev without the upload -- the frames go straight into the conversion kernel in place of the handle's staging
 * buffer, so the result equals ctx_cnn_forward_u8_dev on the same bytes bit for bit.  Any byte address (the kernel loads bytes);
 * d_frames must have been written on ctx_cnn_stream(h) or before a synchronisation.  Asynchronous on the handle's stream. */
int ctx_cnn_forward_dev_u8(ctx_cnn* h, const uint8_t* d_frames, int n, const float** d_out);
/* The trainer's input pipeline in front of the front end (mode 'oursinception', scripts/train_script.py:144-163; data parallel as
 * ctx_dp_train_step_sampled).  ctx_cnn_demos_upload keeps vdata[T][N][H][W][3] (uint8 frames at the front end's input size) in HBM on
 * the handle's device, replacing an earlier upload (CTX_E_NOMEM when it does not fit: 33 GB at 299x299, T = 25, N = 5000).
 * ctx_cnn_forward_sampled_dev: every rank passes the SAME global index arrays choicesrc / choicetgt [B_global]
 * (np.random.choice(ntrain, batch_size) twice, :154-155); rank r takes the global rows b in [r B/world, (r+1) B/world) and builds
 * 3 B_local images [src | ctx | tgt]:  src[b] = vdata[b % T][choicesrc[b]],  ctx[b] = vdata[0][choicetgt[b]],
 * tgt[b] = vdata[b % T][choicetgt[b]]  -- gathered, preprocessed and channel-padded into buffer 0 by one kernel, bit-identical to
 * ctx_cnn_forward_u8_dev on the same frames gathered on the host -- then runs the pass; *d_out as ctx_cnn_forward_u8_dev.  Every index
 * of the WHOLE arrays is checked before anything is launched (every rank refuses the same bad call); B_global % world != 0 and
 * 3 B_local > max_images are refused too (CTX_E_INVALID).  Asynchronous on the handle's stream. */
int ctx_cnn_demos_upload(ctx_cnn* h, const uint8_t* vdata, int T, int N);
int ctx_cnn_forward_sampled_dev(ctx_cnn* h, const int32_t* choicesrc, const int32_t* choicetgt, int B_global, int rank, int world,
                                const float** d_out);
int ctx_cnn_read_buffer(ctx_cnn* h, int index, int n, float* out);   /* end-point tests */
/* Per-op HIP-event times (ms, averaged over `iters` passes over the n images currently in buffer 0); measurement only. */
int ctx_cnn_profile(ctx_cnn* h, int n, int iters, float* ms, int max_ops);
void* ctx_cnn_stream(ctx_cnn* h);
int ctx_cnn_sync(ctx_cnn* h);

/* ---- Inception-feature baseline reward (modes 'inception' / 'inceptionsame', rllab/sampler/base.py:69-111, 178-189) ----
 * Per-timestep demo statistics, accumulated on the device from the activation buffers in place (their padded channel stride):
 *   ctx_cnn_stats_reset   slots = the buffers (index as in ctx_cnn_create; not buffer 0) with their REAL channel counts
 *                         channels[i] (> buffer width - 32) to accumulate, over videos of nframes frames (1 <= nframes <= max_images).
 *                         Every slot's statistics are [nframes, h, w, channels[i]].  Clears the accumulators.
 *   ctx_cnn_stats_add_u8  frames: host uint8 [nvideos * nframes, H, W, 3]; runs the forward (whole videos per pass, max_images /
 *                         nframes of them) and adds  x  (pass 0) or  (x - mean)^2  (pass 1) per element, videos in order.
 *   ctx_cnn_stats_finish  pass 0: mean = sum / count; pass 1: std = sqrt(sum / count).  Pass 1 must see as many videos as pass 0.
 *   ctx_cnn_stats_read    slot's means (after finish(0)) and stds (after finish(1); nullable) into host [nframes, h, w, c]; *count
 *                         (nullable) = videos of pass 0.
 * Every sum is a sequential f32 loop in video order without contraction, division and sqrt correctly rounded: the results equal
 * numpy's float32  np.mean(v, 0) / np.std(v, 0)  over the videos' features bit for bit.  Calls out of order: CTX_E_STATE.
 *
 * The per-path cost on the LAST buffer (the front end's `final` end point):
 *   ctx_cnn_reward_set_stats  means / stds: host f32 [nframes, h, w, channels] (channels = the last buffer's real count).
 *   ctx_cnn_reward_costs      frames: host uint8 [npaths * nframes, H, W, 3] -> costs [npaths * nframes]:
 *                             costs[f] = mean over (h, w, c) of d^2 / (std + 1e-5),  d = means[f % nframes] - x[f], d = 0 where std == 0
 *                             (terms in f32, summed in f64 in a fixed order).  Whole paths per forward; only the costs cross PCIe.
 *                             CTX_E_STATE before ctx_cnn_reward_set_stats.
 * Device-frame forms (frames that ctx_resize_u8_dev left on the device; no new arithmetic -- the same launches read the caller's
 * pointer in place of the staging buffer, results bit-identical to the host forms on the same bytes).  d_frames: DEVICE uint8 at any
 * byte address, written on ctx_cnn_stream(h) or before a synchronisation; arguments are checked as in the host forms:
 *   ctx_cnn_stats_add_dev_u8     d_frames [nvideos * nframes, H, W, 3]; whole videos per forward, chunked and ordered exactly as
 *                                ctx_cnn_stats_add_u8.  Synchronous (returns after the last chunk's accumulation).
 *   ctx_cnn_reward_costs_dev_u8  d_frames [npaths * nframes, H, W, 3] -> host costs, as ctx_cnn_reward_costs.  Synchronous. */
int ctx_cnn_stats_reset(ctx_cnn* h, const int32_t* buffers, const int32_t* channels, int nslots, int nframes);
int ctx_cnn_stats_add_u8(ctx_cnn* h, const uint8_t* frames, int nvideos, int pass);
int ctx_cnn_stats_finish(ctx_cnn* h, int pass);
int ctx_cnn_stats_read(ctx_cnn* h, int slot, float* means, float* stds, int* count);
int ctx_cnn_reward_set_stats(ctx_cnn* h, int channels, const float* means, const float* stds, int nframes);
int ctx_cnn_reward_costs(ctx_cnn* h, const uint8_t* frames, int npaths, float* costs);
int ctx_cnn_stats_add_dev_u8(ctx_cnn* h, const uint8_t* d_frames, int nvideos, int pass);
int ctx_cnn_reward_costs_dev_u8(ctx_cnn* h, const uint8_t* d_frames, int npaths, float* costs);

/* ---- third-person-imitation and GAIL baseline discriminators (modes 'tpil' / 'gail') ---------------------------
 * The two learned image rewards the reference compares against, both retrained inside the RL loop
 * (sandbox/bradly/third_person: discriminators/discriminator.py, algos/cyberpunk_trainer.py, algos/cyberpunk_trainer_gail.py).
 * ABI 4, additions only.  Frames are RAW pixel values 0..255 (float32 or uint8; no scaling anywhere), NHWC.
 *   TPIL  DomainConfusionVelocityDiscriminator (:357-548): a row is two frames (t and min(t + 3, T - 1)); both through
 *         conv3x3+ReLU, 2x2 SAME max pool, conv3x3+ReLU, pool, flatten, FC 128 + ReLU; class MLP 256-128-128-2 on [f1 | f2],
 *         domain MLP 128-128-128-2 behind flip_gradient(f1, 0.2); loss = CE_class + 0.2 CE_dom.
 *   GAIL  ConvDiscriminator (:122-207): a row is one frame and its time step; conv, pool, [flatten | time] -> 128 (ReLU) -> 2.
 *         wc2 / bc2 exist as in the reference (its second conv is commented out), receive no gradient and never move.
 *         H and W must be even (the reference's conv_out_size).
 * Parameters by name in the reference's creation order: wc1 wc2 bc1 bc2, then TPIL: w_feats_one b_feats_one w_targets0 b_targets0 ..
 * w_targets2 b_targets2 w_dom0 b_dom0 .. w_dom2 b_dom2; GAIL: w_0 b_0 w_1 b_1.  Filters HWIO, FC weights [in][out].
 * Arithmetic: f32, every sum in a fixed order (bit-identical from run to run); the max pool's gradient goes to the first maximum
 * of a window in row-major order, ReLU'(0) = 0; cross-entropy in log-sum-exp form, its gradient softmax - labels; argmax ties -> 0;
 * TF Adam (beta 0.9 / 0.999, eps 1e-8 outside the bias correction).  No CPU path: ctx_disc_create without a device is CTX_E_DEVICE.
 *
 * Host-array forms, one per reference call site (x1 [B,H,W,3]; x2_or_time: TPIL the second frames [B,H,W,3] in x1's type, GAIL the
 * time column float [B]; cls / dom one-hot float [B,2]; 1 <= B <= max_batch):
 *   ctx_disc_train     one Adam step; *loss = the loss before the update (sess.run([optimizer, loss])).
 *   ctx_disc_logits    class logits, or their softmax, [B,2].       ctx_disc_accuracy  mean(argmax cls == argmax logits).
 * Resident forms:
 *   ctx_disc_data_upload  frames uint8 [N,T,H,W,3] and per-trajectory one-hot cls / dom [N,2] (dom nullable) into device memory.
 *   ctx_disc_train_epoch  order[n]: flat row indices (trajectory * T + t) into that tensor.  Batch k = rows order[k batch ..): first
 *                         frame t, second frame min(t + shift, T - 1) (GAIL: time = t), the trajectory's targets; one step per batch,
 *                         then (with_accuracy) the accuracy of batch k on the UPDATED parameters -- all batches enqueued without a
 *                         host synchronisation; losses / accs [ceil(n / batch)] come back once.  Bit-identical to the same rows
 *                         through ctx_disc_train_u8 / ctx_disc_accuracy_u8 one batch at a time.
 *   ctx_disc_reward_paths frames uint8 [P,T,H,W,3] -> probs[P T] = softmax(class logits)[:, 0] of the pairs (t, min(t + shift, T - 1))
 *                         (GAIL: of (frame t, time t)).  Whole paths per pass, each frame through the conv stack ONCE; equal bit for
 *                         bit to ctx_disc_logits_u8 on the materialised pairs (a row's sums do not depend on its neighbours).
 * Device-frame forms (frames resized on the device by a ctx_resize plan that shares ctx_disc_stream(h)):
 *   ctx_disc_stream           the handle's hipStream_t, for ctx_resize_create.
 *   ctx_disc_reward_paths_dev d_frames: DEVICE uint8 [P,T,H,W,3] at any byte address (the conv kernel loads bytes), written on
 *                             ctx_disc_stream(h) or before a synchronisation; otherwise ctx_disc_reward_paths, bit for bit: the first
 *                             conv reads the caller's memory in place of the handle's input buffer.  Synchronous.
 *   ctx_disc_data_begin       sizes the resident data set for [N,T,H,W,3] and uploads the per-trajectory targets as
 *                             ctx_disc_data_upload does; *d_frames = the device address of the resident uint8 tensor, which the
 *                             caller fills on ctx_disc_stream(h) (ctx_resize_u8_dev with a destination inside it) before the next
 *                             ctx_disc_train_epoch.  Valid until the next ctx_disc_data_begin / _upload / _destroy.
 *                             ctx_disc_data_upload == ctx_disc_data_begin followed by a copy of the same bytes.
 * ctx_disc_debug_read (tests): pool1 sel1 pool2 sel2 f hc1 hc2 hd1 hd2 logits probs of the last forward; sel = the pool windows'
 * winner (0..3, row-major) + 4 * (maximum > 0), as floats. */
enum { CTX_DISC_TPIL = 0, CTX_DISC_GAIL = 1 };
typedef struct ctx_disc_config { int32_t variant, H, W, C, max_batch; } ctx_disc_config;
typedef struct ctx_disc ctx_disc;
int64_t ctx_disc_param_total_for(const ctx_disc_config* cfg);      /* works without a device; CTX_E_INVALID for a bad config */
int ctx_disc_create(const ctx_disc_config* cfg, int device, ctx_disc** out);
void ctx_disc_destroy(ctx_disc* h);
const char* ctx_disc_last_error(const ctx_disc* h);                /* h == NULL: last creation error of this thread */
int ctx_disc_param_count(const ctx_disc* h);
int ctx_disc_param_info(const ctx_disc* h, int index, const char** name, int* ndim, int64_t* shape4, int64_t* offset);
int ctx_disc_set_params(ctx_disc* h, const float* flat, size_t n);
int ctx_disc_get_params(ctx_disc* h, float* flat, size_t n);
int ctx_disc_get_grads(ctx_disc* h, float* flat, size_t n);        /* of the last training step, taken at its pre-update parameters */
int ctx_disc_set_adam_state(ctx_disc* h, const float* m, const float* v, size_t n, int64_t step);
int ctx_disc_get_adam_state(ctx_disc* h, float* m, float* v, size_t n, int64_t* step);
int ctx_disc_init_params(ctx_disc* h, uint64_t seed);              /* the reference's initialisers; fresh Adam slots */
int ctx_disc_sync(ctx_disc* h);
void* ctx_disc_stream(ctx_disc* h);
int ctx_disc_train(ctx_disc* h, const float* x1, const float* x2_or_time, const float* cls, const float* dom, int B, float lr, float* loss);
int ctx_disc_train_u8(ctx_disc* h, const uint8_t* x1, const void* x2_or_time, const float* cls, const float* dom, int B, float lr,
                      float* loss);
int ctx_disc_logits(ctx_disc* h, const float* x1, const float* x2_or_time, int B, int softmax, float* out);
int ctx_disc_logits_u8(ctx_disc* h, const uint8_t* x1, const void* x2_or_time, int B, int softmax, float* out);
int ctx_disc_accuracy(ctx_disc* h, const float* x1, const float* x2_or_time, const float* cls, int B, float* acc);
int ctx_disc_accuracy_u8(ctx_disc* h, const uint8_t* x1, const void* x2_or_time, const float* cls, int B, float* acc);
int ctx_disc_data_upload(ctx_disc* h, const uint8_t* frames, int N, int T, const float* cls, const float* dom);
int ctx_disc_train_epoch(ctx_disc* h, const int32_t* order, int64_t n, int batch, int shift, float lr, int with_accuracy, float* losses,
                         float* accs);
int ctx_disc_reward_paths(ctx_disc* h, const uint8_t* frames, int P, int T, int shift, float* probs);
int ctx_disc_data_begin(ctx_disc* h, int N, int T, const float* cls, const float* dom, uint8_t** d_frames);
int ctx_disc_reward_paths_dev(ctx_disc* h, const uint8_t* d_frames, int P, int T, int shift, float* probs);
int ctx_disc_debug_read(ctx_disc* h, const char* name, float* host, size_t n);

/* ---- device-side frame resize: scipy.misc.imresize(img, idims) for uint8 RGB frames ------------------------------
 * Every frame the reference uses goes through it first (the environments of gym/envs/mujoco on every rendered frame, scripts/train_script.py:16-19
 * on every demo frame).  For uint8 RGB input it is Pillow's Image.resize(..., BILINEAR): a separable antialiased triangle filter,
 * horizontal pass then vertical pass, each in 22-bit fixed point, rounded half-up and clipped to uint8 BETWEEN the passes
 * (libImaging/Resample.c); a pass whose input and output extents are equal is skipped.  Integer arithmetic, so the device result
 * equals Pillow's bit for bit.  ABI 4, additions only.  A plan is one geometry: 1 <= Hin, Win <= 4096, 1 <= Hout, Wout <= 1024,
 * C == 3, 1 <= max_frames <= 65535, up- or downscaling on each axis independently; anything else is CTX_E_INVALID.
 *   ctx_resize_coeffs    works without a device: the tables of one axis as Resample.c's precompute_coeffs / normalize_coeffs_8bpc
 *                        make them (double, weights summed in order, divided, (int)(+-0.5 + w 2^22)).  xmin / count [out_size],
 *                        kk [out_size][*ksize] row-major, zero beyond count[xx]; *ksize = 2 ceil(max(in/out, 1)) + 1; kk may be NULL
 *                        to query *ksize.  CTX_E_INVALID for sizes < 1.
 *   ctx_resize_create    arguments are validated BEFORE the device is touched (CTX_E_INVALID); no usable device: CTX_E_DEVICE,
 *                        *out = NULL.  stream: a hipStream_t (ctx_stream / ctx_cnn_stream of the consumer) or NULL = private stream.
 *                        A borrowed stream is never destroyed or, in ctx_resize_destroy, waited on: the plan may outlive its owner,
 *                        but must not be CALLED after the owner is gone.
 *   ctx_resize_u8        host uint8 [n,Hin,Win,C] -> host uint8 [n,Hout,Wout,C]; any n >= 1 (chunks of max_frames); synchronous.
 *   ctx_resize_f32_dev   host uint8 in, DEVICE f32 out in the sampler's (x/255 - 0.5)*2 form (the three separately rounded f32
 *                        operations of ctx_encode's image_trans, bit for bit), n <= max_frames.  d_dst NULL: the plan's own buffer
 *                        (valid until the next call); else a device buffer of n*Hout*Wout*C floats, e.g. a slot of ctx_dev_frames.
 *                        *d_out = where it was written -- what ctx_reward_costs_dev, ctx_reward_cache_add_dev, ctx_encode_dev,
 *                        ctx_translate_dev and ctx_cnn_forward_dev take.  Asynchronous on the plan's stream: `frames` must stay
 *                        untouched until the stream has passed the upload.
 *   ctx_resize_u8_dev    host uint8 in, DEVICE uint8 [n,Hout,Wout,C] out, written by the same launches as ctx_resize_u8 (same bits),
 *                        n <= max_frames.  d_dst NULL: the plan's own uint8 buffer, valid until the plan's next call; else ANY byte
 *                        address in device memory with n*Hout*Wout*C bytes behind it (the kernels store bytes), e.g. an offset into
 *                        the tensor of ctx_disc_data_begin.  *d_out = where the result is -- what ctx_cnn_forward_dev_u8,
 *                        ctx_cnn_stats_add_dev_u8, ctx_cnn_reward_costs_dev_u8 and ctx_disc_reward_paths_dev take.  Both passes
 *                        skipped (equal sizes): the result is the uploaded bytes; without a destination *d_out points at the plan's
 *                        input buffer, with one they are copied device-to-device on the stream.  Asynchronous like ctx_resize_f32_dev.
 *   ctx_resize_u8_dev_v / ctx_resize_f32_dev_v   the same with `frames` an array of n pointers, one contiguous [Hin,Win,C] frame each
 *                        (frames where the environment left them: no gather on the host): one hipMemcpyAsync per frame into
 *                        consecutive slots of the plan's input buffer, then the same launches.  A NULL entry is CTX_E_INVALID before
 *                        anything is enqueued.  Every frame must stay untouched until the stream has passed its upload.
 *   ctx_resize_profile   measurement only: one upload of n frames (pinned != 0: from a page-locked copy of them) and one run of the
 *                        kernels into the plan's f32 buffer, each between HIP events on the plan's stream (ms). */
typedef struct ctx_resize ctx_resize;
int ctx_resize_coeffs(int in_size, int out_size, int32_t* xmin, int32_t* count, int32_t* kk, int* ksize);
int ctx_resize_create(int Hin, int Win, int C, int Hout, int Wout, int max_frames, int device, void* stream, ctx_resize** out);
void ctx_resize_destroy(ctx_resize* r);
const char* ctx_resize_last_error(const ctx_resize* r);       /* r == NULL: last creation error of this thread */
int ctx_resize_u8(ctx_resize* r, const uint8_t* frames, int n, uint8_t* out);
int ctx_resize_f32_dev(ctx_resize* r, const uint8_t* frames, int n, float* d_dst, const float** d_out);
int ctx_resize_u8_dev(ctx_resize* r, const uint8_t* frames, int n, uint8_t* d_dst, const uint8_t** d_out);
int ctx_resize_u8_dev_v(ctx_resize* r, const uint8_t* const* frames, int n, uint8_t* d_dst, const uint8_t** d_out);
int ctx_resize_f32_dev_v(ctx_resize* r, const uint8_t* const* frames, int n, float* d_dst, const float** d_out);
int ctx_resize_sync(ctx_resize* r);
int ctx_resize_profile(ctx_resize* r, const uint8_t* frames, int n, int pinned, float* h2d_ms, float* kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* CTXTRANS_H */
