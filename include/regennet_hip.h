/*
 * regennet_hip.h — C-ABI of libregennet_hip.so: the MI355X (gfx950) implementation of ReGenNet's
 * diffusion-sampling hot path. Plain C types only; device memory is passed as raw
 * pointers (e.g. torch.Tensor.data_ptr()), streams as hipStream_t cast to void*.
 *
 * The reference has no FFI of its own (it is pure Python/PyTorch); every entry point below states
 * the reference interface (file:line under the upstream repo) whose arithmetic it replaces. The
 * reference-side binding a maintainer would add is shown in INTEGRATION.md; the in-tree binding is
 * regennet_amd/_lib.py (ctypes).
 *
 * Conventions
 *   - every function returns 0 on success or a negative rgn_status; rgn_last_error() gives text.
 *   - no exceptions cross the boundary (every entry point catches at the boundary: RGN_ERR_INTERNAL);
 *     a handle is NOT thread-safe (one handle per device/stream).
 *   - "x" tensors are fp32 [B, njoints, nfeats, T] contiguous — the reference's boundary layout
 *     (model/cmdm.py:173-177); timesteps are int64 like the reference's `t` tensors.
 */
#ifndef REGENNET_HIP_H
#define REGENNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the entry points below are its ONLY dynamic symbols. */
#if defined(__GNUC__) || defined(__clang__)
#define RGN_API __attribute__((visibility("default")))
#else
#define RGN_API
#endif

typedef struct rgn_ctx* rgn_handle;

typedef enum {
    RGN_OK = 0,
    RGN_ERR_INVALID_ARG = -1,    /* bad pointer / size / enum                                   */
    RGN_ERR_BAD_KEY = -2,        /* unexpected state_dict key (utils/model_util.py:7)           */
    RGN_ERR_BAD_SHAPE = -3,      /* tensor shape does not match the configuration               */
    RGN_ERR_MISSING_KEY = -4,    /* finalize: a required key was never loaded (model_util.py:8) */
    RGN_ERR_STATE = -5,          /* call order violated (e.g. sample before set_schedule)       */
    RGN_ERR_HIP = -6,            /* HIP runtime error (text in rgn_last_error)                  */
    RGN_ERR_UNSUPPORTED = -7,    /* configuration outside the hot path (e.g. latent_dim > 1024) */
    RGN_ERR_INTERNAL = -8        /* a host-side C++ exception (std::bad_alloc ...) caught at the boundary */
} rgn_status;

enum { RGN_CM_ADD = 0, RGN_CM_CONCAT = 1 };                 /* --cm_mode, model/cmdm.py:207-211  */
enum { RGN_COND_NONE = 0, RGN_COND_ACTION = 1, RGN_COND_TEXT = 2 }; /* cond_mode, model_util.py:25-30 */
enum { RGN_PREC_F32 = 0,      /* fp32-input MFMA (v_mfma_f32_32x32x2_f32): exact fp32 products     */
       RGN_PREC_BF16X3 = 1,   /* split-bf16: a*b ~ ah*bh + ah*bl + al*bh on bf16 MFMA, fp32 accum  */
       RGN_PREC_BF16 = 2,     /* plain bf16 MFMA inputs (fastest; outside the 1e-3 parity bound)   */
       RGN_PREC_BF16_X3TAIL = 3 }; /* precision schedule (default): plain-bf16 GEMM operands while the sampler
                                 still contracts errors (large t), split-bf16 for the last steps of a sampling
                                 loop (rgn_set_x3_tail) and for every rgn_denoise call; the residual stream and
                                 LayerNorm/softmax stay hi+lo / fp32 throughout. Inside the 1e-3 parity bound. */
enum { RGN_ARCH_ONLINE = 0,   /* causal nn.TransformerDecoder (model/cmdm.py:205-227)                 */
       RGN_ARCH_OFFLINE = 1,  /* non-causal nn.TransformerEncoder, embedding as token 0 (cmdm.py:228-238) */
       RGN_ARCH_MLP = 3,      /* (2 stays unassigned and refused) DiffMLP time / feature mixer (cmdm.py:239-242, model/mlp.py); num_heads, ff_size, emb_trans_dec and
                                 wo_pos_emb are not read; at most 160 frames; no k_layers, no fp16 sub-phase, no small-batch engine */
       RGN_ARCH_GRU = 4 };    /* nn.GRU(d, d, num_layers) over [pose ; emb] embeddings (cmdm.py:191-199, 243-249; rgn_gru_stack.hip); cm_mode add only; num_heads,
                                 ff_size, emb_trans_dec and wo_pos_emb are not read; no k_layers, no k_step, no fp16 sub-phase, no small-batch engine */
enum { RGN_GRU_SCAN_BATCH = 0,  /* the reference's own recurrence: nn.GRU(batch_first=True) on [T, B, d] scans the B samples of a call, frames are its batch */
       RGN_GRU_SCAN_FRAMES = 1 };/* a recurrence over the frames of every sample */
enum { RGN_SAMPLER_DDPM = 0,  /* GaussianDiffusion.p_sample   diffusion/gaussian_diffusion.py:508  */
       RGN_SAMPLER_DDIM = 1 };/* GaussianDiffusion.ddim_sample diffusion/gaussian_diffusion.py:744 */
enum { RGN_FLAG_UNCOND = 1,   /* y['uncond']=True  (model/cmdm.py:181, mask_cond :129-137)         */
       RGN_FLAG_GUIDED = 2 }; /* ClassifierFreeSampleModel.forward (model/cfg_sampler.py:24-31)    */

/* Mirrors the keyword arguments `CMDM(**get_model_args(args, data))` receives for arch='online' or 'offline'
 * (utils/model_util.py:20-72; model/cmdm.py:13-16). A zero-initialised tail means arch='online'. For arch='offline'
 * emb_trans_dec and wo_pos_emb are ignored: the reference always prepends the embedding token and always adds the
 * positional encoding (cmdm.py:228-238). */
typedef struct {
    int32_t njoints;        /* 56 for SMPL-X (model_util.py:45-46)                     */
    int32_t nfeats;         /* 6 for rot6d (model_util.py:47-48)                       */
    int32_t num_frames;     /* T: 60 ntu / 150 chi3d (model_util.py:61-64)             */
    int32_t latent_dim;     /* d, --latent_dim (parser_util.py:126)                    */
    int32_t ff_size;        /* 1024 (model_util.py:69)                                 */
    int32_t num_heads;      /* 4 (model_util.py:69)                                    */
    int32_t num_layers;     /* --layers                                                */
    int32_t cm_mode;        /* RGN_CM_*                                                */
    int32_t cond_mode;      /* RGN_COND_*                                              */
    int32_t num_actions;    /* rows of embed_action.action_embedding (cmdm.py:361)     */
    int32_t clip_dim;       /* 512 (cmdm.py:15)                                        */
    int32_t emb_trans_dec;  /* --emb_trans_dec (cmdm.py:212-215,224-225)               */
    int32_t wo_pos_emb;     /* --wo_pos_emb (cmdm.py:217)                              */
    int32_t max_batch;      /* largest B any later call will use                       */
    int32_t precision;      /* RGN_PREC_*                                              */
    int32_t device;         /* HIP device ordinal                                      */
    int32_t arch;           /* RGN_ARCH_* (--arch, parser_util.py:32)                  */
} rgn_config;

/* Per-timestep fp64 tables of the (re-spaced) diffusion, each of length S, exactly the attributes
 * GaussianDiffusion.__init__ builds (diffusion/gaussian_diffusion.py:172-209) after
 * SpacedDiffusion.__init__ re-derived the betas (diffusion/respace.py:73-87). */
typedef struct {
    int32_t S;                              /* num_timesteps after respacing                         */
    const int64_t* timestep_map;            /* respace.py:75,85 — ORIGINAL index of each kept step   */
    const double* posterior_mean_coef1;     /* gaussian_diffusion.py:199-201                          */
    const double* posterior_mean_coef2;     /* :202-206                                               */
    const double* model_log_variance;       /* FIXED_SMALL: posterior_log_variance_clipped (:360-363);
                                               FIXED_LARGE: log(append(post_var[1], betas[1:])) (:352-357) */
    const double* sqrt_recip_alphas_cumprod;    /* :184                                              */
    const double* sqrt_recipm1_alphas_cumprod;  /* :185                                              */
    const double* alphas_cumprod;               /* :174                                              */
    const double* alphas_cumprod_prev;          /* :175                                              */
} rgn_schedule;

/* Lifetime. Replaces: CMDM.__init__ (model/cmdm.py:13-111) + model.to(dev()) (sample/cgenerate.py:82). */
RGN_API int rgn_create(const rgn_config* cfg, rgn_handle* out);
RGN_API int rgn_destroy(rgn_handle h);
/* Text of the most recent error on `h` (or of the last failed rgn_create when h == NULL). */
RGN_API const char* rgn_last_error(rgn_handle h);

/* Checkpoint ingestion, keyed by the reference's state_dict names. Replaces
 * load_model_wo_clip / nn.Module.load_state_dict(strict=False) (utils/model_util.py:5-8):
 * an unexpected key -> RGN_ERR_BAD_KEY; keys starting with "clip_model." are accepted and ignored.
 * `host` is caller-owned fp32 host memory, copied during the call. */
RGN_API int rgn_load_weight(rgn_handle h, const char* ref_key, const float* host, const int64_t* shape, int32_t ndim);
/* Checks that no required key is missing (model_util.py:8), folds/packs weights for the kernels and
 * uploads them. Must be called once before any compute entry point. */
RGN_API int rgn_finalize_weights(rgn_handle h);
/* One flat device buffer holds every packed weight so multi-GPU start-up is ONE RCCL broadcast
 * (replaces utils/dist_util.py:54-83 sync_params / load_state_dict). */
RGN_API int rgn_weight_blob(rgn_handle h, void** dev_ptr, uint64_t* nbytes);

/* Replaces SpacedDiffusion.__init__ + _WrappedModel timestep mapping (diffusion/respace.py:64-129)
 * and the per-step _extract_into_tensor gathers (gaussian_diffusion.py:1604-1617). */
RGN_API int rgn_set_schedule(rgn_handle h, const rgn_schedule* s);

/* Binds model_kwargs['y'] for subsequent denoise/sample calls (data_loaders/tensors.py:57-94):
 * cmotion_dev fp32 [B,njoints,nfeats,T]; action_dev int64 [B] (y['action'][:,0]) or NULL;
 * text_feat_dev fp32 [B,clip_dim] = CLIP text features (encode_text output, cmdm.py:153-166) or NULL;
 * scale_dev fp32 [B] (y['scale'], cfg_sampler.py:31) or NULL. Hoists cmo_process(cmotion) and its
 * fuse_process half out of the step loop (model/cmdm.py:202,207-211). Inputs are read, never written. */
RGN_API int rgn_set_condition(rgn_handle h, int32_t B, const float* cmotion_dev, const int64_t* action_dev,
                      const float* text_feat_dev, const float* scale_dev, void* stream);

/* One denoiser evaluation: out = CMDM.forward(x, t, y) (model/cmdm.py:173-252), or with
 * RGN_FLAG_GUIDED the ClassifierFreeSampleModel combination (model/cfg_sampler.py:24-31).
 * t_dev: int64 [B] ORIGINAL timestep indices (what _WrappedModel passes on, respace.py:124-129). */
RGN_API int rgn_denoise(rgn_handle h, const float* x_dev, const int64_t* t_dev, int32_t flags, float* out_dev, void* stream);

/* Steps i = first_index, first_index-1, ..., first_index-count+1 of the sampling loop
 * (p_sample_loop_progressive gaussian_diffusion.py:711-742 / ddim :979-1005) applied in place to
 * x_dev [B,njoints,nfeats,T]:  x <- sampler(x, model(x, map[i]), noise_i).
 *   noise_dev : fp32 [count, B,njoints,nfeats,T], the per-step draws th.randn_like(x)
 *               (gaussian_diffusion.py:544,785) in loop order; NULL -> on-device Philox4x32-10
 *               keyed by (seed, global sample index = sample_offset + b, step i, element).
 *   x0_dev    : optional fp32 output, pred_xstart of the LAST executed step (NULL to skip).
 *   use_graph : replay captured hipGraphs (10 loop iterations each) instead of launching kernels one by one. Honoured by the
 *               throughput kernels; the small-batch engine (<= 640 token rows) launches eagerly either way, which is faster
 *               there (one chain of short kernels; REGENNET_SB_GRAPH=1 forces graphs).
 *   clip_denoised : clamp pred_xstart to [-1,1] (process_xstart, gaussian_diffusion.py:366-372). */
RGN_API int rgn_sample_range(rgn_handle h, int32_t sampler, int32_t guided, float eta, float* x_dev,
                     const float* noise_dev, uint64_t seed, uint64_t sample_offset,
                     int32_t first_index, int32_t count, float* x0_dev, int32_t use_graph,
                     int32_t clip_denoised, void* stream);

/* RGN_PREC_BF16_X3TAIL only: the last `tail_steps` loop indices (i < tail_steps) of every sampling loop run
 * split-bf16, all earlier ones plain bf16. -1 restores the default (max(5, ceil(S/200)) for models of >= 8 layers, max(8, ceil(S/100)) * 8/num_layers for shallower ones, at most S); 0 = plain bf16 throughout;
 * >= S = split-bf16 throughout. Why it is safe: p_sample scales the denoiser output by posterior_mean_coef1[t]
 * (gaussian_diffusion.py:265-276; 0.0016 at t=999, -> 1 at t=0), so early-step rounding is contracted away. */
RGN_API int rgn_set_x3_tail(rgn_handle h, int32_t tail_steps);

/* RGN_PREC_BF16_X3TAIL only, and only where the plain phase runs as the one-kernel decoder stack (k_layers<true>: <= 64 tokens, d = 512, >= 64
 * motions per call): the `steps` plain loop indices right in front of the split-bf16 tail (tail <= i < tail + steps) use IEEE fp16 MFMA operands
 * (11 mantissa bits) instead of bf16 (8) - weights, activation images, q / k / v / p; accumulation, LayerNorm, softmax and the sampler update stay
 * fp32. -1 restores the default (8, or REGENNET_F16_STEPS); 0 = no fp16 phase (then the default split-bf16 tail is the bf16 rule's again). With an
 * fp16 phase the default tail is 2 steps instead of 5 (3 for schedules of <= 10 steps): rgn_set_x3_tail overrides either. fp16 has a 5-bit exponent:
 * rgn_finalize_weights refuses (RGN_ERR_UNSUPPORTED, key named) a checkpoint with a weight of magnitude >= 6e4 unless the "BULK_F16" option is 0.
 * Reference: diffusion/gaussian_diffusion.py:508-560 (why only the last steps' arithmetic reaches the output), model/cmdm.py:227. */
RGN_API int rgn_set_f16_steps(rgn_handle h, int32_t steps);
/* The precision plan rgn_sample_range will follow for B motions on the bound schedule (rgn_set_schedule): loop indices i < *x3_tail run split-bf16,
 * x3_tail <= i < x3_tail + *f16_steps plain fp16 operands, the rest plain bf16 (RGN_PREC_BF16X3: x3_tail = S; other modes: 0 / 0). */
RGN_API int rgn_precision_plan(rgn_handle h, int32_t B, int32_t guided, int32_t* f16_steps, int32_t* x3_tail);

/* const_noise of p_sample (gaussian_diffusion.py:544-547): every motion of the batch receives the per-step draw of the
 * batch's motion 0 (tape entry [k, 0] / the Philox stream of sample_offset + 0); x_T is not affected (:706). Holds for the
 * following rgn_sample_range calls until cleared. */
RGN_API int rgn_set_const_noise(rgn_handle h, int32_t on);

/* Motion in-painting (gaussian_diffusion.py:319-323: y['inpainting_mask'] / y['inpainted_motion']) for the following
 * rgn_sample_range calls: pred = mask ? motion : model_output, before clip_denoised, after the guidance combination, so
 * x0_out, the sampler update and the next evaluation's input all see the blended prediction.
 * mask_dev: uint8 [B,njoints,nfeats,T] (0 / non-zero; the storage of a contiguous torch.bool tensor), motion_dev: fp32,
 * same shape; device pointers. The engine copies both on `stream` into buffers of its own (allocated at the first bind,
 * sized by max_batch; a handle that never binds allocates nothing), so the caller may release or rewrite its arrays when
 * the call returns, and one captured graph serves every mask. Both NULL clears the binding. Exactly one NULL pointer,
 * or B outside (0, max_batch]: RGN_ERR_INVALID_ARG. rgn_sample_range with a binding whose B differs from the bound
 * condition's fails with RGN_ERR_STATE. rgn_denoise never applies the binding: in the reference the blend belongs to
 * the sampler (p_mean_variance), not to CMDM.forward. */
RGN_API int rgn_set_inpainting(rgn_handle h, int32_t B, const uint8_t* mask_dev, const float* motion_dev, void* stream);

/* Evaluations of at most `rows` token rows (motions x tokens, doubled under guidance) run the small-batch engine:
 * column-split GEMMs that spread one row tile over 16-48 workgroups (rgn_sb.hip; d = 512 models with ff_size a multiple of 32 and >= 512, heads of 16 ... 128, <= 160 tokens, bf16 modes - every
 * other model runs the throughput kernels at every batch size), the
 * latency-bound regime of the reference CLI's own default batch (sample/cgenerate.py:109-135, BASELINE configs[0]).
 * Larger evaluations run the row-complete throughput kernels. -1 restores the default (640, or REGENNET_SB_ROWS);
 * 0 switches the small-batch engine off. Results of the two engines agree within the precision mode's error (both are
 * checked against the same goldens), not bit for bit. */
RGN_API int rgn_set_small_batch_rows(rgn_handle h, int32_t rows);

/* Kernel-selection switches of ONE handle, set between rgn_create and rgn_finalize_weights (afterwards: RGN_ERR_STATE, except "LAYERS_GUIDED" - a dispatch rule,
 * not a packing decision: 0 an evaluation per workgroup and step | 1 a motion per workgroup when 2 B > #CUs (default) | 2 always | -1 the default again): the names of the
 * REGENNET_<KEY> environment variables without the prefix - "LAYERS" (0: kernel per stage instead of the one-kernel decoder stack), "LAYERS_STEPS",
 * "LAYERS_GUIDED", "LAYERS_MIN_B", "MLP_X3", "NO_STEP_FUSION", "STEP_NO_QUADS", "NO_QKV_LONG", "QKV_X3_DMA", "BIG_TILE_ROWS", "SB_ROWS", "SB_GRAPH",
 * "STREAMS", "GRAPH_STEPS", "BULK_F16" (0: no fp16 weight planes, no fp16 phase), "F16_STEPS"; an unknown name is RGN_ERR_BAD_KEY. A handle's option takes precedence over the environment, which remains the process-wide default (tools, A/B runs): tests and
 * library users address one engine without touching global state. Every selectable form meets the same parity bound. */
RGN_API int rgn_set_option(rgn_handle h, const char* key, int32_t value);

/* Evaluations of at least `samples` samples of <= 64 tokens (motions, doubled under guidance) run the one-kernel decoder stack
 * (rgn_layers.hip: one workgroup per sample, whole runs of sampler steps per launch); smaller ones the kernel-per-stage chain, which
 * spreads a small batch over more CUs. -1 restores the default (64, or REGENNET_LAYERS_MIN_B). The two forms differ by bf16 roundings
 * in the plain-bf16 phase (both inside the parity bound): callers that compare a motion drawn alone with its row of a batch - the
 * precision-schedule calibration, bench.py's row check, the row-independence tests - select the batch's form with this knob. */
RGN_API int rgn_set_layers_min_b(rgn_handle h, int32_t samples);

/* arch='gru' handles only (others: RGN_ERR_UNSUPPORTED): the axis the GRU scans, RGN_GRU_SCAN_*. A property of the MODEL, not a kernel-selection
 * switch: the two settings are different functions of the same weights. The default is the reference's (batch): sample b of a call then depends on
 * samples 0 .. b - 1 of that call, and the two halves of a guided evaluation are two independent scans (segments). */
RGN_API int rgn_set_gru_scan(rgn_handle h, int32_t scan);
/* The stack's plan for an evaluation of B motions (arch='gru' handles, after rgn_finalize_weights): scan, independent segments, scan steps S,
 * launches per evaluation (S + num_layers - 1) and the bytes of its state ring. */
RGN_API int rgn_gru_stack_info(rgn_handle h, int32_t B, int32_t guided, int32_t* scan, int32_t* segments, int32_t* steps, int32_t* launches, uint64_t* workspace_bytes);

/* Fills x_dev [B,njoints,nfeats,T] with N(0,1) from the same Philox stream (x_T, gaussian_diffusion.py:706). */
RGN_API int rgn_randn(rgn_handle h, float* x_dev, int32_t B, uint64_t seed, uint64_t sample_offset, void* stream);

/* The noise rgn_sample_range adds at loop index `loop_index` (th.randn_like(x), gaussian_diffusion.py:544 / :792), for
 * callers that run the reference's own per-step loop (p_sample / ddim_sample around rgn_denoise: inpainting masks,
 * y['uncond']) and want the SAME draws as the fused loop for a given (seed, sample_offset): [B,njoints,nfeats,T],
 * value (motion b, feature, frame) = Philox(seed; sample_offset + b, loop_index, feature * 4096 + frame).
 * loop_index = -1 is rgn_randn's x_T draw; loop_index < -1: RGN_ERR_INVALID_ARG. */
RGN_API int rgn_randn_step(rgn_handle h, float* x_dev, int32_t B, uint64_t seed, uint64_t sample_offset, int32_t loop_index, void* stream);

/* Post-processing rows next to the path:
 * rot6d -> rotation matrices, Gram-Schmidt (utils/rotation_conversions.py:513-534): d6 [n,6] -> [n,3,3] */
RGN_API int rgn_rot6d_to_matrix(rgn_handle h, const float* d6_dev, float* mat_dev, int64_t n, void* stream);
/* scipy.ndimage.gaussian_filter1d(x, sigma, axis=-1, mode='reflect') on device (sample/cgenerate.py:142):
 * x [rows, T] -> out [rows, T] */
RGN_API int rgn_gaussian_filter1d(rgn_handle h, const float* x_dev, float* out_dev, int64_t rows, int32_t T,
                          float sigma, void* stream);

/* Replaces Rotation2xyz_x.__call__ / Rotation2xyz.__call__ (model/rotation2xyz.py:158-324 / :11-155) for the posed skeleton joints
 * (jointstype 'smplx' / 'smpl'): the rigid-transform chain of the body layer, G_0 = [R_0 | j_0], G_i = G_parent(i) . [R_i | j_i - j_parent(i)],
 * joint i = translation of G_i; then frames with mask == 0 are set to 0, joint 0 is subtracted, and with TRANSLATION and VERTSTRANS the
 * translation row is added (num_person == 1: relative to frame 0, :318; num_person > 1: as stored, :247-249).
 *   x_dev   fp32 [B, R, C * num_person, T], C = 6 | 3 | 4 | 9 by pose_rep; R = J rotation rows (J - 1 without RGN_R2X_GLOB: joint 0 then takes
 *           axis_angle_to_matrix(glob_rot_host)) plus, with RGN_R2X_TRANSLATION, one last row whose channels p C .. p C + 2 are person p's translation
 *   mask_dev uint8 [B, T] (the storage of a contiguous torch.bool tensor), NULL = every frame
 *   rest_joints_host [J, 3] and parents_host [J] (parents[0] = -1, parents[i] < i): the skeleton, read during the call and passed to the kernel
 *           by value - the call keeps no state and can be captured into a graph
 *   xyz_dev fp32 [B, J, 3 * num_person, T]; rotmat_dev (nullable) fp32 [B, num_person, T, J, 3, 3], the matrices the chain used: for rot6d the
 *           very values rgn_rot6d_to_matrix gives.
 * RGN_ERR_INVALID_ARG, with text: a null pointer, B or T < 1, J outside [1, 64], a parent table that is not a tree in index order, num_person < 1,
 * an unknown pose_rep, RGN_R2X_GLOB unset without glob_rot_host. */
enum { RGN_POSE_ROT6D = 0, RGN_POSE_ROTVEC = 1, RGN_POSE_ROTQUAT = 2, RGN_POSE_ROTMAT = 3 };
enum { RGN_R2X_TRANSLATION = 1, RGN_R2X_GLOB = 2, RGN_R2X_VERTSTRANS = 4 };
RGN_API int rgn_rot2xyz(rgn_handle h, const float* x_dev, const uint8_t* mask_dev /*nullable*/, int32_t B, int32_t T,
                        int32_t J, const float* rest_joints_host /*[J,3]*/, const int32_t* parents_host /*[J]*/,
                        int32_t pose_rep, int32_t num_person, int32_t flags /*RGN_R2X_TRANSLATION | _GLOB | _VERTSTRANS*/,
                        const float* glob_rot_host /*[3] or NULL*/, float* xyz_dev, float* rotmat_dev /*nullable [B,P,T,J,3,3]*/,
                        void* stream);
/* rgn_rot2xyz with a body shape PER FRAME, read on the device: what the reference's wrappers do when they are given a `betas` tensor with one row
 * per frame (model/rotation2xyz.py:289-292 hand it straight to the body layer). Joint j's rest position in frame (b, p, t) is
 *   rest_joints[j] + sum_{k < nb} shape_joints[j, :, k] * betas[b * beta_stride_b + p * beta_stride_p + t * beta_stride_t + k]
 * summed in k order in fp32, and the joint 0 that is subtracted is that frame's own.
 *   shape_joints_dev fp32 [J, 3, nb] (the skeleton file's `shape_joints`, or its first nb directions re-packed), nb in [1, 16]
 *   betas_dev        fp32; the three strides are in ELEMENTS and >= 0, and 0 broadcasts along that axis: a contiguous [B, nb] is (nb, 0, 0),
 *                    [B, P, nb] is (P nb, nb, 0), [B, T, nb] is (T nb, 0, nb), [B, P, T, nb] is (P T nb, T nb, nb). A frame with mask == 0 never
 *                    reads its betas (they may be NaN, or lie outside the allocation).
 * Everything else, rotmat_dev included, is rgn_rot2xyz's, bit for bit; the result of a frame depends on that frame's rows and betas alone. The call
 * enqueues on `stream`, allocates nothing, keeps no state and can be captured into a graph.
 * The arguments are checked before the handle or the device is touched - RGN_ERR_INVALID_ARG for everything rgn_rot2xyz refuses, a null
 * shape_joints_dev or betas_dev, nb outside [1, 16], a negative stride - with text in rgn_last_error(h), or rgn_last_error(NULL) when h is NULL
 * (which is itself RGN_ERR_INVALID_ARG once the other arguments have passed). */
RGN_API int rgn_rot2xyz_shaped(rgn_handle h, const float* x_dev, const uint8_t* mask_dev /*nullable*/, int32_t B, int32_t T, int32_t J,
                               const float* rest_joints_host /*[J,3]*/, const int32_t* parents_host /*[J]*/,
                               const float* shape_joints_dev /*[J,3,nb]*/, int32_t nb, const float* betas_dev, int64_t beta_stride_b,
                               int64_t beta_stride_p, int64_t beta_stride_t, int32_t pose_rep, int32_t num_person, int32_t flags,
                               const float* glob_rot_host /*[3] or NULL*/, float* xyz_dev, float* rotmat_dev /*nullable [B,P,T,J,3,3]*/,
                               void* stream);

/* Replaces the loss arithmetic of GaussianDiffusion.training_losses (diffusion/gaussian_diffusion.py:1313-1391, with masked_l2 :213-225 and the
 * three rot2xyz passes of :1254-1258) for a model output that is already on the device: one row of seven terms per motion,
 *   terms_dev fp32 [B, 7] = rot_mse (:1313), rcxyz_mse (:1317-1321), vel_mse (:1357-1362), fc (:1329-1343), orient (:1367-1377), body (:1378-1383),
 *           transl (:1384-1391)
 * each sum(mask (a - b)^2) / (sum(mask) n_entries) with n_entries = a.shape[1] * a.shape[2] of the tensor the reference hands to masked_l2 - so
 * orient and transl ([B,1,T]) divide by T and body ([B,J,T]) by J T on top of the frame count - and the velocity terms under mask[..., 1:]. A motion
 * whose mask leaves no frame (no frame pair) divides 0 by 0 and gets NaN, as in the reference. All seven are always computed; with RGN_LOSS_FC
 * unset the fc column is 0 and the foot joints are not looked at.
 *   target_dev, output_dev, cmotion_dev fp32 [B, R, 6, T], rot6d rows, R = J + 1: J rotation rows and one last row that the chain and vel_mse leave out
 *   mask_dev uint8 [B, T]: the storage of y['mask'][:, 0, 0, :]
 *   rest_joints_host [J, 3], parents_host [J]: the skeleton, as for rgn_rot2xyz (xyz = rot2xyz(sample, mask=None, vertstrans=False): every frame,
 *           joint 0 subtracted); foot_joints_host [4]: the joints of the fc term (the reference: 7, 10, 8, 11)
 *   transl_row: the row whose channels 0..2 the transl term compares (the reference: 55); vel_threshold: ground-truth foot speed per frame up to
 *           which a foot counts as planted
 * orient's angle is the norm of the reference's matrix_to_axis_angle (utils/rotation_conversions.py:98-120, :482-510), not an acos of the trace.
 * Arithmetic: fp64 from the fp32 inputs, each term rounded to fp32 once (an fp32 evaluation of the reference differs from it by that evaluation's own
 * rounding). One workgroup per motion, sums in a fixed order: a motion's row does not depend on the batch and is the same on every run. The call keeps no
 * state and can be captured into a graph.
 * The arguments are checked before the handle or the device is touched - RGN_ERR_INVALID_ARG for a null pointer, B or T < 1, J outside [1, 64], a
 * parent table that is not a tree in index order, R != J + 1, a foot joint outside [0, J), transl_row outside [0, R), an unknown flag - with text in
 * rgn_last_error(h), or rgn_last_error(NULL) when h is NULL (which is itself RGN_ERR_INVALID_ARG once the other arguments have passed). */
enum { RGN_LOSS_FC = 1 };
enum { RGN_LOSS_ROT_MSE = 0, RGN_LOSS_RCXYZ_MSE, RGN_LOSS_VEL_MSE, RGN_LOSS_FC_TERM, RGN_LOSS_ORIENT, RGN_LOSS_BODY, RGN_LOSS_TRANSL, RGN_LOSS_NTERMS };
RGN_API int rgn_loss_terms(rgn_handle h, const float* target_dev, const float* output_dev, const float* cmotion_dev, const uint8_t* mask_dev,
                           int32_t B, int32_t T, int32_t R, int32_t J, const float* rest_joints_host /*[J,3]*/, const int32_t* parents_host /*[J]*/,
                           const int32_t* foot_joints_host /*[4]*/, int32_t transl_row, float vel_threshold, int32_t flags /*RGN_LOSS_FC*/,
                           float* terms_dev /*[B,7]*/, void* stream);

/* ---- The variational bound of held-out motions: GaussianDiffusion.calc_bpd_loop (diffusion/gaussian_diffusion.py:1546-1601) ----
 * The reference walks the S timesteps of a batch one after the other (one randn_like, one q_sample, one forward and ~25 elementwise ops each).
 * The timesteps of a motion do not depend on one another; here they are ROWS: N = n_t x B rows in (timestep, motion) order, row r belongs to
 * motion b = r % B and carries its own loop index t_dev[r] and its own schedule coefficients. Both calls are stateless, allocate nothing, enqueue
 * on `stream` and can be captured into a graph. `features` = R F (njoints x nfeats), so a row has n = features x T elements; n need be no
 * multiple of anything.
 *
 * rgn_q_sample_rows: q_sample (:245-263) per row,
 *   x_t_dev[r] = coef_dev[r, 0] * x_start_dev[r % B] + coef_dev[r, 1] * noise_r
 * in fp32 with two separately rounded products and one add (no fma): bit-equal to the torch expression on the same noise.
 *   x_start_dev fp32 [B, R, F, T]; coef_dev fp32 [N, 2] = (sqrt_alphas_cumprod[t_r], sqrt_one_minus_alphas_cumprod[t_r]), the fp64 table entries
 *           rounded to fp32 (what _extract_into_tensor(...).float() hands the reference's arithmetic, :1604-1617); t_dev int32 [N]
 *   noise_dev fp32 [N, R, F, T], or NULL: the noise is drawn in the kernel, element (feature, frame) of row r being exactly the value
 *           rgn_randn_step(seed, sample_offset + r % B, loop_index = t_dev[r]) yields - Philox(seed; sample_offset + b, t_r, feature * 4096 + frame).
 *           A motion's x_t at a timestep therefore depends neither on how timesteps are grouped into calls nor on the batch it sits in.
 *   x_t_dev fp32 [N, R, F, T]; noise_out_dev (nullable) fp32 [N, R, F, T] receives the noise that was used.
 *
 * rgn_vb_terms: the terms of _vb_terms_bpd (:1204-1237) and of the loop body (:1584-1587) for a model output that is already on the device,
 *   terms_dev fp32 [N, 3] = (vb, xstart_mse, mse), each a mean over the row's n elements, with p = output (clamped to [-1, 1] under RGN_VB_CLIP,
 *   :366-372), mean_q = c1 x0 + c2 x_t (:265-276) and mean_m = c1 p + c2 x_t (:386):
 *     vb, t != 0   mean(0.5 (-1 + lv_m - lv_q + exp(lv_q - lv_m) + (mean_q - mean_m)^2 exp(-lv_m))) / ln 2      diffusion/losses.py:12-39, :1223-1226
 *     vb, t == 0   mean(-log p_disc) / ln 2: the discretised Gaussian log-likelihood of x0 under (mean_m, 0.5 lv_m) as diffusion/losses.py:42-77
 *                  writes it - the tanh approximation of the normal CDF, the +-1/255 bin, the x < -0.999 / x > 0.999 branches and the clamp at 1e-12
 *                  before each log (:1228-1232). Only rows with t_dev[r] == 0 evaluate it; t_dev is looked at for nothing else.
 *     xstart_mse   mean((p - x0)^2)                                                                             :1585
 *     mse          mean((eps - noise)^2), eps = (sr x_t - p) / srm1                                             :419-423, :1586-1587
 *                  noise_dev == NULL: the column is 0 and no noise is read; the other two columns are unchanged bit for bit.
 *   x_start_dev fp32 [B, R, F, T]; x_t_dev, output_dev, noise_dev (nullable) fp32 [N, R, F, T]; t_dev int32 [N]
 *   coef_dev fp32 [N, 6] = posterior_mean_coef1 (c1), posterior_mean_coef2 (c2), posterior_log_variance_clipped (lv_q), the model's log variance
 *           (lv_m: FIXED_SMALL or FIXED_LARGE, :344-364), sqrt_recip_alphas_cumprod (sr), sqrt_recipm1_alphas_cumprod (srm1) at t_r, each the fp64 table
 *           entry rounded to fp32.
 * Arithmetic: fp64 from the fp32 inputs and the fp32 coefficients, every output rounded to fp32 once (rgn_loss_terms' convention). One workgroup per
 * row, sums in a fixed order, no atomics: a row's three numbers depend neither on N nor on the other rows and are the same on every run.
 *
 * Both check their arguments before the handle or the device is touched - RGN_ERR_INVALID_ARG for a null pointer, B, N, features or T < 1,
 * N % B != 0, a row of more than 2^31 - 1 elements, an unknown flag; rgn_q_sample_rows also for a call of more than 2^31 - 1 workgroups (N times
 * ceil(n / 256)) and, when it draws, for T > 4096 or features > 2^19 (the Philox element counter feature * 4096 + frame) - with text in rgn_last_error(h), or rgn_last_error(NULL) when h is NULL (which is itself
 * RGN_ERR_INVALID_ARG once the other arguments have passed). */
enum { RGN_VB_CLIP = 1 };
enum { RGN_VB_VB = 0, RGN_VB_XSTART_MSE, RGN_VB_MSE, RGN_VB_NTERMS };
RGN_API int rgn_q_sample_rows(rgn_handle h, const float* x_start_dev, const float* noise_dev /*nullable*/, const float* coef_dev /*[N,2]*/,
                              const int32_t* t_dev /*[N]*/, int32_t B, int32_t N, int32_t features, int32_t T, uint64_t seed, uint64_t sample_offset,
                              float* x_t_dev, float* noise_out_dev /*nullable*/, void* stream);
RGN_API int rgn_vb_terms(rgn_handle h, const float* x_start_dev, const float* x_t_dev, const float* output_dev, const float* noise_dev /*nullable*/,
                         const int32_t* t_dev /*[N]*/, const float* coef_dev /*[N,6]*/, int32_t B, int32_t N, int32_t features, int32_t T,
                         int32_t flags /*RGN_VB_CLIP*/, float* terms_dev /*[N,3]*/, void* stream);

/* ---- Joint positions of a HumanML3D / KIT feature vector: recover_from_ric ----
 * Replaces what the reference does after every sampling call of a data_rep='hml_vec' model (sample/cgenerate.py:147-152, sample/edit.py:117-120,
 * :153-155, sample/predict.py:114-117): inv_transform with the dataset's Mean / Std (data_loaders/humanml/data/dataset.py:132) and recover_from_ric
 * (data_loaders/humanml/scripts/motion_process.py:362-381, :415-430; qrot / qinv: data_loaders/humanml/common/quaternion.py:54-73), about fifteen
 * small launches and several [B, T, J, 3] temporaries there, one launch here.
 *   x_dev fp32 [B, D, 1, T]: the model's own layout, the sample as the loop returns it (no permute)
 *   D = 12 J - 1 (263 for the 22 joints of HumanML3D, 251 for the 21 of KIT): 1 rotation velocity, 2 root velocities, 1 root height, 3 (J-1) local
 *           positions, 6 (J-1) rotations, 3 J velocities, 4 contacts. Only rows 0 .. 3 (J-1) + 3 of x_dev, mean_dev and std_dev are read.
 *   mean_dev, std_dev fp32 [D], both given or both NULL (NULL: the features are taken as already de-normalised)
 *   xyz_dev fp32 [B, J, 3, T]: what cgenerate.py:152 forms by view / permute. xyz_dev must NOT overlap x_dev.
 * With f_k[t] = x[k, t] * std[k] + mean[k]:
 *   a[t] = sum_{s < t} f_0[s] (a[0] = 0); q[t] = (cos a[t], 0, sin a[t], 0) - the angle is NOT halved, the frame turns by 2 a, as in the reference;
 *   u[0] = 0, u[t] = qrot(qinv(q[t]), (f_1[t-1], 0, f_2[t-1])) - the velocity of frame t-1 under the angle of frame t, rotated by the INVERSE;
 *   r[t] = sum_{s <= t} u[s] with r[t].y = f_3[t]; joint 0 = r[t]; joint j >= 1 = qrot(qinv(q[t]), (f_{4+3(j-1)}, f_{5+3(j-1)}, f_{6+3(j-1)})[t])
 *   with r[t].x and r[t].z added to its x and z.
 * Arithmetic (rgn_loss_terms' convention): the de-normalisation is fp32, a product and an add rounded separately (no fma) - the bits of the
 * reference's expression on fp32 statistics; both sums, sincos and the rotations are fp64 from those fp32 values; every output is rounded to fp32
 * once. One workgroup per motion, sums in an order fixed by T alone, no atomics: a motion's result depends neither on B nor on its neighbours and is
 * the same on every run. The call enqueues on `stream`, allocates nothing, keeps no state and can be captured into a graph.
 * The arguments are checked before the handle or the device is touched - RGN_ERR_INVALID_ARG for a null x_dev / xyz_dev, one statistic without the
 * other, B < 1, T outside [1, 4096], J outside [2, 64], D != 12 J - 1 - with text in rgn_last_error(h), or rgn_last_error(NULL) when h is NULL
 * (which is itself RGN_ERR_INVALID_ARG once the other arguments have passed). */
RGN_API int rgn_hml_to_joints(rgn_handle h, const float* x_dev, const float* mean_dev /*nullable*/, const float* std_dev /*nullable*/, int32_t B,
                              int32_t T, int32_t D, int32_t J, float* xyz_dev /*[B,J,3,T]*/, void* stream);

/* ---- The metrics of the unconstrained evaluation: KID, and precision / recall of the generated feature manifold ----
 * Replace eval/unconstrained/metrics/kid.py:8-126 (polynomial_mmd_averages, polynomial_mmd, _mmd2_and_variance: per subset three sklearn kernel
 * matrices on the host) and eval/unconstrained/metrics/precision_recall.py:30-53 (manifold_estimate: a Python double loop of torch.norm calls) for
 * features that are already on the device. The three calls take no handle: `device` is the HIP device the pointers live on. They allocate nothing,
 * keep no state, enqueue on `stream` itself and can be captured into a graph; no floating-point atomic is used, so two calls on the same inputs agree
 * bit for bit. The arguments are checked before the device is touched: RGN_ERR_INVALID_ARG with text "<function>: ..." in rgn_last_error(NULL); a
 * negative `device` is refused LAST, after every other argument has passed.
 *
 * rgn_poly_mmd: kid.py:8-126 for S subsets in one call. x_dev fp32 [Nx, D] is the reference's codes_g, y_dev fp32 [Ny, D] its codes_r;
 *   idx_x_dev / idx_y_dev int32 [S, m] are the rows np.random.choice drew for each subset (duplicates are legal: a draw with replacement makes them).
 *   An index outside its set gives an unspecified result, never an access outside the buffers (the in-tree binding checks the draws on the host).
 *   Per subset the three m x m kernel matrices K_XX, K_YY, K_XY over the gathered rows are formed tile by tile and never stored:
 *     dot    on the fp32-input MFMA (v_mfma_f32_32x32x2_f32): exact fp32 products, fp32 accumulation over D
 *     k      s = fl(fl(gamma dot) + coef0), k = s^degree by degree - 1 fp32 multiplications (sklearn's polynomial_kernel on fp32 inputs); gamma is
 *            given (kid.py's default None is 1 / D, rounded to fp32 by the caller)
 *   and everything _mmd2_and_variance reads - the row sums of K_XX and K_YY, both marginals of K_XY, the diagonals of K_XX and K_YY, the three sums of
 *   squares - is reduced in fp64 in a fixed order (regennet_amd/csrc/rgn_metrics.hip states it). mmds_dev fp64 [S] = mmd2 with mmd_est='unbiased',
 *   vars_dev fp64 [S] = var_est with var_at_m = min(Nx, Ny), both evaluated in fp64 as kid.py:87-124 writes them.
 *   Geometry: D a multiple of 4 in [4, 1024]; m in [3, 4096] (var_est divides by m - 2); S in [1, 65535]; Nx, Ny >= 2; degree in [1, 8].
 *   x_dev, y_dev and work_dev 16-byte aligned; work_bytes at least rgn_poly_mmd_workspace(S, m): 8 S (8 + nt) 64 nt bytes, nt = ceil(m / 64).
 *
 * rgn_knn_radius: precision_recall.py:34-42. radii_dev fp32 [N]: r_i = the k-th order statistic (0-based, np.partition(d, k)[k]) of the multiset
 *   { d(A_i, A_j) : j = 0..N-1 }, j = i included, equal distances counted separately. 1 <= k <= 15, k < N <= 2^24.
 * rgn_manifold_hits: precision_recall.py:44-53. flags_dev uint8 [M]: flag_i = any_j ( d(B_i, A_j) <= r_j ), compared in fp32; count_dev int32 [1] = the
 *   number of set flags (the reference's n; its early break changes no result). M, N in [1, 2^24].
 * The distance of both is the DIRECT-DIFFERENCE form of torch.norm(A - A'), never the Gram form |a|^2 + |b|^2 - 2 a.b:
 *   d2 = the fp32 chain acc = fma(t, t, acc), t = fl(a_c - b_c), over c = 0, 1, ..., D - 1 ascending; d = sqrt(d2) correctly rounded.
 * d(A_i, A_i) = 0 and d = 0 between identical rows, exactly; the relative error of a distance is at most (D + 1) 2^-24 however small it is.
 * D a multiple of 4 in [4, 1024]; a_dev and b_dev 16-byte aligned. */
RGN_API int rgn_poly_mmd_workspace(int32_t S, int32_t m, uint64_t* nbytes);
RGN_API int rgn_poly_mmd(int32_t device, const float* x_dev /*[Nx,D]*/, int32_t Nx, const float* y_dev /*[Ny,D]*/, int32_t Ny, int32_t D,
                         const int32_t* idx_x_dev /*[S,m]*/, const int32_t* idx_y_dev /*[S,m]*/, int32_t S, int32_t m, int32_t degree, float gamma,
                         float coef0, double* mmds_dev /*[S]*/, double* vars_dev /*[S]*/, void* work_dev, uint64_t work_bytes, void* stream);
RGN_API int rgn_knn_radius(int32_t device, const float* a_dev /*[N,D]*/, int32_t N, int32_t D, int32_t k, float* radii_dev /*[N]*/, void* stream);
RGN_API int rgn_manifold_hits(int32_t device, const float* b_dev /*[M,D]*/, int32_t M, const float* a_dev /*[N,D]*/, const float* radii_dev /*[N]*/,
                              int32_t N, int32_t D, uint8_t* flags_dev /*[M]*/, int32_t* count_dev /*[1]*/, void* stream);

/* ---- Mesh vertices: jointstype='vertices' ----
 * Replaces the body layer the reference keeps in Rotation2xyz.smpl_model / Rotation2xyz_x.smpl_model (model/rotation2xyz.py:14-15 / :161-162, a CPU
 * smplx layer over a licensed model file): the mesh data of a BODY FILE (tools/make_skeleton.py --mesh), resident on `device`.
 *   v_template_host [V, 3]; posedirs_host [9 (J - 1), 3 V] (NULL: no pose blend shapes); lbs_weights_host [V, J]; shapedirs_host [V, 3, nb]
 *   (NULL with nb = 0); identity_joints_host: the joints whose rotation the wrapper does not hand to the layer (Rotation2xyz_x: jaw and eyes,
 *   22-24, model/rotation2xyz.py:294-301) - they take the identity in the chain, the pose feature and the skinning alike.
 * The arguments are checked before the device is touched: RGN_ERR_INVALID_ARG, with text in rgn_body_last_error(NULL), for V outside [1, 65536],
 * J outside [1, 64], nb outside [0, 16], a null v_template / lbs_weights / out, nb > 0 without shapedirs, an identity joint outside [1, J). */
typedef struct rgn_body_ctx* rgn_body_handle;
RGN_API int rgn_body_create(int32_t device, int32_t V, int32_t J, int32_t nb, const float* v_template_host /*[V,3]*/,
                            const float* posedirs_host /*[9(J-1),3V] or NULL*/, const float* lbs_weights_host /*[V,J]*/,
                            const float* shapedirs_host /*[V,3,nb] or NULL*/, const int32_t* identity_joints_host, int32_t n_identity,
                            rgn_body_handle* out);
RGN_API int rgn_body_destroy(rgn_body_handle b);
RGN_API const char* rgn_body_last_error(rgn_body_handle b);   /* NULL: the calling thread's last failed rgn_body_create */
/* Bytes of device memory rgn_rot2verts needs for B motions of T frames and num_person persons (the shaped template, and per tile of 32 frames the
 * skinning transforms and the pose feature). */
RGN_API int rgn_rot2verts_workspace(rgn_body_handle b, int32_t B, int32_t T, int32_t num_person, uint64_t* nbytes);
/* Replaces Rotation2xyz_x.__call__ / Rotation2xyz.__call__ with jointstype='vertices' (model/rotation2xyz.py:303-321 / :236-249) and, inside them,
 * smplx.lbs.lbs: v_shaped = v_template + shapedirs . betas; v_posed = v_shaped + posedirs^T . (R_j - I)_{j >= 1}; the chain of rgn_rot2xyz with
 * A_j = [Rg_j | tg_j - Rg_j . j_j]; vertex = (sum_j w[v, j] A_j) . [v_posed; 1]. Then frames with mask == 0 are set to 0 and - there is NO root
 * subtraction for vertices - with TRANSLATION and VERTSTRANS the translation row is added (one person: relative to frame 0; several: as stored).
 * x_dev, mask_dev, rest_joints_host (for the body's J joints; with betas: rest + shape_joints . betas, formed by the caller), parents_host, pose_rep,
 * num_person, flags, glob_rot_host and rotmat_dev mean what they mean for rgn_rot2xyz and are checked the same way; betas_host [nb] or NULL (zeros).
 *   verts_dev fp32 [B, V, 3 * num_person, T]
 *   work_dev  rgn_rot2verts_workspace bytes; a smaller work_bytes is RGN_ERR_INVALID_ARG
 * fp32 throughout: the two sums run on the fp32-input MFMA (exact products, k-ordered accumulation). Tiles of 32 consecutive frames that are
 * masked throughout cost no arithmetic; a tile with live frames is computed whole and its masked frames are set to 0. The work is enqueued on `stream` itself; the
 * call allocates nothing, keeps no state and can be captured into a graph. */
RGN_API int rgn_rot2verts(rgn_body_handle b, const float* x_dev, const uint8_t* mask_dev /*nullable*/, int32_t B, int32_t T,
                          const float* rest_joints_host /*[J,3]*/, const int32_t* parents_host /*[J]*/, int32_t pose_rep, int32_t num_person,
                          int32_t flags, const float* glob_rot_host /*[3] or NULL*/, const float* betas_host /*[nb] or NULL*/,
                          float* verts_dev /*[B,V,3P,T]*/, float* rotmat_dev /*nullable [B,P,T,J,3,3]*/, void* work_dev, uint64_t work_bytes,
                          void* stream);
/* rgn_rot2verts with a body shape PER FRAME, read on the device; shape_joints_dev, nb, betas_dev and the three strides are rgn_rot2xyz_shaped's
 * (rest_joints_host is the file's, WITHOUT betas), and nb may be smaller than the body's count of shape directions: the rest count as 0.
 *   v_posed = v_template + [shapedirs; posedirs]^T . [betas; (R_j - I)_{j >= 1}]      one sum on the fp32-input MFMA, the shape terms first, each in k order
 * - no shaped template is ever formed - and the chain and A_j take the frame's own rest joints. rest_joints and shape_joints must belong together
 * with the body's shapedirs (shape_joints = J_regressor . shapedirs) for joints and surface to move together.
 *   work_dev  rgn_rot2verts_shaped_workspace bytes (per tile of 32 frames: the skinning transforms, and the betas ahead of the pose feature)
 * Masked tiles, stream, allocation, state and graph capture as for rgn_rot2verts. The arguments are checked before the handle or the device is touched:
 * RGN_ERR_INVALID_ARG for what rgn_rot2xyz_shaped refuses, then for a NULL handle, nb larger than the body's, a bad parent table, a short workspace;
 * text in rgn_body_last_error(b), or rgn_body_last_error(NULL) when b is NULL. */
RGN_API int rgn_rot2verts_shaped_workspace(rgn_body_handle b, int32_t B, int32_t T, int32_t num_person, uint64_t* nbytes);
RGN_API int rgn_rot2verts_shaped(rgn_body_handle b, const float* x_dev, const uint8_t* mask_dev /*nullable*/, int32_t B, int32_t T,
                                 const float* rest_joints_host /*[J,3]*/, const int32_t* parents_host /*[J]*/,
                                 const float* shape_joints_dev /*[J,3,nb]*/, int32_t nb, const float* betas_dev, int64_t beta_stride_b,
                                 int64_t beta_stride_p, int64_t beta_stride_t, int32_t pose_rep, int32_t num_person, int32_t flags,
                                 const float* glob_rot_host /*[3] or NULL*/, float* verts_dev /*[B,V,3P,T]*/,
                                 float* rotmat_dev /*nullable [B,P,T,J,3,3]*/, void* work_dev, uint64_t work_bytes, void* stream);

/* ---- Regressed joint types: jointstype 'vibe' / 'a2m' / 'a2mpl' ----
 * Replaces what the reference's SMPL layer appends to the chain's joints (model/smpl.py:76-98): the vertex joints its smplx parent picks,
 * vertices[:, vertex_joints], and the extra joints vertices2joints(J_regressor_extra, vertices); all_joints = [J chain joints | Np picked | Jr regressed].
 *   vertex_joints_host [Np] vertex ids in [0, V); regressor_host [Jr, V], finite (rows need not be non-negative or sum to 1); Np or Jr may be 0, not
 *   both, and Np + Jr <= 32.
 * Called once after rgn_body_create (again: the data are replaced). The body is compacted HERE: S = the picks united with the regressor's non-zero
 * columns, ascending, padded to a multiple of 32; v_template, shapedirs, posedirs and lbs_weights are laid down again restricted to S, and the
 * [Np + Jr] x |S| weights as an MFMA operand (picks are selections: exact). RGN_ERR_INVALID_ARG with text in rgn_body_last_error(b) (NULL handle:
 * rgn_body_last_error(NULL)) for bad counts, a missing array, a pick outside [0, V), a non-finite weight. */
RGN_API int rgn_body_set_joint_regressors(rgn_body_handle b, int32_t Np, const int32_t* vertex_joints_host /*[Np]*/, int32_t Jr,
                                          const float* regressor_host /*[Jr,V]*/);
/* Bytes of device memory rgn_rot2joints needs: per tile of 32 frames the skinning transforms, the pose feature and the chain's J joint translations,
 * plus the shaped template of the |S| (padded) vertices. Nothing in it depends on V; no buffer of B * V anything exists. */
RGN_API int rgn_rot2joints_workspace(rgn_body_handle b, int32_t B, int32_t T, int32_t num_person, uint64_t* nbytes);
/* Replaces Rotation2xyz.__call__ (model/rotation2xyz.py:17-155) for the joint types that index the SMPL layer's all_joints (model/smpl.py:66-98):
 *   joints[b, m] = all_joints[map[m]], frames with mask == 0 set to 0, row `root` (an OUTPUT row, JOINTSTYPE_ROOT) subtracted from every row, and
 *   with TRANSLATION and VERTSTRANS the translation row added as rgn_rot2xyz adds it.
 * The arguments are rgn_rot2verts's, with in place of verts_dev: n_map in [1, 64], map_host [n_map] with entries in [0, J + Np + Jr) (repeats
 * allowed; passed to the kernel by value), root in [0, n_map), and
 *   joints_dev fp32 [B, n_map, 3 * num_person, T]
 *   work_dev   rgn_rot2joints_workspace bytes
 * Only the vertices of S are skinned - by the wave body of rgn_rot2verts, so a picked row, before the root row is subtracted, is that call's vertex
 * bit for bit - and they are weighed into joints in registers on the same MFMA shape (exact fp32 products, sums in an order the body alone fixes,
 * no atomics); no vertex is ever written. Masked tiles, stream, allocation, state and graph capture as for rgn_rot2verts. The arguments are checked
 * before the handle or the device is touched, then the handle: RGN_ERR_INVALID_ARG for what rgn_rot2verts refuses, n_map outside [1, 64], a null
 * map, root outside [0, n_map), a negative map entry, a NULL handle, a body without regressors, a map entry >= J + Np + Jr, a short workspace;
 * text in rgn_body_last_error(b), or rgn_body_last_error(NULL) when b is NULL. */
RGN_API int rgn_rot2joints(rgn_body_handle b, const float* x_dev, const uint8_t* mask_dev /*nullable*/, int32_t B, int32_t T,
                           const float* rest_joints_host /*[J,3]*/, const int32_t* parents_host /*[J]*/, int32_t pose_rep, int32_t num_person,
                           int32_t flags, const float* glob_rot_host /*[3] or NULL*/, const float* betas_host /*[nb] or NULL*/, int32_t n_map,
                           const int32_t* map_host /*[n_map]*/, int32_t root, float* joints_dev /*[B,n_map,3P,T]*/,
                           float* rotmat_dev /*nullable [B,P,T,J,3,3]*/, void* work_dev, uint64_t work_bytes, void* stream);
/* rgn_rot2joints with a body shape PER FRAME: the beta arguments of rgn_rot2verts_shaped, with their meaning and their checks. A masked frame's
 * betas are never read. */
RGN_API int rgn_rot2joints_shaped_workspace(rgn_body_handle b, int32_t B, int32_t T, int32_t num_person, uint64_t* nbytes);
RGN_API int rgn_rot2joints_shaped(rgn_body_handle b, const float* x_dev, const uint8_t* mask_dev /*nullable*/, int32_t B, int32_t T,
                                  const float* rest_joints_host /*[J,3]*/, const int32_t* parents_host /*[J]*/,
                                  const float* shape_joints_dev /*[J,3,nb]*/, int32_t nb, const float* betas_dev, int64_t beta_stride_b,
                                  int64_t beta_stride_p, int64_t beta_stride_t, int32_t pose_rep, int32_t num_person, int32_t flags,
                                  const float* glob_rot_host /*[3] or NULL*/, int32_t n_map, const int32_t* map_host /*[n_map]*/, int32_t root,
                                  float* joints_dev /*[B,n_map,3P,T]*/, float* rotmat_dev /*nullable [B,P,T,J,3,3]*/, void* work_dev,
                                  uint64_t work_bytes, void* stream);

/* ---- Rendering: z-buffer rasteriser over the vertices rgn_rot2verts writes ----
 * Replaces render/crendermotion.py:20-42 (render_video: centring, the frame loop, the colours) and render/renderer.py:51-150 (Renderer: pyrender on
 * OSMesa, one scene rebuild per frame). The geometry is the reference's - camera, centring, colours, light positions, background; its PBR material
 * is replaced by the Lambert model below, and its clip volume |Z| <= 1 is NOT reproduced: every Z is drawn.
 *   Input      verts fp32 [B, V, 3 P, T] (person p: channels 3 p .. 3 p + 2), faces int32 [F, 3] shared by all persons, mask uint8 [B, T] or NULL.
 *              The global index of person p's face f is p F + f.
 *   Centring   (params.center != 0; crendermotion.py:24-26) per motion, c = fp32(the mean, summed in fp64, over the vertices of person 0 in the
 *              motion's first unmasked frame); (X, Y, Z) = vertex - c in fp32 for every person and frame of the motion (c = 0 otherwise).
 *   Camera     WeakPerspectiveCamera, cam = (sx, sy, tx, ty), with the reference's 180-degree turn about x (renderer.py:98-99) and the image's row
 *              order folded in:  col = (1 + sx (X + tx)) (W / 2),  row = (1 + sy (Y + ty)) (H / 2)  in fp32 in this order, no contraction;
 *              depth is Z, the smaller Z the nearer. Pixel (i, j) is sampled at its centre (j + 0.5, i + 0.5).
 *   Coverage   exact integer arithmetic. x = clamp(rint(256 col), +-2^20), y likewise: pixel centres sit at (256 j + 128, 256 i + 128). With
 *              E(a -> b; p) = (bx - ax)(py - ay) - (by - ay)(px - ax) in 64 bits, area = E(a -> b; c). area == 0 draws nothing; area < 0 swaps b
 *              and c (two-sided, no culling). e0 = E(b -> c; p), e1 = E(c -> a; p), e2 = E(a -> b; p), e0 + e1 + e2 = area. The pixel is covered
 *              iff for each edge e > 0, or e == 0 and the edge a -> b OWNS its points: dy < 0 (a left edge), or dy == 0 and dx > 0 (a top edge),
 *              with (dx, dy) = b - a after the swap. A centre on an edge two triangles share from opposite sides belongs to exactly one of them.
 *   Depth      z = (fp32(e0) za + fp32(e1) zb + fp32(e2) zc) / fp32(area) in fp32. The winner of a pixel is the smallest z, at equal fp32 z the
 *              lower global face index: the unsigned minimum of (order-preserving bits of z) << 32 | face index, whatever order triangles come in.
 *   Normals    per vertex, the sum over its faces, in ascending face order, of (v1 - v0) x (v2 - v0) of the centred positions, divided by its
 *              length (0 stays 0); per pixel n = b0 na + b1 nb + b2 nc with b_k = fp32(e_k) / fp32(area), normalised the same way, negated if
 *              n_Z > 0 (away from the camera).
 *   Shading    I = 0.4 + 0.2 sum_l max(0, n . normalize(L_l - p)), p = (b-interpolated X, Y, and z), L = (0, 1, -1), (0, -1, -1), (1, -1, -2):
 *              the reference's three point lights (renderer.py:72-82) in vertex coordinates, its ambient 0.4, and the weight at which three
 *              fully lit lights give exactly 1. rgb = rint(255 base_p I), clamped to [0, 255]; person p takes colors[min(p, 7)].
 *   Output     rgb uint8 [B, T, H, W, 3]; depth fp32 [B, T, H, W] (nullable; +inf on background); face int32 [B, T, H, W] (nullable; global face
 *              index, -1 on background). Uncovered pixels, and every pixel of a masked frame, are rint(255 background). */
#define RGN_RENDER_MAX_PERSONS 8
typedef struct {
    int32_t width, height;                          /* [1, 4096] each (crendermotion.py:109-110: 1024 x 1024) */
    float cam[4];                                   /* sx, sy, tx, ty (crendermotion.py:20: 0.75, 0.75, 0, 0.10) */
    int32_t center;                                 /* crendermotion.py:24-26 */
    float colors[RGN_RENDER_MAX_PERSONS][3];        /* base colours in [0, 1] (crendermotion.py:20, renderer.py:86-89) */
    float background[3];                            /* in [0, 1] (renderer.py:155: white) */
} rgn_render_params;
/* A renderer for one mesh topology on `device`: uploads faces and the vertex -> face adjacency built from them. Replaces Renderer.__init__
 * (renderer.py:52-83) with its faces file. The arguments are checked before the device is touched: RGN_ERR_INVALID_ARG, with text in
 * rgn_render_last_error(NULL), for V outside [1, 65536], F < 1, null faces / out, a face index outside [0, V). */
typedef struct rgn_render_ctx* rgn_render_handle;
RGN_API int rgn_render_create(int32_t device, int32_t V, int32_t F, const int32_t* faces_host /*[F,3]*/, rgn_render_handle* out);
RGN_API int rgn_render_destroy(rgn_render_handle r);
RGN_API const char* rgn_render_last_error(rgn_render_handle r);   /* NULL: the calling thread's last failed rgn_render_create */
/* Bytes of device memory rgn_render needs for B motions of T frames and num_person persons (per frame and person: 40 bytes a vertex, about 8 a
 * face; it does not depend on the image size, which is only checked). */
RGN_API int rgn_render_workspace(rgn_render_handle r, int32_t B, int32_t T, int32_t num_person, int32_t width, int32_t height, uint64_t* nbytes);
/* Replaces Renderer.render (renderer.py:85-150) for every frame of B motions at once. RGN_ERR_INVALID_ARG, with text: width or height outside
 * [1, 4096], B, T or num_person < 1, num_person x F >= 2^31, null verts / rgb / work / params, a work_bytes below rgn_render_workspace's, a
 * work_dev that is not 16-byte aligned, a batch larger than one launch covers (B x T x num_person x max(V, F) items or
 * B x T x tiles of 64 x 64 pixels above 2^24 - 1 workgroups). The work is enqueued on `stream` itself; the call allocates nothing,
 * keeps no state and can be captured into a graph. Non-finite vertices give unspecified pixels, never an access outside the buffers. */
RGN_API int rgn_render(rgn_render_handle r, const float* verts_dev /*[B,V,3P,T]*/, const uint8_t* mask_dev /*nullable [B,T]*/, int32_t B, int32_t T,
                       int32_t num_person, const rgn_render_params* params, uint8_t* rgb_dev /*[B,T,H,W,3]*/, float* depth_dev /*nullable [B,T,H,W]*/,
                       int32_t* face_dev /*nullable [B,T,H,W]*/, void* work_dev, uint64_t work_bytes, void* stream);

/* Introspection for bench/profiling: name and accumulated HIP-event time (ms) + launch count of the
 * internal kernel classes since the last reset; timing is only collected when enabled. */
RGN_API int rgn_profile_enable(rgn_handle h, int32_t on);
RGN_API int rgn_profile_query(rgn_handle h, int32_t idx, const char** name, double* total_ms, int64_t* launches);
/* The engine's own plan for ONE denoiser evaluation of a sampling loop over B motions (2 B rows when `guided`), in the plain-bf16
 * phase of the precision schedule (split_phase = 0) or its split-bf16 tail (1): for kernel class idx (the classes of rgn_profile_query)
 * the concrete kernel, launches per evaluation (single kernel chain; 0 for k_layers<true>, which is ONE launch per run of steps),
 * the algorithmic FLOPs those launches carry (2 x MAC, full T x T scores) and, for the one-kernel forms, the weight
 * fragment bytes their workgroups stream from L2. Filled by the code that dispatches (plan_eval in rgn_plan.cpp), so a benchmark prices
 * exactly what the engine launches. */
RGN_API int rgn_plan_query(rgn_handle h, int32_t B, int32_t guided, int32_t split_phase, int32_t idx, const char** name,
                           const char** kernel, double* launches_per_eval, double* algo_flops_per_eval, double* l2_bytes_per_eval);
/* Time (ms) one event pair measures around a one-thread no-op kernel on this handle's stream: the dispatch + event
 * latency every bracket of rgn_profile_query carries on top of the kernel itself (calibrated at the first enable). */
RGN_API int rgn_profile_bracket_overhead(rgn_handle h, double* ms);

/* ---- Evaluation harness next to the sampler: the ST-GCN feature extractor / action classifier ----
 * Replaces eval/a2m/recognition/models/stgcn.py:28-123 (STGCN) as used by eval/a2m/stgcn/evaluate.py:9-45: the features
 * feed FID / diversity / multimodality, yhat the accuracy. Checkpoint keys are the reference's state_dict names
 * ('A', 'data_bn.*', 'st_gcn_networks.<i>.{gcn.conv,tcn.0,tcn.2,tcn.3,residual.0,residual.1}.*', 'edge_importance.<i>',
 * 'fcn.*'); '*.num_batches_tracked' entries are accepted and ignored. */
typedef struct rgn_stgcn_ctx* rgn_stgcn_handle;
typedef struct {
    int32_t in_channels;    /* nfeats of batch['output'] = C * num_person (evaluate.py:15; 12 for two persons in rot6d) */
    int32_t num_class;      /* evaluate.py:16 */
    int32_t num_person;     /* evaluate.py:17 */
    int32_t num_nodes;      /* V: graph nodes = joints (56 for the 'smplx' layout, stgcnutils/graph.py:81-82) */
    int32_t num_frames;     /* T of batch['output'] */
    int32_t max_batch;
    int32_t device;
} rgn_stgcn_config;
RGN_API int rgn_stgcn_create(const rgn_stgcn_config* cfg, rgn_stgcn_handle* out);
RGN_API int rgn_stgcn_destroy(rgn_stgcn_handle h);
RGN_API const char* rgn_stgcn_last_error(rgn_stgcn_handle h);
/* host fp32 copies of the checkpoint tensors (model.load_state_dict, evaluate.py:24-25) */
RGN_API int rgn_stgcn_load_weight(rgn_stgcn_handle h, const char* ref_key, const float* host, const int64_t* shape, int32_t ndim);
/* The block plan: (out_channels[i], strides[i]) of the st_gcn blocks, between rgn_stgcn_create and rgn_stgcn_finalize. Default: the ten blocks of
 * eval/a2m/recognition/models/stgcn.py:51-62; the extractor of the unconstrained evaluation (eval/unconstrained/models/stgcn.py:52-63, built by
 * eval/unconstrained/evaluate.py:21-32) has six: (64,1) (64,1) (64,1) (128,2) (128,1) (256,2). Accepted: 2 to 10 blocks, channels from {64, 128, 256}
 * that never decrease and end at 256 (the features are [N, 256]), stride 1 or 2 with stride 2 only where the channel count changes. Block 0 has no
 * residual; a later block has the convolved shortcut exactly when its channel count or stride changes (st_gcn.__init__). Anything else:
 * RGN_ERR_INVALID_ARG with the offending entry named; after finalize: RGN_ERR_STATE. rgn_stgcn_finalize then asks for the keys of the plan's blocks
 * and refuses (RGN_ERR_BAD_KEY, first such key named) a checkpoint that holds 'st_gcn_networks.<i>' / 'edge_importance.<i>' of a block the plan lacks. */
RGN_API int rgn_stgcn_set_blocks(rgn_stgcn_handle h, int32_t n_blocks, const int32_t* out_channels, const int32_t* strides);
/* the plan rules alone, without a handle or a device: RGN_OK, or RGN_ERR_INVALID_ARG with the message (NUL-terminated, cut to cap) in err (nullable) */
RGN_API int rgn_stgcn_check_blocks(int32_t n_blocks, const int32_t* out_channels, const int32_t* strides, char* err, int32_t cap);
/* folds every BatchNorm (eval mode) and the edge importance into the convolutions; RGN_ERR_MISSING_KEY names what is absent.
 * Graphs of fewer than 28 nodes (the 15-node 'openpose' graph of the unconstrained evaluation, the 25-node 'smpl' layout of
 * eval/a2m/stgcn/evaluate.py:11-12) run on a vertex count padded to 16 / 20 / 24 / 28 inside the engine; num_nodes and the input keep the real V. */
RGN_API int rgn_stgcn_finalize(rgn_stgcn_handle h);
/* Kernel-selection switches of ONE recogniser handle (like rgn_set_option; any time before a forward): "SG_NO_WINDOW" (row-shifted GEMMs instead of the
 * LDS-window temporal convolutions), "SG_NO_GCN_FUSE" (aggregation and 1x1 convolution as two launches), "SG_NO_TAIL_FUSE" (k_sg_post for every block), "SG_NO_POLY_TAIL" (... for the two blocks with polyphase output),
 * "SG_NO_S2_WINDOW" (stride-2 blocks as row-shifted GEMM + shortcut GEMM), "SG_TCONV_SMALL" (256-row tiles), "SG_GCN_BN" (widest aggregation tile: 64 |
 * 128 | 256), "SG_GCN_STEP32" (64-wide aggregation tiles: one barrier per 32-deep k-block), "SG_NO_BLOCK0_FUSE" (the first block's graph convolution as aggregation + split GEMM instead of one fp32 kernel). A handle's option takes precedence over REGENNET_<KEY> in the environment; unknown names are RGN_ERR_BAD_KEY. Every form meets the same
 * parity bound (tests/test_eval_gpu.py runs each against the reference's outputs).
 * "SG_F16" (0 | 1, default 0) is not a kernel form but the ARITHMETIC: blocks 1-9 and block 0's temporal convolution on single IEEE fp16 operand planes, one MFMA per
 * product instead of the split-bf16 three (features within 1.5e-3 of the largest feature - measured 4e-4 - instead of 1e-4 / 5e-6; about twice the speed). It exists
 * for the fused kernels only: rgn_stgcn_forward returns RGN_ERR_UNSUPPORTED, with the reason in rgn_stgcn_last_error, for a graph / shape / SG_NO_* selection they do
 * not cover or a checkpoint with a folded weight of magnitude >= 6e4 (key named) - never a silent change of arithmetic. */
RGN_API int rgn_stgcn_set_option(rgn_stgcn_handle h, const char* key, int32_t value);
/* STGCN.forward (stgcn.py:76-123): output_dev fp32 [N, num_nodes, in_channels, T] (batch['output']) ->
 * features_dev fp32 [N, 256] (batch['features'], nullable) and yhat_dev fp32 [N, num_class] (batch['yhat'], nullable) */
RGN_API int rgn_stgcn_forward(rgn_stgcn_handle h, int32_t N, const float* output_dev, float* features_dev, float* yhat_dev, void* stream);

/* ---- The action2motion evaluation's recogniser: a GRU action classifier ----
 * Replaces eval/a2m/action2motion/models.py:6-61 (MotionDiscriminator: nn.GRU(input_size, hidden_size, hidden_layer) -> Linear(hidden_size, 30) -> tanh
 * -> Linear(30, output_size); MotionDiscriminatorForFID stops behind the tanh) as eval/a2m/action2motion/evaluate.py:18-30 and accuracy.py:4-14 use it:
 * the features feed FID / diversity / multimodality, the logits the accuracy. Checkpoint keys are the reference's state_dict names:
 * 'recurrent.weight_ih_l<k>' [3 H, input_size or H], 'recurrent.weight_hh_l<k>' [3 H, H], 'recurrent.bias_ih_l<k>', 'recurrent.bias_hh_l<k>' [3 H]
 * (gate order r, z, n), 'linear1.weight' [lin1_size, H], 'linear1.bias', 'linear2.weight' [output_size, lin1_size], 'linear2.bias'.
 * Arithmetic: fp32 throughout - every product exact (the fp32-input MFMA v_mfma_f32_16x16x4_f32 for the gates, fma chains for the head), sums in an
 * order the geometry alone fixes, no atomics: a sequence's outputs are the same bits whatever batch it sits in and on every run. */
typedef struct rgn_gru_ctx* rgn_gru_handle;
typedef struct {
    int32_t input_size;     /* njoints * nfeats of batch['output_xyz'] (72 for HumanAct12, evaluate.py:11; models.py:22-23) */
    int32_t hidden_size;    /* 128 (models.py:69) */
    int32_t num_layers;     /* 2 (models.py:69) */
    int32_t lin1_size;      /* 30 (models.py:16) */
    int32_t output_size;    /* num_classes (models.py:17) */
    int32_t device;         /* HIP device ordinal */
} rgn_gru_config;
/* MotionDiscriminator.__init__ (models.py:7-17). The geometry is checked before the device is touched - RGN_ERR_UNSUPPORTED with the reason in
 * rgn_gru_last_error(NULL) unless hidden_size is a multiple of 32 in [32, 256], 1 <= num_layers <= 4, 1 <= input_size <= 1024 (padded to the MFMA's k
 * granule inside the engine), 1 <= lin1_size <= 64, 1 <= output_size <= 1024 - then the device: RGN_ERR_HIP, "no HIP device". */
RGN_API int rgn_gru_create(const rgn_gru_config* cfg, rgn_gru_handle* out);
RGN_API int rgn_gru_destroy(rgn_gru_handle h);
RGN_API const char* rgn_gru_last_error(rgn_gru_handle h);    /* NULL: the calling thread's last failed call without a handle */
/* classifier.load_state_dict(model["model"]) (models.py:69, :77), one host fp32 tensor per call: an unknown key, or a key given twice, is
 * RGN_ERR_BAD_KEY; a shape other than the configuration's RGN_ERR_BAD_SHAPE (both shapes in the text). */
RGN_API int rgn_gru_load_weight(rgn_gru_handle h, const char* ref_key, const float* host, const int64_t* shape, int32_t ndim);
/* Every key seen once (RGN_ERR_MISSING_KEY names the absent ones); the recurrent weights are packed in MFMA operand order, b_ih + b_hh folded for the
 * r and z gates (kept apart for n, where r multiplies W_hn h + b_hn), and everything is uploaded. */
RGN_API int rgn_gru_finalize(rgn_gru_handle h);
/* MotionDiscriminator.forward / MotionDiscriminatorForFID.forward (models.py:20-38 / :45-61) for N sequences of T frames in one launch:
 *   x_dev       fp32 [N, input_size, T]: the reference's [bs, njoints, nfeats, T] as it lies, frames innermost (no permuted copy is made, :23-24)
 *   lengths_dev int64 [N], 1 <= lengths[n] <= T: the state behind frame lengths[n] - 1 is selected (:31); frames at or behind a sequence's length
 *               are never looked at (they may be NaN), and a workgroup stops at the longest length of its 16 sequences. Lengths are read on the device
 *               only: one outside [1, T] is CLAMPED into it - nothing outside x is ever read - and flagged (rgn_gru_length_status)
 *   h0_dev      fp32 [num_layers, N, hidden_size]: hidden_unit (:25-27; the caller draws it)
 *   features_dev fp32 [N, lin1_size] = tanh(linear1(out)) (:34-35), nullable; logits_dev fp32 [N, output_size] = linear2(features) (:37), nullable
 * The arguments are checked before the handle or the device is touched - RGN_ERR_INVALID_ARG for a null x / lengths / h0, both outputs null, N < 1,
 * T outside [1, 4096] - with text in rgn_gru_last_error(h), or rgn_gru_last_error(NULL) when h is NULL (which is itself RGN_ERR_INVALID_ARG once the
 * other arguments have passed). The call enqueues on `stream`, allocates nothing and can be captured into a graph. */
RGN_API int rgn_gru_forward(rgn_gru_handle h, int32_t N, int32_t T, const float* x_dev, const int64_t* lengths_dev, const float* h0_dev,
                            float* features_dev /*nullable*/, float* logits_dev /*nullable*/, void* stream);
/* *clamped = 1 when a forward since the last query (or since finalize) met a length outside [1, T], else 0; synchronises the device and clears the flag. */
RGN_API int rgn_gru_length_status(rgn_gru_handle h, int32_t* clamped);

/* ---- The text-to-motion evaluation: movement encoder, bidirectional-GRU co-embedding encoders, matching ----
 * Replaces data_loaders/humanml/networks/modules.py:79-98 (MovementConvEncoder), :311-350 (TextEncoderBiGRUCo) and :353-386 (MotionEncoderBiGRUCo) as
 * data_loaders/humanml/networks/evaluator_wrapper.py:121-187 (EvaluatorMDMWrapper) drives them, and the distance / top-k part of
 * data_loaders/humanml/utils/metrics.py:6-56 as eval/eval_humanml.py:20-71 uses it. Checkpoint keys are the reference's state_dict names behind the
 * sub-model's prefix ('movement_encoder.', 'text_encoder.', 'motion_encoder.'): 'movement_encoder.main.0.weight' [Hm, dim_pose - 4, 4],
 * 'motion_encoder.gru.weight_hh_l0_reverse' [3 H, H], 'text_encoder.hidden' [2, 1, Ht], 'motion_encoder.output_net.1.weight' [H] (the LayerNorm) ...
 * Arithmetic: fp32 throughout, products exact (v_mfma_f32_16x16x4_f32, fma chains), sums in an order the geometry alone fixes, no atomics: a sequence's
 * outputs are the same bits whatever batch it sits in, at whatever place, and on every run. */
typedef struct rgn_t2m_ctx* rgn_t2m_handle;
typedef struct {
    int32_t device;            /* HIP device ordinal */
    int32_t dim_pose;          /* 263 (humanml) or 251 (kit): evaluator_wrapper.py:134; the encoder reads the first dim_pose - 4 (:165) */
    int32_t movement_hidden;   /* 512 (:135) */
    int32_t movement_latent;   /* 512 (:136) */
    int32_t motion_hidden;     /* 1024 (:130) */
    int32_t dim_word;          /* 300 (:127) */
    int32_t dim_pos_ohot;      /* 15 = len(POS_enumerator) (:129) */
    int32_t text_hidden;       /* 512 (:132) */
    int32_t coemb;             /* 512 (:133) */
    int32_t unit_length;       /* 4 (:138) */
} rgn_t2m_config;
/* build_evaluators (evaluator_wrapper.py:95-106). The geometry is checked before the device is touched - RGN_ERR_UNSUPPORTED with the reason in
 * rgn_t2m_last_error(NULL) unless the four hidden sizes are multiples of 64 in [64, 1024], 5 <= dim_pose <= 1024, dim_word and coemb multiples of 4 in
 * [4, 1024], 1 <= dim_pos_ohot <= 1024, unit_length == 4 - then the device: RGN_ERR_HIP, "no HIP device". */
RGN_API int rgn_t2m_create(const rgn_t2m_config* cfg, rgn_t2m_handle* out);
RGN_API int rgn_t2m_destroy(rgn_t2m_handle h);
RGN_API const char* rgn_t2m_last_error(rgn_t2m_handle h);    /* NULL: the calling thread's last failed call without a handle */
/* load_state_dict(checkpoint['movement_encoder' | 'text_encoder' | 'motion_encoder']) (evaluator_wrapper.py:114-116), one host fp32 tensor per call:
 * an unknown key, or a key given twice, is RGN_ERR_BAD_KEY; a shape other than the configuration's RGN_ERR_BAD_SHAPE (both shapes in the text). */
RGN_API int rgn_t2m_load_weight(rgn_t2m_handle h, const char* ref_key, const float* host, const int64_t* shape, int32_t ndim);
/* Every key seen once (RGN_ERR_MISSING_KEY names the absent ones); weights are packed in MFMA operand order and uploaded. */
RGN_API int rgn_t2m_finalize(rgn_t2m_handle h);
/* Bytes of device workspace that serve any of the calls below at up to N sequences, T frames and Lw words (monotone in each). RGN_ERR_INVALID_ARG for
 * N outside [1, 2^19], T outside [4, 4096], Lw outside [1, 256]. SIZE: every stage's rows are kept, and the hoisted gate inputs [N, T2, 2, 3 H] fp32
 * dominate - at the real geometry 1.9 MB per 196-frame motion, of which the gate inputs are 1.2 MB: 59 MB at N = 32, 1.9 GB at N = 1024. A caller
 * short of memory evaluates in batches (the harness's are 32). */
RGN_API int rgn_t2m_workspace(rgn_t2m_handle h, int32_t N, int32_t T, int32_t Lw, size_t* bytes);
/* MovementConvEncoder.forward (modules.py:94-98; dropout is off in eval mode): x_dev fp32, frame t of motion n at x_dev + (n T + t) in_stride, the first
 * dim_pose - 4 values read -> mov_dev fp32 [N, T2, movement_latent], T1 = (T-2)/2+1, T2 = (T1-2)/2+1. m_lens_dev int64 [N] nullable: with it only
 * movement frames j < m_lens[n] / unit_length (clamped into [1, T2] and flagged) are computed and stored, and input frames at or behind
 * 4 (m_lens[n] / 4) + 3 are never read (they may be NaN); without it every frame. */
RGN_API int rgn_t2m_movements(rgn_t2m_handle h, int32_t N, int32_t T, int32_t in_stride, const float* x_dev, const int64_t* m_lens_dev /*nullable*/,
                              float* mov_dev, void* work, size_t work_bytes, void* stream);
/* MotionEncoderBiGRUCo.forward (modules.py:373-386): mov_dev fp32 [N, T2, movement_latent], lens_dev int64 [N] in [1, T2] (movement frames; clamped and
 * flagged otherwise; frames at or behind a length are never read) -> emb_dev fp32 [N, coemb]. */
RGN_API int rgn_t2m_encode_movements(rgn_t2m_handle h, int32_t N, int32_t T2, const float* mov_dev, const int64_t* lens_dev, float* emb_dev, void* work,
                                     size_t work_bytes, void* stream);
/* EvaluatorMDMWrapper.get_motion_embeddings (evaluator_wrapper.py:175-187) without its sort: motions_dev fp32 [N, T, dim_pose], m_lens_dev int64 [N] in
 * frames -> emb_dev fp32 [N, coemb], row n for motion n. The two calls above in one; the movements stay in the workspace. */
RGN_API int rgn_t2m_motion_embeddings(rgn_t2m_handle h, int32_t N, int32_t T, const float* motions_dev, const int64_t* m_lens_dev, float* emb_dev,
                                      void* work, size_t work_bytes, void* stream);
/* TextEncoderBiGRUCo.forward (modules.py:335-350): word_embs_dev fp32 [N, Lw, dim_word], pos_ohot_dev fp32 [N, Lw, dim_pos_ohot], cap_lens_dev int64 [N]
 * in [1, Lw] (clamped and flagged otherwise; word rows at or behind a length are never read) -> emb_dev fp32 [N, coemb]. Rows need not be sorted by
 * length (pack_padded_sequence demands it; the kernels are order-free).
 * All four calls check their arguments before the handle or the device is touched (RGN_ERR_INVALID_ARG, text in rgn_t2m_last_error(h), or (NULL) when
 * h is NULL), enqueue on `stream`, allocate nothing and can be captured into a graph. */
RGN_API int rgn_t2m_text_embeddings(rgn_t2m_handle h, int32_t N, int32_t Lw, const float* word_embs_dev, const float* pos_ohot_dev,
                                    const int64_t* cap_lens_dev, float* emb_dev, void* work, size_t work_bytes, void* stream);
/* *clamped = 1 when a call since the last query (or since finalize) met a length outside its range, else 0; synchronises the device, clears the flag. */
RGN_API int rgn_t2m_length_status(rgn_t2m_handle h, int32_t* clamped);
/* euclidean_distance_matrix + argsort + calculate_top_k (metrics.py:6-44) and calculate_matching_score (:47-56) on consecutive groups of `group` <= 32
 * (text, motion) pairs, as eval_humanml.py:36-45 applies them per batch: d[i, j] = || text_i - motion_j || by direct differences in fp32 (not the
 * reference's -2ab + a^2 + b^2, which cancels); diag_dev fp32 [N] = d[i, i] (the matching-score terms); rank_dev int32 [N] = #{ j in the group :
 * d[i, j] < d[i, i] }. Top-k hit <=> rank < k. TIES: a motion exactly as far as the true one does not count against it (the reference's argsort breaks
 * such a tie by position). The last group may be short. D a multiple of 4 in [4, 1024]. Errors in rgn_t2m_last_error(NULL). */
RGN_API int rgn_t2m_match(int32_t device, const float* text_dev, const float* motion_dev, int32_t N, int32_t D, int32_t group, float* diag_dev,
                          int32_t* rank_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* REGENNET_HIP_H */
