/* hcflow.h -- C ABI of the MI355X-native HCFlow forward / inverse engine (libhcflow_hip.so).
 *
 * The reference (JingyunLiang/HCFlow) is pure PyTorch: its drop-in boundary is the Python class
 * looked up by codes/models/networks.py:36-41 (define_G -> HCFlowNet_SR / HCFlowNet_Rescaling with
 * forward(hr, lr, z, u, eps_std, add_gt_noise, step, reverse, training),
 * codes/models/modules/HCFlowNet_SR_arch.py:34-42, HCFlowNet_Rescaling_arch.py:26-36). There is no
 * FFI in the reference, so this C ABI sits directly beneath that class: hcflow_amd/arch.py keeps
 * the reference's module surface and state_dict and forwards every call to the entry points
 * below (last row). Each entry point names the reference code it replaces.
 *
 * Conventions: plain pointers and sizes, no torch types. Return 0 on success, a negative HCF_ERR_*
 * code otherwise (never throws); hcf_last_error() gives a message. Image tensors are dense NCHW
 * fp32 DEVICE pointers owned by the caller; parameters are passed as HOST pointers and packed /
 * uploaded by hcf_finalize(). All work is enqueued on the caller's HIP stream; hcf_inverse / hcf_forward_sr /
 * hcf_forward_rescale never synchronise with the device once the workspace has reached its steady-state size (the first call
 * per shape sizes and may allocate it): a steady-state call walks the layer graph once and returns, so it can be captured into
 * a HIP graph. The f16x3 range flag is read back asynchronously; hcf_check_range() is the call that waits for it.
 */
#ifndef HCFLOW_H_
#define HCFLOW_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HCF_OK 0
#define HCF_ERR_ARG (-1)
#define HCF_ERR_HIP (-2)
#define HCF_ERR_STATE (-3)
#define HCF_ERR_KEY (-4)
#define HCF_ERR_SHAPE (-5)
#define HCF_ERR_UNSUPPORTED (-6)
#define HCF_ERR_NOMEM (-7)

/* enum values used in hcf_config */
#define HCF_KIND_SR 0
#define HCF_KIND_RESCALING 1
#define HCF_SQUEEZE_CHECKERBOARD 0
#define HCF_SQUEEZE_HAAR 1
#define HCF_PERM_INVCONV 0
#define HCF_PERM_NONE 1
#define HCF_COUPLING_AFFINE 0
#define HCF_COUPLING_AFFINE3SHIFT 1
#define HCF_NN_FCN 0
#define HCF_NN_DENSEBLOCK 1

/* flags for hcf_inverse / hcf_forward_* */
#define HCF_FLAG_NO_CLAMP 1u        /* return the flow output before torch.clamp(.,0,1) (parity tests) */
#define HCF_FLAG_NO_RANGE_CHECK 2u  /* f16x3 mode: do not even enqueue the read-back of the range flag (hcf_check_range) */
#define HCF_FLAG_KEEP_COND 4u       /* hcf_inverse: compute the deepest level's conditional features + prior head and keep them */
#define HCF_FLAG_REUSE_COND 8u      /* hcf_inverse: the caller asserts that lr (contents, B, h, w) is the one of the previous
                                     * KEEP / REUSE call: the kept features are used if still valid (else recomputed and kept).
                                     * They depend on lr only (FlowNet_SR_x4.py:113-115, FlowNet_SR_x8.py:129), so a tau sweep or
                                     * repeated sampling of one LR batch skips that level's RRDB trunks; results are bit-identical. */

/* numerics of the convolutions (hcf_set_precision) */
#define HCF_PRECISION_EXACT 0       /* exact fp32 MFMA (v_mfma_f32_32x32x2_f32) */
#define HCF_PRECISION_F16X3 1       /* fp32-equivalent: 3 f16 MFMAs per product block, fp32 accumulate */

typedef void* hcf_stream_t;        /* a hipStream_t */
typedef struct hcf_engine hcf_engine;

/* The yml network_G block as the reference reads it in FlowNet.__init__
 * (FlowNet_SR_x4.py:17-27, FlowNet_SR_x8.py, FlowNet_Rescaling_x4.py:15-29) and
 * ConditionalFlow.__init__ (ConditionalFlow.py:15-41). */
typedef struct hcf_config {
  int32_t kind;             /* HCF_KIND_* : HCFlowNet_SR or HCFlowNet_Rescaling */
  int32_t scale;            /* 4 or 8 (= 2^L) */
  int32_t in_nc;            /* network_G.in_nc (3) */
  float quant;              /* opt.quant (SR) / datasets.train.quant (rescaling) */
  int32_t L;                /* flowDownsampler.L : 2 or 3 */
  int32_t K[4];             /* flowDownsampler.K per level */
  int32_t after[4];         /* splitOff.after_flowstep per level */
  int32_t squeeze;          /* HCF_SQUEEZE_* */
  int32_t perm, coupling, nn_module, hidden;          /* main flow steps */
  int32_t c_perm, c_coupling, c_nn_module, c_hidden;  /* conditional (splitOff) flow steps */
  int32_t rrdb_nb[2];
  int32_t rrdb_nf, rrdb_gc;
  int32_t lu_decomposed;    /* FlowStep(LU_decomposed=...) (FlowStep.py:9-10,20): every invertible 1x1 conv holds the factors
                             * l, log_s, u (parameters) and p, sign_s (buffers) of W = P (L o mask + I) (U o mask^T + diag(sign_s
                             * exp(log_s))) instead of `weight` (Permutations.py:41-57,78-92); dlogdet = sum(log_s) * pixels */
} hcf_config;

/* ---- life cycle -------------------------------------------------------------------------- */
/* Replaces HCFlowNet_SR.__init__ / HCFlowNet_Rescaling.__init__ -> FlowNet.__init__
 * (HCFlowNet_SR_arch.py:12-31). Touches no device. */
int hcf_create(const hcf_config* cfg, hcf_engine** out);
void hcf_destroy(hcf_engine* e);
const char* hcf_last_error(const hcf_engine* e);

/* state_dict introspection: the keys / shapes the reference modules register, in registration
 * order (SURVEY.md 8b "State-dict (strict)"). shape has up to 4 entries. */
int hcf_param_count(const hcf_engine* e);
int hcf_param_info(const hcf_engine* e, int index, const char** key, int32_t* ndim, int64_t shape[4]);

/* Replaces nn.Module.load_state_dict(strict=True) as used by BaseModel.load_network
 * (codes/models/base_model.py:96-120): one call per tensor with a HOST fp32 pointer. */
int hcf_set_param(hcf_engine* e, const char* key, const float* host_data, const int64_t* shape, int32_t ndim);

/* Pack weights for the kernels (implicit-GEMM layout, ActNorm folded into conv epilogues, W^-1 in
 * fp64 as Permutations.py:74 does, slogdet hoisted out of the pass) and upload to `device`.
 * Must be called after the last hcf_set_param and again whenever parameters change. */
int hcf_finalize(hcf_engine* e, int device);

/* ---- the hot path -------------------------------------------------------------------------- */
/* netG(lr=lr, z=None, u=None, eps_std=tau, reverse=True): HCFlowNet_SR.reverse_flow_diracLR
 * (HCFlowNet_SR_arch.py:70-75) and HCFlowNet_Rescaling.reverse_flow_diracLR
 * (HCFlowNet_Rescaling_arch.py:49-54) -> FlowNet.reverse_flow (FlowNet_SR_x4.py:106-123).
 *   lr      [B,3,h,w]  device
 *   eps     n_eps device pointers, sampling order (deepest level first), each [B,C_l,h_l,w_l] and
 *           ALREADY N(0,tau) distributed (what GaussianDiag.sample draws, Basic.py:98-99); an
 *           entry (or the whole array) may be NULL -> drawn on device (Philox, `seed`) * tau
 *   out_hr  [B,3,h*scale,w*scale] device */
int hcf_inverse(hcf_engine* e, const float* lr, const float* const* eps, int32_t n_eps, float tau, uint64_t seed,
                float* out_hr, int32_t B, int32_t h, int32_t w, uint32_t flags, hcf_stream_t stream);
/* The same for a SHARD of a larger batch (batch-sharded multi-GPU sampling): sample b of this call is sample
 * first_sample + b of the batch, and the device Philox draws are those of that global sample -- N shards with the same seed
 * draw exactly the eps of the one-GPU batch (the reference seeds every rank identically, train_HCFlow.py:43-46, which would give
 * every shard the same eps). The IMAGES are bit-identical when the shards take the same kernel schedule as the full batch
 * (always for equal per-sample sizes at the BASELINE shapes; a layer's Winograd / direct choice follows how many units a launch
 * has, so very small or very large shards agree to fp32 rounding instead). hcf_inverse = first_sample 0. */
int hcf_inverse_ex(hcf_engine* e, const float* lr, const float* const* eps, int32_t n_eps, float tau, uint64_t seed,
                   int64_t first_sample, float* out_hr, int32_t B, int32_t h, int32_t w, uint32_t flags, hcf_stream_t stream);

/* The same with ONE TEMPERATURE PER SAMPLE: the reference's validation loop draws every (heat, sample) pair of an image in a
 * call of its own (test_HCFlow.py:116-131, HCFlow_SR_model.py:296-316); here the rows of one call may each have their heat.
 *   taus_dev  [B] fp32 DEVICE memory, finite and >= 0 (the caller checks), read by the prior kernels when the pass runs: it
 *             must stay valid and unchanged until then. taus_dev[b] belongs to sample b of THIS call (not first_sample + b).
 * Row b holds the bits of hcf_inverse_ex(tau = taus[b]) with the same seed and global sample index first_sample + b (same
 * kernel schedule, see above). Levels with an injected eps ignore the vector, as they ignore tau. Enqueue-only like its
 * neighbours: no host copy, no synchronisation, no allocation in the steady state. */
int hcf_inverse_taus(hcf_engine* e, const float* lr, const float* const* eps, int32_t n_eps, const float* taus_dev, uint64_t seed,
                     int64_t first_sample, float* out_hr, int32_t B, int32_t h, int32_t w, uint32_t flags, hcf_stream_t stream);

/* Sampling that RETURNS THE DENSITY of what it drew (sample_and_log_prob): hcf_inverse_ex (taus_dev == NULL) or hcf_inverse_taus
 * (taus_dev != NULL, tau ignored) with one more output. SR engines only: a rescaling engine's forward pass tracks no log-det, so
 * the quantity has no reference there (HCF_ERR_UNSUPPORTED).
 *   out_logp [B] fp32 device. DEFINITION: out_logp[b] is the out_logp that hcf_encode_sr returns for hr = the UNCLAMPED image of
 *            this call with noise = NULL: log-det + the prior log-densities in nats, including -ln(quant) * H * W, WITHOUT the
 *            Dirac-LR term. It is the density under the model at temperature 1, whatever tau drew the sample (tau = 0 gives the
 *            density of the mean sample). Without HCF_FLAG_NO_CLAMP out_hr is clamped; the density is still that of the
 *            unclamped sample.
 * The pass evaluates every term already: each affine coupling's logscale on the z1 the forward pass would see, the prior's logs
 * and the eps it applies, and the host-side ActNorm / slogdet constants; per-block fp32 partial sums (no atomics) are reduced in
 * fp64 in a fixed order, so a row's bits depend neither on the call nor on the batch it sits in. out_hr, the flags and the other
 * arguments are those of the two entries above, and out_hr holds their bits. Enqueue-only: no synchronisation, and no allocation
 * in the steady state. */
int hcf_inverse_logp(hcf_engine* e, const float* lr, const float* const* eps, int32_t n_eps, float tau, const float* taus_dev,
                     uint64_t seed, int64_t first_sample, float* out_hr, float* out_logp, int32_t B, int32_t h, int32_t w,
                     uint32_t flags, hcf_stream_t stream);

/* netG(hr=hr, lr=lr, reverse=False) for HCFlowNet_SR: normal_flow_diracLR (HCFlowNet_SR_arch.py:47-67).
 *   hr [B,3,H,W], lr [B,3,H/scale,W/scale] (NULL -> no Dirac term), noise [B,3,H,W] U[0,1) or NULL
 *   (NULL -> no dequantisation noise is added)
 *   out_lr [B,3,H/scale,W/scale] = clamp(Quant(z)); out_nll [1]; out_logdet [B] objective per sample
 *   (nullable); out_z [B,3,H/scale,W/scale] pre-quantisation latent (nullable) */
int hcf_forward_sr(hcf_engine* e, const float* hr, const float* lr, const float* noise, float* out_lr, float* out_nll,
                   float* out_logdet, float* out_z, int32_t B, int32_t H, int32_t W, hcf_stream_t stream);

/* Encode for HCFlowNet_SR: the forward flow of normal_flow_diracLR (HCFlowNet_SR_arch.py:52-56 -> FlowNet.normal_flow,
 * FlowNet_SR_x4.py:84-101, FlowNet_SR_x8.py:91-116) that RETURNS what each conditional prior standardises instead of folding it
 * into the log-probability (ConditionalFlow.py:46-57, Basic.py:78-94): eps_l = (a_l - mean_l) * exp(-logs_l). Fed back through
 * hcf_inverse(lr = out_z, eps = out_eps, tau ignored, HCF_FLAG_NO_CLAMP) the flow returns hr + noise / quant.
 *   hr [B,3,H,W]; noise [B,3,H,W] U[0,1) or NULL (NULL -> no dequantisation noise is added: the decode target is hr itself)
 *   out_z    [B,3,H/scale,W/scale] pre-quantisation LR latent, not clamped
 *   out_eps  n_eps device buffers, deepest level first: the order and the shapes of hcf_inverse's eps; n_eps = number of levels
 *   out_logp [B] (nullable): logdet + sum of the prior log-densities in nats, WITHOUT the Dirac-LR term (HCFlowNet_SR_arch.py:63).
 *            The reference's constant -ln(quant) * H * W (:53) is part of it whether or not noise is given.
 *   flags    HCF_FLAG_NO_RANGE_CHECK or 0 */
int hcf_encode_sr(hcf_engine* e, const float* hr, const float* noise, float* out_z, float* const* out_eps, int32_t n_eps,
                  float* out_logp, int32_t B, int32_t H, int32_t W, uint32_t flags, hcf_stream_t stream);

/* netG(hr=hr, reverse=False) for HCFlowNet_Rescaling: normal_flow_diracLR
 * (HCFlowNet_Rescaling_arch.py:39-46): out_lr = clamp(LR^), out_z1 [B,6,H/2,W/2], out_z2 [B,21,H/4,W/4] */
int hcf_forward_rescale(hcf_engine* e, const float* hr, float* out_lr, float* out_z1, float* out_z2, int32_t B, int32_t H,
                        int32_t W, uint32_t flags, hcf_stream_t stream);

/* Convolution numerics. HCF_PRECISION_EXACT (default): fp32 MFMA, an exact fp32 fma chain.
 * HCF_PRECISION_F16X3: every fp32 product is formed from f16 hi/lo parts (a_hi b_hi + a_hi b_lo +
 * a_lo b_hi, error ~2^-22) on the 16x faster f16 matrix cores with fp32 accumulation; deviation
 * from fp64 on the full nets equals plain fp32's. An input beyond the f16 range (|x| >= 65504) cannot be
 * split: it raises a sticky device flag whose value every f16x3 inference pass copies to pinned host memory asynchronously.
 * hcf_check_range waits for the passes enqueued so far and reports (and clears) it: *overflowed = 1 means the outputs of the
 * f16x3 passes since the last check are invalid and must be recomputed with HCF_PRECISION_EXACT (hcflow_amd/arch.py does that
 * by default after every pass; `set_range_check("lazy")` defers it). hcf_fallback_count = number of raised checks. The taped
 * training passes (hcf_train_*) check and re-run by themselves (they synchronise anyway). */
int hcf_set_precision(hcf_engine* e, int32_t mode);
int hcf_get_precision(const hcf_engine* e);
int hcf_check_range(hcf_engine* e, int32_t* overflowed);
/* The same check with the affected SAMPLES: every op of the path is per-sample (HCFlowNet_SR_arch.py:70-75, thops.sum(dim=[1,2,3])),
 * so an out-of-range activation invalidates only the samples whose tiles saw it. *sample_slots: bit (b mod 30) is set for every
 * sample index b (within its call's batch) that was flagged since the last check -- a superset for B > 30 (slots alias); all 30
 * bits when a flagging kernel could not name its sample (device flag: bit 0 = overflow, bits 1..30 = sample slots, bit 31 =
 * "unattributed", latched on its own so that slots named by another kernel or pass cannot mask it). The caller re-runs only those samples with HCF_PRECISION_EXACT
 * (hcflow_amd/arch.py: one B = 1 pass per flagged sample through hcf_inverse_ex with its sample offset) instead of the whole
 * batch. Reports and clears like hcf_check_range (one fallback counted). */
int hcf_check_range_samples(hcf_engine* e, int32_t* overflowed, uint32_t* sample_slots);
int64_t hcf_fallback_count(const hcf_engine* e);

/* Side stream `slot` (0 / 1) of `device` (-1: the current one): the process holds at most two per device (low priority,
 * non-blocking, created on first use, never destroyed) and every engine uses them -- the training pass for its weight-gradient and
 * conditional-feature-gradient work, the module for the two half batches of a split inference call (hcflow_amd/arch.py:
 * set_streams(2)). Replaces nothing in the reference (it runs on one stream; codes/models/HCFlow_SR_model.py:184-205, 209-262);
 * exported so that the host side does not create further streams of its own: HIP spreads streams over four hardware queues. */
int hcf_aux_stream(int32_t device, int32_t slot, hcf_stream_t* out);

/* bytes of device workspace currently held (activations arena) and of packed weights */
size_t hcf_workspace_bytes(const hcf_engine* e);
size_t hcf_weight_bytes(const hcf_engine* e);

/* ---- NLL training step (reference: HCFlow_SR_model.optimize_parameters, HCFlow_SR_model.py:195-202:
 *      `_, nll = netG(hr, lr, reverse=False); nll.backward()`) -------------------------------------------------
 * hcf_train_forward_sr = hcf_forward_sr (same outputs; hr / lr / noise are required) that additionally keeps every
 * intermediate tensor in HBM and records the backward pass. hcf_train_backward then writes
 *   d(grad_nll * nll) / d(parameter)   for EVERY parameter, concatenated in hcf_param_info order (= state_dict
 * order, each tensor flattened), into `dparams` (device buffer of `numel` = total parameter count floats); the
 * caller slices it into its .grad tensors. One backward per forward; `lr` must stay alive in between. The convs follow
 * hcf_set_precision (f16x3: forward, data-gradient and weight-gradient convs on the split kernels, the latter only for
 * layers whose taped forward was range-checked; exact: fp32 MFMA). Every per-channel and split-K sum is reduced in a fixed
 * order: the gradients are bit-reproducible run to run (no floating-point atomics). SR nets only. */
int hcf_train_forward_sr(hcf_engine* e, const float* hr, const float* lr, const float* noise, float* out_lr,
                         float* out_nll, float* out_logdet, int32_t B, int32_t H, int32_t W, hcf_stream_t stream);
int hcf_train_backward(hcf_engine* e, float grad_nll, float* dparams, int64_t numel, hcf_stream_t stream);
/* The same backward pass in two calls, for a caller whose gradient all-reduce overlaps the backward pass (the reference trains under
 * DistributedDataParallel, HCFlow_SR_model.py:33-36, whose buckets are reduced as their gradients arrive). phase 0 runs the part
 * of the pass that was taped last -- the output terms and the level-0 conditional flow -- and completes every parameter-gradient
 * reduction it enqueued on `stream`: when it returns (stream order), the slices of `dparams` of all parameters whose key starts with
 * "flow.level0_condFlow." (about half of an SR x4 net) are FINAL and nothing later touches them. phase 1 (same `dparams`) runs the
 * rest. The two calls together write exactly what hcf_train_backward writes, bit for bit. Calls on the other tape slot
 * (hcf_train_select_tape) may run between the phases. */
int hcf_train_backward_phase(hcf_engine* e, int32_t phase, float grad_nll, float* dparams, int64_t numel, hcf_stream_t stream);

/* Gradients through the REVERSE (sampling) path (reference: the HR pixel / feature / GAN losses of the HCFlow+ / ++
 * recipes, HCFlow_SR_model.py:207-255: `fake_H = netG(lr=, eps_std=, reverse=True)` followed by a loss on fake_H and
 * backward()). hcf_train_inverse = hcf_inverse (same arguments and output) with a tape; hcf_train_backward_inverse
 * takes dL/d(out_hr) (device [B,3,H,W], the clamp's gradient mask is applied inside) and writes dL/d(parameter) for
 * every parameter like hcf_train_backward. */
int hcf_train_inverse(hcf_engine* e, const float* lr, const float* const* eps, int32_t n_eps, float tau, uint64_t seed,
                      float* out_hr, int32_t B, int32_t h, int32_t w, uint32_t flags, hcf_stream_t stream);
int hcf_train_backward_inverse(hcf_engine* e, const float* grad_out, float* dparams, int64_t numel, float* grad_lr,
                               hcf_stream_t stream);     /* grad_lr: optional device [B,3,h,w], receives dL/d lr */
/* The same with the gradients of the latents (optimising in the latent space with the weights frozen: editing, projection onto
 * a constraint, refining a sample against a metric). grad_eps: n_eps device tensors in sampling order, deepest level first and
 * shaped as hcf_inverse's eps (the array and each entry nullable): grad_eps[i] receives dL/d eps_i of a = mean + e^logs eps
 * (GaussianDiag.sample, Basic.py:96-101; logs = s for the SR prior, 0.318 atan(2 s) for the rescaling prior,
 * ConditionalFlow.py:59-69,86-96). A level whose eps the taped pass drew on the device has a gradient too: w.r.t. the drawn
 * N(0, tau) values. hcf_train_backward_inverse = this call with grad_eps = NULL, n_eps = 0.
 * dparams = NULL with numel = 0 asks for the gradients of the inputs alone: the pass launches no weight-gradient kernel, no
 * per-channel sum and no log-det update, touches no parameter-gradient slot and does not fork the weight-gradient stream; the
 * data-gradient chain (direct and Winograd convs, fused epilogue backward) is the one of the full pass. The forward passes'
 * backward entries take the same form (hcf_train_backward_ex below); the two-phase backward refuses a null dparams. */
int hcf_train_backward_inverse_ex(hcf_engine* e, const float* grad_out, float* dparams, int64_t numel, float* grad_lr,
                                  float* const* grad_eps, int32_t n_eps, hcf_stream_t stream);
/* The forward passes differentiated w.r.t. their IMAGES (the flow as a density over images: MAP restoration with the NLL as image
 * prior, likelihood-guided refinement of a sample, training a network that feeds the rescaler or the encoder).
 * hcf_train_backward_ex = hcf_train_backward that also returns d(grad_nll * nll) / d hr (grad_hr, device [B,3,H,W], nullable) and
 * / d lr (grad_lr, device [B,3,H/scale,W/scale], nullable) of normal_flow_diracLR (HCFlowNet_SR_arch.py:47-67): hr + noise / quant
 * (:52) has an identity Jacobian w.r.t. hr and squeeze2d's transpose is unsqueeze2d; lr enters through the Dirac term
 * logp(lr; mean = Quant(z), logs = -6) (:58-63) alone, d / d lr = (Quant(z) - lr) e^12 per element. d / d noise is not returned.
 * hcf_train_backward_rescale_ex = hcf_train_backward_rescale with grad_hr (device [B,3,H,W], nullable): the input end is the
 * Haar transform's transpose, (Haar fwd)^T = Haar inv / 4 (Basic.py:450-487).
 * Both: dparams = NULL with numel = 0 gives the image gradients alone, as hcf_train_backward_inverse_ex does for the latents (no
 * weight-gradient kernel, no per-channel sum, no log-det update, no fork of the weight-gradient stream; the data-gradient
 * launches of the full pass); hcf_train_backward_counts then reads 0/0/0/0. hcf_train_backward = hcf_train_backward_ex without
 * the image gradients, likewise hcf_train_backward_rescale. */
int hcf_train_backward_ex(hcf_engine* e, float grad_nll, float* dparams, int64_t numel, float* grad_hr, float* grad_lr,
                          hcf_stream_t stream);
int hcf_train_backward_rescale_ex(hcf_engine* e, const float* g_lr, const float* g_z1, const float* g_z2, float* dparams,
                                  int64_t numel, float* grad_hr, hcf_stream_t stream);
/* hcf_encode_sr with a tape (same arguments, same outputs: out_z, out_eps deepest level first, out_logp [B], here required;
 * flags are accepted and ignored: a taped pass checks its own range and re-runs on the exact kernels), and its backward:
 * seeds g_z = dL/d out_z, g_eps[i] = dL/d out_eps[i] (the array and each entry nullable; n_eps entries) and g_logp = dL/d out_logp
 * as a device vector [B] (nullable) -> grad_hr = dL/d hr (device [B,3,H,W]). Each conditional prior contributes through both of
 * its outputs, eps = (a - mean) e^-logs and its log-density (ConditionalFlow.py:46-57). The pass is input-gradient-only by
 * definition: dparams must be NULL and numel 0; anything else is refused with HCF_ERR_UNSUPPORTED (the full backward under a
 * per-sample seed on the log-det terms is hcf_train_backward_encode_ex below). d / d noise is not returned. */
int hcf_train_encode_sr(hcf_engine* e, const float* hr, const float* noise, float* out_z, float* const* out_eps, int32_t n_eps,
                        float* out_logp, int32_t B, int32_t H, int32_t W, uint32_t flags, hcf_stream_t stream);
int hcf_train_backward_encode(hcf_engine* e, const float* g_z, const float* const* g_eps, int32_t n_eps, const float* g_logp,
                              float* dparams, int64_t numel, float* grad_hr, hcf_stream_t stream);
/* The backward of hcf_train_encode_sr that also takes a gradient buffer (training the net on any objective over the encode's
 * outputs: a per-sample weighted NLL, a latent regulariser, distillation on eps): the same seeds -> dparams = dL/d parameters
 * (flat, state_dict order, fully defined on return as after hcf_train_backward_ex) and grad_hr (nullable: a plain hr under
 * trainable weights). With dparams the pass is the full backward: the weight-gradient launches, the per-channel sums and the
 * data-independent log-det updates (logs += k, dW += k W^-T, log_s += k) of the NLL backward. Where that pass has the host scalar
 * k = grad_obj * B * H * W, the seed here is per sample: k = H * W * S with S = sum_b g_logp[b] summed once on the device (one
 * block, fixed order, float64; hcf_op_seed_sum) into a float the tape slot owns, which the one batched log-det launch reads.
 * g_logp = NULL: the log-density has no gradient, no log-det update is queued (hcf_train_backward_counts: out[3] = 0 while
 * out[0..2] > 0). dparams = NULL with numel = 0 is hcf_train_backward_encode's input-gradient-only pass (counters 0/0/0/0), bit for
 * bit; grad_hr is the same bits with and without dparams. The two-phase backward does not take an encode tape. */
int hcf_train_backward_encode_ex(hcf_engine* e, const float* g_z, const float* const* g_eps, int32_t n_eps, const float* g_logp,
                                 float* dparams, int64_t numel, float* grad_hr, hcf_stream_t stream);
/* Parameter-gradient work of the LAST backward pass on the selected tape slot (hcf_train_select_tape): out[0] = weight-gradient
 * launches of one conv, out[1] = convs handed to the batched weight-gradient launches of the dense blocks, out[2] = per-channel
 * sum jobs, out[3] = axpy (log-det) jobs. All zero after an input-gradient-only pass. */
int hcf_train_backward_counts(const hcf_engine* e, int64_t out[4]);

/* Rescaling net (reference: one generator step of HCFlow_Rescaling_model.optimize_parameters, :212-256 --
 * `fake_LR, z1, z2 = netG(hr, reverse=False)`; losses on all three; `fake_H = netG(lr=Quant(fake_LR), reverse=True)`;
 * loss on fake_H; ONE backward through both passes). hcf_train_forward_rescale = hcf_forward_rescale with a tape;
 * hcf_train_backward_rescale takes dL/d(out_lr), dL/d z1, dL/d z2 (device, each nullable; the clamp mask of out_lr is
 * applied inside). Both passes of the step must keep their tapes alive at once: hcf_train_select_tape picks the slot
 * (0 or 1) that the following taped passes / backward calls use. With hcf_train_backward_inverse's grad_lr the
 * gradient flows from the inverse pass into the forward pass (through the caller's straight-through Quant). */
int hcf_train_select_tape(hcf_engine* e, int32_t slot);
int hcf_train_forward_rescale(hcf_engine* e, const float* hr, float* out_lr, float* out_z1, float* out_z2, int32_t B,
                              int32_t H, int32_t W, uint32_t flags, hcf_stream_t stream);
int hcf_train_backward_rescale(hcf_engine* e, const float* g_lr, const float* g_z1, const float* g_z2, float* dparams,
                               int64_t numel, hcf_stream_t stream);

/* In-place parameter updates on the GPU (optimiser steps; reference: base_model / HCFlow_SR_model keep netG's
 * parameters on the device and Adam updates them in place, HCFlow_SR_model.py:108-125,202). After hcf_finalize,
 * hcf_bind_param_device tells the engine where each parameter lives in DEVICE memory (fp32, contiguous, same shape
 * as hcf_param_info reports; the pointer must stay valid); hcf_refresh_from_device then rewrites every weight pack
 * and table from those tensors with device kernels (host work only for the invertible 1x1 convs' fp64 inverse and
 * log-determinant: one small D2H + H2D round trip) -- milliseconds instead of the host repack of hcf_finalize. */
int hcf_bind_param_device(hcf_engine* e, const char* key, const float* dev_ptr);
int hcf_refresh_from_device(hcf_engine* e, hcf_stream_t stream);

/* ActNorm data-dependent initialisation (reference: _ActNorm.initialize_parameters, ActNorms.py:29-43, reached from
 * _ActNorm.forward when `not self.inited` in train() mode, :78-80). hcf_actnorm_init_request() arms the NEXT
 * hcf_forward_sr / hcf_forward_rescale call: each listed ActNorm (state_dict prefix, e.g.
 * "flow.layers.1.actnorm" or "flow.layers.1.affine.f.conv1.actnorm") whose stored bias is all zero gets
 * bias = -mean, logs = log(1 / (sqrt(var) + 1e-6)) of the tensor that reaches it, per channel over (B, H, W), in
 * forward order, and the pass continues with the fitted values (the pass runs on the exact fp32 kernels and
 * synchronises the stream once per fitted layer). Afterwards hcf_get_param() returns the fitted tensors (HOST
 * buffer of `numel` floats; works for any parameter key) so that the caller can store them in its own module. */
int hcf_actnorm_init_request(hcf_engine* e, const char* const* prefixes, int32_t n);
int hcf_get_param(hcf_engine* e, const char* key, float* host_out, int64_t numel);

/* timing hook used by bench.py: when enabled, every conv launch is bracketed by HIP events on the
 * launch stream. hcf_conv_time_ms() sums the recorded launches of one kernel variant
 * (taps in {9,1} = 3x3 / 1x1, nt = N tiles of 32 output channels; 0 = any; kind = 0 plain conv, 1 with the fused
 * 1x1 second layer, 2 with the fused flow-step tail, 3 reading an upsampled source, 4 the Winograd form of the f16x3
 * conv, 5 the persistent small-K FCN conv1 + conv2 kernel (hcf_conv_fcn.hip), 6 the Winograd form of a conditional FCN
 * conv1 with the 1x1 conv2 in its epilogue, 7 the 32 -> 32 completion of a fat dense-block launch (adds a stored partial), -1 any): total time, launch count,
 * algorithmic FLOPs (2 * taps * cin * cout per output pixel) and algorithmic HBM bytes (each source window,
 * residual and the weights read once, the output written once). reset != 0 clears the records. */
int hcf_profile_convs(hcf_engine* e, int enable);
int hcf_conv_time_ms(hcf_engine* e, int32_t taps, int32_t nt, int32_t kind, int32_t reset, double* total_ms,
                     int64_t* launches, double* flops, double* bytes);

/* ---- the optimiser step of the training caller (reference: HCFlow_SR_model.py:118-120 / HCFlow_Rescaling_model.py:140-142
 * build torch.optim.Adam(optim_params, lr, weight_decay, betas) over netG's ~1500 parameter tensors and step it once per
 * iteration, optimize_parameters :202) as ONE launch. param / exp_avg / exp_avg_sq: device fp32 buffers of one layout (every
 * parameter tensor in a slot at a multiple-of-4 offset; 16-byte aligned bases). chunks_dev: DEVICE table, one entry per
 * <= HCF_ADAM_CHUNK consecutive elements of a tensor: its gradient slice (device fp32, any alignment), the slot offset
 * (floats, multiple of 4) and the length. Arithmetic of torch.optim.Adam with amsgrad = False, maximize = False, L2 weight
 * decay: g += wd p; m += (g - m)(1 - beta1); v = v beta2 + (1 - beta2) g g; p -= lr / (1 - beta1^step) * m /
 * (sqrt(v) / sqrt(1 - beta2^step) + eps); step >= 1 is the count AFTER this update. Enqueues on `stream`, no sync. */
#define HCF_ADAM_CHUNK 4096
typedef struct hcf_adam_chunk {
  const float* grad;
  uint32_t offset;
  uint32_t n;
} hcf_adam_chunk;
int hcf_adam_step(float* param, float* exp_avg, float* exp_avg_sq, const hcf_adam_chunk* chunks_dev, int32_t n_chunks,
                  double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step, hcf_stream_t stream);

/* ---- validation metrics around the path (reference: the per-image metric block of test_HCFlow.py:103-182) ------
 * hcf_metric_psnr_ssim: util.tensor2img (utils/util.py:790-816) on gt and sr, then util.calculate_psnr_ssim(gt, sr,
 * crop_border) (:898-982; Y channel as data/util.py:209-230) and, for scale > 1, the same on
 * imresize(gt, 1/scale), imresize(sr, 1/scale) with crop 0 (utils/imresize.py, MATLAB bicubic with antialiasing).
 * gt, sr: device [B,3,H,W] RGB fp32; out: HOST double [B][8] = psnr, ssim, psnr_y, ssim_y, then the four
 * down-scaled ("bicHR") values (0 when scale <= 1). float64 arithmetic. hcf_metric_imresize_down (scale >= 2) returns the
 * down-scaled tensor2img image itself (HOST double [B][3 (B,G,R)][ceil(H/scale)][ceil(W/scale)], 0..255 units).
 * Both are one-shot wrappers over hcf_metric_pair_* below: they allocate their device buffers, run embed (+ compare), copy
 * the result to the host, synchronise `stream` and free. So the eight numbers are bit for bit those of embed + compare: two
 * calls agree exactly and an image's numbers do not depend on the rest of the batch; the planes of imresize_down are the
 * ones embed keeps (rows first, not re-quantised). Checked before anything touches a device: null pointers, B, H, W < 1,
 * negative crop_border or scale, a shape the pair entries refuse (B > 21845, scale > 1024, ...) -> HCF_ERR_ARG;
 * H - 2 crop_border < 1 or W - 2 crop_border < 1 -> HCF_ERR_SHAPE. */
int hcf_metric_psnr_ssim(const float* gt, const float* sr, int32_t B, int32_t H, int32_t W, int32_t crop_border,
                         int32_t scale, double* out, hcf_stream_t stream);
int hcf_metric_imresize_down(const float* x, int32_t B, int32_t H, int32_t W, int32_t scale, double* out,
                             hcf_stream_t stream);

/* Streaming per-pixel statistics of a SET of samples: what the reference gets from torch.cat(sr_img_list).std([0]) with every
 * sample of an image held at once (test_HCFlow.py:127-131, :165-167), here with a state that does not grow with the number of
 * samples: one (mean, M2) pair of doubles per element, updated by Welford's recurrence (hcf_metrics.hip).
 *   hcf_metric_stats_bytes   size of the caller-allocated device state for [B,3,H,W] samples (16 bytes per element plus one
 *                            double per 1024 elements for the finishing pass); 0 for an invalid shape. Needs no clearing.
 *   hcf_metric_stats_add     folds one sample batch x (device [B,3,H,W] fp32) into the state. n = the number of samples the
 *                            state holds AFTER this call (a host count, by value): n = 1 starts a new set. One launch.
 *   hcf_metric_stats_finish  from a state of n >= 1 samples: mean [B,3,H,W] fp32, std [B,3,H,W] fp32 (unbiased, n - 1, in the
 *                            samples' units; 0 for n = 1) and diversity [B] DEVICE double = mean over (c, y, x) of 255 * std,
 *                            summed in float64 in a fixed order (no atomics: two runs agree bit for bit, and an image's values
 *                            do not depend on the rest of the batch). The state is left as it was: adding may go on.
 * All three only enqueue on `stream`: no synchronisation, no allocation. */
size_t hcf_metric_stats_bytes(int32_t B, int32_t H, int32_t W);
int hcf_metric_stats_add(void* state, size_t state_bytes, const float* x, int32_t B, int32_t H, int32_t W, int64_t n,
                         hcf_stream_t stream);
int hcf_metric_stats_finish(void* state, size_t state_bytes, int32_t B, int32_t H, int32_t W, int64_t n, float* mean, float* std,
                            double* diversity, hcf_stream_t stream);

/* PSNR / SSIM of many samples against ONE prepared GT: the eight numbers of hcf_metric_psnr_ssim (util.tensor2img,
 * utils/util.py:790-816; util.calculate_psnr_ssim, :898-982; utils/imresize.py) with the GT-side work done once per GT and
 * nothing allocated, copied from the host or synchronised per sample (hcf_pair_metrics.hip: the one implementation).
 *   hcf_metric_pair_ref_bytes  size of the caller-allocated device buffer that holds a prepared GT batch [B,3,H,W] (private
 *                              layout: the tensor2img planes as uint8; for scale > 1 the bicubic down-scaled planes as fp64 and the
 *                              tables of imresize.py's contributions()); 0 for an invalid shape (utils/util.py:790-816,
 *                              utils/imresize.py).
 *   hcf_metric_pair_workspace  size of the caller-allocated device scratch of one compare call; 0 for an invalid shape. Image
 *                              b's part starts at b * (the size for B = 1) (utils/util.py:898-982, utils/imresize.py).
 *   hcf_metric_pair_embed      prepares gt (device [B,3,H,W] RGB fp32) into ref. The one entry that copies host tables (kept alive
 *                              by the library) to the device, stream-ordered; it allocates nothing (utils/util.py:790-816,
 *                              utils/imresize.py).
 *   hcf_metric_pair_compare    sr (device [B,3,H,W] RGB fp32) against ref -> out, DEVICE double [B][8] = psnr, ssim, psnr_y,
 *                              ssim_y, then the four down-scaled values: inf where the mse is 0, nan where a side of the compared
 *                              window is under 11 pixels, columns 4..7 = 0 for scale <= 1. image_out: NULL or device uint8
 *                              [B][H][W][3] BGR = util.tensor2img(sr) of every image. SSIM by the separable 11 + 11 tap form of
 *                              the reference's Gaussian window, float64; every sum is joined in a fixed order (no atomics: two
 *                              runs agree bit for bit, an image's numbers do not depend on the rest of the batch). Only enqueues
 *                              on `stream` (utils/util.py:790-816, 898-982, utils/imresize.py).
 * compare takes the crop_border / scale that embed was given. Checked before anything touches a device: null pointers, B, H, W < 1,
 * negative crop_border or scale -> HCF_ERR_ARG; short buffers, H - 2 crop_border < 1 or W - 2 crop_border < 1 -> HCF_ERR_SHAPE. */
size_t hcf_metric_pair_ref_bytes(int32_t B, int32_t H, int32_t W, int32_t scale);
size_t hcf_metric_pair_workspace(int32_t B, int32_t H, int32_t W, int32_t scale);
int hcf_metric_pair_embed(const float* gt, int32_t B, int32_t H, int32_t W, int32_t crop_border, int32_t scale, void* ref,
                          size_t ref_bytes, hcf_stream_t stream);
int hcf_metric_pair_compare(const void* ref, size_t ref_bytes, const float* sr, int32_t B, int32_t H, int32_t W, int32_t crop_border,
                            int32_t scale, double* out, uint8_t* image_out, void* work, size_t work_bytes, hcf_stream_t stream);

/* The 8-bit image boundary of a rescaling net used as a codec (hcf_image_codec.hip): HR -> LR^ -> stored 8-bit image -> HR^.
 *   hcf_metric_quantize    x (device [B,3,H,W] RGB fp32) -> q (NULL or device [B,3,H,W] fp32) = rint(clamp(x, 0, 1) * 255.f) / 255.f,
 *                          the forward value of the reference's Quantization (Basic.Quant.forward, models/modules/Basic.py:186-202,
 *                          applied by HCFLowRescalingModel.test(), HCFlow_Rescaling_model.py:306-324): round half to even, an IEEE
 *                          fp32 division. NaN stays NaN and -0.0 gives -0.0 (== 0), both as through torch.clamp on the host; +-inf are clamped. image_out
 *                          (NULL or device uint8 [B][H][W][3] BGR): the same integers = util.tensor2img(x) of every image
 *                          (utils/util.py:790-816), i.e. what hcf_metric_pair_compare's image_out holds for x (a NaN is byte 0
 *                          there and here). One launch writes both; either may be NULL, not both.
 *   hcf_metric_from_image  image (device uint8 [B][H][W][3] BGR) -> out (device [B,3,H,W] RGB fp32) = float(u) / 255.f with the same
 *                          division: what the reference's datasets make of a stored image (data/util.py:72-79 read_img: astype(np.float32) / 255.;
 *                          data/GT_dataset.py:107-111: BGR -> RGB, then HWC -> CHW). A stored image
 *                          is a fixed point: quantize(from_image(u)) gives from_image(u) and u back, bit for bit.
 * One thread owns the same pixels of all three planes; 16-byte accesses where H * W is a multiple of 4 and the addresses are
 * aligned, else one pixel per thread (a batch slice of an odd-sized tensor is legal). Both only enqueue one kernel on `stream`: no
 * allocation, copy, synchronisation or atomic. Checked before anything touches a device: null x / image / out, q and image_out
 * both NULL, B, H, W < 1, B > 65535 or H * W > 2^36 -> HCF_ERR_ARG. */
int hcf_metric_quantize(const float* x, int32_t B, int32_t H, int32_t W, float* q, uint8_t* image_out, hcf_stream_t stream);
int hcf_metric_from_image(const uint8_t* image, int32_t B, int32_t H, int32_t W, float* out, hcf_stream_t stream);

/* ---- per-op entry points (unit parity tests; tensors are device NCHW fp32) ------------------- */
/* F.conv2d(x, w, stride 1, padding k/2) with the fused epilogue
 *   y = res2 + rs2 * (res1 + rs1 * act((conv + bias) * scale))
 * w is a HOST pointer in PyTorch layout [cout, cin, k, k]; bias/scale HOST [cout] or NULL;
 * x is the channel-concatenation of n_src device tensors [B, src_c[i], H >> src_up[i], W >> src_up[i]]
 * (nearest-upsampled by 2^src_up[i]); res1/res2 device [B,cout,H,W] or NULL. k in {1,3}. */
int hcf_op_conv2d(const float* const* src, const int32_t* src_c, const int32_t* src_up, int32_t n_src, int32_t B,
                  int32_t H, int32_t W, const float* w, const float* bias, const float* scale, int32_t cout, int32_t k,
                  int32_t act, const float* res1, float rs1, const float* res2, float rs2, float* out,
                  hcf_stream_t stream);

/* Backward of hcf_op_conv2d without epilogue (torch.autograd of F.conv2d(cat(up(src_i)), w, bias, 1, k/2); the
 * reference reaches it through loss.backward() in HCFlow_SR_model.optimize_parameters, HCFlow_SR_model.py:195-202):
 * g = dL/dy, device [B,cout,H,W]. dsrc[i] (device [B, src_c[i], H >> up, W >> up]) may be NULL; dw is a HOST buffer
 * [cout, cin, k, k], dbias a HOST buffer [cout]; either may be NULL. Data gradients run on the forward conv
 * kernels with transposed / flipped weights (process-wide op precision). The weight gradient runs on
 * hcf_conv_wgrad.hip: fp32 MFMA in exact mode, the f16x3 matrix-core kernel (g scaled by a power of two from
 * max |g|, both operands split) in f16x3 mode; split-K partial tiles are added in a fixed order (deterministic). */
int hcf_op_conv2d_backward(const float* const* src, const int32_t* src_c, const int32_t* src_up, int32_t n_src,
                           int32_t B, int32_t H, int32_t W, const float* w, int32_t cout, int32_t k, const float* g,
                           float* const* dsrc, float* dw, float* dbias, hcf_stream_t stream);

/* Basic.squeeze2d / unsqueeze2d factor 2 (Basic.py:127-157) and HaarDownsampling (Basic.py:470-487) */
int hcf_op_squeeze2d(const float* x, float* out, int32_t B, int32_t C, int32_t H, int32_t W, int32_t haar, hcf_stream_t stream);
int hcf_op_unsqueeze2d(const float* x, float* out, int32_t B, int32_t C4, int32_t H, int32_t W, int32_t haar, hcf_stream_t stream);
/* FlowStep.reverse_flow tail / normal_flow head+coupling on given tensors (FlowStep.py:40-64):
 *   inverse: out = actnorm^-1( Winv @ coupling^-1(z, h) );  forward: zmid = W @ actnorm(z) then
 *   out = coupling(zmid, h), logdet[b] = sum logscale.  mat: HOST [C,C] (W for forward; the entry
 *   inverts it in fp64 for inverse) or NULL; bias/logs HOST [C]; mode/ns as hcf_common.h StepArgs. */
int hcf_op_step_inverse(const float* z, const float* h, float* out, int32_t B, int32_t C, int32_t H, int32_t W,
                        int32_t hC, int32_t mode, int32_t ns, const float* mat, const float* an_bias,
                        const float* an_logs, hcf_stream_t stream);
int hcf_op_step_forward_head(const float* z, float* out, int32_t B, int32_t C, int32_t H, int32_t W, const float* mat,
                             const float* an_bias, const float* an_logs, hcf_stream_t stream);
int hcf_op_step_forward_couple(const float* z, const float* h, float* out, float* logdet, int32_t B, int32_t C,
                               int32_t H, int32_t W, int32_t hC, int32_t mode, int32_t ns, hcf_stream_t stream);
/* The fused f16x3 conv launches of the default inference path, ONE launch per call (tests/test_gpu_fused_convs.py). Both entries
 * always run the f16x3 kernels (never the Winograd form, which the engine excludes for these launches), build their packs with the
 * engine's host packer, return a launcher's refusal as their status without substituting anything, and return HCF_ERR_UNSUPPORTED
 * without writing their outputs when the launch raised the f16 range flag.
 *   info[16] (HOST, filled from the launch made): 0 launcher (0 the persistent fcn12 kernel, 1 the f16x3 kernel), 1 the plan's /
 *   launcher's status, 2 .. 10 the f16x3 kernel's template arguments NTB, VEC, UP, FUSE2, TAILC, TH, SCALED, K1, N16 (launcher 1),
 *   11 grid, 12 block, 13 tiles walked and 14 the `pre` instantiation (launcher 0), 15 the range flag word.
 *
 * FCN layers 1 + 2 (Basic.py:441-444):
 *   out = relu(((W2 . relu(((conv3x3(cat(up(src_i)), w1) + pre) + bias1) * scale1)) + bias2) * scale2)
 * sources as hcf_op_conv2d; w1 HOST [64,cin,3,3], w2 HOST [64,64,1,1], bias / scale HOST [64] or NULL; pre device [B,64,H,W] or NULL
 * (it travels as res1, as in the engine); out device [B,64,H,W]. form 0: what the engine's run_conv does -- the persistent form
 * first, the direct FUSE2 form when that returns HCF_ERR_UNSUPPORTED; form 1: the direct FUSE2 form (which refuses `pre`:
 * HCF_ERR_ARG). */
int hcf_op_fcn12(const float* const* src, const int32_t* src_c, const int32_t* src_up, int32_t n_src, int32_t B, int32_t H,
                 int32_t W, const float* w1, const float* bias1, const float* scale1, const float* w2, const float* bias2,
                 const float* scale2, const float* pre, float* out, int32_t form, int32_t* info, hcf_stream_t stream);
/* Conv2dZeros with the inverse flow step in its epilogue (FlowStep.py:53-64): h = (conv3x3(h2, w3) + bias3) * scale3, then
 * out_z = actnorm^-1(Winv @ coupling^-1(z, h)) as hcf_op_step_inverse (same tables, same fp64 inverse of mat). h2 device
 * [B,hid,H,W]; w3 HOST [f_out,hid,3,3]; bias3 / scale3 HOST [f_out] or NULL; z, out_z device [B,C,H,W]; out_zpad device
 * [B,16,H,W] or NULL: out_z[:, :zpad_n] zero-padded to 16 channels, as the kernel stores it for the next step. */
int hcf_op_conv2d_step_inverse(const float* h2, int32_t hid, const float* w3, const float* bias3, const float* scale3,
                               int32_t f_out, const float* z, int32_t C, int32_t mode, int32_t ns, const float* mat,
                               const float* an_bias, const float* an_logs, float* out_z, float* out_zpad, int32_t zpad_n,
                               int32_t B, int32_t H, int32_t W, int32_t* info, hcf_stream_t stream);
/* The conv kernels on the CALLER's memory (tests/test_gpu_view_convs.py): every activation is a channel window of an NHWC buffer
 * the caller owns, described as the engine's View is (hcf_common.h) and used AS IS -- the entries allocate nothing for
 * activations, copy nothing and zero-fill nothing; only packs, flags, partial-sum scratch and the input maximum are theirs.
 * Test path: the engine never calls them. */
typedef struct hcf_view {
  float* p;              /* device: base of the NHWC buffer [B][H >> up][W >> up][cs] */
  int32_t cs, c0, n;     /* floats per pixel, first channel and channels of the window: 0 <= c0, 1 <= n, c0 + n <= cs */
  int32_t up;            /* log2 nearest-upsample factor of a conv source (0 .. 8, must divide H and W); 0 for every other view */
} hcf_view;
/* hcf_op_conv2d's arithmetic, out = res2 + rs2 * (res1 + rs1 * act((conv(cat(up(src_i)), w) + bias) * scale)), with src (n_src
 * = 1 .. 3 descriptors), res1 / res2 (NULL: none) and out (n = cout <= 96) as views; w HOST [cout,cin,k,k], bias / scale HOST
 * [cout] or NULL. Routing as hcf_op_conv2d for the process-wide op precision (f16x3: Winograd where eligible and not ablated, else
 * the f16x3 kernel, > 64 output channels exact), plus: k = 1 takes the f16x3 kernel's K1 rows where its plan accepts the call and
 * the exact kernel where it answers HCF_ERR_UNSUPPORTED (as the engine does); scaled != 0 (f16x3 only) is the training
 * data-gradient form: the entry takes max |x| over the source windows (launch_absmax) and passes it as ConvArgs::in_max.
 *   info[16] (HOST): 0 launcher (0 exact, 1 f16x3, 2 Winograd 32 channels, 3 Winograd 64), 1 the plan's / launcher's status,
 *   2 .. 10 the f16x3 kernel's template arguments NTB, VEC, UP, FUSE2, TAILC, TH, SCALED, K1, N16 (launcher 1) or 2 VEC, 3 vec_epi,
 *   4 NT of conv_mfma_kernel (launcher 0), 11 grid, 12 block, 13 vec_epi, 14 strip_w, 15 the range flag word.
 * HCF_ERR_UNSUPPORTED with info[15] != 0: an input left the f16 range (the out window then holds what the launch wrote). */
int hcf_op_conv2d_views(const hcf_view* src, int32_t n_src, int32_t B, int32_t H, int32_t W, const float* w, const float* bias,
                        const float* scale, int32_t k, int32_t act, const hcf_view* res1, float rs1, const hcf_view* res2,
                        float rs2, const hcf_view* out, int32_t scaled, int32_t* info, hcf_stream_t stream);
/* ONE launch of the training path's fused data-gradient form (ConvArgs::fb_y; tests/test_gpu_fused_dgrad.py): the conv's output is
 * the complete dL/dy of the conv that produced `y`, and the launch applies that producer's epilogue backward in its own epilogue.
 *   d = conv(cat(src_i), w), dz = d * act'(y) (fb_act: 0 none, 1 relu: y > 0, 2 leaky relu 0.2: y >= 0), out = dL/dpre = dz * fb_scale
 *   sum_pre[c] += sum out, sum_zy[c] += zy_mult * sum dz * y (want_zy), *fb_max = max(*fb_max, max |out|),
 *   *fb_max2 = max(*fb_max2, max |out|, max |src windows|); a launch whose out is all zero touches neither maximum.
 * ConvArgs as launch_dgrad (hcf_engine_train.inc) fills them: unit bias and scale, no activation, no residuals, plain store, in_max =
 * max |x| over the source windows in a slot of the entry's own, NaN-filled partial rows reduced by one sum job over exactly the rows
 * the launch left. src: 1 .. 3 views (up = 0); w HOST [n, cin, k, k], k = 3 or 1; y and out: views of n <= 64 channels; fb_scale HOST
 * [n] or NULL; sum_pre [n], sum_zy [n] (may be NULL without want_zy; given without it, it receives the zeros of the second partial
 * row), fb_max, fb_max2 (NULL: not kept): the caller's DEVICE memory, the maxima in / out. Launch order as the engine's: the fused 32-channel Winograd kernel (k = 3, not ablated with bit 256; a pack from 16
 * input channels on), where it refuses the fused SCALED rows of the f16x3 kernel. No fused form accepts the call, or the op
 * precision is exact: HCF_ERR_UNSUPPORTED -- never an unfused launch.
 *   info[18] (HOST): 0 .. 15 as hcf_op_conv2d_views (launcher 1 or 2), 16 rows of partial sums reduced, 17 Winograd: units walked. */
int hcf_op_conv2d_dgrad_fused_views(const hcf_view* src, int32_t n_src, int32_t B, int32_t H, int32_t W, const float* w, int32_t k,
                                    const hcf_view* y, int32_t fb_act, const float* fb_scale, int32_t want_zy, float zy_mult,
                                    const hcf_view* out, float* sum_pre, float* sum_zy, float* fb_max, float* fb_max2, int32_t* info,
                                    hcf_stream_t stream);
/* dw HOST [g.n, cin, k, k] = the weight gradient of that conv given g = dL/d(conv output) as a view (taps = 9 or 1). f16x3 op
 * precision: the matrix-core kernel with max |g| taken over the window, the fp32 kernel when max |x| over the source windows is
 * not below 65504 (as hcf_op_conv2d_backward).
 *   info[16] (HOST), plan_conv_wgrad's: 0 status, 1 f16x3 kernel, 2 TAPS, 3 VEC, 4 DB, 5 strip_w, 6 tpb, 7 nblk_x. */
int hcf_op_conv2d_wgrad_views(const hcf_view* src, int32_t n_src, int32_t B, int32_t H, int32_t W, const hcf_view* g, int32_t taps,
                              float* dw, int32_t* info, hcf_stream_t stream);
/* hcf_op_conv_epilogue_backward on views, each with its own cs / c0 and all of n channels: gy in, gpre out (gpre may BE gy: the
 * engine runs it in place), y (NULL as there), g1 / g2 (NULL: not wanted) accumulated. scale HOST [n] or NULL; the sums, maxima and
 * carry2 as there. info[4] (HOST): 0 the vector kernel ran, 1 blocks. */
int hcf_op_conv_epilogue_backward_views(const hcf_view* gy, const hcf_view* y, const float* scale, int32_t act, int32_t has1,
                                        float rs1, const hcf_view* g1, int32_t has2, float rs2, const hcf_view* g2,
                                        const hcf_view* gpre, float* sum_pre, float* sum_zy, float zy_mult, float* absmax,
                                        float* absmax2, const float* carry2, int32_t B, int32_t H, int32_t W, int32_t* info,
                                        hcf_stream_t stream);
/* GaussianDiag.logp / sample (Basic.py:78-101) with (mean, logs) = h[:,0::2], h[:,1::2] */
int hcf_op_gauss_logp(const float* h, const float* x, float* out_logp, int32_t B, int32_t C, int32_t H, int32_t W,
                      hcf_stream_t stream);
int hcf_op_gauss_sample(const float* h, const float* eps, float tau, uint64_t seed, float* out, int32_t B, int32_t C,
                        int32_t H, int32_t W, int32_t rescale, hcf_stream_t stream);

/* Backward kernels of the training path (hcf_train.hip), one entry per launcher, on the tensors the engine would have taped.
 * Tensors are device NCHW fp32 unless noted; per-channel tables are HOST pointers as above. Per-channel sums take the engine's
 * route: per-block partial rows, then one fixed-order reduction (launch_sum_jobs), ADDED to the caller's device arrays.
 *
 * One forward flow step  za = (zin + b) e^s,  zb = W za,  zout = coupling(zb, h):  coupling backward, then head backward.
 * In: gzout = dL/dzout, zout, h [B,hC,H,W], za; mat = W (HOST [C,C] or NULL), an_logs = s; gobj = dL/d(objective_b) (the
 * sum of the coupling's log-scales). Out: gzin, gh; g_bias[C] += dL/db, g_logs[C] += dL/ds (device). */
int hcf_op_step_forward_backward(const float* gzout, const float* zout, const float* h, const float* za, float* gzin,
                                 float* gh, float* g_bias, float* g_logs, int32_t B, int32_t C, int32_t H, int32_t W,
                                 int32_t hC, int32_t mode, int32_t ns, const float* mat, const float* an_logs, float gobj,
                                 hcf_stream_t stream);
/* One inverse flow step  zc = coupling^-1(z, h),  y = W^-1 zc,  x = y e^-s - b.  In: gx = dL/dx, x, zc, h; mat = W (inverted
 * in fp64 by the entry, as hcf_op_step_inverse does). Out: gz, gh, gzc = dL/dzc, y; g_bias[C] +=, g_logs[C] += (device). */
int hcf_op_step_inverse_backward(const float* gx, const float* x, const float* zc, const float* h, float* gz, float* gh,
                                 float* gzc, float* y, float* g_bias, float* g_logs, int32_t B, int32_t C, int32_t H,
                                 int32_t W, int32_t hC, int32_t mode, int32_t ns, const float* mat, const float* an_bias,
                                 const float* an_logs, hcf_stream_t stream);
/* Gaussian prior backward with (mean, s) = h[:,0::2], h[:,1::2]; rescale: logs = 0.318 atan(2 s), else logs = s.
 *   kind 0 (logp):   objective += logp(a; mean, s)              -> ga, gh out (scaled by gobj)
 *   kind 1 (sample): a = mean + e^logs eps, ga = dL/da IN       -> gh out
 *   kind 2 (encode): z = (a - mean) e^-logs, gz_nchw = dL/dz (NULL: zero) -> ga, gh out */
int hcf_op_prior_backward(int32_t kind, const float* a, const float* h, float* ga, float* gh, const float* gz_nchw,
                          int32_t B, int32_t C, int32_t H, int32_t W, int32_t rescale, float gobj, hcf_stream_t stream);
/* kind 1 of the above that also returns the gradient of the latent (GaussianDiag.sample, Basic.py:96-101, as the conditional
 * priors call it, ConditionalFlow.py:59-69 SR, :86-96 rescaling): a = mean + e^logs eps, ga = dL/da IN -> gh out (the same
 * values as kind 1, bit for bit) and geps_nchw [B,C,H,W] = dL/d eps = ga e^logs out (NULL: not wanted, the call is kind 1). */
int hcf_op_prior_sample_backward(const float* a, const float* h, const float* ga, float* gh, float* geps_nchw, int32_t B,
                                 int32_t C, int32_t H, int32_t W, int32_t rescale, hcf_stream_t stream);
/* Dirac-LR term with the straight-through Quant: gz [B,3,H,W] += gobj * d logp(lr; mean = Quant(z), logs = -6) / dz */
int hcf_op_quant_logp_backward(const float* z, const float* lr, float* gz, int32_t B, int32_t H, int32_t W, float gobj,
                               hcf_stream_t stream);
/* The same that also returns d / d lr: glr [B,3,H,W] = gobj * (Quant(z) - lr) * e^12 (NULL: not wanted; gz is then bit-identical to
 * hcf_op_quant_logp_backward's). lr is the value the Dirac density is evaluated at (HCFlowNet_SR_arch.py:58-63). */
int hcf_op_quant_logp_backward_lr(const float* z, const float* lr, float* gz, float* glr, int32_t B, int32_t H, int32_t W,
                                  float gobj, hcf_stream_t stream);
/* Prior backward of the SR encode, where eps = (a - mean) e^-logs leaves the pass and logp(a; mean, logs) joins its log-density
 * (ConditionalFlow.py:46-57, Basic.py:78-94): seeds geps_nchw = dL/d eps (NULL: zero) and dL/d logp_b = glogp[b] (device [B]; NULL:
 * the scalar gobj for every sample) -> ga, gh out = kind 2 + kind 0 of hcf_op_prior_backward, each term in that kernel's own
 * arithmetic: with only one seed the other kind's output comes out bit for bit. */
int hcf_op_prior_encode_logp_backward(const float* a, const float* h, float* ga, float* gh, const float* geps_nchw,
                                      const float* glogp, int32_t B, int32_t C, int32_t H, int32_t W, int32_t rescale, float gobj,
                                      hcf_stream_t stream);
/* Input end of the taped forward passes: gz [B,4C,H,W] = dL/d z of z = squeeze2d(hr) (haar 0) or Haar(hr) (haar 1) ->
 * ghr [B,C,2H,2W] = dL/d hr: unsqueeze2d(gz) (Basic.py:143-157), or Haar inv(gz) / 4 (Basic.py:450-487); exact. */
int hcf_op_input_grad(const float* gz, float* ghr, int32_t B, int32_t C, int32_t H, int32_t W, int32_t haar,
                      hcf_stream_t stream);
/* Gradients of an NCHW (clamped) output: kind 0: gz += g;  1: gz += g where 0 <= z <= 1;  2: gz = 0 where z is outside
 * [0, 1] (g unused, may be NULL);  3: gz = (0 <= z <= 1) ? g : 0 on the flat tensors. */
int hcf_op_output_grad_backward(int32_t kind, const float* g, const float* z, float* gz, int32_t B, int32_t C, int32_t H,
                                int32_t W, hcf_stream_t stream);
/* Backward of the fused conv epilogue  y = res2 + rs2 * (res1 + rs1 * act((acc + bias) * scale))  given gy = dL/dy:
 * gpre = dL/dacc out; g1 / g2 (NULL: not wanted) += the residuals' gradients when has1 / has2; sum_pre[n] += sum gpre,
 * sum_zy[n] += zy_mult * sum dz y (device, NULL: not wanted); absmax / absmax2 (device floats, raised) and carry2 as
 * hcf_common.h EpiBwdArgs. scale: HOST [n] or NULL; y may be NULL when act is none and sum_zy is NULL. Every tensor is
 * placed at channels [c0, c0 + n) of an NHWC buffer of cs >= c0 + n floats per pixel, as the engine's windows are. */
int hcf_op_conv_epilogue_backward(const float* gy, const float* y, const float* scale, int32_t act, int32_t has1, float rs1,
                                  float* g1, int32_t has2, float rs2, float* g2, float* gpre, float* sum_pre, float* sum_zy,
                                  float zy_mult, float* absmax, float* absmax2, const float* carry2, int32_t B, int32_t n,
                                  int32_t H, int32_t W, int32_t cs, int32_t c0, hcf_stream_t stream);
/* LU-decomposed invertible 1x1 conv, W = P L U': dl, du [C,C] and dlog_s [C] += the chain rule of dW = dL/dW
 * (hcf_common.h LuChainArgs). All device, row-major, C <= 48. */
int hcf_op_lu_chain(const float* dW, const float* P, const float* L, const float* U, float* dl, float* du, float* dlog_s,
                    int32_t C, hcf_stream_t stream);
/* out[0] = sum_b g[b] over a device vector [B]: one block, a fixed order that depends on B alone, float64 accumulation, one fp32
 * store, no atomics -- the sum of a per-sample seed on logp that the log-det jobs of hcf_train_backward_encode_ex read. */
int hcf_op_seed_sum(const float* g, int32_t B, float* out, hcf_stream_t stream);
/* One data-independent log-det update as the training backward queues them: y[i] += k * (x ? x[i] : 1), i < n, with
 * k = alpha (k_dev NULL: the host form of the NLL and rescaling passes) or alpha * *k_dev (k_dev: one device float). x nullable. */
int hcf_op_axpy_job(const float* x, float* y, int32_t n, float alpha, const float* k_dev, hcf_stream_t stream);

/* ---- auxiliary nets of the HCFlow+ / ++ recipes (reference: Discriminator_VGG_160 / VGGFeatureExtractor,
 *      codes/models/modules/discriminator_vgg_arch.py:68-157; used by HCFlow_SR_model.py:75-95,219-285) ------------------
 * Stride-1 "same" convolution (k = 3 or 1) and its gradients on DEVICE tensors with the flow's own conv / weight-gradient
 * kernels: x, y, g, dx are dense NHWC fp32 [B][H][W][cs] (cs % 4 == 0, 16-byte aligned), w is the PyTorch-layout weight
 * [cout][cin][k][k] in device memory (packs are rebuilt on the device per call), bias [cout] or NULL.
 *   hcf_aux_conv2d:          y[..., 0:cout] = act(conv(x[..., 0:cin], w) + bias), act 0 none / 1 relu / 2 leaky relu 0.2
 *   hcf_aux_conv2d_backward: dx[..., 0:cin] = dL/dx (nullable), dw = dL/dw given g = dL/d(conv output)
 * `work`: device scratch of hcf_aux_conv2d_workspace(...) bytes; with HCF_PRECISION_F16X3 (3x3 forward only) the int at
 * work[0] is raised when an input leaves the f16 range (the caller zeroes it before a network pass and reads it after).
 * The discriminator's 4x4 stride-2 convs run as squeeze2d + 3x3 conv with a re-indexed weight (hcflow_amd/gan.py). */
size_t hcf_aux_conv2d_workspace(int32_t cin, int32_t cout, int32_t k, int32_t B, int32_t H, int32_t W);
int hcf_aux_conv2d(const float* x, int32_t cs_in, int32_t cin, int32_t B, int32_t H, int32_t W, const float* w,
                   const float* bias, int32_t cout, int32_t k, int32_t act, float* y, int32_t cs_out, void* work,
                   size_t work_bytes, int32_t precision, hcf_stream_t stream);
int hcf_aux_conv2d_backward(const float* x, int32_t cs_in, int32_t cin, int32_t B, int32_t H, int32_t W, const float* w,
                            int32_t cout, int32_t k, const float* g, int32_t cs_g, float* dx, int32_t cs_dx, float* dw,
                            void* work, size_t work_bytes, int32_t precision, hcf_stream_t stream);

/* BatchNorm2d(C, affine=True) + LeakyReLU(0.2) of Discriminator_VGG_128 / PatchGANDiscriminator
 * (discriminator_vgg_arch.py:12-33,42-55,171-183), with an output window: reads the window (y0, x0, Ho, Wo) of an H x W input
 * and writes a compact Ho x Wo output. A padding-0 3x3 conv is the interior (1, 1, H-2, W-2) of hcf_aux_conv2d's same-padded
 * output, so these entries plus the aux conv give the PatchGAN layers without a conv kernel of their own.
 *   x:     device NHWC [B][H][W][cs_x];  y: device NHWC [B][Ho][Wo][cs_y], channels >= C written 0 (cs % 4 == 0, 16-byte aligned)
 *   mode:  0 window (+ activation) only; 1 train(): batch statistics (biased variance), running_mean / running_var (nullable as
 *          a pair) moved in place with the unbiased variance and `momentum`; 2 eval(): running statistics
 *   act:   0 none, 1 relu, 2 leaky relu 0.2
 *   save_mean / save_invstd: device [C], written by the forward pass (modes 1, 2), read by the backward pass
 * Statistics are reduced through fp64 per-block partials in a fixed order (bit-reproducible, no float atomics); no host sync.
 * hcf_aux_bn_act_backward writes dx over the FULL H x W input, zero outside the window (the exact gradient of the same-padded
 * conv's output); dgamma / dbeta (device [C], overwritten) are nullable: a frozen net's pass (netD in the G step,
 * HCFlow_SR_model.py:237-243) skips them. `work`: device scratch of hcf_aux_bn_act_workspace(C, B, Ho, Wo) bytes, used by the
 * train() forward and by a backward pass with mode 1 or parameter gradients. */
size_t hcf_aux_bn_act_workspace(int32_t C, int32_t B, int32_t Ho, int32_t Wo);
int hcf_aux_bn_act(const float* x, int32_t cs_x, int32_t C, int32_t B, int32_t H, int32_t W, int32_t y0, int32_t x0, int32_t Ho,
                   int32_t Wo, const float* gamma, const float* beta, float* running_mean, float* running_var, int32_t mode,
                   double momentum, double eps, int32_t act, float* y, int32_t cs_y, float* save_mean, float* save_invstd,
                   void* work, size_t work_bytes, hcf_stream_t stream);
int hcf_aux_bn_act_backward(const float* x, int32_t cs_x, int32_t C, int32_t B, int32_t H, int32_t W, int32_t y0, int32_t x0,
                            int32_t Ho, int32_t Wo, const float* gamma, const float* beta, const float* save_mean,
                            const float* save_invstd, int32_t mode, int32_t act, const float* dy, int32_t cs_dy, float* dx,
                            int32_t cs_dx, float* dgamma, float* dbeta, void* work, size_t work_bytes, hcf_stream_t stream);

/* ---- VGG19 perceptual loss of the HCFlow++ generator step: the memory-bound ops BETWEEN the aux convs of
 * l_g_fea = l_fea_w * cri_fea(netF(fake_H), netF(real_H).detach())  (HCFlow_SR_model.py:229-232, HCFlow_Rescaling_model.py:237-240;
 * netF = VGGFeatureExtractor(feature_layer=34, use_bn=False), networks.py:60-68). hcflow_amd/gan.py: PerceptualLoss chains them
 * with hcf_aux_conv2d / hcf_aux_conv2d_backward; none of these entries launches a convolution. Activations are dense NHWC fp32
 * (cs % 4 == 0, 16-byte aligned), act is 0 none / 1 relu / 2 leaky relu 0.2; no host synchronisation, no atomics.
 *
 * hcf_aux_input_norm: `x = (x - self.mean) / self.std` (discriminator_vgg_arch.py:153-154) and the layout change in one pass:
 *   x device NCHW [B][3][H][W] -> y device NHWC [B][H][W][4], y[..., c] = (x[c] - mean[c]) / stdev[c], y[..., 3] = 0.
 *   mean, stdev: device [3] (the module's buffers, :139-145); both NULL: the layout change only (use_input_norm=False).
 * hcf_aux_input_norm_backward: g NHWC [B][H][W][4] -> dx NCHW [B][3][H][W], dx[c] = g[..., c] / stdev[c] (stdev NULL: the copy). */
int hcf_aux_input_norm(const float* x, const float* mean, const float* stdev, int32_t B, int32_t H, int32_t W, float* y,
                       hcf_stream_t stream);
int hcf_aux_input_norm_backward(const float* g, const float* stdev, int32_t B, int32_t H, int32_t W, float* dx,
                                hcf_stream_t stream);
/* hcf_aux_maxpool2: nn.MaxPool2d(kernel_size=2, stride=2) of torchvision's VGG19 `features` (discriminator_vgg_arch.py:137,146),
 * floor mode: x [B][H][W][cs_x] -> y [B][H/2][W/2][cs_y]; an odd last row / column is not read; channels >= C of y written 0.
 * A NaN wins its window, as in PyTorch.
 * hcf_aux_maxpool2_act_backward: the pool's and the preceding activation's backward in one pass. gp [B][H/2][W/2][cs_gp] is
 * the gradient of the pooled tensor, y [B][H][W][cs_y] the pool's input = the conv's output AFTER its fused activation;
 * gpre [B][H][W][cs_g] = gradient w.r.t. the conv's pre-activation: in each 2x2 window gp goes to the FIRST maximum in row-major
 * order (PyTorch's rule: a strict > while scanning), kept only where y > 0 when act is relu (act 0 or 1 only); every other
 * element, an odd last row / column and channels >= C are written 0. */
int hcf_aux_maxpool2(const float* x, int32_t cs_x, int32_t C, int32_t B, int32_t H, int32_t W, float* y, int32_t cs_y,
                     hcf_stream_t stream);
int hcf_aux_maxpool2_act_backward(const float* gp, int32_t cs_gp, const float* y, int32_t cs_y, int32_t C, int32_t B, int32_t H,
                                  int32_t W, int32_t act, float* gpre, int32_t cs_g, hcf_stream_t stream);
/* hcf_aux_act_backward: gpre = g * act'(y) over n floats (n % 4 == 0), y the activation's OUTPUT: relu g * (y > 0), leaky relu
 * g * (y > 0 ? 1 : 0.2), none the copy -- the expressions of hcflow_amd/gan.py _ConvNHWC.backward (nn.ReLU(inplace=True) of the
 * VGG19 stack). gpre may alias g. */
int hcf_aux_act_backward(const float* g, const float* y, int32_t act, int64_t n, float* gpre, hcf_stream_t stream);
/* hcf_aux_feature_loss: cri_fea = nn.L1Loss() (kind 0) / nn.MSELoss() (kind 1) with the default mean reduction
 * (HCFlow_SR_model.py:62-66): loss[0] = mean over n floats of |a - b| or (a - b)^2 (device float), and, when grad is not NULL,
 * grad[i] = dloss/da[i] = sign(a - b) / n (0 where equal) or 2 (a - b) / n. a, b, grad: device [n], 16-byte aligned, any n >= 1.
 * The sum runs in fp64 through per-block partials of a grid fixed by n and one fixed-order final block: bit-reproducible.
 * work: device scratch of hcf_aux_feature_loss_workspace(n) bytes. */
size_t hcf_aux_feature_loss_workspace(int64_t n);
int hcf_aux_feature_loss(const float* a, const float* b, int64_t n, int32_t kind, float* loss, float* grad, void* work,
                         size_t work_bytes, hcf_stream_t stream);

/* ---- LPIPS v0.1, AlexNet (the LPIPS column of the reference's test log: test_HCFlow.py:48 builds lpips.LPIPS(net='alex'),
 * :132 evaluates it on (2 gt - 1, 2 sr - 1)); hcflow_amd/lpips.py is the module around it. One call runs the whole network on
 * both inputs and the LPIPS head, in exact fp32 (fp32 MFMA), on `stream`, without host synchronisation; the result for an image
 * depends on that image pair only and is bit-reproducible.
 *   in0, in1: device [B,3,H,W] fp32 NCHW, in [-1, 1] (normalize != 0: in [0, 1], mapped by 2x - 1); H, W >= 31
 *   params:   HOST array of HCF_LPIPS_NPARAMS device pointers, PyTorch layouts: shift[3], scale[3], conv1 weight re-indexed
 *             to the 5x5 conv on the 4x4 space-to-depth grid [64][48][5][5] (hcflow_amd/lpips.py: alex_conv1_as_s2d), conv1
 *             bias[64], conv2 w[192][64][5][5] / b, conv3 w[384][192][3][3] / b, conv4 w[256][384][3][3] / b,
 *             conv5 w[256][256][3][3] / b, then the five linear heads lin0..lin4 ([C_l] each)
 *   out:      device [B] = LPIPS per image pair;  out_layers: device [B][5] per-layer terms, or NULL
 *   work:     device scratch of hcf_lpips_workspace(B, H, W) bytes (0: shape below AlexNet's minimum) */
#define HCF_LPIPS_NPARAMS 17
size_t hcf_lpips_workspace(int32_t B, int32_t H, int32_t W);
int hcf_lpips_alex(const float* in0, const float* in1, int32_t B, int32_t H, int32_t W, int32_t normalize,
                   const float* const* params, float* out, float* out_layers, void* work, size_t work_bytes,
                   hcf_stream_t stream);

/* ---- LPIPS as a loss: the image gradients of the measure above (test_HCFlow.py:48,132), for use where a feature loss enters
 * the generator step (HCFlow_SR_model.py:229-232); hcflow_amd/lpips.py: LPIPSLoss. No parameter gradients.
 * GUARANTEE: a successful hcf_lpips_alex call leaves in `work` the space-to-depth input and the feature maps of every layer of
 * both inputs, and they stay valid for as long as the caller keeps that buffer unchanged. The layout is private: the backward
 * entry reads it through the plan the forward wrote it with, so pass the SAME (B, H, W, normalize, params) and the same buffer.
 *   gout:      device [B], dL/d out[b]
 *   which:     bit 0: in0 wants a gradient, bit 1: in1 (1, 2 or 3); the backward convolutions cover those halves only
 *   gin0/gin1: device [B,3,H,W] fp32 NCHW, overwritten for the bits set (the other may be NULL)
 *   fwd_work:  the work buffer of the forward call (fwd_work_bytes >= the forward's workspace size), read only
 *   work:      device scratch of the backward's own workspace size for (B, H, W, which); 0: bad shape or `which`
 * Exact fp32, on `stream`, no host synchronisation, no atomics: bit-reproducible, and sample b's gradient depends on that image
 * pair and gout[b] only. Where a pixel's feature vector is all zero the gradient through its norm is defined as 0 (autograd of
 * f / (sqrt(sum f^2) + 1e-10) yields NaN there). Max-pool ties go to the first maximum in row-major order, as in PyTorch. */
size_t hcf_lpips_backward_workspace(int32_t B, int32_t H, int32_t W, int32_t which);
int hcf_lpips_alex_backward(int32_t B, int32_t H, int32_t W, int32_t normalize, const float* const* params,
                            const float* gout, int32_t which, float* gin0, float* gin1, const void* fwd_work,
                            size_t fwd_work_bytes, void* work, size_t work_bytes, hcf_stream_t stream);

/* ---- LPIPS against a stored reference, with the per-pixel map (hcflow_amd/lpips.py: LPIPSMap): the measure above for sample
 * sets, where one GT meets many samples. hcf_lpips_alex_embed runs the AlexNet part over ONE input of B images (not a stacked
 * 2B) and leaves its five feature maps in `store` (hcf_lpips_embed_bytes(B, H, W) bytes; 0: bad shape; the layout is private
 * and stays valid while the caller leaves the buffer alone). hcf_lpips_alex_map embeds x the same way into `work` and runs the
 * head against the stored reference of the SAME (B, H, W, normalize, params):
 *   out [B], out_layers [B][5]: as hcf_lpips_alex(ref, x): bit-equal to it (one per-pixel function, the same partial sums)
 *   out_map [B][H][W]:   D = sum over the layers l = 0..4, in that order, of the bilinear upsampling (align_corners = False,
 *                        PyTorch's F.interpolate / lpips' upsample()) of the layer's per-pixel value
 *                        d_l = sum_c w_lc (f0_c / (sqrt n0 + 1e-10) - f1_c / (sqrt n1 + 1e-10))^2 to H x W: the value of
 *                        lpips.LPIPS(spatial=True). Source row of output row y on an h-row grid: sy = max(0, (y + .5) h / H - .5),
 *                        i0 = floor(sy), i1 = min(i0 + 1, h - 1), weight sy - i0; columns alike
 *   out_map_mean [B]:    the mean of D over the image (NOT `out`: the upsampling moves the mean by about 1e-4 relative)
 *   best_map [B][H][W]:  read and written: best = first != 0 ? D : fminf(best, D), the per-pixel best over the calls so far
 *   out_best_mean [B]:   the mean of the updated best_map (needs best_map)
 * Every output may be NULL; with neither out_map, out_map_mean nor best_map no map kernel is launched. The means are fp64 sums
 * of per-block partials over a grid fixed by (H, W), added in a fixed order. out_map / best_map take 16-byte accesses when
 * W % 4 == 0 and they are 16-byte aligned, scalar ones otherwise (the same arithmetic). work: hcf_lpips_map_workspace(B, H, W)
 * bytes. On `stream`, no host synchronisation, no atomics: bit-reproducible, and image b's results depend on image b only. */
size_t hcf_lpips_embed_bytes(int32_t B, int32_t H, int32_t W);
int hcf_lpips_alex_embed(const float* x, int32_t B, int32_t H, int32_t W, int32_t normalize, const float* const* params,
                         void* store, size_t store_bytes, hcf_stream_t stream);
size_t hcf_lpips_map_workspace(int32_t B, int32_t H, int32_t W);
int hcf_lpips_alex_map(const void* ref_store, size_t ref_bytes, const float* x, int32_t B, int32_t H, int32_t W,
                       int32_t normalize, const float* const* params, float* out, float* out_layers, float* out_map,
                       float* out_map_mean, float* best_map, float* out_best_mean, int32_t first, void* work, size_t work_bytes,
                       hcf_stream_t stream);

/* Range-headroom probe of the f16x3 path (tools/range_headroom.py): while enabled, every conv launch of the following passes
 * also records max |x| over its input windows and -- for layers that own a Winograd pack -- max |B^T d B| over the F(2x2,3x3)
 * input patches, i.e. the values the split has to represent (f16 limit 65504). hcf_debug_range_probe_read returns record
 * `index` (launch order): key = state-dict key of the conv's weight, maxima[2] = {max |x|, max |V| (0 if not Winograd)},
 * info[6] = {cin, cout, H, W, ran on f16x3, has a Winograd pack}; HCF_ERR_KEY past the last record. Debug / evidence only. */
int hcf_debug_range_probe(hcf_engine* e, int32_t enable);
int hcf_debug_range_probe_read(hcf_engine* e, int32_t index, char* key, int32_t key_cap, float* maxima, int32_t* info);

/* Shader clock INSIDE the dominant kernel: while enabled, block 0 of every launch of the 64-channel Winograd kernel adds its life
 * in shader cycles (s_memtime) and in 100 MHz ticks (s_memrealtime) to two device counters (scalar registers only, one block);
 * hcf_debug_last_clock_mhz() synchronises and returns 100 * cycles / ticks since the enable (0 before any launch; without the
 * probe: the clock of the last hcf_bench_conv call of a TIMERS build). bench.py reads it inside its single-stream timed region
 * (roofline.clock): the board runs this workload at its power cap, the held clock is part of the roofline fraction. */
int hcf_debug_clock_probe(int32_t enable);
double hcf_debug_last_clock_mhz(void);
/* tools/conv_bench.py --ablate: timing-only ablations of the f16x3 kernel (results invalid); 0 = off */
int hcf_debug_set_ablation(int32_t bits);
/* What the conv launchers would select for a call, WITHOUT a GPU (tests/test_conv_plan_cpu.py): plan_conv_f16x3 / plan_conv_wgrad on
 * shapes and window strides given as integers; an "aligned" flag stands for a view's 16-byte addressability.
 *   in[HCF_PLAN_N_IN]:  0 kind (0 f16x3 conv, 1 weight gradient), 1 taps, 2 B, 3 H, 4 W, 5 nsrc, 6 + 5 i .. : source i = {n, cs, c0, up,
 *     aligned}, 21 .. 24 out (kind 1: g) = {n, cs, c0, aligned}, 25 .. 27 res1 = {0 none / 1 aligned / 2 unaligned, cs, c0}, 28 .. 30 res2
 *     likewise, 31 tC (kind 1: blocks_hint), 32 bit0 w2, bit1 bias2, bit2 scale2, 33 in_max (kind 1: g_max) given, 34 act,
 *     35 .. 37 fb_y = {0 none / 1 aligned / 2 unaligned, cs, c0}, 38 bit0 fb_part, bit1 fb_scale, bit2 fb_scale unaligned, bit3 fb_max2 is
 *     in_max, 39 bit0 out.p null, bit1 ovf null
 *   out[HCF_PLAN_N_OUT], kind 0: 0 status, 1 .. 9 the kernel's template arguments NTB, VEC, UP, FUSE2, TAILC, TH, SCALED, K1, N16,
 *     10 grid, 11 block, 12 any_up, 13 vec_epi, 14 strip_w, 15 strip_magic (zeros when refused), 16 rows of per-block partial sums
 *     the engine plans for a scaled launch on [B, H, W], 17 their bound over tile heights
 *   kind 1: 0 status, 1 f16x3 kernel, 2 TAPS, 3 VEC, 4 DB (LDS form), 5 nblk_x, 6 nicb, 7 nocb, 8 block, 9 dynamic LDS bytes, 10 tpb,
 *     11 cin_total, 12 strip_w, 13 strip_magic, 14 scratch floats, 15 blocks per channel-block pair of the reduce (the plan as it
 *     is, also when refused: workspaces are sized from it before the arguments are complete) */
#define HCF_PLAN_N_IN 40
#define HCF_PLAN_N_OUT 18
int hcf_debug_conv_plan(const int32_t* in, int32_t n_in, int64_t* out, int32_t n_out);
/* Which kernel families a conv call would try, in order, WITHOUT a GPU (tests/test_conv_route_cpu.py): the order every conv launch
 * of the library goes through (engine, per-op entries, auxiliary nets). taps 1 / 9; packs: the weight packs the caller has, bit0 exact,
 * bit1 f16x3, bit2 Winograd, bit3 a fused second layer's f16x3 pack, bit4 its Winograd fragment; tail != 0: a flow-step tail is fused;
 * allow: the forms the caller admits, bit (1 << form). forms[4] receives the forms -- 0 Winograd, 1 fcn12, 2 f16x3, 3 exact, -1 beyond
 * the last -- the launch stops at the first that does not answer HCF_ERR_UNSUPPORTED. Honours hcf_debug_set_ablation (256: no
 * Winograd). Returns the number of forms, or HCF_ERR_ARG. */
int hcf_debug_conv_route(int32_t taps, int32_t packs, int32_t tail, int32_t allow, int32_t* forms, int32_t n_forms);
/* precision used by the per-op entry points hcf_op_conv2d / hcf_bench_conv (process-wide test knob) */
int hcf_op_set_precision(int32_t mode);
/* tools/conv_bench.py: times `iters` back-to-back launches of the conv kernel on random NHWC slabs */
int hcf_bench_conv(int32_t B, int32_t H, int32_t W, const int32_t* src_c, int32_t n_src, int32_t cout, int32_t k,
                   int32_t iters, double* ms_per_launch, double* flops_per_launch, hcf_stream_t stream);

/* ---- device-side training batches (hcf_data.hip): crop + flip + transpose + bicubic LR of a batch in one launch ----
 * The reference's GT_dataset.__getitem__ (train phase) on images that already live in device memory as packed HWC uint8:
 *   gt[b] = crop of uint8 / 255.f (true division) at (top_lr * scale, left_lr * scale), size (lr_h * scale) x (lr_w * scale);
 *   lq[b] = the window (top_lr, left_lr, lr_h, lr_w) of imresize_np(WHOLE image, 1 / scale) (data/util.py:407-474: antialiased
 *           cubic, H pass then W pass on the H result, symmetric padding of the whole image), computed for the window only;
 *   both then augment's hflip ([:, ::-1]), vflip ([::-1]), rot90 (transpose) in that order, BGR -> RGB when `bgr`, HWC -> CHW.
 * Outputs are float32 NCHW in device memory: gt [B,3,lr_h*scale,lr_w*scale], lq [B,3,lr_h,lr_w] (a rot90 sample is the
 * transpose, accepted for square crops only); either may be NULL (not wanted), not both.
 *   bank:   device, bank_bytes bytes; image i = 3 * H * W bytes at its byte offset
 *   images: HOST [n_images][3] = {byte offset, H, W}
 *   crops:  HOST [B][6] = {image, top_lr, left_lr, hflip, vflip, rot90}
 * scale is an integer in 2 .. 8. For an integer factor the normalised cubic weights are one vector of 4 * scale + 2 taps for
 * every output pixel: tap k of output o reads source index o * scale + k + c0, c0 = scale - 1 + floor(0.5 - 2.5 * scale),
 * reflected once at each border (i < 0: -i - 1, i >= n: 2n - 1 - i). The weights are computed on the host in double and rounded
 * to float; they and the per-sample records travel as kernel arguments: no allocation, no copy, no synchronisation, and up to
 * HCF_DATA_LAUNCH_BATCH samples per launch (larger batches: several launches of the same kernel).
 * Every record is validated BEFORE any HIP call: HCF_ERR_ARG for null pointers, scale outside 2 .. 8, an image index, offset or crop
 * outside its table / bank / image, flags other than 0 / 1, rot90 on a non-square crop; HCF_ERR_SHAPE for an image smaller than
 * 4 * scale in either dimension (one reflection would not reach). The kernel clamps every source index into its image besides. */
#define HCF_DATA_LAUNCH_BATCH 64
int hcf_data_prepare_batch(const uint8_t* bank, size_t bank_bytes, const int64_t* images, int32_t n_images,
                           const int32_t* crops, int32_t B, int32_t lr_h, int32_t lr_w, int32_t scale, int32_t bgr,
                           float* gt, float* lq, hcf_stream_t stream);

/* ---- paired image banks (hcf_data.hip): the LRHR_PKL and GTLQ / GTLQnpy / GTLQx samples of a batch in one launch ----
 * The reference's paired datasets (LRHR_PKL_dataset.py:96-135, GTLQnpy_dataset.py:42-78, GTLQx_dataset.py:82-122) on pairs that
 * already live in device memory as two packed HWC uint8 banks. The LQ image is data, never computed from the HR image:
 *   lq[b] = the window (top_lr, left_lr, lr_h, lr_w) of LQ image i, uint8 / 255.f (true division);
 *   gt[b] = the window (top_lr * scale, left_lr * scale, lr_h * scale, lr_w * scale) of HR image i, uint8 / 255.f;
 *   both then hflip ([:, ::-1]), vflip ([::-1]), rot90 (transpose) in that order, the channel reversal when `bgr`, HWC -> CHW.
 * np.rot90(k, axes=(1, 2)) after np.flip(axis=2) of the PKL mode is a flag triple of this map (hcflow_amd/data.py: PKL_FLAGS).
 * Outputs are float32 NCHW in device memory: gt [B,3,lr_h*scale,lr_w*scale], lq [B,3,lr_h,lr_w] (a rot90 sample is the
 * transpose, accepted for square crops only); either may be NULL (not wanted), not both.
 *   gt_bank, lq_bank:     device, gt_bytes / lq_bytes bytes; image i = 3 * H * W bytes at its byte offset
 *   gt_images, lq_images: HOST [n_images][3] = {byte offset, H, W}, row i of both = pair i
 *   crops:                HOST [B][6] = {image, top_lr, left_lr, hflip, vflip, rot90}, on the LQ grid
 * scale is an integer in 2 .. 8 and a runtime argument of the one kernel (there are no taps). The per-sample records travel as
 * kernel arguments: no allocation, no copy, no synchronisation, up to HCF_DATA_LAUNCH_BATCH samples per launch (larger batches:
 * several launches of the same kernel).
 * Every record is validated BEFORE any HIP call: HCF_ERR_ARG for null pointers, scale outside 2 .. 8, n_images < 1, an offset or
 * image outside its bank, an image index or crop outside its (LQ) image, flags other than 0 / 1, rot90 on a non-square crop;
 * HCF_ERR_SHAPE for a pair with H_gt < scale * H_lq or W_gt < scale * W_lq. A larger HR image is legal (the reference's
 * mod-crop, GTLQx_dataset.py:118-120): its extra rows and columns are never read. The kernel clamps every source index into its
 * image besides. */
int hcf_data_prepare_paired(const uint8_t* gt_bank, size_t gt_bytes, const int64_t* gt_images,
                            const uint8_t* lq_bank, size_t lq_bytes, const int64_t* lq_images, int32_t n_images,
                            const int32_t* crops, int32_t B, int32_t lr_h, int32_t lr_w, int32_t scale, int32_t bgr,
                            float* gt, float* lq, hcf_stream_t stream);

/* ---- differentiable MATLAB-bicubic resize (hcf_resize.hip): tensor to tensor, down and up, with its transpose ----
 * The reference's imresize of a float image with method 'bicubic' (utils/imresize.py:136-174), per plane of a dense NCHW fp32
 * DEVICE tensor x [B,C,H,W], C >= 1: `up` = 0 scales by 1 / s (antialiased), `up` = 1 by s, s an integer in 2 .. 8. The output
 * is [B,C,Ho,Wo] with Ho = ceil(H * scale), Wo = ceil(W * scale) (:31-35; non-multiples are legal: 13 x 18 at 1/4 -> 4 x 5).
 * Nothing is clipped: up-scaling overshoots [0, 1] as the reference's float path does. Per axis the op is the matrix A of
 * contributions (:63-83): u = o / scale + 0.5 (1 - 1 / scale) (1-based), P = ceil(4 max(1, 1 / scale)) + 2 taps, weights
 * scale * cubic(scale * t) (down) or cubic(t) (up) (:53-60), each output row normalised to sum 1, indices mirrored through
 * aux = [0 .. n-1, n-1 .. 0] modulo 2n (which wraps more than once when the image is shorter than the support). y = A_h x A_w^T,
 * rows first (:157,169-171: equal scales keep dimension 0 first).
 * Arithmetic: the weights are computed in float64 on the host and rounded once to fp32; each pass is one fp32 fma chain in tap
 * order k = 0 .. P-1; the row pass runs first, then the column pass; no atomics. A result is bit-reproducible and independent
 * of the batch around the image, and a contiguous view that is only 4-byte aligned gives the bits of an aligned copy.
 * The backward is the exact transpose gx = A_h^T gy A_w, columns first, in gather form over transposed tables: per input index
 * the (output index, weight) entries in ascending (output, tap) order, one fp32 fma chain in that order; mirrored taps that land
 * on one input index stay separate entries. The same determinism properties hold.
 *   hcf_resize_workspace         bytes of the caller-allocated device scratch of either call (the [B,C,Ho,W] intermediate of
 *                                the two passes); 0 for arguments the calls refuse.
 *   hcf_resize_bicubic           y [B,C,Ho,Wo] from x [B,C,H,W].
 *   hcf_resize_bicubic_backward  gx [B,C,H,W] from gy [B,C,Ho,Wo]; H, W are the FORWARD input's size.
 *   hcf_resize_tables            host only, touches no device: the table the kernels use for one axis of length in_len.
 *                                transposed = 0: rows = out_len lists of L = P entries, entry k of row o = tap k of output o.
 *                                transposed = 1: rows = in_len lists, row i = the (output, weight) entries of input index i in
 *                                the order above, L = the longest list. Returns L (> 0) or a negative status. With w, idx and
 *                                cnt all NULL only L is returned; otherwise w [rows * L] (float64: the kernels use each value
 *                                rounded once to fp32), idx [rows * L] (-1 behind a list's end) and cnt [rows] are filled,
 *                                entry k of row r at r * L + k; capacity = entries available in w and idx.
 * The device tables are cached in the library per (device, length, s, direction) and uploaded once: the FIRST use of a key may
 * allocate, copy from the host and synchronise once; every later call of that shape allocates nothing, copies nothing from the
 * host and never synchronises. A graph capture therefore needs one warm-up call of the same shape outside the capture.
 * Every entry checks its arguments before any HIP call: null pointers, B, C, H, W (in_len) < 1, s outside 2 .. 8, `up` /
 * `transposed` other than 0 / 1 -> HCF_ERR_ARG; a work_bytes (capacity) that is too small, an output side beyond int32, a
 * tensor (input, output or intermediate) whose byte count leaves int64, more than 65535^2 planes -> HCF_ERR_SHAPE. */
size_t hcf_resize_workspace(int32_t B, int32_t C, int32_t H, int32_t W, int32_t s, int32_t up);
int hcf_resize_bicubic(const float* x, int32_t B, int32_t C, int32_t H, int32_t W, int32_t s, int32_t up, float* y, void* work,
                       size_t work_bytes, hcf_stream_t stream);
int hcf_resize_bicubic_backward(const float* gy, int32_t B, int32_t C, int32_t H, int32_t W, int32_t s, int32_t up, float* gx,
                                void* work, size_t work_bytes, hcf_stream_t stream);
int hcf_resize_tables(int32_t in_len, int32_t s, int32_t up, int32_t transposed, double* w, int32_t* idx, int32_t* cnt,
                      int64_t capacity);

/* ---- training criteria (hcf_loss.hip): pixel, reconstruction, Charbonnier, latent and GAN terms, each with its backward ----
 * Every term is evaluated in fp64 from the fp32 inputs and summed in fp64 through per-block partials of a grid that the SHAPE
 * alone decides and one fixed-order final block: no atomics, no cross-block waiting, bit-reproducible. A result is rounded to
 * fp32 once. No entry allocates, copies to or from the host or synchronises; all run on `stream`. Inputs need 4-byte alignment
 * only: any base pointer and any row length give the bits an aligned copy gives. A backward recomputes from the inputs (the
 * forward stores no gradient) and reads its upstream gradient `g` from DEVICE memory; where g == 0 it stores exact zeros,
 * also for a non-finite difference, so a term the caller dropped does not poison its inputs.
 *
 * Pair criterion. x, y: [B][n] fp32 contiguous (y NULL: zeros), d = (double)x - (double)y,
 *   kind 0  |d|                  nn.L1Loss (HCFlow_SR_model.py:47-52 cri_pix_hr)
 *   kind 1  d^2                  nn.MSELoss; ReconstructionLoss('l2') (loss.py:83-84)
 *   kind 2  sqrt(d^2 + eps)      CharbonnierLoss (loss.py:5-15); ReconstructionLoss('l1') (loss.py:85-87)
 * A block never straddles a sample; S_b = the sample's partials joined in a fixed order that depends on n alone, so row b of
 * a batch has the bits of the one-row call; S = S_0 + S_1 + ... in index order.
 *   out (nullable)      one float, fp32(scale * S)
 *   out_rows (nullable) [B], fp32(row_scale * S_b)                 (at least one of the two)
 * The sums cover every element: one NaN or inf makes the result non-finite (the callers' isnan / isfinite gates need no pass
 * of their own, HCFlow_SR_model.py:210, HCFlow_Rescaling_model.py:223-228).
 * Backward: gx = fp32((double)g[b * g_stride] * scale * f'(d)), f' = sign(d) (0 at 0) / 2 d / d / sqrt(d^2 + eps); gy (nullable)
 * = -gx in the same launch; at least one of gx, gy. g_stride 0: one upstream scalar; 1: one per sample (then `scale` is the
 * forward's row_scale).
 * HCF_ERR_ARG: x NULL, no output, B < 1, n < 1, kind outside 0 .. 2, eps negative or not finite, g NULL, g_stride outside
 * 0 / 1, a pointer that is not 4-byte aligned, work NULL or not 8-byte aligned; HCF_ERR_SHAPE: B * n > 2^40 or more than 2^23
 * blocks (B * min(ceil(n / 4096), 1024)); HCF_ERR_NOMEM: work_bytes below the workspace size. */
size_t hcf_loss_pair_workspace(int64_t B, int64_t n);
int hcf_loss_pair(const float* x, const float* y, int64_t B, int64_t n, int32_t kind, double eps, double scale, double row_scale,
                  float* out, float* out_rows, void* work, size_t work_bytes, hcf_stream_t stream);
int hcf_loss_pair_backward(const float* x, const float* y, int64_t B, int64_t n, int32_t kind, double eps, double scale,
                           const float* g, int32_t g_stride, float* gx, float* gy, hcf_stream_t stream);

/* Mean square over several tensors: out = fp32(sum_k sum_i z_k[i]^2 / N), N = sum_k len[k] -- the latent term
 * (torch.cat([z1.flatten(), z2.flatten()]) ** 2).mean() of HCFlow_Rescaling_model.py:216 without the concatenation. z, len: HOST
 * tables of `count` device pointers / lengths, 1 <= count <= 8, read during the call. Backward: gz[k][i] = fp32((double)g[0] *
 * (2 / N) * z_k[i]) for every k with gz[k] != NULL (gz: a host table as z), exact zeros where g[0] == 0.
 * HCF_ERR_ARG: a NULL table or tensor, count outside 1 .. 8, a length < 1, misaligned pointers, out / g NULL, no gz[k] at all;
 * HCF_ERR_SHAPE: N > 2^40; HCF_ERR_NOMEM: work_bytes below the workspace size. */
size_t hcf_loss_sumsq_workspace(const int64_t* len, int32_t count);
int hcf_loss_sumsq(const float* const* z, const int64_t* len, int32_t count, float* out, void* work, size_t work_bytes,
                   hcf_stream_t stream);
int hcf_loss_sumsq_backward(const float* const* z, const int64_t* len, int32_t count, const float* g, float* const* gz,
                            hcf_stream_t stream);

/* GAN criteria (loss.py:19-51 GANLoss and its callers HCFlow_SR_model.py:242-247 generator step, :271-278 discriminator step).
 * a: na logits with target ta; b (nullable: then nb must be 0): nb logits with target tb. The discriminator outputs [B,1]
 * (Discriminator_VGG_128 / _160) and [B,1,h,w] (PatchGAN): na, nb <= 2^20, beyond that HCF_ERR_SHAPE.
 *   type 0  max(v,0) - v t + log1p(exp(-|v|))    nn.BCEWithLogitsLoss, 'gan' / 'ragan'
 *   type 1  (v - t)^2                            nn.MSELoss, 'lsgan'
 *   type 2  t > 0.5 ? -v : v                     wgan_loss, 'wgan-gp'
 * relativistic 0: v = a (and v = b); 1 (needs b): v_a = a - mean(b), v_b = b - mean(a). All arithmetic fp64, ONE block, fixed
 * order. out[5] = {term_a = mean_i f(v_a[i], ta), term_b (0 without b), total, mean(a), mean(b) (0 without b)} as fp32; total =
 * term_a + term_b, halved when `halve` != 0 (:247, :278).
 * Backward: the analytic gradient of `total`, times the device scalar g[0], to ga (nullable) and gb (nullable), at least one;
 * the relativistic form includes the paths through both means; one launch; exact zeros where g[0] == 0.
 * HCF_ERR_ARG: a NULL, na < 1, nb < 0, b NULL with nb > 0 or the reverse, type outside 0 .. 2, relativistic / halve outside
 * 0 / 1, relativistic without b, out / g NULL, neither ga nor gb, gb without b, misaligned pointers, a target that is not
 * finite. */
int hcf_loss_gan(const float* a, int64_t na, double ta, const float* b, int64_t nb, double tb, int32_t type,
                 int32_t relativistic, int32_t halve, float* out, hcf_stream_t stream);
int hcf_loss_gan_backward(const float* a, int64_t na, double ta, const float* b, int64_t nb, double tb, int32_t type,
                          int32_t relativistic, int32_t halve, const float* g, float* ga, float* gb, hcf_stream_t stream);

/* ---- SSIM as a criterion (hcf_ssim.hip): the reference's ssim / calculate_ssim (utils/util.py:914-955) with its gradient ----
 * x, y: dense NCHW fp32 DEVICE tensors [B,C,H,W] with values in [0, data_range]. Per plane the "valid" map of (H-10) x (W-10)
 * values S = ((2 mu_x mu_y + C1)(2 s_xy + C2)) / ((mu_x^2 + mu_y^2 + C1)(s_x + s_y + C2)) under the window w = k k^T, k =
 * cv2.getGaussianKernel(11, 1.5), C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2; a sample's value is the mean over its
 * planes of the planes' map means. With data_range = 1 on [0, 1] data this is the reference's number on the same data times 255.
 * y_channel = 1 (C must be 3, RGB order): one plane per sample, Y = (65.481 R + 128.553 G + 24.966 B + 16 data_range) / 255
 * (data/util.py:209-230 bgr2ycbcr(only_y=True)); the gradient reaches the three channels by those weights.
 * The rules of the training criteria above hold: fp64 terms from the fp32 inputs (the window is applied separably, rows then
 * columns, one fma chain in tap order each), per-block fp64 partials of a grid that H and W alone decide, one fixed-order final
 * block, one rounding to fp32; no atomics; nothing allocates, copies or synchronises. Results are bit-reproducible, row b does
 * not depend on the batch around it, and any 4-byte aligned tensor gives the bits of an aligned copy. Identical inputs give
 * exactly 1 per sample and a loss of exactly 0. One non-finite pixel makes its sample's value non-finite.
 *   hcf_loss_ssim_workspace  bytes of the caller-allocated device scratch of hcf_loss_ssim; 0 for a shape it refuses.
 *   hcf_loss_ssim            out_rows [B] = fp32(SSIM_b); out_loss (nullable) one float, fp32(1 - mean_b SSIM_b).
 *   hcf_loss_ssim_backward   recomputes from x and y (the forward saves nothing). Upstream gradient from DEVICE memory:
 *                            g_stride 1: g [B], one per sample (the gradient of out_rows; scale = 1); g_stride 0: g[0] for
 *                            every sample (the gradient of out_loss; scale = -1 / B). gx = fp32(g_b * scale * dSSIM_b / dx),
 *                            gy likewise, either nullable (at least one); both come from one launch. A sample whose g_b is 0
 *                            gets exact zeros, also where its pixels are not finite.
 * HCF_ERR_ARG: a NULL x, y, out_rows, work or g, neither gx nor gy, B, C, H or W < 1, y_channel / g_stride outside 0 / 1, a
 * data_range that is not positive and finite, a scale that is not finite, a pointer that is not 4-byte aligned (work: 8);
 * HCF_ERR_SHAPE: H or W < 11 (the map is empty) or > 2^20, y_channel with C != 3, more than 65535 planes (B * C, or B with
 * y_channel); HCF_ERR_NOMEM: work_bytes below the workspace size. Every check comes before the first HIP call. */
size_t hcf_loss_ssim_workspace(int64_t B, int32_t C, int32_t H, int32_t W, int32_t y_channel);
int hcf_loss_ssim(const float* x, const float* y, int64_t B, int32_t C, int32_t H, int32_t W, int32_t y_channel, double data_range,
                  float* out_rows, float* out_loss, void* work, size_t work_bytes, hcf_stream_t stream);
int hcf_loss_ssim_backward(const float* x, const float* y, int64_t B, int32_t C, int32_t H, int32_t W, int32_t y_channel,
                           double data_range, const float* g, int32_t g_stride, double scale, float* gx, float* gy,
                           hcf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HCFLOW_H_ */
