/*
 * simq.h -- C-ABI of libsimq.so: the MI355X (gfx950) implementation of the
 * spatial-action-map DQN training step of jimmyyhwu/spatial-intention-maps.
 *
 * The reference defines NO FFI for this path (it is pure Python over
 * torch.nn); the boundary it does define is the Python object contract of
 *   networks.py:6-26    FCN(num_input_channels, num_output_channels).forward
 *   resnet.py:93-104    ResNet.features
 *   train.py:108-141    train(cfg, policy_net, target_net, optimizer, batch, ...)
 *   train.py:28-45      ReplayBuffer.push / sample
 *   policies.py:47-74   DQNPolicy.step
 * Each entry point below names the reference lines it replaces.  The Python
 * mirror of those objects (package `simq`) binds this header with ctypes; see
 * INTEGRATION.md for the stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (simq_last_error() has the
 *     message, thread-local); no C++ exception crosses the boundary;
 *   - every pointer named d_* is a DEVICE pointer owned by the caller (in the
 *     Python host: a torch-ROCm tensor's data_ptr()); the library allocates no
 *     device memory;
 *   - every launch goes to the hipStream_t passed as `stream` (void* here so the
 *     header needs no HIP include); calls are asynchronous;
 *   - activations are NHWC fp32; convolution weights are OHWI fp32 (= [Cout][R][S][Cin]);
 *     the Q-map output is NCHW [B][Cout][96][96] because the reference's flat
 *     action index is CHW-ordered (envs.py:858);
 *   - a plan is immutable after creation and may be shared by streams; workspaces
 *     carry all mutable state.
 */
#ifndef SIMQ_H
#define SIMQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMQ_VERSION 500            /* 0.5.0: simq_plan_options.gemm_split, simq_train_args.third_stream, simq_plan_adopt_side_stream, stem / head inspection names */
#define SIMQ_STATE_WIDTH 96         /* envs.py:2010 */

/* forward modes of simq_forward */
#define SIMQ_MODE_EVAL 0            /* BN uses running stats (policies.py:56, train.py:216)          */
#define SIMQ_MODE_TRAIN 1           /* BN batch stats + running update, activations saved for backward (train.py:114) */
#define SIMQ_MODE_TRAIN_NOGRAD 2    /* same arithmetic as TRAIN, nothing kept for backward (train.py:121)       */

/* kinds reported by simq_param_tensor_info */
#define SIMQ_KIND_CONV_W 0
#define SIMQ_KIND_CONV_B 1
#define SIMQ_KIND_BN_W 2
#define SIMQ_KIND_BN_B 3

/* arithmetic of the 3x3 / 1x1 convolutions (BatchNorm statistics, accumulation, master weights, optimiser: always fp32;
 * the 7x7 stem on the Cin = 3..10 image and the 32 -> Cout head conv3 always run in fp32) */
#define SIMQ_PREC_FP32 0            /* v_mfma_f32_16x16x4_f32: exact fp32 FMA chains                                   */
#define SIMQ_PREC_BF16X3 1          /* split-bf16: v = hi + lo, hi*hi + hi*lo + lo*hi on the bf16 matrix cores (~2^-17) */
#define SIMQ_PREC_BF16 2            /* plain bf16 operands, fp32 accumulate (BASELINE configs 3 and 5)                  */

typedef struct simq_plan simq_plan;

int simq_version(void);
/* 0 for the product library.  SIMQ_BUILD_ABLATIONS: libsimq_ablate.so (tools only): kernel-selection switches are read from SIMQ_*
 * environment variables and the timing-ablation kernels are present; bench.py and the parity tests refuse such a build. */
#define SIMQ_BUILD_ABLATIONS 1
int simq_build_flags(void);
const char* simq_last_error(void);

/* ---- plan: the network of networks.py:7-14 for (Cin, Cout); replaces FCN.__init__ ---------- */
int simq_plan_create(int num_input_channels, int num_output_channels, simq_plan** out);   /* SIMQ_PREC_FP32 */
int simq_plan_create_ex(int num_input_channels, int num_output_channels, int precision, simq_plan** out);
/* (replaces networks.FCN.__init__, networks.py:7-14, like simq_plan_create: the reference has one arithmetic -- cuDNN's -- and no such
 * choice.)  What a plan computes WITH -- which algebraic form, storage precision and fusion each layer uses -- is fixed when the plan is
 * created and is a property of the plan; the library never reads it from the process environment.  Every default below is what the
 * parity tests and the bench run; the other settings exist for A/B measurements and diagnostics and some of them change the
 * round-off of the results (noted per field).  Fill the struct with simq_plan_options_default, change fields, pass it to
 * simq_plan_create_opts (NULL = defaults); struct_bytes must be sizeof(simq_plan_options). */
typedef struct simq_plan_options {
    int struct_bytes;
    /* fp32 plans: Winograd forms of the wide 3x3 layers (docs/history.md 4) */
    int winograd;                 /* 1: layers with Cin*Cout >= winograd_min_cc run as F(2x2,3x3) / F(4x4,3x3); 0: direct implicit GEMM */
    int winograd_min_cc;          /* 128*128: layers 2-4 */
    int winograd_f4_forward;      /* 1: the forwards nothing is differentiated through (target net, greedy next action, step()) in F(4x4,3x3) */
    int winograd_f4_min_tiles;    /* 256: ... from this many 4x4 tiles (B*36) */
    int winograd_f4_grad;         /* 2: dgrads in F(4x4,3x3); 1: the grad-mode forward too (doubles the median gradient error); 0: neither */
    int winograd_f4_fwd_grad_min_cc; /* 512*512 (0 = never).  With winograd_f4_grad = 2: the GRAD-MODE forward of the layers with Cin*Cout >= this
                                   * value runs in F(4x4,3x3) as well -- layer4's three 512->512 convolutions, 66 % of the grad-mode forward's
                                   * matrix flops.  Their round-off passes through no further residual block: the gradient study (19 batches
                                   * against fp64) is unchanged by it, while 256*512 and below raise the gradient's error (docs/history.md 4) */
    int winograd_wgrad;           /* 1: weight gradients of the Winograd layers through the transform domain */
    int winograd_wgrad_f4;        /* 1: ... in F(4x4,3x3) where the tile count allows */
    /* bf16 plans: storage */
    int stem_bf16;                /* 1: first convolution + its weight gradient on the bf16 matrix cores where 7 * num_input_channels <= 63;
                                   * 2: as 1, and the wide-row form of both kernels where 64 <= 7 * num_input_channels <= 95 (10..13 channels,
                                   * DESIGN 26); 0: the fp32 kernels.  Any other value is refused */
    int bf16_act_grads;           /* 1: activation gradients between the residual blocks' kernels travel as bf16 */
    int keep_fp32_activations;    /* 0: post-BN activations exist as bf16 planes only; 1 keeps fp32 copies (simq_workspace_tensor readers) */
    int fold_eval_bn_bf16;        /* 1: eval-mode BatchNorm folded into the convolution epilogues (one rounding instead of two) */
    /* every precision: fusions (0 = separate reduction launches, same arithmetic in a different summation order) */
    int fuse_bn_backward_sums;    /* 1 */
    int fuse_stem_backward_sums;  /* 1 */
    /* train-mode "conv -> BatchNorm -> ReLU -> conv" chains with ONE consumer (bn1 of every BasicBlock, resnet.py:34-40; bn1 of the head,
     * networks.py:18-20): the activation in between is never stored.  Same arithmetic (the fma / max bn_apply performs), bit-identical results. */
    int fuse_bn1_apply;           /* 1 (fp32 plans): the consuming convolution applies scale*y+shift -> ReLU while it stages its operand (Winograd input
                                   * transforms, image-tile / implicit-GEMM loaders), its weight gradient and the BatchNorm backward recompute the
                                   * activation / its mask from the saved pre-BN output.  Needs fuse_bn_backward_sums. */
    int deterministic;            /* 0.  1: run-to-run bit-identical results UP TO the rounding of the fp64 reductions (debugging aid, e.g. rank
                                   * divergence in data-parallel runs): every fp32 reduction of the step has a fixed order -- the weight gradients
                                   * whose pixel reduction is split over blocks leave per-split partial tiles in a slab that a second launch adds
                                   * in split order, instead of fp32 atomics (64 MB more workspace, plus a slab of the first convolution's own,
                                   * 96 x 64 x 49 x num_input_channels floats and at most 64 MB, so that its weight gradient may run beside the
                                   * last block's); the one-hot head backward still runs one block per transition, each leaves its terms of the
                                   * last layer's gradients in 512 B of workspace and a one-block launch adds them in transition order.  The
                                   * BatchNorm sums (forward statistics, the backward's [sum dz | sum dz*xhat]) stay fp64 atomics in
                                   * arbitrary order in either setting: a result changes only if two orders of an fp64 sum round to different fp32
                                   * values (~1e-9 per consumer; never observed: tests/diag/diag_determinism.py, tests/test_gpu_overlap.py compare
                                   * whole steps bit for bit), so "bit-identical" is an observation about those sums, not a guarantee. */
    int bn1_mask_from_preact;     /* 1 (plain-bf16 plans): the backward pass takes that ReLU mask from the saved pre-BN output (scale*y+shift > 0)
                                   * instead of reading the activation's plane -- one bf16 plane less in bn_bwd_apply and in the dgrad epilogue */
    /* Round 5: what used to be process-global simq_tune_* switches.  A plan's result and its launch schedule depend on the plan alone. */
    int wgrad_ksplit;             /* 0.  K-split of the transform-domain weight-gradient GEMMs (the wgrad half of loss.backward(), train.py:132, of the
                                   * 128->256- and 256-channel 3x3 convolutions): 0 = chosen by shape, 1 = none, 2 / 4 = forced where the tile count
                                   * divides.  Changes the SUMMATION ORDER of those gradients (fixed per setting: deterministic), nothing else. */
    /* scheduling only (same kernels on the same operands; results are bit-identical for deterministic plans): */
    int fwd_overlap;              /* 2.  Where simq_train_step forks its no-grad forwards (train.py:119-122).  2 = all three forwards side by side from
                                   * the start of the step: the target net's on the side stream, the policy's no-grad forward on a third, plan-owned
                                   * stream with its BatchNorm running-statistics update deferred and applied behind the grad-mode forward's, in the
                                   * reference's order (bit-identical buffers); 0 = the target-net forward on the side stream behind the policy's
                                   * grad-mode forward, the policy's no-grad forward on the main stream; 1 = as 0 with the target-net forward forked at
                                   * the start of the step.  Steps under SyncBN keep form 0. */
    int wgrad_overlap;            /* 4.  The weight gradient of every residual-block convolution runs on a side stream beside the dgrads of the walk --
                                   * simq_train_step's side stream, or a plan-owned one (per device, destroyed with the plan) when a backward entry
                                   * point is called on its own; the caller's stream is joined before the call returns its last launch.
                                   * 4 = until the temporaries of the block are written again two blocks later (a second set of gradient temporaries
                                   * in the workspace; matrix-core plans: for the default planes-only form, with dy1 on a plane of its own -- other
                                   * matrix-core plans keep the serial order); fp32 plans only: 1 = until the end of the residual block, 3 = beside
                                   * the dgrad of the same convolution only; 2 = as 1 for every precision (measured slower for bf16); 0 = behind the
                                   * dgrad on the caller's stream: no hidden stream at all (graph capture, profilers that must see every launch on
                                   * the caller's stream). */
    int plane_xcd;                /* 1.  The batched transform-domain GEMMs of the Winograd layers walk whole transform elements per XCD; 0 = launch order */
    int wgrad_xcd_group;          /* 1.  Pixel-split weight-gradient kernels place the tiles that share a pixel range on one XCD: 1 = the bf16 kernel
                                   * only, 2 = the fp32 kernel too (measured slower there), 0 = launch order */
    int tail_split;               /* 0.  fp32 implicit GEMM: balanced last round (K-sliced tail tiles + fix-up kernel); pays only when the forwards run
                                   * serialised; changes the fp32 summation order of the sliced tiles */
    int early_target_after_block; /* 4.  simq_train_args.target_stream (the target net's forward of step t+1 on a stream that does not wait for step t):
                                   * that forward additionally waits until step t's backward walk reaches residual block N (7 = layer4's second block,
                                   * the first of the walk ... 0 = layer1's first, the last), so that it runs beside the END of that backward pass, the
                                   * optimiser step and the weight-cache refresh -- the part of a step with the fewest matrix kernels -- instead of
                                   * racing through the start of the backward pass.  -1 = no such wait.  Ordering only: results are bit-identical. */
    /* Round 6: fp32 plans -- which matrix pipe contracts the transform-domain GEMMs of the Winograd layers (forward, dgrad, weight gradient) */
    int gemm_split;               /* 1.  0 = v_mfma_f32_16x16x4_f32 on the fp32 operands (the fp32 FMA chain of rounds 1-5).
                                   * 1 = the bf16 matrix cores through an EXACT three-way split of both fp32 operands (v = v0 + v1 + v2 in bf16
                                   * pieces cut by truncation, no bit dropped) and SIX of the nine piece products, fp32 accumulate
                                   * (gemm_split3.hip): fp32 operands, fp32 accumulators, fp32 output, at 6/16 of the matrix-pipe time.  The
                                   * split is exact; the product is not: the three dropped piece products (a1 b2 + a2 b1 + a2 b2) are bounded
                                   * by 2^-21 |a b| per product (about 4 fp32 ulp, reached by mantissas 0x00FFFF), carry the product's sign --
                                   * a bias towards zero, not zero-mean round-off -- and average about 2^-24.6 |a b| on random mantissas.  On
                                   * randn operands the rms error against fp64 is 0.85 x form 0's (tests/test_gpu_ops.py); the kept terms,
                                   * the bound and the bias are pinned by tests/test_gpu_split3.py against tests/split3_oracle.py.  Bit-exact
                                   * statements hold while every piece is at least 2^-126 in magnitude (operands from about 2^-103 up; what
                                   * happens below: DESIGN.md 4).  An Inf operand yields NaN (Inf - Inf in the split), not +-Inf as form 0.
                                   * Changes the round-off of those contractions (summation order and the dropped terms), nothing else. */
    /* plain-bf16 plans: the element type of the INPUT */
    int bf16_states;              /* 0.  1 = every entry point of this plan that takes states reads them as [batch][96][96][Cin] bf16 (uint16_t
                                   * storage, NHWC, 2-byte aligned) behind its `const float*`: d_x of simq_forward / simq_forward_sync,
                                   * simq_train_args.state / next_state, and the backward entries through the copy the grad-mode forward
                                   * keeps (which is then a bf16 copy).  Only for plans whose first convolution runs stem_conv_bf16 -- precision
                                   * SIMQ_PREC_BF16, stem_bf16 = 1 and 7 * num_input_channels <= 63, or stem_bf16 = 2 and <= 95 (the wide-row
                                   * form) -- the creation of any other plan with
                                   * the option fails: that convolution (and its weight gradient) rounds every fp32 input element to
                                   * bf16 before anything else and nothing else reads the input, so a bf16 state that is the round-to-
                                   * nearest-even of the fp32 state gives bit for bit what the fp32 state gives, in half the bytes.  The
                                   * workspace of such a plan is never larger than the same plan's without the option. */
} simq_plan_options;
void simq_plan_options_default(simq_plan_options* options);
int simq_plan_create_opts(int num_input_channels, int num_output_channels, int precision, const simq_plan_options* options,
                          simq_plan** out);
int simq_plan_get_options(const simq_plan* plan, simq_plan_options* out);
int simq_plan_precision(const simq_plan* plan);
void simq_plan_destroy(simq_plan* plan);

/* Flat parameter buffer layout.  All tensors that receive a gradient (70 in the
 * reference; resnet18.fc.* is excluded because features() never uses it) live
 * in ONE fp32 buffer of simq_param_count() elements, in reference state_dict
 * order.  Gradients and SGD momentum use identically laid-out buffers.  */
int64_t simq_param_count(const simq_plan* plan);
int simq_param_num_tensors(const simq_plan* plan);
/* name: reference key without the "module." prefix, e.g. "resnet18.layer1.0.conv1.weight".
 * shape: conv weights report {Cout, R, S, Cin} (OHWI, device layout), vectors {C,1,1,1}.      */
int simq_param_tensor_info(const simq_plan* plan, int index, char* name, int name_cap,
                           int64_t* offset, int64_t shape[4], int* kind);
/* BN running statistics: one fp32 buffer, per BN layer [mean(C) | var(C)], reference order. */
int64_t simq_bnbuf_count(const simq_plan* plan);
int simq_bn_num_layers(const simq_plan* plan);
int simq_bn_layer_info(const simq_plan* plan, int index, char* name, int name_cap, int64_t* offset, int* channels);

/* Bytes of workspace simq_forward/simq_backward need for `batch` samples. */
int64_t simq_workspace_bytes(const simq_plan* plan, int batch);
/* ... when the workspace only ever serves forward passes (the target net's, the no-grad forward's `ws_tmp`, policy.step): the same
 * layout without the scratch slabs of the weight-gradient kernels at its end (75.5 MB per workspace in plain-bf16 plans). */
int64_t simq_workspace_bytes_forward(const simq_plan* plan, int batch);

/* Weight cache: derived copies of the convolution weights (flipped/transposed for dgrad; bf16 planes for the matrix-core
 * precisions).  Caller-owned buffer of simq_wcache_bytes(); call simq_weights_prepare after EVERY change of d_params
 * (optimiser step, load_state_dict, target sync) and pass the buffer to simq_forward / simq_backward.               */
int64_t simq_wcache_bytes(const simq_plan* plan);
int simq_weights_prepare(const simq_plan* plan, const float* d_params, void* d_wcache, void* stream);

/* Inspection aid (parity bisecting): where a saved NHWC fp32 activation lives inside the workspace after simq_forward.
 * name: "stem.conv" | "stem.pool" | "layer<1-4>.<0-1>" (BasicBlock outputs) | "head.a1" | "head.a2".
 * In the matrix-core precisions the block outputs live as bf16 planes only; their fp32 copies are written by plans created with
 * simq_plan_options.keep_fp32_activations = 1 (diagnostics).
 * Which forward wrote what: "head.a2" (the 48x48x32 activation) is written by GRAD-MODE forwards only (SIMQ_MODE_TRAIN: the backward pass
 * reads it) -- the no-grad forward and the folded eval head (one pass: upsample -> ReLU -> conv3) never store it, the offset then holds
 * whatever an earlier forward left.  "head.a1": eval-mode forwards of every plan and train-mode forwards of plans WITHOUT
 * fuse_bn1_apply; fp32 plans with the fusion (the default) never store it in the train modes and the call refuses the name.          */
int simq_workspace_tensor(const simq_plan* plan, int batch, const char* name, int64_t* byte_offset, int64_t* elems,
                          int* channels);

/* The block-internal tensors a forward pass leaves in its workspace (teacher-forced parity tests: every stored tensor against an fp64
 * recomputation from the STORED tensors it was computed from).  name: "layer<1-4>.<0-1>.<y1|a1|y2|yd|out>" (pre-BatchNorm outputs of
 * conv1 / conv2 / the downsample convolution, the activation between the two convolutions, the block output; NHWC [batch][24][24][C]),
 * "layer<l>.<b>.<bn1|bn2|bnd>" (4*C floats: scale | shift | mean | invstd as the consuming kernel formed them), "stem.pool.plane"
 * (matrix-core precisions), "layer<l>.<b>.<red1|red2|redd>" (2*C doubles: the BatchNorm's reduction slot -- after a backward pass
 * [sum dz | sum dz*xhat]).  Round 6, the stem (resnet.py:94-97) and the head (networks.py:18-26 in the order the plan runs it): "stem.y0"
 * ([batch][48][48][64], the 7x7 convolution's pre-BN output), "stem.bn" / "stem.red", "stem.idx" (uint8 [batch][24][24][64]: the max-pool's
 * first maximal window slot dy*3+dx), "head.y1" ([batch][24][24][128] conv1 pre-BN), "head.bn1" / "head.red1", "head.a1.plane" (matrix-core
 * precisions), "head.z2" ([batch][24][24][32]: conv2 + bias, before the first bilinear x2), "head.y2" ([batch][48][48][32]: BatchNorm 2's input),
 * "head.bn2" / "head.red2", "head.z3" ([batch][48][48][Cout]: conv3 before the second bilinear x2 and the bias).
 * storage: 0 fp32, 1 bf16, 2 fp64, 3 uint8.  Fails for tensors the plan does not store (e.g. a1 under fuse_bn1_apply). */
int simq_workspace_tensor_ex(const simq_plan* plan, int batch, const char* name, int64_t* byte_offset, int64_t* elems, int* channels,
                             int* storage);

/* ---- FCN.forward (networks.py:16-26) ---------------------------------------------------------
 * d_x      [batch][96][96][Cin] fp32 NHWC  (== the reference's HWC replay states, stacked); a plan with
 *          simq_plan_options.bf16_states = 1 reads [batch][96][96][Cin] bf16 behind this pointer instead
 * d_q      [batch][Cout][96][96] fp32 NCHW
 * d_bnbuf  running stats; updated in place in TRAIN / TRAIN_NOGRAD modes (momentum 0.1,
 *          unbiased variance), read-only in EVAL.                                            */
int simq_forward(const simq_plan* plan, int mode, int batch, const float* d_params, const void* d_wcache, float* d_bnbuf,
                 const float* d_x, float* d_q, void* d_workspace, void* stream);

/* ---- autograd backward of FCN.forward (loss.backward(), train.py:132) ----------------------------
 * d_workspace must be the one used by the matching simq_forward(mode=TRAIN) call.
 * d_dq     [batch][Cout][96][96] upstream gradient (dense).
 * d_grads  flat gradient buffer (param layout); OVERWRITTEN.
 * (No backward entry takes states: the first convolution's weight gradient reads the copy the grad-mode forward left in the workspace --
 * a bf16 copy, half the size, in a plan with simq_plan_options.bf16_states = 1.)
 * The matching forward must be a simq_forward / simq_forward_sync call: simq_train_step convolves the caller's minibatch IN PLACE and leaves
 * no copy of it in the workspace, so a backward entry point called on its own behind a simq_train_step would differentiate the first
 * convolution against whatever an earlier simq_forward left there (the Python host refuses that: FCN._train_workspace_for_backward). */
int simq_backward(const simq_plan* plan, int batch, const float* d_params, const void* d_wcache, const float* d_dq,
                  float* d_grads, void* d_workspace, void* stream);

/* Inspection aid of the backward walk (teacher-forced parity tests, tests/test_gpu_bf16_points.py): simq_backward with every gradient
 * tensor that travels between the kernels of a residual block (resnet.py:31-47 reversed) copied into d_trace as it becomes final --
 * the walk itself reuses four temporaries.  name: "layer<1-4>.<0-1>.<g_out|dy2|dz|dyd|da1|dy1|g_ds|g_in>" = gradient w.r.t. the block output
 * (as received), conv2's pre-BN output, the masked gradient dz = g_out * [out > 0] (identity blocks: the shortcut's addend), the
 * downsample convolution's pre-BN output (downsample blocks), the activation between the convolutions, conv1's pre-BN output, the
 * downsample convolution's data gradient (downsample blocks: the addend of conv1's data gradient), the block input; NHWC [batch][24][24][C].
 * Round 6: "head.<da2|dy2>" ([batch][48][48][32]: w.r.t. the activation behind / the input of the head's BatchNorm 2), "head.dz2"
 * ([batch][24][24][32]: w.r.t. conv2's output), "head.<da1|dy1>" ([batch][24][24][128]: behind / in front of BatchNorm 1), "stem.dz"
 * ([batch][48][48][64]: max-pool + ReLU backward) and "stem.dy0" (w.r.t. the 7x7 convolution's output).
 * storage as simq_workspace_tensor_ex.  d_trace: simq_backward_trace_bytes() bytes. */
int64_t simq_backward_trace_bytes(const simq_plan* plan, int batch);
int simq_backward_trace_tensor(const simq_plan* plan, int batch, const char* name, int64_t* byte_offset, int64_t* elems, int* channels,
                               int* storage);
int simq_backward_traced(const simq_plan* plan, int batch, const float* d_params, const void* d_wcache, const float* d_dq,
                         float* d_grads, void* d_workspace, void* d_trace, void* stream);

/* Two-phase form for data-parallel callers: phase 1 (zero-fill + head + layer4) leaves d_grads[simq_grad_bucket_split() ..]
 * final, so its all-reduce can overlap phase 2 (layers 3..1 + stem, which completes d_grads[0 .. split)).  phase 0 = both. */
int simq_backward_phase(const simq_plan* plan, int batch, const float* d_params, const void* d_wcache, const float* d_dq,
                        float* d_grads, void* d_workspace, int phase, void* stream);
int64_t simq_grad_bucket_split(const simq_plan* plan);
/* The same walk for the TD loss's upstream gradient in its natural one-hot form: dQ[b][d_action[b]] = clamp(d_q_sa[b] - d_y[b],
 * -1, 1) * grad_scale and zero elsewhere (train.py:115,129) -- no dense dQ map, the head starts from B pixels.  phase as above. */
int simq_backward_onehot(const simq_plan* plan, int batch, const float* d_params, const void* d_wcache, const int64_t* d_action,
                         const float* d_q_sa, const float* d_y, float grad_scale, float* d_grads, void* d_workspace, int phase,
                         void* stream);

/* ---- optional cross-rank BatchNorm statistics ("SyncBN") ----------------------------------------------------------
 * The reference's multi-GPU form (nn.DataParallel, policies.py:39) normalises every replica with ITS OWN batch statistics, and that is
 * what the data-parallel step does by default.  With a simq_sync the train-mode BatchNorms of simq_forward_sync / simq_backward_sync
 * use the statistics of the GLOBAL minibatch instead, which makes an N-rank step arithmetically the single-device step on the whole
 * minibatch: after every convolution the [sum | sum of squares] of its BatchNorm (2*C doubles), and in the backward walk every
 * [sum dz | sum dz*xhat], are handed to `reduce` (sum over ranks, in place, ordered on `stream`) before they are consumed -- 44 small
 * latency-bound reductions per step.  global_batch = transitions over all ranks (row counts scale by global_batch / batch);
 * d gamma / d beta are written as 1/world_size of the global sums, so that the flat-gradient all-reduce restores them.
 * simq_comm_reduce_f64 is a ready-made `reduce` over a simq_comm (user = the communicator). */
typedef int (*simq_reduce_fn)(void* user, double* d_buf, int64_t count, void* stream);
typedef struct simq_sync { simq_reduce_fn reduce; void* user; int global_batch; int world_size; } simq_sync;
/* (d_x as in simq_forward: bf16 states behind the pointer in a plan with simq_plan_options.bf16_states = 1) */
int simq_forward_sync(const simq_plan* plan, int mode, int batch, const float* d_params, const void* d_wcache, float* d_bnbuf,
                      const float* d_x, float* d_q, void* d_workspace, void* stream, const simq_sync* sync);
/* d_dq != NULL: dense upstream gradient (simq_backward_phase); d_dq == NULL: the one-hot form (simq_backward_onehot) */
int simq_backward_sync(const simq_plan* plan, int batch, const float* d_params, const void* d_wcache, const float* d_dq,
                       const int64_t* d_action, const float* d_q_sa, const float* d_y, float grad_scale, float* d_grads,
                       void* d_workspace, int phase, void* stream, const simq_sync* sync);
int simq_comm_reduce_f64(void* comm, double* d_buf, int64_t count, void* stream);
/* A rank whose shard holds no input for a synchronised train-mode forward (the double-DQN forward over the non-final next states of
 * an all-terminal shard) still has to take part in that forward's reductions: contributes zeros, in the forward's order.
 * The reduced sums are the global batch statistics: with d_bnbuf != NULL the rank also applies the running-mean / running-var
 * update the other ranks apply (momentum 0.1, unbiased variance over rows x sync->global_batch), so that its BatchNorm buffers do
 * not drift from theirs (the caller counts the forward in num_batches_tracked like the ranks that had rows).
 * d_workspace: any workspace of this plan sized for `layout_batch` >= 1. */
int simq_forward_sync_null(const simq_plan* plan, int layout_batch, float* d_bnbuf, void* d_workspace, void* stream, const simq_sync* sync);

/* ---- learner pieces of train() (train.py:115-129) -------------------------------------------- */
/* flat max / first-index argmax over each row of d_q [rows][n]  (train.py:121,124; policies.py:64): tensor.max(1) -- a NaN is the
 * maximum, the first NaN's index is returned and d_max is NaN */
int simq_q_argmax(const float* d_q, int rows, int n, int64_t* d_index, float* d_max, void* stream);
/* d_out[i] = d_q[i][d_index[i]]  (train.py:115,122) */
int simq_q_gather(const float* d_q, int rows, int n, const int64_t* d_index, float* d_out, void* stream);
/* next_state_values[nonfinal_pos[i]] = d_values[i]; others 0 (train.py:116,122); 1 <= batch <= 4096 (the minibatch limit of every entry point),
 * 0 <= n_nonfinal <= batch */
int simq_scatter_next_values(const float* d_values, const int32_t* d_nonfinal_pos, int n_nonfinal,
                             float* d_next_state_values, int batch, void* stream);
/* y = r + gamma*v ; td = |q_sa - y| ; loss = mean Huber(delta=1) ; dq = one-hot dLoss/dQ
 * (train.py:115,126-129 and the gradient autograd would deliver to `output`).  A NaN difference gives a NaN gradient.
 * grad_scale = 1/global_batch (train.py:129 'mean'; data-parallel ranks pass the GLOBAL batch).
 * d_out4: {sum Huber, sum |td|, unused, unused} over this rank's rows (host divides).       */
int simq_td_huber(const float* d_q, int batch, int n, const int64_t* d_action, const float* d_reward,
                  const float* d_next_state_values, float gamma, float grad_scale,
                  float* d_q_sa, float* d_y, float* d_td_error, float* d_out4, float* d_dq, void* stream);

/* ---- clip_grad_norm_ + SGD.step (train.py:133-135,186) ----------------------------------------
 * total_norm = ||g||_2 ; g *= min(1, max_norm/(total_norm+1e-6)) (skipped when max_norm <= 0);
 * a NaN norm gives a NaN coefficient, an Inf norm 0, as clip_grad_norm_ has them;
 * g += wd*p ; m = first_step ? g : momentum*m + g ; p -= lr*m.
 * d_scratch: >= 16 bytes; receives {double sumsq}.  d_total_norm (may be NULL): 1 float.     */
int simq_clip_sgd_step(float* d_params, float* d_grads, float* d_momentum, int64_t count,
                       float max_norm, float lr, float momentum, float weight_decay, int first_step,
                       void* d_scratch, float* d_total_norm, void* stream);

/* ---- replay minibatch gather (train.py:40-42,109,112) -------------------------------------------
 * d_ring [capacity][96][96][C] fp32; d_out[i] = d_ring[d_index[i]].  item_floats a multiple of 4.
 * The kernel moves bits, 16 bytes at a time: a ring of bf16 states (96 * 96 * C is even for every C, so an item is a whole number of
 * 4-byte words) is gathered with item_floats = 96 * 96 * C / 2, the pointers standing for the bf16 arrays.                          */
int simq_replay_gather(const float* d_ring, int64_t item_floats, const int64_t* d_index, int count,
                       float* d_out, void* stream);

/* ---- replay pool scatter: the inverse of simq_replay_gather, for observations that are already on the device ------------------
 * d_pool [pool_slots][item_floats] fp32; d_pool[slots[p]] = d_src[p] for p < count.  `slots` is a HOST array: every slot is checked
 * before anything is copied or launched (0 <= slot < pool_slots, none named twice, no written slot sharing a byte with d_src or
 * d_desc; 1 <= count <= 65535), then copied to d_desc (at least 8 * count bytes of device scratch, 8-byte aligned) on `stream`.
 * Any item size: rows move as 16-byte vectors where the two addresses allow it, float by float elsewhere.  A refusal writes
 * nothing.  Bits are moved, not values: a pool of bf16 states takes item_floats = 96 * 96 * C / 2 (see simq_replay_gather). */

/* ---- states fp32 <-> bf16 (simq_plan_options.bf16_states) ---------------------------------------------------------------
 * simq_states_to_bf16: d_dst[i] = the bf16 nearest to d_src[i], ties to even -- the conversion the first convolution of a plain-bf16
 * plan applies to an fp32 state: overflow goes to +-Inf, denormals and +-0 are kept, a NaN stays a NaN (its payload is not part of the
 * contract).  simq_states_to_f32: the exact widening (the 16 bits become the high half of the float).  n >= 1 elements; fp32
 * pointers 4-byte, bf16 pointers 2-byte aligned, the two arrays disjoint.  Eight elements move as 16-byte vectors where both addresses
 * reach a 16-byte boundary together, one by one at the ends and where they never do. */
int simq_states_to_bf16(const float* d_src, uint16_t* d_dst, int64_t n, void* stream);
int simq_states_to_f32(const uint16_t* d_src, float* d_dst, int64_t n, void* stream);
int simq_replay_scatter(const float* d_src, int64_t item_floats, const int64_t* slots, int count, float* d_pool, int64_t pool_slots,
                        void* d_desc, int64_t desc_bytes, void* stream);

/* ---- the whole TD step in one call (reference train.train, train.py:108-141, lines 114-135) -------------------------------
 * Policy forward (train-mode BN) on `state`; double DQN: policy forward (train mode, no grad) on `next_state` + argmax, target
 * forward (eval) + gather -- vanilla DQN: target forward + max; scatter into the bootstrap vector, TD target + Huber + dLoss/dQ
 * (scaled by 1/global_batch), backward, global-norm clip + momentum SGD, refresh of the policy weight cache.  Exactly the
 * launches simq.learner.train_step issues, sequenced by the library.  All pointers are device memory owned by the caller; both
 * weight caches must be current on entry (simq_weights_prepare).  side_stream (may be NULL): the target forward runs there,
 * fork/join by events.  Results: out4[0] = sum of Huber terms, out4[1] = sum of |td| over this rank's batch; q_sa, y, td per
 * transition; *total_norm = pre-clip gradient norm.  With `comm` set the gradient buckets are all-reduced between backward and SGD.
 * dq may be NULL: the backward then starts from the one-hot form (simq_backward_onehot) and no dense dQ map is written. */
typedef struct simq_train_args {
    const simq_plan* plan;
    int batch, num_nonfinal, global_batch, use_double_dqn, first_step;
    int sync_bn;                 /* with `comm`: global-minibatch BatchNorm statistics (simq_sync over the communicator) */
    float gamma, lr, momentum, weight_decay, max_norm, reserved2_;
    float* params; void* wcache; float* bnbuf; float* grads; float* momentum_buf; void* ws_train; void* ws_tmp;   /* policy */
    const float* t_params; const void* t_wcache; float* t_bnbuf; void* t_ws;                                      /* target */
    const float* state; const float* next_state; const int64_t* action; const float* reward; const int32_t* nonfinal_pos;
                                 /* (read until the END of the call's stream work: the grad-mode forward convolves `state` in place and the first
                                  * convolution's weight gradient reads it again -- no copy into the workspace.  A plan with
                                  * simq_plan_options.bf16_states = 1 reads [batch | num_nonfinal][96][96][Cin] bf16 behind both pointers) */
    float* q; float* q_next; float* q_tgt; float* dq;               /* [batch|num_nonfinal][Cout*96*96] scratch / outputs */
    float* nsv; float* vals; int64_t* best; float* q_sa; float* y; float* td; float* out4;
    void* opt_scratch; float* total_norm;
    void* stream; void* side_stream;
    int global_nonfinal;         /* sync_bn: non-final next states over all ranks (the double-DQN forward's global row count) */
    int struct_bytes;            /* sizeof(simq_train_args) of the caller's header: checked, so that a struct from another version is refused
                                  * instead of misread (the field sits where round 2's reserved3_ was) */
    struct simq_comm* comm;      /* NULL: single process.  Otherwise the data-parallel form: `batch` is this rank's shard of a
                                  * minibatch of `global_batch` transitions; head + layer4 gradients (simq_grad_bucket_split) are
                                  * summed over the ranks while layers 3..1 + stem are still being differentiated, then the rest
                                  * (out4 is summed over the ranks right behind the TD / Huber launch: three collectives per step,
                                  * in this order on every rank); every rank applies the identical clip + SGD.  num_nonfinal may then be 0 (a shard
                                  * whose transitions are all terminal still has to join the collectives). */
    float* loss_host;            /* NULL, or 4 floats of PINNED host memory: out4 is copied there as soon as it is final (behind the
                                  * TD / Huber launch; with `comm`: behind the all-reduce of out4 that follows it, on the
                                  * communicator's stream), on the library's own copy stream or the caller's third stream.  The
                                  * host then calls simq_train_loss_wait() instead of synchronising the stream: train.py:137-139's
                                  * loss.item() without waiting for backward + SGD, so that the next step is enqueued while this one runs */
    void* target_stream;         /* NULL, or a stream the CALLER has already ordered behind everything the target-net forward reads (next_state,
                                  * the target net's parameters / weight cache, the previous reader of q_tgt and t_ws): the forward of
                                  * train.py:122 is then enqueued there WITHOUT waiting for `stream` -- it depends on nothing this step or the
                                  * previous one computes, so it may run beside the previous step's backward pass and SGD (the host enqueues
                                  * step t+1 while step t still runs, see loss_host) -- and `stream` waits for it where the values are
                                  * gathered.  Needs the three-forward form (side_stream, fwd_overlap = 2, double DQN, non-final next states, no SyncBN):
                                  * an ERROR otherwise (round 6; it used to be ignored silently).  Results are bit-identical. */
    void* third_stream;          /* NULL: the policy's no-grad forward of the three-forward form runs on a stream the plan owns.  Otherwise the
                                  * caller's stream for it (round 6).  Why a caller would care: the HIP runtime multiplexes streams onto 4 hardware
                                  * queues by default, kernels of ONE hardware queue run in order, and which queue a stream lands on follows the
                                  * order in which the process's streams were first used -- with the launch stream and the side (or this) stream on
                                  * one queue the step loses its forward overlap (-13 % measured: profiles/r06_third_leg_order_effect.txt).  The
                                  * Python host picks `stream` / `side_stream` / `third_stream` / `target_stream` from streams it has TESTED to run
                                  * concurrently (simq.learner.LearnerStreams); a C caller can do the same with two spin kernels. */
} simq_train_args;
int simq_train_step(const simq_train_args* a);
/* blocks until the loss_host copy of the last simq_train_step of `plan` on the current device has landed.  The step's streams must belong
 * to the device that was current when simq_train_step was called (checked).  The copy stream and its two events belong to the plan (one
 * set per device, created on first use, destroyed by simq_plan_destroy) -- as do the third stream of fwd_overlap = 2 and the side stream
 * of a backward pass called on its own (wgrad_overlap).  A plan is used by one host thread at a time. */
int simq_train_loss_wait(const simq_plan* plan);
/* Round 6.  The backward entry points called on their own (simq_backward*, FCN.backward) run the weight gradients beside the dgrads on a
 * side stream the plan owns (simq_plan_options.wgrad_overlap).  A stream the library creates lands on whatever hardware queue the runtime
 * gives it -- the launch stream's, on a bad day, and then nothing overlaps (see simq_train_args.third_stream: forward + backward alone 6 500 ->
 * 5 460 tr/s on configs[1] when that happened).  A caller that has tested its streams hands one over here: it is used instead (for the
 * calling thread's current device) and stays the caller's -- simq_plan_destroy does not destroy it.  NULL: back to the plan's own stream. */
int simq_plan_adopt_side_stream(const simq_plan* plan, void* side_stream);

/* ---- gradient exchange between data-parallel ranks (replaces the reduce-add of nn.DataParallel, policies.py:39) --------------
 * One process per GPU; RCCL (librccl.so.1, bound at run time) over xGMI.  Rank 0 obtains a SIMQ_COMM_ID_BYTES identifier and
 * hands it to the other ranks out of band (the Python host: torch.distributed broadcast / a file); every rank then calls
 * simq_comm_init with its HIP device current.  The communicator owns one non-blocking stream: simq_comm_allreduce /
 * simq_comm_broadcast enqueue there, ordered behind everything already submitted to `producer_stream`, and return at once;
 * simq_comm_wait makes `consumer_stream` wait for every collective enqueued so far.  All ranks must issue the same sequence.
 * In-place sum of `count` elements (dtype SIMQ_COMM_F32 / SIMQ_COMM_F64); broadcast of raw bytes from rank `root`. */
#define SIMQ_COMM_ID_BYTES 128
#define SIMQ_COMM_F32 0
#define SIMQ_COMM_F64 1
typedef struct simq_comm simq_comm;
int simq_comm_unique_id(void* id_out /* SIMQ_COMM_ID_BYTES, host memory */);
int simq_comm_init(const void* id, int world_size, int rank, simq_comm** out);
/* Round 6: run the communicator's collectives on a stream of the CALLER's instead of the communicator's own (NULL: back to its own).  The
 * point is the hardware queue (see simq_train_args.third_stream): a gradient bucket must travel beside the backward pass, so its stream may
 * share a queue neither with the launch stream nor with the side stream of the weight gradients -- the Python host hands over the learner's
 * third stream, idle from the end of the forward phase to the next step.  Synchronises the stream in use so far (the collectives of one
 * communicator stay ordered); every rank must adopt at the same point of its sequence of collectives. */
int simq_comm_adopt_stream(simq_comm* comm, void* stream);
int simq_comm_world_size(const simq_comm* comm);
int simq_comm_rank(const simq_comm* comm);
int simq_comm_allreduce(simq_comm* comm, void* d_buf, int64_t count, int dtype, void* producer_stream);
int simq_comm_broadcast(simq_comm* comm, void* d_buf, int64_t bytes, int root, void* producer_stream);
int simq_comm_wait(simq_comm* comm, void* consumer_stream);
/* Hang diagnosis (no reference counterpart: nn.DataParallel lives in one process): out = {collectives enqueued by this rank,
 * collectives the device has completed (event queries, no synchronisation), kind of the last one (0 all-reduce fp32, 1 all-reduce fp64,
 * 2 broadcast), its element / byte count}.  Safe to call from a watchdog thread while another thread waits on the device. */
int simq_comm_progress(simq_comm* comm, int64_t out[4]);
/* Exposed communication time (no reference counterpart: measurement aid of the data-parallel step).  With timing on, every simq_comm_wait
 * brackets the consumer stream's wait with a pair of timing events; simq_comm_last_wait_ms blocks until the LAST wait has been passed and
 * returns how long the consumer stream stood waiting for collectives still in flight -- inside simq_train_step that is the un-overlapped
 * part of the second gradient bucket (bucket 1 travels beside backward phase 2, the loss scalars beside the whole backward pass).  ~0 when everything was hidden. */
int simq_comm_time_waits(simq_comm* comm, int on);
int simq_comm_last_wait_ms(simq_comm* comm, float* ms);
int simq_comm_destroy(simq_comm* comm);

/* ---- intention-prediction head (train_intention, train.py:143-158; step_intention, policies.py:97-117) ----------
 * simq_bce_with_logits: nn.BCEWithLogitsLoss() ('mean') over n logits vs targets; *d_loss_sum (double) receives the SUM
 *   (host divides by n), d_dlogits (may be NULL) the gradient (sigmoid(x) - t) / n.
 * simq_split_last_channel: x [pixels][C] -> s[:, :, :-1] as [pixels][C-1] and s[:, :, -1] as [pixels].
 * simq_sigmoid_concat: out [pixels][Cs+1] = concat(state [pixels][Cs], sigmoid(logit [pixels])); d_prob (may be NULL)
 *   also receives the sigmoid map.                                                                               */
int simq_bce_with_logits(const float* d_logits, const float* d_target, int64_t n, float* d_dlogits, double* d_loss_sum, void* stream);
int simq_split_last_channel(const float* d_x, float* d_head, float* d_last, int64_t pixels, int channels, void* stream);
int simq_sigmoid_concat(const float* d_state, const float* d_logit, float* d_out, float* d_prob, int64_t pixels, int channels, void* stream);

/* ---- the same three over typed states: bf16 replay pools end to end --------------------------------------------------------
 * Element types are flags: 0 fp32, 1 bf16.  fp32 arrays 4-byte, bf16 arrays 2-byte aligned; every array a call writes is disjoint from
 * every other array of the call (checked).  1 <= pixels <= 2^30.  Where every array of a call is 16-byte aligned, whole tiles of 256
 * pixels move as 16-byte vectors on both sides (256 * C elements are a whole number of them for every C); the last partial tile, and
 * everything when some array is not 16-byte aligned or a tile exceeds 64 KB, moves element by element -- same values either way.
 * simq_intention_split: d_state [pixels][channels] -> d_head [pixels][channels-1] and d_last [pixels] fp32 (may be NULL), 2 <= channels <=
 *   4096.  Same type: bits are moved (NaN payloads kept); fp32 -> bf16: simq_states_to_bf16's conversion; bf16 -> fp32 (and d_last of a bf16
 *   state): the exact widening.
 * simq_bce_with_logits_state: simq_bce_with_logits with the target read IN PLACE from the last channel of d_state (d_state[p * channels +
 *   channels - 1], a bf16 state widened exactly): the same terms and the same gradient expression, element for element.  The loss sum is
 *   reproducible: per-block fp64 partial sums go to d_scratch (simq_bce_state_scratch_bytes() bytes, 8-byte aligned) and a second small
 *   launch adds them in block order -- no atomics.
 * simq_sigmoid_concat_x: simq_sigmoid_concat with the element types of d_state [pixels][channels] and d_out [pixels][channels+1] chosen
 *   independently; a bf16 d_out receives the sigmoid rounded as simq_states_to_bf16 rounds (what the Q-network's first convolution would do
 *   to the fp32 value); d_prob (may be NULL) stays fp32.  1 <= channels <= 4095. */
int simq_intention_split(const void* d_state, int state_bf16, void* d_head, int head_bf16, float* d_last, int64_t pixels, int channels, void* stream);
int64_t simq_bce_state_scratch_bytes(void);
int simq_bce_with_logits_state(const float* d_logits, const void* d_state, int state_bf16, int64_t pixels, int channels, float* d_dlogits,
                               double* d_loss_sum, void* d_scratch, void* stream);
int simq_sigmoid_concat_x(const void* d_state, int state_bf16, const float* d_logit, void* d_out, int out_bf16, float* d_prob, int64_t pixels,
                          int channels, void* stream);

/* ---- the whole intention supervision step in one call (reference train.train_intention, train.py:143-158, lines 145-153) ----------------
 * On `stream`, sequenced by the library as simq_train_step is: simq_intention_split of `state` into `head` (in the element type the plan
 * reads: bf16 with simq_plan_options.bf16_states, else fp32; a bf16 `state` for a plan without the option is widened by the split) and,
 * when `target` is given, the ground-truth map into it; train-mode forward that convolves `head` in place (no copy into the workspace);
 * simq_bce_with_logits_state on `state`; copy of *loss_sum to loss_host; backward from the dense `dlogits` with `head` as the first
 * convolution's input, weight gradients on `side_stream` when one is given; momentum SGD without clipping; refresh of the weight cache.
 * The plan has one output channel and channels - 1 input channels; 1 <= batch <= 4096; the weight cache must be current on entry.
 * `state` and `head` are read until the END of the call's stream work.  *loss_sum is the SUM of the batch * 96 * 96 terms (the host divides).
 * There is no `comm` field: data-parallel intention steps keep the separate calls (simq.learner.train_intention_step without `fused`). */
typedef struct simq_intention_args {
    const simq_plan* plan;
    int struct_bytes;            /* sizeof(simq_intention_args) of the caller's header: checked, a struct of another version is refused */
    int batch, channels;         /* channels: of `state` (the plan reads channels - 1) */
    int state_bf16;              /* element type of `state`: 0 fp32, 1 bf16 */
    int first_step;              /* 1: the momentum buffer is initialised by this step */
    float lr, momentum, weight_decay;
    float* params; void* wcache; float* bnbuf; float* grads; float* momentum_buf; void* ws_train;
    const void* state;           /* [batch][96][96][channels] */
    void* head;                  /* [batch][96][96][channels-1] in the plan's state type: written, then convolved in place */
    float* logits; float* dlogits;   /* [batch][96][96] */
    float* target;               /* NULL, or [batch][96][96] fp32: receives the ground-truth map (the last channel of `state`) */
    double* loss_sum; void* bce_scratch;   /* one double; simq_bce_state_scratch_bytes() bytes */
    void* opt_scratch; float* total_norm;  /* as simq_train_args (total_norm may be NULL) */
    double* loss_host;           /* NULL, or one double of PINNED host memory: *loss_sum is copied there on the plan's copy stream right behind
                                  * the BCE launch; the host calls simq_train_loss_wait(plan) instead of synchronising the stream.  The wait is
                                  * per plan: an intention net has its own, a TD step's pending copy is not disturbed. */
    void* stream; void* side_stream;
} simq_intention_args;
int simq_train_intention_step(const simq_intention_args* a);

/* layout helpers for callers that hold NCHW tensors (apply_transform, policies.py:44-45) */
int simq_nchw_to_nhwc(const float* d_in, float* d_out, int batch, int channels, int hw, void* stream);
int simq_nhwc_to_nchw(const float* d_in, float* d_out, int batch, int channels, int hw, void* stream);

/* ---- single-op entry points (unit-test surface; same kernels the plan launches) -------------
 * The convolution operators end in `const simq_launch_opts* opts` (NULL = what a default plan launches): kernel selection and block
 * scheduling of THAT call -- the per-kernel parity tests force every tile of a launcher's menu through it (tests/test_gpu_ops.py),
 * tools/ run their A/Bs through it.  The library keeps no process-global switch of any kind. */
typedef struct simq_launch_opts {
    int struct_bytes;             /* sizeof(simq_launch_opts), checked */
    int force_bm, force_bn;       /* 0 / 0: the launcher's own rule; otherwise the block tile BM x BN of the launcher's menu (a tile the shape does
                                   * not admit falls back to the rule) */
    int tail_split;               /* as simq_plan_options.tail_split */
    int plane_xcd;                /* as simq_plan_options.plane_xcd (1) */
    int wgrad_xcd_group;          /* as simq_plan_options.wgrad_xcd_group (1) */
    int wgrad_ksplit;             /* as simq_plan_options.wgrad_ksplit (0) */
    int gemm_split;               /* as simq_plan_options.gemm_split (0) */
} simq_launch_opts;
void simq_launch_opts_default(simq_launch_opts* opts);
int simq_conv2d_fwd(const float* d_x, const float* d_w_ohwi, const float* d_bias, float* d_y,
                    int batch, int hin, int win, int cin, int cout, int r, int s, int stride, int pad,
                    double* d_stats /* NULL or [2*cout] zeroed */, void* stream, const simq_launch_opts* opts);
/* The same 3x3 / stride-1 / pad-1 convolution through the Winograd F(2x2,3x3) path (conv_winograd.hip: input transform,
 * 16 batched transform-domain GEMMs, output transform + epilogue), as the plan uses it for the 512-channel layers.
 * Requirements: hin, win even; cin % 16 == 0; cout % 64 == 0; cin / 4 and cout / 4 divide 256.
 * d_scratch: 16*cout*cin + 16*T*(cin+cout) floats, T = batch*(hin/2)*(win/2) (transformed weights | V | Mt). */
int simq_conv2d_fwd_winograd(const float* d_x, const float* d_w_ohwi, const float* d_bias, float* d_y,
                             int batch, int hin, int win, int cin, int cout,
                             double* d_stats /* NULL or [2*cout] zeroed */, float* d_scratch, void* stream, const simq_launch_opts* opts);
/* The same convolution in Winograd F(4x4,3x3) form (36 transform-domain GEMMs over a quarter of the tiles; interpolation points
 * {0, 1, -1, 1/2, -2, inf}): the form the plan uses for forwards nothing is differentiated through (target net, double-DQN argmax
 * forward, policy.step).  hin, win multiples of 4.  d_scratch: 36*cout*cin + 36*T4*(cin+cout) floats, T4 = batch*(hin/4)*(win/4). */
int simq_conv2d_fwd_winograd4(const float* d_x, const float* d_w_ohwi, const float* d_bias, float* d_y,
                              int batch, int hin, int win, int cin, int cout,
                              double* d_stats /* NULL or [2*cout] zeroed */, float* d_scratch, void* stream, const simq_launch_opts* opts);
/* The OUTPUT TRANSFORM of that form on its own (per-kernel tests, tools/): y = A^T m A per 4x4 output tile from the transform-domain
 * products d_mt [36][T4][channels], T4 = batch*(h/4)*(w/4), followed by the whole convolution epilogue, every part optional (NULL / 0):
 *   v = y + bias[n] ; (stats[n] += v, stats[channels+n] += v*v) ; v = v*scale[n] + shift[n] ; v += addend[pixel][n] ; relu ; store ;
 *   with bnr_red1 (a dgrad's fused BatchNorm-backward sums):  dz = mask > 0 ? v : 0, the mask being bnr_mask (fp32), else bnr_mask16
 *   (bf16 bits), else recomputed as bnr_y1*bnr_mscale[n] + bnr_mshift[n] > 0 ;  bnr_red1[n] += dz,
 *   bnr_red1[channels+n] += dz*(bnr_y1 - bnr_mean1[n])*bnr_invstd1[n] ; and the same against (bnr_y2, bnr_mean2, bnr_invstd2) into bnr_red2.
 * Activation-shaped tensors are fp32 [batch][h][w][channels]; the fp64 sums [2*channels] are added into (zero them first).
 * form 1: the two-phase kernel the plans launch (a tile's epilogue loads issued back to back, then its arithmetic, then its stores);
 * form 0: the one-pixel-at-a-time kernel it replaced, kept as the oracle -- same operations in the same order, bit-identical y and,
 * on data whose fp64 sums are exact, bit-identical sums.  h, w multiples of 4; channels / 4 divides 256. */
typedef struct simq_wino4f_epilogue {
    int struct_bytes;               /* sizeof(simq_wino4f_epilogue): a struct of another version is refused */
    int relu;
    const float* bias; double* stats; const float* scale; const float* shift; const float* addend;
    const float* bnr_mask; const uint16_t* bnr_mask16; const float* bnr_mscale; const float* bnr_mshift;
    const float* bnr_y1; const float* bnr_mean1; const float* bnr_invstd1; double* bnr_red1;
    const float* bnr_y2; const float* bnr_mean2; const float* bnr_invstd2; double* bnr_red2;
} simq_wino4f_epilogue;
int simq_wino4f_output(const float* d_mt, float* d_y, int batch, int h, int w, int channels, const simq_wino4f_epilogue* epilogue,
                       int form, void* stream);
/* The plan's elementwise BatchNorm pass, on its own (per-kernel parity tests): train-mode nn.BatchNorm2d + residual + ReLU
 * (resnet.py:35-36,42-45) with the batch statistics GIVEN as [sum | sum of squares] over `rows` (what the producing convolution's
 * epilogue leaves):  out = [relu]( (y - mean) * invstd * gamma + beta  [+ res] ).
 * storage 0: y / res / out fp32 [rows][channels];  1: all three bf16 (the all-bf16 form of plain-bf16 plans: 16-byte accesses).
 * d_saved [4*channels]: scale | shift | mean | invstd (written);  d_running [2*channels]: running mean | var (momentum 0.1, updated). */
int simq_bn_relu_apply(const void* d_y, const double* d_stats, const float* d_gamma, const float* d_beta, const void* d_res, int relu,
                       void* d_out, int64_t rows, int channels, int storage, float* d_saved, float* d_running, void* stream);
/* ... and its backward:  dz = g * mask,  dy = gamma * invstd * (dz - sum(dz)/rows - xhat * sum(dz*xhat)/rows),  dgamma = sum(dz*xhat),
 * dbeta = sum(dz), with the two sums GIVEN in d_red [2*channels] (in the plan they come from the dgrad epilogue that produced g).
 * mask_kind 0: no mask; 1: d_mask = the activation that followed (fp32 or bf16 per `storage`), mask = activation > 0;
 * 2: recomputed from the pre-BN output, mask = (y * scale + shift > 0) with d_saved's scale | shift (simq_plan_options.fuse_bn1_apply /
 * bn1_mask_from_preact).  d_saved as written by simq_bn_relu_apply.  d_dz_out: NULL or the masked gradient (same storage as g). */
int simq_bn_relu_backward(const void* d_g, const void* d_mask, int mask_kind, const void* d_y, const float* d_saved, const float* d_gamma,
                          const double* d_red, void* d_dy, void* d_dz_out, float* d_dgamma, float* d_dbeta, int64_t rows, int channels,
                          int storage, void* stream);
/* conv( relu( y_pre * in_scale[ci] + in_shift[ci] ) ): the second convolution of a train-mode "conv -> BatchNorm -> ReLU -> conv" chain
 * (reference resnet.py:34-40, networks.py:18-20) consuming the FIRST convolution's pre-BatchNorm output -- the BatchNorm + ReLU in
 * between is applied while the operand is staged and the activation is never stored (simq_plan_options.fuse_bn1_apply; fp32).
 * Zero padding applies to the activation.  form 0: implicit GEMM / image tile (any r x s, cin % 16 == 0); 1: Winograd F(2x2,3x3);
 * 2: Winograd F(4x4,3x3) (3x3 / stride 1 / pad 1 geometries of simq_conv2d_fwd_winograd / _winograd4, same d_scratch; NULL for form 0). */
int simq_conv2d_fwd_bnrelu_in(const float* d_y_pre, const float* d_in_scale, const float* d_in_shift, const float* d_w_ohwi,
                              const float* d_bias, float* d_y, int batch, int hin, int win, int cin, int cout, int r, int s, int stride,
                              int pad, int form, float* d_scratch, void* stream, const simq_launch_opts* opts);
/* ... and that convolution's weight gradient, dW = dY^T * relu(y_pre * in_scale + in_shift) (the activation recomputed on load).
 * form 0: direct (cin % 64 == 0); 1: transform domain (geometry / d_scratch of simq_conv2d_wgrad_winograd). */
int simq_conv2d_wgrad_bnrelu_in(const float* d_y_pre, const float* d_in_scale, const float* d_in_shift, const float* d_dy, float* d_dw,
                                int batch, int hin, int win, int cin, int cout, int r, int s, int stride, int pad, int form,
                                float* d_scratch, void* stream, const simq_launch_opts* opts);
/* The encoder's first convolution (reference resnet.py:94: 7x7, stride 2, pad 3, cin -> 64, no bias) on the bf16 matrix cores with
 * the operands gathered straight from the fp32 NHWC input -- the form plain-bf16 plans use (stem_conv_bf16.hip).  7 * cin <= 63 (the
 * *_wide entries below take 64 <= 7 * cin <= 95),
 * win a multiple of 32, hin even.  d_y: bf16 [batch][hin/2][win/2][64] (pre-BatchNorm, rounded once from the fp32 accumulators);
 * d_stats: NULL or [2*64] zeroed (sum | sum of squares of the UNROUNDED outputs); d_scratch: 58 368 bytes (bf16 weight layout). */
/* ... and in exact fp32 (v_mfma_f32_16x16x4_f32 fed by 16-byte runs of the NHWC input; what fp32 / split-bf16 plans run): 7 * cin <= 64,
 * win a multiple of 32, hin even.  d_y: fp32 [batch][hin/2][win/2][64]; d_stats: NULL or [2*64] zeroed (sum | sum of squares). */
int simq_conv2d_fwd_stem_f32(const float* d_x, const float* d_w_ohwi, float* d_y, int batch, int hin, int win, int cin, double* d_stats,
                             void* stream);
int simq_conv2d_fwd_stem_bf16(const float* d_x, const float* d_w_ohwi, uint16_t* d_y, int batch, int hin, int win, int cin,
                              double* d_stats, void* d_scratch, void* stream);
/* Weight gradient of that convolution from the bf16 plane of dy (bf16 [batch][hin/2][win/2][64]): both operands staged transposed in
 * LDS, contraction over pixels on the bf16 matrix cores, per-block partial sums added in a fixed order (deterministic).
 * d_dw: [64][7][7][cin] fp32, overwritten.  d_scratch: min(512, ceil(batch * hin/2 * win/32 / 16)) * 64 * 49 * cin floats. */
int simq_conv2d_wgrad_stem_bf16(const float* d_x, const uint16_t* d_dy, float* d_dw, int batch, int hin, int win, int cin,
                                float* d_scratch, void* stream);
/* The same two operators over bf16 states -- d_x [batch][hin][win][cin] bf16, 2-byte aligned -- as a plan with
 * simq_plan_options.bf16_states = 1 launches them: the same kernels with the element type of x as a template parameter, a lane's
 * fragment one 16-byte load that assumes 2-byte alignment, the bf16 bits handed to the matrix core as they lie in memory.  Every other
 * argument, the scratch sizes and the results' layout as above; on d_x = RNE(x) they return what the fp32-input operators return on x. */
int simq_conv2d_fwd_stem_bf16_x16(const uint16_t* d_x, const float* d_w_ohwi, uint16_t* d_y, int batch, int hin, int win, int cin,
                                  double* d_stats, void* d_scratch, void* stream);
int simq_conv2d_wgrad_stem_bf16_x16(const uint16_t* d_x, const uint16_t* d_dy, float* d_dw, int batch, int hin, int win, int cin,
                                    float* d_scratch, void* stream);
/* The wide-row forms of the four operators above: 64 <= 7 * cin <= 95 (cin 10..13), the same kernels with three k-steps of the matrix
 * core per filter row instead of two -- what a plain-bf16 plan with simq_plan_options.stem_bf16 = 2 launches for such an input (the
 * narrow entries keep refusing cin >= 10, these refuse everything else).  Arguments, results and their layout as above, except
 * d_scratch of the forward: simq_conv2d_fwd_stem_bf16_wide_scratch_bytes() bytes (87 040: bf16 weight rows of 7 * 96 + 8), and
 * d_scratch of the weight gradient: simq_conv2d_wgrad_stem_bf16_slabs(batch, hin, win, cin, -1) * 64 * 49 * cin floats. */
int64_t simq_conv2d_fwd_stem_bf16_wide_scratch_bytes(void);
int simq_conv2d_fwd_stem_bf16_wide(const float* d_x, const float* d_w_ohwi, uint16_t* d_y, int batch, int hin, int win, int cin,
                                   double* d_stats, void* d_scratch, void* stream);
int simq_conv2d_wgrad_stem_bf16_wide(const float* d_x, const uint16_t* d_dy, float* d_dw, int batch, int hin, int win, int cin,
                                     float* d_scratch, void* stream);
int simq_conv2d_fwd_stem_bf16_wide_x16(const uint16_t* d_x, const float* d_w_ohwi, uint16_t* d_y, int batch, int hin, int win, int cin,
                                       double* d_stats, void* d_scratch, void* stream);
int simq_conv2d_wgrad_stem_bf16_wide_x16(const uint16_t* d_x, const uint16_t* d_dy, float* d_dw, int batch, int hin, int win, int cin,
                                         float* d_scratch, void* stream);
/* Partial-sum slabs (64 * 49 * cin floats each) the stem weight gradient, narrow or wide, uses for this batch when its scratch holds
 * capacity_bytes: min(what the batch asks for -- the formula at simq_conv2d_wgrad_stem_bf16 --, capacity_bytes / slab bytes); 0 when not
 * even one slab fits (the launch then refuses), capacity_bytes < 0: no limit, which is what the eight standalone entries assume of
 * d_scratch.  (The blocks are persistent, so any count >= 1 covers the batch.  A plan keeps the slabs in a dead workspace slot of
 * batch * 1 179 648 bytes: that holds the 9 * batch slabs asked for up to cin = 10 and fewer beyond.)  -1 on a bad argument. */
int simq_conv2d_wgrad_stem_bf16_slabs(int batch, int hin, int win, int cin, int64_t capacity_bytes);
/* Weight gradient of the same convolution through the transform domain (dy / x transforms, 16 batched contractions over
 * the tiles, G^T dU G).  Additionally cin % 128 == 0 and cout % 128 == 0.  d_dw is overwritten.
 * the tiles, G^T dU G); uses F(4x4,3x3) when hin, win are multiples of 4 and batch*(hin/4)*(win/4) is a multiple of 16.
 * d_scratch: 16*T*(cin+cout) + 36*cout*cin floats. */
int simq_conv2d_wgrad_winograd(const float* d_x, const float* d_dy, float* d_dw_ohwi,
                               int batch, int hin, int win, int cin, int cout, float* d_scratch, void* stream, const simq_launch_opts* opts);
/* `batch` independent row-major GEMMs y_g[m][n] = x_g[m][k] * w_g[n][k]^T in exact fp32 (v_mfma_f32_16x16x4_f32), g-th operands at
 * base + g * rows * cols: the transform-domain contraction of a Winograd layer (16 or 36 transform elements; what cuDNN's Winograd
 * kernels do inside nn.Conv2d, reference resnet.py:14-16 under train.py:23) -- the dominant kernel of the fp32 step, on its own for the
 * per-kernel tests and probes.  k % 16 == 0, n % 64 == 0. */
int simq_gemm_f32_batched(const float* d_x, const float* d_w, float* d_y, int m, int n, int k, int batch, void* stream,
                          const simq_launch_opts* opts);
int simq_conv2d_dgrad(const float* d_dy, const float* d_w_ohwi, float* d_wt_scratch, float* d_dx,
                      int batch, int hin, int win, int cin, int cout, int r, int s, int pad, void* stream, const simq_launch_opts* opts);
int simq_conv2d_wgrad(const float* d_x, const float* d_dy, float* d_dw_ohwi /* zeroed by callee */,
                      int batch, int hin, int win, int cin, int cout, int r, int s, int stride, int pad,
                      void* stream, const simq_launch_opts* opts);
/* bf16 matrix-core variants: the fp32 inputs are split into bf16 planes in d_scratch first
 * (nplanes 1: plain bf16; 2: split-bf16 hi/lo, 3 MFMA products).  d_scratch: 2*(|x|+|w|) resp. 2*(|x|+|dy|) uint16. */
int simq_conv2d_fwd_bf16(const float* d_x, const float* d_w_ohwi, const float* d_bias, float* d_y, int batch, int hin, int win,
                         int cin, int cout, int r, int s, int stride, int pad, int nplanes, void* d_scratch, double* d_stats,
                         void* stream, const simq_launch_opts* opts);
int simq_conv2d_wgrad_bf16(const float* d_x, const float* d_dy, float* d_dw_ohwi, int batch, int hin, int win, int cin, int cout,
                           int r, int s, int stride, int pad, int nplanes, void* d_scratch, void* stream, const simq_launch_opts* opts);
/* (the weight-gradient half of loss.backward(), train.py:132, of one nn.Conv2d.)  The same with d_slab =
 * simq_conv2d_wgrad_bf16_slab_bytes() of scratch: the image-tile weight-gradient kernel (3x3 on 24x24 maps, Cout %
 * 256 == 0, Cin % 32 == 0, >= 2 images per block) then leaves per-block partial tiles there and a second launch adds them in a fixed
 * order (deterministic) instead of fp32 atomics -- the form the plans use.  d_slab = NULL: as simq_conv2d_wgrad_bf16. */
int64_t simq_conv2d_wgrad_bf16_slab_bytes(void);
int simq_conv2d_wgrad_bf16_slab(const float* d_x, const float* d_dy, float* d_dw_ohwi, int batch, int hin, int win, int cin, int cout,
                                int r, int s, int stride, int pad, int nplanes, void* d_scratch, void* d_slab, void* stream, const simq_launch_opts* opts);
/* The second launch of the deterministic weight gradients on its own: d_dw[e] = ((d_slab[0][e] + d_slab[1][e]) + d_slab[2][e]) + ... in
 * fp32, d_slab = [splits][n] floats, d_dw = n floats, overwritten.  No alignment beyond a float's is required of either pointer. */
int simq_wgrad_slab_sum(const float* d_slab, float* d_dw, int64_t n, int splits, void* stream);
int simq_upsample2x_fwd(const float* d_in, float* d_out, int batch, int h, int w, int c, void* stream);
int simq_upsample2x_bwd(const float* d_dout, float* d_din, int batch, int h, int w, int c, void* stream);

/* ---- shortest-path distance images (shortest_paths.pyx:26-114 GridGraph._spfa, and the Mapper maps of envs.py:2287-2300,
 * 2513-2516) --------------------------------------------------------------------------------------------------------------------
 * One problem = one 8-connected grid [rows][cols] of uint8 (free where != 0) and one source pixel.  An edge joins two free cells
 * inside the grid; straight edges weigh 1, diagonal ones float32(sqrt 2).  The source gets 0 even when blocked (then nothing else is
 * reachable); unreachable cells get -1.  Every update is fl32(d[u] + w) accepted when strictly smaller, iterated to the fixed point,
 * so the distances equal the reference SPFA's bit for bit (SPFA's parents, which depend on its queue order, come from
 * simq_grid_paths below, which emulates the search itself).
 * Optional epilogue, in the reference's order: img = d / pixels_per_meter (fp32 division; 1 = none); unreachable_to_max != 0:
 * img[img < 0] = img.max(); img *= scale (1 = none).
 * `problems`: host array of n descriptors, validated here (rows, cols >= 1, rows * cols < 2^22, source inside the grid, the grid
 * inside the grids_bytes of d_grids, the image inside the out_floats of d_out, no two images overlapping; several problems may
 * share one grid) and copied to the caller's device buffer d_problems (n descriptors) on `stream`.  d_status[n] (int32): 0 =
 * converged, 1 = the cap of rows * cols + 1 passes was hit (the image is then not the fixed point; cannot happen by the bound
 * above), 2 = bad descriptor (the kernel checks again and writes nothing else). */
typedef struct simq_grid_problem {
    int64_t grid_offset;        /* byte offset of the problem's [rows][cols] uint8 grid in d_grids */
    int64_t out_offset;         /* float offset of its [rows][cols] fp32 image in d_out */
    int32_t rows, cols;
    int32_t src_i, src_j;
} simq_grid_problem;
#define SIMQ_GRID_MAX_CELLS (1 << 22)
int simq_grid_distance_images(const uint8_t* d_grids, int64_t grids_bytes, const simq_grid_problem* problems, int n,
                              simq_grid_problem* d_problems, float* d_out, int64_t out_floats, float pixels_per_meter,
                              int unreachable_to_max, float scale, int32_t* d_status, void* stream);

/* The same images with the snap of OccupancyMap.shortest_path_image (envs.py:2513-2516, 2522-2523) on the device: the source of a
 * problem is replaced by closest[:, src_i, src_j] before the search -- int32 [2][rows][cols] at d_closest + closest_offset, the layout
 * simq_occupancy_maps writes and simq_grid_paths / simq_grid_distance_queries read -- so that a chain occupancy maps -> distance
 * images needs no pixel on the host.  The search and the epilogue are those of simq_grid_distance_images, bit for bit.
 * Upstream status: d_upstream (n_upstream int32 words on the device, e.g. the d_status simq_occupancy_maps wrote; NULL with
 * n_upstream == 0) is read by the kernel, never by the host.  A problem with upstream >= 0 whose word d_upstream[upstream] is nonzero
 * is not searched and its closest block is not read (the closest cells of a configuration space without a free cell are undefined):
 * d_status[p] becomes that word as it is and every cell of the image SIMQ_GRID_SNAPPED_FILL.  The caller, who owns d_upstream, tells
 * a passed-on word from the codes below by looking at both arrays.
 * `problems`: host array of n descriptors, validated here before anything is copied or launched (rows, cols >= 1, rows * cols <
 * SIMQ_GRID_MAX_CELLS; the source as given inside the grid; grid, closest block and image inside the declared extent of their
 * buffers; upstream -1 or below n_upstream; no two images overlapping; nothing the launch writes -- d_out, d_status, d_problems --
 * sharing a byte with any other buffer of the call; 4-byte alignment of d_closest, d_out, d_upstream and d_status, 8 of d_problems) and
 * copied to d_problems (n descriptors) on `stream`.  Several problems may share a grid and a closest block.  d_status[n] (int32): 0 =
 * converged, 1 = the cap of passes was hit (cannot happen, as above), 2 = bad descriptor (the kernel checks again and writes nothing
 * else), 3 = the snapped pixel lies outside the grid or on a cell that is not free: nothing is searched, the image is filled with
 * SIMQ_GRID_SNAPPED_FILL and every other problem of the call is unaffected; or the upstream word. */
typedef struct simq_grid_snapped_problem {
    int64_t grid_offset;        /* byte offset of the problem's [rows][cols] uint8 grid in d_grids */
    int64_t closest_offset;     /* int32 offset of its [2][rows][cols] closest cells in d_closest */
    int64_t out_offset;         /* float offset of its [rows][cols] fp32 image in d_out */
    int32_t rows, cols;
    int32_t src_i, src_j;       /* the pixel before the snap */
    int32_t upstream;           /* index of its word in d_upstream, or -1 */
    int32_t reserved_;
} simq_grid_snapped_problem;
#define SIMQ_GRID_SNAPPED_FILL 0.0f
int simq_grid_distance_images_snapped(const uint8_t* d_grids, int64_t grids_bytes, const int32_t* d_closest, int64_t closest_ints,
                                      const simq_grid_snapped_problem* problems, int n, simq_grid_snapped_problem* d_problems,
                                      float* d_out, int64_t out_floats, float pixels_per_meter, int unreachable_to_max, float scale,
                                      const int32_t* d_upstream, int n_upstream, int32_t* d_status, void* stream);

/* ---- shortest-path waypoints: SPFA's parents and the dense path (shortest_paths.pyx:69-137 GridGraph._spfa and the walk of
 * GridGraph.shortest_path; the front half of OccupancyMap.shortest_path, envs.py:2477-2490) --------------------------------------
 * One problem = one grid [rows][cols] of uint8 (free where != 0), a source pixel and a target pixel; one wavefront emulates the
 * reference's search exactly, problems are the parallel axis, every problem of a call in one launch.  The rules that decide the
 * parents (they depend on the order of the queue, unlike the distances):
 *   edges       leave a free cell u only (a blocked source relaxes nothing) and go to the free neighbours inside the grid in the order
 *               (di, dj) = (0,-1) (0,1) (-1,-1) (-1,0) (-1,1) (1,-1) (1,0) (1,1): direction codes 0 .. 7; weights 1 and float32(sqrt 2)
 *   relaxation  new = fl32(d[u] + w) is accepted when strictly smaller than d[v]; the parent of v becomes u on every acceptance;
 *               d starts at inf = float32(2 * rows * cols) of the full grid, the source at 0
 *   queue       first in, first out, slots numbered from 1 (head = 0, the source in slot tail = 1); a pop takes slot ++head.  An
 *               accepted v that is not queued goes to slot ++tail; a queued one is not moved.  After each push the two slots tail
 *               and head + 1 are exchanged when d[queue[tail]] < d[queue[head + 1]] (strict; the same slot when the pushed vertex
 *               is the only one queued)
 *   order       the eight relaxations of one pop are sequential: the push at edge k compares against the front's distance as it
 *               stands after edges <= k of that pop (the front may be a neighbour of u that a later edge lowers)
 * The walk starts at the target and follows the parents until it meets the source or a cell without parent.  Outputs per problem:
 *   dense path  int32 (i, j) pairs, target first, at pair path_offset of d_paths, at most path_capacity pairs; its length in
 *               d_lengths[p].  Length 1 (the target alone) for an unreachable target, a blocked source and target == source.
 *   parents     (parents_offset >= 0) int32 [rows][cols] at d_parents + parents_offset: the ravelled index i * cols + j of the parent
 *               in the full grid, -1 where none
 *   distances   (dist_offset >= 0) fp32 [rows][cols] at d_dist + dist_offset, -1 where unreachable, 0 at the source even when it is
 *               blocked: what simq_grid_distance_images writes without its epilogue
 *   end pixels  d_endpoints[4 p .. 4 p + 4): the source and target the search used (after the snap below)
 * Two optional front stages, those of OccupancyMap.shortest_path:
 *   thin_offset >= 0     the skimage.draw.line from the source to the target as given (the rule of simq_intention_maps above) is
 *                        read from the problem's second uint8 map in d_grids; when every cell on it is 1 (the reference's
 *                        (1 - cspace_thin[rr, cc]).sum() == 0 in uint8 arithmetic), the problem ends with status 1 and length 0:
 *                        no search, no path, no image; the end pixels hold the pair as given
 *   closest_offset >= 0  source and target are replaced by closest[:, i, j] before the search: int32 [2][rows][cols] at d_closest +
 *                        closest_offset, the layout simq_occupancy_maps writes.  The line above is tested on the pixels as given.
 * The search state lives in LDS over a window of the grid that the caller declares: rows [box_i0, box_i0 + box_rows), columns
 * [box_j0, box_j0 + box_cols), which must hold every free cell (empty when there is none).  The window plus a blocked one-cell halo
 * has (box_rows + 2) * (box_cols + 2) <= SIMQ_GRID_PATH_MAX_BOX_CELLS cells (8 bytes each of the 160 KiB); a Mapper room needs
 * 94 x 94, and simq_grid_paths_large below takes the windows over the cap.  The kernel reads the whole grid once and gives status 2
 * when a free cell lies outside the window.
 * `problems`: host array of n descriptors, validated here before anything is copied or launched (rows, cols >= 1, rows * cols <
 * SIMQ_GRID_MAX_CELLS; source and target inside the grid; the window inside the grid and under the cap; path_capacity >= 1; every
 * input and output inside the declared extent of its buffer; no two problems' outputs overlapping; the output buffers, d_lengths,
 * d_endpoints, d_status and d_problems disjoint from each other and from the inputs; 4-byte alignment of the int32 / fp32 buffers, 8
 * of d_problems) and copied to the caller's device buffer d_problems (n descriptors) on `stream`.  Several problems may share a
 * grid.  d_closest, d_parents, d_dist may be NULL when no problem uses them.  d_status[n] (int32): 0 = path traced, 1 = straight line
 * clear, 2 = bad descriptor (the kernel checks again -- sizes, pixels, the snapped pixels, the window -- and writes nothing else),
 * 3 = path_capacity too small: d_lengths[p] holds the needed count, nothing is written past the capacity, the images are complete,
 * 4 = the search passed its cap of 64 * free cells + 64 pops (cannot happen: SPFA here pops each cell 1.0 - 1.1 times). */
typedef struct simq_grid_path_problem {
    int64_t grid_offset;        /* byte offset of the problem's [rows][cols] uint8 grid in d_grids */
    int64_t thin_offset;        /* byte offset of its [rows][cols] uint8 thin map in d_grids, or -1 */
    int64_t closest_offset;     /* int32 offset of its [2][rows][cols] closest cells in d_closest, or -1 */
    int64_t path_offset;        /* pair offset of its dense path in d_paths (int32 offset 2 * path_offset) */
    int64_t parents_offset;     /* int32 offset of its [rows][cols] parent image in d_parents, or -1 */
    int64_t dist_offset;        /* float offset of its [rows][cols] distance image in d_dist, or -1 */
    int32_t path_capacity;      /* pairs */
    int32_t rows, cols;
    int32_t src_i, src_j, tgt_i, tgt_j;
    int32_t box_i0, box_j0, box_rows, box_cols;
    int32_t reserved_;
} simq_grid_path_problem;
#define SIMQ_GRID_PATH_MAX_BOX_CELLS 20000
int simq_grid_paths(const uint8_t* d_grids, int64_t grids_bytes, const int32_t* d_closest, int64_t closest_ints,
                    const simq_grid_path_problem* problems, int n, simq_grid_path_problem* d_problems, int32_t* d_paths,
                    int64_t path_pairs, int32_t* d_lengths, int32_t* d_endpoints, int32_t* d_parents, int64_t parents_ints, float* d_dist,
                    int64_t dist_floats, int32_t* d_status, void* stream);

/* The same search for windows of any size: the state lies in a workspace of the caller's in global memory instead of LDS, so
 * SIMQ_GRID_PATH_MAX_BOX_CELLS does not apply -- any window inside a grid of rows * cols < SIMQ_GRID_MAX_CELLS is taken, the empty one
 * and those under the cap included.  Rules, front stages, outputs, the kernel's re-check (status 2 for a free cell outside the window
 * included) and status words are those of simq_grid_paths: for a problem both entry points accept, every byte either writes is equal.
 * One wavefront per problem as there, and a pop costs a few times what it costs in LDS: this entry point is for the windows the
 * other refuses.
 * Workspace: d_work (work_bytes bytes, 16-byte aligned) is the caller's; the library allocates nothing.  Problem p's state is the
 * simq_grid_paths_large_work_bytes(box_rows, box_cols) bytes from byte work_offset (a multiple of 16) on: fp32 distances over the
 * window plus its halo, a ring of window cells + 1 uint32 entries, one parent byte and one flag byte per cell, in that order, the sum
 * rounded up to 16 (10 bytes a cell; 543 840 for a 232 x 232 window).  The kernel initialises what it reads; the content after the
 * call is unspecified.  simq_grid_paths_large_work_bytes is a host function of the two numbers alone (-1 for a negative side or
 * box_rows * box_cols >= SIMQ_GRID_MAX_CELLS).
 * Validation as for simq_grid_paths, without the cap, and in addition: d_work not NULL and 16-byte aligned; every problem's range
 * inside work_bytes at a non-negative multiple of 16; no two problems' ranges overlapping; d_work sharing no byte with any other
 * buffer of the call. */
typedef struct simq_grid_path_large_problem {
    int64_t grid_offset;        /* the fields of simq_grid_path_problem, with the same meaning ... */
    int64_t thin_offset;
    int64_t closest_offset;
    int64_t path_offset;
    int64_t parents_offset;
    int64_t dist_offset;
    int64_t work_offset;        /* ... and the byte offset of the problem's search state in d_work, a multiple of 16 */
    int32_t path_capacity;
    int32_t rows, cols;
    int32_t src_i, src_j, tgt_i, tgt_j;
    int32_t box_i0, box_j0, box_rows, box_cols;
    int32_t reserved_;
} simq_grid_path_large_problem;
int64_t simq_grid_paths_large_work_bytes(int32_t box_rows, int32_t box_cols);
int simq_grid_paths_large(const uint8_t* d_grids, int64_t grids_bytes, const int32_t* d_closest, int64_t closest_ints,
                          const simq_grid_path_large_problem* problems, int n, simq_grid_path_large_problem* d_problems,
                          int32_t* d_paths, int64_t path_pairs, int32_t* d_lengths, int32_t* d_endpoints, int32_t* d_parents,
                          int64_t parents_ints, float* d_dist, int64_t dist_floats, int32_t* d_status, void* d_work, int64_t work_bytes,
                          void* stream);

/* ---- waypoints from dense paths: exact simplification and pruning (shortest_paths.pyx:139-154, the back half of
 * GridGraph.shortest_path: skimage.measure.approximate_polygon, then the waypoints a clear line makes unnecessary) ---------------
 * One problem = one dense path c[0 .. n) of integer pixels (r, c), n >= 1, target first, where simq_grid_paths left it (problem p
 * reads pair path_offset of d_paths, d_lengths[p] and d_path_status[p]), its uint8 grid in d_grids and an integer tolerance t in
 * [1, 255] (the reference uses 1).  One wavefront per problem, every problem of a call in one launch on `stream`, so the search
 * and this stage queue back to back with no read-back between them.
 *
 * The rule.  approximate_polygon evaluates its comparisons in float64 through arctan2 / sin / cos, and on integer pixels those
 * comparisons meet exact ties whose outcome is rounding noise.  Every one of them is a comparison of rationals, decided here in
 * int64: the result equals the float algorithm wherever that does not depend on rounding, and is defined where it does.
 *   simplify  1. keep[0] = keep[n - 1] = true.
 *             2. A segment (s, e) with e > s + 1 is evaluated once, starting with (0, n - 1).
 *             3. With dr = r_e - r_s, dc = c_e - c_s, L = dr^2 + dc^2, every interior point k gets a squared distance as a fraction:
 *                a0 = (r_k - r_s) dr + (c_k - c_s) dc, a1 = -(r_k - r_e) dr - (c_k - c_e) dc; if a0 > 0 and a1 > 0 it is
 *                ((r_k - r_s) dc - (c_k - c_s) dr)^2 / L (perpendicular), otherwise min(|c_k - c_s|^2, |c_k - c_e|^2) / 1 (the
 *                nearer end point).
 *             4. m is the maximum, compared by cross-multiplication; the segment is split iff m > t^2 (strict).
 *             5. It is split at the first k that attains m: keep[k] = true, and (s, k) and (k, e) are evaluated in turn.
 *             6. A segment's verdict depends on its end points only, so the kept set does not depend on the order of evaluation (the
 *                kernel keeps no stack: it resolves the first unresolved gap between consecutive kept points).
 *   prune     sparse = the kept points in path order; path = [sparse[0]]; for k = 1 .. len(sparse) - 2, sparse[k] is kept iff the
 *             skimage.draw.line (the rule of simq_intention_maps below) from path[-1] to sparse[k + 1] crosses a cell of the grid
 *             that is not 1 (the reference's uint8 (1 - grid[rr, cc]).sum() > 0); sparse[-1] is appended when len(sparse) > 1.
 *   output    reversed: int32 (i, j) pairs, source first, at pair way_offset of d_ways, at most way_capacity pairs; d_counts[p].
 * Magnitudes.  Every coordinate must lie inside its grid, whose sides are at most 2^15, so |cross| < 2^31, cross^2 < 2^62,
 * L < 2^31, e^2 L < 2^62 and t^2 L < 2^47: all in int64.  Coordinates are data on the device, so it is the kernel that refuses
 * them (status 2); the host refuses rows or cols above 2^15.  A path of more than SIMQ_GRID_WAYPOINTS_MAX_PATH points is status 2
 * as well (the kept flags are a bit mask in LDS; simq_grid_paths writes at most SIMQ_GRID_PATH_MAX_BOX_CELLS + 1).
 * Work is bounded by n: at most n - 2 splits and n - 1 verdicts, at most n - 2 lines of at most max(rows, cols) cells.
 * `problems`: host array of n descriptors, validated here before anything is copied or launched (rows, cols in [1, 2^15], rows *
 * cols < SIMQ_GRID_MAX_CELLS; tolerance in [1, 255]; way_capacity >= 1; the grid, the first pair of the path and the waypoint range
 * inside the declared extent of their buffers; no two problems' waypoint ranges overlapping; d_ways, d_counts, d_status and
 * d_problems disjoint from each other and from the inputs; 8-byte alignment of d_paths, d_ways and d_problems, 4 of the other int32
 * buffers) and copied to d_problems (n descriptors) on `stream`.  Several problems may share a grid.
 * d_status[n] (int32): 0 = ok; 1 = nothing to do: d_path_status[p] was 1 (straight line, d_counts[p] = 0) or 3 (the dense path was
 * cut short by its capacity, d_counts[p] = -1); 2 = bad descriptor, length, path status or coordinate (the kernel checks again and
 * writes nothing else); 3 = way_capacity too small: d_counts[p] holds the needed count and nothing is written past the capacity;
 * 4 = a loop passed its bound (cannot happen). */
typedef struct simq_grid_waypoint_problem {
    int64_t grid_offset;        /* byte offset of the problem's [rows][cols] uint8 grid in d_grids */
    int64_t path_offset;        /* pair offset of its dense path in d_paths */
    int64_t way_offset;         /* pair offset of its waypoints in d_ways */
    int32_t rows, cols;
    int32_t way_capacity;       /* pairs */
    int32_t tolerance;          /* 1 .. 255 */
} simq_grid_waypoint_problem;
#define SIMQ_GRID_WAYPOINTS_MAX_PATH 20480
int simq_grid_waypoints(const uint8_t* d_grids, int64_t grids_bytes, const int32_t* d_paths, int64_t path_pairs,
                        const int32_t* d_lengths, const int32_t* d_path_status, const simq_grid_waypoint_problem* problems, int n,
                        simq_grid_waypoint_problem* d_problems, int32_t* d_ways, int64_t way_pairs, int32_t* d_counts,
                        int32_t* d_status, void* stream);

/* ---- actions to waypoints (envs.py:856-902 Robot.store_new_action; envs.py:2477-2504 OccupancyMap.shortest_path) -------------------
 * The rule.  Per robot: an action a, its position (x, y) and heading (float64), its type and its mapper.  Constants: W = 96
 * (Mapper.LOCAL_MAP_PIXEL_WIDTH), CUBE_WIDTH = 0.044 (envs.py:25), END_EFFECTOR_LOCATION = BACKPACK_OFFSET + BASE_LENGTH of the
 * robot's class (envs.py:804-807, 1059-1060, 1279-1280), C_out = NUM_OUTPUT_CHANNELS of the class.
 *   1. action = unravel_index(a, (C_out, W, W)) = (channel, row, col); a outside [0, C_out W W) is refused.
 *   2. (dx, dy) = pixel_indices_to_position(row, col, (W, W)); dist = sqrt(dx**2 + dy**2); theta = heading + atan2(-dx, dy);
 *      target = (x + dist cos(theta), y + dist sin(theta), 0).
 *   3. waypoints = OccupancyMap.shortest_path(position, target) when use_shortest_path_movement is set, else [position, target].
 *      shortest_path: both positions to pixels; the straight-line test on the thin map; otherwise both pixels snapped to their closest
 *      free cells, SPFA's path (simq_grid_paths' rules), simplified by the exact rule of simq_grid_waypoints with tolerance 1, pruned,
 *      reversed; pixels back to positions (z = 0) with the two given positions at the ends; fewer than two waypoints: the two
 *      positions alone.
 *   4. headings[0] = heading; headings[k] = restrict_heading_range(atan2(dy_k, dx_k)) over successive waypoints, where
 *      restrict_heading_range(h) = (h + pi) % (2 pi) - pi with Python's float %.
 *   5. signed_dist = distance(wp[-2], wp[-1]) - (END_EFFECTOR_LOCATION + CUBE_WIDTH / 2); the last waypoint becomes
 *      wp[-2] + signed_dist (cos, sin)(headings[-1]), z = 0.
 *   6. With more than two waypoints and signed_dist < 0: wp[-2] = wp[-1] and headings[-2] is formed again from wp[-3] to wp[-2].
 * Every float64 above is CPython's math on the host: `** 2` is libm's pow, and the library has no trigonometry.  What this entry
 * point does is the integer and fp32 part of step 3, from the two pixels to the waypoint pixels, in ONE launch: one wavefront per
 * problem runs the straight-line test, the snap, the search, the walk, the simplification and the pruning, with the dense path in LDS
 * (no path buffer, no path capacity).  simq_grid_paths followed by simq_grid_waypoints (tolerance 1) gives the same waypoints, counts
 * and end pixels.
 * Inputs lie where a caller keeps them: three bases -- d_cspace (uint8 configuration spaces, free where != 0), d_thin (uint8 thin
 * maps; NULL when no problem tests the line) and d_closest (int32 [2][rows][cols] blocks; NULL when no problem snaps) -- each with its
 * extent, and per problem an element offset into each.  Several problems may share a map.  The window (box_*) is the caller's, as
 * for simq_grid_paths: it must hold every free cell, the kernel's pass over the grid gives status 2 when one lies outside, and
 * (box_rows + 2) * (box_cols + 2) <= SIMQ_GRID_PATH_MAX_BOX_CELLS; simq_action_waypoints_large below takes the windows over the cap.
 * Upstream status: d_upstream (n_upstream int32 words on the device; NULL with 0) as for simq_grid_distance_images_snapped: a problem
 * with upstream >= 0 whose word is not 0 gets that word as its status and count 0; nothing else of it is read or written.
 * Outputs per problem: int32 (i, j) waypoint pixels, source first, at pair way_offset of d_ways, at most way_capacity pairs;
 * d_counts[p] (1, the target alone, for an unreachable or blocked target, a blocked source and target == source: the caller applies
 * the reference's len(path) < 2); d_endpoints[4 p .. 4 p + 4), the pixels the search used (as given when the line is clear).
 * `problems`: host array of n descriptors, validated here before anything is copied or launched (rows, cols >= 1, rows * cols <
 * SIMQ_GRID_MAX_CELLS; both pixels inside the grid; the window inside the grid and under the cap; way_capacity >= 1; every input and
 * the waypoint range inside the declared extent of its base; upstream -1 or below n_upstream; no two waypoint ranges overlapping;
 * d_problems, d_ways, d_counts, d_endpoints and d_status disjoint from each other and from every input; 8-byte alignment of d_problems
 * and d_ways, 4 of the other int32 buffers) and copied to d_problems (n descriptors) on `stream`.
 * d_status[n] (int32): 0 = traced, 1 = straight line clear (count 0), 2 = bad descriptor, pixel, snapped pixel or window (the kernel
 * checks again and writes nothing else), 3 = way_capacity too small: d_counts[p] holds the need and nothing is written past the
 * capacity, 4 = a loop passed its bound (cannot happen); or the upstream word. */
typedef struct simq_action_waypoint_problem {
    int64_t cspace_offset;      /* byte offset of the problem's [rows][cols] uint8 configuration space in d_cspace */
    int64_t thin_offset;        /* byte offset of its [rows][cols] uint8 thin map in d_thin, or -1 (no straight-line test) */
    int64_t closest_offset;     /* int32 offset of its [2][rows][cols] closest cells in d_closest, or -1 (no snap) */
    int64_t way_offset;         /* pair offset of its waypoints in d_ways */
    int32_t way_capacity;       /* pairs */
    int32_t rows, cols;
    int32_t src_i, src_j, tgt_i, tgt_j;
    int32_t box_i0, box_j0, box_rows, box_cols;
    int32_t upstream;           /* index of its word in d_upstream, or -1 */
} simq_action_waypoint_problem;
int simq_action_waypoints(const uint8_t* d_cspace, int64_t cspace_bytes, const uint8_t* d_thin, int64_t thin_bytes,
                          const int32_t* d_closest, int64_t closest_ints, const simq_action_waypoint_problem* problems, int n,
                          simq_action_waypoint_problem* d_problems, int32_t* d_ways, int64_t way_pairs, int32_t* d_counts,
                          int32_t* d_endpoints, const int32_t* d_upstream, int n_upstream, int32_t* d_status, void* stream);

/* The same launch for windows of any size: the search state, and after the search the dense path and the kept flags, lie in a
 * workspace of the caller's in global memory instead of LDS (the state and the carve-up of simq_grid_paths_large), so
 * SIMQ_GRID_PATH_MAX_BOX_CELLS does not apply; the windows under the cap are accepted too.  Rules, front stages, the upstream word,
 * outputs, the kernel's re-check and status words are those of simq_action_waypoints: for a problem both entry points accept, every
 * byte either writes is equal.  No dynamic LDS.
 * Limits: box_rows + 2 and box_cols + 2 at most 32 767, so that window coordinates stay below 2^15 and the simplification's products
 * below 2^62 for any caller (a map simq_occupancy_maps_large writes has at most 2 050).  The dense path is not bounded by
 * SIMQ_GRID_WAYPOINTS_MAX_PATH: it has at most as many points as the window has free cells, n <= box_rows * box_cols, which is what the
 * workspace is laid out for, and the loop bounds of the simplification and the pruning follow n (at most n - 2 splits, 2 n verdicts,
 * n lines).
 * Workspace: as for simq_grid_paths_large -- problem p's state is the simq_action_waypoints_large_work_bytes(box_rows, box_cols) =
 * simq_grid_paths_large_work_bytes(box_rows, box_cols) bytes from byte work_offset (a multiple of 16) on; after the search the path
 * lies as 16-bit window pairs where the distances lay and the kept flags as a bit mask where the ring lay.  The kernel initialises
 * what it reads; the content after the call is unspecified.  The host function gives -1 for a negative side, a side over 32 765 or
 * box_rows * box_cols >= SIMQ_GRID_MAX_CELLS.
 * Validation as for simq_action_waypoints, with the limit above in place of the cap, and the workspace rules of
 * simq_grid_paths_large. */
typedef struct simq_action_waypoint_large_problem {
    int64_t cspace_offset;      /* the fields of simq_action_waypoint_problem, with the same meaning ... */
    int64_t thin_offset;
    int64_t closest_offset;
    int64_t way_offset;
    int64_t work_offset;        /* ... and the byte offset of the problem's search state in d_work, a multiple of 16 */
    int32_t way_capacity;
    int32_t rows, cols;
    int32_t src_i, src_j, tgt_i, tgt_j;
    int32_t box_i0, box_j0, box_rows, box_cols;
    int32_t upstream;
} simq_action_waypoint_large_problem;
int64_t simq_action_waypoints_large_work_bytes(int32_t box_rows, int32_t box_cols);
int simq_action_waypoints_large(const uint8_t* d_cspace, int64_t cspace_bytes, const uint8_t* d_thin, int64_t thin_bytes,
                                const int32_t* d_closest, int64_t closest_ints, const simq_action_waypoint_large_problem* problems,
                                int n, simq_action_waypoint_large_problem* d_problems, int32_t* d_ways, int64_t way_pairs,
                                int32_t* d_counts, int32_t* d_endpoints, const int32_t* d_upstream, int n_upstream, int32_t* d_status,
                                void* d_work, int64_t work_bytes, void* stream);

/* ---- shortest-path distance queries: the point form of the distance images (envs.py:2506-2511 OccupancyMap.shortest_path_distance,
 * reached through Mapper.distance_to_receptacle, envs.py:2189-2194, by every partial reward; shortest_paths.pyx:150-158
 * GridGraph.shortest_path_distance) ------------------------------------------------------------------------------------------------
 * One problem = one grid [rows][cols] of uint8 (free where != 0), one source pixel and n_targets >= 0 target pixels; one wavefront
 * per problem, every problem of a call in one launch.  Per problem:
 *   snap        (closest_offset >= 0) the source, then each target, is replaced by closest[:, i, j]: int32 [2][rows][cols] at
 *               d_closest + closest_offset, the layout simq_occupancy_maps writes and simq_grid_paths reads
 *   search      the distances of simq_grid_distance_images from the snapped source -- the same updates, fl32(d[u] + w) accepted when
 *               strictly smaller, to the same fixed point -- in the problem's working image, fp32 [rows][cols] at d_work + work_offset
 *   queries     target q of the problem is pair target_offset + q of `targets` (int32 (i, j) pairs) and its distance goes to
 *               d_out[target_offset + q]: the label of the snapped target, -1 where it is unreachable -- the value
 *               GridGraph.shortest_path_distance returns, before OccupancyMap divides it by the pixels per metre
 * images != 0 makes the working images outputs: each then holds what simq_grid_distance_images writes without its epilogue for the
 * snapped source (-1 where unreachable); with images == 0 their content after the call is unspecified.
 * `problems` (n descriptors) and `targets` (n_targets_total pairs) are host arrays, validated here before anything is copied or
 * launched: rows, cols >= 1, rows * cols < SIMQ_GRID_MAX_CELLS; the source and every target inside the grid; every target range
 * inside `targets`; grid, closest block and working image inside the declared extent of their buffers, d_out of at least
 * n_targets_total floats; 4-byte alignment of d_closest, d_work, d_out and d_status, 8 of d_descriptors; no two problems sharing a
 * working image or a target (and so d_out) range; nothing the launch writes -- d_work, d_out, d_status, d_descriptors -- sharing a byte
 * with any other buffer of the call.  Both arrays are then copied, the descriptors first and the targets behind them, to
 * d_descriptors (n * sizeof(simq_grid_query_problem) + 8 * n_targets_total bytes) on `stream`.  Several problems may share a grid
 * and a closest block.  d_closest may be NULL when no problem snaps; targets and d_out when n_targets_total is 0.  d_status[n]
 * (int32): 0 = ok, 1 = the cap of rows * cols + 1 passes was hit (cannot happen, as for the images), 2 = bad descriptor or a
 * pixel outside the grid -- given or snapped; the kernel checks again: nothing is written for a bad descriptor or source, and only
 * that target's distance is left unwritten for a bad target. */
typedef struct simq_grid_query_problem {
    int64_t grid_offset;        /* byte offset of the problem's [rows][cols] uint8 grid in d_grids */
    int64_t closest_offset;     /* int32 offset of its [2][rows][cols] closest cells in d_closest, or -1 */
    int64_t work_offset;        /* float offset of its [rows][cols] fp32 working image in d_work */
    int64_t target_offset;      /* pair offset of its first target in `targets`, float offset of its first distance in d_out */
    int32_t n_targets;
    int32_t rows, cols;
    int32_t src_i, src_j;
    int32_t reserved_;
} simq_grid_query_problem;
int simq_grid_distance_queries(const uint8_t* d_grids, int64_t grids_bytes, const int32_t* d_closest, int64_t closest_ints,
                               const simq_grid_query_problem* problems, int n, const int32_t* targets, int64_t n_targets_total,
                               void* d_descriptors, float* d_work, int64_t work_floats, int images, float* d_out, int64_t out_floats,
                               int32_t* d_status, void* stream);

/* ---- local state images (Mapper.get_state's crop / rotation: envs.py:2199-2215 _get_local_map / _get_local_distance_map,
 * 2243-2275 _create_global_overhead_map / _create_global_robot_map, 2368-2375 the nonspatial channels) -----------------------------
 * One problem = one robot's state: d_out[p][96][96][C] fp32 (NHWC, what simq_forward and the replay ring take), every channel of
 * every problem in one launch.  A channel is (kind, map, value):
 *   MAP       local pixel = the global map `map` sampled through the rotation below                       (_get_local_map)
 *   DISTANCE  as MAP, minus the minimum of the 96 x 96 local image (one fp32 subtract)                    (_get_local_distance_map)
 *   ROBOTS    max(0, max over the problem's robot stamps of map_value * mask pixel)                       (_create_global_robot_map(seg=False))
 *   OVERHEAD  seg = the ROBOTS rule with seg_value and seg_mask; seg > 0 ? seg : pixel of base map `map` (_create_global_overhead_map)
 *   CONSTANT  `value`                                                                                     (envs.py:2375)
 * Sampling is scipy.ndimage.rotate(crop, angle, order=0) with its defaults (reshape, constant 0 outside) followed by the centre crop.
 * The caller computes, in float64 as scipy does, for an n x n image rotated by `angle` degrees: c, s = cosdg(angle), sindg(angle);
 * r = [c, s, -s, c]; shape = int(ptp(R @ corners) + 0.5) per axis; offset = (n - 1) / 2 - R @ ((shape - 1) / 2).  A problem's
 * rotation has n = 136 (the crop around the robot's pixel) and angle = 90 - degrees(heading); a robot stamp's has n = 96 (its mask)
 * and angle = degrees(heading) - 90.  Per local pixel (i, j) the kernel forms, in float64 and without contraction,
 *   (oi, oj) = (i + shape[0] / 2 - 48, j + shape[1] / 2 - 48);  cc_h = offset[h] + (oi * r[2h] + oj * r[2h + 1]);
 * a pixel with cc_h < 0 or cc_h > n - 1 is 0, otherwise it is the global pixel (pixel_i - 68 + floor(cc_0 + 0.5), pixel_j - 68 +
 * floor(cc_1 + 0.5)).  A robot stamp covers the global pixels [pixel - shape / 2, pixel - shape / 2 + shape) and is sampled there by
 * the same rule.  Results equal the reference's bit for bit.
 * Maps are fp32 [rows][cols] device arrays read in place (d_data: any device address, e.g. an image simq_grid_distance_images
 * wrote); d_masks is a bank [n_masks][96][96] fp32 (Mapper.robot_masks).  Everything is validated on the host before anything is
 * copied or launched: the 136 x 136 crop inside its map (68 <= pixel <= rows - 68), every stamp of a problem inside the map, map /
 * mask / robot indices in range, a channel's map of the problem's shape, rotated shapes in [n, ceil(n * sqrt 2)], finite doubles,
 * d_out large enough and disjoint from every map and the mask bank.  The descriptors are then copied to d_desc (at least
 * simq_local_state_desc_bytes(...) bytes of device scratch, 8-byte aligned) on `stream`. */
#define SIMQ_LOCAL_MAP 0
#define SIMQ_LOCAL_DISTANCE 1
#define SIMQ_LOCAL_ROBOTS 2
#define SIMQ_LOCAL_OVERHEAD 3
#define SIMQ_LOCAL_CONSTANT 4
#define SIMQ_LOCAL_CROP 136         /* round_up_to_even(sqrt(2) * 96), envs.py:2201 */
#define SIMQ_LOCAL_MAX_CHANNELS 64
typedef struct simq_local_rotation {
    double r[4];                /* [[c, s], [-s, c]] row-major */
    double offset[2];
    int32_t shape[2];           /* of the rotated image */
} simq_local_rotation;
typedef struct simq_local_map {
    const float* d_data;        /* [rows][cols] fp32 on the device */
    int32_t rows, cols;
} simq_local_map;
typedef struct simq_local_robot {
    simq_local_rotation rot;    /* of the 96 x 96 mask, angle = degrees(heading) - 90 */
    int32_t pixel_i, pixel_j;   /* position_to_pixel_indices of the robot (envs.py:2391-2396) */
    int32_t mask;               /* ROBOTS: index into d_masks (a lifting LiftingRobot: the mask with the cube, envs.py:2258-2260) */
    float seg_value;            /* OVERHEAD: camera.get_seg_value('robot_group_k') as fp32 */
    float map_value;            /* ROBOTS: 1 (or 0.5: a LiftingRobot that is not lifting) */
    int32_t seg_mask;           /* OVERHEAD: index into d_masks (always the robot class's own mask, envs.py:2254-2256) */
} simq_local_robot;
typedef struct simq_local_problem {
    simq_local_rotation rot;    /* of the 136 x 136 crop, angle = 90 - degrees(heading) */
    int32_t pixel_i, pixel_j;   /* the robot's pixel in its global maps */
    int32_t rows, cols;         /* shape of the environment's global maps */
    int32_t robot_begin, robot_count;   /* the environment's robots: robots[robot_begin .. robot_begin + robot_count) */
} simq_local_problem;
typedef struct simq_local_channel {
    int32_t kind;               /* SIMQ_LOCAL_* */
    int32_t map;                /* MAP / DISTANCE / OVERHEAD: index into maps */
    float value;                /* CONSTANT */
    int32_t reserved_;
} simq_local_channel;
int64_t simq_local_state_desc_bytes(int n_maps, int n_robots, int n, int n_channels);
/* channels: [n][n_channels], problem-major.  robots / d_masks may be NULL when n_robots == 0. */
int simq_local_state_images(const simq_local_map* maps, int n_maps, const float* d_masks, int n_masks, const simq_local_robot* robots,
                            int n_robots, const simq_local_problem* problems, int n, const simq_local_channel* channels, int n_channels,
                            void* d_desc, int64_t desc_bytes, float* d_out, int64_t out_floats, void* stream);

/* simq_local_state_images with a destination per problem: problem p's [96][96][C] image begins at d_pool + slots[p] * 96 * 96 * C
 * floats (a replay pool whose free slots are not consecutive).  `slots` is a HOST array of n slots, checked with everything else
 * before anything is copied or launched: 0 <= slot < pool_slots, none named twice, and no WRITTEN slot sharing a byte with a map, the
 * mask bank or d_desc -- the pool as a whole may hold them (a map kept in another slot of the same allocation is read in place).
 * The slot table travels behind the descriptors: d_desc takes simq_local_state_slots_desc_bytes(...) bytes.  Every other rule, and
 * every image, is simq_local_state_images'. */
int64_t simq_local_state_slots_desc_bytes(int n_maps, int n_robots, int n, int n_channels);
int simq_local_state_images_slots(const simq_local_map* maps, int n_maps, const float* d_masks, int n_masks, const simq_local_robot* robots,
                                  int n_robots, const simq_local_problem* problems, int n, const simq_local_channel* channels,
                                  int n_channels, const int64_t* slots, void* d_desc, int64_t desc_bytes, float* d_pool, int64_t pool_slots,
                                  void* stream);

/* Both entries with bf16 images (a replay pool of bf16 states, simq_plan_options.bf16_states): the same descriptors, checks, kernel
 * and d_desc sizes; d_out / d_pool hold bf16 elements (2-byte aligned, out_elems counts elements, a pool slot is 96 * 96 * C of them).
 * The element stored is the fp32 value the fp32 entry stores -- a distance channel has its minimum subtracted in fp32 first -- rounded
 * once to nearest even, with the conversion the first convolution of a plain-bf16 plan applies to an fp32 state. */
int simq_local_state_images_bf16(const simq_local_map* maps, int n_maps, const float* d_masks, int n_masks, const simq_local_robot* robots,
                                 int n_robots, const simq_local_problem* problems, int n, const simq_local_channel* channels,
                                 int n_channels, void* d_desc, int64_t desc_bytes, uint16_t* d_out, int64_t out_elems, void* stream);
int simq_local_state_images_slots_bf16(const simq_local_map* maps, int n_maps, const float* d_masks, int n_masks,
                                       const simq_local_robot* robots, int n_robots, const simq_local_problem* problems, int n,
                                       const simq_local_channel* channels, int n_channels, const int64_t* slots, void* d_desc,
                                       int64_t desc_bytes, uint16_t* d_pool, int64_t pool_slots, void* stream);

/* simq_local_state_images_slots with a POOL per problem as well: problem p's [96][96][C] image begins at slot dests[p].slot of pool
 * pools[dests[p].pool], and a slot holds 96 * 96 * C elements of that pool's type -- fp32, or bf16 (the element the bf16 entries
 * store), so that the states of robot groups whose replay pools differ, in place and in type, are written by one launch.  `pools`
 * (1 .. SIMQ_LOCAL_MAX_POOLS entries; one may receive no problem) and `dests` (n entries) are HOST arrays and travel behind the
 * other descriptor blocks: d_desc takes simq_local_state_pools_desc_bytes(...) bytes (the slots size plus the two tables; -1 where
 * simq_local_state_slots_desc_bytes gives -1).  Checked on the host with everything else, before anything is copied or launched:
 * every d_pool non-NULL and aligned to its element (4 bytes, or 2), bf16 0 or 1, pool_slots in the slots entry's range, no two pools
 * sharing a byte (so none listed twice), 0 <= dests[p].pool < n_pools, 0 <= dests[p].slot < that pool's pool_slots, no (pool, slot)
 * named twice (the same slot number in two pools is fine), and no WRITTEN slot of any pool sharing a byte with a map, the mask bank
 * or d_desc -- a map kept in another slot of a listed pool is read in place.  Every other rule is simq_local_state_images_slots',
 * and every byte written is the byte that entry (fp32 pool) or simq_local_state_images_slots_bf16 (bf16 pool) writes for the same
 * problem into the same slot.  Logged as "local_state_pools". */
#define SIMQ_LOCAL_MAX_POOLS 16
typedef struct simq_local_pool {
    void* d_pool;               /* [pool_slots][96][96][C] on the device */
    int64_t pool_slots;
    int32_t bf16;               /* 0: fp32 elements, 1: bf16 elements */
    int32_t reserved_;
} simq_local_pool;
typedef struct simq_local_dest {
    int64_t slot;               /* of pools[pool] */
    int32_t pool;
    int32_t reserved_;
} simq_local_dest;
int64_t simq_local_state_pools_desc_bytes(int n_maps, int n_robots, int n, int n_channels, int n_pools);
int simq_local_state_images_pools(const simq_local_map* maps, int n_maps, const float* d_masks, int n_masks, const simq_local_robot* robots,
                                  int n_robots, const simq_local_problem* problems, int n, const simq_local_channel* channels,
                                  int n_channels, const simq_local_pool* pools, int n_pools, const simq_local_dest* dests, void* d_desc,
                                  int64_t desc_bytes, void* stream);

/* ---- global intention / history maps (Mapper._create_global_intention_or_history_map, envs.py:2301-2346, and the per-robot spatial
 * maps of Mapper._get_intention_channels, envs.py:2360-2366) ----------------------------------------------------------------------
 * One problem = one global map d_out[p][rows][cols] fp32, every map of a call in one launch; the kernel writes every pixel, so the
 * caller zero-fills nothing.  A map is the maximum, per pixel, over the points of the problem's segments, then dilated with the disk
 * di^2 + dj^2 <= radius^2 (radius = intention_map_line_thickness - 1; 0: no dilation; pixels outside the map are absent).
 * A segment is the skimage.draw.line from (r0, c0) to (r1, c1): with n = max(|dr|, |dc|), m = min(|dr|, |dc|), point i = 0 .. n is
 * i steps along the major axis (the rows when |dr| > |dc|) and (2 * m * i + n) / (2 * n) (integer division) along the minor one;
 * drop_last leaves point n out (the reference drops it for every segment of a path but the last: a drop_last segment with n = 0
 * draws nothing).  STORE puts `value` (intention_map_scale as fp32: the circle, binary and line encodings and the spatial channel; a
 * single pixel is the segment r0 = r1, c0 = c1); RAMP puts (float)clip(y_i, 0, 1) with np.linspace(start, stop, n + 1)'s float64
 * y_i = i * step + start (product and sum rounded separately), y_n = stop, where the caller computes, in float64 and in the
 * reference's order, start = 1 - path_length, stop = 1 - (path_length + segment_length), step = (stop - start) / n (0 when n = 0).
 * The order of segments does not matter.  Results equal the reference's bit for bit.
 * Everything is validated on the host before anything is copied or launched: end pixels inside the map, modes and flags, finite
 * doubles, a stored value that is finite, >= 0 and not -0 (the maximum is taken on the fp32 bit patterns), segment ranges inside the
 * segment array, radius in [0, SIMQ_INTENTION_MAX_RADIUS], rows * cols < 2^28, d_out large enough and disjoint from d_desc.  The
 * descriptors are then copied to d_desc (at least simq_intention_desc_bytes(...) bytes of device scratch, 8-byte aligned) on `stream`. */
#define SIMQ_INTENTION_STORE 0
#define SIMQ_INTENTION_RAMP 1
#define SIMQ_INTENTION_MAX_RADIUS 8
typedef struct simq_intention_segment {
    double start, stop, step;   /* RAMP */
    int32_t r0, c0, r1, c1;     /* Mapper.position_to_pixel_indices of the two waypoints (envs.py:2391-2396) */
    int32_t mode;               /* SIMQ_INTENTION_* */
    int32_t drop_last;          /* 1: point n is not drawn */
    float value;                /* STORE */
    int32_t reserved_;
} simq_intention_segment;
typedef struct simq_intention_problem {
    int32_t seg_begin, seg_count;   /* the map's segments: segments[seg_begin .. seg_begin + seg_count); none: a map of zeros */
} simq_intention_problem;
int64_t simq_intention_desc_bytes(int n_segments, int n);
/* segments may be NULL when n_segments == 0. */
int simq_intention_maps(const simq_intention_segment* segments, int n_segments, const simq_intention_problem* problems, int n, int rows,
                        int cols, int radius, void* d_desc, int64_t desc_bytes, float* d_out, int64_t out_floats, void* stream);
/* ---- the same maps for problems of several room shapes and line thicknesses in one launch ------------------------------------------
 * Problem p gives exactly the map simq_intention_maps gives for the same segments with rows = rows_p, cols = cols_p and
 * radius = radius_p, written row-major at d_out[out_offset_p .. out_offset_p + rows_p * cols_p): every pixel of every problem is
 * written, no other float of d_out is touched (the maps may lie in any order, with gaps).  One launch for all problems: its grid is
 * the sum of the problems' counts of 32 x 256 tiles, and the workgroups find their problem by a binary search over the prefix of those
 * counts.  d_desc (at least simq_intention_shapes_desc_bytes(...) bytes of device scratch, 8-byte aligned) receives the segments, the
 * problems and that prefix -- int32 [n + 1], the last entry the grid size, padded to a multiple of 8 bytes -- in this order.
 * Two problems may name one segment range; the segments then have to fit the maps of both.  The launch log names it
 * "intention_maps_shapes".
 * Everything is validated on the host before anything is copied or launched: n in 1 .. 2^20, n_segments in 0 .. 2^24; per problem
 * rows, cols >= 1, rows * cols < 2^28, radius in [0, SIMQ_INTENTION_MAX_RADIUS], its segment range inside the segment array, its
 * floats inside d_out and disjoint from d_desc; every segment of a problem's range ends inside that problem's map; modes, flags, finite
 * doubles and the stored-value rule as above; no two problems' floats overlap; at most 2^31 - 1 workgroups; d_desc 8-byte and d_out
 * 4-byte aligned, d_desc large enough. */
typedef struct simq_intention_shaped_problem {
    int64_t out_offset;             /* the first float of the map in d_out */
    int32_t rows, cols;             /* the map's shape */
    int32_t seg_begin, seg_count;   /* the map's segments: segments[seg_begin .. seg_begin + seg_count); none: a map of zeros */
    int32_t radius;                 /* intention_map_line_thickness - 1 */
    int32_t reserved_;
} simq_intention_shaped_problem;
int64_t simq_intention_shapes_desc_bytes(int n_segments, int n);
/* segments may be NULL when n_segments == 0. */
int simq_intention_maps_shapes(const simq_intention_segment* segments, int n_segments, const simq_intention_shaped_problem* problems, int n,
                               void* d_desc, int64_t desc_bytes, float* d_out, int64_t out_floats, void* stream);

/* ---- occupancy maps: configuration space, thin configuration space and closest free cells (OccupancyMap.update, envs.py:2452-2455,
 * read through OccupancyMap._closest_valid_cspace_indices, envs.py:2522-2523) ------------------------------------------------------
 * One problem = one occupancy map [rows][cols] of uint8 (occupied where != 0), one room mask of the same shape (inside the room where
 * != 0), a dilation radius and a thin radius; every problem of a call in one launch, three outputs per problem, every element written:
 *   configuration space  d_cspace[out_offset + i * cols + j] (uint8) is 1 where room_mask != 0 and no occupied cell lies at an offset
 *                        di^2 + dj^2 <= radius^2 inside the map, 0 elsewhere (cells outside the map are absent: the border value 0
 *                        of scipy.ndimage.binary_dilation with the disk footprint)
 *   thin space           d_thin[out_offset + i * cols + j] (uint8) is 0 where some cell with room_mask != 0 and occupancy != 0 lies
 *                        within di^2 + dj^2 <= thin_radius^2, 1 elsewhere
 *   closest free cells   d_closest[2 * out_offset + h * rows * cols + i * cols + j] (int32, h = 0: row, 1: column; the layout and
 *                        dtype of scipy.ndimage.distance_transform_edt(1 - configuration_space, return_indices=True)) is the free
 *                        cell of the configuration space nearest to (i, j) by squared Euclidean distance; a free cell maps to itself
 * Radius 0 is no dilation.  Ties between nearest free cells follow scipy's two one-dimensional passes: f0[i][j] = the nearest free row
 * of column j, the smaller row on a tie; the answer at (i, j) is (f0[i][j'], j') for the column j' that minimises
 * (j' - j)^2 + (f0[i][j'] - i)^2 over the columns that hold a free cell, the smaller j' on a tie -- among the nearest free cells the
 * smallest column, then the smallest row.  All arithmetic is integer; results equal the reference's element for element.
 * `problems`: host array of n descriptors, validated here before anything is copied or launched (rows, cols in [1,
 * SIMQ_OCCUPANCY_MAX_DIM], radii in [0, SIMQ_OCCUPANCY_MAX_RADIUS], both inputs inside the maps_bytes of d_maps, the outputs inside
 * the cspace_bytes of d_cspace and d_thin each and the closest_ints of d_closest, no two problems' outputs overlapping, the output
 * buffers and d_status disjoint from each other, from d_maps and from d_problems; several problems may share a room mask) and copied
 * to the caller's device buffer d_problems (n descriptors) on `stream`.  d_status[n] (int32): 0 = ok, 1 = the configuration space
 * has no free cell (the closest cells are all -1; both uint8 maps are valid), 2 = bad descriptor (the kernel checks again and writes
 * nothing else).  The planes lie in LDS, which bounds the sides; simq_occupancy_maps_large below takes the larger maps. */
#define SIMQ_OCCUPANCY_MAX_DIM 256
#define SIMQ_OCCUPANCY_MAX_RADIUS 16
typedef struct simq_occupancy_problem {
    int64_t occupancy_offset;   /* byte offset of the problem's [rows][cols] uint8 occupancy map in d_maps */
    int64_t mask_offset;        /* byte offset of its [rows][cols] uint8 room mask in d_maps */
    int64_t out_offset;         /* byte offset of its maps in d_cspace and in d_thin; its closest cells start at int 2 * out_offset */
    int32_t rows, cols;
    int32_t radius, thin_radius;
} simq_occupancy_problem;
int simq_occupancy_maps(const uint8_t* d_maps, int64_t maps_bytes, const simq_occupancy_problem* problems, int n,
                        simq_occupancy_problem* d_problems, uint8_t* d_cspace, uint8_t* d_thin, int64_t cspace_bytes, int32_t* d_closest,
                        int64_t closest_ints, int32_t* d_status, void* stream);

/* The same three results for maps of up to SIMQ_OCCUPANCY_LARGE_MAX_DIM cells a side: the 16-bit plane of column distances, then of
 * nearest free rows, lies in a workspace of the caller's in global memory instead of LDS, and the configuration space is read back
 * from d_cspace where the kernel has just written it.  Rules, outputs, the kernel's re-check and the status words are those of
 * simq_occupancy_maps: for a problem both entry points accept -- the maps under SIMQ_OCCUPANCY_MAX_DIM are accepted here too --
 * every byte either writes is equal.  One workgroup per problem as there, its columns and pixels looped over the block; a pass over
 * a map costs a few times what it costs in LDS, so this entry point is for the maps the other refuses.
 * Limits: rows, cols in [1, SIMQ_OCCUPANCY_LARGE_MAX_DIM] and rows * cols < SIMQ_GRID_MAX_CELLS (what the distance images and the
 * action waypoints behind this stage take); radii in [0, SIMQ_OCCUPANCY_MAX_RADIUS].
 * Workspace: d_work (work_bytes bytes, 16-byte aligned) is the caller's; the library allocates nothing.  Problem p's plane is the
 * simq_occupancy_maps_large_work_bytes(rows, cols) = (2 * rows * cols + 15) / 16 * 16 bytes from byte work_offset (a multiple of 16)
 * on: one uint16 per cell (a row index no longer fits a byte), rounded up to 16.  The kernel initialises what it reads; the content
 * after the call is unspecified.  simq_occupancy_maps_large_work_bytes is a host function of the two numbers alone (-1 for a shape
 * outside the limits above).
 * Validation as for simq_occupancy_maps with the limits above, and in addition: d_work not NULL and 16-byte aligned; every problem's
 * range inside work_bytes at a non-negative multiple of 16; no two problems' ranges overlapping; d_work sharing no byte with any
 * other buffer of the call. */
#define SIMQ_OCCUPANCY_LARGE_MAX_DIM 2048
typedef struct simq_occupancy_large_problem {
    int64_t occupancy_offset;   /* the fields of simq_occupancy_problem, with the same meaning ... */
    int64_t mask_offset;
    int64_t out_offset;
    int64_t work_offset;        /* ... and the byte offset of the problem's plane in d_work, a multiple of 16 */
    int32_t rows, cols;
    int32_t radius, thin_radius;
} simq_occupancy_large_problem;
int64_t simq_occupancy_maps_large_work_bytes(int32_t rows, int32_t cols);
int simq_occupancy_maps_large(const uint8_t* d_maps, int64_t maps_bytes, const simq_occupancy_large_problem* problems, int n,
                              simq_occupancy_large_problem* d_problems, uint8_t* d_cspace, uint8_t* d_thin, int64_t cspace_bytes,
                              int32_t* d_closest, int64_t closest_ints, int32_t* d_status, void* d_work, int64_t work_bytes,
                              void* stream);

/* ---- observation maps: camera frames into the overhead and occupancy maps (Camera.capture_image, envs.py:1926-1954; the scatters of
 * Mapper.update, envs.py:2053-2061, and OccupancyMap.update, envs.py:2444-2449) ----------------------------------------------------
 * One problem = one camera frame (depth buffer [height][width] fp32 and body ids [height][width] int32, both in d_frames, a buffer of
 * 4-byte words) and one pair of persistent maps updated in place: the overhead map [rows][cols] fp32 in d_overhead and the occupancy
 * map [rows][cols] uint8 in d_occupancy.  Every problem of a call in one launch.  All arithmetic is fp32, every product and sum rounded
 * on its own (no fused multiply-add), the division correctly rounded; per frame pixel (h, w), frame index k = h * width + w:
 *   depth  = far_near / (far - far_minus_near * buffer[k])
 *   p_c    = cam_c + depth * ((principal_c + px[w] * right_c) + py[h] * up_c)                        c = x, y, z
 *   seg    = 1/8 [id == 0] + 2/8 [min_obstacle <= id <= max_obstacle] + 3/8 [has_receptacle and id == receptacle]
 *            + 4/8 [min_cube <= id <= max_cube]            (a sum of eighths: exact; an id that matches nothing has seg 0)
 *   (i, j) = (clip(floor(rows / 2 - p_y * 96), 0, rows - 1), clip(floor(cols / 2 + p_x * 96), 0, cols - 1))
 *            (Mapper.position_to_pixel_indices, envs.py:2391-2396: a point outside the map lands on its border pixels; the clip is
 *            taken on the float, so a point beyond the int32 range lands on the border of its side too)
 * The caller forms the three depth constants (far * near, far, far - near, each rounded to fp32 once), the camera vectors and the
 * tables px[width], py[height] on the host in the reference's own sequence of float32 operations (envs.py:1931-1943); the library has
 * no trigonometry and no normalisation.
 *   overhead map   pixel (i, j) takes the seg of the point with the greatest p_z among those that land on it; among points of equal
 *                  greatest p_z (-0 equals +0) the one with the largest frame index k -- what the reference's assignment in
 *                  ascending-z order gives when the sort is stable.  A seg of 0 is written like any other.  A pixel no point lands
 *                  on keeps its value.
 *   occupancy map  pixel (i, j) becomes 1 where a point with seg == 2/8 lands, whatever its height, and is otherwise left as it is.
 * A frame with a point that is not finite (a depth buffer outside what the near and far planes allow) changes neither map of its
 * problem and gives status 1, the other problems of the launch are not affected; the reference would let such a point win or lose
 * pixels by the accident of its sort.
 * `problems`: host array of n descriptors, validated here before anything is copied or launched (height, width >= 1 and height *
 * width <= SIMQ_OBSERVATION_MAX_POINTS; rows, cols in [1, 2^24), so that rows / 2 and rows - 1 are exact in fp32, and rows * cols <
 * 2^28; the frame, its ids and both tables inside the frame_words of d_frames; both maps inside overhead_floats / occupancy_bytes; finite camera vectors and constants; has_receptacle 0 or
 * 1; no two maps of the launch -- overhead or occupancy, of one problem or of two -- sharing a byte, because the order of two updates
 * of one map matters; every map disjoint from d_frames, d_problems and d_status; alignment) and copied to the caller's device buffer
 * d_problems (n descriptors) on `stream`.  Several problems may share a frame or the tables.  d_status[n] (int32): 0 = updated, 1 = a
 * point was not finite (both maps unchanged), 2 = bad descriptor (the kernel checks sizes and offsets again and writes nothing else). */
#define SIMQ_OBSERVATION_MAX_POINTS (1 << 22)
typedef struct simq_observation_problem {
    int64_t depth_offset;       /* word offset of the depth buffer [height][width] fp32 in d_frames */
    int64_t ids_offset;         /* word offset of the body ids [height][width] int32 in d_frames */
    int64_t px_offset;          /* word offset of px[width] fp32 in d_frames */
    int64_t py_offset;          /* word offset of py[height] fp32 in d_frames */
    int64_t overhead_offset;    /* float offset of the [rows][cols] fp32 overhead map in d_overhead */
    int64_t occupancy_offset;   /* byte offset of the [rows][cols] uint8 occupancy map in d_occupancy */
    float cam[3], principal[3], right[3], up[3];
    float far_near, far, far_minus_near;
    int32_t min_obstacle, max_obstacle;
    int32_t receptacle, has_receptacle;    /* has_receptacle 0: no receptacle term (rescue environments) */
    int32_t min_cube, max_cube;
    int32_t height, width;      /* of the frame */
    int32_t rows, cols;         /* of both maps */
    int32_t reserved_;
} simq_observation_problem;
int simq_observation_update(const void* d_frames, int64_t frame_words, const simq_observation_problem* problems, int n,
                            simq_observation_problem* d_problems, float* d_overhead, int64_t overhead_floats, uint8_t* d_occupancy,
                            int64_t occupancy_bytes, int32_t* d_status, void* stream);

/* ---- observation maps, ordered frame sequences: several camera frames per pair of maps in one launch --------------------------------
 * What successive simq_observation_update launches leave in a pair of maps, one frame each and in the order given, computed by one
 * launch, bit for bit.  `frames`: host array of n_frames descriptors; the frame, camera and id-range fields of simq_observation_problem
 * mean what they mean above.  `begin`: host table [n_sequences + 1]; sequence s is the frames begin[s] .. begin[s + 1] - 1 in
 * application order, and all of them name one overhead_offset, occupancy_offset, rows and cols: the maps of the sequence.  In everything
 * else the frames of a sequence may differ (height and width, so that cameras may mix; the id ranges).  Per frame the projection, seg,
 * pixel (i, j) and the rule among the points of ONE frame are those of simq_observation_update, unchanged: the same fp32 operations,
 * none fused, the correctly rounded division; among equal greatest p_z the largest frame index k; -0 equals +0.  Across the frames
 * of a sequence:
 *   overhead map   pixel (i, j) takes the value that the LAST frame of the sequence with a point on (i, j) gives it by the per-frame
 *                  rule; the heights in earlier frames do not matter.  A seg of 0 is written like any other.  A pixel that no frame
 *                  of the sequence reaches keeps its value.
 *   occupancy map  pixel (i, j) becomes 1 where a point with seg == 2/8 of ANY applied frame lands, and is otherwise left as it is.
 *   a frame with a point that is not finite is skipped as a whole: it gives status 1, decides no overhead pixel and sets no occupancy
 *                  byte, and the other frames of its sequence are applied as if it were absent (the per-problem rule of
 *                  simq_observation_update carried to frames).
 * The configuration space is derived from the final occupancy map only (simq_occupancy_maps), so nothing between the frames is lost.
 * A sequence holds at most SIMQ_OBSERVATION_MAX_SEQUENCE frames: the kernel orders points by one 64-bit key, [position in the
 * sequence + 1 : 10 bits][order-preserving bits of p_z : 32][frame index k : 22], k < SIMQ_OBSERVATION_MAX_POINTS = 2^22 leaves 10
 * bits, and key 0 marks the untouched pixel.  More frames of one map take successive launches.
 * Validated here before anything is copied or launched: per frame everything simq_observation_update checks per problem; begin[0] = 0,
 * begin[n_sequences] = n_frames and begin rising, so every sequence has 1 .. SIMQ_OBSERVATION_MAX_SEQUENCE frames; the frames of a
 * sequence agreeing on the four map fields; no two SEQUENCES sharing a byte of any map, overhead or occupancy (the frames of one map
 * belong in one sequence); every map disjoint from d_frames, d_problems, d_begin and d_status, and those from each other; alignment
 * (d_problems 8-byte, the others 4-byte).  A refusal writes nothing.  The descriptors are copied to the caller's device buffers
 * d_problems (n_frames descriptors) and d_begin (n_sequences + 1 int32) on `stream`.  d_status[n_frames] (int32), one word per frame:
 * 0 = applied, 1 = a point was not finite (the frame was skipped), 2 = bad descriptor: the kernel checks sizes, offsets and the
 * agreement of the map fields again, and a sequence with a bad descriptor writes nothing and gives 2 for all its frames. */
#define SIMQ_OBSERVATION_MAX_SEQUENCE 1023
int simq_observation_update_sequences(const void* d_frames, int64_t frame_words, const simq_observation_problem* frames, int n_frames,
                                      const int32_t* begin, int n_sequences, simq_observation_problem* d_problems, int32_t* d_begin,
                                      float* d_overhead, int64_t overhead_floats, uint8_t* d_occupancy, int64_t occupancy_bytes,
                                      int32_t* d_status, void* stream);

/* ---- Q-map visualisations: the state and output panels of utils.get_state_output_visualization (utils.py:97-131), as the training
 * loop draws them for tensorboard (train.py:292-304) and enjoy.py --debug on every step --------------------------------------------
 * One problem = one state [96][96][channels] fp32 NHWC (a batch row, a slice of a replay ring: read in place) and one output
 * [n][96][96] fp32 (a Q-map, or the stacked ground-truth and predicted intention of train.py:300-303), 1 <= n <= SIMQ_VISUALIZATION_MAX_OUTPUTS,
 * 1 <= channels <= SIMQ_LOCAL_MAX_CHANNELS; every problem of a call in one launch.  Problem p's image starts at float out_offset of
 * d_out and is [96][W][3] fp32, W = 96 + 1 + 96 * n + (n - 1) (chw = 0), or [3][96][W], the transpose(2, 0, 1) of train.py:297
 * (chw = 1).  Along a row:
 *   columns [0, 96)            the state panel (get_state_visualization): state channels (0, 0, 0) for channels = 1, (1, 0, 0) for
 *                              channels = 2, (1, 0, channels - 1) otherwise
 *   column 96, and one column between two output panels: 0 (the vertical bars; none after the last panel)
 *   output panel q = 0 .. n-1  columns [97 + 97 * q, 97 + 97 * q + 96).  With mn, mx the minimum and maximum over the WHOLE [n][96][96]
 *                              output (scale_min_max: one pair for all channels), in fp32, every operation rounded on its own:
 *                                d = (mx - mn) + 1e-6f;  x = (v - mn) / d  (the correctly rounded quotient, no reciprocal);
 *                                k = (uint8) rint_half_even(255 * x)       (to_uint8_image)
 *                                colour c: (one_minus_alpha * state[i][j][0]) + (alpha_f * jet[k][c])   (get_output_visualization)
 *                              one_minus_alpha = (float)(1.0 - alpha) and alpha_f = (float)alpha, formed here on the host as numpy forms
 *                              them from a python scalar; the two products and the sum are not fused.
 * d_jet is the caller's colour map [256][3] fp32 (utils.JET); the library holds none.  Results equal the reference's bit for bit
 * under numpy >= 2 (a python float combined with a float32 array stays float32) for finite outputs; a NaN or an infinity in an output,
 * or a range mx - mn that overflows, is outside that claim (the reference casts a NaN to uint8 there): k is then clamped into [0, 255].
 * `problems`: host array of n_problems descriptors, validated here before anything is copied or launched (n and channels in range,
 * alpha finite, chw 0 or 1; every pointer non-NULL and 4-byte aligned, d_problems 8-byte; every address range below 2^63; each image
 * inside the out_floats of d_out and no two images sharing a float; every image disjoint from every state, every output, d_jet and
 * d_problems) and copied to the caller's device buffer d_problems (n_problems descriptors) on `stream`. */
#define SIMQ_VISUALIZATION_MAX_OUTPUTS 4
typedef struct simq_visualization_problem {
    const float* d_state;       /* [96][96][channels] fp32 on the device */
    const float* d_output;      /* [n][96][96] fp32 on the device */
    int64_t out_offset;         /* float offset of the problem's image in d_out */
    int32_t n, channels;
} simq_visualization_problem;
int simq_state_output_visualizations(const simq_visualization_problem* problems, int n_problems, simq_visualization_problem* d_problems,
                                     const float* d_jet, double alpha, int chw, float* d_out, int64_t out_floats, void* stream);

/* ---- measurement aid (bench.py): HIP-event timing of the GEMM-class launches ----------------
 * Between start and stop every implicit-GEMM launch (forward + dgrad; kind 0: the fp32 96x64 tile that dominates the
 * headline workload, kind 2: every other tile / precision) and every wgrad launch (kind 1) is
 * bracketed by hipEventRecord on its own stream.  stop() fills, per kind (max_kinds >= 3 to see all),
 * {launches, total ms, total algorithmic flops (2*M*N*K), total algorithmic bytes}.  Not thread-safe. */
int simq_profile_start(void);
int simq_profile_stop(double* out, int max_kinds);
/* ... and a launch log (always on): every launcher names the kernel FAMILY that took a launch -- "igemm_bf16_img_whole" / "_half" (image
 * tile), "igemm_bf16_c64", "igemm_bf16_pp", "igemm_bf16_dma", "igemm_bf16_reg", "wgrad_bf16_img", "wgrad_bf16_pp", "wgrad_bf16_reg",
 * "stem_conv_bf16", "stem_wgrad_bf16", "stem_conv_bf16_wide[_x16]", "stem_wgrad_bf16_wide[_x16]", "bn_apply16", "bn_bwd_apply16[_mask_from_y]", "gemm_f32_batched", "igemm_f32", "conv_img_f32",
 * "stem_conv_f32", "winograd_f2" / "winograd_f4" [_wgrad], "wgrad_f32" [_batched], "local_state" [_bf16], "local_state_slots" [_bf16],
 * "local_state_pools", "intention_maps", "intention_maps_shapes" ... (csrc: note_launch).  simq_launch_count: launches
 * of one family since the last reset (0 for a name that never ran); simq_launch_counts: "name=count;..." of every family that ran.
 * The parity tests use it to assert that the kernels a batch size is meant to select DID run. */
int simq_launch_counts_reset(void);
int64_t simq_launch_count(const char* family);
int simq_launch_counts(char* buf, int cap);

#ifdef __cplusplus
}
#endif
#endif /* SIMQ_H */
