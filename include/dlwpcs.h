/*
 * dlwpcs.h -- C ABI of the MI355X-native DLWP-CS cubed-sphere hot path (libdlwpcs.so, HIP, gfx950).
 *
 * This is the drop-in boundary described in SURVEY.md section 8(b): everything the Python layers
 * `DLWP.custom.CubeSpherePadding2D` / `DLWP.custom.CubeSphereConv2D` (and the Keras stock ops wired between them in
 * the DLWP-CS U-Net) need from the device.  Conventions:
 *
 *   - plain C types only; every tensor argument is a raw DEVICE pointer + explicit sizes.  No torch types.
 *   - the CALLER owns every buffer (inputs, outputs, weights, gradients, tables, workspace); the library allocates
 *     nothing and keeps no mutable global state (the opt-in launch profiler at the end of this header excepted), so it
 *     is re-entrant across streams and devices.
 *   - every device entry point enqueues on the caller's `stream` (a hipStream_t) and returns without synchronising.
 *   - return value: 0 = OK, <0 = error code (DLWPCS_E_*); a human-readable message for the calling thread is
 *     available from dlwpcs_last_error().  Nothing throws across the boundary.
 *   - tensors on the hot path are `channels_last`:  x[b][face][row][col][channel]  (face axis = 6,
 *     faces 0-3 equatorial going east, 4 = south pole, 5 = north pole; reference DLWP/custom.py:1057-1070).
 *     `channels_first` (B,C,6,H,W) callers convert with dlwpcs_cf_to_cl / dlwpcs_cl_to_cf.
 *   - dtype: DLWPCS_F32 -- every tensor fp32, arithmetic is exact-fp32 MFMA (v_mfma_f32_32x32x2_f32), fp32 accumulate.
 *            DLWPCS_BF16 -- mixed precision (the reference trains under TF's AMP graph rewrite, Azure/train_cs.py:429):
 *            ACTIVATIONS and their gradients (src*, y, dy, dsrc*, x/dx of the stock ops, mse y/t/dy) are bfloat16 in
 *            HBM; PARAMETERS and their gradients (w_*, b_*, dw_*, db_*, Adam state) stay fp32 master copies; the
 *            contraction runs on v_mfma_f32_32x32x16_bf16 (operands rounded to bf16, fp32 accumulate), every
 *            elementwise kernel computes in fp32 and rounds once on store (round-to-nearest-even).
 *
 * Reference interfaces replaced (paths relative to the reference repository root):
 *   CubeSpherePadding2D.call        DLWP/custom.py:1082-1308   -> dlwpcs_halo_table, dlwpcs_pad_fwd/_bwd
 *   CubeSphereConv2D.call           DLWP/custom.py:921-1002    -> dlwpcs_conv_fwd / _bwd_data / _bwd_weights
 *   ReLU(0.1,10), AveragePooling3D((1,2,2)), UpSampling3D((1,2,2)), concatenate
 *                                   Azure/train_cs.py:197-199,277-305 -> epilogue/loader flags of dlwpcs_conv_*,
 *                                                                 dlwpcs_act_*, dlwpcs_avgpool2_*, dlwpcs_upsample2_*
 *   loss='mse', Adam()              Azure/train_cs.py:424-430  -> dlwpcs_mse_fwd_bwd, dlwpcs_adam_step, dlwpcs_adam_step_fused
 */
#ifndef DLWPCS_H
#define DLWPCS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DLWPCS_VERSION 105            /* 0.1.5: dlwpcs_comm_* / dlwpcs_allreduce_f32, gather-form data gradient by default; the chain launch is gone */

/* error codes */
#define DLWPCS_OK             0
#define DLWPCS_E_INVALID     -1       /* bad argument (shape, flag, null pointer) */
#define DLWPCS_E_UNSUPPORTED -2       /* valid request this build has no kernel for */
#define DLWPCS_E_WORKSPACE   -3       /* workspace too small */
#define DLWPCS_E_LAUNCH      -4       /* HIP launch error */

/* dtype tags */
#define DLWPCS_F32  0
#define DLWPCS_BF16 1                 /* activations / activation gradients stored as bfloat16 (see "dtype" above) */

/* activation tags (epilogue of conv_fwd, mask of the backward kernels) */
#define DLWPCS_ACT_NONE        0
#define DLWPCS_ACT_LEAKY_CLIP  1      /* keras ReLU(negative_slope=alpha, max_value=vmax): Azure/train_cs.py:199 */

typedef void *dlwpcs_stream_t;        /* hipStream_t */

int dlwpcs_version(void);
const char *dlwpcs_last_error(void);

/* ------------------------------------------------------------------------------------------------------------- *
 * Halo tables (HOST functions, no device work).  Replace the slice/reverse/transpose/concat graph of
 * CubeSpherePadding2D.call (DLWP/custom.py:1082-1308) by one gather table.
 * ------------------------------------------------------------------------------------------------------------- */

/* out[6*M*M], M = N+2p: flat source index (face*N + row)*N + col of every padded cell. */
int dlwpcs_halo_table(int N, int p, int32_t *out);

/* inv[6*N*N*4]: for every source cell the up-to-4 EXTRA padded cells (flat index (face*M + i)*M + j) that read
 * it besides its own identity copy at (face, row+p, col+p); unused slots are -1.  (Fan-out <= 5) */
int dlwpcs_halo_inverse_table(int N, int p, int32_t *inv);

/* Gather form of the data gradient (p = 1, 3x3 layers; the adjoint of DLWP/custom.py:1198-1308 folded into the kernel that
 * computes the gradient, SURVEY 2a "cs_conv_dgrad ... with halo scatter folded in").  out[dlwpcs_dgrad_gather_plan_ints(N)]:
 * the inverse table of dlwpcs_halo_inverse_table(N, 1) FIRST (so the buffer serves every call that takes inv_table_dev), then
 * the plan: a data-gradient halo table (the forward's table where the neighbour contributes exactly the term the correlation
 * forms, -1 elsewhere), six source slots per border cell and two weight-id triples per face for the terms it does not (see
 * csrc/halo_table.cpp).  A data-gradient call whose inv_table_dev is such a buffer sets DLWPCS_CONV_DGRAD_GATHER.
 * dlwpcs_dgrad_gather_plan_ints returns 0 for face sizes the plan does not serve (N < 8). */
size_t dlwpcs_dgrad_gather_plan_ints(int N);
int dlwpcs_dgrad_gather_plan(int N, int32_t *out);

/* ------------------------------------------------------------------------------------------------------------- *
 * Stand-alone padding layer, channels_last.  x: (B,6,N,N,C)  y: (B,6,N+2p,N+2p,C)
 * ------------------------------------------------------------------------------------------------------------- */
int dlwpcs_pad_fwd(const void *x, void *y, int B, int N, int C, int p, int dtype,
                   const int32_t *table_dev, dlwpcs_stream_t stream);
/* dx[src] = sum of dy over every padded cell that gathered from src (deterministic inverse gather, no atomics). */
int dlwpcs_pad_bwd(const void *dy, void *dx, int B, int N, int C, int p, int dtype,
                   const int32_t *inv_table_dev, dlwpcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- *
 * Fused cubed-sphere convolution.
 *
 * Virtual input V (B,6,N,N,C0+C1) = concat_channels( up0 ? nearest_upsample_x2(src0) : src0 , src1 ).
 *   halo == 1 : V is halo-padded on the fly through `table` (CubeSpherePadding2D(p=(k-1)/2) fused into the load)
 *               and convolved 'valid' -> y (B,6,N,N,Cout).
 *   halo == 0 : V is consumed as is ('valid'): y (B,6,N-k+1,N-k+1,Cout).  (CubeSphereConv2D on an already padded
 *               tensor, or the 1x1 head.)
 * Weight groups follow CubeSphereConv2D.call (DLWP/custom.py:921-1002): w_eq on faces 0-3, w_pol on face 4,
 * face 5 uses w_np when given (independent_north_pole) else w_pol, with the kernel ROWS reversed when
 * flip_north_pole (== flip -> conv -> flip of the reference for stride 1).  Kernels are HWIO (k,k,Cin,Cout) fp32,
 * biases (Cout,) or NULL.  Epilogue: + bias, then `act`.
 * k in {1,3}, stride 1, dilation 1 (the hot-path configuration, Azure/train_cs.py:200-207); anything else returns
 * DLWPCS_E_UNSUPPORTED and is served by dlwpcs_gconv_*.
 * ------------------------------------------------------------------------------------------------------------- */
/* dlwpcs_conv_desc.flags */
#define DLWPCS_CONV_ACCUMULATE_WGRAD 1   /* bwd_weights ADDS to dw_* / db_* (shared layers, flat gradient buffer) */
#define DLWPCS_CONV_PREPACKED        2   /* conv_fwd: w_eq = wpk_fwd, b_eq = bias_pk (or NULL); conv_bwd_data: w_eq = wpk_bwd,
                                          * all produced by dlwpcs_pack_batch; the other kernel / bias pointers are ignored.
                                          * Without the flag every call re-packs its weights into the workspace. */
#define DLWPCS_CONV_REUSE_DZ         4   /* set on BOTH conv_bwd_weights and the conv_bwd_data call that FOLLOWS it on the
                                          * same stream with the same desc and workspace (act != NONE): where the bf16
                                          * weight-gradient kernel applies it leaves dz = dy * act'(y) in the workspace
                                          * and bwd_data reads that instead of dy and y; otherwise the flag is ignored */
#define DLWPCS_CONV_DEFER_RING0     16   /* conv_bwd_data[_masked], halo, source 0 written directly and not masked: the border
                                          * fix-up launch of source 0 is left out -- dsrc0 holds the interior contributions, the
                                          * halo ring stays in the workspace (dlwpcs_conv_ring_info) and the caller's next pass
                                          * over dsrc0 adds it (dlwpcs_avgpool2_bwd_ring).  Only where dlwpcs_conv_ring_info
                                          * returns 1 for the descriptor; ignored otherwise */
#define DLWPCS_CONV_DGRAD_GATHER    64   /* conv_bwd_data[_masked], halo, k = 3, bf16 with 16-B channel vectors, gradient arriving as dz:
                                          * inv_table_dev is a dlwpcs_dgrad_gather_plan buffer and the data gradient is computed in
                                          * GATHER form on the N x N grid -- every border cell sums the terms of the neighbouring
                                          * faces itself (extra MFMAs on gathered dz rows): no halo ring is written, no fix-up launch
                                          * follows, dlwpcs_conv_ring_info returns 0.  Ignored where the kernel does not apply. */
#define DLWPCS_CONV_OUT_PADDED      32   /* conv_fwd of the pointwise bf16 output layer (k = 1, 32 -> even C_out in 8..32, no halo): y has
                                        * C_out rounded up to a multiple of 8 channels per pixel, the padding written as zeros -- the
                                        * layout a following dlwpcs_conv_fwd takes as its source with c0_valid = C_out (an
                                        * autoregressive rollout feeds the output straight back, Azure/train_cs.py:401-406,
                                        * DLWP/model/models.py:446-454); DLWPCS_E_UNSUPPORTED for any other layer */
#define DLWPCS_CONV_DEFER_REDUCE     8   /* conv_bwd_weights: run the weight-gradient kernel only and leave the per-worker
                                          * partial sums in the workspace (dw_* / db_* are not touched); the caller keeps
                                          * that workspace untouched until it has run dlwpcs_wgrad_reduce_batch over the
                                          * item dlwpcs_conv_wgrad_reduce_item describes (one reduction launch for all
                                          * layers of a backward pass instead of one per layer) */

typedef struct dlwpcs_conv_desc {
    int32_t B;              /* batch */
    int32_t N;              /* face size of the virtual input V */
    int32_t C0, C1;         /* channels of src0 / src1 (C1 = 0: no second source) */
    int32_t Cout;
    int32_t ksize;          /* 1 or 3 */
    int32_t halo;           /* 1: fuse the cube-sphere halo gather, 0: plain 'valid' */
    int32_t up0;            /* 1: src0 is (B,6,N/2,N/2,C0), nearest-upsampled x2 on load */
    int32_t flip_north_pole;
    int32_t act;            /* DLWPCS_ACT_* */
    float   alpha, vmax;    /* parameters of DLWPCS_ACT_LEAKY_CLIP.  For 0 <= alpha <= 1 and vmax > 0 (every activation of the
                             * reference's models) the fused convolution evaluates it as min(max(x, alpha*x), vmax): identical
                             * for all finite and infinite x, and a NaN stays a NaN like in keras' ReLU (the min is
                             * gfx950's NaN-propagating v_minimum3_f32; the select form used for other alpha, by
                             * dlwpcs_act_fwd and by the oracle returns NaN as well).  alpha < 0 or vmax < 0: rejected. */
    int32_t dtype;          /* DLWPCS_F32 | DLWPCS_BF16 (dtype of src*, y, dy, dsrc*; parameters are always fp32) */
    int32_t flags;          /* DLWPCS_CONV_* bits */
    int32_t c0_valid;       /* 0: every channel of src0 is real.  > 0 (C1 must be 0): src0 is stored with C0 channels per
                             * pixel but only the first c0_valid are variables, the rest is zero padding up to the vector
                             * width (7 variables in an 8-channel layout: 16-B loads instead of scalar ones).  The HWIO
                             * kernels and their gradients keep c0_valid input rows; dsrc0 is written with C0 channels,
                             * zeros in the padding. */
} dlwpcs_conv_desc;

size_t dlwpcs_conv_workspace_bytes(const dlwpcs_conv_desc *d);      /* max over fwd / bwd_data / bwd_weights */

/* Weight packing hoisted out of the per-call path: the kernels consume the HWIO fp32 weights in matrix-core fragment
 * order (3 face variants, rounded to bf16 in DLWPCS_BF16 mode).  A model packs ALL its layers with one launch per step
 * (after the optimizer update) and passes the packed buffers with DLWPCS_CONV_PREPACKED.
 * dlwpcs_conv_packed_bytes: size of one packed buffer of the layer described by d (only ksize, C0+C1, Cout, dtype matter).
 * dlwpcs_pack_batch: items_dev is a DEVICE array of n_items descriptors (caller-owned; pointers inside are device
 * pointers); wpk_fwd / wpk_bwd / bias_pk may individually be NULL to skip that output. */
#define DLWPCS_PACK_FWD  0
#define DLWPCS_PACK_BWD  1
#define DLWPCS_PACK_BIAS 2
typedef struct dlwpcs_pack_item {
    const void *w_eq, *w_pol, *w_np;      /* HWIO fp32 kernels (w_np NULL unless independent north pole) */
    const void *b_eq, *b_pol, *b_np;      /* fp32 biases or NULL */
    void *wpk_fwd, *wpk_bwd, *bias_pk;    /* outputs */
    int32_t ksize, Cin, Cout, flip_north_pole, dtype, reserved;
} dlwpcs_pack_item;
size_t dlwpcs_conv_packed_bytes(const dlwpcs_conv_desc *d, int which);
int dlwpcs_pack_batch(const dlwpcs_pack_item *items_dev, int n_items, dlwpcs_stream_t stream);

int dlwpcs_conv_fwd(const dlwpcs_conv_desc *d,
                    const void *src0, const void *src1,
                    const void *w_eq, const void *w_pol, const void *w_np,
                    const void *b_eq, const void *b_pol, const void *b_np,
                    void *y, const int32_t *table_dev,
                    void *workspace, size_t workspace_bytes, dlwpcs_stream_t stream);
/* dlwpcs_conv_fwd + the 2x2 average pooling of its output (AveragePooling3D((1,2,2)) behind the block's last convolution,
 * Azure/train_cs.py:282,287) as a SECOND output y_pooled (B,6,N/2,N/2,Cout): written by the convolution's epilogue where the
 * tiling allows (every consumer wave owns whole pairs of rows: the U-Net levels at N = 48 / 24), by dlwpcs_avgpool2_fwd behind
 * it otherwise -- the same bits either way.  Halo convolutions on even face sizes. */
int dlwpcs_conv_fwd_pool(const dlwpcs_conv_desc *d, const void *src0, const void *src1,
                         const void *w_eq, const void *w_pol, const void *w_np,
                         const void *b_eq, const void *b_pol, const void *b_np,
                         void *y, void *y_pooled, const int32_t *table_dev,
                         void *workspace, size_t workspace_bytes, dlwpcs_stream_t stream);
/* Inference: dlwpcs_conv_fwd of layer `d` + the POINTWISE OUTPUT LAYER `dh` behind it (the U-Net's last 3x3 CubeSphereConv2D
 * and its 1x1 head, Azure/train_cs.py:300-305; reference layer: DLWP/custom.py:921-1002 with kernel_size 1) -- y_head =
 * conv1x1(act(conv(...)))).  Both layers take dlwpcs_pack_batch operands (DLWPCS_CONV_PREPACKED in both descriptors: wpk_fwd /
 * bias_pk and head_wpk_fwd / head_bias_pk; a bias pointer may be NULL).  Where the tiling allows -- bf16, 32 output channels of
 * `d`, a head without activation whose stored rows are 32 channels (C_out = 32, or 25..31 with DLWPCS_CONV_OUT_PADDED in dh->flags:
 * the rollout's 26 = 13 variables x 2 steps) -- the head is FOLDED INTO THE EPILOGUE of the convolution: the tile's activated
 * result, rounded to bf16 as it would have been stored, is contracted with the head's fragments straight out of the accumulators,
 * y is never written (113 MB written + 113 MB read back per pass at C96, batch 32, and a launch) and *fused = 1.  Otherwise the
 * two launches of dlwpcs_conv_fwd run (y holds the layer's output, *fused = 0).  y must be a valid (B,6,No,No,Cout) buffer either
 * way; fused may be NULL.  The folded result differs from the two-launch one only by the summation order inside the head's MFMA
 * (fp32 accumulation in both). */
int dlwpcs_conv_fwd_head(const dlwpcs_conv_desc *d, const void *src0, const void *src1, const void *wpk_fwd,
                         const void *bias_pk, const dlwpcs_conv_desc *dh, const void *head_wpk_fwd,
                         const void *head_bias_pk, void *y, void *y_head, const int32_t *table_dev,
                         void *workspace, size_t workspace_bytes, int *fused, dlwpcs_stream_t stream);

/* Gradients w.r.t. the sources.  dy: gradient w.r.t. the (post-activation) output y; y: the saved forward output
 * (needed when act != NONE: dz = dy * act'(.) is applied on load), NULL otherwise.
 * dsrc0: same shape as src0 (the 2x2 block sum of the upsample adjoint is applied when up0), dsrc1 like src1.
 * Either may be NULL to skip it (first layer).  inv_table_dev from dlwpcs_halo_inverse_table (halo==1 only). */
int dlwpcs_conv_bwd_data(const dlwpcs_conv_desc *d,
                         const void *dy, const void *y,
                         const void *w_eq, const void *w_pol, const void *w_np,
                         void *dsrc0, void *dsrc1, const int32_t *inv_table_dev,
                         void *workspace, size_t workspace_bytes, dlwpcs_stream_t stream);

/* Pre-masked gradient convention (training steps of a network whose activations are fused into the convolutions): the
 * gradient w.r.t. the OUTPUT y of an activated layer is multiplied by act'(y) where it is PRODUCED -- by the data-gradient
 * call of the layer that consumes y, by the pooling / loss kernels -- so that the layer itself receives dz = dy * act'(y):
 * neither its data gradient nor its weight gradient reads y again, and no dz hand-over is written.
 *   dz       gradient w.r.t. this layer's PRE-activation output (act / alpha / vmax of d are ignored)
 *   m0, m1   NULL, or the source tensors themselves (src0 / src1 of the forward call: outputs of activated layers with
 *            ReLU(negative_slope = m_alpha, max_value = m_vmax)): dsrc0 / dsrc1 come out multiplied by act'(m0) / act'(m1).
 * The multiply happens in the direct-store epilogue of the matrix-core kernel and in the ring fix-up / inverse-gather
 * kernels; shapes those do not serve get one elementwise launch inside the call.  Otherwise like dlwpcs_conv_bwd_data. */
int dlwpcs_conv_bwd_data_masked(const dlwpcs_conv_desc *d, const void *dz,
                                const void *w_eq, const void *w_pol, const void *w_np,
                                void *dsrc0, void *dsrc1, const void *m0, const void *m1, float m_alpha, float m_vmax,
                                const int32_t *inv_table_dev,
                                void *workspace, size_t workspace_bytes, dlwpcs_stream_t stream);

/* The SMALL-FACE kernel behind the same parameter records: bf16, k = 3, halo, one source (C1 = 0, no up0, no c0_valid), faces of
 * N * N <= 320 cells (the coarsest U-Net level, N = 12), C0 and C_out multiples of 32.  One workgroup per (sample, face, 32 output
 * channels) holds the whole haloed face in LDS, several workgroups per CU -- where the persistent kernel of dlwpcs_conv_fwd /
 * dlwpcs_conv_bwd_data_masked runs a single under-filled tile per workgroup.  The same arithmetic in the same order: y, dsrc0 and
 * the halo ring in the workspace are bitwise what those calls produce (DLWPCS_CONV_DEFER_RING0 / dlwpcs_conv_ring_info apply
 * unchanged).  dlwpcs_conv_small_bwd_data takes the gradient as dz like dlwpcs_conv_bwd_data_masked (dsrc1 / m1 must be NULL).
 * Every other request returns DLWPCS_E_UNSUPPORTED and has launched nothing: the caller falls back to the general entry point.
 * Not bracketed by the opt-in launch profiler. */
int dlwpcs_conv_small_fwd(const dlwpcs_conv_desc *d,
                          const void *src0, const void *src1,
                          const void *w_eq, const void *w_pol, const void *w_np,
                          const void *b_eq, const void *b_pol, const void *b_np,
                          void *y, const int32_t *table_dev,
                          void *workspace, size_t workspace_bytes, dlwpcs_stream_t stream);
int dlwpcs_conv_small_bwd_data(const dlwpcs_conv_desc *d, const void *dz,
                               const void *w_eq, const void *w_pol, const void *w_np,
                               void *dsrc0, void *dsrc1, const void *m0, const void *m1, float m_alpha, float m_vmax,
                               const int32_t *inv_table_dev,
                               void *workspace, size_t workspace_bytes, dlwpcs_stream_t stream);

/* 1 if a data-gradient call on d with DLWPCS_CONV_DEFER_RING0 defers the fix-up of source 0; then *dxv_offset = byte offset of
 * the padded gradient (B,6,N+2,N+2,channels) inside that call's workspace and *channels = C0 + C1 (source 0 = the first C0). */
int dlwpcs_conv_ring_info(const dlwpcs_conv_desc *d, size_t *dxv_offset, int *channels);

/* Gradients w.r.t. kernels and biases (deterministic: fixed-order partial sums, no atomics).
 * dw_*: HWIO like the kernels; db_*: (Cout,) or NULL.  dw_np/db_np NULL unless independent north pole. */
int dlwpcs_conv_bwd_weights(const dlwpcs_conv_desc *d,
                            const void *src0, const void *src1, const void *dy, const void *y,
                            void *dw_eq, void *dw_pol, void *dw_np,
                            void *db_eq, void *db_pol, void *db_np,
                            const int32_t *table_dev,
                            void *workspace, size_t workspace_bytes, dlwpcs_stream_t stream);

/* Deferred, batched reduction of the per-worker partial sums (DLWPCS_CONV_DEFER_REDUCE).
 * dlwpcs_conv_wgrad_reduce_item (host only, launches nothing): fills *item with what the reduction of the layer
 * described by d needs — the same d (flags included: ACCUMULATE_WGRAD decides add vs overwrite), destinations and
 * workspace as the dlwpcs_conv_bwd_weights call that produced the partials.  `nblocks` is the item's share of the launch.
 * dlwpcs_wgrad_reduce_batch: items_dev is a DEVICE copy of the n_items host items (the host copy supplies the launch
 * geometry; both must hold the same items).
 * Items whose destinations overlap (a layer applied twice) must all carry ACCUMULATE_WGRAD: items run concurrently,
 * every destination element is owned by one thread per item, so overlapping items are only safe as atomics-free adds
 * when the caller serialises them — put them in separate launches.  Bitwise reproducible like the per-layer path
 * (same fixed summation order). */
typedef struct dlwpcs_reduce_item {
    const float *partial, *bpartial;                       /* inside the layer's workspace */
    float *dw_eq, *dw_pol, *dw_np, *db_eq, *db_pol, *db_np;
    int32_t ksize, Cin, Cout, CinP, CoutP, n_eq, n_4, n_5, flip_north_pole, accumulate, vec, nblocks;
    int32_t reserved[4];
} dlwpcs_reduce_item;
int dlwpcs_conv_wgrad_reduce_item(const dlwpcs_conv_desc *d,
                                  void *dw_eq, void *dw_pol, void *dw_np,
                                  void *db_eq, void *db_pol, void *db_np,
                                  void *workspace, size_t workspace_bytes, dlwpcs_reduce_item *item);
int dlwpcs_wgrad_reduce_batch(const dlwpcs_reduce_item *items_dev, const dlwpcs_reduce_item *items_host, int n_items,
                              dlwpcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- *
 * Batched weight gradients: ONE persistent launch for every layer of a backward pass (DLWPCS_BF16 hot-path shapes).
 * The weight gradient of a layer needs only the layer's saved inputs and dz, the gradient w.r.t. its PRE-activation
 * output, so nothing in the backward chain waits for it: a training step queues one item per layer and runs them
 * together after the last data gradient.  The host plan cuts the joint work list of all layers into one equal-cost
 * chain per compute unit (a layer gets workers in proportion to its work, few partial sums), the reduction adds the
 * partial sums in a fixed order (bitwise reproducible) and ACCUMULATES into dw_* / db_* (shared layers add up;
 * the caller zeroes the gradient buffer once per step).  Replaces n_items calls of dlwpcs_conv_bwd_weights.
 *
 *   dz          (B,6,No,No,Cout) bf16: dy * act'(y) already applied by whoever produced the gradient
 *               (dlwpcs_conv_bwd_data_masked, dlwpcs_avgpool2_bwd_add_masked, ...); act / alpha / vmax / flags of d are
 *               ignored
 *   plan        built on the HOST from the descriptors (and from which of the bias / north-pole pointers are non-NULL);
 *               holds geometry only -- every tensor address travels by value in the kernel arguments, so one plan (and
 *               its device copy, which the caller makes once) serves every step and a captured hipGraph keeps replaying
 *               the addresses it was captured with.
 * dlwpcs_wgrad_batch_supported: 1 if the layer described by d can be an item (others use dlwpcs_conv_bwd_weights).
 * ------------------------------------------------------------------------------------------------------------- */
#define DLWPCS_WGRAD_BATCH_MAX 24
typedef struct dlwpcs_wgrad_item {
    dlwpcs_conv_desc d;
    const void *src0, *src1;              /* the layer's saved inputs (src1 NULL when C1 == 0) */
    const void *dz;
    const void *y;                        /* NULL: dz is pre-masked.  Else (3x3 kernels, d.act = LEAKY_CLIP): `dz` holds the plain
                                           * gradient dy and y the layer's saved output; the kernel forms dy * act'(y) on load */
    const int32_t *table_dev;             /* halo table (halo == 1) */
    void *dw_eq, *dw_pol, *dw_np;         /* fp32 HWIO, accumulated into; dw_np NULL unless independent north pole */
    void *db_eq, *db_pol, *db_np;         /* fp32 (Cout,) or NULL */
} dlwpcs_wgrad_item;
int dlwpcs_wgrad_batch_supported(const dlwpcs_conv_desc *d);
int dlwpcs_wgrad_batch_sizes(const dlwpcs_wgrad_item *items, int n_items, size_t *plan_bytes, size_t *workspace_bytes);
int dlwpcs_wgrad_batch_plan(const dlwpcs_wgrad_item *items, int n_items, void *plan_host, size_t plan_bytes);
int dlwpcs_wgrad_batch(const dlwpcs_wgrad_item *items, int n_items, const void *plan_host, const void *plan_dev,
                       void *workspace, size_t workspace_bytes, dlwpcs_stream_t stream);
/* The same with the optimizer fused into the reduction (one launch less, the gradients never travel through HBM again):
 * every dw_* / db_* must be a view into the flat gradient buffer g (n floats); p, m, v are the flat parameter / Adam-state
 * buffers with the same offsets.  A reduced element is consumed on the spot: g' = (g[i] + sum of partial sums) *
 * grad_scale -> the Adam update of dlwpcs_adam_step_dev (same arithmetic, same bits) -> g[i] = 0.  Elements of g that no
 * item covers are NOT updated (alignment padding; a caller with parameters outside the items uses dlwpcs_wgrad_batch +
 * dlwpcs_adam_step_dev instead).  state_dev = {t - 1, ticket} as for dlwpcs_adam_step_fused (the weight-gradient launch
 * increments t, the reduction reads it), hyper_dev = {lr, beta1, beta2, eps, grad_scale}.  Items that share their gradient
 * tensors (a layer applied twice: integration_steps = 2, /root/reference/Azure/train_cs.py:391-408) must share ALL of them; they are
 * reduced in successive launches and the optimizer consumes a tensor in the launch of its LAST item (round 6; rounds 3-5 rejected
 * such lists with DLWPCS_E_UNSUPPORTED and the caller ran reduction, optimizer and operand packing as launches of their own). */
int dlwpcs_wgrad_batch_adam(const dlwpcs_wgrad_item *items, int n_items, const void *plan_host, const void *plan_dev,
                            void *workspace, size_t workspace_bytes, float *p, float *g, float *m, float *v, size_t n,
                            int32_t *state_dev, const float *hyper_dev, dlwpcs_stream_t stream);
/* ... and what else ends a training step, in the same launch:
 *  tail != NULL: the deferred second stage of the fused head's loss (DLWPCS_HEAD_DEFER_STAGE2);
 *  pack_items_host != NULL (HOST array, one dlwpcs_pack_item per gradient item, same order; bf16): every updated parameter is also
 *  written -- rounded to bf16 -- into its places in the layer's packed operands (wpk_fwd / wpk_bwd / bias_pk, the outputs of
 *  dlwpcs_pack_batch), so that the next pass needs no packing launch.  The packed buffers must hold a full dlwpcs_pack_batch
 *  result already (the zero padding is not rewritten); w_eq of pack item i must be the parameter tensor that dw_eq of gradient
 *  item i belongs to (same offset in p as dw_eq has in g). */
struct dlwpcs_loss_tail;
int dlwpcs_wgrad_batch_adam_tail(const dlwpcs_wgrad_item *items, int n_items, const void *plan_host, const void *plan_dev,
                                 void *workspace, size_t workspace_bytes, float *p, float *g, float *m, float *v, size_t n,
                                 int32_t *state_dev, const float *hyper_dev, const struct dlwpcs_loss_tail *tail,
                                 const dlwpcs_pack_item *pack_items_host, dlwpcs_stream_t stream);

/* The data-parallel form of the step's last launch (reference counterpart: the multi-GPU model of DLWP/model/models.py:369-374,
 * one optimizer step on the gradient of the GLOBAL batch): dlwpcs_wgrad_batch leaves the finished local gradients in g, the
 * caller sums g over the ranks (RCCL all-reduce of the flat buffer), and this ONE launch then does what dlwpcs_wgrad_batch_adam_tail
 * does after its reduction -- g * grad_scale -> Adam (same arithmetic, same bits) -> g = 0, packed bf16 operands refreshed, loss
 * tail -- without reading any partial sum.  The items name the gradient tensors (dw_* / db_*: views into g) and the plan gives
 * their geometry; src / dz / table pointers are ignored.  state_dev = {t, ticket}: this launch computes with t + 1 and its last
 * workgroup stores it (the form of dlwpcs_adam_step_fused), so no earlier launch has to move the counter. */
int dlwpcs_wgrad_batch_apply(const dlwpcs_wgrad_item *items, int n_items, const void *plan_host, const void *plan_dev,
                             float *p, float *g, float *m, float *v, size_t n, int32_t *state_dev, const float *hyper_dev,
                             const struct dlwpcs_loss_tail *tail, const dlwpcs_pack_item *pack_items_host, dlwpcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- *
 * Generic (any kernel size / stride / dilation / 'same') per-face convolution on an ALREADY PADDED channels_last
 * tensor: the off-hot-path options of CubeSphereConv2D (DLWP/custom.py:824-842).  Direct VALU kernels.
 * x: (B,6,H,W,Cin) -> y: (B,6,Ho,Wo,Cout);  pad_{t,l}: zero padding already resolved by the caller ('same').
 * Weight groups: faces 0-3 use w_eq / b_eq, face 4 w_pol / b_pol; face 5 uses w_np if given, else w_pol, and -- chosen
 * separately -- b_np if given, else b_pol.  b_eq and b_pol are both given or both null (no bias; b_np is then ignored).
 * dlwpcs_gconv_bwd_weights is the adjoint of exactly that rule: face 5's kernel gradient goes to dw_np if given, else it is
 * summed into dw_pol; face 5's bias gradient goes to db_np if given, else it is summed into db_pol, whether or not dw_np is
 * given.  db_eq and db_pol are both given or both null (no bias gradient is computed), db_np only together with them;
 * anything else is DLWPCS_E_INVALID.  Every tensor that is given is written completely, a null one is not touched.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct dlwpcs_gconv_desc {
    int32_t B, H, W, Cin, Cout;
    int32_t kh, kw, sh, sw, dh, dw;
    int32_t pad_t, pad_l;   /* zero padding before the first row / column ('same'), 0 for 'valid' */
    int32_t Ho, Wo;
    int32_t flip_north_pole;
    int32_t dtype;
} dlwpcs_gconv_desc;

int dlwpcs_gconv_fwd(const dlwpcs_gconv_desc *d, const void *x,
                     const void *w_eq, const void *w_pol, const void *w_np,
                     const void *b_eq, const void *b_pol, const void *b_np, void *y, dlwpcs_stream_t stream);
int dlwpcs_gconv_bwd_data(const dlwpcs_gconv_desc *d, const void *dy,
                          const void *w_eq, const void *w_pol, const void *w_np, void *dx, dlwpcs_stream_t stream);
int dlwpcs_gconv_bwd_weights(const dlwpcs_gconv_desc *d, const void *x, const void *dy,
                             void *dw_eq, void *dw_pol, void *dw_np, void *db_eq, void *db_pol, void *db_np,
                             dlwpcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- *
 * Keras stock ops between the custom layers (Azure/train_cs.py:197-199), channels_last, n = element count.
 * ------------------------------------------------------------------------------------------------------------- */
int dlwpcs_act_fwd(const void *x, void *y, size_t n, int act, float alpha, float vmax, int dtype,
                   dlwpcs_stream_t stream);
/* dx = dy * act'(.) evaluated from the saved OUTPUT y */
int dlwpcs_act_bwd(const void *dy, const void *y, void *dx, size_t n, int act, float alpha, float vmax, int dtype,
                   dlwpcs_stream_t stream);
/* x: (B,6,N,N,C) -> y: (B,6,N/2,N/2,C), 2x2 mean;  backward spreads dy/4 */
int dlwpcs_avgpool2_fwd(const void *x, void *y, int B, int N, int C, int dtype, dlwpcs_stream_t stream);
int dlwpcs_avgpool2_bwd(const void *dy, void *dx, int B, int N, int C, int dtype, dlwpcs_stream_t stream);
/* dx = dskip + avgpool2_bwd(dy): the pooled tensor also feeds a skip connection whose gradient is dskip (N,N like dx);
 * one pass instead of avgpool2_bwd + add.  dx may alias dskip. */
int dlwpcs_avgpool2_bwd_add(const void *dy, const void *dskip, void *dx, int B, int N, int C, int dtype,
                            dlwpcs_stream_t stream);
/* Pre-masked gradients: dx = act'(m) * (dskip + avgpool2_bwd(dy)); m = the pooled tensor itself (output of an activated layer,
 * ReLU(m_alpha, m_vmax)), dskip may be NULL (no skip connection).  dx may alias dskip. */
int dlwpcs_avgpool2_bwd_masked(const void *dy, const void *dskip, const void *m, void *dx, int B, int N, int C,
                               float m_alpha, float m_vmax, int dtype, dlwpcs_stream_t stream);
/* The same, with dy = the pooled tensor's gradient as a data-gradient call with DLWPCS_CONV_DEFER_RING0 left it: the ring cells
 * (`ring` = that call's workspace + dxv_offset, `ring_channels` per cell, the pooled tensor's window starting at `ring_choff`;
 * inv_half_dev = dlwpcs_halo_inverse_table(N/2, 1)) are added to the border cells of the N/2 grid on the fly.  m may be NULL
 * here (no mask: plain pooling adjoint + fix-up). */
int dlwpcs_avgpool2_bwd_ring(const void *dy, const void *dskip, const void *m, void *dx, int B, int N, int C,
                             float m_alpha, float m_vmax, int dtype, const void *ring, const int32_t *inv_half_dev,
                             int ring_channels, int ring_choff, dlwpcs_stream_t stream);
/* x: (B,6,N,N,C) -> y: (B,6,2N,2N,C), nearest;  backward sums 2x2 blocks */
int dlwpcs_upsample2_fwd(const void *x, void *y, int B, int N, int C, int dtype, dlwpcs_stream_t stream);
int dlwpcs_upsample2_bwd(const void *dy, void *dx, int B, int N, int C, int dtype, dlwpcs_stream_t stream);
/* y[:, :Ca] = a, y[:, Ca:] = b over `rows` pixels;  split is the adjoint */
int dlwpcs_concat2(const void *a, const void *b, void *y, size_t rows, int Ca, int Cb, int dtype,
                   dlwpcs_stream_t stream);
int dlwpcs_split2(const void *y, void *a, void *b, size_t rows, int Ca, int Cb, int dtype, dlwpcs_stream_t stream);
/* Channel padding for dlwpcs_conv_desc.c0_valid: y (rows, Cp) <- x (rows, C), zeros in channels C..Cp-1; slice is the adjoint
 * (x (rows, C) <- the first C channels of y (rows, Cp)). */
int dlwpcs_pad_channels(const void *x, void *y, size_t rows, int C, int Cp, int dtype, dlwpcs_stream_t stream);
int dlwpcs_slice_channels(const void *y, void *x, size_t rows, int Cp, int C, int dtype, dlwpcs_stream_t stream);
/* Rollout state re-injection (replaces the per-step numpy concatenate / transpose / reshape of the reference's
 * TimeSeriesEstimator.predict, DLWP/model/extensions.py:281-299, and the Reshape / Permute / Concatenate chain of
 * Azure/train_cs.py:401-406): out (B,S,T*(V+E)) <- state (B,S,T*V) with extra (B,T,S,E) appended as the last E channels of
 * every one of the T time steps.  All three tensors have element type `dtype`. */
int dlwpcs_state_repack(const void *state, const void *extra, void *out, int B, size_t S, int T, int V, int E,
                        int dtype, dlwpcs_stream_t stream);
/* layout converters for data_format='channels_first' callers: (B,C,S) <-> (B,S,C), S = 6*H*W */
int dlwpcs_cf_to_cl(const void *x, void *y, int B, int C, size_t S, int dtype, dlwpcs_stream_t stream);
int dlwpcs_cl_to_cf(const void *x, void *y, int B, int C, size_t S, int dtype, dlwpcs_stream_t stream);
/* y = a + b (gradient accumulation at skip connections / shared weights) */
int dlwpcs_add(const void *a, const void *b, void *y, size_t n, int dtype, dlwpcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- *
 * Training-step tail (Azure/train_cs.py:424-430): keras 'mse' with a loss weight, metric 'mae', and Adam.
 * ------------------------------------------------------------------------------------------------------------- */
/* loss_out[0] += weight*mean((y-t)^2), loss_out[1] += mean(|y-t|);  dy = weight*2*(y-t)/n  (dy may be NULL).
 * scratch: >= dlwpcs_mse_scratch_bytes() bytes.  Deterministic two-stage reduction, fp32 arithmetic.
 * dtype = dtype of y and dy; t has the same dtype unless DLWPCS_MSE_TARGET_F32 is OR-ed in (bf16 prediction scored
 * against the fp32 target, as TF's AMP does: the loss is computed in fp32). */
#define DLWPCS_MSE_TARGET_F32 0x100
#define DLWPCS_MSE_OVERWRITE  0x200   /* OR-ed into dtype: loss_out[0..1] = ... instead of +=  (loss_out need not be zeroed) */
size_t dlwpcs_mse_scratch_bytes(void);
int dlwpcs_mse_fwd_bwd(const void *y, const void *t, void *dy, float *loss_out, size_t n, float weight, int dtype,
                       void *scratch, dlwpcs_stream_t stream);
/* TF2.1-keras Adam on flat fp32 buffers: lr_t = lr*sqrt(1-b2^t)/(1-b1^t); p -= lr_t*m/(sqrt(v)+eps).
 * `step_dev` points to a device int32 holding t-1 (incremented by the kernel), so the call is graph-capturable.
 * grad_scale multiplies g first (1/world_size after a sum all-reduce). */
/* Fused training tail (bf16): pointwise output layer (k = 1, 32 -> even C_out in 8..32, Azure/train_cs.py:228) + 'mse' loss
 * (+ 'mae') against the fp32 target + loss gradient dy (bf16, what the head's weight gradient reads) + the head's data
 * gradient dx (bf16, (B,6,N,N,32)) in one pass: replaces dlwpcs_conv_fwd + dlwpcs_mse_fwd_bwd + dlwpcs_conv_bwd_data of the
 * output layer; the prediction itself is not written.  wpk_fwd / bias_pk / wpk_bwd are dlwpcs_pack_batch outputs;
 * loss_out[0] = weight * mse, loss_out[1] = mae (overwrite != 0: assigned, else added); scratch >= dlwpcs_head_mse_scratch_bytes(). */
size_t dlwpcs_head_mse_scratch_bytes(void);
/* OR-ed into `overwrite`: the launch that finishes the loss (second stage of its reduction) is left to the caller --
 * dlwpcs_head_mse_tail describes it; dlwpcs_loss_tail_run runs it as a launch of its own, dlwpcs_wgrad_batch_adam_tail as one
 * extra workgroup of the weight-gradient reduction that ends the training step (same code, same bits). */
#define DLWPCS_HEAD_DEFER_STAGE2 2
typedef struct dlwpcs_loss_tail {
    const float *partial;        /* the scratch of dlwpcs_head_mse_step: [nblocks][2] workgroup sums */
    float *loss_out;
    int nblocks;
    float inv_n, weight;
    int overwrite;
} dlwpcs_loss_tail;
int dlwpcs_head_mse_tail(const dlwpcs_conv_desc *d, float weight, int overwrite, void *scratch, float *loss_out,
                         dlwpcs_loss_tail *tail);
int dlwpcs_loss_tail_run(const dlwpcs_loss_tail *tail, dlwpcs_stream_t stream);
int dlwpcs_head_mse_step(const dlwpcs_conv_desc *d, const void *x, const void *wpk_fwd, const void *bias_pk,
                         const void *wpk_bwd, const float *target, float weight, void *dy, void *dx, float *loss_out,
                         int overwrite, void *scratch, dlwpcs_stream_t stream);

/* The same with dx multiplied by act'(x; m_alpha, m_vmax): x is the output of an activated layer that expects its gradient
 * pre-masked (see dlwpcs_conv_bwd_data_masked). */
int dlwpcs_head_mse_step_masked(const dlwpcs_conv_desc *d, const void *x, const void *wpk_fwd, const void *bias_pk,
                                const void *wpk_bwd, const float *target, float weight, void *dy, void *dx, float *loss_out,
                                int overwrite, void *scratch, float m_alpha, float m_vmax, dlwpcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- *
 * Training losses of the reference's DLWP/custom.py:1543-1676 (and keras 'mae'), with their gradient.
 * ------------------------------------------------------------------------------------------------------------- */
#define DLWPCS_LOSS_MSE 0            /* weight * mean((w*(y-t))^2)                           keras mean_squared_error */
#define DLWPCS_LOSS_MAE 1            /* weight * mean(|w*(y-t)|)                              keras mean_absolute_error */
#define DLWPCS_LOSS_ACC 2            /* weight * anomaly-correlation loss of w*y, w*t against the climatology c */
#define DLWPCS_REG_NONE   0          /* regularize_mean of the anomaly-correlation loss */
#define DLWPCS_REG_MSE    1
#define DLWPCS_REG_MAE    2
#define DLWPCS_REG_GLOBAL 3
/* Fields are fp32 device arrays indexed by the flat element index e of y:  field[(e / div) % period].  A field that is constant
 * along the channels of a channels_last tensor is stored per cell (div = C, period = 6*N*N); a field of one sample's shape has
 * div = 1, period = the sample's element count.  weight / clim NULL: w = 1 / c = 0.  (The latitude-weighted loss of the reference
 * scores w*y against w*t: the weight enters an MSE squared.) */
typedef struct dlwpcs_loss_desc {
    int kind;                    /* DLWPCS_LOSS_* */
    float loss_weight;           /* keras loss_weights entry */
    const float *weight;         /* latitude weight field w, or NULL */
    int weight_div, weight_period;
    const float *clim;           /* climatology c (DLWPCS_LOSS_ACC), or NULL */
    int clim_div, clim_period;
    int regularize;              /* DLWPCS_REG_* (DLWPCS_LOSS_ACC) */
    int reverse;                 /* DLWPCS_LOSS_ACC: nonzero -> m - a / -a, else a - m / a */
    int overwrite;               /* bit 0: loss_out = ... instead of +=;  DLWPCS_HEAD_DEFER_STAGE2 (head step only) */
} dlwpcs_loss_desc;
/* loss_out[0] (+)= the loss, loss_out[1] (+)= mean(|y-t|) (the unweighted 'mae' metric); dy = d loss_out[0] / dy (may be NULL).
 * dtype as for dlwpcs_mse_fwd_bwd (DLWPCS_MSE_TARGET_F32 may be OR-ed in).  n < 2^32.  scratch >= dlwpcs_loss_scratch_bytes().
 * Deterministic; no host synchronisation (the anomaly-correlation gradient coefficients stay in device memory). */
size_t dlwpcs_loss_scratch_bytes(void);
int dlwpcs_loss_fwd_bwd(const dlwpcs_loss_desc *L, const void *y, const void *t, void *dy, float *loss_out, size_t n,
                        int dtype, void *scratch, dlwpcs_stream_t stream);
/* Masked losses: dlwpcs_loss_fwd_bwd for targets with holes (DLWPCS_LOSS_MSE / DLWPCS_LOSS_MAE, with or without a weight field).
 *   hole     element e is a hole iff t[e] != t[e] after widening to fp32: any NaN payload, either sign; +-inf is data (the
 *            convention of dlwpcs_missing_count).  y is never inspected.
 *   sums     at a hole d = y - t is replaced by 0 by a SELECT (not a multiplication) before the element's arithmetic, so a NaN
 *            or inf y[e] at a hole reaches neither sum; everywhere else the arithmetic is dlwpcs_loss_fwd_bwd's.
 *   dy       at a hole +0.0 is stored (a select again); elsewhere gscale * (the plain gradient term).
 *   count    the number of non-holes, an exact integer (uint32 per lane, added over the workgroup in a fixed order, one uint32 per
 *            workgroup in the scratch, added by the second stage).  valid_out[0] = count whenever valid_out is given.
 *   result   loss_out[0] (+)= loss_weight * S0 / D, loss_out[1] (+)= S1 / D with S0 / S1 the sums of the loss terms / of |d| and
 *            D = n (DLWPCS_NORM_ALL: a hole contributes 0, as if y == t there) or D = count (DLWPCS_NORM_VALID: a nan-mean).  The
 *            weighted forms divide by the same D, not by sum w (the reference's weight field has mean 1).
 *            count == 0: both results are 0 (not NaN) and dy is +0.0 everywhere.
 * L, dtype (DLWPCS_MSE_TARGET_F32 included), loss_out and L->overwrite bit 0 as for dlwpcs_loss_fwd_bwd; scratch >=
 * dlwpcs_loss_scratch_bytes(); dy and valid_out may be NULL.  Refused with nothing written: DLWPCS_LOSS_ACC, a climatology, an
 * unknown `normalize`, n >= 2^32.
 * Launches (none synchronises with the host, no atomics): the first stage has dlwpcs_loss_fwd_bwd's geometry -- the 8-wide kernel
 * when n % 8 == 0 and y, t, dy sit on 32-byte boundaries, min(ceil(items / 256), 1024) workgroups, the same lane -> element map,
 * fp32 lane sums and workgroup tree -- and the second is one workgroup in fp64.
 *   NORM_ALL    two launches; gscale = loss_weight * 2 / (float)n (MSE; loss_weight / (float)n for MAE) is formed on the host and
 *               the first stage writes dy; inv_n = 1.f / (float)n.  Bit for bit dlwpcs_loss_fwd_bwd on copies of y and t with
 *               zeros written at the holes.
 *   NORM_VALID  three launches; the first stage writes no dy, the second forms inv = (float)(1.0 / (double)(float)count) and
 *               gscale = (float)((double)(loss_weight * 2.f) / (double)(float)count) (loss_weight for MAE) in device memory (an
 *               fp64 quotient of two fp32 values rounded once to fp32 is the correctly rounded fp32 quotient: without holes these
 *               are the bits the plain call forms on the host, and so are loss_out and dy), and a third launch of at most 2048
 *               workgroups writes dy. */
#define DLWPCS_NORM_ALL   0   /* divide by n: a hole contributes 0, as if y == t there */
#define DLWPCS_NORM_VALID 1   /* divide by the number of valid elements (a nan-mean) */
int dlwpcs_loss_masked_fwd_bwd(const dlwpcs_loss_desc *L, const void *y, const void *t, int normalize,
                               void *dy, float *loss_out, uint32_t *valid_out, size_t n, int dtype,
                               void *scratch, dlwpcs_stream_t stream);
/* dlwpcs_head_mse_step(_masked) for DLWPCS_LOSS_MSE / DLWPCS_LOSS_MAE with an optional per-cell weight field (weight_div = C_out,
 * weight_period = 6*N*N); mask_dx != 0: the masked form.  The deferred tail is described by dlwpcs_head_mse_tail as before. */
int dlwpcs_head_loss_step(const dlwpcs_conv_desc *d, const dlwpcs_loss_desc *L, const void *x, const void *wpk_fwd,
                          const void *bias_pk, const void *wpk_bwd, const float *target, void *dy, void *dx, float *loss_out,
                          void *scratch, int mask_dx, float m_alpha, float m_vmax, dlwpcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- *
 * Forecast verification (reference DLWP/verify.py:18-164: forecast_error, persistence_error, climo_error).  ONE fp32 strided
 * reduction: operand 0 = a (the forecast x), 1 = b (the verification y), 2 = c (climatology, NULL -> 0), 3 = w (weights,
 * NULL -> 1), all fp32 device arrays addressed in ELEMENTS by per-operand strides (0 = broadcast).  For every output
 * (lead f < n_lead, kept index o over keep_ext[], channel k < kc) it reduces every t < n_f = clamp(min(t_len, t_cap - t_slope*f), 0)
 * and every reduced index r over red_ext[] (the last reduced dim is the row the lanes stream along):
 *   a[f*lead_stride[0] + t*t_stride[0] + o.keep_stride[0] + r.red_stride[0] + k*kc_stride[0]]   (likewise b, c, w)
 * Outputs are stored row-major over (f, keep..., k), fp64 (out_f32 = 0) or fp32.  Per method, each term counts its own
 * non-NaN entries (np.nanmean of each factor) and an empty count gives NaN:
 *   MSE / RMSE: nanmean(w*d^2) (sqrt), d = y - x      MAE: nanmean(|d*w|)
 *   ACC: nanmean(w*av*af) / sqrt(nanmean(w*av^2) * nanmean(w*af^2)),  av = y - c, af = x - c
 *   COS: sum(af*av*w) / (|af*w| * |av*w|), no NaN skipping          MEAN: nanmean(y) (a ignored)
 * kc (1, 2 or 4) is the kept innermost channel axis handled inside a workgroup (per-variable scores of channels_last data).
 * At most two launches, no atomics (fixed-order slab partials), bitwise reproducible, no host synchronisation.
 * scratch >= dlwpcs_score_scratch_bytes(d) (0 when the first launch finishes the outputs itself).
 * ------------------------------------------------------------------------------------------------------------- */
#define DLWPCS_SCORE_MSE  0
#define DLWPCS_SCORE_RMSE 1
#define DLWPCS_SCORE_MAE  2
#define DLWPCS_SCORE_ACC  3
#define DLWPCS_SCORE_COS  4
#define DLWPCS_SCORE_MEAN 5
#define DLWPCS_SCORE_MAX_DIMS 8
typedef struct dlwpcs_score_desc {
    int32_t method;              /* DLWPCS_SCORE_* */
    int32_t n_lead;
    int32_t t_len, t_cap, t_slope;
    int32_t n_keep, n_red, kc;
    int64_t keep_ext[DLWPCS_SCORE_MAX_DIMS];
    int64_t red_ext[DLWPCS_SCORE_MAX_DIMS];
    int64_t lead_stride[4], t_stride[4], kc_stride[4];
    int64_t keep_stride[4][DLWPCS_SCORE_MAX_DIMS];
    int64_t red_stride[4][DLWPCS_SCORE_MAX_DIMS];
} dlwpcs_score_desc;
size_t dlwpcs_score_scratch_bytes(const dlwpcs_score_desc *d);
int dlwpcs_score(const dlwpcs_score_desc *d, const float *a, const float *b, const float *c, const float *w, void *out,
                 int out_f32, void *scratch, size_t scratch_bytes, dlwpcs_stream_t stream);
/* The same reduction with ONE operand looked up by row instead of laid out over (lead, time): the climatology -- operand c of
 * ACC / COS, operand a of MSE / RMSE / MAE (the error of a climatology forecast) -- is a (K, inner...) table, and for lead f
 * and time t its row is row_dev[f * t_len + t] (int32 on the device, one load per (f, t) row); its offset is row * table_row_stride plus the kept / reduced / channel strides of the descriptor as
 * before, and its lead_stride and t_stride must be 0.  Same plan, same partial-sum slabs, same order: the result is bitwise
 * that of dlwpcs_score on the materialised (n_lead, t_len, inner...) operand.  Scratch as for dlwpcs_score.  The kernel TRUSTS
 * the table: every entry that is read lies in [0, K).  DLWPCS_SCORE_MEAN is refused. */
int dlwpcs_score_indexed(const dlwpcs_score_desc *d, const float *a, const float *b, const float *c, const float *w,
                         const int32_t *row_dev, int64_t table_row_stride, void *out, int out_f32,
                         void *scratch, size_t scratch_bytes, dlwpcs_stream_t stream);
/* Which code dlwpcs_score (indexed = 0) or dlwpcs_score_indexed (indexed != 0) would run for these arguments.  Host only: no
 * launch, no device call; the pointers are looked at for NULL and for 16-byte alignment and never dereferenced.  info[0] = the
 * kernel form (0: a workgroup per output group, one element per lane and load; 1: the same with 16-byte loads of a and b; 2: one
 * lane per output), info[1] = slabs per group (> 1: partial sums in scratch and a second launch), info[2] / info[3] = how the
 * 16-byte form reads c / w (-1: operand absent, 0: element by element, 1: 16-byte loads, 2: one load per cell of 4 channels),
 * info[4] / info[5] = the grid of the first launch, info[6] = info[7] = 0.  Returns what the entry point would return for the
 * same descriptor and operands. */
int dlwpcs_score_plan_info(const dlwpcs_score_desc *d, const void *a, const void *b, const void *c, const void *w,
                           int indexed, int64_t table_row_stride, int32_t info[8]);

/* ------------------------------------------------------------------------------------------------------------- *
 * Climatologies (reference DLWP/verify.py:167-214 monthly_climo_error, :426-456 daily_climatology / daily_climo_time_series).
 * A row set: fp32 device rows of up to DLWPCS_SCORE_MAX_DIMS inner dims, every dim with its stride in ELEMENTS in the source and
 * in the output (so a channels-first array is reduced or gathered straight into a channels-last result); source row r starts at
 * r * src_row_stride, output row i at i * out_row_stride.  Lanes run along the LAST dim of the descriptor: list the dim that is
 * contiguous in the source last.  16-byte loads when that dim has source stride 1 and every extent / stride / pointer allows
 * it, else one element per lane.
 *
 * dlwpcs_group_mean: out[k] = per-element mean of the rows row_index[group_start[k] .. group_start[k + 1]) for k < n_groups,
 * NaN entries skipped per element (xarray groupby().mean(), np.nanmean): an element with no finite-or-infinite member is NaN,
 * +-inf propagate.  count (may be NULL): int32, same layout as out, the members that entered each element.
 * Sums are fp64, rounded to fp32 once.  Fixed order, whatever the grid: a group's rows are cut into slabs of
 * DLWPCS_GROUP_SLAB_ROWS rows in CSR order, a slab is summed row by row from zero, and the slab sums are added in slab order.
 * split = 0: one launch, a lane walks the slabs of its group itself.  split = 1: launch 1 gives every (group, slab) its own
 * workgroups and writes the slab sums to scratch, launch 2 adds them -- the same additions, hence the same bits; for few
 * groups over many rows (monthly, K = 1).  split < 0: chosen from the grid size.  max_group_rows >= the longest group (the
 * host built the CSR and knows it); scratch >= dlwpcs_group_mean_scratch_bytes(...) of the same arguments (0 for one launch).
 * No atomics, no host synchronisation, no allocation.  The kernel TRUSTS the CSR: group_start non-decreasing, every row_index
 * in range of the source.
 *
 * dlwpcs_rows_gather: out[i] = source row index[i] for i < n (int32 device table); a negative index writes a NaN row.
 * One launch.
 * ------------------------------------------------------------------------------------------------------------- */
#define DLWPCS_GROUP_SLAB_ROWS 512
typedef struct dlwpcs_rows_desc {
    int32_t n_inner;                                /* 0..DLWPCS_SCORE_MAX_DIMS */
    int32_t reserved;
    int64_t src_row_stride, out_row_stride;
    int64_t inner_ext[DLWPCS_SCORE_MAX_DIMS];
    int64_t src_stride[DLWPCS_SCORE_MAX_DIMS];
    int64_t out_stride[DLWPCS_SCORE_MAX_DIMS];
} dlwpcs_rows_desc;
size_t dlwpcs_group_mean_scratch_bytes(const dlwpcs_rows_desc *d, int n_groups, int64_t max_group_rows, int split);
int dlwpcs_group_mean(const dlwpcs_rows_desc *d, const float *src, const int32_t *group_start, const int32_t *row_index,
                      int n_groups, int64_t max_group_rows, int split, float *out, int32_t *count, void *scratch,
                      size_t scratch_bytes, dlwpcs_stream_t stream);
int dlwpcs_rows_gather(const dlwpcs_rows_desc *d, const float *src, const int32_t *index, int64_t n, float *out,
                       dlwpcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- *
 * Grouped quantiles along the row axis (DLWP/verify.py climatology_quantiles): the row set and the CSR of dlwpcs_group_mean
 * (strides in elements, lanes along the last inner dim, a trusted CSR; groups may be empty, a row may appear in several groups;
 * max_group_rows >= the longest group: it chooses the form, and the staged form reads no more rows of a group).  out[q] for probs[q] lies at
 * q * out_prob_stride elements; below that the layout is dlwpcs_group_mean's output layout.  count (may be NULL): int32, the
 * layout of one q slice, the members that entered each (group, element).  probs is a HOST array, read during the call.
 *
 * Definition (the tests compare bits against it).  The members of a (group, element) are the entries of the group's rows there
 * that are not NaN, n of them; +-inf are values like any other, -0 enters as +0.  n = 0: the result is the quiet NaN 0x7fc00000
 * and the count is 0.  Otherwise, with the members sorted x_(0) <= .. <= x_(n-1), in fp64 and with contraction off:
 *   h = (n - 1) * p;   j = floor(h);   g = h - j;   v = (g == 0) ? x_(j) : x_(j) + g * (x_(j+1) - x_(j))
 * and v is rounded to fp32 once: numpy's default ('linear') quantile, np.nanquantile.  A v that is NaN (inf - inf between
 * infinite neighbours) is stored as 0x7fc00000 too.  0 <= probs[q] <= 1 and 1 <= n_probs <= DLWPCS_QUANTILE_MAX_PROBS, anything
 * else is DLWPCS_E_INVALID.
 *
 * One lane owns one (group, element) column and selects by bitwise radix selection on order-preserving 32-bit keys, 32 passes
 * over the column shared by all n_probs order statistics (classes of 1, 2, 4, 8, 16 probabilities) and one more for x_(j+1):
 * no sort, exact.  Staged form: the column lies in LDS ([slot][lane]), read from memory once; classes of rows x lanes
 * 64 x 256, 128 x 128, 256 x 64 (64 KiB) and 640 x 64 (160 KiB), the smallest that holds max_group_rows.  Long form (longer
 * groups): the same passes read the rows from memory each time, 34 reads of the group.  One launch, no atomics, no allocation,
 * no host synchronisation (capturable); a zero extent launches nothing; the result does not depend on the grid.
 *
 * dlwpcs_group_quantile_plan_info (host only; src is looked at for NULL, never dereferenced): info[0] = form (0 staged, 1 long),
 * info[1] / info[2] = rows and lanes of the class (long: 0 and the threads of a workgroup), info[3] = the n_probs class,
 * info[4] / info[5] = the grid, info[6] = LDS bytes of a workgroup, info[7] = 0.
 * ------------------------------------------------------------------------------------------------------------- */
#define DLWPCS_QUANTILE_MAX_PROBS 16
int dlwpcs_group_quantile(const dlwpcs_rows_desc *d, const float *src, const int32_t *group_start, const int32_t *row_index,
                          int n_groups, int64_t max_group_rows, const double *probs /* host */, int n_probs,
                          float *out, int64_t out_prob_stride, int32_t *count /* may be NULL */, dlwpcs_stream_t stream);
int dlwpcs_group_quantile_plan_info(const dlwpcs_rows_desc *d, const void *src, int n_groups, int64_t max_group_rows,
                                    int n_probs, int32_t info[8]);   /* host only, pointers never dereferenced */

/* ------------------------------------------------------------------------------------------------------------- *
 * Filters along the row axis (DLWP/verify.py time_filter / running_mean): a finite-impulse-response filter with a decimation
 * step over the n_rows rows of a row set (dlwpcs_rows_desc: strides in elements, lanes along the last inner dim).  taps is an
 * fp32 DEVICE array of n_taps finite values, trusted.  Output row j < n_out lies at j * out_row_stride.
 *
 * Definition (the tests compare bits against it).  With T = n_rows, K = n_taps, s = step, o = origin, output row j at element e
 * is, in fp32, every operation rounded once, in this order, no contraction:
 *     acc = 0.f; w = 0.f; n = 0; bad = false
 *     for k = 0 .. K-1:                     r = j*s + k - o
 *         missing = (r < 0 || r >= T) || isnan(x[r, e])
 *         if missing: bad = true                      (nothing is added, in either mode)
 *         else:       acc = acc + h[k] * x[r, e];  w = w + h[k];  n = n + 1
 *     DLWPCS_FILTER_SUM  (0): out = (bad || isnan(acc)) ? QNAN : acc
 *     DLWPCS_FILTER_MEAN (1): q = acc / w (IEEE division);  out = (n > 0 && w >= min_weight && !isnan(q)) ? q : QNAN
 * QNAN is 0x7fc00000: every NaN that is stored has these bits.  +-inf are values like any other; 0 * inf and inf - inf end as
 * QNAN.  count (may be NULL): int32 in the output's layout, n.  1 <= K <= DLWPCS_TIME_FILTER_MAX_TAPS, s >= 1, 0 <= o < K,
 * n_rows >= 0, n_out >= 0, mode 0 / 1, form -1 / 0 / 1 and slab_rows >= 0; anything else is DLWPCS_E_INVALID.  A zero extent or
 * n_out = 0 launches nothing.  One launch, no atomics, no host synchronisation, no allocation, no scratch (capturable); the
 * result does not depend on the grid, the slab length or the form.
 *
 * The grid is column tiles of 256 chunks x time slabs of slab_rows output rows (0: the library chooses).  A chunk is four
 * elements (16-byte loads) where the layout, the pointers and the class allow it, else one.
 * form 0, streaming: a lane walks the input rows of its slab once, in order, and keeps the A = ceil(K / s) outputs a row
 * contributes to in registers, in classes of 1, 2, 4, 8, 16, 32 accumulators whose slot is a compile-time index (the row loop
 * is unrolled over one period of the class); a slab re-reads the K - s rows it shares with its predecessor.  A > 32 is refused.
 * form 1, gather: a lane computes the outputs of its slab eight at a time from one pass over the rows they read; any K and s.
 * form -1: streaming where A <= 8, else gather (measured: classes 16 and 32 are slower than the gather form).  Both forms do the
 * additions above in tap order: the same bits.
 *
 * dlwpcs_time_filter_plan_info (host only; src and out are looked at for NULL and for 16-byte alignment, never dereferenced):
 * info[0] = form, info[1] = the accumulator class (gather: 0), info[2] = 1 for 16-byte chunks, info[3] = output rows per slab,
 * info[4] / info[5] = the grid, info[6] = LDS bytes of a workgroup (0: the taps come through the scalar cache), info[7] = 0.
 * Returns what the entry point would return for the same arguments.
 * ------------------------------------------------------------------------------------------------------------- */
#define DLWPCS_TIME_FILTER_MAX_TAPS 4096
#define DLWPCS_FILTER_SUM 0
#define DLWPCS_FILTER_MEAN 1
int dlwpcs_time_filter(const dlwpcs_rows_desc *d, const float *src, int64_t n_rows, const float *taps /* device */, int n_taps,
                       int64_t step, int64_t origin, int64_t n_out, int mode, float min_weight, int form, int64_t slab_rows,
                       float *out, int32_t *count /* may be NULL */, dlwpcs_stream_t stream);
int dlwpcs_time_filter_plan_info(const dlwpcs_rows_desc *d, const void *src, const void *out, int64_t n_rows, int n_taps,
                                 int64_t step, int64_t n_out, int mode, int form, int64_t slab_rows, int32_t info[8]);

/* ------------------------------------------------------------------------------------------------------------- *
 * Spectra along the row axis (DLWP/verify.py time_spectrum, time_cross_spectrum, time_coherence, time_fourier,
 * wavenumber_frequency_spectrum): Welch's segment-averaged spectrum over the T = n_rows rows of a row set (dlwpcs_rows_desc:
 * strides in elements, lanes along the last inner dim).  Segment s holds the rows s * hop .. s * hop + M - 1, M = n_segment,
 * 2 <= M <= DLWPCS_TIME_SPECTRUM_MAX_M (more: DLWPCS_E_UNSUPPORTED), hop >= 1; there are n_seg = T >= M ? (T - M) / hop + 1 : 0
 * of them.  window: M fp32 on the DEVICE, finite, trusted; window_power = S_w = sum w_t^2 > 0, taken in fp64 from the fp32 table
 * by the caller.  twiddle: the table of dlwpcs_zonal_spectrum for L = M, {cos, -sin}(2 pi m / M), 8-byte aligned.
 *
 * Definition.  Per column and segment, in fp32, every operation rounded once, no contraction:
 *     detrend = 1:  mean = (float)(sum / (double)M), sum the fp64 sum of the segment's rows in row order;  detrend = 0: mean = 0.f
 *     y_t = w_t * (x_t - mean)
 *     Re X_f = fma chain over t = 0 .. M - 1 of y_t * cos(2 pi ft / M),  Im X_f = ... of y_t * (-sin(2 pi ft / M)), from zero, the
 *     twiddles read from the table at (f t) mod M (v_mfma_f32_32x32x2_f32)
 * for the K = n_freq frequencies f = 0 .. K - 1 (n_freq = 0: all M / 2 + 1).  P_f = c_f |X_f|^2 / (M S_w) with c_f = 1 at f = 0
 * and at f = M / 2 for even M, else 2: sum_f P_f = sum_t y_t^2 / S_w, and with a window of ones and detrend = 0 it is the
 * convention of dlwpcs_zonal_spectrum.  A segment COUNTS for a column when all its M values are finite (pair form: in both
 * operands); an infinity makes it missing.
 *
 * mode DLWPCS_SPECTRUM_POWER, b == NULL: out[f * out_row_stride + column] (the descriptor's out strides) is the mean of P_f over
 * the segments that count, NaN (0x7fc00000) where fewer than min_count >= 1 count.  b != NULL (same descriptor, own pointer), the
 * pair form: quantity q lies at q * out_outer_stride: P_aa, P_bb, the co-spectrum c_f Re(A conj B) / (M S_w) and the quadrature
 * spectrum c_f Im(A conj B) / (M S_w); quantity 0 has the bits of the single form on a.  count (may be NULL): int32 per column
 * in the layout of one frequency row, the segments that counted.
 * Summation order, whatever the plan: per (column, frequency, quantity) the fp32 products Re^2 + Im^2 (fma(Im, Im, Re * Re), and
 * likewise the other three) are widened to fp64 and added one by one in segment order from zero inside slabs of
 * DLWPCS_TIME_SPECTRUM_SLAB_SEGMENTS segments, the slab sums are added in slab order from zero, and the stored value is
 * (float)((total * (c_f / (M S_w))) / n), n the segments that counted.  split = 0: a workgroup walks the slabs of its tile.
 * split = 1: slabs get workgroups of their own and write their sums to scratch, a second launch adds them -- the same additions,
 * the same bits; for few columns under many segments.  split < 0: chosen.  scratch >= dlwpcs_time_spectrum_scratch_bytes(...) of the
 * same arguments (pair = 1 for the pair form), 8-byte aligned (0 bytes: may be NULL).
 *
 * mode DLWPCS_SPECTRUM_COEFFICIENTS (b must be NULL): no averaging; Re X_f of segment s lies at s * out_outer_stride +
 * f * out_row_stride + column, Im X_f out_part_stride further, unscaled; a segment that does not count gives NaN.  min_count,
 * split, count and scratch are not used.
 *
 * A launch of a fixed number of persistent workgroups strides over the list of tiles (32 columns x 128 frequencies x slab); which
 * workgroup computes a tile influences no bit.  No atomics, no host synchronisation, no allocation, at most two launches
 * (capturable).  n_seg = 0: the averaged forms store NaN and count 0, the coefficient form launches nothing.
 *
 * dlwpcs_time_spectrum_plan_info (host only; a and b are looked at for NULL and 16-byte alignment, never dereferenced):
 * info[0] = column tiles, info[1] = frequency tiles, info[2] = slabs, info[3] = tiles of the launch, info[4] = workgroups,
 * info[5] = split, info[6] = 1 for 16-byte loads, info[7] = LDS bytes of a workgroup.  Returns what the entry point would return
 * for the same arguments.
 * ------------------------------------------------------------------------------------------------------------- */
#define DLWPCS_TIME_SPECTRUM_MAX_M 1728
#define DLWPCS_TIME_SPECTRUM_SLAB_SEGMENTS 8
#define DLWPCS_SPECTRUM_POWER 0
#define DLWPCS_SPECTRUM_COEFFICIENTS 1
size_t dlwpcs_time_spectrum_scratch_bytes(const dlwpcs_rows_desc *d, int64_t n_rows, int n_segment, int64_t hop, int n_freq,
                                          int pair, int split);
int dlwpcs_time_spectrum(const dlwpcs_rows_desc *d, const float *a, const float *b /* NULL: single form */, int64_t n_rows,
                         int n_segment, int64_t hop, const float *window /* device */, const float *twiddle /* device */,
                         double window_power, int detrend, int n_freq, int min_count, int mode, int split,
                         int64_t out_outer_stride, int64_t out_part_stride, float *out, int32_t *count /* may be NULL */,
                         void *scratch, size_t scratch_bytes, dlwpcs_stream_t stream);
int dlwpcs_time_spectrum_plan_info(const dlwpcs_rows_desc *d, const void *a, const void *b, int64_t n_rows, int n_segment,
                                   int64_t hop, int n_freq, int mode, int split, int64_t info[8]);

/* ------------------------------------------------------------------------------------------------------------- *
 * The Gram matrix of a row set (DLWP/verify/eof.py pattern_covariance, eof_analysis, EOFAnalysis.project): the weighted,
 * centred inner products between the Ta = n_rows_a rows of a and the Tb = n_rows_b rows of b over the columns of a row set
 * (dlwpcs_rows_desc: strides in elements).  b == NULL is the symmetric form, b = a (db and n_rows_b are not looked at).
 * db has da's n_inner, inner extents and out strides, and its own source strides.  A COLUMN is one element of the inner dims;
 * columns are numbered q = 0 .. E - 1 in the row-major order of inner_ext.  The descriptor's OUT strides address what exists once
 * per column: weight_root (fp32, device, NULL = ones), the given means mean_a / mean_b and the output mean_out (may be NULL).
 *
 * Definition.  Per column, in fp32, every operation rounded once, no contraction:
 *     centring mode 0 (DLWPCS_ROW_GRAM_CENTER_NONE): mean = 0.f;  1 (_OWN): mean = (float)(sum / (double)T), sum the fp64 sum of
 *     the operand's T rows in row order (the rule of dlwpcs_time_spectrum's segment mean);  2 (_GIVEN): mean = mean_x[column]
 *     y[s] = r * (x[s] - mean),  r = weight_root[column]: the weight root goes on both operands
 * A column is EXCLUDED when any of its values in a or in b is not finite (exponent all ones), when its weight root is not
 * finite, or when a given mean is NaN; it contributes nothing.  n_valid (int64, device, may be NULL) is the number of columns
 * kept; mean_out is operand a's mean, NaN (0x7fc00000) at an excluded column.
 * Summation order, whatever the plan: the columns are cut into slabs of DLWPCS_ROW_GRAM_SLAB_COLS consecutive q; within a slab
 * the value of (s, t) is the fp32 fmaf chain from zero over the slab's columns in q order of y_a[s] * y_b[t]
 * (v_mfma_f32_32x32x2_f32), an excluded column entering as 0 * 0.  The slab sums are widened to fp64 and added in slab order from
 * zero within a group of DLWPCS_ROW_GRAM_GROUP_SLABS slabs, the group sums are added in group order from zero, and out[s * ld_out
 * + t] (double, ld_out >= Tb) is that fp64 total, not rounded again.  The symmetric form computes the tile pairs on or below the
 * diagonal and stores every element s >= t at (s, t) and at (t, s): out == out^T bit for bit, and it has the bits of the cross
 * form on (a, a).
 * split = 0: a workgroup walks all the groups of its tile pair.  split = 1: each (tile pair, group) is a tile of its own and
 * writes its fp64 group sums to scratch, a finishing launch adds them in group order -- the same additions, the same bits; for
 * few tile pairs over many columns.  split < 0: chosen.  scratch >= dlwpcs_row_gram_scratch_bytes(...) of the same arguments
 * (db == NULL for the symmetric form), 8-byte aligned; it also holds the per-column means.
 *
 * At most three launches: the column pass (one read of the data: means, exclusion, kept-column counts per workgroup), the
 * products on persistent workgroups that stride over the list of 128 x 128 tiles (which workgroup computes a tile influences no
 * bit), the finish.  No atomics, no host synchronisation, no allocation (capturable).  E = 0 stores zeros and n_valid = 0;
 * Ta = 0 or Tb = 0 is an empty output: nothing is launched and nothing stored.
 *
 * dlwpcs_row_gram_plan_info (host only; a and b are looked at for NULL and 16-byte alignment, never dereferenced):
 * info[0] = row tiles of a, info[1] = row tiles of b, info[2] = tile pairs, info[3] = slabs, info[4] = groups, info[5] = split,
 * info[6] = 1 for 16-byte loads, info[7] = workgroups of the product launch.  Returns what the entry point would return for the
 * same arguments.
 * ------------------------------------------------------------------------------------------------------------- */
#define DLWPCS_ROW_GRAM_SLAB_COLS 512
#define DLWPCS_ROW_GRAM_GROUP_SLABS 16
#define DLWPCS_ROW_GRAM_CENTER_NONE 0
#define DLWPCS_ROW_GRAM_CENTER_OWN 1
#define DLWPCS_ROW_GRAM_CENTER_GIVEN 2
size_t dlwpcs_row_gram_scratch_bytes(const dlwpcs_rows_desc *da, int64_t n_rows_a, const dlwpcs_rows_desc *db /* NULL: symmetric */,
                                     int64_t n_rows_b, int split);
int dlwpcs_row_gram(const dlwpcs_rows_desc *da, const float *a, int64_t n_rows_a, const dlwpcs_rows_desc *db,
                    const float *b /* NULL: symmetric form */, int64_t n_rows_b, const float *weight_root /* may be NULL */,
                    int center_a, const float *mean_a, int center_b, const float *mean_b, int split, double *out, int64_t ld_out,
                    float *mean_out /* may be NULL */, int64_t *n_valid /* may be NULL */, void *scratch, size_t scratch_bytes,
                    dlwpcs_stream_t stream);
int dlwpcs_row_gram_plan_info(const dlwpcs_rows_desc *da, const void *a, int64_t n_rows_a, const dlwpcs_rows_desc *db, const void *b,
                              int64_t n_rows_b, int split, int64_t info[8]);

/* ------------------------------------------------------------------------------------------------------------- *
 * Least-squares fits along the row axis (DLWP/verify.py time_regression, detrend, harmonic_climatology): per element of a row set
 * (dlwpcs_rows_desc: strides in elements, lanes along the last inner dim) the K coefficients of the basis that fit the rows
 * present best.  x: T = n_rows fp32 rows.  basis: a contiguous (T, K) fp32 DEVICE array, finite, trusted, 1 <= K <=
 * DLWPCS_REGRESSION_MAX_TERMS.  S = slab_rows > 0 (0: DLWPCS_REGRESSION_SLAB_ROWS), min_count >= K, pivot_tol a double in [0, 1)
 * (0: 2^-40), mode DLWPCS_FIT_SKIP or DLWPCS_FIT_PROPAGATE; anything else is DLWPCS_E_INVALID before any launch.
 *
 * Definition (the tests compare bits against it).  Every operation at element e is fp64, rounded once, no contraction in 4 and 5:
 *  1. row r is present when x[r, e] is not NaN; an infinity is a value.
 *  2. rows are cut into slabs of S; a slab starts from zero and takes its present rows in row order:
 *         c[k] += b[r,k] * x[r,e];   G[i][j] += b[r,i] * b[r,j] for j <= i;   n += 1
 *     (the factors are fp32, so the products are exact and a fused multiply-add has the same bits)
 *  3. the slab sums are added to totals that start from zero, in slab order.
 *  4. L D L^T without a square root.  For j = 0 .. K-1:
 *         s = 0; for p < j in order: s = s + (L[j][p] * L[j][p]) * d[p];        d[j] = G[j][j] - s
 *         the column is SINGULAR unless d[j] > pivot_tol * G[j][j]   (nothing after it is computed)
 *         for i > j:  s = 0; for p < j in order: s = s + (L[i][p] * L[j][p]) * d[p];   L[i][j] = (G[i][j] - s) / d[j]
 *  5. for i ascending:  s = 0; for p < i in order: s = s + L[i][p] * z[p];   z[i] = c[i] - s
 *     w[i] = z[i] / d[i]
 *     for i descending: s = 0; for p = i+1 .. K-1 in order: s = s + L[p][i] * a[p];   a[i] = w[i] - s
 *  6. coef[k, e] = (float)a[k].  All K coefficients of the element are QNAN (0x7fc00000) when n < min_count, the column is
 *     singular, any (float)a[k] is not finite, or mode is PROPAGATE and n < T.
 *  7. count (may be NULL): int32, n.
 * coef[k] lies at k * coef_term_stride elements; below that the layout is dlwpcs_group_mean's output layout (out_stride[] of the
 * descriptor; out_row_stride is not used), and count has the layout of one term.
 *
 * split follows dlwpcs_group_mean.  0: a lane walks its slabs and adds their sums.  1: every (column tile, slab) has its own
 * workgroups and the slab sums of c and n go to scratch.  < 0: split when there are fewer than 512 column tiles and more than one
 * slab.  Either way a finishing launch, one element per lane, adds what the first stored in slab order and solves.  gram = 0: a
 * column with no missing row has the G of every other such column, so that G, its L and d are computed once per call into scratch
 * (two small launches) and the column only does the two solves; a column with gaps re-reads its rows in the finishing launch for
 * a G of its own (not in PROPAGATE mode, which answers QNAN).  gram = 1: every column its own G.  gram < 0: the library's choice
 * (0).  Every combination gives the same bits.  K is served in classes of 1, 2, 4, 8, 16 terms; a chunk of the first launch is
 * four elements (16-byte loads) up to class 8 where the layout and the pointers allow it, else one.  scratch >=
 * dlwpcs_time_regression_scratch_bytes(...) of the same arguments, 8-byte aligned: the shared factor, the slab sums of its G
 * (136 doubles a slab) and the sums of c and n (K doubles and an int32 per element, times the slabs when split).  No atomics, no
 * allocation, no host synchronisation (capturable); a zero extent launches nothing; n_rows = 0 (src and basis may then be NULL)
 * answers QNAN and a count of 0.
 *
 * dlwpcs_time_regression_plan_info (host only; src and coef are looked at for NULL and for 16-byte alignment, never dereferenced):
 * info[0] = split, info[1] = gram, info[2] = the term class, info[3] = elements per chunk, info[4] / info[5] = the grid of the
 * first launch over the rows, info[6] = LDS bytes of a workgroup of it (0), info[7] = rows per slab.
 *
 * dlwpcs_time_regression_apply: out[r, e] for r < n_rows from the coefficients and a basis of n_rows rows (which need not be the
 * rows of the fit: a climatology is evaluated at forecast valid times this way).  f = 0; for k in order: f = f + b[r,k] *
 * coef[k,e] in fp64 (exact products, fma allowed).  DLWPCS_FIT_FITTED: out = (float)f, src may be NULL.  DLWPCS_FIT_RESIDUAL:
 * out = (float)((double)x[r,e] - f).  The output is QNAN where a coefficient of the element is NaN or the value is NaN (a NaN x
 * among them).  src and out are addressed through d; coef[k] of an element lies at k * coef_term_stride + sum of coordinate *
 * coef_stride[i] (a HOST array of n_inner strides, read during the call; NULL: out_stride[]).  One launch over column tiles x
 * row slabs: every row is read once, the coefficients of a lane stay in registers.
 * ------------------------------------------------------------------------------------------------------------- */
#define DLWPCS_REGRESSION_MAX_TERMS 16
#define DLWPCS_REGRESSION_SLAB_ROWS 512
#define DLWPCS_FIT_SKIP 0
#define DLWPCS_FIT_PROPAGATE 1
#define DLWPCS_FIT_FITTED 0
#define DLWPCS_FIT_RESIDUAL 1
size_t dlwpcs_time_regression_scratch_bytes(const dlwpcs_rows_desc *d, int64_t n_rows, int n_terms, int64_t slab_rows, int split);
int dlwpcs_time_regression(const dlwpcs_rows_desc *d, const float *src, int64_t n_rows, const float *basis /* device */, int n_terms,
                           int mode, int64_t min_count, double pivot_tol, int64_t slab_rows, int split, int gram, float *coef,
                           int64_t coef_term_stride, int32_t *count /* may be NULL */, void *scratch, size_t scratch_bytes,
                           dlwpcs_stream_t stream);
int dlwpcs_time_regression_plan_info(const dlwpcs_rows_desc *d, const void *src, const void *coef, int64_t n_rows, int n_terms,
                                     int mode, int64_t min_count, int64_t slab_rows, int split, int gram, int64_t coef_term_stride,
                                     int32_t info[8]);
int dlwpcs_time_regression_apply(const dlwpcs_rows_desc *d, const float *src /* may be NULL */, int64_t n_rows,
                                 const float *basis /* device */, int n_terms, const float *coef, int64_t coef_term_stride,
                                 const int64_t *coef_stride /* host, may be NULL */, int mode, float *out, dlwpcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- *
 * Lagged covariances along the row axis (DLWP/verify/timeseries.py lag_covariance, lag_correlation, autocorrelation,
 * lag_regression, decorrelation_time, effective_sample_size): over the T = n_rows rows of a row set (dlwpcs_rows_desc: strides in
 * elements, lanes along the last inner dim; every other dim is "columns").  a is fp32.  b takes one of three forms:
 *     DLWPCS_LAG_AUTO  (0): b == NULL and b = a (and center_b == NULL means center_a);
 *     DLWPCS_LAG_PAIR  (1): b has a's shape and a's strides (the same descriptor, its own pointer);
 *     DLWPCS_LAG_INDEX (2): b is a contiguous fp32 DEVICE vector of T values shared by every column.
 * The lags are l_i = lag0 + i * lag_step for i < n_lags, lag_step >= 1, 1 <= n_lags <= DLWPCS_TIME_LAG_MAX_LAGS; they may be
 * negative, and a lag with |l| >= T simply has no pairs.  Lag l pairs a[t] with b[t + l]: a positive lag means a leads.
 *
 * Definition (the tests compare bits against it).  Per column and lag:
 *     da[t] = a[t] - ca and db[t] = b[t] - cb, ONE fp32 subtraction each.  center_a / center_b (may be NULL: subtract nothing)
 *     hold one fp32 value per column at sum of coordinate * center_stride[i] (a HOST array of n_inner strides, read during the
 *     call; NULL: out_stride[] of the descriptor): the layout of a one-row result, which is what dlwpcs_group_mean with one group
 *     writes.  In the index form center_b is one scalar.  An entry is PRESENT when it is not NaN; a missing entry has da = +0.
 *     S_l = the sum over slabs, ascending, of (the sum over the rows t of the slab, ascending, with 0 <= t + l < T, of
 *     (double)da[t] * (double)db[t + l]); the slab of a pair is the slab of its a row t, slabs are DLWPCS_TIME_LAG_SLAB_ROWS rows,
 *     fixed, and every slab sum and the total start at +0.  The factors are fp32, so each product is exact in fp64 and a fused
 *     multiply-add has the bits of a multiply and an add; adding the +-0 of a missing pair changes nothing.
 *     n_l = the number of pairs with both entries present (int32).
 *     out = (float)(S_l / (double)n_l): one fp64 division, rounded to fp32 once; QNAN where n_l < need_l, with need_l =
 *     max(min_count, 1) in mode DLWPCS_LAG_SKIP and need_l = max(T - |l|, 1) in mode DLWPCS_LAG_PROPAGATE (any missing entry in
 *     range spoils the lag).  An infinite entry is a value: IEEE decides (inf * 0 of a missing partner is NaN); every NaN that is
 *     stored is QNAN = 0x7fc00000.
 * out[i] for lag i lies at i * out_row_stride + the column's out offset: a's dims in the order the caller chose, the lags where
 * the row axis stood.  count (may be NULL): int32, the same layout, n_l.
 *
 * The bits do not depend on the plan.  A pass serves a block of lag_block consecutive lags (0: chosen; at most 16) in classes of
 * 1, 4, 8 and 16 accumulators per element; a chunk is four elements (16-byte loads) where the layout and the pointers allow it,
 * else one.  split = 0: a lane walks the slabs of its chunk and stores the result.  split = 1: every (column tile, slab, lag
 * block) is a tile of its own and writes fp64 slab sums and int32 counts to scratch, a finishing launch adds them in slab order
 * and divides -- the same additions, the same bits; for few columns under many rows.  split < 0: chosen.  scratch >=
 * dlwpcs_time_lag_scratch_bytes(...) of the same arguments, 8-byte aligned (0 bytes: may be NULL).  A launch of a fixed number of
 * persistent workgroups strides over the list of tiles; which workgroup computes a tile influences no bit.  No atomics, no host
 * synchronisation, no allocation, at most two launches (capturable).  No columns: nothing is launched.  n_rows = 0 (a and b may
 * then be NULL): every lag is QNAN with a count of 0.
 *
 * dlwpcs_time_lag_plan_info (host only; a and b are looked at for NULL and 16-byte alignment, never dereferenced): info[0] =
 * lags per pass, info[1] = passes, info[2] = elements per chunk, info[3] = slabs, info[4] = split, info[5] = tiles of the launch,
 * info[6] = workgroups, info[7] = scratch bytes.  Returns what the entry point would return for the same arguments.
 * ------------------------------------------------------------------------------------------------------------- */
#define DLWPCS_TIME_LAG_MAX_LAGS 1024
#define DLWPCS_TIME_LAG_SLAB_ROWS 512
#define DLWPCS_LAG_AUTO 0
#define DLWPCS_LAG_PAIR 1
#define DLWPCS_LAG_INDEX 2
#define DLWPCS_LAG_SKIP 0
#define DLWPCS_LAG_PROPAGATE 1
size_t dlwpcs_time_lag_scratch_bytes(const dlwpcs_rows_desc *d, int form, int64_t n_rows, int64_t lag_step, int n_lags, int split,
                                     int lag_block);
int dlwpcs_time_lag(const dlwpcs_rows_desc *d, const float *a, const float *b /* NULL: auto form */, int form, int64_t n_rows,
                    int64_t lag0, int64_t lag_step, int n_lags, const float *center_a /* may be NULL */,
                    const float *center_b /* may be NULL */, const int64_t *center_stride /* host, may be NULL */, int mode,
                    int min_count, int split, int lag_block, float *out, int32_t *count /* may be NULL */, void *scratch,
                    size_t scratch_bytes, dlwpcs_stream_t stream);
int dlwpcs_time_lag_plan_info(const dlwpcs_rows_desc *d, const void *a, const void *b, int form, int64_t n_rows, int64_t lag_step,
                              int n_lags, int split, int lag_block, int64_t info[8]);

/* ------------------------------------------------------------------------------------------------------------- *
 * Block-bootstrap means along the row axis (DLWP/verify/resample.py bootstrap_mean, bootstrap_interval, bootstrap_difference):
 * B = n_resamples means over rows drawn with replacement, in blocks, from the T = n_rows rows of a row set (dlwpcs_rows_desc:
 * strides in elements, lanes along the last inner dim; every other dim is "columns").  src is fp32.
 *
 * Draw table: starts, int32 on the DEVICE, contiguous (B, nb), values in 0 .. T-1 (a value outside is clamped into that range: no
 * row outside the series is ever read).  Block length L = block_length, 1 <= L <= T; n_draw >= 1 rows are drawn per resample;
 * nb = n_blocks = ceil(n_draw / L), anything else is DLWPCS_E_INVALID.  Resample b draws, in this order, for block j = 0 .. nb-1
 * the rows (starts[b, j] + i) mod T, i = 0 .. L-1; the last block is cut after n_draw - (nb - 1) L rows.  The kernel always wraps:
 * whether a start may lie where its block wraps (circular) or not (moving blocks) is the caller's choice when it draws.
 *
 * Definition (the tests compare bits against it).  Per element and resample:
 *     a block's entries are added in row order into an fp64 sum from +0, fp32 widened to fp64; the block sums are added in draw
 *     order into the resample's fp64 total from +0.  The counts (int32) are added the same way.  A NaN entry is missing: skipped
 *     and not counted.  +-inf are values and propagate (inf - inf is NaN).
 *     out = (float)(total / (double)count): one fp64 division, rounded to fp32 once.  Mode DLWPCS_RESAMPLE_SKIP: QNAN where
 *     count < max(min_count, 1); DLWPCS_RESAMPLE_PROPAGATE: QNAN where count < n_draw.  Every NaN stored is QNAN = 0x7fc00000.
 * out[b] lies at b * out_row_stride + the column's out offset: src's dims in the order the caller chose with the row axis B long,
 * exactly like dlwpcs_group_mean.  count (may be NULL): int32, the same layout.
 *
 * "Block first, then blocks" makes two implementations legal with the same bits: a nested loop over the drawn rows (what is built)
 * and a table of block sums per start added nb times per resample (not built: info[5] = 0).
 *
 * Forms, form = DLWPCS_RESAMPLE_CHOOSE (-1), _STAGED (0), _DIRECT (1).  Staged: a workgroup copies a tile of 64 columns x up to
 * 640 rows, or 32 columns x up to DLWPCS_RESAMPLE_STAGED_ROWS = 1280 rows, into LDS once and serves its resamples from there;
 * T beyond that is DLWPCS_E_UNSUPPORTED when staged is forced and runs direct when chosen.  Direct: the same loops read the rows
 * from memory, any T.  splits = the number of resample ranges a column tile's resamples are cut into, each a work item of its own
 * (0: chosen -- more than one only with fewer column tiles than workgroups; it is capped at B).  A fixed number of persistent
 * workgroups strides over the (column tile, range) items.  One lane computes all of a (resample, element), so the bits depend on
 * neither the form, the chunk width (16-byte loads where layout and pointer allow), the split nor the grid.  Limits: T, n_draw
 * and B at most DLWPCS_RESAMPLE_MAX_ROWS = 2^31 - 1 (DLWPCS_E_UNSUPPORTED beyond); element offsets are 64-bit.  No atomics, no
 * scratch, no host synchronisation, no allocation, one launch on the given stream (capturable).  B = 0 or no columns: nothing is
 * launched (and nothing else is checked).
 *
 * dlwpcs_row_resample_plan_info (host only; src is looked at for NULL and 16-byte alignment, never dereferenced): info[0] = form,
 * info[1] = tile columns, info[2] = staged row cap, info[3] = workgroups, info[4] = LDS bytes of a workgroup, info[5] = block-sum
 * table used (always 0), info[6] = elements per staging chunk (4 or 1; direct: 1), info[7] = resample ranges.  Returns what the
 * entry point would return for the same arguments.
 * ------------------------------------------------------------------------------------------------------------- */
#define DLWPCS_RESAMPLE_STAGED_ROWS 1280
#define DLWPCS_RESAMPLE_MAX_ROWS 2147483647
#define DLWPCS_RESAMPLE_CHOOSE (-1)
#define DLWPCS_RESAMPLE_STAGED 0
#define DLWPCS_RESAMPLE_DIRECT 1
#define DLWPCS_RESAMPLE_SKIP 0
#define DLWPCS_RESAMPLE_PROPAGATE 1
int dlwpcs_row_resample(const dlwpcs_rows_desc *d, const float *src, const int32_t *starts /* device */, int64_t n_rows,
                        int64_t n_resamples, int64_t n_blocks, int64_t block_length, int64_t n_draw, int mode, int min_count,
                        int form, int64_t splits, float *out, int32_t *count /* may be NULL */, dlwpcs_stream_t stream);
int dlwpcs_row_resample_plan_info(const dlwpcs_rows_desc *d, const void *src, int64_t n_rows, int64_t n_resamples, int64_t n_blocks,
                                  int64_t block_length, int64_t n_draw, int form, int64_t splits, int64_t info[8]);

/* ------------------------------------------------------------------------------------------------------------- *
 * Spells along the row axis (DLWP/verify/spells.py spell_statistics, spell_length, spell_position, spell_mask): the maximal runs
 * of rows on which a condition holds, per column, over the T = n_rows rows of a row set (dlwpcs_rows_desc: strides in elements,
 * lanes along the last inner dim; every other dim is "columns").  src is fp32.
 *
 * Threshold: a table thr of K >= 1 fp32 rows on the device, addressed in elements by thr_row_stride and one stride per inner dim,
 * thr_stride[] (a HOST array of n_inner strides, read during the call; NULL: all 0).  A stride of 0 broadcasts: a scalar threshold
 * is one element with every stride 0, a per-variable threshold has stride 0 on the spatial dims.  Row t compares against table
 * row thr_index[t] (int32 on the DEVICE, trusted to lie in [0, K)); thr_index == NULL: every row compares against table row 0.
 *
 * Definition (the tests compare against it; every result is an integer, so equality holds everywhere).  With x[t, e] the entry
 * and h[t, e] its threshold:
 *     c[t, e] = x cmp h, the IEEE comparison, cmp = DLWPCS_SPELL_GT (0), _GE (1), _LT (2), _LE (3): false whenever either side is
 *     NaN; +-inf are values like any other.  m[t, e] = isnan(x) || isnan(h) marks a missing entry.
 *     A spell of a column is a maximal interval [s, e] of rows with c true, of length n = e - s + 1; the first and the last row of
 *     the series close a spell like a false row does.  A spell QUALIFIES when n >= min_length (min_length >= 1; it may exceed T).
 *     pos[t, e] (int32, may be NULL): the 1-based place of t inside its qualifying spell, 0 outside one.
 *     len[t, e] (int32, may be NULL): the length n of the qualifying spell that holds t, 0 outside one.
 *     Both have T rows in the output layout of the descriptor (row t at t * out_row_stride + the column's out offset).
 *     stats (int32, may be NULL): statistic k at k * stat_stride + the column's out offset (the layout of one output row):
 *         0 n_valid        rows with m false
 *         1 n_true         rows with c true, whatever min_length
 *         2 n_spells       qualifying spells
 *         3 spell_rows     the sum of their lengths
 *         4 longest        the largest qualifying length, 0 if none
 *         5 longest_start  s of the first qualifying spell of that length, -1 if none
 *     missing = DLWPCS_SPELL_BREAK (0): a missing row is simply a false row.  DLWPCS_SPELL_PROPAGATE (1): in a column with any
 *     missing row, pos, len and the statistics 1 to 5 are all -1; n_valid stays exact.
 *
 * The slab combine rule (why the rows may be cut anywhere).  A run of consecutive rows has the partial (rows n, head, tail,
 * n_valid, n_true, cnt, spell_rows, longest, start): head counts its leading trues and tail its trailing trues; the run is all-true
 * if and only if head == n (then tail == n and the closed fields are empty); cnt, spell_rows, longest and start describe only the
 * qualifying spells that have a false row on both sides inside the run, start being an absolute row.  Joining A before B: n_valid
 * and n_true add.  Both all-true: the result is all-true.  Only A all-true: head = A.n + B.head, tail = B.tail.  Only B all-true:
 * head = A.head, tail = A.tail + B.n.  Otherwise head = A.head, tail = B.tail, and the joined run of A.tail + B.head rows, if that
 * is > 0, closes at start B.first_row - A.tail and is counted if it is >= min_length.  A's closed fields are taken first, then
 * the joined run, then B's; a longer spell replaces longest and start, an equally long one only if it starts earlier.  At the
 * ends of the series: for an all-true series the one run of n rows closes at start 0; otherwise head closes at start 0 and tail
 * at n - tail, where they are > 0.
 *
 * Forms.  A lane owns one chunk of columns (four with 16-byte loads where the layout and src allow it, else one); work items are
 * (column tile of 64 chunks, time slab) and a fixed number of persistent workgroups strides over them.  Statistics only (pos and
 * len NULL): a lane walks its slab once carrying the partial; one slab is one launch at any T, several slabs (chosen with few
 * column tiles) store one partial of eight int32 per (slab, column) and a second launch joins them in slab order.  Per-row
 * outputs: a lane packs the condition of its slab into W words of 32 rows in registers, W = 1, 2, 4, 8, 16 or 32 (the four-column
 * chunk: at most 8; a larger slab takes the one-column chunk), and writes pos and len row by row; one slab (T <= 32 W) is one
 * launch that also stores the statistics, several slabs take three: the partials, one lane per column scanning them forward and
 * backward into every slab's carries, the column's propagate flag and the statistics, and the rows, for which the series is read
 * a second time.  slab_rows = 0: the library chooses; per-row outputs accept 32, 64, 128, 256, 512 and 1024, statistics only any
 * positive multiple of 32 (anything else: DLWPCS_E_INVALID).  The result is independent of form, class, slab length, chunk
 * width and grid.  scratch >= dlwpcs_time_spell_scratch_bytes(d, src, n_rows, slab_rows, per_row = pos or len given), 16-byte
 * aligned (0 bytes: may be NULL).  Limits: T at most DLWPCS_SPELL_MAX_ROWS = 2^31 - 1 (DLWPCS_E_UNSUPPORTED beyond); element
 * offsets are 64-bit.  Bad enums, min_length < 1 and negative extents are DLWPCS_E_INVALID.  No atomics, no allocation, no host
 * synchronisation, at most three launches on the given stream (capturable).  T = 0 or no columns: nothing is launched and
 * nothing is written.
 *
 * dlwpcs_time_spell_plan_info (host only; src is looked at for NULL and 16-byte alignment, never dereferenced): info[0] = form
 * (0 statistics, 1 statistics in slabs, 2 rows, 3 rows in slabs), info[1] = slab rows, info[2] = slabs, info[3] = register class
 * W (statistics only: 0), info[4] = elements per chunk (4 or 1), info[5] = workgroups, info[6] = launches, info[7] = scratch
 * bytes.  Returns what the entry point would return for the same arguments.
 * ------------------------------------------------------------------------------------------------------------- */
#define DLWPCS_SPELL_MAX_ROWS 2147483647
#define DLWPCS_SPELL_GT 0
#define DLWPCS_SPELL_GE 1
#define DLWPCS_SPELL_LT 2
#define DLWPCS_SPELL_LE 3
#define DLWPCS_SPELL_BREAK 0
#define DLWPCS_SPELL_PROPAGATE 1
#define DLWPCS_SPELL_STATS 6
size_t dlwpcs_time_spell_scratch_bytes(const dlwpcs_rows_desc *d, const void *src, int64_t n_rows, int64_t slab_rows, int per_row);
int dlwpcs_time_spell(const dlwpcs_rows_desc *d, const float *src, int64_t n_rows, const float *thr /* device */,
                      int64_t thr_row_stride, const int64_t *thr_stride /* host, may be NULL */,
                      const int32_t *thr_index /* device, may be NULL */, int cmp, int64_t min_length, int missing, int64_t slab_rows,
                      int32_t *pos /* may be NULL */, int32_t *len /* may be NULL */, int32_t *stats /* may be NULL */,
                      int64_t stat_stride, void *scratch, size_t scratch_bytes, dlwpcs_stream_t stream);
int dlwpcs_time_spell_plan_info(const dlwpcs_rows_desc *d, const void *src, int64_t n_rows, int64_t slab_rows, int per_row,
                                int64_t info[8]);

/* ------------------------------------------------------------------------------------------------------------- *
 * Rank statistics along the row axis (DLWP/verify/ranks.py time_ranks, kendall_tau, mann_kendall, spearman_correlation): counts
 * over the pairs of rows of a column, over the T = n_rows rows of a row set (dlwpcs_rows_desc: strides in elements, lanes along
 * the last inner dim; every other dim is "columns").  a is fp32.
 *
 * Rank forms.  DLWPCS_RANK_TREND (0): b == NULL, the partner of row t is t itself.  DLWPCS_RANK_PAIR (1): b has a's shape and
 * strides.  DLWPCS_RANK_INDEX (2): b is a contiguous device vector of T values shared by every column.
 *
 * Definition (the tests compare integers against it).  Per column:
 *     Row t is PRESENT when a[t] is not NaN and, in the pair and index forms, b[t] is not NaN either; P is the set of present
 *     rows.  Comparisons are IEEE: -0 == +0, and +-inf are values like any other.
 *     lt_a[t] = #{s in P : a[s] < a[t]},  eq_a[t] = #{s in P : a[s] == a[t]} (t included);  lt_b, eq_b: the same counts for b.
 *     rank_a[t] (fp32, may be NULL; T rows in the output layout of the descriptor, row t at t * out_row_stride + the column's
 *     out offset) = (float)lt_a[t] + 0.5f * (float)(eq_a[t] + 1): the mid-rank, 1-based, exact in fp32 under the row cap below;
 *     QNAN = 0x7fc00000 on a row not in P.  rank_b likewise; asking for it in the trend form is DLWPCS_E_INVALID.
 *     stats (int64, may be NULL): statistic k at k * stat_stride + the column's out offset (the layout of one output row).  Pairs
 *     are i < j, both in P:
 *         0 n_valid     |P|
 *         1 concordant  sgn(a_j - a_i) * sgn(b_j - b_i) > 0   (the signs from comparisons: inf against inf is a tie)
 *         2 discordant  the same product < 0
 *         3 tie_a       a_i == a_j and b_i != b_j
 *         4 tie_b       b_i == b_j and a_i != a_j
 *         5 tie_both    both equal
 *         6 tie3_a      the sum over the tie groups of a, of size g, of g(g-1)(2g+5); equal to the sum over t in P of
 *                       (eq_a[t]-1)(2 eq_a[t]+5)
 *         7 tie3_b      the same for b
 *     In the trend form the statistics 4, 5 and 7 are 0.  The statistics 1 to 5 add up to n_valid (n_valid - 1) / 2.
 *     missing = DLWPCS_RANK_SKIP (0): deletion to P, as above.  DLWPCS_RANK_PROPAGATE (1): a column with any row outside P has the
 *     statistics 1 to 7 = -1 and every rank QNAN; n_valid stays exact.
 *
 * Plans.  A workgroup of eight waves owns a tile of columns.  Staged (form 1): the tile, and b's in the pair form, is copied into
 * LDS once with the missing rows masked, and every pair is served from there; the tiles are 64 columns x up to
 * DLWPCS_RANK_STAGE_ROWS_SMALL = 160 rows (40 KB, four workgroups a compute unit), 64 x DLWPCS_RANK_STAGE_ROWS_64 = 640,
 * 32 x DLWPCS_RANK_STAGE_ROWS_32 = 1280 and 16 x DLWPCS_RANK_STAGE_ROWS_16 = 2560 (160 KB); the pair form holds two tiles, so
 * each cap is halved.  The smallest tile that holds T rows is taken.  Direct (form 2): the same loops on memory, 64 columns a
 * workgroup, at any T.  form 0: staged where T fits, else direct; form 1 with more rows than the last cap is
 * DLWPCS_E_UNSUPPORTED.  A lane holds 8 rows i of its column in registers and the rows are dealt round robin in super-blocks over
 * the waves of the `splits` workgroups that share a tile (splits 0: chosen; at most 4096).  The ranks (rank_a or rank_b given)
 * take one launch in which every row meets every row; a split needs no partial.  The statistics take a launch of their own that
 * visits every pair i < j once; tie3 comes from the equal rows BEHIND each row (a tie group of g rows has g-1, g-2, .. 0 of them and
 * g(g-1)(2g+5) = sum over k < g of 6k(k+2)), so no second pass counts eq.  With splits > 1 every workgroup leaves eight int64 per
 * column in scratch and a finishing launch adds them: integer addition has no order, so a split never changes a result.  Chunks:
 * 16-byte staging loads (4 elements) where the layout and the pointers allow it, else 1; the direct form: 1.  The result is
 * independent of form, tile, chunk width, splits and grid.  scratch >= dlwpcs_time_rank_scratch_bytes(.., per_row = 0, ..) where
 * stats is given, 16-byte aligned (0 bytes: may be NULL).  Limits: T at most DLWPCS_RANK_MAX_ROWS = 65536, so that every pair
 * count is below 2^31 and every mid-rank exact in fp32, and column tiles x splits at most 2^22, the workgroups of one grid
 * dimension (DLWPCS_E_UNSUPPORTED beyond either); element offsets are 64-bit.  Bad enums and
 * negative extents are DLWPCS_E_INVALID.  No atomics, no allocation, no host synchronisation, at most three launches on the given
 * stream (capturable).  T = 0 or no columns: nothing is launched and nothing is written.
 *
 * dlwpcs_time_rank_plan_info (host only; a and b are looked at for NULL and alignment, never dereferenced) describes the launch
 * of the ranks (per_row = 1) or of the statistics (per_row = 0): info[0] = form (1 staged, 2 direct), info[1] = tile columns,
 * info[2] = tile rows (direct: 0), info[3] = elements per chunk (4 or 1), info[4] = splits, info[5] = workgroups of the main
 * launch, info[6] = launches, info[7] = scratch bytes.  Returns what the entry point would return for the same arguments.
 * ------------------------------------------------------------------------------------------------------------- */
#define DLWPCS_RANK_MAX_ROWS 65536
#define DLWPCS_RANK_STAGE_ROWS_SMALL 160
#define DLWPCS_RANK_STAGE_ROWS_64 640
#define DLWPCS_RANK_STAGE_ROWS_32 1280
#define DLWPCS_RANK_STAGE_ROWS_16 2560
#define DLWPCS_RANK_TREND 0
#define DLWPCS_RANK_PAIR 1
#define DLWPCS_RANK_INDEX 2
#define DLWPCS_RANK_SKIP 0
#define DLWPCS_RANK_PROPAGATE 1
#define DLWPCS_RANK_STATS 8
size_t dlwpcs_time_rank_scratch_bytes(const dlwpcs_rows_desc *d, const void *a, const void *b, int rank_form, int64_t n_rows,
                                      int per_row, int form, int64_t splits);
int dlwpcs_time_rank(const dlwpcs_rows_desc *d, const float *a, const float *b /* device, NULL in the trend form */, int rank_form,
                     int64_t n_rows, int missing, int form, int64_t splits, float *rank_a /* may be NULL */,
                     float *rank_b /* may be NULL */, int64_t *stats /* may be NULL */, int64_t stat_stride, void *scratch,
                     size_t scratch_bytes, dlwpcs_stream_t stream);
int dlwpcs_time_rank_plan_info(const dlwpcs_rows_desc *d, const void *a, const void *b, int rank_form, int64_t n_rows, int per_row,
                               int form, int64_t splits, int64_t info[8]);

/* ------------------------------------------------------------------------------------------------------------- *
 * Offline-map remapping (cubed sphere <-> lat-lon, DLWP/remap): one sparse matrix in CSR form applied to a stack of fields,
 *   y[o, r, k] = sum_{j in [row_ptr[r], row_ptr[r+1])} val[j] * x[o, col[j], k]      for r < n_b,
 * the terms of each output added in CSR order with fp32 fma (no atomics, no split rows: bitwise repeatable, and eager and
 * graph replay give the same bits).  o runs over up to three outer dims, k over at most one inner dim; every dim has its own
 * stride in ELEMENTS for x and for y, so permuted views need no copy.  Offsets are 64-bit.  x is fp32 or bf16 (x_dtype =
 * DLWPCS_F32 / DLWPCS_BF16), y and val are fp32.  row_ptr has n_b + 1 entries, col holds 0-based source cells.
 * The kernel TRUSTS the CSR: row_ptr non-decreasing from 0 to nnz, every col in [0, n_a).  The host validates a map when it
 * loads it (DLWP.remap.OfflineMap); nothing here re-checks it.
 * One launch, no host synchronisation, no allocation (capturable).  A zero extent returns DLWPCS_OK without a launch.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct dlwpcs_sparse_map_desc {
    int64_t n_a, n_b, nnz;              /* source cells, destination rows, CSR entries (nnz < 2^31, n_b * inner_ext < 2^31) */
    int32_t x_dtype;                    /* DLWPCS_F32 or DLWPCS_BF16 */
    int32_t n_outer;                    /* 0..3 outer dims */
    int64_t outer_ext[3];
    int64_t x_outer_stride[3], y_outer_stride[3];
    int64_t x_space_stride, y_space_stride;
    int64_t inner_ext;                  /* 1 when there is no inner dim */
    int64_t x_inner_stride, y_inner_stride;
} dlwpcs_sparse_map_desc;
int dlwpcs_sparse_map_apply(const dlwpcs_sparse_map_desc *d, const int32_t *row_ptr, const int32_t *col, const float *val,
                            const void *x, float *y, dlwpcs_stream_t stream);

/* The same map over data with holes: a NaN in x is a MISSING value (+-inf is data), and an entry with val[j] == 0 is not there at
 * all (the bilinear maps' triangle rows repeat a cell with weight exactly 0: neither present nor missing).  For destination row r
 * and one (outer, inner) position, over the row's non-zero entries in CSR order:
 *   acc   the fp32 fma chain of val[j] * x[col[j]] over the entries whose x is not NaN (grouped as dlwpcs_sparse_map_apply's)
 *   wval  the fp32 sum of val[j] over those entries;   wall  the fp32 sum of val[j] over all of them
 *   nmiss the number of entries whose x is NaN
 * y is MISSING (a quiet NaN) iff nmiss > 0 and (wval < min_valid * wall [one fp32 multiply], or every entry is missing, or
 * min_valid >= 1); otherwise y = acc * (wall / wval) with DLWPCS_MAP_RENORMALIZE, y = acc without.  Where nothing is missing
 * wval == wall bitwise and y has the bits of dlwpcs_sparse_map_apply.  frac (NULL, or fp32 with y's shape and strides) receives
 * wval / wall: exactly 1 where nothing is missing, 0 for a row without non-zero entries (whose y is 0).
 * The decision is fp32 additions in a fixed order, one multiply and one compare: DLWP.remap.OfflineMap.apply_host takes the
 * same one bit for bit.  min_valid must lie in [0, 1]; the weights are expected to be >= 0 (the host refuses others).
 * One launch, no LDS, no atomics, no host synchronisation, no allocation (capturable); bitwise repeatable. */
#define DLWPCS_MAP_RENORMALIZE 1
int dlwpcs_sparse_map_apply_masked(const dlwpcs_sparse_map_desc *d, const int32_t *row_ptr, const int32_t *col,
                                   const float *val, const void *x, float *y, float *frac, float min_valid, int flags,
                                   dlwpcs_stream_t stream);

/* Missing values per plane of a contiguous (n_planes, plane) array: count[p] = the number of NaN elements (dtype DLWPCS_F32: any
 * payload, either sign; +-inf is not counted) or of -32768 codes (dtype DLWPCS_I16, the packed series' missing code) of plane p.
 * x needs the alignment of its element only, plane may be any size < 2^31.  One streaming pass; every count is written by exactly
 * one workgroup (no atomics: count need not be zeroed).  One launch, no host synchronisation, no allocation. */
#define DLWPCS_I16 2                  /* dlwpcs_missing_count only: int16 codes */
int dlwpcs_missing_count(const void *x, int dtype, int64_t n_planes, int64_t plane, int32_t *count, dlwpcs_stream_t stream);
/* Fill the missing values of x in place (dtype DLWPCS_F32 or DLWPCS_BF16, n < 2^32 elements): x[e] = fill[(e / fill_div) %
 * fill_period] where x[e] is NaN (any payload, either sign); every other element, -0.0 and +-inf included, keeps its bits.  fill:
 * fp32 device table of fill_period values; a bf16 element receives the value rounded to nearest even.  x needs the alignment of
 * its element only.  One streaming launch, no host synchronisation, no allocation. */
int dlwpcs_fill_missing(void *x, int dtype, size_t n, const float *fill, int fill_div, int fill_period,
                        dlwpcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- *
 * Zonal power spectra and cross-spectra (DLWP/verify.py zonal_spectrum, zonal_cross_spectrum, zonal_coherence): a score that
 * depends on scale.  For a real row x[0..L-1] along longitude (unit stride),
 *   X_k = sum_j x_j exp(-2 pi i jk / L),  P_k = c_k |X_k|^2 / L^2,  c_k = 1 for k = 0 and for k = L/2 when L is even, else 2,
 * for k < K = n_wave (0: all L/2 + 1, where sum_k P_k = mean_j x_j^2).  The leading axes arrive as n_dims merged dims with an
 * extent, an element stride per operand (0: a, 1: b, 2: w; 0 = broadcast) and a flag: kept dims index the GROUPS (row-major
 * in the order given), the others the rows of a group, over which the result is the weighted mean
 *   sum w P_k / sum w   over the rows that COUNT: rows whose L values are all finite (pair form: in a and in b).
 * Unlike dlwpcs_missing_count an infinity makes a row missing too: it has no finite transform.  skipped (may be NULL) receives the
 * number of rows of every group that did not count.  A group without a counted row, or with sum w == 0, gives NaN.  w NULL: unit
 * weights; the weights are expected to be finite.  remove_mean: the row's mean (fp64 sum, rounded to fp32) is subtracted before
 * the transform and P_0 is reported as the fp64 mean squared -- the error of the other wavenumbers then scales with the
 * anomaly's variance instead of the offset's square.
 *   b == NULL: out (groups, K) fp32.    b != NULL, the pair form: out (4, groups, K) = P_aa, P_bb, the co-spectrum
 *   c_k Re(A_k conj B_k) / L^2 and the quadrature spectrum c_k Im(A_k conj B_k) / L^2; out[0] has the bits of the single form on a.
 * The transform runs as an exact-fp32 matrix product with twiddles read from `twiddle`: 2 L floats, {cos, -sin}(2 pi m / L) for
 * m < L interleaved, each evaluated in fp64 and rounded once (the caller makes it once per L; 8-byte aligned).  The rows' terms
 * are added one by one in row order in fp64; a row that does not count adds nothing.  Few groups of very many rows are cut into
 * slabs (then scratch >= dlwpcs_zonal_spectrum_scratch_bytes(d) bytes, 8-byte aligned, holds one fp64 partial per slab and a
 * second launch adds them in order); otherwise the scratch size is 0 and one launch does everything.  At most two launches, no
 * atomics, bitwise repeatable, no host synchronisation, no allocation.  2 <= L <= 1728 (DLWPCS_E_UNSUPPORTED beyond);
 * |X_k|^2 must stay below the fp32 range.  a, b and w need the alignment of their elements only; 16-byte loads are used when
 * L % 4 == 0, every stride of a and b is a multiple of 4 and both pointers are 16-byte aligned.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct dlwpcs_zonal_spectrum_desc {
    int32_t L;                   /* longitudes per row */
    int32_t n_wave;              /* wavenumbers served, 1 .. L/2 + 1; 0: all */
    int32_t n_dims;              /* leading dims, at most DLWPCS_SCORE_MAX_DIMS */
    int32_t remove_mean;
    int64_t ext[DLWPCS_SCORE_MAX_DIMS];
    int32_t kept[DLWPCS_SCORE_MAX_DIMS];          /* 1: indexes the groups, 0: averaged */
    int64_t stride[3][DLWPCS_SCORE_MAX_DIMS];     /* elements: a, b, w */
} dlwpcs_zonal_spectrum_desc;
size_t dlwpcs_zonal_spectrum_scratch_bytes(const dlwpcs_zonal_spectrum_desc *d);
int dlwpcs_zonal_spectrum(const dlwpcs_zonal_spectrum_desc *d, const float *a, const float *b /* NULL: single form */,
                          const float *w /* NULL: unit weights */, const float *twiddle, void *scratch, float *out,
                          int32_t *skipped /* may be NULL */, dlwpcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- *
 * Spherical-harmonic power spectra (DLWP/verify.py spherical_spectrum, spherical_cross_spectrum, spherical_correlation): power
 * per total wavenumber n.  A field is x[i, j] on nlat latitudes (mu_i = sin(lat_i), quadrature weights w_i >= 0, sum w_i = 2)
 * and L equally spaced longitudes (unit stride).  With Pbar_n^m the associated Legendre functions normalised to
 * (1/2) int Pbar_n^m Pbar_n'^m dmu = delta_nn' (no Condon-Shortley phase), for 0 <= m <= n <= T:
 *   X_m(i) = sum_j x[i,j] exp(-2 pi i j m / L),   a_n^m = sum_i (w_i / 2) Pbar_n^m(mu_i) X_m(i) / L,
 *   S_n = sum_{m=0..n} c_m |a_n^m|^2,  c_0 = 1, c_m = 2 otherwise:  sum_n S_n is the area-weighted mean square of a field
 *   band-limited to T, S_0 the squared global mean.
 * The leading axes arrive as n_dims merged dims with an extent and an element stride per operand (0: a, 1: b); they index the
 * FIELDS, row-major in the order given.  Latitude i of a field lies lat_stride elements from latitude 0 (either operand its own).
 *   b == NULL: out (fields, T + 1) fp32.   b != NULL, the pair form: out (3, fields, T + 1) = S_aa, S_bb and the co-spectrum
 *   sum_m c_m Re(a_n^m conj b_n^m); out[0] has the bits of the single form on a.
 * A field that holds a NaN or an infinity (pair form: in a or in b) gets NaN rows; skipped (may be NULL) receives 1 for such a
 * field and 0 for every other, one int32 per field.  Means over fields are dlwpcs_group_mean's business.
 * Two launches.  Stage A, Fourier: (fields x nlat rows x L) . (L x 2 (T + 1)) on v_mfma_f32_32x32x2_f32 with dlwpcs_zonal_spectrum's
 * twiddle table and reduced-index lookup, written to scratch as [operand][field][m][re | im][nlat_pad] fp32, then one int32 per
 * (field, latitude) that says whether the row held a non-finite value; nlat_pad = nlat rounded up to a multiple of 4.  Stage B,
 * Legendre: per order m the product (degrees x nlat) . (nlat x fields) on the same instruction; a workgroup (one wave) owns 32
 * degrees x 32 fields and walks m = 0 .. its last degree in order.  Per m the fp32 products Re^2 + Im^2 (pair: also the two
 * others) are widened to fp64, multiplied by c_m / L^2 and added in order of m; the sum is rounded to fp32 once.  No atomics,
 * bitwise repeatable, no host synchronisation, no allocation: scratch >= dlwpcs_sht_spectrum_scratch_bytes(d), 16-byte aligned.
 * legendre: the caller's table (w_i / 2) Pbar_n^m(mu_i) in fp32, each entry evaluated in fp64 and rounded once, 16-byte
 * aligned: (T + 1)(T + 2) / 2 rows of nlat_pad floats, row (m, n) = m (T + 1) - m (m - 1) / 2 + (n - m), entries i >= nlat zero.
 * twiddle: as for dlwpcs_zonal_spectrum, for this L.
 * Limits: 2 <= L <= 1728 (DLWPCS_E_UNSUPPORTED beyond), 2 <= nlat <= 8192, 0 <= T, 2 T + 1 <= L; 721 x 1440 at T = 360 is served
 * (its table holds 190 MB).  Whether T suits the latitudes' quadrature is the caller's check: the descriptor does not carry it.
 * The grid is (field tiles of 32) x (degree tiles of 32): a handful of fields leaves most of the device idle.
 * ------------------------------------------------------------------------------------------------------------- */
#define DLWPCS_SHT_MAX_NLAT 8192
typedef struct dlwpcs_sht_spectrum_desc {
    int32_t nlat;                /* latitudes */
    int32_t L;                   /* longitudes per row */
    int32_t T;                   /* truncation: degrees 0 .. T */
    int32_t n_dims;              /* leading dims, at most DLWPCS_SCORE_MAX_DIMS */
    int64_t lat_stride[2];       /* elements: a, b */
    int64_t ext[DLWPCS_SCORE_MAX_DIMS];
    int64_t stride[2][DLWPCS_SCORE_MAX_DIMS];     /* elements: a, b */
} dlwpcs_sht_spectrum_desc;
size_t dlwpcs_sht_spectrum_scratch_bytes(const dlwpcs_sht_spectrum_desc *d);
int dlwpcs_sht_spectrum(const dlwpcs_sht_spectrum_desc *d, const float *a, const float *b /* NULL: single form */,
                        const float *twiddle, const float *legendre, void *scratch, float *out,
                        int32_t *skipped /* may be NULL */, dlwpcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- *
 * Spherical-harmonic analysis and synthesis (DLWP/verify.py spherical_analysis, spherical_synthesis, spherical_filter,
 * spherical_laplacian), with the definitions, tables and limits of dlwpcs_sht_spectrum above.
 *
 * dlwpcs_sht_analysis: the coefficients a_n^m of the fields of operand a (operand 0 of the descriptor; operand 1 is not read),
 *   coef[field][row (m, n)][re, im] fp32, dense, (T + 1)(T + 2) / 2 rows per field in the order of the Legendre table, 8-byte
 *   aligned.  Two launches: stage A of dlwpcs_sht_spectrum in its single form, then its stage B storing coefficients: the same
 *   tiles, operand mapping and masks, a workgroup owning 32 degrees x 32 fields x 8 orders.  Rounding: the fp32 sum over the
 *   latitudes is divided by L in fp64 and rounded to fp32 -- ONE rounding of the exact quotient (the quotient of two fp32 numbers
 *   rounded to 53 bits and then to 24 equals the quotient rounded to 24).  Im a_n^0 is what the sum gives (+-0).  A field that
 *   holds a NaN or an infinity gets all-NaN coefficients and a 1 in skipped (may be NULL; 0 for every other field).
 *   scratch >= dlwpcs_sht_analysis_scratch_bytes(d), 16-byte aligned.
 *
 * dlwpcs_sht_synthesis: x[i, j] = sum_{m=0..T} c_m Re( e^{+2 pi i j m / L} sum_{n=m..T} r_n a_n^m Pbar_n^m(mu_i) ), c_0 = 1 and
 *   c_m = 2 otherwise, for every field of coef (layout above), written through the descriptor's leading strides and latitude
 *   stride with longitude at unit stride.  response: T + 1 floats r_n, or NULL, which gives the bits of a response of ones.
 *   Im a_n^0 is ignored.  For a field band-limited to T, synthesis(analysis(x)) = x up to rounding.
 *   legendre here is the UNWEIGHTED table Pbar_n^m(mu_i) in fp32, each entry evaluated in fp64 and rounded once, with the
 *   packing, padding and alignment of the analysis table (it is NOT the analysis table divided by the weights).
 *   Two launches.  Inverse Legendre: per order m the product (latitudes x degrees) . (degrees x fields) on
 *   v_mfma_f32_32x32x2_f32, G_m(i) = sum_n P[(m, n)][i] fl(r_n a_n^m) with the degrees in order, two per instruction; a workgroup
 *   (one wave) owns one order, 32 latitudes and 32 fields; written to scratch as gs[field][m][re | im][nlat_pad].  Inverse
 *   Fourier: per 32 rows (field, latitude) and 32 longitudes one instruction per order m = 0 .. T in order, the operands
 *   {c_m cos, -c_m sin}(2 pi j m / L) from dlwpcs_zonal_spectrum's twiddle table at the reduced index (j m) mod L and {Re, Im} G_m;
 *   16-byte stores where L, the strides and the pointer are multiples of 4 elements, element stores of the same values otherwise.
 *   Masked degrees, latitudes, longitudes and fields are selected to zero in both operands.  A field with NaN coefficients comes
 *   out NaN and touches no other field.  scratch >= dlwpcs_sht_synthesis_scratch_bytes(d), 16-byte aligned.
 * Both: no atomics, a fixed summation order (bitwise repeatable), no host synchronisation, no allocation; a field's result
 * depends on its own data only; zero fields is success without a launch.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct dlwpcs_sht_synthesis_desc {
    int32_t nlat;                /* latitudes */
    int32_t L;                   /* longitudes per row */
    int32_t T;                   /* truncation: degrees 0 .. T */
    int32_t n_dims;              /* leading dims of the output, at most DLWPCS_SCORE_MAX_DIMS */
    int64_t lat_stride;          /* elements between the latitudes of a field of the output */
    int64_t ext[DLWPCS_SCORE_MAX_DIMS];
    int64_t stride[DLWPCS_SCORE_MAX_DIMS];        /* elements */
} dlwpcs_sht_synthesis_desc;
size_t dlwpcs_sht_analysis_scratch_bytes(const dlwpcs_sht_spectrum_desc *d);
int dlwpcs_sht_analysis(const dlwpcs_sht_spectrum_desc *d, const float *a, const float *twiddle, const float *legendre,
                        void *scratch, float *coef, int32_t *skipped /* may be NULL */, dlwpcs_stream_t stream);
size_t dlwpcs_sht_synthesis_scratch_bytes(const dlwpcs_sht_synthesis_desc *d);
int dlwpcs_sht_synthesis(const dlwpcs_sht_synthesis_desc *d, const float *coef, const float *response /* NULL: ones */,
                         const float *twiddle, const float *legendre, void *scratch, float *out, dlwpcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- *
 * Vector spherical harmonics (DLWP/verify.py spherical_uv, spherical_vrtdiv, spherical_gradient; DLWP/barotropic), with the
 * definitions, packing, twiddle table and limits of dlwpcs_sht_spectrum above.  With phi the latitude and
 * eps_n^m = sqrt((n^2 - m^2) / (4 n^2 - 1)) the caller supplies two more fp32 tables in the packing, padding and alignment of the
 * Legendre table, each entry evaluated in fp64 and rounded once (DLWP/remap/spharm.py derivative_table, zonal_table):
 *   D_n^m(mu_i) = dPbar_n^m / dphi = [ -n eps_{n+1}^m Pbar_{n+1}^m + (n + 1) eps_n^m Pbar_{n-1}^m ] / cos(phi_i)
 *   Q_n^m(mu_i) = m Pbar_n^m / cos(phi_i);      at a pole row both are their limits (zero but for m = 1).
 * The descriptor is dlwpcs_sht_spectrum_desc with operand 0 = u and operand 1 = v (each its own leading and latitude strides,
 * longitude at unit stride).  Coefficients are fp32 {re, im} pairs, dense, (T + 1)(T + 2) / 2 rows per field, 8-byte aligned.
 *
 * dlwpcs_sht_vector_synthesis: with psi_n^m = fl(rpsi_n A_n^m), chi_n^m = fl(rchi_n B_n^m) (coef_a = A, coef_b = B; rpsi, rchi:
 *   T + 1 floats or NULL = ones with the same bits; Im of order 0 enters as zero),
 *     u = -dpsi/dphi + (1/cos) dchi/dlambda,  v = (1/cos) dpsi/dlambda + dchi/dphi:
 *     U_m(i) = sum_n [ -D psi + i Q chi ],   V_m(i) = sum_n [ i Q psi + D chi ],   then the inverse Fourier stage of the synthesis.
 *   The factor 1 / radius belongs in the responses.  dtable, qtable: the UNWEIGHTED D and Q.  Either potential may be NULL and
 *   then costs no matrix instruction; both NULL is refused.  Three launches: the inverse vector Legendre stage -- the grid and
 *   tile of the scalar one, four accumulators, the factor i carried as the exact swap and negation of the B operand, per pair of
 *   degrees the psi term before the chi term -- into scratch as gs[u | v][field][m][re | im][nlat_pad], then the scalar
 *   synthesis' inverse Fourier kernel once per component through that output's strides.  Masked degrees, latitudes, longitudes
 *   and fields are selected to zero in both operands.  scratch >= dlwpcs_sht_vector_synthesis_scratch_bytes(d), 16-byte aligned.
 *
 * dlwpcs_sht_vector_analysis: with X_m stage A of dlwpcs_sht_spectrum in its pair form (U_m, V_m),
 *     vrt_n^m = r_n sum_i [ i wQ V_m + wD U_m ] / L,     div_n^m = r_n sum_i [ i wQ U_m - wD V_m ] / L,
 *   wdtable, wqtable the WEIGHTED tables (w_i / 2) D and (w_i / 2) Q; response: T + 1 floats r_n (1 / radius for vorticity and
 *   divergence) or NULL = ones with the same bits.  Either output may be NULL and its matrix work is skipped; both NULL is
 *   refused.  Two launches: stage A, then the coefficient stage with the grid, tiles and masks of dlwpcs_sht_analysis and up to
 *   four accumulators; per latitude the wD term before the wQ term in vrt, the wQ term before the wD term in div.  Rounding: the
 *   fp32 sum over the latitudes is widened to fp64, divided by L and multiplied by r_n there, and rounded to fp32 once.  A field
 *   with a NaN or an infinity in u or in v gets all-NaN coefficients in both outputs and a 1 in skipped (may be NULL; 0 for every
 *   other field).  scratch >= dlwpcs_sht_vector_analysis_scratch_bytes(d), 16-byte aligned.
 * Both: no atomics, a fixed summation order (bitwise repeatable), no host synchronisation, no allocation; a field's result
 * depends on its own data only; zero fields is success without a launch.
 * ------------------------------------------------------------------------------------------------------------- */
size_t dlwpcs_sht_vector_synthesis_scratch_bytes(const dlwpcs_sht_spectrum_desc *d);
int dlwpcs_sht_vector_synthesis(const dlwpcs_sht_spectrum_desc *d, const float *coef_a /* may be NULL */,
                                const float *coef_b /* may be NULL */, const float *rpsi /* NULL: ones */,
                                const float *rchi /* NULL: ones */, const float *twiddle, const float *dtable, const float *qtable,
                                void *scratch, float *out_u, float *out_v, dlwpcs_stream_t stream);
size_t dlwpcs_sht_vector_analysis_scratch_bytes(const dlwpcs_sht_spectrum_desc *d);
int dlwpcs_sht_vector_analysis(const dlwpcs_sht_spectrum_desc *d, const float *u, const float *v, const float *response /* NULL: ones */,
                               const float *twiddle, const float *wdtable, const float *wqtable, void *scratch,
                               float *vrt /* may be NULL */, float *div /* may be NULL */, int32_t *skipped /* may be NULL */,
                               dlwpcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- *
 * The barotropic vorticity model's streaming kernels (DLWP/barotropic).  One launch each, on the current stream, no atomics, no
 * host synchronisation, no allocation; 16-byte accesses where the extents and pointers allow, element accesses of the same values
 * otherwise; every operation one fp32 rounding in the order written (no contraction).  Zero fields is success without a launch.
 *
 * dlwpcs_barotropic_flux: F = (f_i + zeta) u, G = (f_i + zeta) v on dense (fields, nlat, L) fp32 grids; coriolis: nlat floats f_i.
 *
 * dlwpcs_barotropic_update: one time step on dense (fields, rows) fp32 {re, im} coefficients, in place, Re and Im alike, with
 *   d = damp[row] (rows floats, the damping rate of the row's degree):
 *     t = (tend - d zeta_prev) / (1 + d dt)
 *     first_step != 0:  new = zeta + dt t,            zeta' = zeta + robert (new - zeta)
 *     otherwise:        z1 = zeta + robert (zeta_prev - 2 zeta),  new = zeta_prev + (2 dt) t,  zeta' = z1 + robert new
 *     zeta_prev <- zeta',  zeta <- new.
 *   tend, zeta and zeta_prev must be three buffers.
 * Limits: fields * nlat < 2^31 (flux), fields and rows < 2^31 (update), and at most 65536 * 65535 workgroups of 256 threads
 * (four elements or one coefficient per thread); beyond: DLWPCS_E_UNSUPPORTED, before any launch.
 * ------------------------------------------------------------------------------------------------------------- */
int dlwpcs_barotropic_flux(int64_t fields, int32_t nlat, int32_t L, const float *coriolis, const float *zeta, const float *u,
                           const float *v, float *F, float *G, dlwpcs_stream_t stream);
int dlwpcs_barotropic_update(int64_t fields, int64_t rows, const float *damp, float dt, float robert, int32_t first_step,
                             const float *tend, float *zeta, float *zeta_prev, dlwpcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- *
 * Ensemble scores (DLWP/verify.py ensemble_mean, ensemble_spread, ensemble_crps, ensemble_error, rank_histogram): the member
 * axis of an fp32 ensemble collapsed element by element.  The element dims arrive as n_dims merged dims with an extent and an
 * element stride per operand (0: ens, 1: valid; 0 = broadcast), the members lie member_stride elements apart: a permuted view
 * or a member axis in the middle needs no copy.  With the members x_1..x_M of an element and its verification y, in fp32:
 *   mean    x_1 + (sum_i (x_i - x_1)) / M
 *   spread  sqrt(sum_i ((x_i - x_1) - tbar)^2 / (M - ddof)), tbar the mean of the x_i - x_1; `variance`: its square instead
 *   crps    A - B / 2,  A = (1 / M) sum_i |x_i - y|,  B = sum_ij |x_i - x_j| / M^2  (`fair`: / (M (M - 1))), evaluated as the
 *           integral of (F(t) - 1{t >= y})^2 over the gaps of the SORTED differences d_i = x_i - y: a sum of non-negative terms
 *           k^2 (part of gap k below y) + (M - k)^2 (part above y), over M^2, plus the tail |d| beyond the ensemble; the fair
 *           form subtracts sum_k k (M - k) gap_k / (M^2 (M - 1)).  No offset of the data reaches the error, M identical members
 *           give spread 0 and crps = the fp32 |x - y| exactly.
 *   rank    the number of members with x_i < y (the inputs compared as they are), 0..M
 * An element with a NaN or infinite member gets NaN in mean, spread and crps and -1 in rank; a NaN or infinite y gets NaN in
 * crps and -1 in rank only.  Outputs (each may be NULL: not computed) are contiguous in the row-major order of the element
 * dims; crps and rank need valid.  2 <= M <= 128 (DLWPCS_E_UNSUPPORTED beyond): M <= 32 is sorted by a compare-exchange network
 * in registers (classes of 4, 8, 16, 32 slots, the unused ones never enter a sum), 33..128 in lane-private columns of LDS
 * (classes of 64 and 128).  Lanes run along the LAST element dim: list the dim that is contiguous in ens last.  16-byte loads
 * (four elements per lane) in the classes up to 16 when that dim has stride 1 and an extent that is a multiple of 4, every other
 * stride of ens and member_stride are multiples of 4 and ens is 16-byte aligned; one element per lane otherwise -- the same bits.
 * One launch, no scratch, no atomics, no allocation, no host synchronisation (capturable).  A zero extent launches nothing.
 *
 * dlwpcs_ensemble_plan_info (host only; the pointers are looked at for NULL and alignment, never dereferenced): info[0] = the
 * class (slots: 4, 8, 16, 32, 64, 128), info[1] = 1: 16-byte loads of ens, 0: one element per load, info[2] = how valid is read
 * (-1: absent, 0: element by element, 1: 16-byte loads), info[3] = 1: members in LDS, 0: in registers, info[4] / info[5] = the
 * grid, info[6] = threads of a workgroup, info[7] = 0.  Returns what the entry point would return for the descriptor.
 * ------------------------------------------------------------------------------------------------------------- */
#define DLWPCS_ENSEMBLE_MAX_M 128
typedef struct dlwpcs_ensemble_desc {
    int32_t M;                   /* members, 2 .. DLWPCS_ENSEMBLE_MAX_M */
    int32_t n_dims;              /* element dims, at most DLWPCS_SCORE_MAX_DIMS */
    int32_t fair;                /* crps: pair term over M (M - 1) */
    int32_t ddof;                /* spread: 0 or 1 */
    int32_t variance;            /* out_spread holds the variance */
    int32_t reserved;
    int64_t member_stride;       /* elements */
    int64_t ext[DLWPCS_SCORE_MAX_DIMS];
    int64_t stride[2][DLWPCS_SCORE_MAX_DIMS];     /* elements: ens, valid */
} dlwpcs_ensemble_desc;
int dlwpcs_ensemble_stats(const dlwpcs_ensemble_desc *d, const float *ens, const float *valid /* may be NULL */,
                          float *out_mean, float *out_spread, float *out_crps, int32_t *out_rank, dlwpcs_stream_t stream);
int dlwpcs_ensemble_plan_info(const dlwpcs_ensemble_desc *d, const void *ens, const void *valid, int32_t info[8]);

/* ------------------------------------------------------------------------------------------------------------- *
 * Category scores of an ensemble (DLWP/verify.py ensemble_probability, brier_score, ranked_probability_score,
 * categorical_error, reliability_counts): per element, with members x_1..x_M, thresholds t_0 <= .. <= t_{Q-1} (their order is
 * the caller's business, nothing checks it) and verification y,
 *   k_j = #{i : x_i <= t_j},   o_j = 1{y <= t_j}.
 * Operands as in dlwpcs_ensemble_stats: merged element dims with a stride in elements per operand (0: ens, 1: valid, 2: thr;
 * 0 = broadcast), members member_stride apart, thresholds thr_stride apart.  Outputs (each may be NULL) are contiguous in the
 * row-major order of the element dims, E elements; the per-threshold ones have the threshold as the leading dim:
 *   prob    (Q, E)  (float)k_j / (float)M
 *   brier   (Q, E)  e_j * e_j,  e_j = (float)(k_j - o_j M) / (float)M
 *   rps     (E)     brier_0 + brier_1 + .. added in that order from 0.f; `fair`: minus
 *                   (float)(sum_j k_j (M - k_j)) / ((float)(M M) * (float)(M - 1))   (needs M >= 2)
 *   rps_ref (E)     sum_j (ref_prob[j] - (float)o_j)^2 in the same order from 0.f
 *   code    (Q, E)  int32 2 k_j + o_j: what a reliability diagram is counted from
 * Every fp32 operation happens once, in that order, with contraction off; the integers are exact (the fair sum stays below 2^24).
 * Missing values: an element with a NaN or infinite member is NaN / -1 in every output; a NaN or infinite y in brier, rps,
 * rps_ref and code (prob is still given); a NaN t_j in threshold j's outputs and in rps and rps_ref; +-inf thresholds are
 * compared as they are.  Without valid only prob may be asked for.  1 <= M <= DLWPCS_CATEGORY_MAX_M and 1 <= Q <=
 * DLWPCS_CATEGORY_MAX_Q, DLWPCS_E_UNSUPPORTED beyond.  One lane per element, thresholds and counters in registers (classes of
 * 1, 2, 4, 8, 16 thresholds; unused slots hold +inf and are never stored), one loop over the members that reads ens once.  16-byte
 * form (four neighbours along the last dim per lane) in the classes up to 8 under the conditions of dlwpcs_ensemble_stats: the
 * same bits.  One launch, no scratch, no atomics, no allocation, no host synchronisation (capturable); a zero extent launches
 * nothing.
 *
 * dlwpcs_ensemble_category_plan_info (host only; pointers looked at for NULL and alignment): info[0] = the Q class, info[1] = 1:
 * 16-byte loads of ens, info[2] = how valid is read (-1 absent, 0 element by element, 1 16-byte loads), info[3] = how thr is
 * read (0 element by element, 1 16-byte loads, 2 one vector for every element), info[4] / info[5] = the grid, info[6] = threads
 * of a workgroup, info[7] = 0.
 * ------------------------------------------------------------------------------------------------------------- */
#define DLWPCS_CATEGORY_MAX_M 1024
#define DLWPCS_CATEGORY_MAX_Q 16
typedef struct dlwpcs_category_desc {
    int32_t M, Q, n_dims, fair;
    int64_t member_stride, thr_stride;                    /* elements: between members of ens, between thresholds of thr */
    int64_t ext[DLWPCS_SCORE_MAX_DIMS];
    int64_t stride[3][DLWPCS_SCORE_MAX_DIMS];             /* ens, valid, thr; 0 = broadcast */
    float ref_prob[DLWPCS_CATEGORY_MAX_Q];                /* climatological P(y <= t_j): the reference forecast of the skill score */
} dlwpcs_category_desc;
int dlwpcs_ensemble_category(const dlwpcs_category_desc *d, const float *ens, const float *valid /* may be NULL */,
                             const float *thr, float *out_prob, float *out_brier, float *out_rps, float *out_rps_ref,
                             int32_t *out_code, dlwpcs_stream_t stream);
int dlwpcs_ensemble_category_plan_info(const dlwpcs_category_desc *d, const void *ens, const void *valid, const void *thr,
                                       int32_t info[8]);

/* ------------------------------------------------------------------------------------------------------------- *
 * Conservative offline maps made on the device (DLWP/remap/overlap.py is the host twin and states the maths): A[r, c], the
 * area in steradians of (lat-lon cell r) intersected with (equiangular cubed-sphere cell c), in closed form and fp64, in CSR
 * form over the lat-lon cells (lat-major).  The cube is given by its face frames {e0, eu, ev} (centre, width and height
 * direction; a point of face f at edge tangents (x, y) is normalize(e0 + x eu + y ev), the cell edges lie at
 * tan(-pi/4 + k pi / (2N)) with +-1 and 0 exact), the lat-lon grid by sin(latitude) of its n_lat + 1 edges (monotone either
 * way, +-1 exact at a pole) and its n_lon + 1 ascending longitude edges in radians spanning 2 pi.
 * Two phases, so that no atomic decides an order: dlwpcs_overlap_count writes counts[r], the number of entries of row r with
 * A > dust * min(area_r, area_c) (cells that only share an edge give |A| of rounding size); the caller scans the counts
 * exclusively into row_ptr[n_lat * n_lon + 1]; dlwpcs_overlap_fill writes col (cube cells (f * N + i) * N + j, ascending
 * within a row) and area at row_ptr[r] ....  It never writes at or beyond nnz nor beyond a row's end, whatever row_ptr holds.
 * One lane per lat-lon cell; candidates per face come from a bounding cap of the cell, not from all pairs.  The same call
 * gives the same bits.  One launch each, no host synchronisation, no allocation.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct dlwpcs_overlap_desc {
    int32_t N, n_lat, n_lon, reserved;
    double frames[6][3][3];             /* [face][e0, eu, ev][x, y, z] */
    double dust;                        /* >= 0; DLWP.remap uses 1e-10 */
} dlwpcs_overlap_desc;
int dlwpcs_overlap_count(const dlwpcs_overlap_desc *d, const double *sin_lat_edges, const double *lon_edges, int32_t *counts,
                         dlwpcs_stream_t stream);
int dlwpcs_overlap_fill(const dlwpcs_overlap_desc *d, const double *sin_lat_edges, const double *lon_edges,
                        const int64_t *row_ptr, int32_t *col, double *area, int64_t nnz, dlwpcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- *
 * Bilinear sampling of a cubed-sphere field at arbitrary points (DLWP/remap/bilinear.py is the host twin and states the maths):
 * for every point (lat, lon in degrees; any finite longitude) the four cells (f * N + i) * N + j and weights of the face of the
 * cube's DUAL mesh that holds it.  The dual mesh has the cell centres as vertices and great-circle arcs between them as sides:
 * per cube face the quadrilaterals of neighbouring centres, per cube edge a strip of quadrilaterals of the cells on both sides,
 * per cube vertex the triangle of the three corner cells.  In a quadrilateral V0..V3 the weights are the bilinear factors of
 * the (s, t) with (1-s)(1-t) V0 + s(1-t) V1 + s t V2 + (1-s) t V3 = lambda P; in a triangle the barycentric coordinates of the
 * radial projection of P, and the fourth slot repeats the third cell with weight exactly 0.  Weights are >= 0 and sum to 1; the
 * interpolant is continuous across cube edges and corners.  The cube is given by its face frames as in dlwpcs_overlap_desc and by
 * its topology: per face and side (0: width index 0, 1: width N - 1, 2: height 0, 3: height N - 1) the neighbour face, the
 * neighbour's side that is the same cube edge, and 1 when positions along the edge run the other way there.
 * One lane per point, fp64; one launch, no host synchronisation, no allocation, no atomics; the same call gives the same bits.
 * Every col written lies in [0, 6 N^2) whatever the inputs hold; a non-finite point gets cell 0 and NaN weights.
 * n_points == 0: DLWPCS_OK without a launch.  N < 1, frames that are not orthonormal to 1e-9, edge entries out of range:
 * DLWPCS_E_INVALID.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct dlwpcs_cube_bilinear_desc {
    int32_t N, reserved;
    int64_t n_points;
    double frames[6][3][3];             /* [face][e0, eu, ev][x, y, z] */
    int32_t edge[6][4][3];              /* [face][side]{neighbour face, its side, reversed} */
} dlwpcs_cube_bilinear_desc;
int dlwpcs_cube_bilinear(const dlwpcs_cube_bilinear_desc *d, const double *lat_deg, const double *lon_deg,
                         int32_t *col /* [4 n_points] */, double *w /* [4 n_points] */, dlwpcs_stream_t stream);

int dlwpcs_adam_step(float *p, const float *g, float *m, float *v, size_t n, int32_t *step_dev,
                     float lr, float beta1, float beta2, float eps, float grad_scale, dlwpcs_stream_t stream);
/* Same update as one launch: `state_dev` points to TWO device int32 {t-1, 0}; the second is a ticket counter (must be 0
 * between calls, the kernel leaves it 0): the last workgroup to finish increments t-1, so no second launch is needed.
 * DLWPCS_ADAM_ZERO_GRAD: g[i] = 0 after it has been consumed (the next step's gradient accumulation starts from zeros
 * without a fill launch). */
#define DLWPCS_ADAM_ZERO_GRAD 1
int dlwpcs_adam_step_fused(float *p, float *g, float *m, float *v, size_t n, int32_t *state_dev,
                           float lr, float beta1, float beta2, float eps, float grad_scale, int flags,
                           dlwpcs_stream_t stream);
/* Same kernel, hyper-parameters read from DEVICE memory: hyper_dev -> five floats {lr, beta1, beta2, eps, grad_scale}.
 * A step captured in a hipGraph then honours `optimizer.lr = x` / learning-rate schedules between replays (by-value
 * arguments are frozen at capture).  Same element arithmetic as dlwpcs_adam_step_fused -> same bits for equal values. */
int dlwpcs_adam_step_dev(float *p, float *g, float *m, float *v, size_t n, int32_t *state_dev,
                         const float *hyper_dev, int flags, dlwpcs_stream_t stream);

/* Weight regularizers / constraints of CubeSphereConv2D (DLWP/custom.py:837-842 -> add_weight(regularizer=, constraint=), :898-914).
 * dlwpcs_l1l2_regularize: keras regularizers.L1L2 on one fp32 weight: *penalty += l1 * sum|w| + l2 * sum w^2 (penalty may be NULL)
 * and g[i] += (l1 * sign(w[i]) + 2 * l2 * w[i]) * inv_grad_scale (g may be NULL; inv_grad_scale = 1 / the optimizer's grad_scale, so
 * that the penalty's gradient is not averaged over the ranks).  One workgroup, fixed summation order.
 * dlwpcs_weight_constraint: keras constraints on one fp32 weight viewed as a (rows, cols) matrix -- one norm per column, i.e. over
 * the weight's leading axes (axis=[0,1,2] of a (k,k,Cin,Cout) kernel: rows = k*k*Cin, cols = Cout) -- applied in place. */
#define DLWPCS_CONSTRAINT_MAX_NORM     1   /* a = max_value */
#define DLWPCS_CONSTRAINT_NON_NEG      2
#define DLWPCS_CONSTRAINT_UNIT_NORM    3
#define DLWPCS_CONSTRAINT_MIN_MAX_NORM 4   /* a = min_value, b = max_value, rate */
int dlwpcs_l1l2_regularize(const float *w, float *g, size_t n, float l1, float l2, float inv_grad_scale, float *penalty,
                           dlwpcs_stream_t stream);
int dlwpcs_weight_constraint(float *w, int rows, int cols, int kind, float a, float b, float rate, dlwpcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- *
 * Batch feed (reference ArrayDataGenerator.generate, DLWP/model/generators.py:872-984): with the whole data array
 * (T, V, S) fp32 resident in HBM (S = flattened space, e.g. 6*N*N), one launch assembles a batch window
 *   channels_last : out[b][s][c_off + n*c_stride + j] = array[samples[b] + t_off + n*t_stride][var_idx[j]][s]
 *   channels_first: out[b][c_off + n*c_stride + j][s] = (same)
 * for n < n_steps, j < nv.  out is (B, S, Ctot) or (B, Ctot, S) of `dtype` (fp32 source rounded to bf16 on the fly).
 * The caller guarantees samples[b] + t_off + (n_steps-1)*t_stride < T.  Predictors, insolation channels and targets
 * of a batch are three calls with different (array, var_idx, c_off, c_stride, t_off).
 * ------------------------------------------------------------------------------------------------------------- */
int dlwpcs_batch_gather(const void *array, int64_t T, int V, int64_t S, const int32_t *samples_dev, int B,
                        const int32_t *var_idx_dev, int nv, int n_steps, int t_off, int t_stride, void *out,
                        int Ctot, int c_off, int c_stride, int channels_last, int dtype, dlwpcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- *
 * Solar forcing (reference DLWP/util.py:306-364): the computing twin of a one-variable (nv = 1) batch_gather out of a dense
 * (T, 1, S) insolation array.  Same output addressing, row r = samples[b] + t_off + n*t_stride (the caller guarantees
 * 0 <= r < T), but the value is computed from two host-built fp64 tables (DLWP.util.SolarForcing) instead of read:
 *   row_tab  (T, 4): {sin(decl), cos(decl), S0 * dist^-2, day}  -- day holds the host's fp32 fractional day of the year
 *   cell_tab (S, 3): {sin(phi), cos(phi), lon / 360}            -- lon / 360 holds the host's fp32 quotient
 *   out[..] = max(0, scale[r] * (sinphi[s] * sindec[r] - cosphi[s] * cosdec[r] * cos(hour))),  hour = f32(2 pi) * (day[r] + lonfrac[s])
 * hour is formed with two rounded fp32 operations exactly as the host forms it, the cosine is the accurate cosf, the combine is
 * fp64 without contraction, the result is rounded to fp32 and then to `dtype`: the result differs from DLWP.util.insolation only
 * through the cosine, and a bf16 output is the round-to-nearest-even of the fp32 output.
 * ------------------------------------------------------------------------------------------------------------- */
int dlwpcs_solar_fill(const double *row_tab, int64_t T, const double *cell_tab, int64_t S, const int32_t *samples_dev, int B,
                      int n_steps, int t_off, int t_stride, void *out, int Ctot, int c_off, int c_stride, int channels_last,
                      int dtype, dlwpcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- *
 * Per-variable data scaling (reference DLWP/model/preprocessing.py:645-682 data_to_series(scale_variables=True), :844-882
 * mean_by_batch / std_by_batch; Tutorial 4 cell 19 undoes it on every forecast).  Both calls see an fp32 device array as
 * (R rows, C channels, S inner elements), element (r, c, s) at r * row_stride + c * chan_stride + s * inner_stride, strides in
 * ELEMENTS and >= 0:
 *   channels-first (T, V, S):      R = T, C = V, strides (V * S, S, 1)
 *   channels-last  (R * S, C):     the row extent folded into S: R = 1, strides (0, 1, C), or (S * C, 1, C)
 * dst_* are the strides of the output of dlwpcs_channel_affine (dlwpcs_channel_moments ignores them).
 *
 * dlwpcs_channel_moments: out[c] = {n, s1, s2} (double[C][3]) over the selected rows and all S inner elements of channel c:
 * n = the count, s1 = sum (x - center[c]), s2 = sum (x - center[c])^2, the difference formed in fp64, the sums fp64.
 * center: fp64 device table of C entries, NULL = 0.  rows: int32 device list of n_rows source rows (the training subset;
 * duplicates and any order are legal and counted as given; every entry in [0, R) -- TRUSTED), NULL = all R rows in order
 * (n_rows is ignored).  skipna = 0: NaN propagates into s1 / s2 (numpy .sum()) and n counts every element; 1: NaN elements
 * are left out of all three.  No floating-point atomics: launch 1 gives every (channel, column tile, row slab) a workgroup
 * that writes one partial triple to scratch, launch 2 adds a channel's partials in index order -- the partition depends on
 * the descriptor and n_rows only, so two calls give the same bits.  scratch >= dlwpcs_channel_moments_scratch_bytes(d, n_rows)
 * (n_rows <= 0 there = all rows), 8-byte aligned.  16-byte loads when inner_stride == 1, S % 4 == 0 and every row / channel
 * start is 16-byte aligned; one element per lane, any strides, otherwise.
 *
 * dlwpcs_channel_affine: dst(r, c, s) = src(r, c, s) * a[c] + b[c]   (DLWPCS_AFFINE_MUL_ADD: Tutorial 4 cell 19)
 *                                    or (src(r, c, s) - b[c]) / a[c]   (DLWPCS_AFFINE_SUB_DIV: preprocessing.py:660)
 * with fp32 device tables a, b of C entries.  Two separately rounded fp32 operations, never an fma; NaN / inf as IEEE gives
 * them.  Source and destination have their own strides (channels-last in, channels-first out is cell 17 + 19 in one launch);
 * dst == src with equal strides is legal, any other overlap is not.  Paths: both sides inner-contiguous with S % 4 == 0 and
 * 16-byte aligned: 16-byte loads and stores along a row; both sides one flat channels-last stream (chan stride 1, inner stride
 * C, rows back to back): 16-byte loads and stores over the stream, the tables in LDS; anything else: one element per lane,
 * lanes along the destination's contiguous dim.  C > DLWPCS_AFFINE_MAX_CHANNELS or more than 2^31 - 1 elements in a row of
 * the one-element path: DLWPCS_E_UNSUPPORTED.
 * One launch (moments: two), no host synchronisation, no allocation.  A zero extent returns DLWPCS_OK without a launch
 * (moments: out is zeroed).
 * ------------------------------------------------------------------------------------------------------------- */
#define DLWPCS_AFFINE_MUL_ADD 0
#define DLWPCS_AFFINE_SUB_DIV 1
#define DLWPCS_AFFINE_MAX_CHANNELS 1024
typedef struct dlwpcs_chan_desc {
    int64_t R, C, S;
    int64_t row_stride, chan_stride, inner_stride;
    int64_t dst_row_stride, dst_chan_stride, dst_inner_stride;
} dlwpcs_chan_desc;
size_t dlwpcs_channel_moments_scratch_bytes(const dlwpcs_chan_desc *d, int64_t n_rows);
int dlwpcs_channel_moments(const dlwpcs_chan_desc *d, const float *src, const int32_t *rows, int64_t n_rows,
                           const double *center, int skipna, double *out, void *scratch, size_t scratch_bytes,
                           dlwpcs_stream_t stream);
int dlwpcs_channel_affine(const dlwpcs_chan_desc *d, const float *src, const float *a, const float *b, int mode, float *dst,
                          dlwpcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- *
 * The resident series in 16-bit packed form (the CF / netCDF convention, the one ERA5 is distributed in):
 *   x = q * scale[v] + offset[v]
 * with q an int16 code in [-32767, 32767], code -32768 = missing (decodes to NaN), scale and offset fp32 device tables of V
 * entries, scale != 0 (it may be negative).  All arrays are contiguous (T, V, S).  Every arithmetic step below is ONE rounded
 * fp32 operation, never an fma, so numpy's float32 arithmetic gives the same bits.
 *
 * dlwpcs_channel_range: range[v] = {min, max} (float[V][2]) over the FINITE elements of variable v, {+inf, -inf} when it has
 * none; nonfinite[v] (int64[V]) = the number of NaN / +-inf elements.  Exact: neither depends on the order.  Two launches
 * (per-workgroup partials in scratch, then one workgroup per variable); scratch >= dlwpcs_channel_range_scratch_bytes(T, V, S),
 * 8-byte aligned.  16-byte loads when S % 4 == 0 and src is 16-byte aligned, one element per lane otherwise.  T == 0 or S == 0
 * writes the empty range; V == 0 returns DLWPCS_OK without a launch.
 *
 * dlwpcs_pack_i16: dst = clamp(rint((src - offset[v]) / scale[v]), -32767, 32767): subtract, IEEE divide, round half to even,
 * clamp; a NaN or +-inf source element gives -32768.
 * dlwpcs_unpack_i16: dst = float(src) * scale[v], then + offset[v]; -32768 gives NaN (0x7fc00000).
 * Both: one launch; a lane moves 8 elements with 16-byte accesses when S % 8 == 0 and both pointers are 16-byte aligned, single
 * elements otherwise.  A zero extent returns DLWPCS_OK without a launch.
 *
 * dlwpcs_batch_gather_i16: the decoding twin of dlwpcs_batch_gather -- same arguments, output addressing, limits and error codes --
 * out of an int16 array:
 *   channels_last : out[b][s][c_off + n*c_stride + j] = decode(array[samples[b] + t_off + n*t_stride][var_idx[j]][s])
 *   channels_first: out[b][c_off + n*c_stride + j][s] = (same)
 * decode(q) = float(q) * scale[var_idx[j]] + offset[var_idx[j]] as above, the fp32 value then stored as `dtype`: a bf16 output
 * is the round-to-nearest-even of the fp32 output (the NaN of a fill code: 0x7fc0).  Three forms.  channels_last, the gathered channels being the whole output row
 * (c_off == 0, c_stride == nv, Ctot == n_steps * nv), S % 8 == 0, array and out 16-byte aligned, n_steps * nv * 257 floats of LDS
 * <= 64 KiB: 256 pixels x all channels per workgroup, a lane loads 16 bytes = 8 codes, the output is written as 16-byte vectors.
 * Any other channels_last call (any S, a channel window inside a wider row, an unaligned pointer): 64 pixels x all channels
 * through a padded LDS tile, one code per lane.  channels_first: rows copied along s, 8 codes per lane when S % 8 == 0 and both
 * pointers are 16-byte aligned, one otherwise.  The samples are TRUSTED, as in dlwpcs_batch_gather.
 * ------------------------------------------------------------------------------------------------------------- */
size_t dlwpcs_channel_range_scratch_bytes(int64_t T, int64_t V, int64_t S);
int dlwpcs_channel_range(const float *src, int64_t T, int64_t V, int64_t S, float *range, int64_t *nonfinite, void *scratch,
                         size_t scratch_bytes, dlwpcs_stream_t stream);
int dlwpcs_pack_i16(const float *src, int64_t T, int64_t V, int64_t S, const float *scale, const float *offset, int16_t *dst,
                    dlwpcs_stream_t stream);
int dlwpcs_unpack_i16(const int16_t *src, int64_t T, int64_t V, int64_t S, const float *scale, const float *offset, float *dst,
                      dlwpcs_stream_t stream);
int dlwpcs_batch_gather_i16(const int16_t *array, int64_t T, int V, int64_t S, const float *scale, const float *offset,
                            const int32_t *samples_dev, int B, const int32_t *var_idx_dev, int nv, int n_steps, int t_off,
                            int t_stride, void *out, int Ctot, int c_off, int c_stride, int channels_last, int dtype,
                            dlwpcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- *
 * Data-parallel exchange: ONE in-place sum of the flat fp32 gradient buffer over the ranks, through an RCCL
 * communicator the caller owns, enqueued on the CALLER's stream -- inside a captured training step the collective is a plain
 * node of the step's graph between dlwpcs_wgrad_batch (reduction into the buffer) and dlwpcs_wgrad_batch_apply.
 * Reference counterpart: keras.utils.multi_gpu_model, DLWP/model/models.py:369-374 (host-side averaging over replicas).
 *   dlwpcs_comm_load(path):    dlopen RCCL (the librccl.so PyTorch ships: one RCCL per process); once per process
 *   dlwpcs_comm_unique_id(id): 128 bytes from ncclGetUniqueId -- rank 0 calls it and hands the bytes to the other ranks
 *   dlwpcs_comm_init(&comm, id, rank, world): ncclCommInitRank on the calling thread's current device (collective: every rank)
 *   dlwpcs_allreduce_f32(comm, buf, n, stream): ncclAllReduce(sum, in place); capturable; no host synchronisation
 *   dlwpcs_comm_destroy(comm)
 * ------------------------------------------------------------------------------------------------------------- */
int dlwpcs_comm_load(const char *librccl_path);
int dlwpcs_comm_unique_id(void *id128);
int dlwpcs_comm_init(void **comm, const void *id128, int rank, int world);
int dlwpcs_comm_destroy(void *comm);
int dlwpcs_allreduce_f32(void *comm, float *buf, size_t n, dlwpcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- *
 * Hardware self-check of the gather-form data gradient (DLWPCS_CONV_DGRAD_GATHER): its kernel masks MFMA operands by
 * address -- lanes that must add nothing read LDS beyond the workgroup's allocation, which returns zeros on gfx950.
 * Writes to *nonzero_dev (device int32, caller-owned) the number of non-zero dwords such reads returned at the offsets
 * the kernel uses: 0 = the assumption holds on this device.
 * ------------------------------------------------------------------------------------------------------------- */
int dlwpcs_lds_oob_probe(int32_t *nonzero_dev, dlwpcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- *
 * Opt-in launch profiler (bench.py `roofline`): when enabled, every MFMA convolution kernel launch is bracketed by two
 * HIP events recorded on the launch stream.  Off by default.  Enabled while a stream is being graph-captured, the events
 * become external event-record nodes of that graph (tag suffix "@graph"): every replay records them again and
 * dlwpcs_prof_get returns the duration of the launch inside the last completed replay; destroy the graph before
 * dlwpcs_prof_reset.
 * dlwpcs_prof_get: tag = kernel name as rocprofv3 prints it (template arguments included), ms = event-elapsed time,
 * flops / bytes = ALGORITHMIC work of that launch (2*B*6*N^2*k^2*Cin*Cout; unpadded tensors touched once + weights).
 * ------------------------------------------------------------------------------------------------------------- */
int dlwpcs_prof_enable(int on);
int dlwpcs_prof_reset(void);
int dlwpcs_prof_count(void);
int dlwpcs_prof_get(int i, char *tag, int tag_len, double *ms, double *flops, double *bytes);
/* Host only, no device needed: the tags the profiler can report -- one per kernel instantiation the library carries, registered
 * when the library is loaded.  A tag is the kernel's name exactly as the code object / rocprofv3 / `nm -C` spell it (a suffix in
 * parentheses names a mode of the same kernel).  dlwpcs_prof_known_tags: how many; dlwpcs_prof_known_tag: the i-th. */
int dlwpcs_prof_known_tags(void);
int dlwpcs_prof_known_tag(int i, char *tag, int tag_len);

#ifdef __cplusplus
}
#endif
#endif /* DLWPCS_H */
