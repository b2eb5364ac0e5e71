/* afd.h -- C ABI of libafd_hip.so: the MI355X (gfx950) engine under the alias-free DDPM hot path.
 *
 * The reference (MDFahimAnjum/AliasFree-Diffusion-Models-PyTorch) has no FFI: its hot path is a
 * plain Python API over torch ATen ops.  Each entry point below names the reference lines whose
 * device work it replaces (paths relative to the reference root).  The Python host package binds
 * these with ctypes; nothing here takes or returns a torch type.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 (NCHW, contiguous unless a stride is given) except
 *     where a parameter is documented as HOST (filter taps, shape tables);
 *   - `stream` is a hipStream_t passed as void*; entry points only enqueue work: they never
 *     allocate, never synchronise and are legal inside hipGraph stream capture;
 *   - workspaces are caller-provided; `*_workspace_bytes` tells how much;
 *   - return value: AFD_OK or an AFD_E* code; afd_last_error() gives the message for this thread.
 *   - batch strides are in ELEMENTS; 0 means "contiguous" (C*H*W of that tensor).
 */
#ifndef AFD_H_
#define AFD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AFD_OK 0
#define AFD_EINVAL 1     /* null pointer, non-positive size, unsupported shape */
#define AFD_ELAUNCH 2    /* hip launch / runtime error */
#define AFD_MAX_TAPS 15  /* largest supported filter side N */

typedef void* afd_stream_t;

const char* afd_version(void);
const char* afd_last_error(void);
/* number of HIP devices visible (0 on a CPU-only host); never initialises a context */
int afd_device_count(void);

/* ---- F1: filter design (HOST code, no GPU) -------------------------------------- filtrs.py:20-37
 * N x N radial jinc * outer-product Kaiser(beta) window, sum-normalised, fp64 -> fp32.
 * taps_out: HOST float[N*N].  has_beta = 0 reproduces beta=None. */
int afd_lowpass_kernel(double omega_c, int N, int has_beta, double beta, float* taps_out);

/* ---- F2: custom_upsample(x, f, factor=2) ---------------------------------------- filtrs.py:79-94
 * x (B,C,H,W) -> y (B,C,2H,2W).  taps: HOST float[N*N].  *_bwd is the exact adjoint (dx from dy). */
int afd_filt_up2_fwd(const float* x, float* y, int B, int C, int H, int W, long x_bstride, long y_bstride,
                     const float* taps, int N, afd_stream_t stream);
int afd_filt_up2_bwd(const float* dy, float* dx, int B, int C, int H, int W, long dy_bstride, long dx_bstride,
                     const float* taps, int N, afd_stream_t stream);

/* ---- F3: custom_downsample(x, f, factor=2) -------------------------------------- filtrs.py:71-77
 * x (B,C,H,W) -> y (B,C,ceil(H/2),ceil(W/2)) (even rows / columns of the filtered image). */
int afd_filt_down2_fwd(const float* x, float* y, int B, int C, int H, int W, long x_bstride, long y_bstride,
                       const float* taps, int N, afd_stream_t stream);
int afd_filt_down2_bwd(const float* dy, float* dx, int B, int C, int H, int W, long dy_bstride, long dx_bstride,
                       const float* taps, int N, afd_stream_t stream);

/* ---- F4: filtered nonlinearity  y = down2(GELU_erf(up2(v)))  ------------ ddpm_utils.py:123-125,129-131
 * Optional fused prologue (any pointer may be NULL):
 *     v[b,c,:,:] = x[b,c,:,:] * (rstd[b]*gamma[c]) + (beta[c] - mean[b]*rstd[b]*gamma[c]) + res[b,c,:,:]
 * i.e. GroupNorm(1,C)-apply (ddpm_utils.py:122,127) and the residual add (:128) folded into the load.
 * stats: float[B*2] = {mean, rstd} per sample, or NULL (then gamma/beta are ignored).
 * workspace: only read when the shape is off the fused fast path (N != 3 or a non-square /
 * non-power-of-two plane); size from afd_filt_act_workspace_bytes (0 on the fast path).
 * bwd writes dv = dL/dv (same shape as x); the caller chains dv into GroupNorm-backward / the residual.
 * gn_partials (or NULL; needs stats; fused fast path only): the kernel also emits GroupNorm-backward's
 * per-plane sums of dv, layout (B,2,C) -- pass them to afd_groupnorm1_bwd with have_partials = 1. */
size_t afd_filt_act_workspace_bytes(int B, int C, int H, int W, int N, int backward);
int afd_filt_act_fwd(const float* x, float* y, int B, int C, int H, int W,
                     const float* stats, const float* gamma, const float* beta, const float* res,
                     const float* taps_up, const float* taps_down, int N,
                     void* workspace, afd_stream_t stream);
/* the forward INCLUDING the GroupNorm(1,C) statistics, for samples small enough that one workgroup holds one (C * H <= 1024
 * threads, H = W in {4, 8, 16}, N = 3: afd_filt_act_fwd_gn_supported != 0): the statistics launch disappears; stats_out
 * (B*2) receives {mean, rstd} for the backward entry points. */
size_t afd_filt_act_fwd_gn_supported(int C, int H, int W, int N);
int afd_filt_act_fwd_gn(const float* x, float* y, int B, int C, int H, int W, float eps, float* stats_out,
                        const float* gamma, const float* beta, const float* res,
                        const float* taps_up, const float* taps_down, int N, afd_stream_t stream);
/* ... and the backward that also finishes GroupNorm's backward for such samples: dx = dL/dx of the GroupNorm INPUT leaves
 * instead of dv (dres, or NULL: also write dv = the residual branch's gradient); gn_partials (B,2,C) as in afd_filt_act_bwd --
 * the caller still folds them into dgamma / dbeta (afd_colsum2).  No afd_groupnorm1_bwd call for these sites. */
int afd_filt_act_bwd_gn(const float* x, const float* dy, float* dx, float* dres, int B, int C, int H, int W, const float* stats,
                        const float* gamma, const float* beta, const float* res, const float* taps_up, const float* taps_down, int N,
                        float* gn_partials, afd_stream_t stream);
int afd_filt_act_bwd(const float* x, const float* dy, float* dv, int B, int C, int H, int W,
                     const float* stats, const float* gamma, const float* beta, const float* res,
                     const float* taps_up, const float* taps_down, int N,
                     void* workspace, float* gn_partials, afd_stream_t stream);

/* ---- F6: nn.GroupNorm(1, C), eps, affine ---------------------------- ddpm_utils.py:85,88,113,116
 * fwd: stats_out[b] = {mean, rstd}; if y != NULL:
 *     y = act( gn(x)*gamma + beta + res ) + emb[b,c]
 *   res  (B,C,H,W) or NULL : residual of DoubleConv (ddpm_utils.py:93);
 *   act  0 = identity, 1 = exact GELU (nn.GELU, :86 / F.gelu, :93);
 *   emb  (B,C) or NULL     : time-embedding add of Down/Up (:218-219, :244-245).
 * bwd: given dy (= dL/dy) recomputes the chain; writes dx, dres (may be NULL), and per-sample
 *   partials laid out (B, 2, C): [b][0][c] = sum dz*xhat (-> dgamma), [b][1][c] = sum dz (-> dbeta), which
 *   the kernel's tail reduces over b into dgamma / dbeta (both NULL: the caller reduces the partials itself, e.g. with
 *   afd_colsum; accumulate = 1 adds into them, as autograd's .grad accumulation would).  The partial buffer holds
 *   B*C*2 floats.  demb = sum_hw dy is (B,C). */
int afd_groupnorm1_fwd(const float* x, float* y, float* stats_out, int B, int C, int HW, float eps,
                       const float* gamma, const float* beta, const float* res, int act, const float* emb,
                       afd_stream_t stream);
/* test hook: 0 = the sample-resident backward (one launch, x / dy read once) wherever the sample fits the registers
 * (C*HW <= 32768, HW/4 a power of two: default), 1 = always the plane pass + apply pass of round 1 */
int afd_debug_norm_path(int mode);
int afd_groupnorm1_bwd(const float* x, const float* dy, const float* stats, int B, int C, int HW,
                       const float* gamma, const float* beta, const float* res, int act,
                       float* dx, float* dres, float* dgamma_dbeta_partial /* B*C*2 floats, (B,2,C) */, float* demb /* (B,C) or NULL */,
                       int have_partials /* 1: the partials were already produced by afd_filt_act_bwd */,
                       float* dgamma /* (C) or NULL */, float* dbeta /* (C) or NULL */, int accumulate, afd_stream_t stream);
/* out[j] (+)= sum_i in[i*cols + j], i < rows (deterministic tree; accumulate != 0 adds into out) */
int afd_colsum(const float* in, float* out, int rows, int cols, int accumulate, afd_stream_t stream);
/* same with an explicit row stride (elements): sums a column block of a wider matrix */
int afd_colsum_strided(const float* in, long row_stride, float* out, int rows, int cols, int accumulate, afd_stream_t stream);
/* (rows,2,C) partials -> out_a[C] (+)= sum over rows of block 0, out_b[C] (+)= block 1, in one launch */
int afd_colsum2(const float* in, float* out_a, float* out_b, int rows, int C, int accumulate, afd_stream_t stream);

/* ---- F5/F10: convolution as implicit GEMM (3x3 pad 1, or 1x1) --------- ddpm_utils.py:84,87,112,115;
 *      nn.Linear / MHA projections on NCHW tokens (ddpm_utils.py:59-66,71,73); outc (ddpm_models.py:84)
 * x (B,Cin,H,W), w (Cout,Cin,k,k) k in {1,3}, y (B,Cout,H,W).
 * epilogue: y = act(conv + bias[co]) + res      (bias/res may be NULL; act 0 none, 1 exact GELU)
 * dgrad:   dx = conv_transpose(dy, w)           wgrad: dw = sum_b,hw dy (x) x ; dbias = sum dy
 * wgrad needs a workspace (split-K partial slabs + the (B,Cout) dbias partials); size from
 * afd_conv_wgrad_workspace_bytes. */
/* test hook: 0 = choose the tile by workgroup count (default), 1 = always the 64x128 tile,
 * 2 = always the 32x64 in-workgroup split-K tile (when the shape allows it);
 * 8 / 9 / 10 = 1x1 streaming kernel chosen by the measured rule (default) / never / whenever the shape is covered;
 * 32 / 33 / 34 = wgrad workgroups of 4 waves / 8 waves / chosen per layer (default);
 * 96 / 97 / 98 = Winograd form of the 3x3 wgrad chosen by rule (default) / never / whenever the shape is covered;
 * 84 / 85 / 86 = bf16x3 form of the 3x3 wgrad (csrc/bf3_wgrad.hip) by rule (default) / never / whenever the shape is covered
 *                (85 also switches the 1x1 form off); 88 / 89 = bf16x3 form of the 1x1 wgrad by rule (default) / never;
 * 80 / 81 / 82 = the DIRECT matrix-core form of the 3x3 forward / dgrad (see afd_conv3x3_weight_kinds below) by the measured
 *                rule (default) / never / wherever the shape is covered;
 * 74 / 75 = the f16x2 split-K kernel for the 4x4 maps and the thin 8x8 launches (csrc/h2.hip conv_h2_sk; also a direct form:
 *           afd_conv3x3_weight_kinds reports it) by rule (default) / never (round 1's fp32 Winograd split-K kernel instead);
 *           73 = wherever the shape is covered, ahead of the tile kernel (tests);
 * 48 / 49 = workgroups per launch of the matrix-core 3x3 weight gradient: one per CU (256: fastest alone, default) / 160 (fastest
 *           beside the dependent chain on another stream: -1 % on the train step; training.TrainStep asks for it);
 * 50 / 51 / 52 = waves per workgroup of the f16x2 3x3 weight gradient (csrc/h2_wgrad.hip): by the measured rule (default) /
 *           eight everywhere (one workgroup holds a CU) / four wherever covered (two workgroups per CU, or one beside a
 *           workgroup of the dependent chain; a 64 x 64 block becomes two 64 x 32 workgroups and half the splits) (tests);
 *           53 / 54 / 55 = four waves on blocks of 64 x 32 / 32 x 64 / 32 x 32 (output x input channels) wherever the channel
 *           counts allow (tests);
 * 60 / 61 = the f16x2 tile kernel's operand feed: by rule (default: both operands from LDS, the weights by LDS-DMA, where a
 *           workgroup holds one block of 32 output channels on the 32 x 32 maps; the weights straight from L2 into registers
 *           elsewhere) / always the register-fed kernel;  62 / 63 / 59 = the LDS-fed kernel wherever the shape is covered,
 *           trying its (128 pixels x 64 channels) / (256 x 32) / (128 x 32) workgroup first (tests);
 * 76 / 77 = arithmetic of that direct form: two fp16 pieces under an online power-of-two scale (csrc/h2.hip, default) /
 *           three bf16 pieces (round 2, csrc/bf3.hip);  78 / 79 = the same choice for the matrix-core 3x3 weight gradient
 *           (csrc/h2_wgrad.hip / csrc/bf3_wgrad.hip);
 * 92 / 93 = streaming vector kernels for the 1x1 output layer (<= 4 output channels) and its dgrad (csrc/ends.hip) by rule
 *           (default) / never;
 * 64 ... 70 = the Winograd form of the 3x3 forward / dgrad, 71 / 72 = the slice-walking form of the f16x2 split-K kernel (both
 *           described at afd_conv3x3_wino_workspace_bytes below); 100000 + g (g < 100000) = persistent Winograd grid of g
 *           workgroups (0 = one item per workgroup, default).
 * Every other integer is refused with AFD_EINVAL and changes nothing.  The defaults are 0, 8, 34, 48, 50, 60, 64, 74, 76, 78, 80,
 * 84, 88, 92, 96 and 100000. */
int afd_debug_conv_path(int mode);
/* the switches afd_debug_conv_path sets, read back (nothing is launched): copies them, in the member order of ConvSwitches
 * (csrc/conv_forms.h), into values[0..min(n, count)) and returns count. */
int afd_debug_conv_state(long* values, int n);
int afd_conv_fwd(const float* x, const float* w, const float* bias, const float* res, float* y,
                 int B, int Cin, int Cout, int H, int W, int ksize, int act, afd_stream_t stream);
int afd_conv_dgrad(const float* dy, const float* w, float* dx,
                   int B, int Cin, int Cout, int H, int W, int ksize, afd_stream_t stream);
size_t afd_conv_wgrad_workspace_bytes(int B, int Cin, int Cout, int H, int W, int ksize);
/* which kernel afd_conv_wgrad (dbias == NULL) runs for the shape: 0 = direct implicit GEMM on the fp32 MFMA,
 * 1 = Winograd F(3x3,2x2) on the fp32 MFMA, 2 = pixel-reduction GEMM on the bf16 MFMA with exact three-piece splits
 * (fp32 accuracy), 3 = the first layer's vector-FMA form (3 input channels: memory-bound), 4 = the pixel-reduction GEMM on
 * the fp16 MFMA with two-piece splits under online power-of-two scales (fp32-class accuracy, half the products of 2; the
 * default since round 3).  For reporting (bench.py prices each launch against the peak of the instruction it issues).
 * The answer goes by the shape alone.  Two things send a call to form 0 whatever it says: a 3x3 call WITH dbias (forms 1-4
 * have no bias row), and an x or dy that is not 16-byte aligned (forms 1, 2 and 4 stage both with 16-byte loads).
 *
 * Alignment and accumulate (every wgrad entry point): x, dy and the workspace are fp32 tensors at any 4-byte offset, the
 * fast forms want x and dy 16-byte aligned and fall back otherwise.  dw and dbias may sit at ANY 4-byte offset (a training
 * step hands in views of one flat gradient buffer with no padding between tensors): every form writes its slabs to the
 * workspace, and the one access to dw / dbias is the scalar read-add-write of the final fold.  accumulate = 1: dw[i] =
 * dw[i] + t[i], ONE fp32 add of the finished sum t onto what dw held -- bit for bit what `dw_old + afd_conv_wgrad(...,
 * accumulate = 0)` gives.  That add is not atomic: two calls that accumulate into one dw (a parameter used twice in one
 * backward) must be ordered on one stream, and two fold descriptors with one dst must not share an afd_fold_batched call
 * (ops.deal_lane / ops.fold_batches see to both). */
int afd_conv_wgrad_form(int B, int Cin, int Cout, int H, int W, int ksize);
/* the plan of the matrix-core 3x3 weight gradient (forms 2 and 4) for the shape under the current afd_debug_conv_path
 * settings, as afd_conv_wgrad_workspace_bytes sizes it and afd_conv_wgrad launches it: returns the number of slabs (= splits
 * over the pixel tiles; 0 = the shape does not take these forms) and fills info[0..4] = tiles per split, tiles, output
 * channels per workgroup, input channels per workgroup, waves per workgroup (8: one workgroup per CU; 4: two).  Nothing is
 * launched. */
int afd_conv_wgrad3_plan(int B, int Cin, int Cout, int H, int W, int* info);
int afd_conv_wgrad(const float* x, const float* dy, float* dw, float* dbias /* or NULL */,
                   int B, int Cin, int Cout, int H, int W, int ksize, int accumulate,
                   void* workspace, afd_stream_t stream);

/* ---- the deterministic tail of every parameter gradient, batched (csrc/fold.hip) ----------------------------------
 *      backward of nn.Conv2d / nn.Linear / nn.GroupNorm / nn.LayerNorm parameters: ddpm_utils.py:59-66,84-88,112-118
 * A fold: dst[(j % inner) * rstride + j / inner] (+)= sum_{s < splits} part[s * stride + j], j < n, fixed order, no
 * atomics (identity map: inner = n, rstride = 1; [tap][plane] slabs -> OIHW: inner = n / 9, rstride = 9).
 * afd_fold_batched folds any number of them in ceil(n / 56) launches (descs: HOST array; the descriptors travel as
 * kernel arguments, so the call is legal under stream capture and needs no device table).  The result of a fold does
 * not depend on what it is batched with -- PROVIDED no two descriptors of a call share a dst: a fold reads dst, adds and
 * writes back without atomics, one workgroup per 32 or 128 elements, so two folds into one dst in one launch race.  dst may
 * sit at any 4-byte offset (scalar accesses); part is read with 16-byte loads where n % 128 == 0, inner % 4 == 0,
 * stride % 4 == 0 and part is 16-byte aligned, with scalar loads otherwise (the launcher tests all four).
 * afd_conv_wgrad_partials = afd_conv_wgrad without its final fold: launches the slab producer and writes the fold
 * descriptor(s) (weights, then bias) to folds_out[0..*n_folds) (HOST, room for 2) for a later afd_fold_batched ON THE
 * SAME STREAM; the workspace must stay alive until that fold has run.  Shapes whose kernel has no slab stage are
 * completed at once and report *n_folds = 0. */
typedef struct afd_fold_desc {
  const float* part;     /* partial slabs */
  float* dst;
  long n;                /* elements per slab */
  long stride;           /* elements between consecutive slabs (>= n) */
  long inner, rstride;   /* element map, see above */
  int splits;            /* number of slabs */
  int accumulate;        /* != 0: add into dst */
} afd_fold_desc;         /* 56 bytes */
int afd_fold_batched(const afd_fold_desc* descs, int n, afd_stream_t stream);
int afd_conv_wgrad_partials(const float* x, const float* dy, float* dw, float* dbias /* or NULL */,
                            int B, int Cin, int Cout, int H, int W, int ksize, int accumulate,
                            void* workspace, afd_fold_desc* folds_out, int* n_folds, afd_stream_t stream);

/* Winograd F(2x2,3x3) form of the 3x3 forward / dgrad (same results up to fp32 re-association: every product
 * and sum is fp32; 16 multiplies per 2x2 output tile and channel pair instead of 36).  Covers the square
 * 64x64 ... 4x4 maps with Cin % 8 == 0 and Cout % 32 == 0 (dgrad: roles swapped).
 * afd_conv3x3_wino_workspace_bytes returns 0 when the layer is not covered (or too small to gain): the caller
 * then uses afd_conv_fwd / afd_conv_dgrad.  The workspace holds the transformed weights (16*Cin*Cout floats; the
 * forward and the dgrad forms differ); weights_ready != 0 says it still holds them from an earlier call with the
 * same w and the same pass, so the transform launch is skipped (sampling: w is constant over the 999 steps).
 * afd_debug_conv_path: 64 / 65 = Winograd chosen by the measured rule (default) / never; 66..69 = whenever covered,
 * with workgroups of 64x64 / 32x64 / 64x32 / 32x32 (output channels x tiles); 70 = the small-map (4x4, 8x8)
 * in-workgroup split-K kernel wherever it is covered.
 * 74 / 75 / 73 = the f16x2 split-K kernel of the 4x4 and thin 8x8 maps (conv_h2_sk) by rule (default) / never / wherever the
 * shape is covered.  71 / 72 = its slice-walking form on the 4x4 maps (conv_h2_skw: a wave keeps the weight fragments of a tap
 * for 1, 2 or 4 consecutive 32-pixel slices; the same bits as conv_h2_sk): 71 = wherever the split-K kernel runs, with two or
 * four slices per wave (tests, small shapes), 72 = never (conv_h2_sk everywhere: the A/B baseline); by default the measured rule
 * chooses (K >= 128 and at least two workgroups per CU), and 74 returns 71 / 72 to it.  A failed opt-in to the form's dynamic LDS
 * (up to 160 KB) makes afd_conv3x3_wino_fwd / _dgrad return AFD_ELAUNCH with nothing launched. */
size_t afd_conv3x3_wino_workspace_bytes(int B, int Cin, int Cout, int H, int W, int dgrad);
/* the transformed weights of both passes (either pointer may be NULL) in ONE launch: the dgrad image is the forward
 * image with permuted transform indices.  Buffers of 16*Cin*Cout floats each; afterwards call the entry points below
 * with weights_ready = 1. */
int afd_conv3x3_wino_weights(const float* w, float* u_fwd, float* u_dgrad, int Cin, int Cout, int kinds, afd_stream_t stream);
/* Some layers run a DIRECT form on the bf16 matrix cores at fp32 accuracy instead (csrc/bf3.hip: every operand split
 * exactly into three bf16 pieces, six cross terms per product; chosen by the library per pass from the shape): their
 * workspace holds the split weights (54 bytes per (cin, cout) pair -- the same buffer size serves both forms).
 * kinds: bit 0 / bit 1 set = the forward / the dgrad image of this layer is the DIRECT form's (records of 8 matrix-core
 * inputs per (piece, tap, channel group, output row)) instead of the Winograd one; bit 2 (only with bit 0 or 1) = that direct
 * image holds three bf16 pieces (round 2's arithmetic, afd_debug_conv_path 77) instead of two fp16 pieces + one scale per
 * output row.  The value depends on B (the rule wants >= 2 workgroups per CU) and on afd_debug_conv_path: pass what this
 * function returned WHEN THE IMAGE WAS BUILT to the two weight entry points (afd_wino_desc.kinds for the batched one) and to
 * afd_conv3x3_wino_fwd / _dgrad.  afd_debug_conv_path 80 / 81 / 82 = the direct form by the measured rule (default) / never /
 * wherever the shape is covered. */
int afd_conv3x3_weight_kinds(int B, int Cin, int Cout, int H, int W);
/* ... and of EVERY layer of a model in one launch (a train step transforms ~30 weight tensors; one launch instead of
 * 30 takes them off the critical path).  descs (DEVICE array): one entry per layer; wg_desc (DEVICE, n_wg ints): the
 * layer each 256-thread workgroup works on -- layer i owns workgroups [first_wg, first_wg + ceil(Cin*Cout/256)). */
typedef struct afd_wino_desc {
  const float* w;        /* (Cout,Cin,3,3) */
  float* u_fwd;          /* 16*Cin*Cout floats or NULL */
  float* u_dgrad;        /* 16*Cin*Cout floats or NULL */
  int Cin, Cout, first_wg, kinds;   /* kinds: afd_conv3x3_weight_kinds of the layer */
} afd_wino_desc;
int afd_conv3x3_wino_weights_batched(const afd_wino_desc* descs, const int* wg_desc, int n_wg, afd_stream_t stream);
/* weights_ready != 0: the workspace already holds the image, built for `kinds` (what afd_conv3x3_weight_kinds returned when
 * it was built); the call fails with AFD_EINVAL if that is not the form it is about to read (the choice between the forms
 * depends on the batch size -- e.g. a last partial batch -- and on afd_debug_conv_path).  weights_ready == 0: the image is
 * built first, in the form this call reads; `kinds` is ignored. */
int afd_conv3x3_wino_fwd(const float* x, const float* w, const float* bias, const float* res, float* y,
                         int B, int Cin, int Cout, int H, int W, int act, void* workspace, int weights_ready, int kinds,
                         afd_stream_t stream);
int afd_conv3x3_wino_dgrad(const float* dy, const float* w, float* dx, const float* add_to_dx /* or NULL: dx = dgrad + add,
                           the gradient that reaches x through the block's residual branch */,
                           int B, int Cin, int Cout, int H, int W, void* workspace, int weights_ready, int kinds,
                           afd_stream_t stream);

/* ---- F10: LayerNorm over channels of an NCHW tensor (= nn.LayerNorm([C]) on (B,L,C) tokens) ------
 * ddpm_utils.py:60,62,70.  stats_out (B,HW,2) = {mean, rstd}. */
int afd_layernorm_c_fwd(const float* x, float* y, float* stats_out, int B, int C, int HW, float eps,
                        const float* gamma, const float* beta, afd_stream_t stream);
int afd_layernorm_c_bwd(const float* x, const float* dy, const float* stats, int B, int C, int HW,
                        const float* gamma, float* dx, const float* add_to_dx /* or NULL: dx = LN'(dy) + add (the gradient
                        that reaches x through the block's residual branch: one pass instead of an extra add) */,
                        float* dgamma_dbeta_partial /* (B,2,C) */,
                        float* dgamma /* (C) or NULL */, float* dbeta /* (C) or NULL */, int accumulate,
                        afd_stream_t stream);
/* the two halves separately: afd_layernorm_c_bwd with dgamma_dbeta_partial = dgamma = dbeta = NULL writes dx only (the
 * critical path of backward); this one computes only the parameter gradients (nothing downstream waits for them, so
 * the host may issue it on another stream) */
int afd_layernorm_c_bwd_params(const float* x, const float* dy, const float* stats, int B, int C, int HW,
                               float* dgamma_dbeta_partial /* (B,2,C) */, float* dgamma, float* dbeta, int accumulate,
                               afd_stream_t stream);
/* the plane pass of afd_layernorm_c_bwd_params alone: part (B,2,C) = per-sample sums over the pixels of dy*xhat and dy;
 * the caller folds them (afd_fold_batched: two descriptors, n = C, stride = 2C, splits = B) */
int afd_layernorm_c_bwd_partials(const float* x, const float* dy, const float* stats, int B, int C, int HW, float* part,
                                 afd_stream_t stream);

/* ---- F10: multi-head self-attention core (softmax(QK^T/sqrt(d))V), flash-style ------------------
 * ddpm_utils.py:71 (nn.MultiheadAttention, batch_first, 4 heads).  qkv (B,3C,L): channel
 * n = {0:q,1:k,2:v}*C + head*d + j, token index contiguous (the NCHW image of in_proj's output).
 * o (B,C,L); lse (B,heads,L) saved for backward.  Never materialises the L x L scores. */
/* tuning hook: force R rows per lane (1, 2, 4) of the all-vector kernels for head dim 8; 0 = default;
 * 10 / 11 = the MFMA two-pass backward for head dim 8 only below L = 1024 / at every L (default);
 * 20 / 21 = head dim 8, L % 256 == 0: the rank-8 products on the vector pipe (two-pass backward) / on the fp16 matrix pipe with
 * the one-pass backward (default);
 * 30 / 31 = head dim 16 / 32 at L in {16,32,48,64}: the all-vector kernels / the one-wave-per-head fp32 matrix-pipe kernels (default);
 * 40 / 41 = head dim 16, L % 256 == 0: the same choice as 20 / 21 (41, the fp16 matrix pipe and the one-pass backward, is the default) */
int afd_debug_attn_rows(int rows);
int afd_attn_fwd(const float* qkv, float* o, float* lse, int B, int heads, int d, int L, afd_stream_t stream);
int afd_attn_bwd(const float* qkv, const float* o, const float* d_o, const float* lse, float* dqkv,
                 float* delta_workspace /* (B,heads,L) floats */, int B, int heads, int d, int L, afd_stream_t stream);

/* ---- F10: the token-wise chains of SelfAttention fused around the core ------------------- ddpm_utils.py:68-74
 * Tokens are the pixels of the NCHW tensor (P = H*W per image), every nn.Linear is a 1x1 convolution with its (out,in)
 * weight, so the block is   x -> [head] -> qkv -> afd_attn_fwd -> att -> [tail] -> out   with
 *   head: h = LayerNorm(x; gamma, beta) (:70);  qkv = w_in h + b_in  (the MHA in-projection, :71);
 *   tail: a = w_o att + b_o + x (:71-72);  f = LayerNorm(a) ;  u = w_1 f + b_1;  g = GELU(u);  out = w_2 g + b_2 + a  (:73).
 * Covered: C in {32, 64, 128} (afd_tok_supported); other widths use the unfused entry points above.
 * head_fwd: h_out / stats_out (B,P,2 = {mean, rstd}) may be NULL (inference).
 * tail_fwd: a_out, stats_out, f_out, u_out, g_out are the tensors backward needs -- all five or none (NULL = inference).
 * tail_bwd: du = (w_2^T d_out) * GELU'(u);  df = w_1^T du;  d_a = LayerNorm'(df; a) + d_out;  d_att = w_o^T d_a.
 *           du / df / d_a are also what the weight-gradient kernels and afd_layernorm_c_bwd_params consume
 *           (dW_2 from (g, d_out), dW_1 from (f, du), dW_o from (att, d_a), LayerNorm parameters from (a, df)).
 * head_bwd: dh = w_in^T dqkv;  dx = LayerNorm'(dh; x) + d_res   (d_res = d_a of the tail: the residual branch);
 *           dh_out (or NULL) for the LayerNorm parameter gradients. */
int afd_tok_supported(int C);
/* test hook: cap the workgroups per launch of the four kernels below (forces several passes per workgroup); 0 = default */
int afd_debug_tok_grid(int max_workgroups);
/* test hook: 0 = kernel form by the rule, 1 = never the wide (one wave per 32-channel block) forms, 2 = wide wherever they exist
 * (1 and 2: fp32 forms only);
 * 3 = the fp32 forms by their own rule, never the f16x2 forms (csrc/tok_h2.hip: C in {64, 128}, every product as two fp16
 *     pieces on the fp16 matrix pipe);  4 = the f16x2 forms wherever they exist;
 * 5 / 6 = as 4, with 2 / 4 waves (= pixel tiles) per workgroup at C = 64 (tuning) */
int afd_debug_tok_path(int mode);
int afd_tok_head_fwd(const float* x, const float* gamma, const float* beta, const float* w_in, const float* b_in,
                     float* h_out, float* stats_out, float* qkv, int B, int C, int P, float eps, afd_stream_t stream);
int afd_tok_tail_fwd(const float* att, const float* x, const float* w_o, const float* b_o, const float* gamma, const float* beta,
                     const float* w_1, const float* b_1, const float* w_2, const float* b_2,
                     float* a_out, float* stats_out, float* f_out, float* u_out, float* g_out, float* out,
                     int B, int C, int P, float eps, afd_stream_t stream);
int afd_tok_tail_bwd(const float* d_out, const float* u, const float* a, const float* stats, const float* gamma,
                     const float* w_2, const float* w_1, const float* w_o,
                     float* du_out, float* df_out, float* da_out, float* datt_out, int B, int C, int P, afd_stream_t stream);
int afd_tok_head_bwd(const float* dqkv, const float* x, const float* stats, const float* gamma, const float* w_in,
                     const float* d_res, float* dh_out, float* dx_out, int B, int C, int P, afd_stream_t stream);

/* ---- elementwise / pooling used by variants 0 and 2 --------------------------------------------
 * gelu: nn.GELU (ddpm_utils.py:64); maxpool: nn.MaxPool2d(2) (:203,258);
 * bilinear: nn.Upsample(scale_factor=2, 'bilinear', align_corners=True) (:226,280). */
int afd_gelu_fwd(const float* x, float* y, long n, afd_stream_t stream);
int afd_gelu_bwd(const float* x, const float* dy, float* dx, long n, afd_stream_t stream);
int afd_maxpool2_fwd(const float* x, float* y, int B, int C, int H, int W, afd_stream_t stream);
int afd_maxpool2_bwd(const float* x, const float* dy, float* dx, int B, int C, int H, int W, afd_stream_t stream);
int afd_bilinear_up2_fwd(const float* x, float* y, int B, int C, int H, int W, long y_bstride, afd_stream_t stream);
int afd_bilinear_up2_bwd(const float* dy, float* dx, int B, int C, int H, int W, long dy_bstride, afd_stream_t stream);
/* strided batch copy: dst[b, 0:n] = src[b, 0:n] (torch.cat of the skip, ddpm_utils.py:242) */
int afd_copy_batched(const float* src, float* dst, int B, long n, long src_bstride, long dst_bstride, afd_stream_t stream);
/* y = a + b (gradient accumulation of skip connections) */
int afd_add(const float* a, const float* b, float* y, long n, afd_stream_t stream);

/* ---- F9: time embedding ------------------------------------- ddpm_models.py:261-269,272-273
 * temb[b, k] = sin(t[b]*inv_freq[k]), temb[b, half+k] = cos(...); t int64, inv_freq (half,) fp32
 * (computed once on the host exactly as the reference does).
 * silu_linear: out[b, n] = sum_k silu(temb[b,k]) * w[n,k] + bias[n]      ddpm_utils.py:208-214
 * bias / dbias may be NULL.  bwd, accumulate = 1: dw[n,k] = dw[n,k] + t and dbias[n] = dbias[n] + t, one fp32 add of the
 * finished batch sum t each (= old + what accumulate = 0 writes), not atomic: calls that accumulate into one dw run in
 * order on one stream.  Every pointer may sit at any 4-byte offset (scalar accesses only); afd_embed_add_bwd likewise. */
int afd_pos_encoding(const int64_t* t, const float* inv_freq, float* temb, int B, int half, afd_stream_t stream);
int afd_silu_linear_fwd(const float* temb, const float* w, const float* bias, float* out,
                        int B, int K, int N, afd_stream_t stream);
int afd_silu_linear_bwd(const float* temb, const float* w, const float* dout, float* dw, float* dbias,
                        float* dtemb /* or NULL; accumulated into */, int B, int K, int N, int accumulate, afd_stream_t stream);
/* the forward of up to 8 such layers that share temb in ONE launch (the six stages' emb_layer of a UNet forward: their
 * input exists as soon as the forward starts).  descs: HOST array of n entries. */
typedef struct afd_silu_desc {
  const float* w;        /* (N, K) */
  const float* bias;     /* (N) or NULL */
  float* out;            /* (B, N) */
  int N;
} afd_silu_desc;
int afd_silu_linear_fwd_batched(const float* temb, const afd_silu_desc* descs, int n, int B, int K, afd_stream_t stream);
/* out_i[b][:] = table_i[idx[b]][:] (idx clamped to [0, rows)) for up to 8 tables (descs[i].w = table_i (rows, N_i),
 * descs[i].out = (B, N_i), bias unused) in one launch.  Sampling: emb_layer(pos_encoding(t)) depends on the integer t only,
 * so the host package tabulates it for every timestep once per trajectory (with the two entry points above) and a denoise
 * step gathers its rows -- bit-identical to computing them (ddpm_models.py:261-269, ddpm_utils.py:208-214). */
int afd_gather_rows_batched(const int64_t* idx, const afd_silu_desc* descs, int n, int B, int rows, afd_stream_t stream);

/* label conditioning: out[b, :] = temb[b, :] + table[y[b], :]   (nn.Embedding lookup + add, ddpm_models.py:254,276-277)
 * y: (B,) int64 class indices in [0, num_classes); out may alias temb.
 * bwd: dtable[k, :] (+)= sum over {b : y[b] == k} of dout[b, :], rows summed in batch order (deterministic, no atomics);
 * rows of classes absent from y are zeroed (accumulate = 0) or left alone (accumulate = 1). */
int afd_embed_add_fwd(const float* temb, const float* table, const int64_t* y, float* out, int B, int D, int num_classes,
                      afd_stream_t stream);
/* the same with the NULL label (classifier-free guidance): a row with y[b] < 0 carries no label and out[b, :] is a bit copy of
 * temb[b, :]; every row with y[b] >= 0 is bit-identical to afd_embed_add_fwd (labels >= num_classes clamp the same way).
 * afd_embed_add_fwd itself clamps a negative label to class 0.  out may alias temb.
 * afd_embed_add_bwd below needs no null-label form: y[b] == k never holds for k >= 0 when y[b] < 0, so a null row adds
 * nothing to any row of dtable (and a class that only appears as a null label gets a zero row). */
int afd_label_embed_add_fwd(const float* temb, const float* table, const int64_t* y, float* out, int B, int D, int num_classes,
                            afd_stream_t stream);
int afd_embed_add_bwd(const float* dout, const int64_t* y, float* dtable, int B, int D, int num_classes, int accumulate,
                      afd_stream_t stream);

/* ---- F14/F16: DDPM noise / denoise / quantise ------------------ ddpm_models.py:317-321, 367-374, 381-385
 * Bit-exact restatements of the reference's fp32 expression order (no FMA contraction).
 * t: (B,) int64 indices into the (T,) schedule tables. */
int afd_noise_images(const float* x, const float* eps, const int64_t* t, const float* alpha_hat,
                     float* x_t, int B, long per_sample, afd_stream_t stream);
int afd_denoise_step(const float* x, const float* eps_pred, const float* noise /* NULL => zeros (i == 1) */,
                     const float* alpha, const float* alpha_hat, const float* beta, int i,
                     float* x_out, long n, afd_stream_t stream);
/* same update with the step index read from device memory (t_dev[0]): the form a captured hipGraph replays */
int afd_denoise_step_dev(const float* x, const float* eps_pred, const float* noise,
                         const float* alpha, const float* alpha_hat, const float* beta, const int64_t* t_dev,
                         float* x_out, long n, afd_stream_t stream);
/* classifier-free guidance: the guided noise and the denoise update in one pass.  eps2: the (2n)-element output of ONE forward
 * over [conditional rows ; unconditional rows] (element j at j and n + j).  e = torch.lerp(e_u, e_c, cfg_scale) with ATen's
 * scalar formula, one rounding per operation (|s| < 0.5: u + s (c - u); otherwise c - (c - u)(1 - s)), then exactly the
 * afd_denoise_step expression.  x_out may alias x; x_out2 is NULL or a second destination of the same n values (the other
 * half of the sampler's 2n input buffer).  n: elements of x (n images times the per-image size). */
int afd_denoise_step_cfg(const float* x, const float* eps2, const float* noise /* NULL => zeros (i == 1) */,
                         const float* alpha, const float* alpha_hat, const float* beta, int i, float cfg_scale,
                         float* x_out, float* x_out2, long n, afd_stream_t stream);
/* same with the step index read from t_dev[0] (graph-replayable) */
int afd_denoise_step_cfg_dev(const float* x, const float* eps2, const float* noise,
                             const float* alpha, const float* alpha_hat, const float* beta, const int64_t* t_dev, float cfg_scale,
                             float* x_out, float* x_out2, long n, afd_stream_t stream);
/* DDIM (Song et al. 2021): one step t -> t_prev of a strided chain, for a model trained on the eps-objective.
 * a_t = alpha_hat[t], a_p = alpha_hat[t_prev].  fp32 with one IEEE rounding per operation (no FMA contraction, correctly
 * rounded / and sqrt), evaluated in exactly this order:
 *   x0  = (x - sqrt(1 - a_t) * eps) / sqrt(a_t)
 *   r   = (1 - a_p) / (1 - a_t)          q = 1 - a_t / a_p
 *   var = (eta * eta) * (r * q)          sigma = sqrt(var)          dir = sqrt(max((1 - a_p) - var, 0))
 *   out = ((sqrt(a_p) * x0) + (dir * eps)) + (noise ? sigma * noise : +0)
 * eta = 0: deterministic; eta = 1: ancestral.  noise is NULL for the last step of a chain (and for every step when eta = 0).
 * Requires 0 <= t_prev < t (host form), eta >= 0, n > 0.  x_out may alias x.  n: elements of x. */
int afd_ddim_step(const float* x, const float* eps, const float* noise /* NULL => none */, const float* alpha_hat, int t, int t_prev,
                  float eta, float* x_out, long n, afd_stream_t stream);
/* same with t = t_dev[0] and t_prev = t_prev_dev[0] read on the device (graph-replayable; the indices are not checked) */
int afd_ddim_step_dev(const float* x, const float* eps, const float* noise, const float* alpha_hat, const int64_t* t_dev,
                      const int64_t* t_prev_dev, float eta, float* x_out, long n, afd_stream_t stream);
/* classifier-free guided DDIM step: eps2 as for afd_denoise_step_cfg (conditional element j at j, unconditional at n + j),
 * eps = torch.lerp(e_u, e_c, cfg_scale) with the same scalar formula, then exactly the afd_ddim_step expression.  x_out may
 * alias x; x_out2 is NULL or a second destination of the same n values. */
int afd_ddim_step_cfg(const float* x, const float* eps2, const float* noise, const float* alpha_hat, int t, int t_prev, float eta,
                      float cfg_scale, float* x_out, float* x_out2, long n, afd_stream_t stream);
int afd_ddim_step_cfg_dev(const float* x, const float* eps2, const float* noise, const float* alpha_hat, const int64_t* t_dev,
                          const int64_t* t_prev_dev, float eta, float cfg_scale, float* x_out, float* x_out2, long n,
                          afd_stream_t stream);
/* The DDIM step with the noise scale read from a table (Analytic-DPM, Bao et al. 2022: Diffusion.sample_analytic): sig is a
 * (T,) fp32 device table indexed by t, and the step is afd_ddim_step's with sigma = sig[t] in place of sqrt(var):
 *   x0  = (x - sqrt(1 - a_t) * eps) / sqrt(a_t)
 *   r   = (1 - a_p) / (1 - a_t)          q = 1 - a_t / a_p
 *   var = (eta * eta) * (r * q)          sigma = sig[t]             dir = sqrt(max((1 - a_p) - var, 0))
 *   out = ((sqrt(a_p) * x0) + (dir * eps)) + (noise ? sigma * noise : +0)
 * so the mean is DDIM's at that eta, and the output is afd_ddim_step's bit for bit whenever sig[t] holds its fp32 sigma.
 * The same requirements and aliasing rules as afd_ddim_step[_cfg][_dev]; sig must not be NULL.  No masked form. */
int afd_ddim_step_var(const float* x, const float* eps, const float* noise /* NULL => none */, const float* alpha_hat,
                      const float* sig, int t, int t_prev, float eta, float* x_out, long n, afd_stream_t stream);
int afd_ddim_step_var_dev(const float* x, const float* eps, const float* noise, const float* alpha_hat, const float* sig,
                          const int64_t* t_dev, const int64_t* t_prev_dev, float eta, float* x_out, long n, afd_stream_t stream);
int afd_ddim_step_var_cfg(const float* x, const float* eps2, const float* noise, const float* alpha_hat, const float* sig, int t,
                          int t_prev, float eta, float cfg_scale, float* x_out, float* x_out2, long n, afd_stream_t stream);
int afd_ddim_step_var_cfg_dev(const float* x, const float* eps2, const float* noise, const float* alpha_hat, const float* sig,
                              const int64_t* t_dev, const int64_t* t_prev_dev, float eta, float cfg_scale, float* x_out,
                              float* x_out2, long n, afd_stream_t stream);
/* The ascending DDIM step (DDIM inversion): one move s -> u of a chain walked upwards, 0 <= s < u; level 0 is the image, read
 * as alpha_hat[0] exactly as afd_ddim_step's last step t_prev = 0 reads it.  a_s = alpha_hat[s], a_u = alpha_hat[u].  fp32 with
 * one IEEE rounding per operation (no FMA contraction, correctly rounded / and sqrt), evaluated in exactly this order:
 *   x0  = (x - sqrt(1 - a_s) * eps) / sqrt(a_s)
 *   out = (sqrt(a_u) * x0) + (sqrt(1 - a_u) * eps)
 * the algebraic inverse of afd_ddim_step's eta = 0 step u -> s for the eps that step used.  No noise, no masked form.
 * Requires 0 <= s < u (host forms; u is not checked against the table's length) and n > 0.  x_out is normally apart from x (a
 * fixed-point refinement re-reads the base state) and may be x itself; x_out and x_out2 must not overlap eps.  n: elements of x. */
int afd_ddim_invert_step(const float* x, const float* eps, const float* alpha_hat, int s, int u, float* x_out, long n,
                         afd_stream_t stream);
/* same with s = s_dev[0] and u = u_dev[0] read on the device (graph-replayable; the indices are not checked) */
int afd_ddim_invert_step_dev(const float* x, const float* eps, const float* alpha_hat, const int64_t* s_dev, const int64_t* u_dev,
                             float* x_out, long n, afd_stream_t stream);
/* classifier-free guided form: eps2 as for afd_ddim_step_cfg (conditional element j at j, unconditional at n + j),
 * eps = torch.lerp(e_u, e_c, cfg_scale) with the same scalar formula, then exactly the afd_ddim_invert_step expression.
 * x_out2 is NULL or a second destination of the same n values; neither output may overlap any of eps2's 2n values. */
int afd_ddim_invert_step_cfg(const float* x, const float* eps2, const float* alpha_hat, int s, int u, float cfg_scale, float* x_out,
                             float* x_out2, long n, afd_stream_t stream);
int afd_ddim_invert_step_cfg_dev(const float* x, const float* eps2, const float* alpha_hat, const int64_t* s_dev,
                                 const int64_t* u_dev, float cfg_scale, float* x_out, float* x_out2, long n, afd_stream_t stream);
/* DPM-Solver++(2M) (Lu et al. 2022): one multistep update t -> t_prev of the probability-flow ODE, for a model trained on the
 * eps-objective.  coef: 5 fp32 values in device memory, [alpha_t, sigma_t, A, B0, B1] of this step (Diffusion.dpmpp_coefficients
 * builds the table on the host).  fp32 with one IEEE rounding per operation (no FMA contraction, correctly rounded /), in
 * exactly this order:
 *   x0     = (x - (sigma_t * eps)) / alpha_t
 *   out    = ((A * x) + (B0 * x0)) + (x0_prev ? B1 * x0_prev : +0)
 *   x0_out = x0                     (the next step's x0_prev)
 * x0_prev is NULL on a first-order step.  Because coef is read on the device, the same call serves graph replay.  x_out may
 * alias x; x0_out may be x0_prev itself (in-place state) and must not overlap x, eps, x_out or any other part of x0_prev.
 * Requires n > 0.  n: elements of x. */
int afd_dpmpp_step(const float* x, const float* eps, const float* x0_prev /* NULL => +0 */, const float* coef, float* x_out,
                   float* x0_out, long n, afd_stream_t stream);
/* classifier-free guided form: eps2 as for afd_denoise_step_cfg, eps = torch.lerp(e_u, e_c, cfg_scale) with the same scalar
 * formula, then exactly the afd_dpmpp_step expression.  x_out2 is NULL or a second destination of out; x0_out must not overlap
 * it either (nor any of eps2's 2n values). */
int afd_dpmpp_step_cfg(const float* x, const float* eps2, const float* x0_prev, const float* coef, float cfg_scale, float* x_out,
                       float* x_out2, float* x0_out, long n, afd_stream_t stream);
/* UniPC (Zhao et al. 2023; multistep, data prediction, B(h) = expm1(-h)), orders 1-3: at one evaluation of the network, the
 * corrector of the move that led here and the predictor of the next move, for a model trained on the eps-objective.  coef: 12 fp32
 * values in device memory, one row of Diffusion.unipc_coefficients, [alpha, sigma, Ac, c0, c1, c2, c3, Ap, p0, p1, p2, slot].
 * fp32 with one IEEE rounding per operation (no FMA contraction, correctly rounded /), in exactly this order:
 *   m  = (x - (sigma * eps)) / alpha
 *   xc = ((((Ac * xc) + (c0 * m)) + (c1 * h1)) + (c2 * h2)) + (c3 * h3)      (in place)
 *   xn = (((Ap * xc) + (p0 * m)) + (p1 * h1)) + (p2 * h2)                    (x_out; the xc of the line above)
 * hist holds three planes of n values, a ring: h_j is plane (slot - j) mod 3, and m is written to plane slot (h3's: each element
 * reads its h3 first).  slot is coef[11], read on the device and clamped into {0, 1, 2}.  Every term is evaluated on every call,
 * so hist must hold finite values (zeros before the first call) wherever the row's weights are 0.  Because coef is read on the
 * device, the same call serves graph replay.  x_out may alias x; xc and hist must not overlap each other, x, eps or x_out.
 * Requires n > 0.  n: elements of x. */
int afd_unipc_step(const float* x, const float* eps, float* xc, float* hist, const float* coef, float* x_out, long n,
                   afd_stream_t stream);
/* classifier-free guided form: eps2 as for afd_denoise_step_cfg, eps = torch.lerp(e_u, e_c, cfg_scale) with the same scalar
 * formula, then exactly the afd_unipc_step expression.  x_out2 is NULL or a second destination of xn; xc and hist must not
 * overlap it either (nor any of eps2's 2n values). */
int afd_unipc_step_cfg(const float* x, const float* eps2, float* xc, float* hist, const float* coef, float cfg_scale, float* x_out,
                       float* x_out2, long n, afd_stream_t stream);
/* ---- likelihood: the variational bound in bits/dim (Ho et al. 2020, section 3.3; Diffusion.calc_bpd) ----
 * A row r pairs image img[r] of x0 (n_img images of `per` fp32 values each) with timestep t[r].  img and t are int64 device
 * arrays of `rows` values, read on the device: the caller keeps them in [0, n_img) and [1, T) (nothing checks them here).
 * Outputs may overlap no input.  Every entry point needs its counts > 0.
 * Gathered noising: x_t[r] = afd_noise_images' expression on x0[img[r]], eps[r] and t[r], bit for bit. */
int afd_noise_images_gather(const float* x0, long n_img, const int64_t* img, const float* eps, const int64_t* t, const float* alpha_hat,
                            float* x_t, long rows, long per, afd_stream_t stream);
/* The bound's term of each row, one workgroup per row, in fp64.  coef: the (T, 4) fp64 device table of
 * Diffusion.vlb_coefficients, row t = [w_t, c_t, log_scale_t, prior constant].  With d_j = double(eps_hat_j) - double(eps_j):
 *   sq[r]   = sum_j d_j^2
 *   term[r] = w_t * sq[r] + per * c_t                                                         t != 1 (KL, nats)
 *           = -sum_j log P(x0_j | mean_j, log_scale_1)                                       t == 1 (decoder, nats)
 * mean_j = c1 * (x_t_j - c2 * eps_hat_j) in fp32, afd_denoise_step's expression at i = 1 without noise, and P the discretised
 * Gaussian of Ho et al. in fp64 (bins of half-width 1/255, open edge bins below -0.999 and above 0.999, Phi by the tanh
 * approximation, probabilities clamped at 1e-12).  Only decoder rows read x0 and x_t.  Deterministic: fixed per-thread order,
 * fixed wave tree, waves summed in order, no atomics.  alpha, alpha_hat, beta: the (T,) fp32 schedule tables. */
int afd_vlb_terms(const float* x0, long n_img, const int64_t* img, const float* x_t, const float* eps, const float* eps_hat,
                  const int64_t* t, const double* coef, long T, const float* alpha, const float* alpha_hat, const float* beta,
                  double* term, double* sq, long rows, long per, afd_stream_t stream);
/* The prior's data-dependent part: out[i] = half_ah * sum_j double(x0[i, j])^2, half_ah = alpha_hat[T-1] / 2 from the host */
int afd_vlb_prior(const float* x0, double half_ah, double* out, long n_img, long per, afd_stream_t stream);
/* ---- inpainting (RePaint, Lugmayr et al. 2022): masked steps and the renoise up-move ----
 * Each masked entry point is its unmasked counterpart above with two more operands after noise: x0 (n fp32 values, the known
 * image) and mask (n bytes; nonzero = known).  Per element j, with t_prev = i - 1 for the DDPM forms:
 *   gen   = the unmasked update, bit for bit (for the guided forms the lerp first, as above), except that its noise term is
 *           +0 when t_prev == 0 (DDPM: i == 1) and, for DDIM, when eta == 0
 *   known = x0                                               if t_prev == 0
 *           (sqrt(a_p) * x0) + (sqrt(1 - a_p) * noise)       otherwise, a_p = alpha_hat[t_prev] (afd_noise_images' order)
 *   out   = mask[j] ? known : gen                            (x_out2, when given, receives the same values)
 * noise is read once per element and serves whichever region the element is in; it may be NULL only when t_prev == 0 on the
 * host forms and never on the _dev forms.  x_out may alias x; x0 and mask must not overlap x_out or x_out2.  The host forms
 * need i >= 1 (DDPM) or 0 <= t_prev < t (DDIM); every form needs eta >= 0 and n > 0. */
int afd_denoise_step_masked(const float* x, const float* eps_pred, const float* noise, const float* x0, const uint8_t* mask,
                            const float* alpha, const float* alpha_hat, const float* beta, int i, float* x_out, long n,
                            afd_stream_t stream);
int afd_denoise_step_masked_dev(const float* x, const float* eps_pred, const float* noise, const float* x0, const uint8_t* mask,
                                const float* alpha, const float* alpha_hat, const float* beta, const int64_t* t_dev, float* x_out,
                                long n, afd_stream_t stream);
int afd_denoise_step_masked_cfg(const float* x, const float* eps2, const float* noise, const float* x0, const uint8_t* mask,
                                const float* alpha, const float* alpha_hat, const float* beta, int i, float cfg_scale, float* x_out,
                                float* x_out2, long n, afd_stream_t stream);
int afd_denoise_step_masked_cfg_dev(const float* x, const float* eps2, const float* noise, const float* x0, const uint8_t* mask,
                                    const float* alpha, const float* alpha_hat, const float* beta, const int64_t* t_dev,
                                    float cfg_scale, float* x_out, float* x_out2, long n, afd_stream_t stream);
int afd_ddim_step_masked(const float* x, const float* eps, const float* noise, const float* x0, const uint8_t* mask,
                         const float* alpha_hat, int t, int t_prev, float eta, float* x_out, long n, afd_stream_t stream);
int afd_ddim_step_masked_dev(const float* x, const float* eps, const float* noise, const float* x0, const uint8_t* mask,
                             const float* alpha_hat, const int64_t* t_dev, const int64_t* t_prev_dev, float eta, float* x_out, long n,
                             afd_stream_t stream);
int afd_ddim_step_masked_cfg(const float* x, const float* eps2, const float* noise, const float* x0, const uint8_t* mask,
                             const float* alpha_hat, int t, int t_prev, float eta, float cfg_scale, float* x_out, float* x_out2, long n,
                             afd_stream_t stream);
int afd_ddim_step_masked_cfg_dev(const float* x, const float* eps2, const float* noise, const float* x0, const uint8_t* mask,
                                 const float* alpha_hat, const int64_t* t_dev, const int64_t* t_prev_dev, float eta, float cfg_scale,
                                 float* x_out, float* x_out2, long n, afd_stream_t stream);
/* q(x_{t_to} | x_{t_from}) of the forward process in one jump, fp32 with one rounding per operation:
 *   a = alpha_hat[t_to] / alpha_hat[t_from];   out = (sqrt(a) * x) + (sqrt(1 - a) * noise)
 * Requires 0 <= t_from < t_to (t_to is not checked against the table's length) and n > 0.  x_out may alias x. */
int afd_renoise(const float* x, const float* noise, const float* alpha_hat, int t_from, int t_to, float* x_out, long n,
                afd_stream_t stream);
/* ---- reference-guided sampling (ILVR, Choi et al. 2021): the low-pass refinement after a sampler step ----
 * With one N x N filter (N odd, N <= 15), D = afd_filt_down2_fwd and U = afd_filt_up2_fwd, both with these taps, and L = levels:
 *   phi(v) = 4^L U^L(D^L(v))                                  (factor 2^L; the 4 per level undoes up2's DC gain of 1/4)
 * Per S x S plane (`planes` of them, contiguous; S a power of two in [4, 64], L >= 1, S / 2^L >= 2), one workgroup per plane:
 *   known = ref                                               if t_prev == 0
 *           (sqrt(a) * ref) + (sqrt(1 - a) * noise)           otherwise, a = alpha_hat[t_prev] (afd_noise_images' order, fp32,
 *                                                             one rounding per operation)
 *   out   = x + 4^L r,   r = U^L(D^L(known - x))              (x_out2, when given, receives the same values)
 * The tap sums run in the general resamplers' order (a outer, b inner, ascending; U visits only the taps that land on a
 * sample), each step a fused multiply-add; no atomics, so the same bits from call to call.  For symmetric taps U = D^T and phi is
 * symmetric positive semi-definite.  noise may be NULL only when t_prev == 0 on the host form and never on the _dev form.
 * x_out may be x itself (the plane is read before it is written) and is otherwise apart from it; ref and noise must not overlap
 * x_out or x_out2.  Requires t_prev >= 0 (not checked against the table's length) and planes > 0. */
int afd_lowpass_refine(const float* x, const float* ref, const float* noise /* NULL only when t_prev == 0 */, const float* alpha_hat,
                       int t_prev, const float* taps /* HOST float[N*N] */, int N, int levels, float* x_out,
                       float* x_out2 /* or NULL */, long planes, int S, afd_stream_t stream);
/* same with t_prev = t_prev_dev[0] read on the device (graph-replayable; the index is not checked; 0 => known = ref) */
int afd_lowpass_refine_dev(const float* x, const float* ref, const float* noise, const float* alpha_hat, const int64_t* t_prev_dev,
                           const float* taps /* HOST float[N*N] */, int N, int levels, float* x_out, float* x_out2 /* or NULL */,
                           long planes, int S, afd_stream_t stream);
int afd_quantize_u8(const float* x, uint8_t* out, long n, afd_stream_t stream);

/* ---- F17 (Config E): scipy.ndimage.rotate(order=3, mode='grid-wrap', prefilter=True) per (H,W) plane ----
 * ddpm_models.py:421-429.  in_coord = M @ out_coord + offset (row, col); matrix4 / offset2 are HOST doubles built
 * exactly as scipy.ndimage.rotate builds them; fp64 prefilter + interpolation, one rounding to fp32.
 * workspace: afd_rotate_workspace_bytes(planes, H, W). */
size_t afd_rotate_workspace_bytes(long planes, int H, int W);
int afd_affine_spline3_wrap(const float* x, float* y, long planes, int H, int W, const double* matrix4, const double* offset2,
                            void* workspace, afd_stream_t stream);
/* ---- equivariance scores (EQ-T / EQ-R, Karras et al. 2021): prefilter once, resample and compare many times ----
 * The prefilter of afd_affine_spline3_wrap as its own entry: x (planes, H, W) fp32 -> coef, its fp64 cubic B-spline
 * coefficients (periodic).  afd_affine_spline3_wrap is this call followed by the interpolation. */
int afd_spline3_prefilter_wrap(const float* x, double* coef, long planes, int H, int W, afd_stream_t stream);
/* Row-wise resampling.  coef: n_src prefiltered fields of C planes each; affine: K transforms of 6 fp64 device values
 * [m00, m01, m10, m11, off0, off1] (in = M @ out + off, row / col order); img and k: int64 device arrays of `rows` values, read
 * on the device: the caller keeps them in [0, n_src) and [0, K) (nothing checks them here).
 *   out[r] (C, H, W) = field img[r] under transform k[r], rounded once to fp32: afd_affine_spline3_wrap's output for that field
 *   and that matrix, bit for bit (the same weight and index arithmetic in the same order). */
int afd_affine_spline3_wrap_rows(const double* coef, long n_src, const int64_t* img, const double* affine, long K, const int64_t* k,
                                 float* out, long rows, int C, int H, int W, afd_stream_t stream);
/* The fused comparison, one workgroup per row, in fp64.  ref = field img[r] of coef under transform k[r], evaluated per pixel and
 * never rounded or stored; the mask of the transform for `margin` (pixels) holds at output pixel o iff o and its unwrapped
 * source c = M o + off both lie in [margin, H-1-margin] x [margin, W-1-margin] (c: two products and two sums per coordinate,
 * each rounded, no fused multiply-add).  With d = double(g[r]) - ref over the masked pixels of all C planes:
 *   out[r] = [sum d^2, sum ref^2, masked pixels * C]      (out: rows x 3 fp64)
 * Deterministic: fixed per-thread order, fixed wave tree, waves summed in order, no atomics.  Outputs may overlap no input. */
int afd_eq_terms(const double* coef, long n_src, const int64_t* img, const double* affine, long K, const int64_t* k, const float* g,
                 double margin, double* out, long rows, int C, int H, int W, afd_stream_t stream);

/* ---- F15: loss + optimiser ------------------------------------------- ddpm_utils.py:489-490,503-507
 * mse: loss_out[0] = mean((pred-target)^2) (deterministic two-stage reduction; workspace >= 4096 floats);
 * mse_bwd: dpred = 2*(pred-target)/n * dloss[0].
 * adamw: torch.optim.AdamW(lr, betas, eps, weight_decay) over flat fp32 buffers; `state` is
 * device float[4] {step, bias_corr1, bias_corr2, _} advanced by afd_adamw_tick (graph-replay safe).
 * The AdamW element, per fp32 value, one rounding per operation in this order (no fused multiply-add), with
 * decay = 1 - lr * weight_decay, step_size = lr / bias_corr1, inv_sqrt_bc2 = 1 / sqrt(bias_corr2) formed once in fp32:
 *     gi = g * grad_scale;  pi = p * decay;  m = m + (gi - m) * (1 - beta1);  v = v * beta2 + gi * gi * (1 - beta2);
 *     p = pi - step_size * (m / (sqrt(v) * inv_sqrt_bc2 + eps))
 * ONE kernel applies it, in every form below: afd_adamw_step (lr by value), afd_adamw_ema_step (lr by value, the EMA rule on
 * the new p in the same pass) and afd_adamw_ctl_step (lr and the clip coefficient read from `ctl` on the device, with or
 * without the EMA).  The forms differ in nothing else: the same inputs give the same bits through each. */
int afd_mse_fwd(const float* pred, const float* target, float* loss_out, float* workspace, long n, afd_stream_t stream);
int afd_mse_bwd(const float* pred, const float* target, const float* dloss, float* dpred, long n, afd_stream_t stream);

/* ---- training objectives: what the network's output means, and a per-timestep loss weight -------- Diffusion(prediction=) /
 * TrainStep(loss_weighting=).  With a = alpha_hat[t[b]], sa = sqrt(a), sb = sqrt(1 - a) (afd_noise_images' two expressions), the
 * target of row b is eps (AFD_PRED_EPS), sa eps - sb x0 (AFD_PRED_V, Salimans & Ho 2022) or x0 (AFD_PRED_X0); it is formed in
 * registers, never written.  t: B int64 timesteps on the device, each in [0, T) (read unchecked); w: T floats indexed by t[b],
 * or NULL for weight 1; pred, x0, eps, dpred: B x chw floats.
 *   fwd: loss_out[0] = (1 / (B chw)) sum_b w[t[b]] sum_i (pred - target)^2: two launches, a deterministic two-stage sum over a
 *        fixed number of partials (workspace >= 4096 floats), no atomics: identical bytes run to run;
 *   bwd: dpred = (dloss[0] * 2 / (B chw) * w[t[b]]) * (pred - target), the target recomputed: one launch.
 * 128-bit accesses when chw % 4 == 0 and the float pointers are 16-byte aligned, element by element otherwise, with the same
 * values either way.
 * afd_pred_to_eps: the network's output `out` at x_t -> eps, one launch; eps_out may be `out` (in place):
 *   AFD_PRED_V: eps = (sa out) + (sb x_t);   AFD_PRED_X0: eps = (x_t - sa out) / sb;   AFD_PRED_EPS is AFD_EINVAL. */
#define AFD_PRED_EPS 0
#define AFD_PRED_V 1
#define AFD_PRED_X0 2
int afd_objective_loss_fwd(const float* pred, const float* x0, const float* eps, const int64_t* t, const float* alpha_hat,
                           const float* w_or_null, int kind, float* loss_out, float* workspace, long B, long chw,
                           afd_stream_t stream);
int afd_objective_loss_bwd(const float* pred, const float* x0, const float* eps, const int64_t* t, const float* alpha_hat,
                           const float* w_or_null, int kind, const float* dloss, float* dpred, long B, long chw,
                           afd_stream_t stream);
int afd_pred_to_eps(const float* out, const float* x_t, const int64_t* t, const float* alpha_hat, int kind, float* eps_out, long B,
                    long chw, afd_stream_t stream);

/* ---- progressive distillation (Salimans & Ho 2022): the teacher's two DDIM steps as one target ------ Diffusion.distill_targets /
 * training.DistillStep.  Row b goes t[b] -> t_mid[b] -> t_prev[b] with eta = 0.  With a = alpha_hat[.], al = sqrt(a), sg = sqrt(1 - a)
 * (primes: at t_mid, double primes: at t_prev; the chain's last level t_prev[b] == 0 is alpha_hat[0], exactly as afd_ddim_step reads
 * it, so the target matches the sampler's last step), and (x_hat, eps_hat) of a raw output p of `kind` at z on level (al, sg):
 *     AFD_PRED_EPS: ((z - sg p) / al, p)     AFD_PRED_V: (al z - sg p, sg z + al p)     AFD_PRED_X0: (p, (z - al p) / sg)
 * afd_distill_mid:    z_mid = al' x_hat_1 + sg' eps_hat_1, from out1 = the teacher's output at (z_t, t);
 * afd_distill_target: z_prev = al'' x_hat_2 + sg'' eps_hat_2, from out2 = the teacher's output at (z_mid, t_mid); then
 *     x_tilde = (z_prev - r z_t) / (al'' - r al), r = sg'' / sg,  eps_tilde = (z_t - al x_tilde) / sg:
 *     the (x0, eps) pair whose one DDIM step from z_t lands on z_prev, so a TrainStep on (x_tilde, t, eps_tilde) re-forms z_t and
 *     trains the student's single step towards the teacher's two.
 * One launch each, no reduction.  Every element is widened to fp64, the roots are taken in fp64 from the fp32 table, everything
 * is evaluated in fp64 and rounded once on the store (al'' - r al is a few 1e-3 between neighbouring levels and the numerator
 * cancels to the same order).  t, t_mid, t_prev: B int64 each on the device, in [0, T) with alpha_hat[t] < alpha_hat[t_mid] <
 * alpha_hat[t_prev], read unchecked; all float tensors B x chw.
 * Aliasing: every output may be any float input of the same call ITSELF (the same pointer: each thread reads its quad of every
 * input before it writes); otherwise it must share no memory with it, and x_tilde, eps_tilde must not overlap each other or the
 * timestep tensors.  128-bit accesses when chw % 4 == 0 and the float pointers are 16-byte aligned, element by element otherwise,
 * with the same values either way.  AFD_EINVAL (nothing launched) on NULL pointers, sizes <= 0, a bad kind or such an overlap. */
int afd_distill_mid(const float* out1, const float* z_t, const int64_t* t, const int64_t* t_mid, const float* alpha_hat, int kind,
                    float* z_mid, long B, long chw, afd_stream_t stream);
int afd_distill_target(const float* out2, const float* z_mid, const float* z_t, const int64_t* t, const int64_t* t_mid,
                       const int64_t* t_prev, const float* alpha_hat, int kind, float* x_tilde, float* eps_tilde, long B, long chw,
                       afd_stream_t stream);

/* ---- consistency distillation (Song et al. 2023; Luo et al. 2023, the discrete-time DDIM-solver form) ------
 * Diffusion.consistency_targets / consistency_sample, training.ConsistencyStep.  coef: the (T, 2) fp64 device table
 * [c_skip, c_out] of Diffusion.consistency_coefficients, c_skip[t] = sd^2 / ((s t)^2 + sd^2), c_out[t] = s t / sqrt((s t)^2 + sd^2),
 * row 0 exactly (1, 0).  With (al, sg) and x_hat(p, z; t) as for afd_distill_* above (level 0 is alpha_hat[0]), the consistency
 * function of a raw output p of `kind` at z on level t is
 *     f(z, t) = c_skip[t] z + c_out[t] x_hat(p, z; t),
 * and where c_out[t] == 0 (the boundary t = 0) p is NOT used: f has z's bits even if p holds NaN or Inf there.
 * afd_consistency_fn:     f_out = f(z, t[b]) per row b, from out = the output at (z, t).
 * afd_consistency_target: out_tgt = the target network's output at (z_prev, t_prev); per row
 *     f_tgt = f(z_prev, t_prev)   (z_prev itself at t_prev == 0),
 *     x_tilde = (f_tgt - c_skip[t] z_t) / c_out[t],   eps_tilde = (z_t - al x_tilde) / sg:
 *     the x0 a student must predict at (z_t, t) for its f to equal f_tgt, and the eps that re-forms z_t with it, so a TrainStep on
 *     (x_tilde, t, eps_tilde) trains the student's f(z_t, t) towards the target's f(z_prev, t_prev).  Needs t[b] >= 1 (c_out[t] > 0)
 *     and t_prev[b] < t[b]; both are read on the device, unchecked, in [0, T).
 * afd_consistency_step[_dev]: the sampler's move at one level for all n_rows rows (t, t_next host ints, 0 <= t_next < t, or
 *     element 0 of two int64 device tensors: graph-replayable).  f = f(z, t) rounded to fp32 once, then
 *         t_next == 0:  x_out = f                                                  (noise is not read and may be NULL)
 *         otherwise:    x_out = (sqrt(a_next) * f) + (sqrt(1 - a_next) * noise)    (afd_noise_images' fp32 expression and order)
 *     so the step has the bits of afd_noise_images(afd_consistency_fn(out, z, t), noise, t_next).
 * One launch each, no reduction, no atomics.  f, x_tilde and eps_tilde are evaluated in fp64 from the widened fp32 elements with
 * the roots taken in fp64 from the fp32 table, and rounded once on the store.  Aliasing: every output may be a float input of the
 * same call ITSELF (f_out: out or z; x_tilde / eps_tilde: out_tgt, z_prev or z_t; x_out: out or z) and must otherwise share no
 * memory with it; outputs must not overlap each other, noise or the timestep tensors.  128-bit accesses when chw % 4 == 0 and the
 * float pointers are 16-byte aligned, element by element otherwise, with the same values either way.  AFD_EINVAL (nothing
 * launched) on NULL pointers, sizes <= 0, a bad kind, such an overlap, host t / t_next out of order, or noise NULL with host
 * t_next > 0. */
int afd_consistency_fn(const float* out, const float* z, const int64_t* t, const float* alpha_hat, const double* coef, int kind,
                       float* f_out, long B, long chw, afd_stream_t stream);
int afd_consistency_target(const float* out_tgt, const float* z_prev, const float* z_t, const int64_t* t, const int64_t* t_prev,
                           const float* alpha_hat, const double* coef, int kind, float* x_tilde, float* eps_tilde, long B, long chw,
                           afd_stream_t stream);
int afd_consistency_step(const float* out, const float* z, const float* noise_or_null, const float* alpha_hat, const double* coef,
                         int kind, int t, int t_next, float* x_out, long n_rows, long chw, afd_stream_t stream);
int afd_consistency_step_dev(const float* out, const float* z, const float* noise_or_null, const float* alpha_hat, const double* coef,
                             int kind, const int64_t* t_dev, const int64_t* t_next_dev, float* x_out, long n_rows, long chw,
                             afd_stream_t stream);

/* ---- learned reverse-process variances and the hybrid loss (Nichol & Dhariwal 2021) ------ Diffusion(variance="learned") /
 * TrainStep(vlb_lambda=).  The network's output out2 holds, per row b, 2 chw floats: the prediction p (eps, v or x0 by `kind`)
 * and, chw floats later, the interpolation coefficient v.  lv_coef: the (T, 3) fp64 device table [lb_t, lbt_t, k_t] of
 * Diffusion.lvar_coefficients (lb_t = log beta_t, lbt_t = log beta~_t, k_t = beta_t^2 / (alpha_t (1 - ah_t))).  Per element:
 *   logvar = ((v + 1) / 2) lb_t + (1 - (v + 1) / 2) lbt_t                                     (v is not clamped)
 *   t >= 2: term = 0.5 (x + expm1(-x) + k_t d^2 exp(-logvar)), x = logvar - lbt_t, d^2 = f2 (p - target)^2 in fp64 with
 *           f2 = 1 (eps), a (v), a / (1 - a) (x0), a = alpha_hat[t]: the KL term with the means' difference in eps-space;
 *   t == 1: term = -log p(x0 | x_1), Ho et al.'s discretised Gaussian exactly as afd_vlb_terms', with log_scale = logvar / 2 and
 *           mean = afd_denoise_step's fp32 expression at i = 1 from x_t (afd_noise_images' expression) and eps_hat
 *           (afd_pred_to_eps' expression).
 * Terms and dL/dv are evaluated in fp64 from the fp32 inputs; dL/dv is rounded once to fp32.  With N = B chw:
 *   L_simple = afd_objective_loss_fwd's value on the p half;  L_vlb = (1 / (N ln 2)) sum term;  L = L_simple + vlb_scale L_vlb
 * afd_lvar_loss_fwd: loss_out = {L, L_vlb} in fp32, sums_out (may be NULL) the same two in fp64.  Two launches; a deterministic
 *   two-stage sum (workspace >= 4096 floats, 8-byte aligned), no atomics.
 * afd_lvar_loss_bwd: one launch writes both halves of dout2: the p half is afd_objective_loss_bwd's dpred bit for bit (the mean is
 *   stopped in L_vlb), the v half is dloss[0] vlb_scale / (N ln 2) d term / d v, through the tanh CDFs on decoder rows and zero
 *   where the 1e-12 clamp is active.
 * afd_split_pred: out2 -> eps_out (B x chw; afd_pred_to_eps' conversion, a copy for AFD_PRED_EPS, where x_t, t and alpha_hat may
 *   be NULL) and, when v_out is not NULL, the v half; one launch.
 * afd_denoise_step_lvar[_dev]: x_out = mean + (float)exp(logvar / 2) noise with afd_denoise_step's mean from eps_hat; noise is
 *   ignored at step 1 and may be NULL.  x: B x chw, out2: B x 2 chw.  _dev reads the step from t_dev[0].  x_out may be x.
 * afd_denoise_step_lvar_cfg[_dev]: out2 holds 2 B rows, conditional then unconditional; the two eps_hat are combined by
 *   afd_denoise_step_cfg's lerp, the variance is the conditional row's; x_out2 (may be NULL) receives the same values as x_out.
 * afd_vlb_terms_lvar: afd_vlb_terms with the per-element variance: term[r] = sum_j term, sq[r] = sum_j d^2, fp64, one workgroup
 *   per row, the same deterministic reduction; out2: rows x 2 per.
 * 128-bit accesses when chw % 4 == 0 and the float pointers are 16-byte aligned, element by element otherwise, with the same
 * values either way.  AFD_EINVAL (nothing written) on sizes <= 0, a bad kind, NULL required pointers, or an output that overlaps
 * an input it may not alias. */
int afd_lvar_loss_fwd(const float* out2, const float* x0, const float* eps, const int64_t* t, const float* alpha,
                      const float* alpha_hat, const float* beta, const double* lv_coef, const float* w_or_null, int kind,
                      double vlb_scale, float* loss_out, double* sums_out_or_null, float* workspace, long B, long chw,
                      afd_stream_t stream);
int afd_lvar_loss_bwd(const float* out2, const float* x0, const float* eps, const int64_t* t, const float* alpha,
                      const float* alpha_hat, const float* beta, const double* lv_coef, const float* w_or_null, int kind,
                      double vlb_scale, const float* dloss, float* dout2, long B, long chw, afd_stream_t stream);
int afd_split_pred(const float* out2, const float* x_t, const int64_t* t, const float* alpha_hat, int kind, float* eps_out,
                   float* v_out_or_null, long B, long chw, afd_stream_t stream);
int afd_denoise_step_lvar(const float* x, const float* out2, const float* noise_or_null, const float* alpha, const float* alpha_hat,
                          const float* beta, const double* lv_coef, int kind, int i, float* x_out, long B, long chw,
                          afd_stream_t stream);
int afd_denoise_step_lvar_dev(const float* x, const float* out2, const float* noise_or_null, const float* alpha,
                              const float* alpha_hat, const float* beta, const double* lv_coef, int kind, const int64_t* t_dev,
                              float* x_out, long B, long chw, afd_stream_t stream);
int afd_denoise_step_lvar_cfg(const float* x, const float* out2, const float* noise_or_null, const float* alpha,
                              const float* alpha_hat, const float* beta, const double* lv_coef, int kind, int i, float cfg_scale,
                              float* x_out, float* x_out2, long B, long chw, afd_stream_t stream);
int afd_denoise_step_lvar_cfg_dev(const float* x, const float* out2, const float* noise_or_null, const float* alpha,
                                  const float* alpha_hat, const float* beta, const double* lv_coef, int kind, const int64_t* t_dev,
                                  float cfg_scale, float* x_out, float* x_out2, long B, long chw, afd_stream_t stream);
int afd_vlb_terms_lvar(const float* x0, long n_img, const int64_t* img, const float* x_t, const float* eps, const float* out2,
                       const int64_t* t, const double* lv_coef, long T, const float* alpha, const float* alpha_hat,
                       const float* beta, int kind, double* term, double* sq, long rows, long per, afd_stream_t stream);

/* ---- loss-aware timestep sampling (Nichol & Dhariwal 2021, loss-second-moment resampling), on the device ------ training.
 * LossSecondMomentSampler / TrainStep(t_sampler=).  State: hist (T, H) fp64, the last H row losses seen at each timestep, and
 * count (T) int32; lo is the smallest timestep that is drawn, n = T - lo (DESIGN.md section 6m has the semantics in full).
 * afd_loss_rows / afd_lvar_loss_rows: the inputs of afd_objective_loss_fwd / afd_lvar_loss_fwd; rows[b] (B doubles) is row b's
 *   share of that loss, times B:  (1 / chw) w[t[b]] sum_i d_i^2  [+ (vlb_scale / (chw ln 2)) sum_i term_i],  with d_i = pred -
 *   target formed by the loss kernels' own fp32 expression and everything after it in fp64.  One launch, one workgroup per row, a
 *   fixed summation tree, no atomics: identical bytes run to run; 128-bit accesses when chw % 4 == 0 and the float pointers are
 *   16-byte aligned, element by element otherwise, with the same values either way.  rows must not overlap an input.
 * afd_tsampler_tick: ONE launch of ONE workgroup.  Update: the rows b = 0 .. B - 1 in order; a row whose loss is not finite (or
 *   whose t lies outside [0, T)) is skipped; hist[t[b]] takes rows[b] at position count[t[b]]++, or, when it is full, shifts left
 *   by one and takes it last.  Refresh: warm[0] = (count[t] == H for every t in [lo, T)); with q_t = sqrt(mean_j hist[t][j]^2),
 *     warm and 0 < sum q < inf:  prob[t] = (q_t / sum q) (1 - uniform_prob) + uniform_prob / n,  iw_t = 1 / (n prob[t])
 *     otherwise:                 prob[t] = 1 / n,  iw_t = 1 exactly;                  t < lo: prob[t] = 0, iw_t = 1
 *   cdf (n doubles) = the inclusive prefix sum of prob over [lo, T) divided by its last value, the last entry exactly 1;
 *   wtab[t] = (float)(w_base[t] iw_t) (w_base NULL: 1), vwtab[t] = (float)iw_t (vwtab may be NULL): the tables the loss kernels
 *   read as w and vw.  fp64 throughout, every sum in a fixed order.  Any T, H and B.
 * afd_tsampler_draw: t_out[b] = lo + the first k with u[b] < cdf[k] (u: B doubles in [0, 1)), clamped to T - 1; one launch.
 * afd_lvar_loss_fwd_tw / _bwd_tw: afd_lvar_loss_fwd / _bwd with a second table vw (T floats, or NULL for 1): vw[t[b]] multiplies
 *   each of row b's bound terms (forward) and row b's dL/dv (backward).  afd_lvar_loss_fwd / _bwd are these with NULL.
 * AFD_EINVAL (nothing launched) on NULL required pointers, sizes <= 0, H < 1, uniform_prob outside [0, 1), lo outside [0, T),
 * a bad kind.  t is read on the device, unchecked by the row kernels. */
int afd_loss_rows(const float* pred, const float* x0, const float* eps, const int64_t* t, const float* alpha_hat,
                  const float* w_or_null, int kind, double* rows, long B, long chw, afd_stream_t stream);
int afd_lvar_loss_rows(const float* out2, const float* x0, const float* eps, const int64_t* t, const float* alpha,
                       const float* alpha_hat, const float* beta, const double* lv_coef, const float* w_or_null, int kind,
                       double vlb_scale, double* rows, long B, long chw, afd_stream_t stream);
int afd_tsampler_tick(const int64_t* t, const double* rows, long B, double* hist, int* count, long T, long H, long lo,
                      double uniform_prob, const float* w_base_or_null, double* prob, double* cdf, float* wtab,
                      float* vwtab_or_null, int* warm, afd_stream_t stream);
int afd_tsampler_draw(const double* cdf, const double* u, long lo, long T, int64_t* t_out, long B, afd_stream_t stream);
int afd_lvar_loss_fwd_tw(const float* out2, const float* x0, const float* eps, const int64_t* t, const float* alpha,
                         const float* alpha_hat, const float* beta, const double* lv_coef, const float* w_or_null,
                         const float* vw_or_null, int kind, double vlb_scale, float* loss_out, double* sums_out_or_null,
                         float* workspace, long B, long chw, afd_stream_t stream);
int afd_lvar_loss_bwd_tw(const float* out2, const float* x0, const float* eps, const int64_t* t, const float* alpha,
                         const float* alpha_hat, const float* beta, const double* lv_coef, const float* w_or_null,
                         const float* vw_or_null, int kind, double vlb_scale, const float* dloss, float* dout2, long B, long chw,
                         afd_stream_t stream);
int afd_adamw_tick(float* state, float beta1, float beta2, afd_stream_t stream);
int afd_adamw_step(float* p, const float* g, float* m, float* v, long n, const float* state,
                   float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                   afd_stream_t stream);

/* ---- EMA of the weights (modules/ddpm_utils.py:26-51) ------------------------------------------------- training.EMA / TrainStep(ema=)
 * The rule, per fp32 element, with one rounding per operation in this order (torch's `old * beta + (1 - beta) * new`):
 *     copy != 0:  ema = p                                        (bit for bit, as load_state_dict)
 *     otherwise:  ema = (ema * beta) + (p * one_minus_beta)
 * beta = float(beta) and one_minus_beta = float(1.0 - beta) with the subtraction done in double on the host (never 1 - beta in
 * fp32 on the device).  Both must lie in [0, 1].
 * afd_ema_step: the rule alone over n elements (ema and p must not overlap).
 * afd_adamw_ema_tick: exactly afd_adamw_tick on adam_state, plus the EMA call counter ema_state = device int[2] {calls, copy}:
 *   copy = (calls < start), then ++calls -- EMA.step_ema's order, kept on the device so a replayed step crosses `start` correctly.
 * afd_adamw_ema_step: afd_adamw_step's form with the EMA: for i < n_active the AdamW element (above), then the rule on the
 *   NEW p with copy = ema_state[1]; for n_active <= i < n_ema the rule alone on the unchanged p (parameters the optimiser never
 *   touches, which the reference's EMA still walks).  Requires 0 < n_active <= n_ema.
 * 16-byte accesses when every pointer is 16-byte aligned, element-wise otherwise; the results do not depend on which. */
int afd_ema_step(float* ema, const float* p, long n, int copy, float beta, float one_minus_beta, afd_stream_t stream);
int afd_adamw_ema_tick(float* adam_state, float beta1, float beta2, int* ema_state, int start, afd_stream_t stream);
int afd_adamw_ema_step(float* p, const float* g, float* m, float* v, long n_active, const float* adam_state, float lr,
                       float beta1, float beta2, float eps, float weight_decay, float grad_scale, float* ema, long n_ema,
                       const int* ema_state, float beta, float one_minus_beta, afd_stream_t stream);

/* ---- gradient-norm clipping + learning-rate schedule, on the device ------ training.FusedAdamW / TrainStep(max_grad_norm=, lr_schedule=)
 * torch.nn.utils.clip_grad_norm_(norm_type=2) and torch.optim.lr_scheduler.LambdaLR (warm-up, then constant / linear / cosine
 * decay) between backward and AdamW, with the learning rate and the clip coefficient in DEVICE memory so that a captured step
 * replays them correctly: [afd_grad_sqnorm_partials ->] afd_adamw_ctl_tick -> afd_adamw_ctl_step, in place of tick + step.
 *
 * afd_grad_sqnorm_partials: partials[j] = fp64 sum over slice j of (double)(g[i] * grad_scale)^2, the product formed in fp32 exactly
 *   as the AdamW kernels form it (the norm of the gradient the optimiser consumes; grad_scale = 1 / world under data parallelism).
 *   n_partials must equal afd_grad_sqnorm_n_partials() (512); slice j is [j*S, (j+1)*S) with S = 4 * ceil(n / 2048), so slices
 *   beyond n hold 0.  Deterministic: fixed slice per workgroup, fixed element order per thread, fixed tree, no atomics -- the
 *   bytes do not depend on the run, the launch grid or the alignment of g (16-byte loads when g is 16-byte aligned, scalar loads
 *   of the same elements in the same order otherwise).  fp64 squares: |g| ~ 1e20 stays finite; inf / NaN elements give inf / NaN.
 * afd_adamw_ctl_tick: one workgroup, in this order:
 *   1. with partials: sq = their sum in index order (fp64), norm = sqrt(sq), and with max_norm > 0
 *      coef = min(1, max_norm / (norm + 1e-6)) (a NaN norm gives a NaN coef, as torch's clamp does); otherwise coef = 1;
 *   2. with skip_nonfinite and norm inf / NaN: ctl.skip = 1, ++ctl.n_skipped, ctl.norm / ctl.sq reported, NOTHING else changes
 *      (no Adam step, no EMA call, lr / coef / index / factor keep their last values); otherwise ctl.skip = 0 and
 *   3. exactly afd_adamw_tick on adam_state (afd_adamw_ema_tick with ema_state / ema_start when ema_state is not NULL);
 *   4. k = step - 1 (the 0-based index of this update), lr = (float)(base_lr * factor(k)), factor in fp64:
 *        k < warmup:       k / max(1, warmup)                         (so lr = 0 at k = 0 when warmup > 0: LambdaLR's semantics)
 *        kind constant:    1
 *        otherwise:        pr = min(1, (k - warmup) / max(1, total - warmup)),
 *                          base = 0.5 * (1 + cos(pi * pr)) (cosine) or 1 - pr (linear), factor = min_ratio + (1 - min_ratio) * base;
 *   5. ctl = device double[8] {lr (the fp32 value, widened), coef, norm, skip, n_skipped, sq, k, factor}.  n_skipped accumulates:
 *      zero the buffer once.
 *   cfg points to HOST memory and is copied into the kernel arguments (captured by value: the schedule is fixed, only its position
 *   is device state).  Rejected before any device is touched: NULL adam_state / cfg / ctl, base_lr not finite or < 0, warmup < 0,
 *   unknown kind, total < warmup for a non-constant kind, min_ratio outside [0, 1], NaN max_norm, n_partials outside [1, 1024]
 *   when partials is given, ema_start < 0 when ema_state is given.
 * afd_adamw_ctl_step: the form of afd_adamw_step (ema == NULL; n_ema, ema_state, beta, one_minus_beta ignored) or of
 *   afd_adamw_ema_step that takes lr = (float)ctl.lr and grad_scale * (float)ctl.coef (an fp32 product) from the device: with
 *   ctl.lr = lr, ctl.coef = 1, ctl.skip = 0 the results are bit-identical to those entry points.  With ctl.skip != 0 every
 *   thread returns at once: p, m, v and ema are not written. */
#define AFD_LR_CONSTANT 0
#define AFD_LR_LINEAR 1
#define AFD_LR_COSINE 2
typedef struct afd_opt_ctl {
  double base_lr;
  long warmup, total;      /* in optimiser updates; total is ignored by AFD_LR_CONSTANT */
  int kind;                /* AFD_LR_* */
  double min_ratio;        /* the decay ends at base_lr * min_ratio */
  double max_norm;         /* <= 0: no clipping */
  int skip_nonfinite;
} afd_opt_ctl;
int afd_grad_sqnorm_n_partials(void);
int afd_grad_sqnorm_partials(const float* g, long n, float grad_scale, double* partials, int n_partials, afd_stream_t stream);
int afd_adamw_ctl_tick(float* adam_state, float beta1, float beta2, int* ema_state, int ema_start, const double* partials,
                       int n_partials, const afd_opt_ctl* cfg, double* ctl, afd_stream_t stream);
int afd_adamw_ctl_step(float* p, const float* g, float* m, float* v, long n_active, const float* adam_state, const double* ctl,
                       float beta1, float beta2, float eps, float weight_decay, float grad_scale, float* ema, long n_ema,
                       const int* ema_state, float beta, float one_minus_beta, afd_stream_t stream);

/* ---- two-lane replay of a captured step (csrc/replay.hip) --------------------------------- training.TrainStep(graph="lanes")
 * A step captured by the host framework as a hipGraph (forward, backward with the weight gradients forked to a side stream,
 * AdamW) is re-issued from a C++ loop on TWO REAL STREAMS: afd_replay_build walks the graph once (kernel / memset / flat
 * memcpy nodes; no-op and event nodes are folded into the dependencies), puts the weight-gradient kernels (by name) on the side
 * lane and everything else on the main lane, and turns the dependencies that cross lanes into event record / wait pairs;
 * afd_replay_run launches the nodes in capture order, each on its lane's stream.  The graph -- and the memory its nodes
 * point into -- must outlive the handle.  counts (may be NULL) receives {work nodes, main lane, side lane, cross-lane waits}.
 * Replaces nothing in the reference (its loop is eager PyTorch, ddpm_utils.py:494-509): it removes the interpreter from the
 * steady-state step without the cross-branch cost of a hipGraph launch. */
int afd_replay_build(void* hip_graph, void** out_handle, int* counts);
int afd_replay_run(void* handle, afd_stream_t main_stream, afd_stream_t side_stream);
int afd_replay_free(void* handle);

/* ---- batch assembly from a device-resident data set (csrc/loader.hip) ------------------------- data.DeviceDataset.batch
 * data is a contiguous (N, C, H, W) store of uint8 pixels or of floats, idx B indices into it (int64, 8-byte aligned: it may be
 * a view into a longer permutation), flip NULL or B bytes (non-zero: mirror that row left-right), labels / y N and B int64
 * class labels, NULL together.  ONE launch writes, for row b with i = idx[b] and w' = flip[b] ? W - 1 - w : w,
 *     u8:   x[b, c, h, w] = table[c * 256 + data[i, c, h, w']]          table: (C, 256) floats, filled on the host
 *     f32:  x[b, c, h, w] = data[i, c, h, w']   as 32-bit words: NaN payloads, infinities and -0.0 survive
 *     y[b] = labels[i]
 * No arithmetic touches a pixel, so the u8 form returns exactly the floats the table holds.  An index outside [0, N) reads
 * nothing outside data: that row of x is quiet NaN (0x7fc00000) and y[b] = INT64_MIN; indices may repeat.
 * 16 source bytes per lane (one 128-bit load; four / one 128-bit stores) when a row of data is a multiple of 16 bytes and data
 * and x are 16-byte aligned; element by element otherwise, with the same values either way.  x (4-byte aligned) must not
 * overlap an input or y.  AFD_EINVAL (nothing launched) on NULL required pointers, sizes <= 0, labels without y or y without
 * labels, misaligned x / idx, an overlapping x, or more than 2^31 - 1 output planes (B C). */
int afd_batch_gather_u8(const uint8_t* data, long N, long C, long H, long W, const int64_t* idx, const uint8_t* flip_or_null,
                        const float* table, float* x, const int64_t* labels_or_null, int64_t* y_or_null, long B,
                        afd_stream_t stream);
int afd_batch_gather_f32(const float* data, long N, long C, long H, long W, const int64_t* idx, const uint8_t* flip_or_null,
                         float* x, const int64_t* labels_or_null, int64_t* y_or_null, long B, afd_stream_t stream);

/* ---- nearest store rows of a set of queries (csrc/nearest.hip) ------------------------------- data.DeviceDataset.nearest
 * data is a contiguous (N, D) store, queries n rows of the same D and element type, 1 <= k <= 16, exclude NULL or n int64:
 * query q skips store row exclude[q] (a negative value skips nothing).  For query q, idx[q * k + t] and dist[q * k + t], t = 0 ..
 * k - 1, are the k store rows of smallest squared L2 distance, ascending; ties go to the lower store index, so the order is total
 * and the result depends on no tiling, partition or launch order.  A slot with no candidate left (k exceeds the rows available)
 * holds idx -1 and dist -1 (u8) / +inf (f32).
 *     u8:   dist = sum_j (a_j - b_j)^2 in pixel units, exact, int64.  D <= 32768, so that int32 holds every partial sum: with
 *           a' = a - 128 (byte ^ 0x80 as int8) the sum is sum a'^2 + sum b'^2 - 2 sum a'b', the cross term on the i8 matrix pipe.
 *     f32:  dist = sum_j ((double)a_j - (double)b_j)^2 summed in fp64 and rounded once to fp32, ranked by (its bits, index); a NaN
 *           distance is reported as the canonical quiet NaN (0x7fc00000) and ranks after +inf, by index.
 * Each search workgroup leaves the k smallest (distance bits << 32 | index) keys of its chunk of the store in the workspace, a
 * second kernel merges the chunks: two launches on `stream`, no allocation, no host synchronisation, no memset (the workspace
 * needs no initial contents), so a call can be captured into a graph.  afd_nn_search_workspace_bytes: the bytes one call needs
 * (at most 512 n k 8; 0 for sizes the search rejects).  u8 data and queries need no alignment: a D that is no multiple of 16, or a
 * pointer that is not 16-byte aligned, takes byte loads instead of 16-byte ones, with the same result.
 * AFD_EINVAL (nothing launched) on a NULL data / queries / idx / dist / workspace, N, D or n <= 0, k outside [1, 16], D > 32768
 * (u8), N or n >= 2^31, idx / exclude / workspace not 8-byte aligned, dist not aligned to its element, f32 data / queries not
 * 4-byte aligned, a workspace smaller than afd_nn_search_workspace_bytes, or idx / dist / workspace overlapping an input or each
 * other. */
size_t afd_nn_search_workspace_bytes(long N, long D, long n, long k, int f32);
int afd_nn_search_u8(const uint8_t* data, long N, long D, const uint8_t* queries, long n, const int64_t* exclude_or_null, long k,
                     int64_t* idx, int64_t* dist, void* workspace, size_t workspace_bytes, afd_stream_t stream);
int afd_nn_search_f32(const float* data, long N, long D, const float* queries, long n, const int64_t* exclude_or_null, long k,
                      int64_t* idx, float* dist, void* workspace, size_t workspace_bytes, afd_stream_t stream);

/* ---- mean power spectrum of a set of images, in fp64 (csrc/spectrum.hip) ----------------------- spectrum.power_spectrum
 * images is a contiguous (n, C, H, W) set, 1 <= H, W <= 64 (odd and non-square planes included), of uint8 pixels read through
 * table (C, 256) floats (data.normalisation_table) or of floats taken as they are; every value is widened to double and everything
 * after that is fp64.  Per plane: remove_mean != 0 subtracts the plane's own mean, then the plane is multiplied by
 * win_h[y] * win_w[x] (either pointer may be NULL: 1), and F = its 2-D DFT in numpy's convention and rfft2 layout, u in [0, H),
 * v in [0, Wh), Wh = W / 2 + 1.
 *     power[c][u][v] = (1 / n) sum_i |F_{i,c}[u][v]|^2                                                   (C, H, Wh)
 *     radial[c][r]   = sum over (u, v) with bins[u][v] == r of m(v) power[c][u][v]                       (C, R)
 * m(v) = 1 for v = 0 and, for an even W, v = W / 2, else 2 (the mirrored half of the full spectrum); bins is (H, Wh) int32 with
 * values in [-1, R), -1 leaves a coefficient out.  radial is a weighted SUM: the caller divides by its counts.  Either of power
 * and radial may be NULL, not both; bins and R are read only when radial is given.  A NaN or an infinity in a plane propagates
 * to its channel's outputs; nothing is clamped.
 * The DFT is two matrix products on the fp64 matrix pipe with twiddles looked up at (j k) mod N in a table of cos and sin of
 * 2 pi m / N built in fp64 from an integer quadrant and remainder.  Workgroup (slice, channel) sums |F|^2 over its images in
 * registers and leaves one partial in the workspace; a second kernel folds the partials in a fixed tree, divides by n once and
 * reduces radial in a fixed order: two launches on `stream`, no atomics, no allocation, no memset (the workspace needs no initial
 * contents), no synchronisation, so a call can be captured into a graph and repeats bit for bit.  The number of slices depends
 * on (n, C) alone.  afd_spectrum_workspace_bytes: the bytes one call needs (at most 768 H Wh 8 for C <= 768; 0 for sizes the
 * call rejects).
 * AFD_EINVAL (nothing launched) on a NULL images / workspace / table (u8), power and radial both NULL, radial without bins or
 * with R <= 0, n or C <= 0, H or W outside [1, 64], n >= 2^31, C >= 2^31 or n C > 2^40, power / radial / win_h / win_w /
 * workspace not 8-byte aligned, bins / table / f32 images not 4-byte aligned, a workspace smaller than
 * afd_spectrum_workspace_bytes, or power / radial / workspace overlapping an input or each other. */
size_t afd_spectrum_workspace_bytes(long n, long C, long H, long W);
int afd_power_spectrum_u8(const uint8_t* images, const float* table, long n, long C, long H, long W, const double* win_h_or_null,
                          const double* win_w_or_null, int remove_mean, const int* bins_or_null, long R, double* power_or_null,
                          double* radial_or_null, void* workspace, size_t workspace_bytes, afd_stream_t stream);
int afd_power_spectrum_f32(const float* images, long n, long C, long H, long W, const double* win_h_or_null,
                           const double* win_w_or_null, int remove_mean, const int* bins_or_null, long R, double* power_or_null,
                           double* radial_or_null, void* workspace, size_t workspace_bytes, afd_stream_t stream);

/* ---- moments of a feature set and polynomial-kernel MMD sums, in fp64 (csrc/fidelity.hip) ----- fidelity.FeatureStats, kernel_distance
 * The two contractions behind FID and KID.  Every fp32 value is widened to double while it is staged and
 * everything after that is fp64 on the fp64 matrix pipe; there is no fp64 copy of an input in memory, and neither the per-row
 * outer products nor a Gram matrix is ever stored.  Each call is two launches on `stream`: the first leaves per-workgroup partials
 * in the workspace, the second folds them in a fixed order.  No atomics, no allocation, no memset (the workspace needs no initial
 * contents), no synchronisation, so a call can be captured into a graph and repeats bit for bit.
 *
 * afd_feature_moments_f32: X is a contiguous (n, D) array of floats, any n >= 1 and D >= 1.
 *     sum[c]      = sum_r X[r][c]                                                                          (D)
 *     outer[i][j] = sum_r X[r][i] X[r][j]                                                                  (D, D)
 * accumulate = 0 overwrites sum and outer, accumulate = 1 adds to what they hold, so a caller can feed batch after batch.  Only
 * the 64 x 64 tiles on or above the diagonal are computed; an element and its mirror image are written from one value, so outer
 * is symmetric bit for bit (with accumulate = 1 the elements on and above the diagonal are the ones read).  n is split into at
 * most 64 slabs, a number that depends on (n, D) alone; a slab sums its rows in index order, and the slabs are added in slab
 * order.  A NaN at X[r][c] makes sum[c], outer[c][:] and outer[:][c] NaN and nothing else.
 * AFD_EINVAL (nothing launched) on a NULL X / sum / outer / workspace, n or D <= 0, n >= 2^31, D > 2^15, n D > 2^40, accumulate
 * not 0 or 1, X not 4-byte aligned, sum / outer / workspace not 8-byte aligned, a workspace smaller than
 * afd_feature_moments_workspace_bytes (0 for sizes the call rejects), or sum / outer / workspace overlapping X or each other.
 *
 * afd_poly_mmd_sums_f32: A (na, D) and B (nb, D) are contiguous arrays of floats, ia and ib (S, m) int64 row indices into A and
 * B, k(x, y) = (gamma x.y + coef0)^degree with degree an int in [1, 8], the power taken by repeated multiplication.  For subset s,
 * with a_i = A[ia[s][i]] and b_j = B[ib[s][j]],
 *     sums[s][0] = sum_{i != j} k(a_i, a_j)     sums[s][1] = sum_{i != j} k(b_i, b_j)     sums[s][2] = sum_{i, j} k(a_i, b_j)
 * Rows are gathered by index while they are staged.  The two symmetric problems compute the 64 x 64 tiles on or above the
 * diagonal: a tile above it counts twice, a diagonal tile leaves i == j out.  A workgroup sums its tile in a fixed order, and the
 * tiles of a sum are added in a fixed order.  Any m >= 2, S >= 1 and D >= 1; indices may repeat.  An index outside [0, na) /
 * [0, nb) reads nothing outside the arrays: that row counts as NaN.  A NaN in a row reaches only the sums of the subsets that
 * index the row, and only those the row takes part in.
 * AFD_EINVAL (nothing launched) on a NULL A / B / ia / ib / sums / workspace, na, nb, D or S <= 0, m < 2, m > 2^16, degree outside
 * [1, 8], D >= 2^31, na D or nb D > 2^40, more than 2^31 - 1 workgroups, A / B not 4-byte aligned, ia / ib / sums / workspace not
 * 8-byte aligned, a workspace smaller than afd_poly_mmd_workspace_bytes (0 for sizes the call rejects), or sums / workspace
 * overlapping an input or each other. */
size_t afd_feature_moments_workspace_bytes(long n, long D);
int afd_feature_moments_f32(const float* X, long n, long D, double* sum, double* outer, int accumulate, void* workspace,
                            size_t workspace_bytes, afd_stream_t stream);
size_t afd_poly_mmd_workspace_bytes(long S, long m, long D);
int afd_poly_mmd_sums_f32(const float* A, long na, const float* B, long nb, long D, const int64_t* ia, const int64_t* ib, long S, long m,
                          int degree, double gamma, double coef0, double* sums, void* workspace, size_t workspace_bytes,
                          afd_stream_t stream);

/* ---- k-th neighbour radii and ball membership of feature sets, in fp64 (csrc/manifold.hip) ---- manifold.manifold_scores
 * The two contractions behind precision / recall / density / coverage.  Every fp32 value is widened to
 * double while it is staged and everything after that is fp64 on the fp64 matrix pipe; there is no fp64 copy of an input in
 * memory, and no distance matrix is ever stored.
 *
 * The distance.  d2(a, b) = max(0, (s_a + s_b) - 2 a.b), where a.b is one chain of mfma_f64_16x16x4_f64 over the D elements, 4 per
 * instruction in ascending order from a zero accumulator, and s_a = a.a is the same chain.  Every product is exact, only the
 * additions round.  So: d2 is a function of the two rows and D alone (not of n, a row's position, the tiling, or which of the two is
 * the query), symmetric bit for bit and the same in both entry points; d2(a, a) == 0 exactly and d2 >= 0;
 * |d2 - exact| <= 2 (D + 4) 2^-52 (|a|^2 + |b|^2); integer-valued rows whose sums stay below 2^53 give the exact integer.  A NaN in
 * either row makes the distance NaN, and so does an infinity (inf - inf).
 *
 * afd_kth_neighbour_f32: X is a contiguous (n, D) array of floats, 1 <= k <= 16.  radius2[i] is the k-th smallest of d2(X_i, X_j)
 * over j != i: rows are excluded by index, so an identical row elsewhere counts as a neighbour at 0.  A NaN distance is no
 * candidate; with fewer than k candidates radius2[i] = +inf.
 *
 * afd_ball_membership_f32: Q (nq, D) and R (nr, D) are contiguous arrays of floats, radius2 nr doubles, exclude NULL or nq int64
 * (query q skips store row exclude[q]; a negative value skips nothing).  For query q over the store rows j != exclude[q]:
 *     count[q]      = the number of j with d2(Q_q, R_j) <= radius2[j]                                    (nq) int32
 *     nearest[q]    = the j of smallest d2(Q_q, R_j), ties to the lower j;  nearest_d2[q] = that d2       (nq) int64, double
 * A NaN distance or a NaN radius is in no ball and is never the nearest; a +inf radius holds every non-NaN distance.  With no
 * candidate nearest = -1 and nearest_d2 = +inf.  nearest and nearest_d2 are given together or not at all; count may be NULL when
 * they are given.
 *
 * Each call is a small pre-pass that leaves the rows' squared norms in the workspace, and two launches on `stream`: workgroup
 * (stripe, segment) carries 64 rows (queries) past its segment of the other side and leaves their partial results in the
 * workspace (the k smallest distances of the segment; the count and the nearest row there), and a second kernel folds the
 * segments in index order.  The number of segments, at most 64, depends on the sizes alone, and the results do not depend on it.
 * No atomics, no allocation, no memset (the workspace needs no initial contents), no synchronisation, so a call can be captured
 * into a graph and repeats bit for bit.  Any pointer alignment of 4 bytes and any D take the same loads.
 * afd_*_workspace_bytes: the bytes one call needs (at most 8 n (1 + 64 k), and 8 (nq + nr) + 20 x 64 nq; 0 for sizes the call
 * rejects).
 * AFD_EINVAL (nothing launched) on a NULL X / radius2 / Q / R / workspace, count, nearest and nearest_d2 all NULL or only one of
 * nearest and nearest_d2 given, n, nq, nr or D <= 0, k outside [1, 16], n, nq or nr >= 2^31, D > 2^15, rows x D > 2^40, X / Q / R /
 * count not 4-byte aligned, radius2 / exclude / nearest / nearest_d2 / workspace not 8-byte aligned, a workspace that is too
 * small, or an output or the workspace overlapping an input or each other. */
size_t afd_kth_neighbour_workspace_bytes(long n, long D, long k);
int afd_kth_neighbour_f32(const float* X, long n, long D, long k, double* radius2, void* workspace, size_t workspace_bytes,
                          afd_stream_t stream);
size_t afd_ball_membership_workspace_bytes(long nq, long nr, long D);
int afd_ball_membership_f32(const float* Q, long nq, const float* R, long nr, long D, const double* radius2,
                            const int64_t* exclude_or_null, int* count_or_null, int64_t* nearest_or_null, double* nearest_d2_or_null,
                            void* workspace, size_t workspace_bytes, afd_stream_t stream);

/* ---- PSNR and SSIM sums of image pairs, in fp64 (csrc/quality.hip) ------------------------------ quality.image_quality
 * a and b are contiguous (rows, C, H, W) sets of floats or of uint8 pixels, planes = rows * C, 1 <= H, W <= 64.  Every value is
 * widened exactly and everything after that is fp64.
 * The region P of an image is the set of pixels where its H x W uint8 mask in `region` is non-zero, shared by the image's
 * channels; region_rows is rows, or 1 when one mask serves all images; a NULL region is every pixel (region_rows is then 1 or
 * rows all the same).  win is a HOST array of K doubles, K odd, 1 <= K <= 15, K <= min(H, W): window (i, j), 0 <= i <= H - K,
 * 0 <= j <= W - K, covers rows i .. i + K - 1 and columns j .. j + K - 1 with the weights win[r] win[s] (the border is cropped).
 * With the weighted sums m_a, m_b, m_aa, m_bb, m_ab of a, b, a a, b b, a b over a window,
 *     v_aa = m_aa - m_a m_a,  v_bb = m_bb - m_b m_b,  v_ab = m_ab - m_a m_b
 *     ssim = ((2 m_a m_b + c1) (2 v_ab + c2)) / ((m_a m_a + m_b m_b + c1) (v_aa + v_bb + c2))
 * A weighted sum is sum_r win[r] (sum_s win[s] p[i + r][j + s]), s and r ascending, each step one fma from a zero accumulator;
 * the products a a, b b, a b are exact in fp64 and take the same chain in the same operand order, and the rational is evaluated
 * without contraction, so a == b gives ssim == 1.0 exactly in every window.
 *     out[plane] = [ sum_{p in P} (a - b)^2,  sum_{p in P} |a - b|,  |P|,
 *                    the sum of ssim over the windows whose centre pixel (i + (K - 1) / 2, j + (K - 1) / 2) is in P,
 *                    the number of those windows ]                                                            (planes, 5)
 *     ssim_map[plane][i][j] = ssim of window (i, j), whatever the region is (may be NULL)      (planes, H - K + 1, W - K + 1)
 * A pixel outside P is not added to the first three (a NaN there stays out of them); otherwise a NaN or an infinity propagates
 * to its own plane's outputs; nothing is clamped.  uint8 inputs give the exact integers in the first three.
 * One launch on `stream`, one workgroup per plane: a thread adds its pixels and its windows in index order, a shuffle tree adds
 * the lanes, the waves are added in order.  No atomics, no workspace, no allocation, no synchronisation, so a call can be
 * captured into a graph and repeats bit for bit.
 * AFD_EINVAL (nothing launched) on a NULL a / b / win / out, planes or C <= 0, planes not a multiple of C, planes >= 2^31, H or W
 * outside [1, 64], K even, K < 1, K > 15 or K > min(H, W), region_rows neither 1 nor planes / C, out / ssim_map not 8-byte
 * aligned, f32 a / b not 4-byte aligned, or out / ssim_map overlapping a, b, region or each other. */
int afd_pair_quality_f32(const float* a, const float* b, long planes, int C, int H, int W, const double* win, int K, double c1,
                         double c2, const uint8_t* region_or_null, long region_rows, double* out, double* ssim_map_or_null,
                         afd_stream_t stream);
int afd_pair_quality_u8(const uint8_t* a, const uint8_t* b, long planes, int C, int H, int W, const double* win, int K, double c1,
                        double c2, const uint8_t* region_or_null, long region_rows, double* out, double* ssim_map_or_null,
                        afd_stream_t stream);

/* ---- spherical interpolation of latent rows (csrc/slerp.hip) --------------------------------------- Diffusion.interpolate
 * a, b: (pairs, row) fp32; w: W fp32 weights in device memory; out: (pairs, W, row) fp32; row <= 3 * 64 * 64.  Per pair, in fp64:
 *   d = sum_i a_i b_i,  na = sum_i a_i^2,  nb = sum_i b_i^2
 *   c = clamp(d / sqrt(na nb), -1, 1),  omega = acos(c),  so = sin(omega)
 *   na == 0, nb == 0 or so < 1e-6 (parallel and antiparallel rows):  ca = 1 - w,  cb = w                  (lerp: the definition)
 *   otherwise:                                ca = sin((1 - w) omega) / so,  cb = sin(w omega) / so
 *   out_i = (float)(ca * a_i + cb * b_i)      (the products and the sum in fp64 without contraction, then one rounding)
 * With finite inputs w = 0 returns a and w = 1 returns b bit for bit.  One launch on `stream`, one workgroup per (pair, weight).
 * The sums run in an order that depends on `row` alone (element i belongs to thread (i / 4) % 256, ascending within a thread;
 * a shuffle tree over the lanes; the four waves in order), whatever the alignment: no atomics, the same bits from call to call.
 * AFD_EINVAL (nothing launched) on a NULL pointer, pairs, W or row <= 0, row > 12288, pairs * W >= 2^31, a pointer that is not
 * 4-byte aligned, or out overlapping a, b or w. */
int afd_slerp_rows(const float* a, const float* b, const float* w, float* out, long pairs, long W, long row, afd_stream_t stream);

/* ---- diffusion posterior sampling for linear operators (csrc/posterior.hip) ------ posterior.LinearOperator / Diffusion.posterior_sample
 * The operator, per (row, channel) plane of a contiguous (B, C, H, W) fp32 tensor, 1 <= H, W <= 64:
 *   A x = m . S_s(k * x)
 * k * x: the correlation with `kernel`, a HOST float[K * K] (K odd, 1 <= K <= 15; NULL with K == 1 is the delta), zero padding K / 2;
 * S_s: every stride-th row and column, stride 1, 2 or 4 dividing H and W, so the measurement plane is h x w = H / s x W / s;
 * m: `mask`, (mask_channels, h, w) device floats with mask_channels 1 (one mask for every channel) or C, or NULL with
 * mask_channels 0.  That is F.conv2d(x, k, padding = K / 2, stride = s, groups = C) times m; DESIGN.md section 6w.
 *   afd_linop_apply:   y (B, C, h, w) = A x
 *   afd_linop_adjoint: g (B, C, H, W) = A^T r, the transposed strided correlation of m . r -- the exact adjoint
 *   afd_dps_residual:  the step side of DPS in one launch, per plane from LDS.  With a = alpha_hat[t_rows[row]] widened to fp64,
 *       (a_t, b_t) = (1 / sqrt(a), -sqrt(1 - a) / sqrt(a))   AFD_PRED_EPS
 *                    (sqrt(a),     -sqrt(1 - a))             AFD_PRED_V
 *                    (0,           1)                        AFD_PRED_X0        each rounded once to fp32,
 *     x0_hat = (a_t x_t) + (b_t out),   r = A x0_hat - y,   sums[row][c] = sum r^2 of the plane in fp64,   g = A^T r.
 *     x0_hat and r stay in LDS.  t_rows: B int64 timesteps on the device (read unchecked), the tensor the model received.
 *   afd_dps_correct:   x[row] -= c_row ((a_t g) + (b_t v)),  c_row = (float)(zeta / sqrt(sum_c sums[row][c])), the sum in fp64 for
 *     c = 0 .. C - 1; a row whose sum is 0 (and every row when zeta == 0) is not touched.  With v the network's vector-Jacobian
 *     product of g, a_t g + b_t v = |r| grad_{x_t} |y - A x0_hat|: DPS's step zeta / |r| (Chung et al. 2023), decided on the device.
 * Tap sums run a outer, b inner, ascending, one fmaf per tap from a zero accumulator; a plane's sum of squares adds a thread's
 * elements in index order, then a shuffle tree over the lanes, then the four waves in order.  One launch each on `stream`, one
 * workgroup per plane (afd_dps_correct: elementwise); no atomics, no workspace, no synchronisation: the same bits from call to call.
 * AFD_EINVAL (nothing launched) on a NULL pointer (but `mask`, and `kernel` with K == 1), B or C <= 0, B C >= 2^31, K even or outside
 * [1, 15], a stride other than 1, 2, 4 or not dividing H and W, H or W outside [1, 64], mask_channels not 1 or C with a mask or
 * not 0 without, an unknown prediction, a zeta that is negative or not finite, sums not 8-byte aligned, or an output overlapping
 * an input. */
int afd_linop_apply(const float* x, float* y, const float* kernel /* HOST float[K*K] */, int K, int stride, const float* mask_or_null,
                    int mask_channels, long B, int C, int H, int W, afd_stream_t stream);
int afd_linop_adjoint(const float* r, float* g, const float* kernel /* HOST float[K*K] */, int K, int stride, const float* mask_or_null,
                      int mask_channels, long B, int C, int H, int W, afd_stream_t stream);
int afd_dps_residual(const float* x_t, const float* out, const int64_t* t_rows, const float* alpha_hat, int prediction, const float* y,
                     const float* kernel /* HOST float[K*K] */, int K, int stride, const float* mask_or_null, int mask_channels,
                     float* g, double* sums, long B, int C, int H, int W, afd_stream_t stream);
int afd_dps_correct(float* x, const float* g, const float* v, const double* sums, const int64_t* t_rows, const float* alpha_hat,
                    int prediction, double zeta, long B, int C, long HW, afd_stream_t stream);

/* ---- likelihoods from the probability-flow ODE (csrc/likelihood.hip) ------------------------------ Diffusion.ode_likelihood
 * afd_ode_trace_rows: for every row r of the contiguous fp32 (rows, per) arrays v and w, in fp64,
 *     acc[r] = acc[r] + ((cvv * sum_j v[r][j]^2) + (cvw * sum_j v[r][j] w[r][j]))          (w NULL: acc[r] + (cvv * sum_j v[r][j]^2))
 *   acc: `rows` doubles on the device, read and written.  With v a probe and w = J_out^T v this adds one evaluation of the
 *   Hutchinson estimate weight * (c1 |v|^2 + c2 v.w) of the divergence (cvv = weight c1, cvw = weight c2, folded on the host in
 *   fp64); with v = x_U, w = NULL and cvv = -0.5 it adds the prior's -|x_U|^2 / 2.  w may be NULL only when cvw == 0.
 *   One 256-thread workgroup per row.  Each fp32 value is widened and the products are formed in fp64 (exact); element j belongs
 *   to thread (j / 4) % 256, a thread adds its elements in ascending j, a shuffle tree adds the 64 lanes, the four waves are added
 *   in order, and one thread does the read-modify-write of acc[r].  16-byte loads when per % 4 == 0 and v, w are 16-byte aligned,
 *   scalar loads otherwise, the same sums either way.  No atomics, no workspace: the same bits from call to call.
 *   AFD_EINVAL (nothing launched) on NULL v or acc, NULL w with cvw != 0, rows <= 0, per <= 0, rows >= 2^31 or rows * per > 2^40, a
 *   coefficient that is not finite, v / w not 4-byte or acc not 8-byte aligned, or acc overlapping v or w.
 * afd_ode_heun_step: the corrector of Heun's rule for the move s -> u of the ODE dy / dsig = eps, y = x / sqrt(a), sig =
 *   sqrt((1 - a) / a), a_s = alpha_hat[s], a_u = alpha_hat[u].  h = (float)(sqrt((1 - a_u) / a_u) - sqrt((1 - a_s) / a_s)) with the
 *   fp32 table values widened and the whole expression in fp64, rounded once.  Then fp32 with one IEEE rounding per operation (no FMA
 *   contraction, correctly rounded / and sqrt), evaluated in exactly this order:
 *     y   = x / sqrt(a_s)
 *     d   = (0.5 * h) * (eps_s + eps_u)                 (0.5 * h is exact)
 *     out = sqrt(a_u) * (y + d)
 *   eps_s: eps at (x_s, s); eps_u: eps at (the Euler predictor afd_ddim_invert_step(x_s, eps_s, s, u), u).  Requires 1 <= s < u (u is
 *   not checked against the table's length: level 0 is left by an Euler move, the network is never evaluated there) and n > 0,
 *   the elements of x.  x_out may be x itself (otherwise apart from it) and must not overlap eps_s or eps_u. */
int afd_ode_trace_rows(const float* v, const float* w_or_null, double cvv, double cvw, double* acc, long rows, long per,
                       afd_stream_t stream);
int afd_ode_heun_step(const float* x, const float* eps_s, const float* eps_u, const float* alpha_hat, int s, int u, float* x_out, long n,
                      afd_stream_t stream);

/* ---- Analytic-DPM (Bao et al. 2022): the statistic of the optimal reverse variance ------------- analytic.py, Diffusion.
 * estimate_analytic_variance.  eps: contiguous fp32 (B, chw); rows: B doubles on the device,
 *     rows[b] = sum_i (double)e_i * (double)e_i          over row b (each product is exact in fp64)
 *   The _cfg form reads eps2, the 2B-row forward [conditional rows ; unconditional rows], and e_i is the guided eps of the two
 *   halves: e = torch.lerp(e_u, e_c, s) formed in fp32 with ATen's scalar formula, one rounding per operation (|s| < 0.5:
 *   u + s (c - u); otherwise c - (c - u)(1 - s)), exactly as the sampler steps form it.
 *   One launch, one 256-thread workgroup per row: thread i takes the quads i, i + 256, ... of the row and their elements in
 *   index order, a shuffle tree adds the 64 lanes and the four waves are added in order.  No atomics, no workspace: identical
 *   bytes run to run; 16-byte loads when chw % 4 == 0 and the pointer is 16-byte aligned, scalar loads of the same elements in
 *   the same order otherwise.  AFD_EINVAL (nothing launched) on NULL pointers, B <= 0, chw <= 0, B >= 2^31 or rows overlapping
 *   the input. */
int afd_eps_sqnorm_rows(const float* eps, double* rows, long B, long chw, afd_stream_t stream);
int afd_eps_sqnorm_rows_cfg(const float* eps2, float cfg_scale, double* rows, long B, long chw, afd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* AFD_H_ */
