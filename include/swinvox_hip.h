/*
 * swinvox_hip.h -- C ABI of libswinvox_hip.so, the MI355X (gfx950) implementation of the SwinVox
 * Encoder -> Decoder -> Merger -> Refiner forward/backward path.
 *
 * The reference (SandeepaInduwaraSamaranayake/SwinVox) has no FFI layer: its hot path is a chain of
 * stock PyTorch operators dispatched from its models/ package.  Each entry point below replaces one operator
 * class of that chain; the comment above every group cites the
 * reference file:line whose operator it stands in for.  The host side (the swinvox_amd/models package) binds
 * these through ctypes and mirrors the reference's nn.Module surface.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer; typed pointers are fp32 (or as declared), void* activation pointers hold the
 *     element type named by the call's `act_dtype` (SV_F32 / SV_BF16, see below); the library never allocates,
 *     frees or retains memory (all buffers, including workspaces, are owned by the caller);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every call only enqueues work;
 *   - return value: 0 on success, <0 on error (SV_ERR_*); sv_last_error() returns a message for the
 *     calling thread; no entry point aborts the process;
 *   - activations are channels-last: 2-D maps [N,H,W,C], 3-D grids [N,D,H,W,C], token lists [rows,C];
 *     a row stride `ld*` (in elements) lets a call read/write a column slice of a wider buffer;
 *   - re-entrant and thread-safe: no global mutable state besides the thread-local error string.
 */
#ifndef SWINVOX_HIP_H
#define SWINVOX_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SV_OK 0
#define SV_ERR_INVALID (-1)
#define SV_ERR_LAUNCH (-2)

enum { SV_ACT_NONE = 0, SV_ACT_RELU = 1, SV_ACT_GELU = 2, SV_ACT_LRELU = 3 };
#define SV_BN_SLOTS 16 /* BatchNorm statistic accumulators are [SV_BN_SLOTS][2*C] doubles (contention spreading) */
enum { SV_MATH_F32 = 0, SV_MATH_BF16 = 1, SV_MATH_FP8 = 2, SV_MATH_FP8_FULL = 3 }; /* MFMA input type of the contraction kernels;
   accumulation stays fp32.  SV_MATH_FP8 and SV_MATH_FP8_FULL are accepted by sv_window_attention_fwd and sv_window_attention_bwd only.
   SV_MATH_FP8 (OCP e4m3, per-tile scales): QK^T and PV of the forward (BASELINE configuration 5); sv_window_attention_bwd treats it as
   SV_MATH_BF16.  SV_MATH_FP8_FULL: the forward is exactly SV_MATH_FP8's; the backward is the gradient of that forward (quantisers
   straight-through) with all five contractions on e4m3 operands and per-tile scales. */
/* Storage type of ACTIVATIONS (and activation gradients) in HBM.  Entry points with an `act_dtype` argument take their
 * activation tensors as void*: every such tensor of one call has this element type.  Parameters, parameter gradients,
 * statistics (mean/rstd/scale/shift/sums), workspaces and drop-path scales are always fp32 (or double where noted).
 * Arithmetic is fp32 in both cases; SV_BF16 halves the HBM traffic of the path (values are rounded to nearest-even on store). */
enum { SV_F32 = 0, SV_BF16 = 1 };

const char* sv_last_error(void);
int sv_version(void);

/* ------------------------------------------------------------------------------------------------
 * Contraction engine (implicit GEMM on MFMA): stands in for nn.Linear / nn.Conv2d / nn.Conv3d /
 * nn.ConvTranspose3d forward, data-gradient and weight-gradient.  Reference call sites:
 * timm Linear layers behind models/swin_transformer.py:78; models/encoder.py:22-23,36,41-111;
 * models/cross_view_attention.py:38,46,49-53; models/decoder.py:24-46; models/merger.py:20-54;
 * models/refiner.py:21-70.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sv_geom {
  int N;              /* images (or rows for a Linear: N = rows, all grids 1x1x1) */
  int Di, Hi, Wi;     /* grid of the GATHERED tensor  */
  int Do, Ho, Wo;     /* grid of the PRODUCED tensor  */
  int Ci, Co;         /* channels of gathered / produced tensor (in-memory, i.e. including padding) */
  int kd, kh, kw;     /* kernel extent */
  int sd, sh, sw;     /* stride */
  int pd, ph, pw;     /* padding */
  int ldi;            /* element stride between consecutive positions of the gathered tensor (>= Ci) */
} sv_geom;

typedef struct sv_epilogue {
  const float* bias;     /* [Co] or NULL */
  const void* residual;  /* ACTIVATION (act_dtype): same positions as the output, row stride ldr, or NULL:  out = residual + scale*val */
  int ldr;
  const float* row_scale; /* optional per-image scale of val before the residual add (drop-path), index = row / rows_per_scale */
  int rows_per_scale;
  void* pre_act;         /* ACTIVATION (act_dtype), optional: receives val (after bias, before activation), same layout as out */
  double* stats;         /* optional [SV_BN_SLOTS][2*Co] DOUBLES: atomically accumulates sum and sum-of-squares of the stored output per channel */
  int act;               /* SV_ACT_* applied to val (after bias) */
  float slope;           /* LeakyReLU slope */
  const void* act_grad_src; /* ACTIVATION (act_dtype), optional: val *= act'(act_grad_src[pos]) (backward through an activation), layout of out */
  int act_grad_kind;     /* SV_ACT_* of that activation */
  int ldc;               /* output row stride (elements) */
  int col_off;           /* first output column */
} sv_epilogue;

/* w_packed: [Co][taps][Ci] produced by sv_pack_weight(s); fp32 with act_dtype = SV_F32, bf16 with act_dtype = SV_BF16.
 * gather form:  out[o, co] = sum_{tap,ci} in[o*s - p + tap, ci] * w[co, tap, ci]      (conv forward; tconv data-grad; Linear) */
int sv_conv_gather(const void* in, const void* w_packed, void* out, const sv_geom* g, const sv_epilogue* e,
                   int math, int act_dtype, void* stream);
/* Halo-tile kernels behind sv_conv_gather / sv_tconv_gather (bf16 storage + bf16 MFMA, plain store with optional statistics): 3 x 3 / stride 1 /
 * padding 1 with Ci = Co = 64 (forward and data gradient) and the 4 x 4 / pads (2, 1) ResNet stem on the space-to-depth image (Ci = 16, Co = 64)
 * keep the weights in LDS and read each input patch once instead of once per tap.  mode 0: off, 1 (default; SV_CONV_HALO in the environment):
 * calls of >= 256 tiles of 8 x 32 positions, 2: every call of those shapes.  Results differ from the gather engine's only in fp32 summation order. */
int sv_set_conv_halo(int mode);
int sv_conv_halo_mode(void);
int sv_set_conv_halo_wgrad(int mode); /* the same switch for the halo-tile WEIGHT gradient of the 3 x 3 / stride 1 convolutions with 64 k channels on both
                                         sides behind sv_conv_wgrad (SV_CONV_HALO_WGRAD; 1 = calls of >= 4 tiles per split) */
long long sv_conv_halo_launches(void); /* calls taken by the halo-tile kernels so far in this process (tests: the path they mean to exercise) */
/* Launch plans: which kernel, tile, operand variant and grid sv_conv_gather / sv_tconv_gather / sv_conv_wgrad give a call.  The entry points
 * launch what the same pure host functions plan, so a caller (tests: the path they mean to exercise) can name the path of a shape without
 * running it; the queries make no GPU call and look at the pointers for their alignment only.  They report the plan for the current halo
 * modes (sv_set_conv_halo, sv_set_conv_halo_wgrad) and the environment switches, with the scheduler counters of the wide and halo kernels
 * available (a launch that cannot get a counter slot runs the plan without those paths). */
enum { SV_PATH_GATHER = 0,               /* igemm_kernel: gathers k = (tap, ci) on the fly; grid_y = parity classes of a transposed gather */
       SV_PATH_DENSE = 1,                /* gemm_dense_kernel: Linear / 1x1 stride-1 layers with bf16 storage, persistent workgroups */
       SV_PATH_WIDE = 2,                 /* gemm_wide_kernel (256 x 128 tile, LDS-DMA ring), bias / activation / statistics epilogue */
       SV_PATH_WIDE_GENERAL = 3,         /* the same with a residual or an activation-gradient source */
       SV_PATH_HALO0 = 4, SV_PATH_HALO1 = 5, SV_PATH_HALO2 = 6,               /* resident-weights halo kernels: 3 x 3 / 64 -> 64, stem, stem data gradient */
       SV_PATH_HALO_BLOCKED_8X32 = 7, SV_PATH_HALO_BLOCKED_16X16 = 8,         /* 3 x 3 halo kernel with blocks of 64 channels, by tile shape */
       SV_PATH_WGRAD_TILED = 9,          /* wgrad_kernel, position splits along the grid */
       SV_PATH_WGRAD_WIDE = 10, SV_PATH_WGRAD_WIDE_SWAP = 11,                 /* wgrad_wide_kernel; SWAP: the 256-side of the tile runs over Ci */
       SV_PATH_WGRAD_HALO = 12 };        /* halo-tile weight gradient of the 3 x 3 convolutions */
enum { SV_OPERANDS_F32 = 0, SV_OPERANDS_BF16_F32 = 1, SV_OPERANDS_BF16 = 2 }; /* fp32 MFMA; bf16 MFMA on fp32 storage; bf16 MFMA on bf16 storage */
typedef struct sv_launch_plan {
  int path;                  /* SV_PATH_* */
  int tile_rows, tile_cols;  /* output tile of a workgroup: rows x columns (halo paths: tile height x width in positions) */
  int operands;              /* SV_OPERANDS_* */
  int vec;                   /* elements per operand load: 4, or 8 (16 bytes of bf16) */
  int grid_x, grid_y, block; /* launch geometry */
} sv_launch_plan;
/* transposed = 0: the plan of sv_conv_gather, 1: of sv_tconv_gather (the layers of models/encoder.py:22-23,36,41-111 and the other call sites
 * above).  Returns what the entry point returns for these arguments up to its launch: 0, or SV_ERR_INVALID for what it refuses. */
int sv_conv_gather_plan(const void* in, const void* w, void* out, const sv_geom* g, const sv_epilogue* e, int math, int act_dtype, int transposed,
                        sv_launch_plan* plan);
/* 1 when the plan of sv_conv_gather for this call is SV_PATH_WIDE or SV_PATH_WIDE_GENERAL (Linear / 1x1 layers with bf16 storage, K % 64 == 0,
 * K >= 192, Co >= 128, 8-aligned rows and >= 256 tiles), else 0.  SV_GEMM_WIDE=0 in the environment disables the path. */
int sv_conv_gather_is_wide(const void* in, const void* w, void* out, const sv_geom* g, const sv_epilogue* e, int math, int act_dtype);
/* scatter-as-gather form: out[o, co] = sum_{tap,ci : (o+p-tap)%s==0} in[(o+p-tap)/s, ci] * w[co, tap, ci]
 * (transposed-conv forward; strided-conv data-grad), decomposed per output parity class            */
int sv_tconv_gather(const void* in, const void* w_packed, void* out, const sv_geom* g, const sv_epilogue* e,
                    int math, int act_dtype, void* stream);
/* The plan of sv_conv_wgrad for these arguments (weight gradient of the layers of models/encoder.py:22-23,36,41-111 and the other call sites
 * above; see sv_launch_plan): SV_PATH_WGRAD_*; tile_rows x tile_cols = anchor channels x (tap, gathered channel) columns of a workgroup's
 * tile of dW, 256 x 128 on the wide path. */
int sv_conv_wgrad_plan(const void* anchor, int lda, const void* gathered, const sv_geom* g, int cg_valid, int math, int act_dtype,
                       sv_launch_plan* plan);
/* 1 when that plan is SV_PATH_WGRAD_WIDE or SV_PATH_WGRAD_WIDE_SWAP (256 x 128 tile of dW, LDS-DMA ring fed by producer waves: Linear / 1x1
 * stride-1 layers with bf16 storage, rows % 64 == 0 and >= 16384, >= 128 8-aligned columns on both sides, at most 256 tiles), else 0.
 * SV_WGRAD_WIDE=0 in the environment disables the path.  Shapes of more than 256 tiles (e.g. Co = 896, Ci = 9344) always ran the tiled kernel;
 * since the query is taken from the plan it answers 0 for them, where it used to answer 1. */
int sv_conv_wgrad_is_wide(const void* anchor, int lda, const void* gathered, const sv_geom* g, int cg_valid, int math, int act_dtype);
/* weight gradient: dw[ca, cg, tap] += sum_r anchor[r, ca] * gathered[r*s - p + tap, cg]   (fp32 atomics; dw pre-zeroed
 * or holding a running sum).  g->Do.. = anchor grid, g->Di.. = gathered grid, g->Co = anchor channels (row stride lda),
 * g->Ci = gathered channels (stride g->ldi); only cg < cg_valid is written; dw index = (ca*cg_valid + cg)*taps + tap.
 * When the kernel has more than one tap the partial sums are gathered in `workspace`
 * (sv_conv_wgrad_workspace_floats(g) floats, caller-owned, contents destroyed) and folded into dw by a second kernel. */
size_t sv_conv_wgrad_workspace_floats(const sv_geom* g);
int sv_conv_wgrad(const void* anchor, int lda, const void* gathered, float* dw, const sv_geom* g, int cg_valid,
                  float* workspace, float* dbias /* optional: dbias[ca] += sum_r anchor[r, ca] */, int math, int act_dtype,
                  void* stream);
/* fp8 forward of the Swin Linear layers (timm Linear behind models/swin_transformer.py:78: qkv, proj, fc1, fc2, patch-merge reduction) on the
 * block-scaled K = 128 MFMA.  Recipe for y = x W^T, x [M, K], W [N, K]: row scales s = 224 / max|row| in fp32 (all-zero row: 1; clamped to
 * at most 2^60), operands e4m3_rne(row * s) (OCP e4m3fn) in rows of Kp = roundup(K, 128) bytes with zero padding, fp32 accumulation with both
 * hardware block scales 1.0, val = acc / (sx[m] * sw[n]) in fp32, then the sv_epilogue arithmetic on val.
 * The row quantiser (timm Linear behind models/swin_transformer.py:78, operand preparation): src [rows, K] with row stride ld (elements of src_dtype,
 * SV_F32 or SV_BF16) -> dst_q [rows, Kp] bytes (16-byte aligned, Kp % 128 == 0, bytes K .. Kp-1 zero) and scales [rows]. */
int sv_quant_rows_e4m3(const void* src, int src_dtype, int rows, int K, int ld, void* dst_q, int Kp, float* scales, void* stream);
/* out[m, n] = epilogue(sum_k xq[m, k] wq[n, k] / (sx[m] sw[n])) (timm Linear behind models/swin_transformer.py:78).  xq [M, Kp], wq [N, Kp] from the row
 * quantiser with Kp = roundup(K, 128); out, e->residual and e->pre_act hold act_dtype elements.  Epilogue forms served: bias, act = SV_ACT_NONE or
 * SV_ACT_GELU with pre_act, residual / ldr with row_scale / rows_per_scale, ldc.  stats, act_grad_src, other activations and col_off != 0 are
 * refused with SV_ERR_INVALID.  GELU is the erf form with SV_F32 storage and the engine's fast form with SV_BF16 storage. */
int sv_linear_fp8(const void* xq, const float* sx, const void* wq, const float* sw, void* out, int M, int K, int N, const sv_epilogue* e,
                  int act_dtype, void* stream);
/* 1 when the fp8 linear serves this call (timm Linear behind models/swin_transformer.py:78): math == SV_MATH_BF16 and an epilogue form listed above; else 0 */
int sv_linear_fp8_supported(int K, int N, const sv_epilogue* e, int math, int act_dtype);
long long sv_linear_fp8_launches(void); /* fp8 linear launches so far in this process (timm Linear behind models/swin_transformer.py:78; tests: the path they mean to exercise) */
/* fp8 BACKWARD of the same Linear layers (timm Linear behind models/swin_transformer.py:78; autograd of F.linear), constants and rounding of the
 * forward recipe, all operands e4m3, quantisers straight-through.
 * The column quantiser (timm Linear behind models/swin_transformer.py:78, operand preparation of the backward): src [M, C] with row stride ld (SV_F32 or
 * SV_BF16 elements) -> dst_q [C][Mp] bytes (the TRANSPOSE, 16-byte aligned, Mp = roundup(M, 128), bytes M .. Mp-1 of every row zero) and
 * scales [C] = 224 / max_m |src[m, c]| (all-zero column: 1; at most 2^60).  colsum (optional, [C] fp32): colsum[c] += sum_m src[m, c], the bias
 * gradient, from the unquantised values.  On the [N, K] fp32 weight it yields the [K][Np] operand of the data gradient. */
int sv_quant_cols_e4m3(const void* src, int src_dtype, int M, int C, int ld, void* dst_q, int Mp, float* scales, float* colsum, void* stream);
/* data gradient dx[m, k] = sum_n dq[m, n] wtq[k, n] / (sd[m] swt[k]) (timm Linear behind models/swin_transformer.py:78, gradient with respect to the
 * input).  dq [M, Np] / sd [M] from the row quantiser on dy, wtq [K, Np] / swt [K] from the column quantiser on W [N, K], Np = roundup(N, 128); dx and
 * e->act_grad_src hold act_dtype elements with row stride e->ldc.  Epilogue forms served: none, act_grad_src with act_grad_kind = SV_ACT_GELU
 * (erf form with SV_F32 storage, the engine's fast form with SV_BF16 storage), ldc.  Everything else is refused with SV_ERR_INVALID. */
int sv_linear_fp8_dgrad(const void* dq, const float* sd, const void* wtq, const float* swt, void* dx, int M, int N, int K, const sv_epilogue* e,
                        int act_dtype, void* stream);
/* 1 when sv_linear_fp8_dgrad serves this call (timm Linear behind models/swin_transformer.py:78): math == SV_MATH_BF16 and an epilogue form listed above; else 0 */
int sv_linear_fp8_dgrad_supported(int N, int K, const sv_epilogue* e, int math, int act_dtype);
/* weight gradient dw[n * ldw + k] += sum_m dyt[n, m] xt[k, m] / (sdc[n] sxc[k]) (timm Linear behind models/swin_transformer.py:78, gradient with respect
 * to the weight; fp32 atomics).  dyt [N, Mp] / sdc [N] and xt [K, Mp] / sxc [K] from the column quantiser on dy [M, N] and x [M, K].  The contraction
 * over the tokens is shared among `splits` workgroups per 128 x 128 tile of dw (at most one per 128 tokens); 0 = as many as give two workgroups
 * to each of 256 CUs. */
int sv_linear_fp8_wgrad(const void* dyt, const float* sdc, const void* xt, const float* sxc, float* dw, int M, int N, int K, int ldw, int splits,
                        void* stream);
long long sv_linear_fp8_bwd_launches(int which); /* launches so far of sv_linear_fp8_dgrad (which = 0) / sv_linear_fp8_wgrad (1) (timm Linear behind models/swin_transformer.py:78; tests: the path they mean to exercise); sv_linear_fp8_launches counts neither */
/* MX form of the fp8 forward of the same Linear layers (timm Linear behind models/swin_transformer.py:78), opt-in.  Operands: rows of
 * Kp = roundup(K, 128) OCP e4m3fn bytes and one E8M0 byte per 32-byte block, [rows][Kp / 32] uint8.  Block scale: amax of the 32 stored values
 * = m 2^e, m in [1, 2): E = e - 8 + (m > 1.75) = ceil(log2(amax / 448)) clamped to [-127, 127], byte = E + 127 (all-zero block: 127; 255 never);
 * elements e4m3_rne(ldexpf(x, -E)), so nothing saturates; bytes K .. Kp-1 zero, blocks wholly in the padding carry 127.  The MFMA applies both
 * operands' block scales in hardware: val = acc, no division.
 * The MX row quantiser (timm Linear behind models/swin_transformer.py:78, operand preparation; the definition every producer equals): src [rows, K] with
 * row stride ld (SV_F32 or SV_BF16) -> dst_q [rows, Kp] (16-byte aligned, Kp == roundup(K, 128)) and scales_u8 [rows, Kp / 32] (4-byte aligned). */
int sv_quant_rows_mx_e4m3(const void* src, int src_dtype, int rows, int K, int ld, void* dst_q, int Kp, void* scales_u8, void* stream);
/* out[m, n] = epilogue(sum_k 2^(xs + ws - 254) xq[m, k] wq[n, k]) (timm Linear behind models/swin_transformer.py:78).  xq / xs, wq / ws from the MX row
 * quantiser; epilogue forms and refusals are sv_linear_fp8's (sv_linear_fp8_supported answers for both).  q_out [M, N] / qs_out [M, N / 32]
 * (optional, both or neither): the MX rows of the STORED output (after the activation, rounded to act_dtype), equal to the MX row quantiser on out -
 * the operand of the next linear.  Refused with SV_ERR_INVALID unless N % 128 == 0, and with a residual.  With q_out given, out may be NULL: the
 * MX rows are written, and e->pre_act when it is given in front of an activation (bit-identical to the call that also stores out) - what a backward
 * on stored MX rows reads.  pre_act without out and without an activation (it would be out itself) is refused with SV_ERR_INVALID. */
int sv_linear_mxfp8(const void* xq, const void* xs, const void* wq, const void* ws, void* out, int M, int K, int N, const sv_epilogue* e,
                    void* q_out, void* qs_out, int act_dtype, void* stream);
long long sv_linear_mxfp8_launches(void); /* sv_linear_mxfp8 launches so far in this process (timm Linear behind models/swin_transformer.py:78; tests: the path they mean to exercise) */
long long sv_quant_rows_mx_launches(void); /* sv_quant_rows_mx_e4m3 launches so far in this process (timm Linear behind models/swin_transformer.py:78, operand preparation; tests) */
/* MX form of the fp8 BACKWARD of the same Linear layers (timm Linear behind models/swin_transformer.py:78; autograd of F.linear), opt-in.  The block
 * exponent, the rounding, byte 127 for all-zero and padding blocks, val = acc without clamp or division are the MX forward's; the quantisers are
 * straight-through and read the stored tensors.
 * The MX column quantiser (timm Linear behind models/swin_transformer.py:78, operand preparation of the MX backward), one launch and one read of src:
 * src [M, C] with row stride ld (SV_F32 or SV_BF16) -> dst_q [C][Mp] bytes (the TRANSPOSE, 16-byte aligned, Mp == roundup(M, 128), bytes M .. Mp-1 of
 * every row zero) and scales_u8 [C][Mp / 32] (4-byte aligned; a block = 32 consecutive rows m of one column; blocks wholly past M carry 127), equal
 * bit for bit to sv_quant_rows_mx_e4m3 on the transposed tensor.  colsum (optional, [C] fp32): colsum[c] += sum_m src[m, c] from the unquantised
 * values.  On the [N, K] fp32 weight it yields the [K][Np] operand of the data gradient. */
int sv_quant_cols_mx_e4m3(const void* src, int src_dtype, int M, int C, int ld, void* dst_q, int Mp, void* scales_u8, float* colsum, void* stream);
/* data gradient dx[m, k] = sum_n 2^(ds + wts - 254) dq[m, n] wtq[k, n] (timm Linear behind models/swin_transformer.py:78, gradient with respect to the
 * input).  dq [M, Np] / ds [M, Np / 32] from the MX row quantiser on dy, wtq [K, Np] / wts [K, Np / 32] from the MX column quantiser on W [N, K].
 * Epilogue forms and refusals are exactly sv_linear_fp8_dgrad's (sv_linear_fp8_dgrad_supported answers for both). */
int sv_linear_mxfp8_dgrad(const void* dq, const void* ds, const void* wtq, const void* wts, void* dx, int M, int N, int K, const sv_epilogue* e,
                          int act_dtype, void* stream);
/* floats of the workspace sv_linear_mxfp8_wgrad needs for this call (timm Linear behind models/swin_transformer.py:78): resulting splits * N * K, and 0
 * when one split results (no workspace is read then). */
size_t sv_linear_mxfp8_wgrad_workspace_floats(int M, int N, int K, int splits);
/* weight gradient dw[n * ldw + k] += sum_m 2^(dys + xs - 254) dyt[n, m] xt[k, m] (timm Linear behind models/swin_transformer.py:78, gradient with
 * respect to the weight), WITHOUT atomics: dw is bit-identical from run to run for a given `splits`.  dyt [N, Mp] / dys [N, Mp / 32] and xt [K, Mp] /
 * xs [K, Mp / 32] from the MX column quantiser on dy [M, N] and x [M, K].  The contraction over the tokens is shared among `splits` workgroups per
 * 128 x 128 tile of dw (at most one per 128 tokens; 0 = as many as give two workgroups to each of 256 CUs).  One resulting split adds into dw
 * directly; more write fp32 partials into `workspace` (16-byte aligned, caller-owned, contents destroyed, stale contents never read) and a second
 * kernel adds them to dw in ascending order.  SV_ERR_INVALID: more than one resulting split with a NULL workspace. */
int sv_linear_mxfp8_wgrad(const void* dyt, const void* dys, const void* xt, const void* xs, float* dw, int M, int N, int K, int ldw, int splits,
                          float* workspace, void* stream);
long long sv_linear_mxfp8_bwd_launches(int which); /* launches so far of sv_linear_mxfp8_dgrad (which = 0) / sv_linear_mxfp8_wgrad (1) (timm Linear behind models/swin_transformer.py:78; tests: the path they mean to exercise); the row recipe's counters do not move */
long long sv_quant_cols_mx_launches(void); /* sv_quant_cols_mx_e4m3 launches so far in this process (timm Linear behind models/swin_transformer.py:78, operand preparation; tests) */
/* MX re-blocker (timm Linear behind models/swin_transformer.py:78, operand preparation of the MX weight gradient from stored MX rows), one launch, xq
 * and xs each read once: the MX rows of a stored tensor, xq [M, Kp] e4m3 bytes (16-byte aligned, Kp == roundup(K, 128)) and xs [M, Kp / 32] E8M0 bytes
 * (4-byte aligned), become the column operand dst_q [K][Mp] (16-byte aligned, Mp == roundup(M, 128), bytes M .. Mp-1 of every row zero) and scales_u8
 * [K][Mp / 32] (4-byte aligned; a block = 32 consecutive tokens of one column, blocks wholly past M carry 127).  Definition: the output equals the MX
 * column quantiser applied to the fp32 tensor byte 2^(s - 127) (an exact decode), columns 0 .. K-1, bit for bit; columns K .. Kp-1 of xq do not
 * influence it.  SV_ERR_INVALID before any GPU call: a NULL pointer, M < 1 or K < 1, Kp != roundup(K, 128), Mp != roundup(M, 128), misalignment,
 * Mp / 128 > 65535 (the grid's limit: M above 8 388 480 tokens). */
int sv_mx_rows_to_cols(const void* xq, int Kp, const void* xs, int M, int K, void* dst_q, int Mp, void* scales_u8, void* stream);
long long sv_mx_rows_to_cols_launches(void); /* sv_mx_rows_to_cols launches so far in this process (timm Linear behind models/swin_transformer.py:78, operand preparation; tests) */
/* MX dual quantiser (timm Linear behind models/swin_transformer.py:78, operand preparation of the MX backward: the upstream gradient feeds the data
 * gradient as MX rows and the weight gradient as MX columns), one launch and one read of src [M, N] (row stride ld, SV_F32 or SV_BF16):
 * row_q [M, Np] / row_s [M, Np / 32] (Np == roundup(N, 128)) equal sv_quant_rows_mx_e4m3's output and col_q [N][Mp] / col_s [N][Mp / 32]
 * (Mp == roundup(M, 128)) equal sv_quant_cols_mx_e4m3's, bit for bit for finite inputs, paddings included; colsum (optional, [N] fp32) as in
 * sv_quant_cols_mx_e4m3.  row_q and row_s may be NULL together: the column form alone.  SV_ERR_INVALID before any GPU call: NULL src, col_q or col_s;
 * exactly one of row_q / row_s NULL; a bad src_dtype; M < 1, N < 1 or ld < N; Np != roundup(N, 128) (also without the row pair) or
 * Mp != roundup(M, 128); row_q / col_q not 16-byte or row_s / col_s not 4-byte aligned; Mp / 128 > 65535. */
int sv_quant_rows_cols_mx_e4m3(const void* src, int src_dtype, int M, int N, int ld, void* row_q, int Np, void* row_s, void* col_q, int Mp,
                               void* col_s, float* colsum, void* stream);
long long sv_quant_rows_cols_mx_launches(void); /* sv_quant_rows_cols_mx_e4m3 launches so far in this process (timm Linear behind models/swin_transformer.py:78, operand preparation; tests) */
/* LDS-halo MFMA stencils for 3x3x3 / stride 1 / pad 1 convolutions with <= 16 output channels per tile (merger.py:20-54),
 * bf16 operands.  x: channels-last positions with row stride ldx, cin_load (multiple of 4) elements read per position,
 * zero-extended to 16*groups channels; w_bf16: [16*ntiles16][27][16*groups] bf16 (forward: rows = output channels;
 * data-gradient: rows = input channels, taps flipped).  Writes out[pos*ldc + col_off + n] for n < cout
 * (= residual[pos*ldr + n] + value when residual != NULL); optional per-channel statistics as in sv_epilogue.stats
 * (ntiles16 == 1 only).  When ldc, col_off (and ldr) are multiples of 4 and the row has room, the columns
 * cout .. roundup4(cout)-1 are treated as PADDING of the row and written too (zero, + residual): 8/16-byte row stores.
 * Persistent kernel: one workgroup walks many 8x8x8 bricks (D % 8 == 0, H % 8 == 0, W % 8 == 0), prefetching the next brick while it contracts the current one.
 * Planar channel storage (the dense per-layer buffers that replace the reference's torch.cat, merger.py:84): with
 * x_plane_stride != 0 memory channel c of the input lives at x[(c / ldx) * x_plane_stride + pos*ldx + c % ldx]; with
 * out_plane_stride != 0 column n goes to out[(n / ldc) * out_plane_stride + pos*ldc + n % ldc] (col_off 0, no residual).
 * Strides in elements, multiples of 4; 0 = interleaved rows (sv_stencil3_wgrad: the same for its gathered operand x). */
int sv_stencil3_fwd(const void* x, int ldx, int cin_load, int groups, const void* w_bf16, int ntiles16,
                    const float* bias, void* out, int ldc, int col_off, int cout, const void* residual, int ldr,
                    double* stats, int I, int D, int H, int W, long long x_plane_stride, long long out_plane_stride, int act_dtype,
                    void* stream);
/* dw[co][ci][27] += sum_vox dy[vox][co] * x[vox + tap][c]; memory channel c maps to ci = (c / c_stride)*c_valid + c % c_stride;
 * optional dbias[co] += sum_vox dy[vox][co].  workspace: NULL (every workgroup adds into dw directly) or
 * sv_stencil3_wgrad_workspace_floats(cout, cin) floats, ZERO on entry: partial sums are spread over slot images and
 * folded into dw by a second small kernel (removes the ~1000-way atomic contention per weight) */
size_t sv_stencil3_wgrad_workspace_floats(int cout, int cin);
int sv_stencil3_wgrad(const void* x, int ldx, int cin_load, int groups, const void* dy, int lddy, int cout_load,
                      float* dw, float* dbias, float* workspace, int cout, int cin, int c_stride, int c_valid, int I, int D, int H, int W,
                      long long x_plane_stride, int act_dtype, void* stream);
/* ConvTranspose3d(kernel 4, stride 2, padding 1), 32 input channels -> 8 output channels (rows of 8 bf16; cout < 8 leaves zero columns),
 * bf16 operands, on an LDS halo brick: the decoder's last up-sampling layer (models/decoder.py:37-40).  x: [I][D][H][W][32];
 * w_packed: the forward pack [cout][64 taps][32] of sv_pack_weight (swap = 1); out: [I][2D][2H][2W][8] = value + bias;
 * stats as in sv_epilogue.stats.  D, H, W must be multiples of 4, 4, 8. */
int sv_tconv4s2_fwd(const void* x, const void* w_packed, const float* bias, void* out, double* stats, int I, int D, int H, int W,
                    int cin, int cout, void* stream);
/* dst[a][t][b] (b padded with zeros to pad_to) from the fp32 parameter src[a][b][t] (swap=0), or dst[b][t][a..pad_to] (swap=1);
 * dst elements are out_dtype (SV_F32 / SV_BF16) */
int sv_pack_weight(const float* src, void* dst, int A, int B, int T, int swap, int pad_to, int out_dtype, void* stream);
/* the same for a whole table of weights in ONE launch.  descs_dev: DEVICE array; rows_out / inner_out as derived by
 * sv_pack_weight (rows_out = swap ? B : A, inner_out = max(pad_to, swap ? A : B)); block0 = exclusive prefix sum of
 * ceil(rows_out*T*inner_out / sv_pack_weights_block_elems()) over the table, total_blocks = its grand total */
typedef struct sv_pack_desc {
  const float* src; void* dst;
  int A, B, T, swap, rows_out, inner_out, block0, reserved;
} sv_pack_desc;
int sv_pack_weights_block_elems(void);
int sv_pack_weights(const sv_pack_desc* descs_dev, int n, int total_blocks, int out_dtype, void* stream);
/* per-column sum over rows: out[c] (+)= sum_r x[r*ld + c]  (bias gradients) */
int sv_colsum(const void* x, int rows, int cols, int ld, float* out, int accumulate, int act_dtype, void* stream);
/* element-wise storage conversion (module boundaries: nn.Module inputs / outputs are fp32) */
int sv_cast(const void* src, int src_dtype, void* dst, int dst_dtype, long long n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Normalisation.  Token LayerNorm = timm norm1/norm2/patch_embed.norm/downsample.norm (eps 1e-5); with
 * merge_H/merge_W > 0 the rows are the PatchMerging 2x2 gather (order h0w0,h1w0,h0w1,h1w1) of a
 * [I,merge_H,merge_W,C/4] map.  Image LayerNorm = nn.LayerNorm([C,H,W]) + Dropout(0.05) of
 * models/swin_transformer.py:64-69,82-89 on NHWC data with the affine pre-transposed to [HW,C].
 * BatchNorm = nn.BatchNorm2d/3d of models/encoder.py, cross_view_attention.py:56, decoder.py, merger.py,
 * refiner.py on channels-last [M,C] (biased batch variance, unbiased running update, eps 1e-5).
 * x / y / dx / dy / z / dz / residual / dres are activations (act_dtype); everything else is fp32 (double where declared).
 * ---------------------------------------------------------------------------------------------- */
int sv_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                     long long rows, int C, float eps, int merge_H, int merge_W, int act_dtype, void* stream);
/* sv_layernorm_fwd that also emits the operand rows sv_linear_fp8 reads (timm LayerNorm -> Linear behind
 * models/swin_transformer.py:78): q [rows, Kp] e4m3 bytes (16-byte aligned), Kp = roundup(C, 128), zeros past C; scales [rows] =
 * sv_quant_rows_e4m3's scale of the STORED row (the row rounded to act_dtype first), so q and scales equal that quantiser's output on y
 * bit for bit.  y may be NULL (the rows are then not stored: inference); mean and rstd may be NULL together.  Refused with SV_ERR_INVALID:
 * what sv_layernorm_fwd refuses, q or scales NULL, Kp != roundup(C, 128), exactly one of mean / rstd NULL. */
int sv_layernorm_quant_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                           void* q, int Kp, float* scales, long long rows, int C, float eps, int merge_H, int merge_W,
                           int act_dtype, void* stream);
long long sv_layernorm_quant_launches(void); /* sv_layernorm_quant_fwd launches so far in this process (timm LayerNorm -> Linear behind models/swin_transformer.py:78; tests: the path they mean to exercise) */
/* sv_layernorm_fwd that also emits the MX operand rows sv_linear_mxfp8 reads (timm LayerNorm -> Linear behind
 * models/swin_transformer.py:78): q [rows, Kp] e4m3 bytes (16-byte aligned), Kp = roundup(C, 128), zeros past C; scales_u8 [rows, Kp / 32]
 * E8M0 bytes (4-byte aligned), 127 for a block that is all zero or lies in the padding.  Both equal sv_quant_rows_mx_e4m3's output on the
 * STORED y (the row rounded to act_dtype first) bit for bit.  y may be NULL (the rows are then not stored: inference); mean and rstd may be
 * NULL together.  Refused with SV_ERR_INVALID before any GPU call: what sv_layernorm_fwd refuses, q or scales_u8 NULL, Kp != roundup(C, 128),
 * exactly one of mean / rstd NULL, q not 16-byte or scales_u8 not 4-byte aligned. */
int sv_layernorm_quant_mx_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                              void* q, int Kp, void* scales_u8, long long rows, int C, float eps,
                              int merge_H, int merge_W, int act_dtype, void* stream);
long long sv_layernorm_quant_mx_launches(void); /* sv_layernorm_quant_mx_fwd launches so far in this process (timm LayerNorm -> Linear behind models/swin_transformer.py:78; sv_layernorm_quant_launches does not count them) */
/* workspace: sv_layernorm_bwd_workspace_floats(C) floats, ZERO on entry (slot-spread dgamma/dbeta partial sums + ticket) */
size_t sv_layernorm_bwd_workspace_floats(int C);
int sv_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                     void* dx, float* dgamma, float* dbeta, float* workspace, long long rows, int C, int merge_H, int merge_W,
                     int accumulate_dx, int act_dtype, void* stream);
size_t sv_ln_image_workspace_floats(int I, int L);
int sv_ln_image_fwd(const void* x, const float* w, const float* b, void* y, float* meanrstd, float* workspace,
                    int I, int L, float eps, float drop_p, uint32_t seed, const uint32_t* seed_epoch, int act_dtype, void* stream);
int sv_ln_image_bwd(const void* dy, const void* x, const float* w, const float* meanrstd, void* dx, float* dw,
                    float* db, double* sums_ws /* [2*I] doubles */, int I, int L, float drop_p, uint32_t seed,
                    const uint32_t* seed_epoch, int act_dtype, void* stream);
int sv_bn_stats(const void* x, long long M, int C, int ld, double* sums, int act_dtype, void* stream);   /* sums: [SV_BN_SLOTS][2*C] doubles (slot 0 is used) */
int sv_bn_finalize(const double* sums, long long count, const float* gamma, const float* beta, float* running_mean,
                   float* running_var, float momentum, float eps, int training, float* scale, float* shift,
                   float* save_mean, float* save_rstd, int C, void* stream);
/* Padded rows: when C is not a multiple of 4, C <= 16 and every row stride involved is a multiple of 4 elements and
 * >= roundup4(C), sv_scale_shift_act and sv_bn_bwd treat the columns C .. roundup4(C)-1 as PADDING of the row: whatever they
 * hold on input is ignored (it may be uninitialised memory) and ZERO is written there (y / dx / dres are stored as whole
 * 4-channel vectors).  A 9-channel tensor kept
 * in 12-wide rows therefore never needs a separate zero fill (swinvox_amd/models/merger.py relies on this). */
int sv_scale_shift_act(const void* x, int ldx, const float* scale, const float* shift, const void* residual, int ldr,
                       void* y, int ldy, long long M, int C, int act, float slope, int act_dtype, void* stream);
/* ResNet stem: BatchNorm + activation + MaxPool2d(3, stride 2, padding 1) in one pass over the convolution's output x [N, H, W, C] (rows of exactly C
 * elements, C % 4 == 0, 256 % (C / 4) == 0): pooled / idx [N, (H+1)/2, (W+1)/2, C] (idx: arg-max tap 0..8 per element, first maximum in scan order).
 * The normalised activation is never stored.  sv_bn_maxpool_bwd: gradient of the pooled map -> dx (w.r.t. x) with the pool's backward computed on the
 * fly inside both passes of the BatchNorm backward; dgamma / dbeta +=; sums_ws: sv_bn_bwd_workspace_doubles(C) doubles, zero on entry.
 * Replaces sv_scale_shift_act + sv_maxpool2d_fwd and sv_maxpool2d_bwd + sv_bn_bwd of reference models/encoder.py:22-23 (resnet50 bn1 / relu / maxpool). */
int sv_bn_act_maxpool_fwd(const void* x, const float* scale, const float* shift, void* pooled, void* idx, int N, int H, int W, int C,
                          int act, float slope, int act_dtype, void* stream);
int sv_bn_maxpool_bwd(const void* dpooled, const void* idx, const void* x, const float* gamma, const float* save_mean, const float* save_rstd,
                      const float* fwd_scale, const float* fwd_shift, int N, int H, int W, int C, int act, float slope, int training,
                      void* dx, float* dgamma, float* dbeta, double* sums_ws, int act_dtype, void* stream);
/* The same fusion around MaxPool3d(2) (floor) for the Refiner's down-sampling layers (reference models/refiner.py:21-39): x [N, D, H, W, C] ->
 * pooled / idx [N, D/2, H/2, W/2, C] (tap = 4 dz + 2 dy + dx, as sv_maxpool3d_fwd); the backward writes dx for every input position, the planes of an
 * odd grid that no window covers included. */
int sv_bn_act_maxpool3d_fwd(const void* x, const float* scale, const float* shift, void* pooled, void* idx, int N, int D, int H, int W, int C,
                            int act, float slope, int act_dtype, void* stream);
int sv_bn_maxpool3d_bwd(const void* dpooled, const void* idx, const void* x, const float* gamma, const float* save_mean, const float* save_rstd,
                        const float* fwd_scale, const float* fwd_shift, int N, int D, int H, int W, int C, int act, float slope, int training,
                        void* dx, float* dgamma, float* dbeta, double* sums_ws, int act_dtype, void* stream);
size_t sv_bn_bwd_workspace_doubles(int C);   /* size of sums_ws below */
int sv_bn_bwd(const void* dz, int lddz, const void* z, int ldz, const void* x, int ldx, const float* gamma,
              const float* save_mean, const float* save_rstd, long long M, int C, int act, float slope, int training,
              void* dx, int lddx, void* dres, int lddres, float* dgamma, float* dbeta, double* sums_ws /* sv_bn_bwd_workspace_doubles(C) doubles, ZERO on entry */,
              const float* fwd_scale, const float* fwd_shift /* optional: with z == NULL the activation mask is recomputed as
              x*fwd_scale + fwd_shift > 0 (valid when the forward added no residual) - saves one tensor read per pass */,
              int act_dtype, void* stream);
/* Activation mask as SIGN WORDS instead of the stored output (BatchNorm in front of a residual sum: bn3 and the down-sampling branch of every
 * bottleneck, reference models/encoder.py:22-23): sv_scale_shift_act_signs also writes, per row and per 256 channels, four 64-bit words - bit l of
 * word j = (value of channel 256 b + 4 l + j before the activation) > 0 - i.e. [M][C/64] uint64, 1/16 of the bytes of a bf16 output;
 * sv_bn_bwd_signs takes its mask from them (and always returns the masked gradient dz * act' through dres, which its second pass reads back
 * instead of (dz, z) wherever the stored value is the masked gradient exactly - ReLU, or fp32 storage; with LeakyReLU in bf16 storage the second
 * pass masks dz from the words itself, so that dx does not inherit the rounding of slope * dz).  C % 256 == 0 (sv_bn_signs_supported), rows 4-aligned. */
int sv_bn_signs_supported(int C);
int sv_scale_shift_act_signs(const void* x, int ldx, const float* scale, const float* shift, const void* residual, int ldr, void* y, int ldy,
                             long long M, int C, int act, float slope, void* signs, int act_dtype, void* stream);
int sv_bn_bwd_signs(const void* dz, int lddz, const void* signs, const void* x, int ldx, const float* gamma, const float* save_mean,
                    const float* save_rstd, long long M, int C, int act, float slope, int training, void* dx, int lddx, void* dres, int lddres,
                    float* dgamma, float* dbeta, double* sums_ws, int act_dtype, void* stream);
/* The first bottleneck of a ResNet layer, out = relu(bn3(y3) + bn_d(yd)) (reference models/encoder.py:22-23: torchvision Bottleneck with downsample):
 * both BatchNorms in the same passes.  Train mode, ReLU, C % 256 == 0, every row stride a multiple of 4 and >= C, 4-element aligned tensors; any
 * other case is refused (use the per-layer entry points).
 * sv_scale_shift_act2_signs: y = relu(fma(x3, scale3, shift3) + t), t = fma(xd, scaled, shiftd) rounded to the storage type, and the sign words of
 * the sum - the bytes of sv_scale_shift_act (down-sampling layer, no activation) followed by sv_scale_shift_act_signs (bn3, residual = its output),
 * without the intermediate tensor.
 * sv_bn_bwd2_signs: d = dz * [sign bit] is formed from dz and the words in both passes and never stored; dx3 / dxd = each layer's input gradient
 * (double arithmetic, as sv_bn_bwd); dgamma / dbeta of both layers +=.  sums_ws3 / sums_wsd: sv_bn_bwd_workspace_doubles(C) doubles each, ZERO on
 * entry (two buffers, or the two halves of one). */
int sv_scale_shift_act2_signs(const void* x3, int ldx3, const float* scale3, const float* shift3, const void* xd, int ldxd, const float* scaled,
                              const float* shiftd, void* y, int ldy, long long M, int C, void* signs, int act_dtype, void* stream);
int sv_bn_bwd2_signs(const void* dz, int lddz, const void* signs, const void* x3, int ldx3, const float* gamma3, const float* save_mean3,
                     const float* save_rstd3, const void* xd, int ldxd, const float* gammad, const float* save_meand, const float* save_rstdd,
                     long long M, int C, void* dx3, int lddx3, void* dxd, int lddxd, float* dgamma3, float* dbeta3, float* dgammad, float* dbetad,
                     double* sums_ws3, double* sums_wsd, int act_dtype, void* stream);
/* Launch plans of the token LayerNorm and the per-layer BatchNorm apply / backward (timm norm1 / norm2 behind models/swin_transformer.py:78;
 * nn.BatchNorm2d/3d of models/encoder.py:22-23 and the other call sites above): which kernel family, access width and grids a call gets.  The
 * entry points launch what the same pure host functions plan, so a caller (tests: the path they mean to exercise) can name the path of a
 * shape without running it; the queries make no GPU call and look at the pointers for NULL and for their alignment only. */
enum { SV_NORM_LN_FWD = 0,               /* ln_fwd_kernel (plain, row-quantising or MX: one geometry) */
       SV_NORM_LN_BWD = 1,               /* ln_bwd_kernel, then ln_bwd_fold_kernel */
       SV_NORM_BN_SCALAR = 2,            /* one element per access: any C, row stride and alignment */
       SV_NORM_BN_NARROW = 3,            /* padded rows: C <= 16, row strides multiples of 4 and >= roundup4(C), 4-element aligned tensors */
       SV_NORM_BN_VECTOR = 4 };          /* C % 4 == 0, row strides multiples of 4, 4-element aligned tensors, 16-byte aligned fp32 vectors */
enum { SV_MASK_PLAIN = 0,                /* the apply pass of sv_bn_bwd masks dz itself: from z, or from x and the forward scale / shift */
       SV_MASK_PREMASK = 1,              /* the reduce pass stores the masked gradient in dres, the apply pass reads it back mask-free */
       SV_MASK_SIGN_APPLY = 2 };         /* the reduce pass stores dres, the apply pass masks dz from the sign words */
typedef struct sv_norm_plan {
  int family;                /* SV_NORM_* */
  int merge;                 /* LayerNorm: 1 = the rows are the PatchMerging gather */
  int storage;               /* SV_F32 / SV_BF16: element type the kernels are instantiated for */
  int vec;                   /* elements per access: 4, or 8 (16 bytes of bf16); 1 in SV_NORM_BN_SCALAR */
  int lanes;                 /* LayerNorm: lanes per row (16 / 32 / 64); BatchNorm: lanes across a row (SV_NORM_BN_VECTOR: 4 channels each), else 0 */
  int nv;                    /* LayerNorm: chunks of `vec` elements per lane (1, 2, 3, 4, 6, 12) */
  int mask;                  /* sv_bn_bwd: SV_MASK_* */
  int launches;              /* entries of `launch` in use, in dispatch order (backward: reduce, fold, apply; LayerNorm backward: rows, fold) */
  struct { int grid_x, grid_y, block, lds_bytes; } launch[3];
  long long rows[2];         /* rows per workgroup of launch 0 (SV_NORM_BN_NARROW backward: per thread) and of the SV_NORM_BN_VECTOR apply launch;
                                0 where the workgroups stride over the rows */
} sv_norm_plan;
/* kind 0: the plan of sv_layernorm_fwd, 1: of sv_layernorm_quant_fwd, 2: of sv_layernorm_quant_mx_fwd (a = x, b = y, c ignored), 3: of
 * sv_layernorm_bwd (a = dy, b = x, c = dx) (timm LayerNorm behind models/swin_transformer.py:78).  Returns 0, or SV_ERR_INVALID with the
 * entry's message for what the entry refuses about these arguments (rows, C, the merge map, act_dtype, a NULL x / dy / dx). */
int sv_layernorm_plan(int kind, const void* a, const void* b, const void* c, long long rows, int C, int merge_H, int merge_W, int act_dtype,
                      sv_norm_plan* plan);
/* The plan of sv_scale_shift_act (signs == NULL) / sv_scale_shift_act_signs for these arguments (nn.BatchNorm2d/3d apply of
 * models/encoder.py:22-23 and the other call sites above).  Returns what the entry point returns up to its launch. */
int sv_scale_shift_act_plan(const void* x, int ldx, const float* scale, const float* shift, const void* residual, int ldr, void* y, int ldy,
                            long long M, int C, int act, float slope, void* signs, int act_dtype, sv_norm_plan* plan);
/* The plan of sv_bn_bwd (signs == NULL) / sv_bn_bwd_signs (z, fwd_scale, fwd_shift NULL) for these arguments (autograd of nn.BatchNorm2d/3d,
 * models/encoder.py:22-23 and the other call sites above).  Returns what the entry point returns up to its launch. */
int sv_bn_bwd_plan(const void* dz, int lddz, const void* z, int ldz, const void* signs, const void* x, int ldx, const float* gamma,
                   const float* save_mean, const float* save_rstd, long long M, int C, int act, float slope, int training, void* dx, int lddx,
                   void* dres, int lddres, float* dgamma, float* dbeta, double* sums_ws, const float* fwd_scale, const float* fwd_shift,
                   int act_dtype, sv_norm_plan* plan);

/* ------------------------------------------------------------------------------------------------
 * Attention cores.  Window attention = timm WindowAttention + SwinTransformerBlock roll/partition/mask
 * (call site models/swin_transformer.py:78): qkv [I*H*W, 3C] rows in natural (h,w) order, columns
 * [q|k|v][head][32]; table [169, heads] (fp32 parameter); out [I*H*W, C].  Cross-view attention = models/
 * cross_view_attention.py:78-105: qkv [B*V*P, 3R] channels-last rows (view image, position), scores over
 * the V views of one sample scaled by 1/sqrt(head_dim*V).  qkv / out / dout / dqkv are activations (act_dtype;
 * SV_BF16 requires math = SV_MATH_BF16); softmax statistics and the bias-table gradient stay fp32.
 * ---------------------------------------------------------------------------------------------- */
int sv_window_attention_fwd(const void* qkv, const float* table, void* out, int I, int H, int W, int C, int heads,
                            int shift, int math, int act_dtype, void* stream);
/* workspace: NULL, or sv_window_attention_bwd_workspace_floats(heads) floats, ZERO on entry (slot images of dtable, folded
 * by a second small kernel; used by the bf16-MFMA kernels) */
size_t sv_window_attention_bwd_workspace_floats(int heads);
int sv_window_attention_bwd(const void* qkv, const float* table, const void* dout, void* dqkv, float* dtable, float* workspace,
                            int I, int H, int W, int C, int heads, int shift, int math, int act_dtype, void* stream);
/* sv_window_attention_fwd that also emits the MX operand rows of the Linear that follows (timm WindowAttention -> proj Linear behind
 * models/swin_transformer.py:78; recipe: sv_quant_rows_mx_e4m3): q_out [tokens, Kp] e4m3 bytes and qs_out [tokens, Kp / 32] E8M0 bytes of the STORED
 * output, equal to the MX row quantiser on out - one head of one token is one block.  Kp == roundup(C, 128); for Kp > C the kernel writes the
 * zero padding bytes and the scale 127 of the padding blocks itself.  out may be NULL (no backward follows).  Served by the workgroup kernels
 * of SV_MATH_BF16 / SV_MATH_FP8 / SV_MATH_FP8_FULL; SV_MATH_F32 is refused with SV_ERR_INVALID. */
int sv_window_attention_fwd_mxq(const void* qkv, const float* table, void* out, int I, int H, int W, int C, int heads, int shift, int math,
                                void* q_out, int Kp, void* qs_out, int act_dtype, void* stream);
/* Consecutive windows one workgroup (bf16 / fp8 kernels) or one wave (exact-fp32 kernels) walks in the launch sv_window_attention_fwd
 * (backward = 0) / _bwd (backward = 1) makes for these arguments (call site models/swin_transformer.py:78); 1 for the fp32 forward.  A
 * pure host function - the launches take their share from the same place - for tests that mean to run a kernel at several windows per
 * workgroup.  Negative SV_ERR_* for a geometry the entry points refuse, for I or heads < 1, and - the query's own rule - for a math
 * code that is none of SV_MATH_F32 / _BF16 / _FP8 / _FP8_FULL. */
int sv_window_attention_windows_per_group(int I, int H, int W, int heads, int math, int backward);
int sv_cross_view_attention_fwd(const void* qkv, void* out, int B, int V, int P, int R, int heads, int act_dtype, void* stream);
int sv_cross_view_attention_bwd(const void* qkv, const void* dout, void* dqkv, int B, int V, int P, int R, int heads,
                                int act_dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Layout / pooling / tail kernels (reference sites in the comments of csrc/elementwise.hip).  void* tensors are
 * activations (act_dtype); weights, their gradients, pooling indices and drop-path scales keep their declared types.
 * ---------------------------------------------------------------------------------------------- */
int sv_transpose(const void* src, void* dst, int batch, int R, int C, int lds, int ldd, long long src_bstride,
                 long long dst_bstride, int act_dtype, void* stream);                       /* dst[b][c][r] = src[b][r][c] */
int sv_add_n(const void* a, const void* b, const void* c, const void* d, void* out, long long M, int C, int ldo, int act_dtype, void* stream);
int sv_axpby(const void* a, const void* b, void* out, float alpha, float beta, long long n, int act_dtype, void* stream);
int sv_relu_bwd(const void* dy, const void* y, void* out, long long n, int act_dtype, void* stream);               /* refiner.py:51 (ReLU after layer5) */
int sv_maxpool2d_fwd(const void* x, void* y, uint8_t* idx, int N, int H, int W, int C, int act_dtype, void* stream);   /* 3x3 s2 p1, encoder.py:23 (resnet maxpool) */
int sv_maxpool2d_bwd(const void* dy, const uint8_t* idx, void* dx, int N, int H, int W, int C, int act_dtype, void* stream);   /* writes every dx element (no pre-zeroing) */
int sv_avgpool2_fwd(const void* x, void* y, int N, int H, int W, int C, int ldy, int col_off, int act_dtype, void* stream); /* encoder.py:123 */
int sv_avgpool2_bwd(const void* dy, void* dx, int N, int H, int W, int C, int ldy, int col_off, int act_dtype, void* stream);
int sv_decoder_seed_fwd(const void* feat, void* out, int I, int C, int act_dtype, void* stream);                      /* decoder.py:59-67 */
int sv_decoder_seed_bwd(const void* dout, void* dfeat, int I, int C, int act_dtype, void* stream);
int sv_maxpool3d_fwd(const void* x, void* y, uint8_t* idx, int N, int D, int H, int W, int C, int act_dtype, void* stream); /* refiner.py:25,31,37 */
int sv_maxpool3d_bwd(const void* dy, const uint8_t* idx, void* dx, int N, int D, int H, int W, int C, int act_dtype, void* stream);
/* seed_epoch (all stochastic entry points; may be NULL): device word mixed into `seed` on the device, so that launches replayed
 * from a captured hipGraph - whose scalar arguments are frozen - draw fresh masks when the caller advances the word per replay. */
int sv_dropout(const void* x, void* y, long long n, float p, uint32_t seed, const uint32_t* seed_epoch, int act_dtype, void* stream);            /* cross_view_attention.py:57,131 */
int sv_droppath_scale(float* scale, int I, float p, uint32_t seed, const uint32_t* seed_epoch, void* stream);                        /* timm DropPath */
int sv_rowscale(const void* x, const float* scale, void* y, long long rows, int C, int rows_per_scale, int act_dtype, void* stream);
int sv_dwconv2x2_fwd(const void* x, const float* w, const float* b, void* y, int I, int C, int act_dtype, void* stream); /* cross_view_attention.py:26-32,68 */
int sv_dwconv2x2_bwd(const void* dy, const void* x, const float* w, void* dx, float* dw, float* db, int I, int C, int act_dtype, void* stream);
int sv_upsample3to7_add_fwd(const void* small, const void* x, int ldx, void* y, int I, int C, int act_dtype, void* stream); /* cross_view_attention.py:110-120 */
int sv_upsample3to7_bwd(const void* dy, void* dsmall, int I, int C, int act_dtype, void* stream);
/* the same four at ATT_SPATIAL_DOWNSAMPLE_RATIO r in {2, 4, 5, 6, 7}: grid g = (7-r)/r+1 (3x3 at r = 2, 1x1 at r >= 4); weight [C,1,r,r];
 * small / dy of the conv are [I*g*g, C]; every other r (3, <= 1, >= 8) is refused (SV_ERR_INVALID).  The 2x2 / 3to7 entries above are r = 2. */
int sv_cva_downsample_fwd(const void* x, const float* w, const float* b, void* y, int I, int C, int r, int act_dtype, void* stream); /* cross_view_attention.py:26-32,68 */
int sv_cva_downsample_bwd(const void* dy, const void* x, const float* w, void* dx, float* dw, float* db, int I, int C, int r, int act_dtype, void* stream);
int sv_cva_upsample_add_fwd(const void* small, const void* x, int ldx, void* y, int I, int C, int r, int act_dtype, void* stream); /* cross_view_attention.py:110-120 */
int sv_cva_upsample_bwd(const void* dy, void* dsmall, int I, int C, int r, int act_dtype, void* stream);
int sv_decoder_head_fwd(const void* x8, const float* w, const float* bias, void* raw12, void* vol, long long M, int act_dtype, void* stream); /* decoder.py:83-94 */
int sv_decoder_head_bwd(const void* draw12, const void* dvol, const void* x8, const float* w, void* dx8, float* dw, float* dbias,
                        long long M, int act_dtype, void* stream);
int sv_merge_views_fwd(const void* wlogit, const void* vol, void* out, int B, int V, int S, int act_dtype, void* stream);  /* merger.py:91-104 */
int sv_merge_views_bwd(const void* wlogit, const void* vol, const void* out, const void* dout, void* dwlogit, void* dvol,
                       int B, int V, int S, int act_dtype, void* stream);
/* Fused Swin MLP branch  x2 = x1 + s * fc2(GELU(fc1(LayerNorm(x1))))  (timm Mlp + norm2 + DropPath of a SwinTransformerBlock behind
 * models/swin_transformer.py:78) with no hidden activation in HBM: bf16 activations / bf16 MFMA only, C in {96, 128, 192}
 * (sv_swin_mlp_supported).  x1, x2, dx1, dx2: [M, C] bf16 token rows; w1 [4C, C], b1 [4C], w2 [C, 4C], b2 [C], ln_g / ln_b [C]: fp32
 * parameters in their native layouts; row_scale (may be NULL): one drop-path factor per rows_per_scale consecutive rows.
 *  sv_swin_mlp_pack:  w1, w2 -> `packs` (16 C^2 bf16 elements): four images in MFMA fragment order, read by _fwd and _bwd.
 *  sv_swin_mlp_fwd:   x2 from x1.
 *  sv_swin_mlp_bwd:   dx1 = dx2 + d(branch)/dx1, recomputing LayerNorm and the pre-activation; dgamma / dbeta += LayerNorm gradients.
 *  sv_swin_mlp_wgrad: dw1, db1, dw2, db2 += weight gradients, recomputing the hidden activation per hidden-unit chunk;
 *                     w1_rows = bf16 [4C][C] (fc1.weight), w2t_rows = bf16 [4C][C] (fc2.weight transposed).                          */
int sv_swin_mlp_supported(int C);
int sv_swin_mlp_pack(const float* w1, const float* w2, void* packs, int C, void* stream);
int sv_swin_mlp_fwd(const void* x1, void* x2, const float* ln_g, const float* ln_b, const void* packs, const float* b1, const float* b2,
                    const float* row_scale, int rows_per_scale, long long M, int C, float eps, void* stream);
int sv_swin_mlp_bwd(const void* x1, const void* dx2, void* dx1, const float* ln_g, const float* ln_b, const void* packs, const float* b1,
                    const float* row_scale, int rows_per_scale, float* dgamma, float* dbeta, long long M, int C, float eps, void* stream);
int sv_swin_mlp_wgrad(const void* x1, const void* dx2, const float* ln_g, const float* ln_b, const void* w1_rows, const void* w2t_rows,
                      const float* b1, const float* row_scale, int rows_per_scale, float* dw1, float* db1, float* dw2, float* db2,
                      long long M, int C, float eps, void* stream);

/* MXFP8 forward of the fused Swin MLP branch (timm Mlp + norm2 + DropPath of a SwinTransformerBlock behind models/swin_transformer.py:78): the
 * unfused MX chain sv_layernorm_quant_mx_fwd -> sv_linear_mxfp8 (GELU, q_out) -> sv_linear_mxfp8 (residual) composed in ONE kernel, both products
 * on the block-scaled K = 128 MFMA with E8M0 scales per 32 channels / 32 hidden units; neither the hidden activation nor a quantised activation
 * reaches HBM.  bf16 token rows, C in {96, 128}.  The backward is sv_swin_mlp_bwd / sv_swin_mlp_wgrad, unchanged (straight-through quantisers),
 * unless the MX siblings below (sv_swin_mlp_bwd_mx, sv_swin_mlp_wgrad_mx) are asked for.
 *  sv_swin_mlp_mx_supported:  1 for C = 96 and C = 128, else 0 (timm Mlp behind models/swin_transformer.py:78).
 *  sv_swin_mlp_mx_pack_bytes: size of `packs` for C (0 when unsupported) (timm Mlp weights behind models/swin_transformer.py:78).
 *  sv_swin_mlp_mx_pack:       w1q [4C, 128] / w1s [4C, 4] and w2q [C, 4C] / w2s [C, 4C / 32], the MX rows sv_quant_rows_mx_e4m3 makes of fc1.weight and
 *                             fc2.weight (timm Mlp behind models/swin_transformer.py:78), -> `packs` in the kernel's fragment order; w1q, w2q and packs
 *                             16-byte aligned.  The bytes are re-ordered, never re-quantised.
 *  sv_swin_mlp_fwd_mx:        x2 from x1; arguments and alignment rules of sv_swin_mlp_fwd, with packs_mx from sv_swin_mlp_mx_pack (timm Mlp +
 *                             norm2 + DropPath behind models/swin_transformer.py:78).
 *  sv_swin_mlp_mx_launches:   sv_swin_mlp_fwd_mx launches so far in this process (timm Mlp behind models/swin_transformer.py:78; tests: the path they mean
 *                             to exercise).
 * Refusals (SV_ERR_INVALID before any GPU call, the entry's name in sv_last_error()): null pointers, unsupported C, M <= 0 or >= 2^31, misaligned
 * operands, rows_per_scale <= 0.                                                                                                              */
int sv_swin_mlp_mx_supported(int C); /* timm Mlp + norm2 + DropPath behind models/swin_transformer.py:78 */
long long sv_swin_mlp_mx_pack_bytes(int C); /* timm Mlp + norm2 + DropPath behind models/swin_transformer.py:78 */
int sv_swin_mlp_mx_pack(const void* w1q, const void* w1s, const void* w2q, const void* w2s, void* packs, int C, void* stream); /* timm Mlp + norm2 + DropPath behind models/swin_transformer.py:78 */
int sv_swin_mlp_fwd_mx(const void* x1, void* x2, const float* ln_g, const float* ln_b, const void* packs_mx, const float* b1, const float* b2,
                       const float* row_scale, int rows_per_scale, long long M, int C, float eps, void* stream); /* timm Mlp + norm2 + DropPath behind models/swin_transformer.py:78 */
long long sv_swin_mlp_mx_launches(void); /* timm Mlp + norm2 + DropPath behind models/swin_transformer.py:78 */

/* MXFP8 data gradient of the fused Swin MLP branch (backward of timm Mlp + norm2 + DropPath of a SwinTransformerBlock behind
 * models/swin_transformer.py:78): the unfused MX backward chain sv_rowscale -> sv_quant_rows_mx_e4m3 (dy) -> sv_linear_mxfp8_dgrad (fc2, GELU' at the
 * pre-activation) -> sv_quant_rows_mx_e4m3 (dh) -> sv_linear_mxfp8_dgrad (fc1) -> sv_layernorm_bwd (+ residual) composed in ONE kernel.  The
 * pre-activation is recomputed as sv_swin_mlp_fwd_mx computes it; dy's MX rows, the pre-activation and dh never reach HBM.  bf16 token rows.  The
 * weight gradients are sv_swin_mlp_wgrad's (bf16 operands) or, on MX operands, sv_swin_mlp_wgrad_mx's below.
 *  sv_swin_mlp_bwd_mx_supported:  1 where the library has a spill-free instantiation (C = 96 and C = 128), else 0.
 *  sv_swin_mlp_bwd_mx_pack_bytes: size of `packs` for C (0 when unsupported).
 *  sv_swin_mlp_bwd_mx_pack:       w1q [4C, 128] / w1s [4C, 4] (sv_quant_rows_mx_e4m3 of fc1.weight), w2tq [4C, 128] / w2ts [4C, 4] and w1tq [C, 4C] /
 *                                 w1ts [C, 4C / 32] (sv_quant_cols_mx_e4m3 of fc2.weight and of fc1.weight: the MX rows of W^T) -> `packs` in the kernel's
 *                                 fragment order; w1q, w2tq, w1tq and packs 16-byte aligned.  The bytes are re-ordered, never re-quantised.
 *  sv_swin_mlp_bwd_mx:            dx1 = dx2 + d(branch)/dx1, dgamma / dbeta += LayerNorm gradients; arguments and alignment rules of sv_swin_mlp_bwd,
 *                                 with packs_mx from sv_swin_mlp_bwd_mx_pack.
 *  sv_swin_mlp_bwd_mx_launches:   sv_swin_mlp_bwd_mx launches so far in this process (tests: the path they mean to exercise).
 * Refusals (SV_ERR_INVALID before any GPU call, the entry's name in sv_last_error()): null pointers (row_scale may be NULL), unsupported C, M <= 0 or
 * >= 2^31, x1 / dx2 / dx1 / packs_mx / ln_g / ln_b not 16-byte aligned, rows_per_scale <= 0.                                                    */
int sv_swin_mlp_bwd_mx_supported(int C); /* backward of timm Mlp + norm2 + DropPath behind models/swin_transformer.py:78 */
long long sv_swin_mlp_bwd_mx_pack_bytes(int C); /* backward of timm Mlp + norm2 + DropPath behind models/swin_transformer.py:78 */
int sv_swin_mlp_bwd_mx_pack(const void* w1q, const void* w1s, const void* w2tq, const void* w2ts, const void* w1tq, const void* w1ts, void* packs, int C,
                            void* stream); /* backward of timm Mlp + norm2 + DropPath behind models/swin_transformer.py:78 */
int sv_swin_mlp_bwd_mx(const void* x1, const void* dx2, void* dx1, const float* ln_g, const float* ln_b, const void* packs_mx, const float* b1,
                       const float* row_scale, int rows_per_scale, float* dgamma, float* dbeta, long long M, int C, float eps,
                       void* stream); /* backward of timm Mlp + norm2 + DropPath behind models/swin_transformer.py:78 */
long long sv_swin_mlp_bwd_mx_launches(void); /* backward of timm Mlp + norm2 + DropPath behind models/swin_transformer.py:78 */

/* MXFP8 weight gradients of the fused Swin MLP branch (backward of timm Mlp + norm2 + DropPath of a SwinTransformerBlock behind
 * models/swin_transformer.py:78): the unfused MX weight-gradient chain sv_layernorm_quant_mx_fwd -> sv_linear_mxfp8 (GELU, pre_act) -> sv_rowscale ->
 * sv_quant_rows_mx_e4m3 (dy) -> sv_linear_mxfp8_dgrad (fc2, GELU' at the bf16 pre-activation) -> sv_quant_cols_mx_e4m3 x 4 (blocks of 32 tokens per
 * column, counted from token 0; colsum = db2 / db1) -> sv_linear_mxfp8_wgrad x 2 composed in ONE kernel.  h and dh are recomputed as sv_swin_mlp_fwd_mx /
 * sv_swin_mlp_bwd_mx compute them (K = C <= 128: one scaled MFMA per output tile, bit-identical operands); only the fp32 order of the sum over the
 * tokens differs from the chain.  Nothing 4C wide and no quantised operand reaches HBM.  bf16 token rows.
 *  sv_swin_mlp_wgrad_mx_supported: 1 where the library has a spill-free instantiation (C = 96 and C = 128), else 0.
 *  sv_swin_mlp_wgrad_mx:           dw1 [4C, C], db1 [4C], dw2 [C, 4C], db2 [C] += weight gradients (fp32, native layouts, float atomics across token
 *                                  splits only: one split, and bit-repeatable results, for M <= 128).  w1q [4C, 128] / w1s [4C, 4]: sv_quant_rows_mx_e4m3 of
 *                                  fc1.weight; w2tq [4C, 128] / w2ts [4C, 4]: sv_quant_cols_mx_e4m3 of fc2.weight - the native images, no pack entry.
 *  sv_swin_mlp_wgrad_mx_launches:  sv_swin_mlp_wgrad_mx launches so far in this process (tests: the path they mean to exercise).
 * Refusals (SV_ERR_INVALID before any GPU call, the entry's name in sv_last_error()): null pointers (row_scale may be NULL), unsupported C, M <= 0 or
 * >= 2^31, x1 / dx2 / w1q / w2tq not 16-byte aligned, w1s / w2ts not 4-byte aligned, rows_per_scale <= 0, row_scale with rows_per_scale < 128
 * (the rule of sv_swin_mlp_wgrad).                                                                                                           */
int sv_swin_mlp_wgrad_mx_supported(int C); /* backward of timm Mlp + norm2 + DropPath behind models/swin_transformer.py:78 */
int sv_swin_mlp_wgrad_mx(const void* x1, const void* dx2, const float* ln_g, const float* ln_b, const void* w1q, const void* w1s, const void* w2tq,
                         const void* w2ts, const float* b1, const float* row_scale, int rows_per_scale, float* dw1, float* db1, float* dw2, float* db2,
                         long long M, int C, float eps, void* stream); /* backward of timm Mlp + norm2 + DropPath behind models/swin_transformer.py:78 */
long long sv_swin_mlp_wgrad_mx_launches(void); /* backward of timm Mlp + norm2 + DropPath behind models/swin_transformer.py:78 */

/* Fused attention branch of a stage-0 Swin block (timm SwinTransformerBlock._attn + the residual of forward(), reached from
 * models/swin_transformer.py:78): x1 = x + row_scale * proj(window_attention(qkv(LayerNorm(x)))) in one kernel, the roll / 7x7 partition /
 * reverse and the shift mask folded into token index math as in sv_window_attention_fwd.  Built for C = 96, 3 heads, bf16 token rows
 * (sv_swin_attn_block_supported): both weight matrices stay in LDS for the lifetime of a workgroup.
 *  x, x1: [I*H*W, C] bf16;  ln_g / ln_b [C], wqkv [3C, C], bqkv [3C], table [169, heads], wproj [C, C], bproj [C]: fp32 parameters in their
 *  native layouts;  row_scale (may be NULL): one drop-path factor per image.
 *  Side outputs for the (unfused) backward, all or none: ln1 [M, C] bf16 + mean / rstd [M] fp32 (LayerNorm output and statistics),
 *  qkv [M, 3C] bf16, att [M, C] bf16 (head outputs before the projection) - the tensors sv_layernorm_fwd, the qkv linear and
 *  sv_window_attention_fwd would have stored.                                                                                          */
int sv_swin_attn_block_supported(int C, int heads, int act_dtype, int math);
int sv_swin_attn_block_fwd(const void* x, const float* ln_g, const float* ln_b, const float* wqkv, const float* bqkv, const float* table,
                           const float* wproj, const float* bproj, const float* row_scale, void* x1, void* ln1, float* mean, float* rstd,
                           void* qkv, void* att, int I, int H, int W, int C, int heads, int shift, float eps, int act_dtype, void* stream);
/* Consecutive windows per window group (two groups per forward workgroup, one per backward workgroup) of the launch sv_swin_attn_block_fwd
 * (backward = 0) / _bwd (backward = 1) makes for these arguments (call site models/swin_transformer.py:78); pure host function, negative
 * SV_ERR_* for a geometry the entry points refuse. */
int sv_swin_attn_block_windows_per_group(int I, int H, int W, int backward);
/* MXFP8 forward of the same branch (timm SwinTransformerBlock._attn + norm1 + DropPath behind models/swin_transformer.py:78), opt-in: the unfused MX
 * chain sv_layernorm_quant_mx_fwd -> sv_linear_mxfp8 (bias) -> sv_window_attention_fwd_mxq (bf16 core) -> sv_linear_mxfp8 (bias, residual x,
 * row_scale per image) composed in ONE kernel.  qkv and proj run on the block-scaled K = 128 MFMA with E8M0 scales per 32 channels (one head of a
 * token = one block of the projection's operand); LN(x) and the head outputs are quantised in registers, no quantised activation reaches HBM.  The
 * attention core, the launch geometry (sv_swin_attn_block_windows_per_group(I, H, W, 0)) and the side outputs are sv_swin_attn_block_fwd's; the
 * backward is sv_swin_attn_block_bwd + the engine's weight gradients on the stored bf16 tensors, unchanged (straight-through quantisers).
 *  sv_swin_attn_block_mx_supported:  1 for C = 96 with 3 heads, else 0 (timm WindowAttention behind models/swin_transformer.py:78).
 *  sv_swin_attn_block_mx_pack_bytes: size of `packs` for C (0 when unsupported) (timm WindowAttention weights behind models/swin_transformer.py:78).
 *  sv_swin_attn_block_mx_pack:       wqkv_q [288, 128] / wqkv_s [288, 4] and wproj_q [96, 128] / wproj_s [96, 4], the MX rows sv_quant_rows_mx_e4m3
 *                                    makes of qkv.weight and proj.weight (timm WindowAttention behind models/swin_transformer.py:78), -> `packs` in the
 *                                    kernel's fragment order; wqkv_q, wproj_q and packs 16-byte aligned.  The bytes are re-ordered, never re-quantised.
 *  sv_swin_attn_block_fwd_mx:        the arguments of sv_swin_attn_block_fwd with packs_mx (from sv_swin_attn_block_mx_pack) in place of wqkv / wproj
 *                                    (timm SwinTransformerBlock._attn behind models/swin_transformer.py:78); side outputs all or none.
 *  sv_swin_attn_block_mx_launches:   sv_swin_attn_block_fwd_mx launches so far in this process (timm SwinTransformerBlock._attn behind
 *                                    models/swin_transformer.py:78; tests: the path they mean to exercise).
 * Refusals (SV_ERR_INVALID before any GPU call, the entry's name in sv_last_error()): everything sv_swin_attn_block_fwd refuses, unsupported
 * (C, heads), NULL or misaligned packs or pack operands, side outputs given only in part.                                                */
int sv_swin_attn_block_mx_supported(int C, int heads); /* timm SwinTransformerBlock._attn behind models/swin_transformer.py:78 */
long long sv_swin_attn_block_mx_pack_bytes(int C); /* timm SwinTransformerBlock._attn behind models/swin_transformer.py:78 */
int sv_swin_attn_block_mx_pack(const void* wqkv_q, const void* wqkv_s, const void* wproj_q, const void* wproj_s, void* packs, int C,
                               void* stream); /* timm SwinTransformerBlock._attn behind models/swin_transformer.py:78 */
int sv_swin_attn_block_fwd_mx(const void* x, const float* ln_g, const float* ln_b, const void* packs_mx, const float* bqkv, const float* table,
                              const float* bproj, const float* row_scale, void* x1, void* ln1, float* mean, float* rstd, void* qkv, void* att,
                              int I, int H, int W, int C, int heads, int shift, float eps, int act_dtype, void* stream); /* timm SwinTransformerBlock._attn + norm1 + DropPath behind models/swin_transformer.py:78 */
long long sv_swin_attn_block_mx_launches(void); /* timm SwinTransformerBlock._attn behind models/swin_transformer.py:78 */
/* Fused BACKWARD of the same branch (data path): reads dx1 [M,96], the qkv rows and LayerNorm statistics the forward stored, and x; writes
 * dqkv [M,288] (the engine's weight-gradient kernels read it: d qkv.weight / bias from (dqkv, ln1), d proj.weight / bias from (s dx1, att)) and
 * dx = dx1 + LayerNormBackward(dqkv Wqkv) [M,96]; accumulates into dgamma / dbeta of norm1 [96] and dtable [169,3].  dbr (optional) receives
 * s * dx1 when a drop-path scale is given (the projection's weight gradient needs it).  workspace: sv_window_attention_bwd_workspace_floats(3)
 * floats, zero on entry.  9 passes over the token map instead of the 17 of sv_conv_gather -> sv_window_attention_bwd -> sv_conv_gather ->
 * sv_layernorm_bwd.  Replaces the autograd of timm SwinTransformerBlock._attn + norm1 + DropPath behind reference models/swin_transformer.py:78
 * (reference core/train.py:272). */
int sv_swin_attn_block_bwd(const void* dx1, const void* qkv, const void* x, const float* mean, const float* rstd, const float* ln_g,
                           const float* wqkv, const float* wproj, const float* table, const float* row_scale, void* dqkv, void* dx,
                           void* dbr, float* dgamma, float* dbeta, float* dtable, float* workspace, int I, int H, int W, int C,
                           int heads, int shift, int act_dtype, void* stream);

/* Layout kernels of the ResNet stem (models/encoder.py:22: Conv2d(3, 64, 7, stride 2, pad 3) as a 4x4 / stride-1 convolution on the
 * space-to-depth image [I][112][112][(sy, sx, c) = 16]) and of the merger's stencil weights (merger.py:20-54):
 *  sv_stem_space_to_depth: images [I,3,224,224] -> x16;  sv_stem_pack: w [64,3,7,7] fp32 -> [64][16 taps][16] (out_dtype);
 *  sv_stem_unpack_grad: dw [64,3,7,7] += dw16 [64][16][4][4];
 *  sv_merger_pack: w [cout][cin][27] fp32 -> bf16 forward pack [16][27][16 | 48] or data-gradient pack [16 | 48][27][16] (taps flipped);
 *                  concat = 1: the 36 input channels sit at columns 12 g + j of the four 12-wide planes.                              */
/* Encoder input in one pass: images [I, 3, S, S] (fp32 when images_f32, else act_dtype; S % 4 == 0) -> x16 [I, S/2, S/2, 16] (the stem's space-to-depth
 * image, as sv_stem_space_to_depth) and xp [I, S/4, S/4, 48] with xp[.., (ky, kx, c)] = images[c][4 py + ky][4 px + kx]: the rows on which timm's
 * PatchEmbed Conv2d(3, C, kernel 4, stride 4) (behind reference models/swin_transformer.py:78) is a Linear(48, C) with the weight re-indexed
 * [co][c][ky][kx] -> [co][(ky, kx, c)].  Replaces the fp32 -> storage cast, the NCHW -> NHWC transpose and sv_stem_space_to_depth. */
int sv_encoder_prep(const void* images, int images_f32, void* x16, void* xp, int I, int S, int act_dtype, void* stream);
/* Adjoint of sv_encoder_prep, the gradient wrt the renderings: dimages [I, 3, S, S] (fp32 when out_f32, else act_dtype) with
 *   dimages[i][c][y][x] = dx16[i][y/2][x/2][(y%2) 8 + (x%2) 4 + c] + dxp[i][y/4][x/4][(y%4) 12 + (x%4) 3 + c],
 * dx16 [I, S/2, S/2, 16] being the data gradient of the torchvision ResNet-50 stem Conv2d(3, 64, 7, stride 2, pad 3) (behind reference
 * models/encoder.py:22) on the space-to-depth image and dxp [I, S/4, S/4, 48] that of timm's PatchEmbed Conv2d(3, C, 4, 4) (behind reference
 * models/swin_transformer.py:78) on the patch rows.  Every element of dimages is written. */
int sv_encoder_prep_bwd(const void* dx16, const void* dxp, void* dimages, int out_f32, int I, int S, int act_dtype, void* stream);
/* Refiner head Conv3d(1, Co, k = 4, p = 2) on a D^3 grid (reference models/refiner.py:21-26) as a (4, 1, 1)-tap convolution over 16 channels (the stem's
 * trick): xc [N, D, D+1, D+1, 16] with xc[.., Y, X, 4 cy + cx] = x[.., Y + cy - 2, X + cx - 2] (zero outside); sv_head_unpack_dx folds the
 * 16-channel data gradient of that convolution back into dx [N, D, D, D]. */
int sv_head_pack_x(const void* x, void* xc, int N, int D, int act_dtype, void* stream);
int sv_head_unpack_dx(const void* dxc, void* dx, int N, int D, int act_dtype, void* stream);
int sv_stem_space_to_depth(const void* images, void* x16, int I, int act_dtype, void* stream);
int sv_stem_pack(const float* w, void* wp, int out_dtype, void* stream);
int sv_stem_unpack_grad(const float* dw16, float* dw, void* stream);
/* sv_stem_native: w [64,3,7,7] fp32 -> w16 [64][16 = (sy, sx, c)][4][4] fp32, the stem weight in the native [Co][Ci][kh][kw] layout of its
 * 4x4 formulation (the inverse of sv_stem_unpack_grad; zero for c = 3 and for taps outside the 7x7 kernel): the source of the data-gradient
 * pack of the stem on the space-to-depth image (torchvision ResNet-50 conv1, behind reference models/encoder.py:22). */
int sv_stem_native(const float* w, float* w16, void* stream);
int sv_merger_pack(const float* w, void* wp_bf16, int cout, int cin, int dgrad, int concat, void* stream);

/* harness-side kernels on fp32 module outputs */
int sv_mean_views(const float* vol, float* out, int B, int V, int S, void* stream);                      /* core/train.py:246 */
int sv_bce_logits(const float* x, const float* t, long long n, float* loss_accum, float* dx, const float* gscale_dev, void* stream); /* core/train.py:165,249,255 */
int sv_iou_counts(const float* logits, const float* gt, const float* thresholds_dev, int nth, int B, int S, float* counts, void* stream); /* core/test.py:141-163: counts[B][nth][4] = {intersection = TP, union, FP, FN} of sigmoid(logits) >= th vs gt, nth <= 8 */

/* Optimiser step on one flat fp32 buffer per module (parameters, gradients and moments share one layout).
 *  sv_grad_sumsq: slots16[blockIdx & 15] += sum (g * gscale)^2 in double; the caller zeroes the 16 slots.  It is the squared
 *    L2 norm torch.nn.utils.clip_grad_norm_ takes over a module's gradients (core/train.py:279-282).
 *  sv_adam_step / sv_sgd_step: torch.optim.Adam (coupled L2 weight decay, no amsgrad) / torch.optim.SGD (momentum) as
 *    configured at core/train.py:98-131 and stepped at :287-292.  Every gradient is first multiplied by
 *    gscale * min(1, max_norm / (sqrt(sum slots16) + 1e-6)) - the data-parallel mean and the clip coefficient, read on the
 *    device; max_norm <= 0 disables clipping.  `step` counts the calls from 1.  When slots16 is given and its sum is not
 *    finite (an inf / NaN gradient element) the step is SKIPPED on the device: p, m, v stay untouched and
 *    skipped_steps[0] (device counter, may be NULL) += 1 - the behaviour of the reference's GradScaler.step() after
 *    unscale_ (core/train.py:276-293).  Bias correction / "first step" use step - skipped_steps[0].                  */
int sv_grad_sumsq(const float* g, long long n, float gscale, double* slots16, void* stream);
int sv_adam_step(float* p, const float* g, float* m, float* v, long long n, double lr, double beta1, double beta2, double eps,
                 double weight_decay, long long step, float gscale, const double* slots16, float max_norm,
                 long long* skipped_steps, void* stream);
int sv_sgd_step(float* p, const float* g, float* momentum_buf, long long n, double lr, double momentum, double weight_decay,
                long long step, float gscale, const double* slots16, float max_norm, long long* skipped_steps, void* stream);

/* Input preparation on the device (the reference does it per sample on the CPU in DataLoader workers).
 *  sv_binvox_decode: utils/binvox_rw.py:118-149 (read_as_3d_array) for B volumes of equal dims: `rle` holds the concatenated
 *    (value, count) byte pairs that follow the "data" header line, volume b owning pairs [pair_offsets[b], pair_offsets[b+1]);
 *    out[b] = float(np.repeat(values, counts) != 0).reshape(d0, d1, d2), transposed (0, 2, 1) when fix_coords (the loader's
 *    default, utils/data_loaders.py:83-86).  decoded[b] = number of voxels the runs describe; the caller rejects a volume
 *    whose count differs from d0*d1*d2 (the reference's reshape raises).
 *  sv_augment_views: utils/data_transforms.py applied in the order of core/train.py:44-59 to I = B*V renderings stored as
 *    8-bit [I][Hs][Ws][C] (C = 4 with alpha, or 3), without a bounding box: centre crop (crop_h, crop_w) when the image is
 *    larger, cv2.resize INTER_LINEAR to (out_h, out_w), RandomBackground (alpha == 0 -> bg), ColorJitter, RandomNoise,
 *    Normalize, RandomFlip, RandomPermuteRGB, ToTensor -> out [I][3][out_h][out_w] fp32.  One sv_aug_sample per SAMPLE (the
 *    reference draws these once per __getitem__ and shares them between the V views), one flip byte per IMAGE.  The
 *    validation pipeline (:60-65) is the same call with identity jitter / zero noise / no flips / identity permutation.
 *    grey_sum_ws: I doubles of scratch (mean grey level per image for the contrast step).                               */
typedef struct sv_aug_sample {
  float bg[3];            /* background colour in [0, 1], channel order of the stored image                              */
  float jitter_value[3];  /* blend factors: [0] brightness, [1] contrast, [2] saturation (1 = unchanged)                 */
  int jitter_order[3];    /* the order the three adjustments are applied in (a permutation of 0, 1, 2)                    */
  float noise[3];         /* RandomNoise offset per stored channel (noise_rgb reversed, data_transforms.py:386-390)       */
  int perm[3];            /* output channel c = stored channel perm[c]                                                    */
  float mean[3], std[3];  /* Normalize                                                                                    */
} sv_aug_sample;
int sv_binvox_decode(const unsigned char* rle, const long long* pair_offsets, int B, int d0, int d1, int d2, int fix_coords,
                     float* out, int* decoded, void* stream);
int sv_augment_views(const unsigned char* src, int I, int V, int Hs, int Ws, int C, int crop_h, int crop_w, int out_h, int out_w,
                     const sv_aug_sample* params_dev, const unsigned char* flip_dev, double* grey_sum_ws, float* out, void* stream);

/* sv_binvox_encode: the run-length writer of utils/binvox_rw.py:239-292 (write) for B volumes of equal dims, the inverse of
 *    sv_binvox_decode.  File order is [d0][d1][d2]; `vol` is [B][d0][d2][d1] when fix_coords (xyz order, what the decoder
 *    produces: file element (i, j, k) = vol[b][(i*d2 + k)*d1 + j]), [B][d0][d1][d2] otherwise.  For cubic volumes that is
 *    the writer's axis_order == 'xyz' branch (:269-270); for non-cubic ones the contract is "inverse of the reader" (the
 *    reference's own writer and reader are not inverses there).  dtype 0 = float32, 1 = uint8 (bool tensors pass as uint8).
 *    threshold < 0: the input is occupancy, a voxel is set iff its value != 0; 0 < threshold < 1: float32 logits, set iff
 *    1.f / (1.f + expf(-x)) >= threshold, the predicate of sv_iou_counts.  Values written are 0 and 1 only.
 *    pairs + b * 2 * pair_capacity receives volume b's (value, count) bytes - the payload that follows the "data" header
 *    line - and n_pairs[b] their number; pair_capacity >= d0*d1*d2 is required and always suffices.
 *    Zero-count pairs: the reference dumps (state, 255) when its counter reaches 255 and restarts it at 0; when the very next
 *    voxel switches value it dumps (state, 0).  So a run of n voxels that is not the last emits n / 255 pairs (v, 255) and
 *    then (v, n % 255) EVEN WHEN n % 255 == 0; the last run emits (v, n % 255) only when that is non-zero.  These bytes are
 *    reproduced exactly; readers (np.repeat, sv_binvox_decode) skip a zero count.                                          */
int sv_binvox_encode(const void* vol, int dtype, int B, int d0, int d1, int d2, int fix_coords, float threshold,
                     unsigned char* pairs, long long pair_capacity, int* n_pairs, void* stream);

/* sv_voxel_surface: the exposed voxel faces of B volumes of equal dims as indexed quad meshes - the face set utils/helpers.py:50-88
 *    (get_volume_views -> Axes3D.voxels, called from core/test.py:178-187) and utils/binvox_rw.py:306-343 draw.
 *    `vol` is [B][d0][d1][d2] in its own axis order (no fix_coords transposition), every dim in 1 .. 64; dtype and threshold as
 *    for sv_binvox_encode (0 = float32, 1 = uint8; threshold < 0: occupancy, set iff != 0; 0 < threshold < 1: float32 logits, set
 *    iff 1.f / (1.f + expf(-x)) >= threshold), the same predicate, so mesh, .binvox file and reported IoU agree voxel for voxel.
 *    Exposed face: voxel (x, y, z) is set and its neighbour in a direction is unset or outside the grid.
 *    Face order: ascending voxel index (x*d1 + y)*d2 + z, then direction -x, +x, -y, +y, -z, +z.  Corners (offsets added to
 *    (x, y, z)), counter-clockwise seen from outside:
 *      -x (0,0,0) (0,0,1) (0,1,1) (0,1,0)     +x (1,0,0) (1,1,0) (1,1,1) (1,0,1)
 *      -y (0,0,0) (1,0,0) (1,0,1) (0,0,1)     +y (0,1,0) (0,1,1) (1,1,1) (1,1,0)
 *      -z (0,0,0) (0,1,0) (1,1,0) (1,0,0)     +z (0,0,1) (1,0,1) (1,1,1) (0,1,1)
 *    Vertex order: the lattice points (i, j, k) of [0..d0] x [0..d1] x [0..d2] that are a corner of an exposed face, each once,
 *    in ascending lattice index (i*(d1+1) + j)*(d2+1) + k.
 *    verts + b * vert_capacity receives volume b's lattice indices, faces + b * 4 * face_capacity its quads as four indices
 *    into that vertex list (`faces` 16-byte aligned), counts[2b] / counts[2b + 1] the number of vertices / faces.
 *    vert_capacity >= (d0+1)(d1+1)(d2+1) and face_capacity >= 3*d0*d1*d2 + d0*d1 + d1*d2 + d0*d2 are required and always
 *    suffice.  One workgroup per volume, no atomics: the output is deterministic.                                          */
int sv_voxel_surface(const void* vol, int dtype, int B, int d0, int d1, int d2, float threshold, unsigned int* verts,
                     long long vert_capacity, unsigned int* faces, long long face_capacity, int* counts, void* stream);

/* sv_augment_images: the bounding-box branch of CenterCrop / RandomCrop (utils/data_transforms.py:93-136, :187-232), which the
 *    Pascal3D and Pix3D loaders take for every sample (utils/data_loaders.py:176-180, :311-315), followed by the rest of the
 *    transform list as sv_augment_views applies it.  I photographs of DIFFERING sizes, one view each, packed into one 8-bit
 *    buffer `src` of src_bytes bytes; image i is [Hs][Ws][C] at byte offset images[i].offset (no alignment required).  All
 *    images of a call share C (3 or 4).  The kept rectangle is img[y_top:y_bottom + 1, x_left:x_right + 1] (inclusive, as
 *    the reference writes it) and the pads are those of its np.pad(..., mode='edge'): the padded crop is
 *    cw = pad_l + (x_right - x_left + 1) + pad_r wide and ch = pad_t + (y_bottom - y_top + 1) + pad_b high and is resized
 *    (cv2.resize INTER_LINEAR, separate scales cw / out_w and ch / out_h) to (out_h, out_w).  No padded copy is made:
 *    padded coordinate s reads source column clamp(x_left - pad_l + s, x_left, x_right), likewise in y.  An image without a
 *    box uses the same table with zero pads and the centre-crop rectangle of sv_augment_views (or the whole image).
 *    How the reference gets the integers from a box in fractions of the image (Python doubles, int() truncating toward
 *    zero) is restated in INTEGRATION.md and swinvox_amd/data.py (bbox_crop_rect); callers of the C ABI compute them so.
 *    images_host (host memory) is validated BEFORE anything is launched - rectangle non-empty and inside the image, pads
 *    >= 0, cw / ch / Hs / Ws at most 2^24, offset >= 0 and offset + Hs*Ws*C <= src_bytes - and then copied to
 *    images_dev_ws (I descriptors of device scratch) on the stream; a bad table is an error code, never a read outside
 *    `src`.  params_dev: one sv_aug_sample per image; flip_dev: one byte per image or NULL; grey_sum_ws: I doubles of
 *    scratch; out [I][3][out_h][out_w] fp32.  I <= 65535.                                                                */
typedef struct sv_aug_image {
  long long offset;                        /* byte offset of the image's first pixel in src                                */
  int Hs, Ws;                              /* its height and width                                                         */
  int x_left, x_right, y_top, y_bottom;    /* kept rectangle, inclusive, inside the image                                  */
  int pad_l, pad_r, pad_t, pad_b;          /* edge-replicated columns / rows around it                                     */
} sv_aug_image;
int sv_augment_images(const unsigned char* src, long long src_bytes, int I, int C, const sv_aug_image* images_host,
                      sv_aug_image* images_dev_ws, int out_h, int out_w, const sv_aug_sample* params_dev,
                      const unsigned char* flip_dev, double* grey_sum_ws, float* out, void* stream);

/* sv_augment_views_bg: sv_augment_views with the folder of RandomBackground(color_range, random_bg_folder_path)
 *    (utils/data_transforms.py:415-452), which the reference's real-photograph experiments paste their renderings over.  The
 *    reference picks one photograph per sample (random.choice, :439) and then, per view, either that photograph or the flat
 *    colour (random.randint(0, 1), :447); its blend alpha * bg + (1 - alpha) * img has alpha in {0, 1}, so it is a select.
 *    All arguments of sv_augment_views keep their meaning.  bank: n_bank photographs as 8-bit [n_bank][out_h][out_w][3] on the
 *    device, channel order of the stored renderings (cv2.imread gives both); a photograph has exactly the output size - the
 *    reference fails on any other (its multiply cannot broadcast) - and nothing is resized or cropped.  bg_index_host (host
 *    memory, I ints): entry i is the photograph of image i, or -1 for the flat colour params_dev[i / V].bg.
 *    Rule: a pixel whose resized alpha is exactly 0 becomes (float)bank[idx][oy][sx][c] / 255.f when idx >= 0, else bg[c];
 *    sx is the column the source is sampled at, out_w - 1 - ox for a flipped image: RandomFlip mirrors the finished image,
 *    photograph included.  The grey mean of the contrast step is taken over the same composite.  C = 3 composites nothing.
 *    The table is validated BEFORE anything is launched: -1 <= idx < n_bank for every image, and bank non-NULL when any idx is
 *    >= 0; it is then copied to bg_index_dev_ws (I ints of device scratch) on the stream.  A bad table is an error code and
 *    nothing is written, never a read outside the bank.  With every index -1 the output has the bits of sv_augment_views.
 *    I <= 65535; two launches, no second pass over the output.                                                           */
int sv_augment_views_bg(const unsigned char* src, int I, int V, int Hs, int Ws, int C, int crop_h, int crop_w, int out_h, int out_w,
                        const sv_aug_sample* params_dev, const unsigned char* flip_dev, const unsigned char* bank, int n_bank,
                        const int* bg_index_host, int* bg_index_dev_ws, double* grey_sum_ws, float* out, void* stream);

/* sv_render_volumes: pictures of B volumes of equal dims from n_cams viewpoints - what utils/helpers.py:50-88 (get_volume_views ->
 *    Axes3D.voxels(edgecolor="k") at elev 30 / azim 45, called from core/test.py:178-187) and utils/binvox_rw.py:306-343 draw, as a
 *    ray-cast.  `vol` is [B][d0][d1][d2] in its own axis order (no fix_coords transposition), every dim in 1 .. 64; dtype and
 *    threshold as for sv_voxel_surface (0 = float32, 1 = uint8; threshold < 0: occupancy, set iff != 0; 0 < threshold < 1: float32
 *    logits, set iff 1.f / (1.f + expf(-x)) >= threshold), the same predicate, so picture, mesh, .binvox file and IoU agree voxel for
 *    voxel.  Voxel (i, j, k) fills [i, i+1] x [j, j+1] x [k, k+1].
 *    Camera: one ray per pixel, affine in the pixel centre; row 0 is the top of the image:
 *      origin = o0 + (col+0.5) ox + (row+0.5) oy        dir = d0 + (col+0.5) dx + (row+0.5) dy
 *    (perspective: ox = oy = 0, o0 is the eye; orthographic: dx = dy = 0).  data.view_camera gives the reference's camera.
 *    Ray-cast, every step one fp32 operation (no fma contraction, IEEE division), per axis a with extent D:
 *      1. slab: dir != 0: t0 = (0 - origin) / dir, t1 = (D - origin) / dir, tnear = min, tfar = max; dir == 0: tnear = -inf and
 *         tfar = +inf when 0 <= origin < D, else a miss.
 *      2. tin = max tnear, tout = min tfar; hit iff tin < tout and tin > 0.  Entry axis = first arg-max of tnear (x before y before z).
 *      3. entry cell = clamp(floor(origin + dir * tin), 0, D - 1); along the entry axis 0 when dir > 0, else D - 1.
 *      4. Amanatides-Woo: tmax = ((cell + (dir > 0)) - origin) / dir, tdelta = |1 / dir| (both +inf for dir == 0); while the cell is
 *         unset, advance the axis with the smallest tmax (first arg-min): cell += sign(dir), tmax += tdelta; leaving the grid is a miss.
 *    ids[b][cam][row][col] = ((i*d1 + j)*d2 + k)*6 + face of the first set voxel on the ray, face = the one the ray entered it
 *    through, numbered -x, +x, -y, +y, -z, +z (the order of sv_voxel_surface); -1 = background.
 *    Shading (skipped when rgb is NULL), an integer rule on the ids: a pixel is an edge pixel iff its id differs from the id of its
 *    right or of its lower neighbour (the pixel itself at the last column / row); edge pixels take edge_rgb, other hit pixels
 *    face_rgb[3*face ..], other pixels plate_dev[ch][row][col] when plate_dev is given, else background_rgb.
 *    rgb is [B][n_cams][3][H][W].  face_rgb (18), edge_rgb (3), background_rgb (3) and cams_host are host memory; cams_host is
 *    validated BEFORE anything is launched and then copied to cams_dev_ws (n_cams cameras of device scratch) on the stream.
 *    mask_ws: B*d0*d1 words of device scratch for d2 <= 32, twice that above (bit k of a row's word(s) = voxel (i, j, k)).
 *    Refused with an error code, before any launch: null pointers (plate_dev and rgb may be NULL), dims outside 1 .. 64, B or n_cams
 *    outside 1 .. 65535, H or W < 1, H*W > 2^24, a camera number that is not finite, a threshold outside the two ranges, a
 *    perspective eye inside or on the box [0, d0] x [0, d1] x [0, d2].  At most three launches, no atomics: deterministic.         */
typedef struct sv_view_camera { float o0[3], ox[3], oy[3], d0[3], dx[3], dy[3]; } sv_view_camera;
int sv_render_volumes(const void* vol, int dtype, int B, int d0, int d1, int d2, float threshold,
                      const sv_view_camera* cams_host, int n_cams, sv_view_camera* cams_dev_ws, int H, int W,
                      const unsigned char* face_rgb, const unsigned char* edge_rgb, const unsigned char* background_rgb,
                      const unsigned char* plate_dev, unsigned int* mask_ws, int* ids, unsigned char* rgb, void* stream);

/* sv_voxelise_meshes: B triangle meshes -> B occupancy volumes of equal dims, the step the reference leaves to the external `binvox`
 *    program (utils/binvox_converter.py and its notebook's convert_obj_to_binvox shell out to it).  That program is part of neither
 *    tree and was never run next to this code: NO PARITY WITH IT IS CLAIMED.  What is computed is the rule below, in exact integer
 *    arithmetic, so that a restatement (tests/mesh_voxel_ref.py) agrees bit for bit.
 *    Grid and fixed point.  S = 1024 units per voxel.  verts: int32 [total_verts][3] in grid units, tris: int32 [total_tris][3], both
 *    on the device; mesh b owns vertices mesh_table[4b] .. + mesh_table[4b+1] and triangles mesh_table[4b+2] .. + mesh_table[4b+3], its
 *    triangle indices counting from its own first vertex.  Dims d0, d1, d2 in 1 .. 64 each (the range of sv_voxel_surface).  Voxel
 *    (i, j, k) is the closed cube [iS, (i+1)S] x [jS, (j+1)S] x [kS, (k+1)S]; its centre ((2i+1)S/2, (2j+1)S/2, (2k+1)S/2) is a lattice
 *    point of the units.  Every coordinate must lie in [-d S, 2 d S] of its axis - the CALLER guarantees it (data.voxelise_mesh_batch
 *    refuses a mesh outside with the reason); inside it every quantity fits int64: differences < 2^18, edge functions and normal
 *    components < 2^37, plane values < 2^57.  A triangle with a zero normal is skipped in both modes.
 *    SV_VOXELISE_SOLID: parity along z.  For a triangle a, b, c: A2 = (b.x-a.x)(c.y-a.y) - (b.y-a.y)(c.x-a.x); A2 == 0: skipped; A2 < 0:
 *    b and c change places for the edge tests only.  The column through the centre P = (Px, Py) is covered when for each directed edge
 *    u -> v, d = v - u, the edge function E = d.x (Py - u.y) - d.y (Px - u.x) is > 0, or is 0 and the edge owns its ties: d.y < 0, or
 *    d.y == 0 and d.x < 0.  With n = (b-a) x (c-a) of the original triangle, voxel k of a covered column is toggled iff
 *    sgn(n.z) (n.x (Px-a.x) + n.y (Py-a.y) + n.z (zk - a.z)) > 0, zk = (2k+1)S/2: the crossing lies strictly below the centre; the
 *    toggled voxels are a suffix of the column.  A voxel is set iff it was toggled an odd number of times.
 *    SV_VOXELISE_SURFACE: voxel (i, j, k) is set iff its closed cube and the closed triangle intersect, decided by the 13 separating
 *    axes (3 cube normals, the triangle's normal, 9 cross products of a cube axis with a triangle edge) with the vertices taken
 *    relative to the cube's centre: the sets are disjoint iff on one axis the triangle's projections lie strictly beyond the cube's
 *    radius S/2 (|x| + |y| + |z| of the axis).  Touching counts: a triangle lying in a lattice plane sets the voxels on BOTH sides of it.
 *    SV_VOXELISE_BOTH: surface | solid, what `binvox -e` is documented to produce (exact surface voxels, interior filled).
 *    XOR and OR commute: the result depends neither on the order of the triangles nor on how they are split over workgroups.
 *    out: [B][d0][d1][d2], 0 / 1 as float32 (out_dtype 0) or uint8 (1).  workspace: sv_voxelise_meshes_workspace_bytes(B, d0, d1, d2)
 *    bytes of device scratch, 8-byte aligned, cleared on the stream by the call (no host synchronisation): the table's device copy
 *    (4 B long longs), then B ints at byte offset 32 B - entry b counts the triangles of mesh b that name a vertex outside 0 ..
 *    n_verts - 1; such a triangle is skipped, never dereferenced, and data.voxelise_mesh_batch raises on a non-zero count -, then
 *    (8-byte aligned) per mesh the solid and the surface mask, d0*d1 rows of one (d2 <= 32) or two 32-bit words, bit k = voxel (i, j, k).
 *    mesh_table (host memory) is validated BEFORE anything is launched: offsets and counts >= 0 and inside total_verts / total_tris,
 *    counts < 2^31; also refused: null out / workspace / table (verts and tris may be NULL when their total is 0), B outside 1 .. 65535,
 *    dims outside 1 .. 64, an unknown mode or out_dtype, a misaligned workspace.  A refused call is an error code; out and the
 *    workspace are untouched.  A mesh without triangles gives an empty volume.  The workspace query returns 0 for what is refused. */
enum { SV_VOXELISE_SOLID = 0, SV_VOXELISE_SURFACE = 1, SV_VOXELISE_BOTH = 2 };
size_t sv_voxelise_meshes_workspace_bytes(int B, int d0, int d1, int d2);
int sv_voxelise_meshes(const int* verts, long long total_verts, const int* tris, long long total_tris, const long long* mesh_table,
                       int B, int d0, int d1, int d2, int mode, int out_dtype, void* out, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SWINVOX_HIP_H */
