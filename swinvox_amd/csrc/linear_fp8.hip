// fp8 (OCP e4m3fn) forward of the Swin linear layers on the block-scaled K = 128 MFMA (v_mfma_scale_f32_16x16x128_f8f6f4).
//
// Recipe, for y = x W^T with x [M, K] (stored activations, bf16 or fp32) and W [N, K] (fp32 parameter):
//   row scales   sx[m] = 224 / max_k |x[m, k]|, sw[n] = 224 / max_k |W[n, k]|, formed in fp32 (IEEE division).  An all-zero row gets scale 1 (the
//                constant and the zero rule of the fp8 window attention, attn.hip).  CLAMP: a scale is at most 2^60, so the product
//                sx[m] sw[n] of the epilogue is finite for every input; a row whose maximum is below 224 / 2^60 = 1.9e-16 quantises to zeros.
//   quantisers   xq = e4m3_rne(x sx), wq = e4m3_rne(W sw), the product formed in fp32 (v_cvt_pk_fp8_f32: round to nearest even).
//   operands     rows of Kp = roundup(K, 128) bytes, the padding bytes zero in BOTH operands: the contraction has no K tail.
//   contraction  acc = sum_k xq wq in fp32 on the 16 x 16 x 128 scaled MFMA, both formats e4m3 (cbsz = blgp = 0), both hardware block scales
//                1.0 (E8M0 exponent 127 in every byte, op-sel 0); val = acc / (sx[m] sw[n]) in fp32 in the epilogue.
//   epilogue     sv_epilogue semantics on val, in the engine's order (igemm.hip epilogue_rows): + bias, pre_act copy, activation, residual +
//                row_scale * val, store rounded to the storage type.  The arithmetic is common.h's (apply_act_t, stf / stnf): GELU is the erf form
//                with fp32 storage and the fast form with bf16 storage (its error is 1/30 of the bf16 rounding unit of the stored value).
//                Served: no activation or GELU, bias, pre_act, residual / ldr, row_scale / rows_per_scale, ldc.  Refused with a status code:
//                stats, act_grad_src, other activations, col_off != 0.
//
// Kernels
//   quant_rows_kernel   one wave per row: amax by a DPP / permlane reduction (wave_max), then Kp bytes and one fp32 scale.  The row is read twice
//                       (the second time from cache); activations (bf16 / fp32) and weights (fp32) take the same kernel.
//                       SECOND PRODUCER of these operand rows: ln_fwd_kernel with its LnQuantOut argument (norm.hip, sv_layernorm_quant_fwd) writes the same bytes and
//                       scales for the rows a token LayerNorm stores (norm1 -> qkv, norm2 -> fc1, patch-merge norm -> reduction), from the
//                       registers that hold the normalised row.  att -> proj and h -> fc2 keep this kernel under the per-row recipe (neither
//                       producer sees a full row); under the MX recipe below their producers emit the operand rows themselves.
//   linear_fp8_kernel   128 x 128 output tile per 256-thread workgroup, 4 waves as 2 x 2, a wave owns 64 x 64 = 4 x 4 MFMA blocks (64 accumulator
//                       registers).  One k-step = 128 bytes of every row = ONE MFMA deep: 16 KB per operand tile, staged through registers
//                       (16-byte global loads of the next step are in flight while the current step's 16 MFMAs per wave run) into two LDS
//                       buffers, one barrier per step.  LDS rows are 128 bytes = eight 16-byte pieces; a plain image would put every row
//                       on the same banks, so piece c of row r lives at position c ^ swz(r), swz(r) = bit 1 of r | bit 3 of r << 2: each of
//                       the four 16-lane groups a ds_read_b128 is served in (lanes 0-3, 12-15, 20-27 / 4-11, 16-19, 28-31 / + 32) then
//                       covers the 64 banks exactly once, for both halves of a fragment (no pitch from 128 to 256 bytes does: all leave
//                       2-way conflicts), and a staging write still fills whole rows.  LDS: 2 x 2 x 128 x 128 = 65 536 bytes, two
//                       workgroups per CU.  Rows and columns past M / N load a clamped (valid) row and are skipped by the epilogue: nothing
//                       is read or written out of range.
//   Operand lane map of the K = 128 form: lane l holds row / column l & 15 and 32 bytes of its row in eight VGPRs.  Both
//   operands use the same k map, so the unit-scale sum does not depend on it (the MX form does: lf_contract); the row / column map and the C/D map (the 16 x 16 one) are what the
//   exact-integer test (tests/test_gpu_linear_fp8.py) establishes.  W is the A operand and x the B operand: a lane then holds output row
//   l & 15 and four consecutive rows of D = output columns per block; the W rows are permuted on their way into LDS so that the lane's four blocks
//   together are 16 consecutive output columns - 16-byte stores, 32 (bf16) / 64 (fp32) contiguous bytes per lane and row.
//
// MX recipe (opt-in: set_linear_fp8(True, recipe="mx")): the same e4m3 operands with one E8M0 power-of-two scale per 32 consecutive elements of
// the contraction, applied by the MFMA.  A scale depends on 32 neighbouring values only, so producers that never see a full row can emit the
// operand.  It is a structural feature, not an accuracy feature: e4m3's three mantissa bits set the error.  NORMATIVE:
//   operand form   rows of Kp = roundup(K, 128) OCP e4m3fn bytes + one E8M0 byte per 32-byte block, [rows][Kp / 32] uint8: four bytes per row and
//                  k-step, so a row's scales of one k-step are one aligned dword.
//   block scale    amax over the 32 STORED values (the value rounded to the storage type first).  amax = m 2^e, m in [1, 2):
//                  E = e - 8 + (m > 1.75) = ceil(log2(amax / 448)), taken from the float's bits (no transcendental), clamped to [-127, 127];
//                  byte = E + 127; an all-zero block takes byte 127; byte 255 is never produced.  Round-up variant: |x 2^-E| <= 448 always, so
//                  nothing saturates.  Pins (amax -> byte, q of the maximum): 1 -> 119, 256; 1.75 -> 119, 448; 1.7578125 -> 120, 224;
//                  224 -> 126, 448; 448 -> 127, 448; 450 -> 128; 0 -> 127, 0; 1e-30 -> 19.
//   elements       q = e4m3_rne(ldexpf(x, -E)): the scaling is an exponent add, exact.
//   padding        bytes K .. Kp - 1 are zero; blocks that lie wholly in the padding carry byte 127.
//   contraction    v_mfma_scale_f32_16x16x128_f8f6f4, cbsz = blgp = 0, the two scale operands from the operands' scale bytes, fp32 accumulation;
//                  val = acc, no division.  The epilogue (bias, pre_act copy, GELU, residual + row_scale, ldc) is the per-row kernel's, unchanged.
//   emission       optional q_out / qs_out: the MX rows of the STORED output (after the activation, rounded to the storage type), for the output
//                  the next linear contracts over (fc1's h): Kp_out = N, so N % 128 == 0, and no residual.  With q_out, out and pre_act may be
//                  null (no backward follows): fc1 then writes 1 byte per hidden element instead of 4.  With q_out, out may also be null
//                  while pre_act is given in front of an activation (fc1 under the MX store below): pre_act and the rows are written,
//                  bit-identical to the call that stores out too.  Without an activation that form stays refused (pre_act would be out itself).
// Kernels of the MX recipe
//   quant_rows_mx_kernel   the definition every producer equals: one wave per row, 8 lanes per block, three lane exchanges for the block maximum.
//   linear_fp8_kernel<.., MX = true>   the kernel above with lf_contract<true>: the scale dwords of a k-step (128 + 128, 1 KB per buffer) are
//                  staged beside the operand tiles - LDS 65 536 + 2 048 = 67 584 bytes, still two workgroups per CU - and the lane maps of the
//                  scale operands and of the e4m3 data are those documented at lf_contract.  Emission: a 32-column block is the 16 + 16
//                  columns of lanes lg and lg ^ 1 of one row: one exchange (lane ^ 16) gives its maximum, each lane stores its 16 bytes and
//                  the even one of the pair the scale byte.  Other producer: win_attn_fwd_wg*_kernel<.., MXQ = true> (attn.hip,
//                  sv_window_attention_fwd_mxq): one head of one token is one block.
//
// Backward (opt-in: set_linear_fp8(True, backward=True)); the constants, the zero rule, the clamp, the rounding, the zero padding to a multiple of 128
// bytes along the contraction, the unit hardware block scales and the fp32 IEEE division of the epilogue are the forward's.  All operands are
// e4m3: inside one contraction its range (224 / 2^-9 = 1e5 below the vector's maximum) loses only terms that do not matter to the sum, and its
// third mantissa bit (e5m2 has two) does matter.  The quantisers are straight-through.
//   data gradient    dx[M, K] = dy[M, N] W[N, K], contraction over N.  dy is quantised per ROW (scale over N: sd[m], the row quantiser above),
//                    W^T per row = per COLUMN k of W (scale over N: swt[k], the column quantiser on the [N, K] fp32 weight, whose [K][Np] output is
//                    the row-major operand the GEMM wants).  val = acc / (sd[m] swt[k]).  Epilogue forms served: none; act_grad_src with
//                    SV_ACT_GELU (val *= gelu'(act_grad_src), common.h's act_grad_t<FAST>, FAST with bf16 storage as in the engine); ldc.
//                    Everything else (stats, bias, residual, row_scale, pre_act, act, another act_grad_kind, col_off) is refused.
//   weight gradient  dw[N, K] += dy^T[N, M] x[M, K], contraction over M.  dy and x are quantised per COLUMN, one scale per column over all M rows of
//                    the stored tensor (sdc[n], sxc[k]), and written transposed as [N][Mp] and [K][Mp] bytes, Mp = roundup(M, 128), zeros past M.
//                    val = acc / (sdc[n] sxc[k]) is added into the fp32 dw in its native [N, K] layout.  db[n] += sum_m dy[m, n] is taken in
//                    fp32 from the stored, unquantised dy by the column quantiser's first pass.
// Kernels of the backward
//   quant_cols_*     pass 1: per-workgroup partial column maxima (and fp64 partial column sums), then an integer atomic max on the bit pattern
//                    of the non-negative float (and one fp32 atomic add per workgroup and column); a C-thread kernel turns the maxima into
//                    scales in place; pass 2: a 128-row x 64-column tile is scaled, rounded and transposed through LDS, 16-byte stores along M.
//   lf_contract      the k-loop of linear_fp8_kernel (staging, swizzled LDS image, fragment reads, MFMA block) over a range of k-steps: the one
//                    copy the forward, the data-gradient and the weight-gradient kernel run.
//   shared by the GEMM kernels (both recipes)   lf_tile_contract: the tile of blockIdx.x, the LDS buffers, lf_contract.  lf_col_scales / lf_row:
//                    the lane's rows and 16 columns, with the division of the per-row recipe.  lf_pieces: the width of a lane's loads and
//                    stores (16 bytes, 4 elements, 1 element), chosen once per lane, one templated body per epilogue.  The data-gradient
//                    kernel shares the first and writes the other two out (reason at the kernel).  LinArgs / DgradArgs / WgradArgs<MX>.
//   linear_fp8_dgrad_kernel   lf_contract over the full contraction + the epilogue above.
//   linear_fp8_wgrad_kernel<MX = false>   grid tiles(N) x tiles(K) x splits, split z contracts the k-steps [z nk / splits, (z + 1) nk / splits); dy^T
//                    is the row operand, so a lane's 16 consecutive outputs run along k, the contiguous dimension of dw; fp32 atomicAdd into dw
//                    (a plain read-add-write when splits == 1).  splits = 0 picks enough workgroups for 2 per CU of 256 CUs
//                    (linear_wgrad_splits, for both recipes).
//
// MX backward (opt-in: set_linear_fp8(True, backward=True, backward_recipe="mx")): both gradients on MX operands.  A block scale over 32 TOKENS of a
// column needs no global maximum, so the transposing quantiser is one launch and one read, and nothing is left to divide out.  NORMATIVE: everything
// is the MX forward's - the block exponent, the rounding, "nothing saturates", byte 127 for all-zero and padding blocks, val = acc, no clamp, no
// division.  The quantisers are straight-through and read the stored bf16 / fp32 tensors.
//   data gradient    dx[M, K] = dy[M, N] W[N, K], contraction over N.  dy from quant_rows_mx_kernel (blocks along n); W^T as [K][Np] bytes +
//                    [K][Np / 32] scale bytes, a block = 32 consecutive n of one column k (the column quantiser below on the [N, K] fp32 weight).
//                    Epilogue forms and refusals are exactly the row recipe's: none, act_grad_src with SV_ACT_GELU, ldc.
//   weight gradient  dw[N, K] += dy^T[N, M] x[M, K], contraction over M.  dy^T as [N][Mp] bytes + [N][Mp / 32] scale bytes, x^T as [K][Mp] bytes +
//                    [K][Mp / 32] scale bytes, Mp = roundup(M, 128); a block = 32 consecutive TOKENS of one column.  Bytes past M are zero, blocks
//                    wholly past M carry 127.  db[n] += sum_m dy[m, n] in fp32 from the unquantised dy in the quantiser's pass.
//   column quantiser its output EQUALS quant_rows_mx_kernel applied to the transposed stored tensor, bit for bit: a partly filled last block takes
//                    the maximum of its valid rows.
// Kernels of the MX backward
//   quant_cols_mx_kernel   ONE launch, src read once: the 128-row x 64-column tile of quant_cols_write_kernel; thread (tx, ty) owns rows 32 ty .. + 31
//                    of column tx = exactly one MX block, so the block maximum stays in its registers (32 values held, no exchange:
//                    mx_pack_block32).  The way out is the transposing quantisers' shared one (store_cols_tile): the [column][33 dwords] LDS
//                    image, 16-byte stores along M, the four scale bytes of a column and tile as one dword, and for the column sums the fp64
//                    partials of a workgroup as one fp32 atomic per column.
//   linear_fp8_dgrad_kernel<.., MX = true>   lf_contract<true> + the epilogue above without its 16 divisions per lane and row; LDS 67 584 bytes.
//   linear_fp8_wgrad_kernel<MX = true>   lf_contract<true> over split z's k-steps; NO atomics into dw.  One split: the only writer of an element does a
//                    16-byte read-add-write into dw.  More: split z stores its fp32 partial tile into a caller-owned workspace [splits][N][K]
//                    (16-byte stores) and linear_mxfp8_wgrad_reduce_kernel adds the partials to dw in ascending z: dw is bit-identical from run to
//                    run for a given `splits`.  splits = 0: enough workgroups for two per CU of 256 CUs, at most one per 128 tokens.
//
// MX store (opt-in: set_linear_fp8(True, backward=True, recipe="mx", backward_recipe="mx", store="mx")): the training tape keeps the MX ROWS the
// forward GEMM consumed in place of the stored tensor, and the weight gradient re-blocks them along the tokens.  NORMATIVE:
//   sv_mx_rows_to_cols   xq [M][Kp] e4m3 bytes + xs [M][Kp / 32] E8M0 bytes (a block = 32 columns of a row) -> dst_q [K][Mp] bytes + scales_u8
//                  [K][Mp / 32] (a block = 32 tokens of a column), Mp = roundup(M, 128).  The output EQUALS the MX column quantiser applied to the
//                  dequantised rows, columns 0 .. K - 1, bit for bit: decode byte 2^(s - 127) in fp32 (exact: at most 4 significant bits, exponent
//                  >= -136); block maximum over the valid tokens; mx_block_exp and pack4_e4m3_mx of common.h; bytes past M zero; blocks wholly past M
//                  byte 127.  Columns >= K of xq do not influence the result.  The decode is exact down to the smallest scale byte only with fp32
//                  denormals PRESERVED (v_ldexp_f32 and v_max_f32 follow the kernel's denormal mode; hipcc's default for gfx9 keeps them, and the
//                  file must not be built with -fgpu-flush-denormals-to-zero): below 2^-126 the decoded values are fp32 denormals.
//   why it is today's recipe   a power-of-two block scale makes e4m3 a floating-point format: rounding under the row block's exponent and then
//                  under the column block's gives the bits of rounding once under the column block's, except for values that are subnormal
//                  under one of the two (tests/test_cpu_linear_mxfp8_store_recipe.py: the weight gradient moves by <= 2.5e-6, L1-relative; bound 1e-5).
// Kernel of the MX store
//   mx_rows_to_cols_kernel   ONE launch, xq and xs read once, no atomics: a 128-token x 128-column tile per workgroup, 16-byte global loads along
//                  K (8 lanes = the 128 contiguous bytes of a row), a byte transpose through LDS (described at the kernel), mx_pack_block32 and
//                  store_cols_tile as in quant_cols_mx_kernel.
//
// MX dual quantiser (opt-in on the host: set_mx_dual_quant(True) under the MX backward): the upstream gradient dy feeds the data gradient as MX rows
// and the weight gradient as MX columns; one launch reads it once and writes both.  NORMATIVE, for finite inputs:
//   sv_quant_rows_cols_mx_e4m3   src [M, N] (row stride ld, bf16 or fp32) ->
//                  row_q [M][Np] + row_s [M][Np / 32], Np = roundup(N, 128): EQUAL to sv_quant_rows_mx_e4m3(src, .., Np) bit for bit (bytes N .. Np - 1
//                  zero, padding blocks byte 127);
//                  col_q [N][Mp] + col_s [N][Mp / 32], Mp = roundup(M, 128): EQUAL to sv_quant_cols_mx_e4m3(src, .., Mp) bit for bit (bytes M .. Mp - 1
//                  of every row zero, blocks wholly past M byte 127, a partly filled block takes the maximum of its valid rows);
//                  colsum[c] += sum_m src[m, c] of the unquantised values: one fp64 partial per workgroup (128 tokens), one fp32 atomicAdd per
//                  workgroup and column - the column quantiser's scheme.
//                  row_q = row_s = NULL: the column form alone.  mx_block_exp and pack4_e4m3_mx of common.h are the only copy of the rounding.
// Kernel of the MX dual quantiser
//   quant_rows_cols_mx_kernel   ONE launch, src read once, no memset, no atomics but colsum's: the re-blocker's 128-token x 128-column tile with
//                  16-byte global loads along the row; the row form leaves from the registers of the load (one lane exchange per block maximum,
//                  16-byte stores), the column form from the values staged in LDS (described at the kernel).  With Np and Mp multiples of 128 the
//                  four row blocks of a token and the four token blocks of a column lie inside the tile: no maximum crosses workgroups.
#include "common.h"
#include <atomic>
#include <type_traits>

namespace sv {

// FP8_ROW_TARGET, FP8_SCALE_MAX, fp8_row_scale and pack4_e4m3 live in common.h: the quantising LayerNorm (norm.hip) forms the same rows.

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// ---- row quantiser -------------------------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void load4_guarded(const T* row, int k, int K, bool vec, float (&v)[4]) {
  if (vec && k + 4 <= K) { ldnf<4>(row + k, v); return; }
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = (k + j < K) ? ldf(row + k + j) : 0.f;
}

template <typename T>
__global__ __launch_bounds__(256) void quant_rows_kernel(const T* __restrict__ src, int rows, int K, long long ld, uint8_t* __restrict__ dst, int Kp,
                                                         float* __restrict__ scales) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;                                   // whole waves leave: no barrier in this kernel
  const T* row = src + (size_t)r * ld;
  const bool vec = (((uintptr_t)row) & (4 * sizeof(T) - 1)) == 0;
  float m = 0.f;
  for (int k = lane * 4; k < K; k += 256) {
    float v[4];
    load4_guarded(row, k, K, vec, v);
    m = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(m, fmaxf(fabsf(v[2]), fabsf(v[3]))));
  }
  m = wave_max(m);
  const float s = fp8_row_scale(m);
  uint32_t* out = reinterpret_cast<uint32_t*>(dst + (size_t)r * Kp);
  for (int k = lane * 4; k < Kp; k += 256) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (k < K) load4_guarded(row, k, K, vec, v);
    out[k >> 2] = pack4_e4m3(v[0] * s, v[1] * s, v[2] * s, v[3] * s);
  }
  if (lane == 0) scales[r] = s;
}

// MX row quantiser: one wave per row, a lane holds 4 consecutive elements and 8 lanes one 32-element block; the block maximum is three lane
// exchanges inside the group of 8 (a group is past Kp as a whole or not at all).  Every lane writes its 4 bytes, the group's first lane the E8M0 byte.
template <typename T>
__global__ __launch_bounds__(256) void quant_rows_mx_kernel(const T* __restrict__ src, int rows, int K, long long ld, uint8_t* __restrict__ dst, int Kp,
                                                            uint8_t* __restrict__ scales) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;                                   // whole waves leave: no barrier in this kernel
  const T* row = src + (size_t)r * ld;
  const bool vec = (((uintptr_t)row) & (4 * sizeof(T) - 1)) == 0;
  uint32_t* out = reinterpret_cast<uint32_t*>(dst + (size_t)r * Kp);
  uint8_t* sc = scales + (size_t)r * (Kp >> 5);
  for (int k = lane * 4; k < Kp; k += 256) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (k < K) load4_guarded(row, k, K, vec, v);
    float m = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));
    m = fmaxf(m, __shfl_xor(m, 1)); m = fmaxf(m, __shfl_xor(m, 2)); m = fmaxf(m, __shfl_xor(m, 4));
    const int E = mx_block_exp(m);
    out[k >> 2] = pack4_e4m3_mx(v[0], v[1], v[2], v[3], E);
    if ((lane & 7) == 0) sc[k >> 5] = (uint8_t)(E + 127);
  }
}

// ---- GEMM ----------------------------------------------------------------------------------------------------------------------------
// One by-value argument struct per GEMM kind.  MX selects the scale operands: E8M0 bytes [rows][pitch / 32] in place of one fp32 scale per row.
template <bool MX> using LfScale = std::conditional_t<MX, uint8_t, float>;

template <bool MX> struct LinArgs {
  const uint8_t* xq; const LfScale<MX>* sx; const uint8_t* wq; const LfScale<MX>* sw; void* out;
  int M, N, Kp;
  const float* bias; const void* residual; int ldr; const float* row_scale; int rows_per_scale; void* pre_act; int act; float slope; int ldc;
  uint8_t* q_out; uint8_t* qs_out;   // MX: [M][N] e4m3 bytes and [M][N / 32] scale bytes of the stored output (N % 128 == 0, no residual), or both null
};
template <bool MX> struct DgradArgs {    // dx[M, K] = dy[M, N] W[N, K]: dy rows and W^T rows, contraction over Np
  const uint8_t* dq; const LfScale<MX>* sd; const uint8_t* wtq; const LfScale<MX>* swt; void* out;
  int M, K, Np;
  const void* act_grad_src; int act_grad_kind; float slope; int ldc;
};
template <bool MX> struct WgradArgs {    // dw[N, K] += dy^T[N, M] x[M, K]: dy^T rows and x^T rows, contraction over Mp
  const uint8_t* dyt; const LfScale<MX>* sdc; const uint8_t* xt; const LfScale<MX>* sxc; float* dw;
  float* ws;                             // MX: [splits][N][K] fp32, used when splits > 1
  int N, K, Mp, ldw, splits;
};

constexpr int LF_BM = 128, LF_BN = 128, LF_BK = 128, LF_PITCH = 128, LF_TILE = LF_BM * LF_PITCH;   // bytes
constexpr int LF_SCALES = 4 * (LF_BM + LF_BN);             // MX: the scale dwords of one k-step, x rows then W rows
__device__ __forceinline__ int lf_swz(int r) { return ((r >> 1) & 1) | (((r >> 3) & 1) << 2); }   // position of piece c in row r: c ^ lf_swz(r)

// The contraction core every fp8 GEMM of this file runs: acc += sum over the k-steps ks0 .. ks1 - 1 (128 bytes each) of the 128 x 128 tile
// at (row0, col0) of xq [M][pitch] times wq [N][pitch]^T.  Staging, the swizzled LDS image, the fragment reads and the MFMA block have this
// one copy.  On return lane (lr, lg) of wave (wm, wn) holds, in acc[nt][mt][i], row row0 + 64 wm + 16 mt + lr and column
// col0 + 64 wn + 16 lg + 4 nt + i: 16 consecutive columns per row.  Rows past M / N read a clamped (valid) row; the caller's epilogue skips them.
// MX (compile time): the operands carry E8M0 block scales, xsc [M][pitch / 32] and wsc [N][pitch / 32] bytes.  The four scale bytes of a row and
// k-step are one aligned dword; thread t < 128 stages the dword of x tile row t, thread 128 + t that of W tile row t (the W rows' permutation),
// into LF_SCALES bytes behind the operand tiles of each buffer.  Lane maps of the scaled MFMA with e4m3 operands, as measured
// (scripts/probes/mfma_scale_lane_probe.hip) and pinned by the exact-integer test with block scales (tests/test_gpu_linear_mxfp8.py):
//   scales  lane l's selected byte scales row / column l & 15 and the 32 k-values k = 32 (l >> 4) .. + 31 of the k-step;
//   data    lane l's registers 0-3 hold k = 16 (l >> 4) .. + 15 and its registers 4-7 k = 64 + 16 (l >> 4) .. + 15 - two K = 64 halves, NOT 32
//           consecutive bytes: a lane's scale byte covers 16 of its own bytes and 16 of a neighbouring lane group's.  The unit-scale form
//           never notices (both operands permute k alike); here lane (lr, lg) takes pieces lg and 4 + lg of its row, shifts the row's
//           scale dword by 8 lg and passes byte 0 (op-sel 0).
// Without MX both scales are the constant 1.0 and nothing is staged.
template <bool MX = false>
__device__ __forceinline__ void lf_contract(const uint8_t* __restrict__ xq, int M, const uint8_t* __restrict__ wq, int N, size_t pitch, int row0, int col0,
                                            int ks0, int ks1, uint8_t* __restrict__ lf_smem, f32x4 (&acc)[4][4],
                                            const uint8_t* __restrict__ xsc = nullptr, const uint8_t* __restrict__ wsc = nullptr) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;                 // the wave's 64 x 64 quarter of the tile
  const int lr = lane & 15, lg = lane >> 4;

  // staging: a tile is 128 rows x 8 pieces of 16 bytes; thread t moves pieces t, t + 256, t + 512, t + 768 of each operand
  const uint8_t* gx[4]; const uint8_t* gw[4]; int so[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int pc = tid + 256 * i, r = pc >> 3, c = pc & 7;
    // W rows are permuted on their way into LDS: tile row 64 wn + 16 nt + i (row i of MFMA block nt) holds output column 64 wn + 16 (i >> 2)
    // + 4 nt + (i & 3), so that a lane's four blocks hold 16 CONSECUTIVE columns (epilogues below).  Fragment reads and banks are unaffected.
    const int nl = (r & 64) + ((r & 15) >> 2) * 16 + ((r >> 4) & 3) * 4 + (r & 3);
    const int m = min(row0 + r, M - 1), n = min(col0 + nl, N - 1);   // past the end: any valid row, the epilogue skips it
    gx[i] = xq + (size_t)m * pitch + c * 16;
    gw[i] = wq + (size_t)n * pitch + c * 16;
    // MX: the lane's fragment must be the hardware's k order (below), pieces lg and 4 + lg of the row; they are stored where the plain
    // image keeps pieces 2 lg and 2 lg + 1, so the fragment reads and their bank pattern are the same in both forms
    const int cp = MX ? (((c & 3) << 1) | (c >> 2)) : c;
    so[i] = r * LF_PITCH + (cp ^ lf_swz(r)) * 16;
  }
  i32x4 rx[4], rw[4];
  const uint8_t* gs = nullptr;                             // MX: this thread's row of scale bytes
  uint32_t rs = 0;
  if constexpr (MX) {
    const int r = tid & 127;
    const int nl = (r & 64) + ((r & 15) >> 2) * 16 + ((r >> 4) & 3) * 4 + (r & 3);
    gs = tid < 128 ? xsc + (size_t)min(row0 + r, M - 1) * (pitch >> 5) : wsc + (size_t)min(col0 + nl, N - 1) * (pitch >> 5);
  }
  auto load_step = [&](size_t k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      rx[i] = *reinterpret_cast<const i32x4*>(gx[i] + k0);
      rw[i] = *reinterpret_cast<const i32x4*>(gw[i] + k0);
    }
    if constexpr (MX) rs = *reinterpret_cast<const uint32_t*>(gs + (k0 >> 5));
  };
  auto store_step = [&](int buf) {
    uint8_t* xs = lf_smem + buf * 2 * LF_TILE;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<i32x4*>(xs + so[i]) = rx[i];
      *reinterpret_cast<i32x4*>(xs + LF_TILE + so[i]) = rw[i];
    }
    if constexpr (MX) reinterpret_cast<uint32_t*>(lf_smem + 4 * LF_TILE + buf * LF_SCALES)[tid] = rs;
  };

  const int o_lo = ((2 * lg) ^ lf_swz(lr)) * 16, o_hi = ((2 * lg + 1) ^ lf_swz(lr)) * 16;   // the lane's two 16-byte pieces of a row
  load_step((size_t)ks0 * LF_BK);
  store_step(0);
  __syncthreads();
  for (int ks = ks0; ks < ks1; ++ks) {
    const int buf = (ks - ks0) & 1;
    if (ks + 1 < ks1) load_step((size_t)(ks + 1) * LF_BK);   // in flight during the MFMAs below
    const uint8_t* xs = lf_smem + buf * 2 * LF_TILE + (wm * 64 + lr) * LF_PITCH;   // rows + 16 mt share bits 1 and 3 with lr: one swizzle per lane
    const uint8_t* ws = lf_smem + buf * 2 * LF_TILE + LF_TILE + (wn * 64 + lr) * LF_PITCH;
    i32x8 fx[4];
    int sxb[4];                                            // MX: the E8M0 byte of this lane's block of x row 16 mt + lr, in byte 0
    const uint32_t* ss = reinterpret_cast<const uint32_t*>(lf_smem + 4 * LF_TILE + buf * LF_SCALES);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const i32x4 lo = *reinterpret_cast<const i32x4*>(xs + mt * 16 * LF_PITCH + o_lo), hi = *reinterpret_cast<const i32x4*>(xs + mt * 16 * LF_PITCH + o_hi);
      fx[mt] = (i32x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      if constexpr (MX) sxb[mt] = (int)(ss[wm * 64 + mt * 16 + lr] >> (8 * lg));
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const i32x4 lo = *reinterpret_cast<const i32x4*>(ws + nt * 16 * LF_PITCH + o_lo), hi = *reinterpret_cast<const i32x4*>(ws + nt * 16 * LF_PITCH + o_hi);
      const i32x8 fw = (i32x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {   // A = W (rows of D = output columns), B = x: the lane holds 4 consecutive output columns
        if constexpr (MX) {
          const int swb = (int)(ss[128 + wn * 64 + nt * 16 + lr] >> (8 * lg));
          acc[nt][mt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw, fx[mt], acc[nt][mt], 0, 0, 0, swb, 0, sxb[mt]);
        } else {
          acc[nt][mt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw, fx[mt], acc[nt][mt], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
        }
      }
    }
    if (ks + 1 < ks1) store_step(buf ^ 1);                 // the other buffer: its readers passed the barrier of the previous step
    __syncthreads();
  }
}

// Where a lane stands in its workgroup's 128 x 128 output tile: wave (wm, wn) owns a 64 x 64 quarter, lane (lr, lg) of it the rows
// row0 + 64 wm + 16 mt + lr and the 16 consecutive columns from c0 (lf_contract's result map).
struct LfTile { int wm, wn, lr, lg, row0, col0, c0; };

// The part every GEMM kernel of this file begins with: tile blockIdx.x of a [R] x [C] output (consecutive workgroups share the row operand),
// the LDS buffers, and acc = the contraction of a [R][pitch] with b [C][pitch] over the k-steps ks0 .. ks1 - 1.
// LDS: [2 buffers][a tile, b tile][128 rows][128 bytes, swizzled] (+ [2][scale dwords] under MX).
template <bool MX>
__device__ __forceinline__ LfTile lf_tile_contract(const uint8_t* __restrict__ a, const LfScale<MX>* __restrict__ sa, int R, const uint8_t* __restrict__ b,
                                                   const LfScale<MX>* __restrict__ sb, int C, int pitch, int ks0, int ks1, f32x4 (&acc)[4][4]) {
  __shared__ __attribute__((aligned(16))) uint8_t lf_smem[2 * 2 * LF_TILE + (MX ? 2 * LF_SCALES : 0)];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tiles_c = (C + LF_BN - 1) / LF_BN;
  LfTile t;
  t.wm = wave >> 1; t.wn = wave & 1; t.lr = lane & 15; t.lg = lane >> 4;
  t.row0 = (blockIdx.x / tiles_c) * LF_BM; t.col0 = (blockIdx.x % tiles_c) * LF_BN;
  t.c0 = t.col0 + t.wn * 64 + t.lg * 16;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  if constexpr (MX) lf_contract<true>(a, R, b, C, (size_t)pitch, t.row0, t.col0, ks0, ks1, lf_smem, acc, sa, sb);
  else lf_contract(a, R, b, C, (size_t)pitch, t.row0, t.col0, ks0, ks1, lf_smem, acc);
  return t;
}

// The walk over a lane's outputs (forward and weight gradient; the data gradient writes its own out, see there).  A kernel whose lane has
// columns (c0 < C) calls lf_col_scales once and then, for mt = 0 .. 3, lf_row: false when the lane's row m of block mt is past R, else v = the
// values of the columns c0 .. c0 + 15 of row m (columns >= C are the caller's to skip).  Per-row recipe: val = acc / (sa[m] sb[c]), fp32 IEEE
// division; MX: val = acc, the MFMA applied both block scales, and sc stays unset.
template <bool MX>
__device__ __forceinline__ void lf_col_scales(const LfTile& t, const LfScale<MX>* __restrict__ sb, int C, float (&sc)[16]) {
  if constexpr (!MX) {
#pragma unroll
    for (int j = 0; j < 16; ++j) sc[j] = sb[min(t.c0 + j, C - 1)];
  }
}
template <bool MX>
__device__ __forceinline__ bool lf_row(const LfTile& t, const f32x4 (&acc)[4][4], int mt, const LfScale<MX>* __restrict__ sa, int R,
                                       const float (&sc)[16], int& m, float (&v)[16]) {
  m = t.row0 + t.wm * 64 + mt * 16 + t.lr;
  if (m >= R) return false;
  if constexpr (MX) {
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = acc[j >> 2][mt][j & 3];
  } else {
    const float sm = sa[m];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = acc[j >> 2][mt][j & 3] / (sm * sc[j]);
  }
  return true;
}

// W consecutive elements <-> registers: common.h's ldnf / stnf, and ldf / stf for a single element
template <int W, typename T> __device__ __forceinline__ void ld_piece(const T* p, float (&v)[W]) {
  if constexpr (W == 1) v[0] = ldf(p); else ldnf<W>(p, v);
}
template <int W, typename T> __device__ __forceinline__ void st_piece(T* p, const float (&v)[W]) {
  if constexpr (W == 1) stf(p, v[0]); else stnf<W>(p, v);
}

// A lane's 16 columns from c0, cut into pieces of W elements: body(integral_constant W, q) for each piece at columns c0 + q .. + W - 1 that
// begins inside C (callers pick W so that a piece is in range as a whole).  A guard per piece, not a break: the loop must unroll fully, q indexes
// registers.  lf_pieces picks W once per lane: CV (one 16-byte access) when `wide`, 4 when `quad`, else single elements.
template <int W, typename F>
__device__ __forceinline__ void lf_pieces_of(int c0, int C, F& body) {
#pragma unroll
  for (int q = 0; q < 16; q += W)
    if (c0 + q < C) body(std::integral_constant<int, W>{}, q);
}
template <int CV, typename F>
__device__ __forceinline__ void lf_pieces(bool wide, bool quad, int c0, int C, F&& body) {
  if (wide || (CV == 4 && quad)) lf_pieces_of<CV>(c0, C, body);
  else if (CV != 4 && quad) lf_pieces_of<4>(c0, C, body);
  else lf_pieces_of<1>(c0, C, body);
}

// ---- forward --------------------------------------------------------------------------------------------------------------------------------------
// MX = false: the per-row recipe.  MX = true: the MX recipe; out may then be null when q_out is given.  Emission: the stored row (after the
// activation, rounded to AT) is quantised as quant_rows_mx_kernel would quantise it; a 32-column block is the 16 + 16 columns of lanes lg and
// lg ^ 1 (lane ^ 16) of the same row, so one exchange gives its maximum.
// Epilogue on the registers: 16-byte pieces (8 bf16 / 4 fp32), 32 / 64 contiguous bytes per lane and row.
template <typename AT, bool FAST, bool MX = false>
__global__ __launch_bounds__(256, 2) void linear_fp8_kernel(const LinArgs<MX> p) {
  f32x4 acc[4][4];   // [column block nt][row block mt]
  const LfTile t = lf_tile_contract<MX>(p.xq, p.sx, p.M, p.wq, p.sw, p.N, p.Kp, 0, p.Kp / LF_BK, acc);

  AT* __restrict__ Y = static_cast<AT*>(p.out);
  AT* __restrict__ PRE = static_cast<AT*>(p.pre_act);
  const AT* __restrict__ RES = static_cast<const AT*>(p.residual);
  constexpr int CV = sizeof(AT) == 2 ? 8 : 4;              // elements of a 16-byte piece
  const bool vec4 = ((p.ldc | p.N) & 3) == 0 && (!RES || (p.ldr & 3) == 0);   // (base pointers: 4 elements, checked on the host)
  const bool vecw = ((p.ldc | p.N) & (CV - 1)) == 0 && (!RES || (p.ldr & (CV - 1)) == 0) &&
                    ((((uintptr_t)Y) | ((uintptr_t)PRE) | ((uintptr_t)RES)) & 15) == 0;
  if (t.c0 >= p.N) return;
  float bias[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) bias[j] = p.bias ? p.bias[min(t.c0 + j, p.N - 1)] : 0.f;
  float scol[16];
  lf_col_scales<MX>(t, p.sw, p.N, scol);
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    int m;
    float v[16];
    if (!lf_row<MX>(t, acc, mt, p.sx, p.M, scol, m, v)) continue;
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] += bias[j];
    if constexpr (MX) {
      if (p.q_out) {   // N % 128 == 0 and no residual (host): all 16 columns are in range and the stored value is act(v)
        float s[16], am = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          s[j] = (float)(AT)apply_act_t<FAST>(v[j], p.act, p.slope);
          am = fmaxf(am, fabsf(s[j]));
        }
        am = fmaxf(am, __shfl_xor(am, 16));                // the partner holds the same row: it is here whenever this lane is
        const int E = mx_block_exp(am);
        *reinterpret_cast<uint4*>(p.q_out + (size_t)m * p.N + t.c0) =
            make_uint4(pack4_e4m3_mx(s[0], s[1], s[2], s[3], E), pack4_e4m3_mx(s[4], s[5], s[6], s[7], E),
                       pack4_e4m3_mx(s[8], s[9], s[10], s[11], E), pack4_e4m3_mx(s[12], s[13], s[14], s[15], E));
        if ((t.lg & 1) == 0) p.qs_out[(size_t)m * (p.N >> 5) + (t.c0 >> 5)] = (uint8_t)(E + 127);
        if (!Y && !PRE) continue;                          // no backward follows: neither out nor pre_act is stored
      }
    }
    const float sc = (RES && p.row_scale) ? p.row_scale[m / p.rows_per_scale] : 1.f;
    const size_t o = (size_t)m * p.ldc + t.c0, orow = (size_t)m * p.ldr + t.c0;
    lf_pieces<CV>(vecw, vec4, t.c0, p.N, [&](auto w, int q) {
      constexpr int W = decltype(w)::value;
      float x[W];
#pragma unroll
      for (int j = 0; j < W; ++j) x[j] = v[q + j];
      if (PRE) st_piece(PRE + o + q, x);
      if constexpr (MX) { if (!Y) return; }                // MX store: pre_act and the emitted rows are all the backward reads
#pragma unroll
      for (int j = 0; j < W; ++j) x[j] = apply_act_t<FAST>(x[j], p.act, p.slope);
      if (RES) {
        float r[W];
        ld_piece(RES + orow + q, r);
#pragma unroll
        for (int j = 0; j < W; ++j) x[j] = r[j] + sc * x[j];
      }
      st_piece(Y + o + q, x);
    });
  }
}

// ---- data gradient: dx[M, K] = dy[M, N] W[N, K], the contraction runs over N -----------------------------------------------------------------
// The walk and the two piece widths are written out in this kernel, as they were before the other GEMM kernels came to share lf_row and
// lf_pieces: through either helper its epilogue compiles to other code and measures 0.5 - 2.4 % slower.  The layers with
// a short contraction (fc2: two k-steps) are all epilogue.
template <typename AT, bool FAST, bool MX = false>
__global__ __launch_bounds__(256, 2) void linear_fp8_dgrad_kernel(const DgradArgs<MX> p) {
  f32x4 acc[4][4];
  const LfTile t = lf_tile_contract<MX>(p.dq, p.sd, p.M, p.wtq, p.swt, p.K, p.Np, 0, p.Np / LF_BK, acc);
  const int wm = t.wm, lr = t.lr, row0 = t.row0;

  AT* __restrict__ Y = static_cast<AT*>(p.out);
  const AT* __restrict__ G = static_cast<const AT*>(p.act_grad_src);   // layout of the output
  constexpr int CV = sizeof(AT) == 2 ? 8 : 4;
  const bool vecw = ((p.ldc | p.K) & (CV - 1)) == 0 && ((((uintptr_t)Y) | ((uintptr_t)G)) & 15) == 0;
  const int c0 = t.c0;
  if (c0 >= p.K) return;
  float swk[16];
  if constexpr (!MX) {
#pragma unroll
    for (int j = 0; j < 16; ++j) swk[j] = p.swt[min(c0 + j, p.K - 1)];
  }
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int m = row0 + wm * 64 + mt * 16 + lr;
    if (m >= p.M) continue;
    float v[16];
    if constexpr (MX) {                                    // the MFMA applied both block scales: val = acc
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = acc[j >> 2][mt][j & 3];
    } else {
      const float sdm = p.sd[m];
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = acc[j >> 2][mt][j & 3] / (sdm * swk[j]);
    }
    const size_t o = (size_t)m * p.ldc + c0;
    if (vecw) {   // K % CV == 0: a piece is in range as a whole
#pragma unroll
      for (int q = 0; q < 16 / CV; ++q) {
        if (c0 + q * CV >= p.K) break;
        float t[CV];
#pragma unroll
        for (int j = 0; j < CV; ++j) t[j] = v[q * CV + j];
        if (G) {
          float a[CV];
          ldnf<CV>(G + o + q * CV, a);
#pragma unroll
          for (int j = 0; j < CV; ++j) t[j] *= act_grad_t<FAST>(a[j], p.act_grad_kind, p.slope);
        }
        stnf<CV>(Y + o + q * CV, t);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (c0 + j < p.K) {
          float t = v[j];
          if (G) t *= act_grad_t<FAST>(ldf(G + o + j), p.act_grad_kind, p.slope);
          stf(Y + o + j, t);
        }
      }
    }
  }
}

// ---- weight gradient: dw[N, K] += dy^T[N, M] x[M, K], the contraction runs over M (the tokens) ------------------------------------------------------
// Grid tiles(N) x tiles(K) x splits; split z contracts the k-steps [z nk / splits, (z + 1) nk / splits).  dy^T is the row operand and x^T the
// permuted one: a lane's 16 consecutive outputs run along k, the contiguous dimension of dw.
template <bool MX>
__global__ __launch_bounds__(256, 2) void linear_fp8_wgrad_kernel(const WgradArgs<MX> p) {
  const int nk = p.Mp / LF_BK, z = blockIdx.y;
  const int ks0 = (int)((long long)z * nk / p.splits), ks1 = (int)((long long)(z + 1) * nk / p.splits);   // splits <= nk: no share is empty
  f32x4 acc[4][4];
  const LfTile t = lf_tile_contract<MX>(p.dyt, p.sdc, p.N, p.xt, p.sxc, p.K, p.Mp, ks0, ks1, acc);   // rows of dw = n, columns = k
  if (t.c0 >= p.K) return;
  const bool one = p.splits == 1;
  // MX: NO atomics into dw.  One split: read-add-write into dw (row stride ldw), this lane is the only writer of its elements; more: a plain
  // store of the partial into slice z of the workspace (row stride K), which the reduce kernel folds into dw
  float* __restrict__ base = (!MX || one) ? p.dw : p.ws + (size_t)z * p.N * p.K;
  const int ldo = (!MX || one) ? p.ldw : p.K;
  const bool vec = ((ldo | p.K) & 3) == 0 && (((uintptr_t)base) & 15) == 0;   // K % 4 == 0: a 16-byte piece is in range as a whole
  float scol[16];
  lf_col_scales<MX>(t, p.sxc, p.K, scol);
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    int n;
    float v[16];
    if (!lf_row<MX>(t, acc, mt, p.sdc, p.N, scol, n, v)) continue;
    float* __restrict__ d = base + (size_t)n * ldo + t.c0;
    if constexpr (MX) {
      lf_pieces<4>(vec, false, t.c0, p.K, [&](auto w, int q) {
        constexpr int W = decltype(w)::value;
        float x[W], o[W];
        if (one) ld_piece(d + q, o);
#pragma unroll
        for (int j = 0; j < W; ++j) x[j] = one ? o[j] + v[q + j] : v[q + j];
        st_piece(d + q, x);
      });
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (t.c0 + j < p.K) {
          if (one) d[j] += v[j];                           // the only writer of this element
          else atomicAdd(d + j, v[j]);
        }
      }
    }
  }
}

// dw[n, k] += ws[0][n, k] + ws[1][n, k] + ...: the partials are added in ascending z, one after the other, so the sum does not depend on the run
__global__ __launch_bounds__(256) void linear_mxfp8_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, int N, int K, int ldw, int splits,
                                                                        int vec) {
  const size_t slice = (size_t)N * K;
  if (vec) {                                               // K % 4 == 0, ldw % 4 == 0, both bases 16-byte aligned
    const int kq = K >> 2;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)N * kq) return;
    const int n = (int)(i / kq), k = (int)(i % kq) * 4;
    float4* d = reinterpret_cast<float4*>(dw + (size_t)n * ldw + k);
    float4 s = *d;
    const float* w = ws + (size_t)n * K + k;
#pragma unroll 4
    for (int z = 0; z < splits; ++z) {
      const float4 t = *reinterpret_cast<const float4*>(w + z * slice);
      s = make_float4(s.x + t.x, s.y + t.y, s.z + t.z, s.w + t.w);
    }
    *d = s;
  } else {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= slice) return;
    const int n = (int)(i / K), k = (int)(i % K);
    float s = dw[(size_t)n * ldw + k];
    for (int z = 0; z < splits; ++z) s += ws[z * slice + i];
    dw[(size_t)n * ldw + k] = s;
  }
}

// ---- transposing quantisers: src [M, C] (row stride ld) -> dst [C][Mp] e4m3 bytes ---------------------------------------------------------------------
// Shared by all four: a tile of 128 rows x COLS columns leaves through an LDS image [column][COLS_PITCH dwords] (32 dwords = 128 rows, + 1:
// conflict-free on both sides - 32 consecutive columns x pitch 33 on the way in, 4 columns x 8 pieces on the way out).
constexpr int COLS_PITCH = 33;
constexpr int QC_COLS = 64, QC_ROWS1 = 256, QC_ROWS2 = 128;   // the column quantisers' tiles: pass 1, pass 2 / MX
constexpr int RB_ROWS = 128, RB_COLS = 128;                   // the re-blocker's and the dual quantiser's tile

// The way out of the image: 16-byte stores along M (COLS x 8 pieces over 256 threads); then thread t < COLS, for column c0 + t, the column's four
// E8M0 bytes of this tile as one aligned dword (sbytes [COLS], or null) and the column sum - the four fp64 partials ssum [4][COLS] of the
// workgroup, added in ascending order, as ONE fp32 atomicAdd (ssum or colsum null: none).  Columns >= C write nothing.
template <int COLS>
__device__ __forceinline__ void store_cols_tile(const uint32_t* tile, const uint32_t* sbytes, const double* ssum, int c0, int C, int m0, int Mp,
                                                uint8_t* __restrict__ dst, uint8_t* __restrict__ scales, float* __restrict__ colsum) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < COLS / 32; ++i) {
    const int pc = tid + 256 * i, col = pc >> 3, piece = pc & 7;
    if (c0 + col < C) {
      const uint32_t* t = tile + col * COLS_PITCH + piece * 4;
      *reinterpret_cast<uint4*>(dst + (size_t)(c0 + col) * Mp + m0 + piece * 16) = make_uint4(t[0], t[1], t[2], t[3]);
    }
  }
  if (tid < COLS && c0 + tid < C) {
    if (sbytes) reinterpret_cast<uint32_t*>(scales + (size_t)(c0 + tid) * (Mp >> 5))[m0 >> 7] = sbytes[tid];
    if (ssum && colsum) atomicAdd(colsum + c0 + tid, (float)(ssum[tid] + ssum[COLS + tid] + ssum[2 * COLS + tid] + ssum[3 * COLS + tid]));
  }
}

// One MX block: the maximum of 32 values of one column, mx_block_exp, 8 x pack4_e4m3_mx into registers; returns the exponent E (byte E + 127).
__device__ __forceinline__ int mx_pack_block32(const float (&v)[32], uint32_t (&pk)[8]) {
  float am = 0.f;
#pragma unroll
  for (int j = 0; j < 32; ++j) am = fmaxf(am, fabsf(v[j]));
  const int E = mx_block_exp(am);
#pragma unroll
  for (int i = 0; i < 8; ++i) pk[i] = pack4_e4m3_mx(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3], E);
  return E;
}
// ... and its place in the image: rows 32 b .. + 31 of column col, byte b of the column's scale dword
__device__ __forceinline__ void place_block32(uint32_t* tile, uint32_t* sbytes, int col, int b, const uint32_t (&pk)[8], int E) {
#pragma unroll
  for (int i = 0; i < 8; ++i) tile[col * COLS_PITCH + b * 8 + i] = pk[i];
  reinterpret_cast<uint8_t*>(sbytes)[col * 4 + b] = (uint8_t)(E + 127);
}

// per-row recipe, pass 1: amax[c] = max over the rows of |src[m, c]| as the bit pattern of the non-negative float (integer max = float max there),
// into a zeroed buffer; optionally colsum[c] += sum over the rows (fp64 partial per workgroup, one fp32 atomic per workgroup and column)
template <typename T>
__global__ __launch_bounds__(256) void quant_cols_amax_kernel(const T* __restrict__ src, int M, int C, long long ld, int* __restrict__ amax_bits,
                                                              float* __restrict__ colsum) {
  __shared__ float smax[4][QC_COLS];
  __shared__ double ssum[4][QC_COLS];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * QC_COLS + tx;
  const int m0 = blockIdx.y * QC_ROWS1, m1 = min(m0 + QC_ROWS1, M);
  float mx = 0.f;
  double sum = 0.0;
  if (c < C) {
    for (int m = m0 + ty; m < m1; m += 4) {
      const float v = ldf(src + (size_t)m * ld + c);
      mx = fmaxf(mx, fabsf(v));
      sum += (double)v;
    }
  }
  smax[ty][tx] = mx;
  ssum[ty][tx] = sum;
  __syncthreads();
  if (ty == 0 && c < C) {
    mx = fmaxf(fmaxf(smax[0][tx], smax[1][tx]), fmaxf(smax[2][tx], smax[3][tx]));
    atomicMax(amax_bits + c, __float_as_int(mx));
    if (colsum) atomicAdd(colsum + c, (float)(ssum[0][tx] + ssum[1][tx] + ssum[2][tx] + ssum[3][tx]));
  }
}

// between the passes: the bit pattern of amax becomes the scale, in place
__global__ void quant_cols_scale_kernel(float* __restrict__ scales, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) {
    const float m = scales[c];
    scales[c] = fp8_row_scale(m);
  }
}

// pass 2: a tile of 128 rows x 64 columns is scaled, rounded to e4m3 and transposed through the image.  Rows past M are zero bytes.
template <typename T>
__global__ __launch_bounds__(256) void quant_cols_write_kernel(const T* __restrict__ src, int M, int C, long long ld, const float* __restrict__ scales,
                                                               uint8_t* __restrict__ dst, int Mp) {
  __shared__ uint32_t tile[QC_COLS * COLS_PITCH];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c0 = blockIdx.x * QC_COLS, m0 = blockIdx.y * QC_ROWS2;
  const int c = c0 + tx;
  const float s = c < C ? scales[c] : 1.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {                            // thread (tx, ty): rows 32 ty + 4 i .. + 3 of column tx
    const int m = m0 + ty * 32 + i * 4;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (c < C && m + j < M) ? ldf(src + (size_t)(m + j) * ld + c) : 0.f;
    tile[tx * COLS_PITCH + ty * 8 + i] = pack4_e4m3(v[0] * s, v[1] * s, v[2] * s, v[3] * s);
  }
  __syncthreads();
  store_cols_tile<QC_COLS>(tile, nullptr, nullptr, c0, C, m0, Mp, dst, nullptr, nullptr);
}

// MX column quantiser: src [M, C] -> dst [C][Mp] e4m3 bytes + scales [C][Mp / 32] E8M0 bytes, equal to quant_rows_mx_kernel on the transposed tensor.
// The tile of quant_cols_write_kernel; thread (tx, ty) owns rows 32 ty .. + 31 of column tx, which is exactly one MX block: its 32 values stay in
// registers between the maximum and the packing, and src is read once.  Rows past M are zeros: a partly filled block takes the maximum of its valid
// rows, a block wholly past M is an all-zero block (byte 127).  colsum as in quant_cols_amax_kernel.
template <typename T>
__global__ __launch_bounds__(256) void quant_cols_mx_kernel(const T* __restrict__ src, int M, int C, long long ld, uint8_t* __restrict__ dst, int Mp,
                                                            uint8_t* __restrict__ scales, float* __restrict__ colsum) {
  __shared__ uint32_t tile[QC_COLS * COLS_PITCH];
  __shared__ uint32_t sbytes[QC_COLS];
  __shared__ double ssum[4 * QC_COLS];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c0 = blockIdx.x * QC_COLS, m0 = blockIdx.y * QC_ROWS2;
  const int c = c0 + tx, mb = m0 + ty * 32;
  float v[32];
#pragma unroll
  for (int j = 0; j < 32; ++j) v[j] = (c < C && mb + j < M) ? ldf(src + (size_t)(mb + j) * ld + c) : 0.f;
  if (colsum) {
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < 32; ++j) sum += (double)v[j];
    ssum[ty * QC_COLS + tx] = sum;
  }
  uint32_t pk[8];
  const int E = mx_pack_block32(v, pk);
  place_block32(tile, sbytes, tx, ty, pk, E);
  __syncthreads();
  store_cols_tile<QC_COLS>(tile, sbytes, ssum, c0, C, m0, Mp, dst, scales, colsum);
}

// MX re-blocker: the MX ROWS of a stored tensor (xq [M][Kp] bytes + xs [M][Kp / 32] scale bytes, a block = 32 columns of a row) become the MX COLUMN
// operand of the weight gradient (dst [K][Mp] bytes + scales [K][Mp / 32], a block = 32 tokens of a column) - see "MX store" in the header.
// One workgroup = 128 tokens x 128 columns, 16 KB in and 16 KB out.
//   load     thread t moves the 16-byte pieces t, t + 256, t + 512, t + 768 of the tile (8 lanes = the 128 contiguous bytes of one row) into a plain
//            [128][128]-byte LDS image (eight lanes of a ds_write_b128 cover the 32 banks once); t < 128 also stages the scale dword of row t (the
//            four k-blocks of the tile).  Rows past M are zero bytes.
//   compute  wave b owns tokens 32 b .. + 31; lane l owns column 64 u + l, u = 0, 1: one MX block per (lane, u).  It reads its 32 bytes down the
//            column (the 32 lanes of a group read 8 consecutive dwords of one row: no conflict), decodes byte 2^(s - 127) in fp32 (exact; the row's
//            scale dword comes from lane j of the wave by v_readlane) and packs the block under the column block's exponent.
//   store    the shared image and way out (store_cols_tile).
__global__ __launch_bounds__(256) void mx_rows_to_cols_kernel(const uint8_t* __restrict__ xq, int Kp, const uint8_t* __restrict__ xs, int M, int K,
                                                              uint8_t* __restrict__ dst, int Mp, uint8_t* __restrict__ scales) {
  __shared__ __attribute__((aligned(16))) uint8_t in[RB_ROWS * RB_COLS];   // [token][column] bytes
  __shared__ uint32_t srows[RB_ROWS];                        // [token]: the scale bytes of the tile's four k-blocks
  __shared__ uint32_t tile[RB_COLS * COLS_PITCH];
  __shared__ uint32_t sbytes[RB_COLS];
  const int tid = threadIdx.x, lane = tid & 63, b = tid >> 6;
  const int k0 = blockIdx.x * RB_COLS, m0 = blockIdx.y * RB_ROWS;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int pc = tid + 256 * i, r = pc >> 3, c = pc & 7;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (m0 + r < M) v = *reinterpret_cast<const uint4*>(xq + (size_t)(m0 + r) * Kp + k0 + c * 16);   // k0 + 127 < Kp: a whole piece is in range
    *reinterpret_cast<uint4*>(in + r * RB_COLS + c * 16) = v;
  }
  if (tid < RB_ROWS) srows[tid] = (m0 + tid < M) ? *reinterpret_cast<const uint32_t*>(xs + (size_t)(m0 + tid) * (Kp >> 5) + (k0 >> 5)) : 0x7f7f7f7fu;
  __syncthreads();
  const int srow = (int)srows[b * 32 + (lane & 31)];         // lane j (and j + 32) holds the scale dword of token 32 b + j
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int col = u * 64 + lane, sh = (col >> 5) * 8;    // the column's k-block inside the tile selects the byte of the scale dword
    float v[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const int s = (__builtin_amdgcn_readlane(srow, j) >> sh) & 0xff;
      v[j] = ldexpf(__builtin_amdgcn_cvt_f32_fp8((int)in[(b * 32 + j) * RB_COLS + col], 0), s - 127);
    }
    uint32_t pk[8];
    const int E = mx_pack_block32(v, pk);
    place_block32(tile, sbytes, col, b, pk, E);
  }
  __syncthreads();
  store_cols_tile<RB_COLS>(tile, sbytes, nullptr, k0, K, m0, Mp, dst, scales, nullptr);
}

// MX dual quantiser: ONE read of src [M, N] gives the MX ROW operand (row_q [M][Np] + row_s [M][Np / 32], equal to quant_rows_mx_kernel) and the MX
// COLUMN operand (col_q [N][Mp] + col_s [N][Mp / 32] + colsum, equal to quant_cols_mx_kernel) - see "MX dual quantiser" in the header.  One workgroup =
// 128 tokens x 128 columns (the re-blocker's tile); ROWS_OUT = false compiles the row work out (the column form alone, with this kernel's loader).
//   load     a chunk = 16 consecutive elements of one tile row (sizeof(T) 16-byte pieces: two for bf16, four for fp32); thread t moves the chunks t,
//            t + 256, t + 512, t + 768 (8 lanes = the 128 columns of one row).  A row that is not 16-byte aligned, and the chunk that crosses N, take
//            load4_guarded's per-element path.  Rows past M and columns >= N are zeros.  The chunk goes into a plain [128][128] LDS image of T
//            as it was loaded (the stored values, no conversion).
//   rows     from the registers of the load: a 32-element block is the chunks of lanes c and c ^ 1, so its maximum is one lane exchange; a lane packs
//            its 16 bytes (one 16-byte store) and the even lane writes the E8M0 byte.  Rows past M write nothing; columns N .. Np - 1 are the padding
//            (zero bytes, byte 127), written like any other chunk.
//   columns  mx_rows_to_cols_kernel's compute and store on the staged values: wave b owns tokens 32 b .. + 31, lane l columns l and 64 + l, one MX
//            block per (lane, column) read down the tile (a wave reads 64 consecutive elements of one row: no conflict); fp64 column sums as in
//            quant_cols_mx_kernel.  The 8 packed dwords, the exponent and the sum wait in registers for a barrier, after which the image, the scale
//            dwords and the partial sums take the place of the input image: LDS is 32 KB (bf16) / 64 KB (fp32).
//            Columns >= N write nothing; rows past M were loaded as zeros and leave as the zero bytes of the column rows.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ float dq_elem(const u32x4 (&p)[sizeof(T)], int j) {   // element j of a chunk held as raw 16-byte pieces
  if constexpr (sizeof(T) == 4) return __uint_as_float(p[j >> 2][j & 3]);
  else return __uint_as_float((j & 1) ? (p[j >> 3][(j >> 1) & 3] & 0xffff0000u) : (p[j >> 3][(j >> 1) & 3] << 16));
}

template <typename T, bool ROWS_OUT>
__global__ __launch_bounds__(256) void quant_rows_cols_mx_kernel(const T* __restrict__ src, int M, int N, long long ld, uint8_t* __restrict__ row_q, int Np,
                                                                 uint8_t* __restrict__ row_s, uint8_t* __restrict__ col_q, int Mp,
                                                                 uint8_t* __restrict__ col_s, float* __restrict__ colsum) {
  constexpr int P = sizeof(T);                             // 16-byte pieces per chunk
  constexpr int IN_BYTES = RB_ROWS * RB_COLS * (int)sizeof(T);
  constexpr int SUM_BYTES = 4 * RB_COLS * 8, TILE_BYTES = RB_COLS * COLS_PITCH * 4, OUT_BYTES = SUM_BYTES + TILE_BYTES + RB_COLS * 4;
  __shared__ __attribute__((aligned(16))) uint8_t smem[IN_BYTES > OUT_BYTES ? IN_BYTES : OUT_BYTES];
  const T* in = reinterpret_cast<const T*>(smem);          // [token][column], then (after the second barrier):
  double* ssum = reinterpret_cast<double*>(smem);          // [4 token blocks][column]
  uint32_t* tile = reinterpret_cast<uint32_t*>(smem + SUM_BYTES);
  uint32_t* sbytes = reinterpret_cast<uint32_t*>(smem + SUM_BYTES + TILE_BYTES);
  const int tid = threadIdx.x, lane = tid & 63, b = tid >> 6;
  const int k0 = blockIdx.x * RB_COLS, m0 = blockIdx.y * RB_ROWS;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ch = tid + 256 * i, r = ch >> 3, c = ch & 7;
    const int m = m0 + r, k = k0 + 16 * c;
    u32x4 raw[P];
#pragma unroll
    for (int p = 0; p < P; ++p) raw[p] = u32x4{0u, 0u, 0u, 0u};
    if (m < M && k < N) {
      const T* row = src + (size_t)m * ld;
      if ((((uintptr_t)row) & 15) == 0 && k + 16 <= N) {
#pragma unroll
        for (int p = 0; p < P; ++p) raw[p] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const uint8_t*>(row + k) + 16 * p);
      } else {
        const bool vec = (((uintptr_t)row) & (4 * sizeof(T) - 1)) == 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float v[4] = {0.f, 0.f, 0.f, 0.f};
          if (k + 4 * q < N) load4_guarded(row, k + 4 * q, N, vec, v);
          if constexpr (sizeof(T) == 4) {
            raw[q] = u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
          } else {                                         // the floats came from bf16: their low halves are zero
            raw[q >> 1][2 * (q & 1)] = (__float_as_uint(v[0]) >> 16) | __float_as_uint(v[1]);
            raw[q >> 1][2 * (q & 1) + 1] = (__float_as_uint(v[2]) >> 16) | __float_as_uint(v[3]);
          }
        }
      }
    }
#pragma unroll
    for (int p = 0; p < P; ++p) *reinterpret_cast<u32x4*>(smem + ((size_t)r * RB_COLS + 16 * c) * sizeof(T) + 16 * p) = raw[p];
    if constexpr (ROWS_OUT) {
      float v[16];
      float am = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) { v[j] = dq_elem<T>(raw, j); am = fmaxf(am, fabsf(v[j])); }
      am = fmaxf(am, __shfl_xor(am, 1));
      const int E = mx_block_exp(am);
      u32x4 o;
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = pack4_e4m3_mx(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3], E);
      if (m < M) {                                         // k + 15 < Np: the grid covers Np / 128 column tiles
        *reinterpret_cast<u32x4*>(row_q + (size_t)m * Np + k) = o;
        if ((c & 1) == 0) row_s[(size_t)m * (Np >> 5) + (k >> 5)] = (uint8_t)(E + 127);
      }
    }
  }
  __syncthreads();
  uint32_t pk[2][8];
  int Eb[2];
  double sum[2] = {0.0, 0.0};
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    float v[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) v[j] = ldf(in + (b * 32 + j) * RB_COLS + u * 64 + lane);
    if (colsum) {
#pragma unroll
      for (int j = 0; j < 32; ++j) sum[u] += (double)v[j];
    }
    Eb[u] = mx_pack_block32(v, pk[u]);
  }
  __syncthreads();                                         // every wave has read the input image: the output images take its place
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    place_block32(tile, sbytes, u * 64 + lane, b, pk[u], Eb[u]);
    if (colsum) ssum[b * RB_COLS + u * 64 + lane] = sum[u];
  }
  __syncthreads();
  store_cols_tile<RB_COLS>(tile, sbytes, ssum, k0, N, m0, Mp, col_q, col_s, colsum);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------
static std::atomic<long long> linear_fp8_launches{0}, linear_mxfp8_launches{0};
static std::atomic<long long> linear_fp8_bwd_launches[2], linear_mxfp8_bwd_launches[2];   // data gradient, weight gradient
static std::atomic<long long> quant_rows_mx_launches{0}, quant_cols_mx_launches{0}, mx_rows_to_cols_launches{0}, quant_rows_cols_mx_launches{0};

// a clean launch moves the entry point's counter (null: the entry point has none)
static int finish_launch(const char* fn, std::atomic<long long>* counter) {
  const int rc = check_launch(fn);
  if (rc == SV_OK && counter) counter->fetch_add(1, std::memory_order_relaxed);
  return rc;
}

// the epilogue forms the forward kernel serves; `why` receives the reason of a refusal
static bool linear_fp8_epilogue_ok(const sv_epilogue* e, int N, const char** why) {
  *why = nullptr;
  if (!e) *why = "null epilogue";
  else if (e->stats) *why = "per-channel statistics (stats) are not served";
  else if (e->act_grad_src) *why = "an activation-gradient source (act_grad_src) is not served";
  else if (e->act != SV_ACT_NONE && e->act != SV_ACT_GELU) *why = "only SV_ACT_NONE and SV_ACT_GELU are served";
  else if (e->col_off != 0) *why = "col_off must be 0";
  else if (e->ldc < N) *why = "ldc < N";
  else if (e->residual && e->ldr < N) *why = "ldr < N";
  return *why == nullptr;
}

// the epilogue forms the data-gradient kernel serves
static bool linear_fp8_dgrad_epilogue_ok(const sv_epilogue* e, int K, const char** why) {
  *why = nullptr;
  if (!e) *why = "null epilogue";
  else if (e->stats) *why = "per-channel statistics (stats) are not served";
  else if (e->bias) *why = "a bias is not served";
  else if (e->residual || e->row_scale) *why = "a residual / row_scale is not served";
  else if (e->pre_act) *why = "pre_act is not served";
  else if (e->act != SV_ACT_NONE) *why = "an activation is not served";
  else if (e->act_grad_src && e->act_grad_kind != SV_ACT_GELU) *why = "only SV_ACT_GELU is served as act_grad_kind";
  else if (e->col_off != 0) *why = "col_off must be 0";
  else if (e->ldc < K) *why = "ldc < K";
  return *why == nullptr;
}

// What the quantiser entry points ask of their operands, in one place.  Every refusal names the entry point (fn) and the operands as its
// signature does; the alignment of the outputs is asked by each entry point under its own pointer names.
struct QuantSrc { const char* fn; const void* src; int dtype; const char* rn; int rows; const char* cn; int cols; int ld; };
static int require_quant_source(const QuantSrc& q) {       // a bf16 / fp32 source of rows x cols elements with row stride ld
  SV_REQUIRE(q.dtype == SV_F32 || q.dtype == SV_BF16, "%s: bad source dtype %d", q.fn, q.dtype);
  SV_REQUIRE(q.rows > 0 && q.cols > 0 && q.ld >= q.cols, "%s: %s (%d) and %s (%d) must be positive, ld (%d) >= %s", q.fn, q.rn, q.rows, q.cn, q.cols, q.ld, q.cn);
  return SV_OK;
}
static int require_padded(const char* fn, const char* pn, int P, const char* ln, int L) {   // the padded length of a quantised dimension
  SV_REQUIRE(P == cdiv(L, 128) * 128, "%s: %s (%d) must be %s (%d) rounded up to a multiple of 128", fn, pn, P, ln, L);
  return SV_OK;
}
static bool quant_src_aligned(const void* src, int dtype) { return ((uintptr_t)src & (dtype == SV_BF16 ? 1 : 3)) == 0; }

// sv_linear_fp8 and sv_linear_mxfp8: the same checks, tile count and storage dispatch; what only the MX form has is asked under MX
template <bool MX>
static int launch_linear(const char* fn, std::atomic<long long>& counter, const void* xq, const void* xs, const void* wq, const void* ws, void* out, int M,
                         int K, int N, const sv_epilogue* e, void* q_out, void* qs_out, int act_dtype, void* stream) {
  SV_REQUIRE(xq && xs && wq && ws && e && (MX || out), "%s: null argument", fn);
  if constexpr (MX) {
    SV_REQUIRE(out || q_out, "%s: out may be null only when q_out is given", fn);
    SV_REQUIRE((q_out != nullptr) == (qs_out != nullptr), "%s: q_out and qs_out go together", fn);
  }
  SV_REQUIRE_ACT(act_dtype);
  SV_REQUIRE(M > 0 && K > 0 && N > 0, "%s: M (%d), K (%d), N (%d) must be positive", fn, M, K, N);
  const char* why;
  SV_REQUIRE(linear_fp8_epilogue_ok(e, N, &why), "%s: %s", fn, why);
  if constexpr (MX) {
    SV_REQUIRE(!q_out || (!e->residual && !e->row_scale), "%s: the emission of the output's MX rows is not served with a residual", fn);
    SV_REQUIRE(!q_out || N % 128 == 0, "%s: the emission of the output's MX rows needs N (%d) %% 128 == 0", fn, N);
    // pre_act exists for the derivative of the activation: without an activation it would be the unstored out under another name
    SV_REQUIRE(out || !e->pre_act || e->act != SV_ACT_NONE, "%s: pre_act without out is served only in front of an activation", fn);
  }
  SV_REQUIRE((((uintptr_t)xq | (uintptr_t)wq | (uintptr_t)q_out) & 15) == 0, "%s: quantised operands must be 16-byte aligned", fn);
  SV_REQUIRE(!MX || (((uintptr_t)xs | (uintptr_t)ws | (uintptr_t)qs_out) & 3) == 0, "%s: scale bytes must be 4-byte aligned", fn);
  const uintptr_t amask = act_dtype == SV_BF16 ? 7 : 15;
  SV_REQUIRE((((uintptr_t)out | (uintptr_t)e->residual | (uintptr_t)e->pre_act) & amask) == 0, "%s: out / residual / pre_act must be aligned to 4 elements", fn);
  const long long tiles = (long long)cdiv(M, LF_BM) * cdiv(N, LF_BN);
  SV_REQUIRE(tiles < (1ll << 31), "%s: too many tiles", fn);
  const LinArgs<MX> a{static_cast<const uint8_t*>(xq), static_cast<const LfScale<MX>*>(xs), static_cast<const uint8_t*>(wq), static_cast<const LfScale<MX>*>(ws),
                      out, M, N, cdiv(K, LF_BK) * LF_BK, e->bias, e->residual, e->ldr, e->row_scale, e->rows_per_scale > 0 ? e->rows_per_scale : 1,
                      e->pre_act, e->act, e->slope, e->ldc, static_cast<uint8_t*>(q_out), static_cast<uint8_t*>(qs_out)};
  SV_DISPATCH_ACT(act_dtype, hipLaunchKernelGGL((linear_fp8_kernel<AT, sizeof(AT) == 2, MX>), dim3((unsigned)tiles), dim3(256), 0, static_cast<hipStream_t>(stream), a););
  return finish_launch(fn, &counter);
}

// sv_linear_fp8_dgrad and sv_linear_mxfp8_dgrad
template <bool MX>
static int launch_dgrad(const char* fn, std::atomic<long long>& counter, const void* dq, const void* ds, const void* wtq, const void* wts, void* dx, int M,
                        int N, int K, const sv_epilogue* e, int act_dtype, void* stream) {
  SV_REQUIRE(dq && ds && wtq && wts && dx && e, "%s: null argument", fn);
  SV_REQUIRE_ACT(act_dtype);
  SV_REQUIRE(M > 0 && N > 0 && K > 0, "%s: M (%d), N (%d), K (%d) must be positive", fn, M, N, K);
  const char* why;
  SV_REQUIRE(linear_fp8_dgrad_epilogue_ok(e, K, &why), "%s: %s", fn, why);
  SV_REQUIRE((((uintptr_t)dq | (uintptr_t)wtq) & 15) == 0, "%s: quantised operands must be 16-byte aligned", fn);
  SV_REQUIRE(!MX || (((uintptr_t)ds | (uintptr_t)wts) & 3) == 0, "%s: scale bytes must be 4-byte aligned", fn);
  const uintptr_t amask = act_dtype == SV_BF16 ? 1 : 3;
  SV_REQUIRE((((uintptr_t)dx | (uintptr_t)e->act_grad_src) & amask) == 0, "%s: dx / act_grad_src are not aligned to their element", fn);
  const long long tiles = (long long)cdiv(M, LF_BM) * cdiv(K, LF_BN);
  SV_REQUIRE(tiles < (1ll << 31), "%s: too many tiles", fn);
  const DgradArgs<MX> a{static_cast<const uint8_t*>(dq), static_cast<const LfScale<MX>*>(ds), static_cast<const uint8_t*>(wtq),
                        static_cast<const LfScale<MX>*>(wts), dx, M, K, cdiv(N, LF_BK) * LF_BK, e->act_grad_src, e->act_grad_kind, e->slope, e->ldc};
  SV_DISPATCH_ACT(act_dtype, hipLaunchKernelGGL((linear_fp8_dgrad_kernel<AT, sizeof(AT) == 2, MX>), dim3((unsigned)tiles), dim3(256), 0, static_cast<hipStream_t>(stream), a););
  return finish_launch(fn, &counter);
}

// the number of splits a weight-gradient call resolves to, under either recipe: the request (0 = two workgroups for each of 256 CUs), at most one
// per 128 tokens and the grid's y limit
static int linear_wgrad_splits(int M, int N, int K, int splits) {
  const long long tiles = (long long)cdiv(N, LF_BM) * cdiv(K, LF_BN);
  const int nk = cdiv(M, LF_BK);
  if (splits == 0) splits = (int)((2 * 256 + tiles - 1) / tiles);
  splits = splits < nk ? splits : nk;
  return splits > 65535 ? 65535 : splits;
}

// sv_linear_fp8_wgrad and sv_linear_mxfp8_wgrad; the workspace and the reduce launch are the MX form's
template <bool MX>
static int launch_wgrad(const char* fn, std::atomic<long long>& counter, const void* dyt, const void* dys, const void* xt, const void* xs, float* dw, int M, int N,
                        int K, int ldw, int splits, float* workspace, void* stream) {
  SV_REQUIRE(dyt && dys && xt && xs && dw, "%s: null argument", fn);
  SV_REQUIRE(M > 0 && N > 0 && K > 0 && ldw >= K, "%s: M (%d), N (%d), K (%d) must be positive, ldw (%d) >= K", fn, M, N, K, ldw);
  SV_REQUIRE(splits >= 0, "%s: splits (%d) must be >= 0", fn, splits);
  SV_REQUIRE((((uintptr_t)dyt | (uintptr_t)xt) & 15) == 0 && (((MX ? (uintptr_t)dys | (uintptr_t)xs : 0) | (uintptr_t)dw) & 3) == 0, "%s: operands are not aligned", fn);
  if constexpr (MX) SV_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace must be 16-byte aligned", fn);
  const long long tiles = (long long)cdiv(N, LF_BM) * cdiv(K, LF_BN);
  SV_REQUIRE(tiles < (1ll << 31), "%s: too many tiles", fn);
  splits = linear_wgrad_splits(M, N, K, splits);
  if constexpr (MX) SV_REQUIRE(splits == 1 || workspace, "%s: %d splits need a workspace of sv_linear_mxfp8_wgrad_workspace_floats floats", fn, splits);
  const WgradArgs<MX> a{static_cast<const uint8_t*>(dyt), static_cast<const LfScale<MX>*>(dys), static_cast<const uint8_t*>(xt),
                        static_cast<const LfScale<MX>*>(xs), dw, workspace, N, K, cdiv(M, LF_BK) * LF_BK, ldw, splits};
  int vec = 0;                                             // MX: the reduce kernel's 16-byte form and its work items
  size_t items = 0;
  if constexpr (MX) {
    vec = ((K | ldw) & 3) == 0 && ((uintptr_t)dw & 15) == 0;
    items = vec ? (size_t)N * (K >> 2) : (size_t)N * K;
    SV_REQUIRE(items / 256 + 1 < (1ull << 31), "%s: dw is too large", fn);
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(linear_fp8_wgrad_kernel<MX>, dim3((unsigned)tiles, (unsigned)splits), dim3(256), 0, s, a);
  if constexpr (MX) {
    if (splits > 1) hipLaunchKernelGGL(linear_mxfp8_wgrad_reduce_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, workspace, dw, N, K, ldw, splits, vec);
  }
  return finish_launch(fn, &counter);
}

}  // namespace sv

using namespace sv;

// ---- counters and capability queries -------------------------------------------------------------------------------------------------------------
extern "C" long long sv_linear_fp8_launches(void) { return linear_fp8_launches.load(std::memory_order_relaxed); }
extern "C" long long sv_linear_mxfp8_launches(void) { return linear_mxfp8_launches.load(std::memory_order_relaxed); }
extern "C" long long sv_quant_rows_mx_launches(void) { return quant_rows_mx_launches.load(std::memory_order_relaxed); }
extern "C" long long sv_quant_cols_mx_launches(void) { return quant_cols_mx_launches.load(std::memory_order_relaxed); }
extern "C" long long sv_mx_rows_to_cols_launches(void) { return mx_rows_to_cols_launches.load(std::memory_order_relaxed); }
extern "C" long long sv_quant_rows_cols_mx_launches(void) { return quant_rows_cols_mx_launches.load(std::memory_order_relaxed); }
extern "C" long long sv_linear_fp8_bwd_launches(int which) {
  return (which == 0 || which == 1) ? linear_fp8_bwd_launches[which].load(std::memory_order_relaxed) : -1;
}
extern "C" long long sv_linear_mxfp8_bwd_launches(int which) {
  return (which == 0 || which == 1) ? linear_mxfp8_bwd_launches[which].load(std::memory_order_relaxed) : -1;
}

extern "C" int sv_linear_fp8_supported(int K, int N, const sv_epilogue* e, int math, int act_dtype) {
  const char* why;
  return (K > 0 && N > 0 && math == SV_MATH_BF16 && (act_dtype == SV_F32 || act_dtype == SV_BF16) && linear_fp8_epilogue_ok(e, N, &why)) ? 1 : 0;
}
extern "C" int sv_linear_fp8_dgrad_supported(int N, int K, const sv_epilogue* e, int math, int act_dtype) {
  const char* why;
  return (N > 0 && K > 0 && math == SV_MATH_BF16 && (act_dtype == SV_F32 || act_dtype == SV_BF16) && linear_fp8_dgrad_epilogue_ok(e, K, &why)) ? 1 : 0;
}
extern "C" size_t sv_linear_mxfp8_wgrad_workspace_floats(int M, int N, int K, int splits) {
  if (M <= 0 || N <= 0 || K <= 0 || splits < 0) return 0;
  const int sp = linear_wgrad_splits(M, N, K, splits);
  return sp > 1 ? (size_t)sp * (size_t)N * (size_t)K : 0;
}

// ---- quantisers ------------------------------------------------------------------------------------------------------------------------------------
extern "C" int sv_quant_rows_e4m3(const void* src, int src_dtype, int rows, int K, int ld, void* dst_q, int Kp, float* scales, void* stream) {
  const char* fn = "sv_quant_rows_e4m3";
  SV_REQUIRE(src && dst_q && scales, "%s: null argument", fn);
  if (const int rc = require_quant_source({fn, src, src_dtype, "rows", rows, "K", K, ld})) return rc;
  SV_REQUIRE(Kp >= K && Kp % 128 == 0, "%s: Kp (%d) must be a multiple of 128 and >= K (%d)", fn, Kp, K);
  SV_REQUIRE(((uintptr_t)dst_q & 15) == 0, "%s: dst_q must be 16-byte aligned", fn);
  SV_REQUIRE(quant_src_aligned(src, src_dtype), "%s: src is not aligned to its element", fn);
  SV_DISPATCH_ACT(src_dtype, hipLaunchKernelGGL(quant_rows_kernel<AT>, dim3(cdiv(rows, 4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                                                static_cast<const AT*>(src), rows, K, (long long)ld, static_cast<uint8_t*>(dst_q), Kp, scales););
  return finish_launch(fn, nullptr);
}

extern "C" int sv_quant_rows_mx_e4m3(const void* src, int src_dtype, int rows, int K, int ld, void* dst_q, int Kp, void* scales_u8, void* stream) {
  const char* fn = "sv_quant_rows_mx_e4m3";
  SV_REQUIRE(src && dst_q && scales_u8, "%s: null argument", fn);
  if (const int rc = require_quant_source({fn, src, src_dtype, "rows", rows, "K", K, ld})) return rc;
  if (const int rc = require_padded(fn, "Kp", Kp, "K", K)) return rc;
  SV_REQUIRE(((uintptr_t)dst_q & 15) == 0 && ((uintptr_t)scales_u8 & 3) == 0, "%s: dst_q must be 16-byte aligned, scales_u8 4-byte aligned", fn);
  SV_REQUIRE(quant_src_aligned(src, src_dtype), "%s: src is not aligned to its element", fn);
  SV_DISPATCH_ACT(src_dtype, hipLaunchKernelGGL(quant_rows_mx_kernel<AT>, dim3(cdiv(rows, 4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                                                static_cast<const AT*>(src), rows, K, (long long)ld, static_cast<uint8_t*>(dst_q), Kp,
                                                static_cast<uint8_t*>(scales_u8)););
  return finish_launch(fn, &quant_rows_mx_launches);
}

extern "C" int sv_quant_cols_e4m3(const void* src, int src_dtype, int M, int C, int ld, void* dst_q, int Mp, float* scales, float* colsum, void* stream) {
  const char* fn = "sv_quant_cols_e4m3";
  SV_REQUIRE(src && dst_q && scales, "%s: null argument", fn);
  if (const int rc = require_quant_source({fn, src, src_dtype, "M", M, "C", C, ld})) return rc;
  if (const int rc = require_padded(fn, "Mp", Mp, "M", M)) return rc;
  SV_REQUIRE(((uintptr_t)dst_q & 15) == 0, "%s: dst_q must be 16-byte aligned", fn);
  SV_REQUIRE(quant_src_aligned(src, src_dtype), "%s: src is not aligned to its element", fn);
  SV_REQUIRE(cdiv(M, QC_ROWS2) <= 65535, "%s: M (%d) is too large", fn, M);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(scales, 0, sizeof(float) * (size_t)C, s) != hipSuccess) return check_launch("sv_quant_cols_e4m3 (clear)");
  const dim3 g1(cdiv(C, QC_COLS), cdiv(M, QC_ROWS1)), g2(cdiv(C, QC_COLS), Mp / QC_ROWS2);
  SV_DISPATCH_ACT(src_dtype, hipLaunchKernelGGL(quant_cols_amax_kernel<AT>, g1, dim3(256), 0, s, static_cast<const AT*>(src), M, C, (long long)ld,
                                                reinterpret_cast<int*>(scales), colsum););
  hipLaunchKernelGGL(quant_cols_scale_kernel, dim3(cdiv(C, 256)), dim3(256), 0, s, scales, C);
  SV_DISPATCH_ACT(src_dtype, hipLaunchKernelGGL(quant_cols_write_kernel<AT>, g2, dim3(256), 0, s, static_cast<const AT*>(src), M, C, (long long)ld, scales,
                                                static_cast<uint8_t*>(dst_q), Mp););
  return finish_launch(fn, nullptr);
}

extern "C" int sv_quant_cols_mx_e4m3(const void* src, int src_dtype, int M, int C, int ld, void* dst_q, int Mp, void* scales_u8, float* colsum, void* stream) {
  const char* fn = "sv_quant_cols_mx_e4m3";
  SV_REQUIRE(src && dst_q && scales_u8, "%s: null argument", fn);
  if (const int rc = require_quant_source({fn, src, src_dtype, "M", M, "C", C, ld})) return rc;
  if (const int rc = require_padded(fn, "Mp", Mp, "M", M)) return rc;
  SV_REQUIRE(((uintptr_t)dst_q & 15) == 0 && ((uintptr_t)scales_u8 & 3) == 0, "%s: dst_q must be 16-byte aligned, scales_u8 4-byte aligned", fn);
  SV_REQUIRE(quant_src_aligned(src, src_dtype) && ((uintptr_t)colsum & 3) == 0, "%s: src / colsum are not aligned to their element", fn);
  SV_REQUIRE(cdiv(M, QC_ROWS2) <= 65535, "%s: M (%d) is too large", fn, M);
  SV_DISPATCH_ACT(src_dtype, hipLaunchKernelGGL(quant_cols_mx_kernel<AT>, dim3(cdiv(C, QC_COLS), Mp / QC_ROWS2), dim3(256), 0, static_cast<hipStream_t>(stream),
                                                static_cast<const AT*>(src), M, C, (long long)ld, static_cast<uint8_t*>(dst_q), Mp,
                                                static_cast<uint8_t*>(scales_u8), colsum););
  return finish_launch(fn, &quant_cols_mx_launches);
}

extern "C" int sv_mx_rows_to_cols(const void* xq, int Kp, const void* xs, int M, int K, void* dst_q, int Mp, void* scales_u8, void* stream) {
  SV_REQUIRE(xq && xs && dst_q && scales_u8, "sv_mx_rows_to_cols: null argument");
  SV_REQUIRE(M > 0 && K > 0, "sv_mx_rows_to_cols: M (%d) and K (%d) must be positive", M, K);
  SV_REQUIRE(Kp == cdiv(K, 128) * 128, "sv_mx_rows_to_cols: Kp (%d) must be K (%d) rounded up to a multiple of 128", Kp, K);
  SV_REQUIRE(Mp == cdiv(M, 128) * 128, "sv_mx_rows_to_cols: Mp (%d) must be M (%d) rounded up to a multiple of 128", Mp, M);
  SV_REQUIRE((((uintptr_t)xq | (uintptr_t)dst_q) & 15) == 0, "sv_mx_rows_to_cols: xq and dst_q must be 16-byte aligned");
  SV_REQUIRE((((uintptr_t)xs | (uintptr_t)scales_u8) & 3) == 0, "sv_mx_rows_to_cols: xs and scales_u8 must be 4-byte aligned");
  SV_REQUIRE(Mp / RB_ROWS <= 65535, "sv_mx_rows_to_cols: M (%d) is too large", M);
  hipLaunchKernelGGL(mx_rows_to_cols_kernel, dim3(Kp / RB_COLS, Mp / RB_ROWS), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const uint8_t*>(xq), Kp,
                     static_cast<const uint8_t*>(xs), M, K, static_cast<uint8_t*>(dst_q), Mp, static_cast<uint8_t*>(scales_u8));
  return finish_launch("sv_mx_rows_to_cols", &mx_rows_to_cols_launches);
}

extern "C" int sv_quant_rows_cols_mx_e4m3(const void* src, int src_dtype, int M, int N, int ld, void* row_q, int Np, void* row_s, void* col_q, int Mp,
                                          void* col_s, float* colsum, void* stream) {
  const char* fn = "sv_quant_rows_cols_mx_e4m3";
  SV_REQUIRE(src && col_q && col_s, "%s: null argument (src, col_q and col_s are required)", fn);
  SV_REQUIRE((row_q != nullptr) == (row_s != nullptr), "%s: row_q and row_s go together", fn);
  if (const int rc = require_quant_source({fn, src, src_dtype, "M", M, "N", N, ld})) return rc;
  if (const int rc = require_padded(fn, "Np", Np, "N", N)) return rc;
  if (const int rc = require_padded(fn, "Mp", Mp, "M", M)) return rc;
  SV_REQUIRE((((uintptr_t)row_q | (uintptr_t)col_q) & 15) == 0, "%s: row_q and col_q must be 16-byte aligned", fn);
  SV_REQUIRE((((uintptr_t)row_s | (uintptr_t)col_s) & 3) == 0, "%s: row_s and col_s must be 4-byte aligned", fn);
  SV_REQUIRE(quant_src_aligned(src, src_dtype) && ((uintptr_t)colsum & 3) == 0, "%s: src / colsum are not aligned to their element", fn);
  SV_REQUIRE(Mp / RB_ROWS <= 65535, "%s: M (%d) is too large", fn, M);
  SV_DISPATCH_ACT(src_dtype, {
    const auto kernel = row_q ? quant_rows_cols_mx_kernel<AT, true> : quant_rows_cols_mx_kernel<AT, false>;   // no rows asked for: the row work is compiled out
    hipLaunchKernelGGL(kernel, dim3(Np / RB_COLS, Mp / RB_ROWS), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const AT*>(src), M, N, (long long)ld,
                       static_cast<uint8_t*>(row_q), Np, static_cast<uint8_t*>(row_s), static_cast<uint8_t*>(col_q), Mp, static_cast<uint8_t*>(col_s), colsum);
  });
  return finish_launch(fn, &quant_rows_cols_mx_launches);
}

// ---- GEMMs -----------------------------------------------------------------------------------------------------------------------------------------
extern "C" int sv_linear_fp8(const void* xq, const float* sx, const void* wq, const float* sw, void* out, int M, int K, int N, const sv_epilogue* e,
                             int act_dtype, void* stream) {
  return launch_linear<false>("sv_linear_fp8", linear_fp8_launches, xq, sx, wq, sw, out, M, K, N, e, nullptr, nullptr, act_dtype, stream);
}
extern "C" int sv_linear_mxfp8(const void* xq, const void* xs, const void* wq, const void* ws, void* out, int M, int K, int N, const sv_epilogue* e,
                               void* q_out, void* qs_out, int act_dtype, void* stream) {
  return launch_linear<true>("sv_linear_mxfp8", linear_mxfp8_launches, xq, xs, wq, ws, out, M, K, N, e, q_out, qs_out, act_dtype, stream);
}
extern "C" int sv_linear_fp8_dgrad(const void* dq, const float* sd, const void* wtq, const float* swt, void* dx, int M, int N, int K, const sv_epilogue* e,
                                   int act_dtype, void* stream) {
  return launch_dgrad<false>("sv_linear_fp8_dgrad", linear_fp8_bwd_launches[0], dq, sd, wtq, swt, dx, M, N, K, e, act_dtype, stream);
}
extern "C" int sv_linear_mxfp8_dgrad(const void* dq, const void* ds, const void* wtq, const void* wts, void* dx, int M, int N, int K, const sv_epilogue* e,
                                     int act_dtype, void* stream) {
  return launch_dgrad<true>("sv_linear_mxfp8_dgrad", linear_mxfp8_bwd_launches[0], dq, ds, wtq, wts, dx, M, N, K, e, act_dtype, stream);
}
extern "C" int sv_linear_fp8_wgrad(const void* dyt, const float* sdc, const void* xt, const float* sxc, float* dw, int M, int N, int K, int ldw, int splits,
                                   void* stream) {
  return launch_wgrad<false>("sv_linear_fp8_wgrad", linear_fp8_bwd_launches[1], dyt, sdc, xt, sxc, dw, M, N, K, ldw, splits, nullptr, stream);
}
extern "C" int sv_linear_mxfp8_wgrad(const void* dyt, const void* dys, const void* xt, const void* xs, float* dw, int M, int N, int K, int ldw, int splits,
                                     float* workspace, void* stream) {
  return launch_wgrad<true>("sv_linear_mxfp8_wgrad", linear_mxfp8_bwd_launches[1], dyt, dys, xt, xs, dw, M, N, K, ldw, splits, workspace, stream);
}
