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
//   linear_fp8_dgrad_kernel   lf_contract over the full contraction + the epilogue above.
//   linear_fp8_wgrad_kernel   grid tiles(N) x tiles(K) x splits, split z contracts the k-steps [z nk / splits, (z + 1) nk / splits); dy^T is the
//                    row operand, so a lane's 16 consecutive outputs run along k, the contiguous dimension of dw; fp32 atomicAdd into dw
//                    (a plain read-add-write when splits == 1).  splits = 0 picks enough workgroups for 2 per CU of 256 CUs.
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
//                    of column tx = exactly one MX block, so the block maximum stays in its registers (32 values held, no exchange).  8 packed dwords
//                    go through the same LDS transpose (pitch 33 dwords) into 16-byte stores along M; the four scale bytes of a column and tile are
//                    gathered in LDS into one dword store.  Column sums: fp64 partial per workgroup, one fp32 atomic per workgroup and column.
//   linear_fp8_dgrad_kernel<.., MX = true>   lf_contract<true> + the epilogue above without its 16 divisions per lane and row; LDS 67 584 bytes.
//   linear_mxfp8_wgrad_kernel   lf_contract<true> over split z's k-steps; NO atomics into dw.  One split: the only writer of an element does a
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
//                  K (8 lanes = the 128 contiguous bytes of a row), a byte transpose through LDS (described at the kernel), 16-byte stores along M,
//                  the four scale bytes of a column and tile as one aligned dword.
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
struct LinFp8Args {
  const uint8_t* xq; const float* sx; const uint8_t* wq; const float* sw; void* out;
  int M, N, Kp;
  const float* bias; const void* residual; int ldr; const float* row_scale; int rows_per_scale; void* pre_act; int act; float slope; int ldc;
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

__device__ __forceinline__ void lf_zero(f32x4 (&acc)[4][4]) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

// MX form of the call: E8M0 scale bytes [rows][Kp / 32] in place of the fp32 row scales, and the optional emission of the stored output's own MX rows
struct LinMxArgs {
  const uint8_t* xq; const uint8_t* xs; const uint8_t* wq; const uint8_t* ws; void* out;
  int M, N, Kp;
  const float* bias; const void* residual; int ldr; const float* row_scale; int rows_per_scale; void* pre_act; int act; float slope; int ldc;
  uint8_t* q_out; uint8_t* qs_out;   // [M][N] e4m3 bytes and [M][N / 32] scale bytes of the stored output (N % 128 == 0, no residual), or both null
};
template <bool MX> struct LinArgsOf { typedef LinFp8Args type; };
template <> struct LinArgsOf<true> { typedef LinMxArgs type; };

// MX = false: the per-row recipe (val = acc / (sx sw)).  MX = true: the MX recipe (block scales applied by the MFMA, val = acc); out may then be
// null when q_out is given.  Emission: the stored row (after the activation, rounded to AT) is quantised as quant_rows_mx_kernel would quantise
// it; a 32-column block is the 16 + 16 columns of lanes lg and lg ^ 1 (lane ^ 16) of the same row, so one exchange gives its maximum.
template <typename AT, bool FAST, bool MX = false>
__global__ __launch_bounds__(256, 2) void linear_fp8_kernel(const typename LinArgsOf<MX>::type p) {
  __shared__ __attribute__((aligned(16))) uint8_t lf_smem[2 * 2 * LF_TILE + (MX ? 2 * LF_SCALES : 0)];   // [2 buffers][x tile, w tile][128 rows][128 bytes, swizzled] (+ [2][scale dwords])
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lr = lane & 15, lg = lane >> 4;
  const int tiles_n = (p.N + LF_BN - 1) / LF_BN;
  const int row0 = (blockIdx.x / tiles_n) * LF_BM, col0 = (blockIdx.x % tiles_n) * LF_BN;   // consecutive workgroups share the x rows

  f32x4 acc[4][4];   // [column block nt][row block mt]
  lf_zero(acc);
  if constexpr (MX) lf_contract<true>(p.xq, p.M, p.wq, p.N, (size_t)p.Kp, row0, col0, 0, p.Kp / LF_BK, lf_smem, acc, p.xs, p.ws);
  else lf_contract(p.xq, p.M, p.wq, p.N, (size_t)p.Kp, row0, col0, 0, p.Kp / LF_BK, lf_smem, acc);

  // ---- epilogue on the registers: with the permuted W rows, lane (lr, lg) holds row 16 mt + lr and, over its four blocks nt, the 16
  // consecutive columns 16 lg + 4 nt + j of the wave's 64: 16-byte stores (8 bf16 / 4 fp32), 32 / 64 contiguous bytes per lane and row
  AT* __restrict__ Y = static_cast<AT*>(p.out);
  AT* __restrict__ PRE = static_cast<AT*>(p.pre_act);
  const AT* __restrict__ RES = static_cast<const AT*>(p.residual);
  constexpr int CV = sizeof(AT) == 2 ? 8 : 4;              // elements of a 16-byte piece
  const bool vec4 = ((p.ldc | p.N) & 3) == 0 && (!RES || (p.ldr & 3) == 0);   // (base pointers: 4 elements, checked on the host)
  const bool vecw = ((p.ldc | p.N) & (CV - 1)) == 0 && (!RES || (p.ldr & (CV - 1)) == 0) &&
                    ((((uintptr_t)Y) | ((uintptr_t)PRE) | ((uintptr_t)RES)) & 15) == 0;
  const int c0 = col0 + wn * 64 + lg * 16;
  if (c0 < p.N) {
    float swn[16], bias[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int n = min(c0 + j, p.N - 1);
      if constexpr (!MX) swn[j] = p.sw[n];
      bias[j] = p.bias ? p.bias[n] : 0.f;
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int m = row0 + wm * 64 + mt * 16 + lr;
      if (m >= p.M) continue;
      float sxm = 1.f;
      if constexpr (!MX) sxm = p.sx[m];
      const float sc = (RES && p.row_scale) ? p.row_scale[m / p.rows_per_scale] : 1.f;
      float v[16];
      if constexpr (MX) {
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = acc[j >> 2][mt][j & 3] + bias[j];
        if (p.q_out) {   // N % 128 == 0 and no residual (host): all 16 columns are in range and the stored value is act(v)
          float t[16], am = 0.f;
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            t[j] = (float)(AT)apply_act_t<FAST>(v[j], p.act, p.slope);
            am = fmaxf(am, fabsf(t[j]));
          }
          am = fmaxf(am, __shfl_xor(am, 16));              // the partner holds the same row: it is here whenever this lane is
          const int E = mx_block_exp(am);
          *reinterpret_cast<uint4*>(p.q_out + (size_t)m * p.N + c0) =
              make_uint4(pack4_e4m3_mx(t[0], t[1], t[2], t[3], E), pack4_e4m3_mx(t[4], t[5], t[6], t[7], E),
                         pack4_e4m3_mx(t[8], t[9], t[10], t[11], E), pack4_e4m3_mx(t[12], t[13], t[14], t[15], E));
          if ((lg & 1) == 0) p.qs_out[(size_t)m * (p.N >> 5) + (c0 >> 5)] = (uint8_t)(E + 127);
          if (!Y && !PRE) continue;                        // no backward follows: neither out nor pre_act is stored
        }
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = acc[j >> 2][mt][j & 3] / (sxm * swn[j]) + bias[j];
      }
      const size_t o = (size_t)m * p.ldc + c0;
      const size_t orow = (size_t)m * p.ldr + c0;
      if (vecw) {   // N % CV == 0: a piece is in range as a whole
#pragma unroll
        for (int q = 0; q < 16 / CV; ++q) {
          if (c0 + q * CV >= p.N) break;
          float t[CV];
#pragma unroll
          for (int j = 0; j < CV; ++j) t[j] = v[q * CV + j];
          if (PRE) stnf<CV>(PRE + o + q * CV, t);
          if constexpr (MX) { if (!Y) continue; }          // MX store: pre_act and the emitted rows are all the backward reads
#pragma unroll
          for (int j = 0; j < CV; ++j) t[j] = apply_act_t<FAST>(t[j], p.act, p.slope);
          if (RES) {
            float r[CV];
            ldnf<CV>(RES + orow + q * CV, r);
#pragma unroll
            for (int j = 0; j < CV; ++j) t[j] = r[j] + sc * t[j];
          }
          stnf<CV>(Y + o + q * CV, t);
        }
      } else if (vec4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (c0 + q * 4 >= p.N) break;
          float t[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) t[j] = v[q * 4 + j];
          if (PRE) stnf<4>(PRE + o + q * 4, t);
          if constexpr (MX) { if (!Y) continue; }
#pragma unroll
          for (int j = 0; j < 4; ++j) t[j] = apply_act_t<FAST>(t[j], p.act, p.slope);
          if (RES) {
            float r[4];
            ldnf<4>(RES + orow + q * 4, r);
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = r[j] + sc * t[j];
          }
          stnf<4>(Y + o + q * 4, t);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          if (c0 + j < p.N) {
            float t = v[j];
            if (PRE) stf(PRE + o + j, t);
            if constexpr (MX) { if (!Y) continue; }
            t = apply_act_t<FAST>(t, p.act, p.slope);
            if (RES) t = ldf(RES + orow + j) + sc * t;
            stf(Y + o + j, t);
          }
        }
      }
    }
  }
}

// ---- data gradient: dx[M, K] = dy[M, N] W[N, K], the contraction runs over N -----------------------------------------------------------------
struct LinFp8DgradArgs {
  const uint8_t* dq; const float* sd; const uint8_t* wtq; const float* swt; void* out;
  int M, K, Np;
  const void* act_grad_src; int act_grad_kind; float slope; int ldc;
};

// MX form of the call: E8M0 scale bytes [M][Np / 32] of dy and [K][Np / 32] of W^T in place of the fp32 scales
struct LinMxDgradArgs {
  const uint8_t* dq; const uint8_t* ds; const uint8_t* wtq; const uint8_t* wts; void* out;
  int M, K, Np;
  const void* act_grad_src; int act_grad_kind; float slope; int ldc;
};
template <bool MX> struct DgradArgsOf { typedef LinFp8DgradArgs type; };
template <> struct DgradArgsOf<true> { typedef LinMxDgradArgs type; };

template <typename AT, bool FAST, bool MX = false>
__global__ __launch_bounds__(256, 2) void linear_fp8_dgrad_kernel(const typename DgradArgsOf<MX>::type p) {
  __shared__ __attribute__((aligned(16))) uint8_t lf_smem[2 * 2 * LF_TILE + (MX ? 2 * LF_SCALES : 0)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lr = lane & 15, lg = lane >> 4;
  const int tiles_k = (p.K + LF_BN - 1) / LF_BN;
  const int row0 = (blockIdx.x / tiles_k) * LF_BM, col0 = (blockIdx.x % tiles_k) * LF_BN;   // consecutive workgroups share the dy rows

  f32x4 acc[4][4];
  lf_zero(acc);
  if constexpr (MX) lf_contract<true>(p.dq, p.M, p.wtq, p.K, (size_t)p.Np, row0, col0, 0, p.Np / LF_BK, lf_smem, acc, p.ds, p.wts);
  else lf_contract(p.dq, p.M, p.wtq, p.K, (size_t)p.Np, row0, col0, 0, p.Np / LF_BK, lf_smem, acc);

  AT* __restrict__ Y = static_cast<AT*>(p.out);
  const AT* __restrict__ G = static_cast<const AT*>(p.act_grad_src);   // layout of the output
  constexpr int CV = sizeof(AT) == 2 ? 8 : 4;
  const bool vecw = ((p.ldc | p.K) & (CV - 1)) == 0 && ((((uintptr_t)Y) | ((uintptr_t)G)) & 15) == 0;
  const int c0 = col0 + wn * 64 + lg * 16;
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
struct LinFp8WgradArgs {
  const uint8_t* dyt; const float* sdc; const uint8_t* xt; const float* sxc; float* dw;
  int N, K, Mp, ldw, splits;
};

__global__ __launch_bounds__(256, 2) void linear_fp8_wgrad_kernel(const LinFp8WgradArgs p) {
  __shared__ __attribute__((aligned(16))) uint8_t lf_smem[2 * 2 * LF_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lr = lane & 15, lg = lane >> 4;
  const int tiles_k = (p.K + LF_BN - 1) / LF_BN;
  const int row0 = (blockIdx.x / tiles_k) * LF_BM, col0 = (blockIdx.x % tiles_k) * LF_BN;   // rows of dw = n, columns = k
  const int nk = p.Mp / LF_BK, z = blockIdx.y;
  const int ks0 = (int)((long long)z * nk / p.splits), ks1 = (int)((long long)(z + 1) * nk / p.splits);   // splits <= nk: no share is empty

  f32x4 acc[4][4];
  lf_zero(acc);
  // dy^T is the row operand and x^T the permuted one: a lane's 16 consecutive outputs run along k, the contiguous dimension of dw
  lf_contract(p.dyt, p.N, p.xt, p.K, (size_t)p.Mp, row0, col0, ks0, ks1, lf_smem, acc);

  const int c0 = col0 + wn * 64 + lg * 16;
  if (c0 >= p.K) return;
  float sxk[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) sxk[j] = p.sxc[min(c0 + j, p.K - 1)];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int n = row0 + wm * 64 + mt * 16 + lr;
    if (n >= p.N) continue;
    const float sdn = p.sdc[n];
    float* __restrict__ d = p.dw + (size_t)n * p.ldw + c0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (c0 + j < p.K) {
        const float val = acc[j >> 2][mt][j & 3] / (sdn * sxk[j]);
        if (p.splits == 1) d[j] += val;                    // the only writer of this element
        else atomicAdd(d + j, val);
      }
    }
  }
}

// ---- MX weight gradient: the same contraction on MX operands, no atomics into dw ----------------------------------------------------------------
struct LinMxWgradArgs {
  const uint8_t* dyt; const uint8_t* dys; const uint8_t* xt; const uint8_t* xs; float* dw; float* ws;   // ws [splits][N][K] fp32, used when splits > 1
  int N, K, Mp, ldw, splits;
};

__global__ __launch_bounds__(256, 2) void linear_mxfp8_wgrad_kernel(const LinMxWgradArgs p) {
  __shared__ __attribute__((aligned(16))) uint8_t lf_smem[2 * 2 * LF_TILE + 2 * LF_SCALES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lr = lane & 15, lg = lane >> 4;
  const int tiles_k = (p.K + LF_BN - 1) / LF_BN;
  const int row0 = (blockIdx.x / tiles_k) * LF_BM, col0 = (blockIdx.x % tiles_k) * LF_BN;   // rows of dw = n, columns = k
  const int nk = p.Mp / LF_BK, z = blockIdx.y;
  const int ks0 = (int)((long long)z * nk / p.splits), ks1 = (int)((long long)(z + 1) * nk / p.splits);   // splits <= nk: no share is empty

  f32x4 acc[4][4];
  lf_zero(acc);
  // dy^T is the row operand and x^T the permuted one: a lane's 16 consecutive outputs run along k, the contiguous dimension of dw
  lf_contract<true>(p.dyt, p.N, p.xt, p.K, (size_t)p.Mp, row0, col0, ks0, ks1, lf_smem, acc, p.dys, p.xs);

  const int c0 = col0 + wn * 64 + lg * 16;
  if (c0 >= p.K) return;
  // one split: read-add-write into dw (row stride ldw), this lane is the only writer of its elements; more: a plain store of the partial
  // into slice z of the workspace (row stride K), which the reduce kernel folds into dw
  const bool one = p.splits == 1;
  float* __restrict__ base = one ? p.dw : p.ws + (size_t)z * p.N * p.K;
  const int ldo = one ? p.ldw : p.K;
  const bool vec = ((ldo | p.K) & 3) == 0 && (((uintptr_t)base) & 15) == 0;   // K % 4 == 0: a 16-byte piece is in range as a whole
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int n = row0 + wm * 64 + mt * 16 + lr;
    if (n >= p.N) continue;
    float* __restrict__ d = base + (size_t)n * ldo + c0;
    if (vec) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (c0 + q * 4 >= p.K) break;
        float4 t = make_float4(acc[q][mt][0], acc[q][mt][1], acc[q][mt][2], acc[q][mt][3]);
        if (one) {
          const float4 o = *reinterpret_cast<const float4*>(d + q * 4);
          t = make_float4(o.x + t.x, o.y + t.y, o.z + t.z, o.w + t.w);
        }
        *reinterpret_cast<float4*>(d + q * 4) = t;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (c0 + j < p.K) {
          const float val = acc[j >> 2][mt][j & 3];
          d[j] = one ? d[j] + val : val;
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

// ---- column quantiser: src [M, C] (row stride ld) -> dst [C][Mp] e4m3 bytes, one scale per column ---------------------------------------------------
constexpr int QC_COLS = 64, QC_ROWS1 = 256, QC_ROWS2 = 128, QC_PITCH = 33;   // pass-2 LDS rows: 32 dwords + 1, conflict-free on both sides

// pass 1: amax[c] = max over the rows of |src[m, c]| as the bit pattern of the non-negative float (integer max = float max there), into a zeroed
// buffer; optionally colsum[c] += sum over the rows (fp64 partial per workgroup, one fp32 atomic per workgroup and column)
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

// pass 2: a tile of 128 rows x 64 columns is scaled, rounded to e4m3 and transposed through LDS; 16-byte stores along M.  Rows past M are zero bytes.
template <typename T>
__global__ __launch_bounds__(256) void quant_cols_write_kernel(const T* __restrict__ src, int M, int C, long long ld, const float* __restrict__ scales,
                                                               uint8_t* __restrict__ dst, int Mp) {
  __shared__ uint32_t tile[QC_COLS * QC_PITCH];            // [column][32 dwords = 128 rows]
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
    tile[tx * QC_PITCH + ty * 8 + i] = pack4_e4m3(v[0] * s, v[1] * s, v[2] * s, v[3] * s);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i) {                            // 64 columns x 8 pieces of 16 bytes
    const int pc = threadIdx.x + 256 * i, col = pc >> 3, piece = pc & 7;
    if (c0 + col < C) {
      const uint32_t* t = tile + col * QC_PITCH + piece * 4;
      *reinterpret_cast<uint4*>(dst + (size_t)(c0 + col) * Mp + m0 + piece * 16) = make_uint4(t[0], t[1], t[2], t[3]);
    }
  }
}

// MX column quantiser: src [M, C] -> dst [C][Mp] e4m3 bytes + scales [C][Mp / 32] E8M0 bytes, equal to quant_rows_mx_kernel on the transposed tensor.
// The tile of quant_cols_write_kernel; thread (tx, ty) owns rows 32 ty .. + 31 of column tx, which is exactly one MX block: its 32 values stay in
// registers between the maximum and the packing, and src is read once.  Rows past M are zeros: a partly filled block takes the maximum of its valid
// rows, a block wholly past M is an all-zero block (byte 127).  colsum as in quant_cols_amax_kernel.
template <typename T>
__global__ __launch_bounds__(256) void quant_cols_mx_kernel(const T* __restrict__ src, int M, int C, long long ld, uint8_t* __restrict__ dst, int Mp,
                                                            uint8_t* __restrict__ scales, float* __restrict__ colsum) {
  __shared__ uint32_t tile[QC_COLS * QC_PITCH];            // [column][32 dwords = 128 rows]
  __shared__ uint32_t sbytes[QC_COLS];                     // [column][4 blocks of the tile]: one dword per column
  __shared__ double ssum[4][QC_COLS];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c0 = blockIdx.x * QC_COLS, m0 = blockIdx.y * QC_ROWS2;
  const int c = c0 + tx, mb = m0 + ty * 32;
  float v[32];
  float am = 0.f;
  double sum = 0.0;
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    v[j] = (c < C && mb + j < M) ? ldf(src + (size_t)(mb + j) * ld + c) : 0.f;
    am = fmaxf(am, fabsf(v[j]));
  }
  if (colsum) {
#pragma unroll
    for (int j = 0; j < 32; ++j) sum += (double)v[j];
    ssum[ty][tx] = sum;
  }
  const int E = mx_block_exp(am);
#pragma unroll
  for (int i = 0; i < 8; ++i) tile[tx * QC_PITCH + ty * 8 + i] = pack4_e4m3_mx(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3], E);
  reinterpret_cast<uint8_t*>(sbytes)[tx * 4 + ty] = (uint8_t)(E + 127);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i) {                            // 64 columns x 8 pieces of 16 bytes
    const int pc = threadIdx.x + 256 * i, col = pc >> 3, piece = pc & 7;
    if (c0 + col < C) {
      const uint32_t* t = tile + col * QC_PITCH + piece * 4;
      *reinterpret_cast<uint4*>(dst + (size_t)(c0 + col) * Mp + m0 + piece * 16) = make_uint4(t[0], t[1], t[2], t[3]);
    }
  }
  if (ty == 0 && c < C) {
    reinterpret_cast<uint32_t*>(scales + (size_t)c * (Mp >> 5))[m0 >> 7] = sbytes[tx];   // the tile's four blocks of column c: one aligned dword
    if (colsum) atomicAdd(colsum + c, (float)(ssum[0][tx] + ssum[1][tx] + ssum[2][tx] + ssum[3][tx]));
  }
}

// MX re-blocker: the MX ROWS of a stored tensor (xq [M][Kp] bytes + xs [M][Kp / 32] scale bytes, a block = 32 columns of a row) become the MX COLUMN
// operand of the weight gradient (dst [K][Mp] bytes + scales [K][Mp / 32], a block = 32 tokens of a column) - see "MX store" in the header.
// One workgroup = 128 tokens x 128 columns, 16 KB in and 16 KB out.
//   load     thread t moves the 16-byte pieces t, t + 256, t + 512, t + 768 of the tile (8 lanes = the 128 contiguous bytes of one row) into a plain
//            [128][128]-byte LDS image (eight lanes of a ds_write_b128 cover the 32 banks once); t < 128 also stages the scale dword of row t (the
//            four k-blocks of the tile).  Rows past M are zero bytes.
//   compute  wave b owns tokens 32 b .. + 31; lane l owns column 64 u + l, u = 0, 1: one MX block per (lane, u).  It reads its 32 bytes down the
//            column (the 32 lanes of a group read 8 consecutive dwords of one row: no conflict), decodes byte 2^(s - 127) in fp32 (exact; the row's
//            scale dword comes from lane j of the wave by v_readlane), takes the maximum and packs 8 dwords under the column block's exponent.
//   store    the 8 dwords go into the [128][33]-dword image of quant_cols_mx_kernel (conflict-free on both sides: 32 consecutive columns x pitch 33
//            on the way in, 4 columns x 8 pieces on the way out) and leave as 16-byte stores along M; the four scale bytes of a column are one dword.
constexpr int RB_ROWS = 128, RB_COLS = 128, RB_PITCH = 33;
__global__ __launch_bounds__(256) void mx_rows_to_cols_kernel(const uint8_t* __restrict__ xq, int Kp, const uint8_t* __restrict__ xs, int M, int K,
                                                              uint8_t* __restrict__ dst, int Mp, uint8_t* __restrict__ scales) {
  __shared__ __attribute__((aligned(16))) uint8_t in[RB_ROWS * RB_COLS];   // [token][column] bytes
  __shared__ uint32_t srows[RB_ROWS];                        // [token]: the scale bytes of the tile's four k-blocks
  __shared__ uint32_t tile[RB_COLS * RB_PITCH];            // [column][32 dwords = 128 tokens]
  __shared__ uint32_t sbytes[RB_COLS];                     // [column][4 token blocks]: one dword per column
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
    float am = 0.f;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const int s = (__builtin_amdgcn_readlane(srow, j) >> sh) & 0xff;
      v[j] = ldexpf(__builtin_amdgcn_cvt_f32_fp8((int)in[(b * 32 + j) * RB_COLS + col], 0), s - 127);
      am = fmaxf(am, fabsf(v[j]));
    }
    const int E = mx_block_exp(am);
#pragma unroll
    for (int i = 0; i < 8; ++i) tile[col * RB_PITCH + b * 8 + i] = pack4_e4m3_mx(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3], E);
    reinterpret_cast<uint8_t*>(sbytes)[col * 4 + b] = (uint8_t)(E + 127);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {                            // 128 columns x 8 pieces of 16 bytes
    const int pc = tid + 256 * i, col = pc >> 3, piece = pc & 7;
    if (k0 + col < K) {
      const uint32_t* t = tile + col * RB_PITCH + piece * 4;
      *reinterpret_cast<uint4*>(dst + (size_t)(k0 + col) * Mp + m0 + piece * 16) = make_uint4(t[0], t[1], t[2], t[3]);
    }
  }
  if (tid < RB_COLS && k0 + tid < K) reinterpret_cast<uint32_t*>(scales + (size_t)(k0 + tid) * (Mp >> 5))[m0 >> 7] = sbytes[tid];   // one aligned dword
}

// MX dual quantiser: ONE read of src [M, N] gives the MX ROW operand (row_q [M][Np] + row_s [M][Np / 32], equal to quant_rows_mx_kernel) and the MX
// COLUMN operand (col_q [N][Mp] + col_s [N][Mp / 32] + colsum, equal to quant_cols_mx_kernel) - see "MX dual quantiser" in the header.  One workgroup =
// 128 tokens x 128 columns; ROWS_OUT = false compiles the row work out (the column form alone, with this kernel's loader).
//   load     a chunk = 16 consecutive elements of one tile row (sizeof(T) 16-byte pieces: two for bf16, four for fp32); thread t moves the chunks t,
//            t + 256, t + 512, t + 768 (8 lanes = the 128 columns of one row).  A row that is not 16-byte aligned, and the chunk that crosses N, take
//            load4_guarded's per-element path.  Rows past M and columns >= N are zeros.  The chunk goes into a plain [128][128] LDS image of T
//            as it was loaded (the stored values, no conversion).
//   rows     from the registers of the load: a 32-element block is the chunks of lanes c and c ^ 1, so its maximum is one lane exchange; a lane packs
//            its 16 bytes (one 16-byte store) and the even lane writes the E8M0 byte.  Rows past M write nothing; columns N .. Np - 1 are the padding
//            (zero bytes, byte 127), written like any other chunk.
//   columns  mx_rows_to_cols_kernel's compute and store on the staged values: wave b owns tokens 32 b .. + 31, lane l columns l and 64 + l, one MX
//            block per (lane, column) read down the tile (a wave reads 64 consecutive elements of one row: no conflict); fp64 column sums as in
//            quant_cols_mx_kernel.  The 8 packed dwords, the scale byte and the sum wait in registers for a barrier, after which the [column][33
//            dwords] image, the scale dwords and the partial sums take the place of the input image: LDS is 32 KB (bf16) / 64 KB (fp32).
//            Columns >= N write nothing; rows past M were loaded as zeros and leave as the zero bytes of the column rows.
constexpr int DQ_ROWS = 128, DQ_COLS = 128, DQ_PITCH = 33;
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
  constexpr int IN_BYTES = DQ_ROWS * DQ_COLS * (int)sizeof(T);
  constexpr int SUM_BYTES = 4 * DQ_COLS * 8, TILE_BYTES = DQ_COLS * DQ_PITCH * 4, OUT_BYTES = SUM_BYTES + TILE_BYTES + DQ_COLS * 4;
  __shared__ __attribute__((aligned(16))) uint8_t smem[IN_BYTES > OUT_BYTES ? IN_BYTES : OUT_BYTES];
  const T* in = reinterpret_cast<const T*>(smem);          // [token][column], then (after the second barrier):
  double* ssum = reinterpret_cast<double*>(smem);          // [4 token blocks][column]
  uint32_t* tile = reinterpret_cast<uint32_t*>(smem + SUM_BYTES);               // [column][32 dwords = 128 tokens]
  uint32_t* sbytes = reinterpret_cast<uint32_t*>(smem + SUM_BYTES + TILE_BYTES);   // [column][4 token blocks]: one dword per column
  const int tid = threadIdx.x, lane = tid & 63, b = tid >> 6;
  const int k0 = blockIdx.x * DQ_COLS, m0 = blockIdx.y * DQ_ROWS;
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
    for (int p = 0; p < P; ++p) *reinterpret_cast<u32x4*>(smem + ((size_t)r * DQ_COLS + 16 * c) * sizeof(T) + 16 * p) = raw[p];
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
    const int col = u * 64 + lane;
    float v[32];
    float am = 0.f;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      v[j] = ldf(in + (b * 32 + j) * DQ_COLS + col);
      am = fmaxf(am, fabsf(v[j]));
    }
    if (colsum) {
#pragma unroll
      for (int j = 0; j < 32; ++j) sum[u] += (double)v[j];
    }
    Eb[u] = mx_block_exp(am);
#pragma unroll
    for (int i = 0; i < 8; ++i) pk[u][i] = pack4_e4m3_mx(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3], Eb[u]);
  }
  __syncthreads();                                         // every wave has read the input image: the output images take its place
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int col = u * 64 + lane;
#pragma unroll
    for (int i = 0; i < 8; ++i) tile[col * DQ_PITCH + b * 8 + i] = pk[u][i];
    reinterpret_cast<uint8_t*>(sbytes)[col * 4 + b] = (uint8_t)(Eb[u] + 127);
    if (colsum) ssum[b * DQ_COLS + col] = sum[u];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {                            // 128 columns x 8 pieces of 16 bytes
    const int pc = tid + 256 * i, col = pc >> 3, piece = pc & 7;
    if (k0 + col < N) {
      const uint32_t* t = tile + col * DQ_PITCH + piece * 4;
      *reinterpret_cast<uint4*>(col_q + (size_t)(k0 + col) * Mp + m0 + piece * 16) = make_uint4(t[0], t[1], t[2], t[3]);
    }
  }
  if (tid < DQ_COLS && k0 + tid < N) {
    reinterpret_cast<uint32_t*>(col_s + (size_t)(k0 + tid) * (Mp >> 5))[m0 >> 7] = sbytes[tid];   // the tile's four blocks of the column: one aligned dword
    if (colsum) atomicAdd(colsum + k0 + tid, (float)(ssum[tid] + ssum[DQ_COLS + tid] + ssum[2 * DQ_COLS + tid] + ssum[3 * DQ_COLS + tid]));
  }
}

static std::atomic<long long> linear_fp8_launches{0};
static std::atomic<long long> quant_rows_cols_mx_launches{0};
static std::atomic<long long> linear_mxfp8_bwd_launches[2], quant_cols_mx_launches{0};   // MX data gradient, MX weight gradient; the MX column quantiser
static std::atomic<long long> mx_rows_to_cols_launches{0};
static std::atomic<long long> linear_mxfp8_launches{0}, quant_rows_mx_launches{0};
static std::atomic<long long> linear_fp8_bwd_launches[2];   // data gradient, weight gradient

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

// the epilogue forms the kernel serves; `why` receives the reason of a refusal
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

}  // namespace sv

using namespace sv;

extern "C" int sv_quant_rows_e4m3(const void* src, int src_dtype, int rows, int K, int ld, void* dst_q, int Kp, float* scales, void* stream) {
  SV_REQUIRE(src && dst_q && scales, "sv_quant_rows_e4m3: null argument");
  SV_REQUIRE(src_dtype == SV_F32 || src_dtype == SV_BF16, "sv_quant_rows_e4m3: bad source dtype %d", src_dtype);
  SV_REQUIRE(rows > 0 && K > 0 && ld >= K, "sv_quant_rows_e4m3: rows (%d) and K (%d) must be positive, ld (%d) >= K", rows, K, ld);
  SV_REQUIRE(Kp >= K && Kp % 128 == 0, "sv_quant_rows_e4m3: Kp (%d) must be a multiple of 128 and >= K (%d)", Kp, K);
  SV_REQUIRE(((uintptr_t)dst_q & 15) == 0, "sv_quant_rows_e4m3: dst_q must be 16-byte aligned");
  SV_REQUIRE(((uintptr_t)src & (src_dtype == SV_BF16 ? 1 : 3)) == 0, "sv_quant_rows_e4m3: src is not aligned to its element");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(cdiv(rows, 4));
  if (src_dtype == SV_BF16) hipLaunchKernelGGL(quant_rows_kernel<__bf16>, grid, dim3(256), 0, s, static_cast<const __bf16*>(src), rows, K, (long long)ld, static_cast<uint8_t*>(dst_q), Kp, scales);
  else hipLaunchKernelGGL(quant_rows_kernel<float>, grid, dim3(256), 0, s, static_cast<const float*>(src), rows, K, (long long)ld, static_cast<uint8_t*>(dst_q), Kp, scales);
  return check_launch("sv_quant_rows_e4m3");
}

extern "C" int sv_linear_fp8_supported(int K, int N, const sv_epilogue* e, int math, int act_dtype) {
  const char* why;
  return (K > 0 && N > 0 && math == SV_MATH_BF16 && (act_dtype == SV_F32 || act_dtype == SV_BF16) && linear_fp8_epilogue_ok(e, N, &why)) ? 1 : 0;
}

extern "C" long long sv_linear_fp8_launches(void) { return linear_fp8_launches.load(std::memory_order_relaxed); }

extern "C" int sv_linear_fp8(const void* xq, const float* sx, const void* wq, const float* sw, void* out, int M, int K, int N, const sv_epilogue* e,
                             int act_dtype, void* stream) {
  SV_REQUIRE(xq && sx && wq && sw && out && e, "sv_linear_fp8: null argument");
  SV_REQUIRE_ACT(act_dtype);
  SV_REQUIRE(M > 0 && K > 0 && N > 0, "sv_linear_fp8: M (%d), K (%d), N (%d) must be positive", M, K, N);
  const char* why;
  SV_REQUIRE(linear_fp8_epilogue_ok(e, N, &why), "sv_linear_fp8: %s", why);
  SV_REQUIRE((((uintptr_t)xq | (uintptr_t)wq) & 15) == 0, "sv_linear_fp8: quantised operands must be 16-byte aligned");
  const uintptr_t amask = act_dtype == SV_BF16 ? 7 : 15;
  SV_REQUIRE((((uintptr_t)out | (uintptr_t)e->residual | (uintptr_t)e->pre_act) & amask) == 0, "sv_linear_fp8: out / residual / pre_act must be aligned to 4 elements");
  const long long tiles = (long long)cdiv(M, LF_BM) * cdiv(N, LF_BN);
  SV_REQUIRE(tiles < (1ll << 31), "sv_linear_fp8: too many tiles");
  LinFp8Args a{static_cast<const uint8_t*>(xq), sx, static_cast<const uint8_t*>(wq), sw, out, M, N, cdiv(K, LF_BK) * LF_BK,
               e->bias, e->residual, e->ldr, e->row_scale, e->rows_per_scale > 0 ? e->rows_per_scale : 1, e->pre_act, e->act, e->slope, e->ldc};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)tiles), block(256);
  if (act_dtype == SV_BF16) hipLaunchKernelGGL((linear_fp8_kernel<__bf16, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((linear_fp8_kernel<float, false>), grid, block, 0, s, a);
  const int rc = check_launch("sv_linear_fp8");
  if (rc == SV_OK) linear_fp8_launches.fetch_add(1, std::memory_order_relaxed);
  return rc;
}

extern "C" long long sv_linear_mxfp8_launches(void) { return linear_mxfp8_launches.load(std::memory_order_relaxed); }
extern "C" long long sv_quant_rows_mx_launches(void) { return quant_rows_mx_launches.load(std::memory_order_relaxed); }

extern "C" int sv_quant_rows_mx_e4m3(const void* src, int src_dtype, int rows, int K, int ld, void* dst_q, int Kp, void* scales_u8, void* stream) {
  SV_REQUIRE(src && dst_q && scales_u8, "sv_quant_rows_mx_e4m3: null argument");
  SV_REQUIRE(src_dtype == SV_F32 || src_dtype == SV_BF16, "sv_quant_rows_mx_e4m3: bad source dtype %d", src_dtype);
  SV_REQUIRE(rows > 0 && K > 0 && ld >= K, "sv_quant_rows_mx_e4m3: rows (%d) and K (%d) must be positive, ld (%d) >= K", rows, K, ld);
  SV_REQUIRE(Kp == cdiv(K, 128) * 128, "sv_quant_rows_mx_e4m3: Kp (%d) must be K (%d) rounded up to a multiple of 128", Kp, K);
  SV_REQUIRE(((uintptr_t)dst_q & 15) == 0 && ((uintptr_t)scales_u8 & 3) == 0, "sv_quant_rows_mx_e4m3: dst_q must be 16-byte aligned, scales_u8 4-byte aligned");
  SV_REQUIRE(((uintptr_t)src & (src_dtype == SV_BF16 ? 1 : 3)) == 0, "sv_quant_rows_mx_e4m3: src is not aligned to its element");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(cdiv(rows, 4));
  uint8_t* q = static_cast<uint8_t*>(dst_q);
  uint8_t* sc = static_cast<uint8_t*>(scales_u8);
  if (src_dtype == SV_BF16) hipLaunchKernelGGL(quant_rows_mx_kernel<__bf16>, grid, dim3(256), 0, s, static_cast<const __bf16*>(src), rows, K, (long long)ld, q, Kp, sc);
  else hipLaunchKernelGGL(quant_rows_mx_kernel<float>, grid, dim3(256), 0, s, static_cast<const float*>(src), rows, K, (long long)ld, q, Kp, sc);
  const int rc = check_launch("sv_quant_rows_mx_e4m3");
  if (rc == SV_OK) quant_rows_mx_launches.fetch_add(1, std::memory_order_relaxed);
  return rc;
}

extern "C" int sv_linear_mxfp8(const void* xq, const void* xs, const void* wq, const void* ws, void* out, int M, int K, int N, const sv_epilogue* e,
                               void* q_out, void* qs_out, int act_dtype, void* stream) {
  SV_REQUIRE(xq && xs && wq && ws && e, "sv_linear_mxfp8: null argument");
  SV_REQUIRE(out || q_out, "sv_linear_mxfp8: out may be null only when q_out is given");
  SV_REQUIRE((q_out != nullptr) == (qs_out != nullptr), "sv_linear_mxfp8: q_out and qs_out go together");
  SV_REQUIRE_ACT(act_dtype);
  SV_REQUIRE(M > 0 && K > 0 && N > 0, "sv_linear_mxfp8: M (%d), K (%d), N (%d) must be positive", M, K, N);
  const char* why;
  SV_REQUIRE(linear_fp8_epilogue_ok(e, N, &why), "sv_linear_mxfp8: %s", why);
  SV_REQUIRE(!q_out || (!e->residual && !e->row_scale), "sv_linear_mxfp8: the emission of the output's MX rows is not served with a residual");
  SV_REQUIRE(!q_out || N % 128 == 0, "sv_linear_mxfp8: the emission of the output's MX rows needs N (%d) %% 128 == 0", N);
  // pre_act exists for the derivative of the activation: without an activation it would be the unstored out under another name
  SV_REQUIRE(out || !e->pre_act || e->act != SV_ACT_NONE, "sv_linear_mxfp8: pre_act without out is served only in front of an activation");
  SV_REQUIRE((((uintptr_t)xq | (uintptr_t)wq | (uintptr_t)q_out) & 15) == 0, "sv_linear_mxfp8: quantised operands must be 16-byte aligned");
  SV_REQUIRE((((uintptr_t)xs | (uintptr_t)ws | (uintptr_t)qs_out) & 3) == 0, "sv_linear_mxfp8: scale bytes must be 4-byte aligned");
  const uintptr_t amask = act_dtype == SV_BF16 ? 7 : 15;
  SV_REQUIRE((((uintptr_t)out | (uintptr_t)e->residual | (uintptr_t)e->pre_act) & amask) == 0, "sv_linear_mxfp8: out / residual / pre_act must be aligned to 4 elements");
  const long long tiles = (long long)cdiv(M, LF_BM) * cdiv(N, LF_BN);
  SV_REQUIRE(tiles < (1ll << 31), "sv_linear_mxfp8: too many tiles");
  LinMxArgs a{static_cast<const uint8_t*>(xq), static_cast<const uint8_t*>(xs), static_cast<const uint8_t*>(wq), static_cast<const uint8_t*>(ws), out,
              M, N, cdiv(K, LF_BK) * LF_BK, e->bias, e->residual, e->ldr, e->row_scale, e->rows_per_scale > 0 ? e->rows_per_scale : 1, e->pre_act,
              e->act, e->slope, e->ldc, static_cast<uint8_t*>(q_out), static_cast<uint8_t*>(qs_out)};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)tiles), block(256);
  if (act_dtype == SV_BF16) hipLaunchKernelGGL((linear_fp8_kernel<__bf16, true, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((linear_fp8_kernel<float, false, true>), grid, block, 0, s, a);
  const int rc = check_launch("sv_linear_mxfp8");
  if (rc == SV_OK) linear_mxfp8_launches.fetch_add(1, std::memory_order_relaxed);
  return rc;
}

extern "C" int sv_quant_cols_e4m3(const void* src, int src_dtype, int M, int C, int ld, void* dst_q, int Mp, float* scales, float* colsum, void* stream) {
  SV_REQUIRE(src && dst_q && scales, "sv_quant_cols_e4m3: null argument");
  SV_REQUIRE(src_dtype == SV_F32 || src_dtype == SV_BF16, "sv_quant_cols_e4m3: bad source dtype %d", src_dtype);
  SV_REQUIRE(M > 0 && C > 0 && ld >= C, "sv_quant_cols_e4m3: M (%d) and C (%d) must be positive, ld (%d) >= C", M, C, ld);
  SV_REQUIRE(Mp >= M && Mp % 128 == 0 && Mp - M < 128, "sv_quant_cols_e4m3: Mp (%d) must be M (%d) rounded up to a multiple of 128", Mp, M);
  SV_REQUIRE(((uintptr_t)dst_q & 15) == 0, "sv_quant_cols_e4m3: dst_q must be 16-byte aligned");
  SV_REQUIRE(((uintptr_t)src & (src_dtype == SV_BF16 ? 1 : 3)) == 0, "sv_quant_cols_e4m3: src is not aligned to its element");
  SV_REQUIRE(cdiv(M, QC_ROWS2) <= 65535, "sv_quant_cols_e4m3: M (%d) is too large", M);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(scales, 0, sizeof(float) * (size_t)C, s) != hipSuccess) return check_launch("sv_quant_cols_e4m3 (clear)");
  const dim3 g1(cdiv(C, QC_COLS), cdiv(M, QC_ROWS1)), g2(cdiv(C, QC_COLS), Mp / QC_ROWS2);
  uint8_t* dst = static_cast<uint8_t*>(dst_q);
  if (src_dtype == SV_BF16) hipLaunchKernelGGL(quant_cols_amax_kernel<__bf16>, g1, dim3(256), 0, s, static_cast<const __bf16*>(src), M, C, (long long)ld, reinterpret_cast<int*>(scales), colsum);
  else hipLaunchKernelGGL(quant_cols_amax_kernel<float>, g1, dim3(256), 0, s, static_cast<const float*>(src), M, C, (long long)ld, reinterpret_cast<int*>(scales), colsum);
  hipLaunchKernelGGL(quant_cols_scale_kernel, dim3(cdiv(C, 256)), dim3(256), 0, s, scales, C);
  if (src_dtype == SV_BF16) hipLaunchKernelGGL(quant_cols_write_kernel<__bf16>, g2, dim3(256), 0, s, static_cast<const __bf16*>(src), M, C, (long long)ld, scales, dst, Mp);
  else hipLaunchKernelGGL(quant_cols_write_kernel<float>, g2, dim3(256), 0, s, static_cast<const float*>(src), M, C, (long long)ld, scales, dst, Mp);
  return check_launch("sv_quant_cols_e4m3");
}

extern "C" int sv_linear_fp8_dgrad_supported(int N, int K, const sv_epilogue* e, int math, int act_dtype) {
  const char* why;
  return (N > 0 && K > 0 && math == SV_MATH_BF16 && (act_dtype == SV_F32 || act_dtype == SV_BF16) && linear_fp8_dgrad_epilogue_ok(e, K, &why)) ? 1 : 0;
}

extern "C" long long sv_linear_fp8_bwd_launches(int which) {
  return (which == 0 || which == 1) ? linear_fp8_bwd_launches[which].load(std::memory_order_relaxed) : -1;
}

extern "C" int sv_linear_fp8_dgrad(const void* dq, const float* sd, const void* wtq, const float* swt, void* dx, int M, int N, int K, const sv_epilogue* e,
                                   int act_dtype, void* stream) {
  SV_REQUIRE(dq && sd && wtq && swt && dx && e, "sv_linear_fp8_dgrad: null argument");
  SV_REQUIRE_ACT(act_dtype);
  SV_REQUIRE(M > 0 && N > 0 && K > 0, "sv_linear_fp8_dgrad: M (%d), N (%d), K (%d) must be positive", M, N, K);
  const char* why;
  SV_REQUIRE(linear_fp8_dgrad_epilogue_ok(e, K, &why), "sv_linear_fp8_dgrad: %s", why);
  SV_REQUIRE((((uintptr_t)dq | (uintptr_t)wtq) & 15) == 0, "sv_linear_fp8_dgrad: quantised operands must be 16-byte aligned");
  const uintptr_t amask = act_dtype == SV_BF16 ? 1 : 3;
  SV_REQUIRE((((uintptr_t)dx | (uintptr_t)e->act_grad_src) & amask) == 0, "sv_linear_fp8_dgrad: dx / act_grad_src are not aligned to their element");
  const long long tiles = (long long)cdiv(M, LF_BM) * cdiv(K, LF_BN);
  SV_REQUIRE(tiles < (1ll << 31), "sv_linear_fp8_dgrad: too many tiles");
  LinFp8DgradArgs a{static_cast<const uint8_t*>(dq), sd, static_cast<const uint8_t*>(wtq), swt, dx, M, K, cdiv(N, LF_BK) * LF_BK,
                    e->act_grad_src, e->act_grad_kind, e->slope, e->ldc};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)tiles), block(256);
  if (act_dtype == SV_BF16) hipLaunchKernelGGL((linear_fp8_dgrad_kernel<__bf16, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((linear_fp8_dgrad_kernel<float, false>), grid, block, 0, s, a);
  const int rc = check_launch("sv_linear_fp8_dgrad");
  if (rc == SV_OK) linear_fp8_bwd_launches[0].fetch_add(1, std::memory_order_relaxed);
  return rc;
}

extern "C" int sv_linear_fp8_wgrad(const void* dyt, const float* sdc, const void* xt, const float* sxc, float* dw, int M, int N, int K, int ldw, int splits,
                                   void* stream) {
  SV_REQUIRE(dyt && sdc && xt && sxc && dw, "sv_linear_fp8_wgrad: null argument");
  SV_REQUIRE(M > 0 && N > 0 && K > 0 && ldw >= K, "sv_linear_fp8_wgrad: M (%d), N (%d), K (%d) must be positive, ldw (%d) >= K", M, N, K, ldw);
  SV_REQUIRE(splits >= 0, "sv_linear_fp8_wgrad: splits (%d) must be >= 0", splits);
  SV_REQUIRE((((uintptr_t)dyt | (uintptr_t)xt) & 15) == 0 && ((uintptr_t)dw & 3) == 0, "sv_linear_fp8_wgrad: operands are not aligned");
  const long long tiles = (long long)cdiv(N, LF_BM) * cdiv(K, LF_BN);
  SV_REQUIRE(tiles < (1ll << 31), "sv_linear_fp8_wgrad: too many tiles");
  const int nk = cdiv(M, LF_BK);
  if (splits == 0) splits = (int)((2 * 256 + tiles - 1) / tiles);   // two workgroups for each of the 256 CUs
  splits = splits < nk ? splits : nk;
  if (splits > 65535) splits = 65535;
  LinFp8WgradArgs a{static_cast<const uint8_t*>(dyt), sdc, static_cast<const uint8_t*>(xt), sxc, dw, N, K, nk * LF_BK, ldw, splits};
  hipLaunchKernelGGL(linear_fp8_wgrad_kernel, dim3((unsigned)tiles, (unsigned)splits), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  const int rc = check_launch("sv_linear_fp8_wgrad");
  if (rc == SV_OK) linear_fp8_bwd_launches[1].fetch_add(1, std::memory_order_relaxed);
  return rc;
}

// ---- MX backward --------------------------------------------------------------------------------------------------------------------------------
extern "C" long long sv_linear_mxfp8_bwd_launches(int which) {
  return (which == 0 || which == 1) ? linear_mxfp8_bwd_launches[which].load(std::memory_order_relaxed) : -1;
}
extern "C" long long sv_quant_cols_mx_launches(void) { return quant_cols_mx_launches.load(std::memory_order_relaxed); }

extern "C" int sv_quant_cols_mx_e4m3(const void* src, int src_dtype, int M, int C, int ld, void* dst_q, int Mp, void* scales_u8, float* colsum, void* stream) {
  SV_REQUIRE(src && dst_q && scales_u8, "sv_quant_cols_mx_e4m3: null argument");
  SV_REQUIRE(src_dtype == SV_F32 || src_dtype == SV_BF16, "sv_quant_cols_mx_e4m3: bad source dtype %d", src_dtype);
  SV_REQUIRE(M > 0 && C > 0 && ld >= C, "sv_quant_cols_mx_e4m3: M (%d) and C (%d) must be positive, ld (%d) >= C", M, C, ld);
  SV_REQUIRE(Mp >= M && Mp % 128 == 0 && Mp - M < 128, "sv_quant_cols_mx_e4m3: Mp (%d) must be M (%d) rounded up to a multiple of 128", Mp, M);
  SV_REQUIRE(((uintptr_t)dst_q & 15) == 0 && ((uintptr_t)scales_u8 & 3) == 0, "sv_quant_cols_mx_e4m3: dst_q must be 16-byte aligned, scales_u8 4-byte aligned");
  SV_REQUIRE(((uintptr_t)src & (src_dtype == SV_BF16 ? 1 : 3)) == 0 && ((uintptr_t)colsum & 3) == 0, "sv_quant_cols_mx_e4m3: src / colsum are not aligned to their element");
  SV_REQUIRE(cdiv(M, QC_ROWS2) <= 65535, "sv_quant_cols_mx_e4m3: M (%d) is too large", M);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(cdiv(C, QC_COLS), Mp / QC_ROWS2);
  uint8_t* q = static_cast<uint8_t*>(dst_q);
  uint8_t* sc = static_cast<uint8_t*>(scales_u8);
  if (src_dtype == SV_BF16) hipLaunchKernelGGL(quant_cols_mx_kernel<__bf16>, grid, dim3(256), 0, s, static_cast<const __bf16*>(src), M, C, (long long)ld, q, Mp, sc, colsum);
  else hipLaunchKernelGGL(quant_cols_mx_kernel<float>, grid, dim3(256), 0, s, static_cast<const float*>(src), M, C, (long long)ld, q, Mp, sc, colsum);
  const int rc = check_launch("sv_quant_cols_mx_e4m3");
  if (rc == SV_OK) quant_cols_mx_launches.fetch_add(1, std::memory_order_relaxed);
  return rc;
}

extern "C" long long sv_mx_rows_to_cols_launches(void) { return mx_rows_to_cols_launches.load(std::memory_order_relaxed); }

extern "C" int sv_mx_rows_to_cols(const void* xq, int Kp, const void* xs, int M, int K, void* dst_q, int Mp, void* scales_u8, void* stream) {
  SV_REQUIRE(xq && xs && dst_q && scales_u8, "sv_mx_rows_to_cols: null argument");
  SV_REQUIRE(M > 0 && K > 0, "sv_mx_rows_to_cols: M (%d) and K (%d) must be positive", M, K);
  SV_REQUIRE(Kp == cdiv(K, 128) * 128, "sv_mx_rows_to_cols: Kp (%d) must be K (%d) rounded up to a multiple of 128", Kp, K);
  SV_REQUIRE(Mp == cdiv(M, 128) * 128, "sv_mx_rows_to_cols: Mp (%d) must be M (%d) rounded up to a multiple of 128", Mp, M);
  SV_REQUIRE((((uintptr_t)xq | (uintptr_t)dst_q) & 15) == 0, "sv_mx_rows_to_cols: xq and dst_q must be 16-byte aligned");
  SV_REQUIRE((((uintptr_t)xs | (uintptr_t)scales_u8) & 3) == 0, "sv_mx_rows_to_cols: xs and scales_u8 must be 4-byte aligned");
  SV_REQUIRE(Mp / RB_ROWS <= 65535, "sv_mx_rows_to_cols: M (%d) is too large", M);
  const dim3 grid(Kp / RB_COLS, Mp / RB_ROWS);
  hipLaunchKernelGGL(mx_rows_to_cols_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const uint8_t*>(xq), Kp,
                     static_cast<const uint8_t*>(xs), M, K, static_cast<uint8_t*>(dst_q), Mp, static_cast<uint8_t*>(scales_u8));
  const int rc = check_launch("sv_mx_rows_to_cols");
  if (rc == SV_OK) mx_rows_to_cols_launches.fetch_add(1, std::memory_order_relaxed);
  return rc;
}

extern "C" long long sv_quant_rows_cols_mx_launches(void) { return quant_rows_cols_mx_launches.load(std::memory_order_relaxed); }

template <typename T>
static void launch_quant_rows_cols_mx(dim3 grid, hipStream_t s, const void* src, int M, int N, int ld, uint8_t* rq, int Np, uint8_t* rs, uint8_t* cq, int Mp,
                                      uint8_t* cs, float* colsum) {
  if (rq) hipLaunchKernelGGL((quant_rows_cols_mx_kernel<T, true>), grid, dim3(256), 0, s, static_cast<const T*>(src), M, N, (long long)ld, rq, Np, rs, cq, Mp, cs, colsum);
  else hipLaunchKernelGGL((quant_rows_cols_mx_kernel<T, false>), grid, dim3(256), 0, s, static_cast<const T*>(src), M, N, (long long)ld, rq, Np, rs, cq, Mp, cs, colsum);
}

extern "C" int sv_quant_rows_cols_mx_e4m3(const void* src, int src_dtype, int M, int N, int ld, void* row_q, int Np, void* row_s, void* col_q, int Mp,
                                          void* col_s, float* colsum, void* stream) {
  SV_REQUIRE(src && col_q && col_s, "sv_quant_rows_cols_mx_e4m3: null argument (src, col_q and col_s are required)");
  SV_REQUIRE((row_q != nullptr) == (row_s != nullptr), "sv_quant_rows_cols_mx_e4m3: row_q and row_s go together");
  SV_REQUIRE(src_dtype == SV_F32 || src_dtype == SV_BF16, "sv_quant_rows_cols_mx_e4m3: bad source dtype %d", src_dtype);
  SV_REQUIRE(M > 0 && N > 0 && ld >= N, "sv_quant_rows_cols_mx_e4m3: M (%d) and N (%d) must be positive, ld (%d) >= N", M, N, ld);
  SV_REQUIRE(Np == cdiv(N, 128) * 128, "sv_quant_rows_cols_mx_e4m3: Np (%d) must be N (%d) rounded up to a multiple of 128", Np, N);
  SV_REQUIRE(Mp == cdiv(M, 128) * 128, "sv_quant_rows_cols_mx_e4m3: Mp (%d) must be M (%d) rounded up to a multiple of 128", Mp, M);
  SV_REQUIRE((((uintptr_t)row_q | (uintptr_t)col_q) & 15) == 0, "sv_quant_rows_cols_mx_e4m3: row_q and col_q must be 16-byte aligned");
  SV_REQUIRE((((uintptr_t)row_s | (uintptr_t)col_s) & 3) == 0, "sv_quant_rows_cols_mx_e4m3: row_s and col_s must be 4-byte aligned");
  SV_REQUIRE(((uintptr_t)src & (src_dtype == SV_BF16 ? 1 : 3)) == 0 && ((uintptr_t)colsum & 3) == 0, "sv_quant_rows_cols_mx_e4m3: src / colsum are not aligned to their element");
  SV_REQUIRE(Mp / DQ_ROWS <= 65535, "sv_quant_rows_cols_mx_e4m3: M (%d) is too large", M);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(Np / DQ_COLS, Mp / DQ_ROWS);
  uint8_t *rq = static_cast<uint8_t*>(row_q), *rs = static_cast<uint8_t*>(row_s), *cq = static_cast<uint8_t*>(col_q), *cs = static_cast<uint8_t*>(col_s);
  if (src_dtype == SV_BF16) launch_quant_rows_cols_mx<__bf16>(grid, s, src, M, N, ld, rq, Np, rs, cq, Mp, cs, colsum);
  else launch_quant_rows_cols_mx<float>(grid, s, src, M, N, ld, rq, Np, rs, cq, Mp, cs, colsum);
  const int rc = check_launch("sv_quant_rows_cols_mx_e4m3");
  if (rc == SV_OK) quant_rows_cols_mx_launches.fetch_add(1, std::memory_order_relaxed);
  return rc;
}

extern "C" int sv_linear_mxfp8_dgrad(const void* dq, const void* ds, const void* wtq, const void* wts, void* dx, int M, int N, int K, const sv_epilogue* e,
                                     int act_dtype, void* stream) {
  SV_REQUIRE(dq && ds && wtq && wts && dx && e, "sv_linear_mxfp8_dgrad: null argument");
  SV_REQUIRE_ACT(act_dtype);
  SV_REQUIRE(M > 0 && N > 0 && K > 0, "sv_linear_mxfp8_dgrad: M (%d), N (%d), K (%d) must be positive", M, N, K);
  const char* why;
  SV_REQUIRE(linear_fp8_dgrad_epilogue_ok(e, K, &why), "sv_linear_mxfp8_dgrad: %s", why);
  SV_REQUIRE((((uintptr_t)dq | (uintptr_t)wtq) & 15) == 0, "sv_linear_mxfp8_dgrad: quantised operands must be 16-byte aligned");
  SV_REQUIRE((((uintptr_t)ds | (uintptr_t)wts) & 3) == 0, "sv_linear_mxfp8_dgrad: scale bytes must be 4-byte aligned");
  const uintptr_t amask = act_dtype == SV_BF16 ? 1 : 3;
  SV_REQUIRE((((uintptr_t)dx | (uintptr_t)e->act_grad_src) & amask) == 0, "sv_linear_mxfp8_dgrad: dx / act_grad_src are not aligned to their element");
  const long long tiles = (long long)cdiv(M, LF_BM) * cdiv(K, LF_BN);
  SV_REQUIRE(tiles < (1ll << 31), "sv_linear_mxfp8_dgrad: too many tiles");
  LinMxDgradArgs a{static_cast<const uint8_t*>(dq), static_cast<const uint8_t*>(ds), static_cast<const uint8_t*>(wtq), static_cast<const uint8_t*>(wts), dx,
                   M, K, cdiv(N, LF_BK) * LF_BK, e->act_grad_src, e->act_grad_kind, e->slope, e->ldc};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)tiles), block(256);
  if (act_dtype == SV_BF16) hipLaunchKernelGGL((linear_fp8_dgrad_kernel<__bf16, true, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((linear_fp8_dgrad_kernel<float, false, true>), grid, block, 0, s, a);
  const int rc = check_launch("sv_linear_mxfp8_dgrad");
  if (rc == SV_OK) linear_mxfp8_bwd_launches[0].fetch_add(1, std::memory_order_relaxed);
  return rc;
}

// the number of splits a call resolves to: the request (0 = two workgroups for each of 256 CUs), at most one per 128 tokens and the grid's y limit
static int mxfp8_wgrad_splits(int M, int N, int K, int splits) {
  const long long tiles = (long long)cdiv(N, LF_BM) * cdiv(K, LF_BN);
  const int nk = cdiv(M, LF_BK);
  if (splits == 0) splits = (int)((2 * 256 + tiles - 1) / tiles);
  splits = splits < nk ? splits : nk;
  return splits > 65535 ? 65535 : splits;
}

extern "C" size_t sv_linear_mxfp8_wgrad_workspace_floats(int M, int N, int K, int splits) {
  if (M <= 0 || N <= 0 || K <= 0 || splits < 0) return 0;
  const int sp = mxfp8_wgrad_splits(M, N, K, splits);
  return sp > 1 ? (size_t)sp * (size_t)N * (size_t)K : 0;
}

extern "C" int sv_linear_mxfp8_wgrad(const void* dyt, const void* dys, const void* xt, const void* xs, float* dw, int M, int N, int K, int ldw, int splits,
                                     float* workspace, void* stream) {
  SV_REQUIRE(dyt && dys && xt && xs && dw, "sv_linear_mxfp8_wgrad: null argument");
  SV_REQUIRE(M > 0 && N > 0 && K > 0 && ldw >= K, "sv_linear_mxfp8_wgrad: M (%d), N (%d), K (%d) must be positive, ldw (%d) >= K", M, N, K, ldw);
  SV_REQUIRE(splits >= 0, "sv_linear_mxfp8_wgrad: splits (%d) must be >= 0", splits);
  SV_REQUIRE((((uintptr_t)dyt | (uintptr_t)xt) & 15) == 0 && (((uintptr_t)dys | (uintptr_t)xs | (uintptr_t)dw) & 3) == 0, "sv_linear_mxfp8_wgrad: operands are not aligned");
  SV_REQUIRE(((uintptr_t)workspace & 15) == 0, "sv_linear_mxfp8_wgrad: workspace must be 16-byte aligned");
  const long long tiles = (long long)cdiv(N, LF_BM) * cdiv(K, LF_BN);
  SV_REQUIRE(tiles < (1ll << 31), "sv_linear_mxfp8_wgrad: too many tiles");
  const int nk = cdiv(M, LF_BK);
  splits = mxfp8_wgrad_splits(M, N, K, splits);
  SV_REQUIRE(splits == 1 || workspace, "sv_linear_mxfp8_wgrad: %d splits need a workspace of sv_linear_mxfp8_wgrad_workspace_floats floats", splits);
  LinMxWgradArgs a{static_cast<const uint8_t*>(dyt), static_cast<const uint8_t*>(dys), static_cast<const uint8_t*>(xt), static_cast<const uint8_t*>(xs), dw,
                   workspace, N, K, nk * LF_BK, ldw, splits};
  const int vec = ((K | ldw) & 3) == 0 && ((uintptr_t)dw & 15) == 0;   // the reduce kernel's 16-byte form
  const size_t items = vec ? (size_t)N * (K >> 2) : (size_t)N * K;
  SV_REQUIRE(items / 256 + 1 < (1ull << 31), "sv_linear_mxfp8_wgrad: dw is too large");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(linear_mxfp8_wgrad_kernel, dim3((unsigned)tiles, (unsigned)splits), dim3(256), 0, s, a);
  if (splits > 1) {
    hipLaunchKernelGGL(linear_mxfp8_wgrad_reduce_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, workspace, dw, N, K, ldw, splits, vec);
  }
  const int rc = check_launch("sv_linear_mxfp8_wgrad");
  if (rc == SV_OK) linear_mxfp8_bwd_launches[1].fetch_add(1, std::memory_order_relaxed);
  return rc;
}
