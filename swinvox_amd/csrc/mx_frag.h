// MXFP8 operand fragments of the fused stage-0 kernels (swin_mlp.hip: swin_mlp_*_mx_kernel; attn.hip: swin_attn_block_fwd_mx_kernel) on
// v_mfma_scale_f32_16x16x128_f8f6f4.  The ONLY copy of: the layout of a weight image in fragment order (mx_pack_item / mx_a_frag / mx_a_scale),
// the token-row quantiser on the B-operand lane map (mx_quant_frag) and the LayerNorm prologue on that map (mx_layernorm).  The rounding itself
// is mx_block_exp / pack4_e4m3_mx of common.h (NORMATIVE recipe: linear_fp8.hip "MX recipe").
//   B operand (tokens on the columns): lane l = (t = l & 15, lg = l >> 4) holds token t; its data registers 0-3 are k = 16 lg .. + 15 and 4-7 are
//   k = 64 + 16 lg .. + 15 of a 128-wide k-step, the scale byte it passes covers k = 32 lg .. + 31 (linear_fp8.hip, lf_contract).
//   A operand (16 weight rows per tile): lane (r, lg) holds row r of the tile, the same k as above, and the row's scale byte of block lg.
#pragma once
#include "common.h"

namespace sv {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// item e = (tile, lane) of an image: the lane's two 16-byte halves (k = 16 lg .. and 64 + 16 lg .. of the row's 128-wide k-step at `src`) and its scale byte
__device__ __forceinline__ void mx_pack_item(const uint8_t* src, uint8_t scale, uint8_t* data, uint8_t* scales, int e) {
  i32x4* d = reinterpret_cast<i32x4*>(data) + (e >> 6) * 128 + (e & 63);
  d[0] = *reinterpret_cast<const i32x4*>(src);
  d[64] = *reinterpret_cast<const i32x4*>(src + 64);
  scales[e] = scale;
}

// maximum of a lane's value and that of lane ^ 16 (the other half of a 32-element MX block)
__device__ __forceinline__ float pair16_max(float v) { float w = v; permlane16_pair(v, w); return fmaxf(v, w); }
// the E8M0 byte lane group lg passes to the MFMA (block lg of the k-step) from the bytes the lanes know: lane group lg' knows blocks lg' >> 1 (its
// registers 0-3, `elo`) and 2 + (lg' >> 1) (registers 4-7, `ehi`)
__device__ __forceinline__ int mx_lane_scale(int elo, int ehi, int lane) {
  const int lg = lane >> 4;
  const int got = __shfl((elo + 127) | ((ehi + 127) << 8), (lane & 15) + 32 * (lg & 1));
  return (got >> (8 * (lg >> 1))) & 0xff;
}

// a token's 16 + 16 values (registers 0-3 / 4-7 of a 128-wide k-step; already rounded to bf16) -> MX B fragment + the scale byte the lane passes
__device__ __forceinline__ void mx_quant_frag(const float (&v)[2][16], i32x8& q, int& sbyte, int lane) {
  int e[2];
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) {
    float m = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) m = fmaxf(m, fabsf(v[hf][j]));
    e[hf] = mx_block_exp(pair16_max(m));
#pragma unroll
    for (int w = 0; w < 4; ++w) q[4 * hf + w] = (int)pack4_e4m3_mx(v[hf][4 * w], v[hf][4 * w + 1], v[hf][4 * w + 2], v[hf][4 * w + 3], e[hf]);
  }
  sbyte = mx_lane_scale(e[0], e[1], lane);
}

// A fragment of row tile `tile` of an image: two 16-byte reads at + 0 / + 1024 (ds_read_b128 where `data` is in LDS, global loads where it is the
// pack in memory: the address space is inferred) - and its scale byte
__device__ __forceinline__ i32x8 mx_a_frag(const uint8_t* data, int tile, int lane) {
  const uint8_t* fa = data + (size_t)(tile * 2) * 1024 + lane * 16;
  const i32x4 lo = *reinterpret_cast<const i32x4*>(fa), hi = *reinterpret_cast<const i32x4*>(fa + 1024);
  return (i32x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
__device__ __forceinline__ int mx_a_scale(const uint8_t* scales, int tile, int lane) { return scales[tile * 64 + lane]; }

// LayerNorm prologue of lane (t, lg): the 16 + 16 channels 64 hf + 16 lg .. + 15 of token `tok` (zero for an invalid token and for the padding of
// C = 96) -> xv = LayerNorm in fp32, rounded to bf16 as the unfused chain stores it; mean and rstd of the row.  The backward (WITH_DX2) passes dx2
// as well: dv = bf16(dsc dx2) of the same channels, loaded under the same guard (sv_rowscale's value).
template <int C, bool WITH_DX2>
__device__ __forceinline__ void mx_layernorm(const __bf16* x1, long long tok, bool valid, int lg, const float* sgam, const float* sbet, float eps,
                                             float (&xv)[2][16], float& mean, float& rstd, const __bf16* dx2 = nullptr, float dsc = 1.f,
                                             float (*dv)[16] = nullptr) {
  const bool hi_live = 64 + 16 * lg < C;                   // C = 96: channels 96 .. 127 are padding
  float s = 0.f;
#pragma unroll
  for (int hf = 0; hf < 2; ++hf)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      bf16x8 raw = VecN<__bf16, 8>::zero(), dr = VecN<__bf16, 8>::zero();
      if (valid && (hf == 0 || hi_live)) {
        raw = *reinterpret_cast<const bf16x8*>(x1 + tok * C + 64 * hf + 16 * lg + 8 * u);
        if constexpr (WITH_DX2) dr = *reinterpret_cast<const bf16x8*>(dx2 + tok * C + 64 * hf + 16 * lg + 8 * u);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        xv[hf][8 * u + j] = (float)raw[j]; s += xv[hf][8 * u + j];
        if constexpr (WITH_DX2) dv[hf][8 * u + j] = (float)(__bf16)(dsc * (float)dr[j]);
      }
    }
  s = lane_step_add<16>(s); s = lane_step_add<32>(s);
  mean = s * (1.f / C);
  float q = 0.f;
#pragma unroll
  for (int hf = 0; hf < 2; ++hf)
    if (hf == 0 || hi_live)
#pragma unroll
      for (int j = 0; j < 16; ++j) { const float d = xv[hf][j] - mean; q += d * d; }
  q = lane_step_add<16>(q); q = lane_step_add<32>(q);
  rstd = rsqrtf(q * (1.f / C) + eps);
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) {
    const bool live = hf == 0 || hi_live;
    const int c0 = live ? 64 * hf + 16 * lg : 0;
#pragma unroll
    for (int j = 0; j < 16; ++j)
      xv[hf][j] = live ? (float)(__bf16)((xv[hf][j] - mean) * rstd * sgam[c0 + j] + sbet[c0 + j]) : 0.f;
  }
}

}  // namespace sv
