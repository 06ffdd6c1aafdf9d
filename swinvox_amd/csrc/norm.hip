// Normalisation kernels (HBM-bound): token LayerNorm (+ fused PatchMerging gather), whole-image
// LayerNorm([C,H,W]) of the Swin stage heads, BatchNorm statistics / apply / backward on channels-last data.
#include "common.h"
#include <atomic>
#include <initializer_list>

namespace sv {

// ------------------------------------------------------------------------------------------------
// token LayerNorm.  A row is handled by LPR lanes (16, 32 or 64) holding NV chunks of VEC elements each in registers
// (two-pass variance), so a wave normalises 64/LPR rows at once and narrow rows (C = 96 ... 384) keep 75 % of the lanes
// busy; VEC = 8 (16-byte accesses) with bf16 storage, 4 otherwise.
// MERGE: the row is the PatchMerging gather of 4 tokens (order h0w0,h1w0,h0w1,h1w1) of a [I,H,W,C0] map.
// QUANT (sv_layernorm_quant_fwd): the lane group also emits the operand row sv_linear_fp8 reads - the e4m3 bytes and the scale of the row AS
// STORED (rounded to the storage type first), by the recipe of linear_fp8.hip: one more lane-group reduction (the maximum) and one more
// store per chunk, no second kernel and no second read.  y / mean / rstd are then optional (inference stores only the bytes).
// MX (sv_layernorm_quant_mx_fwd): the same for the operand rows sv_linear_mxfp8 reads - one E8M0 scale per 32 columns.  The 32 columns of a
// block are the chunks of 32 / VEC adjacent lanes (8 at VEC 4, 4 at VEC 8; LPR is a multiple of 8, so chunk gl + LPR i sits in an aligned lane
// group for every i): the block maximum is the first three (two) DPP steps of group_max, and nothing is divided out.
// ------------------------------------------------------------------------------------------------
// Contention-free reductions across workgroups: partial sums go (atomically) into one of NSLOT accumulator images chosen by
// the workgroup index and a tiny second kernel folds the images.  (A "last workgroup folds" ticket would need a device-scope
// __threadfence(), which writes back the whole per-XCD L2 on this chip - measured 100+ us per call.)
constexpr int BN_BWD_SLOTS = 16, LN_BWD_SLOTS = 32;

struct MergeMap { int H, W, C0; };  // H,W of the un-merged map

template <bool MERGE>
__device__ __forceinline__ size_t ln_src_off(long long row, int e, int C, const MergeMap& mm) {   // e = first element of the chunk
  if constexpr (!MERGE) return (size_t)row * C + e;
  const int blk = e / mm.C0, c = e - blk * mm.C0;   // blk = wp*2 + hp
  const int wp = blk >> 1, hp = blk & 1;
  const int W2 = mm.W >> 1, H2 = mm.H >> 1;
  const int x2 = (int)(row % W2); long long t = row / W2;
  const int y2 = (int)(t % H2); const long long i = t / H2;
  return ((size_t)(i * mm.H + 2 * y2 + hp) * mm.W + (2 * x2 + wp)) * mm.C0 + c;
}

template <int VEC, typename AT> struct LnIO;
template <typename AT> struct LnIO<4, AT> {
  static __device__ __forceinline__ void load(const AT* p, float* v) { const float4 q = ld4f(p); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
  static __device__ __forceinline__ void store(AT* p, const float* v) { st4f(p, make_float4(v[0], v[1], v[2], v[3])); }
};
template <> struct LnIO<8, __bf16> {
  static __device__ __forceinline__ void load(const __bf16* p, float* v) {
    const bf16x8 q = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)q[j];
  }
  static __device__ __forceinline__ void store(__bf16* p, const float* v) {
    bf16x8 q;
#pragma unroll
    for (int j = 0; j < 8; ++j) q[j] = (__bf16)v[j];
    *reinterpret_cast<bf16x8*>(p) = q;
  }
};
__device__ __forceinline__ void ldp(const float* p, float* v, int n) {   // n = 4 or 8 fp32 parameters
  const float4 a = *reinterpret_cast<const float4*>(p);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  if (n == 8) { const float4 b = *reinterpret_cast<const float4*>(p + 4); v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w; }
}
template <int CTRL> __device__ __forceinline__ float ln_dpp_mov(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {   // sum over the LPR (16 / 32 / 64) lanes that share a row, every lane gets it
  // inside a 16-lane DPP row: quad_perm xor 1, xor 2, row_half_mirror, row_mirror (VALU moves, no LDS crossbar round trips)
  v += ln_dpp_mov<0xB1>(v); v += ln_dpp_mov<0x4E>(v); v += ln_dpp_mov<0x141>(v); v += ln_dpp_mov<0x140>(v);
  if constexpr (LPR > 16) v = lane_step_add<16>(v);     // across rows: v_permlane16 / 32 swaps (common.h), VALU as well
  if constexpr (LPR > 32) v = lane_step_add<32>(v);
  return v;
}

template <int LPR>
__device__ __forceinline__ float group_max(float v) {   // maximum over the same lanes (values >= 0: the DPP moves read 0 where they have no source)
  v = fmaxf(v, ln_dpp_mov<0xB1>(v)); v = fmaxf(v, ln_dpp_mov<0x4E>(v)); v = fmaxf(v, ln_dpp_mov<0x141>(v)); v = fmaxf(v, ln_dpp_mov<0x140>(v));
  if constexpr (LPR > 16) { float w = v; permlane16_pair(v, w); v = fmaxf(v, w); }
  if constexpr (LPR > 32) { float w = v; permlane32_pair(v, w); v = fmaxf(v, w); }
  return v;
}

template <int VEC>
__device__ __forceinline__ float block32_max(float v) {   // maximum over the 32 / VEC adjacent lanes that hold one 32-column block (values >= 0)
  v = fmaxf(v, ln_dpp_mov<0xB1>(v)); v = fmaxf(v, ln_dpp_mov<0x4E>(v));
  if constexpr (VEC == 4) v = fmaxf(v, ln_dpp_mov<0x141>(v));
  return v;
}

// the outputs only the quantising forms have
struct LnQuantOut { uint8_t* q; float* scales; int Kp; };   // q [rows][Kp] e4m3 bytes, scales [rows]
struct LnQuantMxOut { uint8_t* q; uint8_t* scales; int Kp; };   // q [rows][Kp] e4m3 bytes, scales [rows][Kp / 32] E8M0 bytes
__device__ __forceinline__ const LnQuantOut& ln_quant_out(const LnQuantOut& o) { return o; }
__device__ __forceinline__ const LnQuantMxOut& ln_quant_out(const LnQuantMxOut& o) { return o; }
template <typename... QO> struct LnIsMx { static constexpr bool value = false; };
template <> struct LnIsMx<LnQuantMxOut> { static constexpr bool value = true; };

// QO is empty (the plain forward: y, mean_out, rstd_out required; its argument list, and with it its code, is what it was before the
// quantising form existed), one LnQuantOut (QUANT: q and scales are written as well, and y / (mean_out, rstd_out) are skipped when null) or
// one LnQuantMxOut (QUANT and MX: the same with one scale byte per 32 columns).
template <bool MERGE, typename AT, int VEC, int LPR, int NV, typename... QO>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const AT* __restrict__ x, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, AT* __restrict__ y,
                                                     float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                     long long rows, int C, float eps, MergeMap mm, QO... qo_) {
  constexpr bool QUANT = sizeof...(QO) == 1;
  constexpr bool MX = LnIsMx<QO...>::value;
  // MX: a 32-column block must be an aligned group of 32 / VEC lanes inside the row's lane group for every i, and one pass of the lane group
  // must cover the (at most 3) scale bytes of the blocks that lie wholly in the padding
  static_assert(!MX || (LPR % 8 == 0 && LPR >= 4 && (VEC == 4 || VEC == 8)), "MX form: LPR must be a multiple of 8, VEC 4 or 8");
  constexpr int RPW = 64 / LPR;                       // rows per wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gl = lane % LPR, gr = lane / LPR;
  const long long row = ((long long)blockIdx.x * 4 + wave) * RPW + gr;
  const bool rok = row < rows;
  const int nchunk = C / VEC;
  float v[NV][VEC];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int ch = gl + LPR * i;
    if (rok && ch < nchunk) {
      LnIO<VEC, AT>::load(x + ln_src_off<MERGE>(row, ch * VEC, C, mm), v[i]);
#pragma unroll
      for (int j = 0; j < VEC; ++j) s += v[i][j];
    }
  }
  const float invC = 1.f / C;                                   // one division per thread, not two per row
  const float mean = group_sum<LPR>(s) * invC;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int ch = gl + LPR * i;
    if (rok && ch < nchunk) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) { const float a = v[i][j] - mean; sq += a * a; }
    }
  }
  const float rstd = rsqrtf(group_sum<LPR>(sq) * invC + eps);
  if (rok && gl == 0 && (!QUANT || mean_out)) { mean_out[row] = mean; rstd_out[row] = rstd; }
  float amax = 0.f;
  int bexp[MX ? NV : 1];                                        // MX: the exponent of the block chunk i of this lane lies in
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int ch = gl + LPR * i;
    if constexpr (MX) amax = 0.f;                               // per block, not per row; lanes without a chunk contribute 0
    if (rok && ch < nchunk) {
      float g[VEC], b[VEC], o[VEC];
      ldp(gamma + ch * VEC, g, VEC); ldp(beta + ch * VEC, b, VEC);
#pragma unroll
      for (int j = 0; j < VEC; ++j) o[j] = (v[i][j] - mean) * rstd * g[j] + b[j];
      if constexpr (QUANT) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {   // the STORED value takes the place of x in the registers: it is what the quantiser of the row sees
          o[j] = (float)(AT)o[j]; v[i][j] = o[j];
          amax = fmaxf(amax, fabsf(o[j]));
        }
        if (y) LnIO<VEC, AT>::store(y + (size_t)row * C + ch * VEC, o);
      } else {
        LnIO<VEC, AT>::store(y + (size_t)row * C + ch * VEC, o);
      }
    }
    if constexpr (MX) bexp[i] = mx_block_exp(block32_max<VEC>(amax));   // outside the branch: every lane of the wave takes the DPP steps
  }
  if constexpr (MX) {
    const LnQuantMxOut& qo = ln_quant_out(qo_...);
    if (rok) {
      uint8_t* __restrict__ qrow = qo.q + (size_t)row * qo.Kp;
      uint8_t* __restrict__ srow = qo.scales + (size_t)row * (qo.Kp >> 5);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int ch = gl + LPR * i;
        if (ch < nchunk) {   // element k of the row is byte k: VEC bytes per chunk
          const uint32_t lo = pack4_e4m3_mx(v[i][0], v[i][1], v[i][2], v[i][3], bexp[i]);
          if constexpr (VEC == 8) {
            const uint32_t hi = pack4_e4m3_mx(v[i][4], v[i][5], v[i][6], v[i][7], bexp[i]);
            *reinterpret_cast<uint2*>(qrow + ch * 8) = make_uint2(lo, hi);
          } else {
            *reinterpret_cast<uint32_t*>(qrow + ch * 4) = lo;
          }
          // the block's first lane (its chunk starts the block, so it exists whenever any chunk of the block does) writes the scale byte
          if (gl % (32 / VEC) == 0) srow[ch * VEC >> 5] = (uint8_t)(bexp[i] + 127);
        }
      }
      // zero bytes C .. Kp - 1 as the row form does, and byte 127 (E = 0) for the blocks that lie wholly in the padding (at most 3 < LPR)
      for (int w = (C >> 2) + gl; w < (qo.Kp >> 2); w += LPR) reinterpret_cast<uint32_t*>(qrow)[w] = 0u;
      if (((C + 31) >> 5) + gl < (qo.Kp >> 5)) srow[((C + 31) >> 5) + gl] = 127;
    }
  } else if constexpr (QUANT) {
    const float sc = fp8_row_scale(group_max<LPR>(amax));
    const LnQuantOut& qo = ln_quant_out(qo_...);
    if (rok) {
      uint8_t* __restrict__ qrow = qo.q + (size_t)row * qo.Kp;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int ch = gl + LPR * i;
        if (ch < nchunk) {   // element k of the row is byte k: VEC bytes per chunk
          const uint32_t lo = pack4_e4m3(v[i][0] * sc, v[i][1] * sc, v[i][2] * sc, v[i][3] * sc);
          if constexpr (VEC == 8) {
            const uint32_t hi = pack4_e4m3(v[i][4] * sc, v[i][5] * sc, v[i][6] * sc, v[i][7] * sc);
            *reinterpret_cast<uint2*>(qrow + ch * 8) = make_uint2(lo, hi);
          } else {
            *reinterpret_cast<uint32_t*>(qrow + ch * 4) = lo;
          }
        }
      }
      // zero bytes C .. Kp - 1 (C % 4 == 0: whole words; up to 31 of them, the group's registers need not reach Kp)
      for (int w = (C >> 2) + gl; w < (qo.Kp >> 2); w += LPR) reinterpret_cast<uint32_t*>(qrow)[w] = 0u;
      if (gl == 0) qo.scales[row] = sc;
    }
  }
}

// backward: dx = rstd * (g - mean(g) - xhat * mean(g*xhat)), g = dy*gamma; dgamma += dy*xhat, dbeta += dy.
// A workgroup walks rows_per_block rows (each row group a strided subset) with the per-column partial sums in registers;
// they are folded through one LDS image (LDS atomics) and reach HBM as one atomic per column per workgroup.
template <bool MERGE, typename AT, int VEC, int LPR, int NV>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const AT* __restrict__ dy, const AT* __restrict__ x,
                                                     const float* __restrict__ gamma, const float* __restrict__ mean_in,
                                                     const float* __restrict__ rstd_in, AT* __restrict__ dx,
                                                     float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                     long long rows, int C, MergeMap mm, int accumulate_dx, int rows_per_block,
                                                     float* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) float red[];  // [2*C]
  constexpr int RPW = 64 / LPR, RPI = 4 * RPW;   // rows per wave / per workgroup iteration
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gl = lane % LPR, gr = lane / LPR;
  const int nchunk = C / VEC;
  for (int c = threadIdx.x; c < 2 * C; c += 256) red[c] = 0.f;
  float dg[NV][VEC], db[NV][VEC], gm[NV][VEC];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int ch = gl + LPR * i;
#pragma unroll
    for (int j = 0; j < VEC; ++j) { dg[i][j] = 0.f; db[i][j] = 0.f; gm[i][j] = 0.f; }
    if (ch < nchunk) ldp(gamma + ch * VEC, gm[i], VEC);
  }
  const long long r0 = (long long)blockIdx.x * rows_per_block;
  const float invC = 1.f / C;
  // The rows of the NEXT iteration are fetched before this iteration's stores: vmcnt retires in issue order, so loads issued behind a store
  // can only be waited for by draining the store - one store round trip per iteration otherwise.
  float xv[NV][VEC], dv[NV][VEC], ov[NV][VEC], mean = 0.f, rstd = 0.f;
  bool rok = false;
  auto fetch = [&](int rr, float (&xo)[NV][VEC], float (&d_)[NV][VEC], float (&old)[NV][VEC], float& mn, float& rs, bool& ok) {
    const long long row = r0 + rr;
    ok = rr < rows_per_block && row < rows;
    mn = ok ? mean_in[row] : 0.f; rs = ok ? rstd_in[row] : 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int ch = gl + LPR * i;
#pragma unroll
      for (int j = 0; j < VEC; ++j) { xo[i][j] = 0.f; d_[i][j] = 0.f; old[i][j] = 0.f; }
      if (ok && ch < nchunk) {
        LnIO<VEC, AT>::load(x + ln_src_off<MERGE>(row, ch * VEC, C, mm), xo[i]);
        LnIO<VEC, AT>::load(dy + (size_t)row * C + ch * VEC, d_[i]);
        if (accumulate_dx) LnIO<VEC, AT>::load(dx + ln_src_off<MERGE>(row, ch * VEC, C, mm), old[i]);
      }
    }
  };
  fetch(wave * RPW + gr, xv, dv, ov, mean, rstd, rok);
  for (int rr = wave * RPW + gr; rr < rows_per_block; rr += RPI) {   // whole row groups stay in the loop: the group reductions need every lane
    const long long row = r0 + rr;
    float xn[NV][VEC], dn[NV][VEC], on[NV][VEC], mean_n, rstd_n;
    bool rok_n;
    fetch(rr + RPI, xn, dn, on, mean_n, rstd_n, rok_n);
    float xh[NV][VEC], g[NV][VEC];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int ch = gl + LPR * i;
      if (rok && ch < nchunk) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          xh[i][j] = (xv[i][j] - mean) * rstd;
          g[i][j] = dv[i][j] * gm[i][j];
          s1 += g[i][j]; s2 += g[i][j] * xh[i][j];
          dg[i][j] += dv[i][j] * xh[i][j]; db[i][j] += dv[i][j];
        }
      }
    }
    const float m1 = group_sum<LPR>(s1) * invC, m2 = group_sum<LPR>(s2) * invC;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int ch = gl + LPR * i;
      if (rok && ch < nchunk) {
        float o[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = rstd * (g[i][j] - m1 - xh[i][j] * m2) + ov[i][j];
        LnIO<VEC, AT>::store(dx + ln_src_off<MERGE>(row, ch * VEC, C, mm), o);
      }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int j = 0; j < VEC; ++j) { xv[i][j] = xn[i][j]; dv[i][j] = dn[i][j]; ov[i][j] = on[i][j]; }
    mean = mean_n; rstd = rstd_n; rok = rok_n;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int ch = gl + LPR * i;
    if (ch < nchunk) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) { atomicAdd(red + ch * VEC + j, dg[i][j]); atomicAdd(red + C + ch * VEC + j, db[i][j]); }
    }
  }
  __syncthreads();
  // one atomic per column per workgroup into one of LN_BWD_SLOTS images; the last workgroup folds them into dgamma / dbeta
  float* slot = ws + (size_t)(blockIdx.x % LN_BWD_SLOTS) * 2 * C;
  for (int c = threadIdx.x; c < 2 * C; c += 256) atomicAdd(slot + c, red[c]);
}
// dgamma[c] += sum_slot ws[slot][c], dbeta[c] += sum_slot ws[slot][C + c]
__global__ __launch_bounds__(256) void ln_bwd_fold_kernel(const float* __restrict__ ws, int C, float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= 2 * C) return;
  float a = 0.f;
#pragma unroll 8
  for (int sl = 0; sl < LN_BWD_SLOTS; ++sl) a += ws[(size_t)sl * 2 * C + c];
  if (c < C) dgamma[c] += a; else dbeta[c - C] += a;
}

// (LPR, NV) for a row of `chunks` VEC-element chunks; NV is rounded up to an instantiated count
static inline bool ln_shape(int chunks, int& lpr, int& nv) {
  lpr = chunks <= 16 ? 16 : (chunks <= 32 ? 32 : 64);
  const int need = (chunks + lpr - 1) / lpr;
  static const int opts[] = {1, 2, 3, 4, 6, 12};
  for (int o : opts) if (need <= o) { nv = o; return true; }
  return false;
}
#define SV_LN_DISPATCH(LPR_, NV_, ...)                                                       \
  do {                                                                                       \
    if (LPR_ == 16) { constexpr int LPR = 16, NV = 1; __VA_ARGS__ }                          \
    else if (LPR_ == 32) { constexpr int LPR = 32, NV = 1; __VA_ARGS__ }                     \
    else if (NV_ == 1) { constexpr int LPR = 64, NV = 1; __VA_ARGS__ }                       \
    else if (NV_ == 2) { constexpr int LPR = 64, NV = 2; __VA_ARGS__ }                       \
    else if (NV_ == 3) { constexpr int LPR = 64, NV = 3; __VA_ARGS__ }                       \
    else if (NV_ == 4) { constexpr int LPR = 64, NV = 4; __VA_ARGS__ }                       \
    else if (NV_ == 6) { constexpr int LPR = 64, NV = 6; __VA_ARGS__ }                       \
    else { constexpr int LPR = 64, NV = 12; __VA_ARGS__ }                                    \
  } while (0)

// ------------------------------------------------------------------------------------------------
// long-row LayerNorm with a full-size affine (Swin stage heads: nn.LayerNorm([C,H,W]) on NHWC data whose
// affine parameters were transposed to [HW,C] once per step).  L = H*W*C up to 301,056 per image.
// Pass 1: every workgroup reduces a CHUNK of one image to (mean_chunk, M2_chunk); pass 2 merges the
// chunk moments (Chan) and applies the affine (+ optional dropout mask).
// ------------------------------------------------------------------------------------------------
constexpr int LNL_CHUNK = 4096;  // elements per workgroup in pass 1 (16 per thread)

template <typename AT>
__global__ __launch_bounds__(256) void lnl_moments_kernel(const AT* __restrict__ x, float* __restrict__ part, int L, int nchunks) {
  __shared__ float sc[4];
  const int img = blockIdx.y, ck = blockIdx.x;
  const int e0 = ck * LNL_CHUNK;
  int n = L - e0; if (n > LNL_CHUNK) n = LNL_CHUNK;
  const AT* src = x + (size_t)img * L + e0;
  float4 v[4];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = (threadIdx.x + 256 * i) * 4;
    if (e < n) { v[i] = ld4f(src + e); s += v[i].x + v[i].y + v[i].z + v[i].w; }
  }
  const float mean = block_sum<4>(s, sc) / n;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = (threadIdx.x + 256 * i) * 4;
    if (e < n) {
      const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
      q += a * a + b * b + c * c + d * d;
    }
  }
  const float m2 = block_sum<4>(q, sc);
  if (threadIdx.x == 0) {
    part[((size_t)img * nchunks + ck) * 2 + 0] = mean;
    part[((size_t)img * nchunks + ck) * 2 + 1] = m2;
  }
}

__global__ void lnl_finalize_kernel(const float* __restrict__ part, float* __restrict__ meanrstd, int L, int nchunks, float eps, int I) {
  const int img = blockIdx.x * blockDim.x + threadIdx.x;
  if (img >= I) return;
  float n_a = 0.f, mean_a = 0.f, m2_a = 0.f;
  for (int c = 0; c < nchunks; ++c) {
    int nb = L - c * LNL_CHUNK; if (nb > LNL_CHUNK) nb = LNL_CHUNK;
    const float mean_b = part[((size_t)img * nchunks + c) * 2], m2_b = part[((size_t)img * nchunks + c) * 2 + 1];
    const float n = n_a + nb, delta = mean_b - mean_a;
    mean_a += delta * nb / n;
    m2_a += m2_b + delta * delta * n_a * nb / n;
    n_a = n;
  }
  meanrstd[img * 2] = mean_a;
  meanrstd[img * 2 + 1] = rsqrtf(m2_a / L + eps);
}

template <typename AT>
__global__ __launch_bounds__(256) void lnl_apply_kernel(const AT* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ b, const float* __restrict__ meanrstd,
                                                        AT* __restrict__ y, int L, float drop_p, uint32_t seed, const uint32_t* __restrict__ epoch) {
  seed = eff_seed(seed, epoch);
  const int img = blockIdx.y;
  const float mean = meanrstd[img * 2], rstd = meanrstd[img * 2 + 1];
  const float keep_inv = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
  for (int e = (blockIdx.x * 256 + threadIdx.x) * 4; e < L; e += gridDim.x * 1024) {
    const float4 xv = ld4f(x + (size_t)img * L + e);
    const float4 wv = *reinterpret_cast<const float4*>(w + e), bv = *reinterpret_cast<const float4*>(b + e);
    float o[4] = {(xv.x - mean) * rstd * wv.x + bv.x, (xv.y - mean) * rstd * wv.y + bv.y,
                  (xv.z - mean) * rstd * wv.z + bv.z, (xv.w - mean) * rstd * wv.w + bv.w};
    if (drop_p > 0.f) {
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = uniform01(seed, (uint64_t)img * L + e + j) < drop_p ? 0.f : o[j] * keep_inv;
    }
    st4f(y + (size_t)img * L + e, make_float4(o[0], o[1], o[2], o[3]));
  }
}

// backward pass 1: per-image sums of g and g*xhat (g = dy*mask*w) -> sums[I][2] (atomics)
template <typename AT>
__global__ __launch_bounds__(256) void lnl_bwd_reduce_kernel(const AT* __restrict__ dy, const AT* __restrict__ x,
                                                             const float* __restrict__ w, const float* __restrict__ meanrstd,
                                                             double* __restrict__ sums, int L, float drop_p, uint32_t seed, const uint32_t* __restrict__ epoch) {
  seed = eff_seed(seed, epoch);
  __shared__ float sc[4];
  const int img = blockIdx.y;
  const float mean = meanrstd[img * 2], rstd = meanrstd[img * 2 + 1];
  const float keep_inv = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
  float s1 = 0.f, s2 = 0.f;
  for (int e = (blockIdx.x * 256 + threadIdx.x) * 4; e < L; e += gridDim.x * 1024) {
    const float4 dv = ld4f(dy + (size_t)img * L + e);
    const float4 xv = ld4f(x + (size_t)img * L + e);
    const float4 wv = *reinterpret_cast<const float4*>(w + e);
    const float d[4] = {dv.x, dv.y, dv.z, dv.w}, xx[4] = {xv.x, xv.y, xv.z, xv.w}, ww[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float dd = d[j];
      if (drop_p > 0.f) dd = uniform01(seed, (uint64_t)img * L + e + j) < drop_p ? 0.f : dd * keep_inv;
      const float g = dd * ww[j];
      s1 += g; s2 += g * (xx[j] - mean) * rstd;
    }
  }
  s1 = block_sum<4>(s1, sc);
  s2 = block_sum<4>(s2, sc);
  if (threadIdx.x == 0) { atomicAdd(sums + img * 2, (double)s1); atomicAdd(sums + img * 2 + 1, (double)s2); }
}

// backward pass 2: dx per element; dw/db accumulated over the images by the thread that owns elements e..e+3 (L % 4 == 0).
// The images are split over gridDim.y (each slice ends in one float atomic per element): with a single slice the launch is
// L / 1024 = 294 workgroups at most, each thread walking all I images serially - 1.4 TB/s on the stage-0 head.
template <typename AT>
__global__ __launch_bounds__(256) void lnl_bwd_apply_kernel(const AT* __restrict__ dy, const AT* __restrict__ x,
                                                            const float* __restrict__ w, const float* __restrict__ meanrstd,
                                                            const double* __restrict__ sums, AT* __restrict__ dx,
                                                            float* __restrict__ dw, float* __restrict__ db, int L, int I,
                                                            float drop_p, uint32_t seed, const uint32_t* __restrict__ epoch) {
  seed = eff_seed(seed, epoch);
  const int e = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (e >= L) return;
  const float keep_inv = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
  const float4 wq = *reinterpret_cast<const float4*>(w + e);
  const float wv[4] = {wq.x, wq.y, wq.z, wq.w};
  float aw[4] = {0.f, 0.f, 0.f, 0.f}, ab[4] = {0.f, 0.f, 0.f, 0.f};
  const int per = (I + gridDim.y - 1) / gridDim.y, i0 = blockIdx.y * per;
  const int i1 = i0 + per < I ? i0 + per : I;
  for (int img = i0; img < i1; ++img) {
    const float mean = meanrstd[img * 2], rstd = meanrstd[img * 2 + 1];
    const double m1 = sums[img * 2] / L, m2 = sums[img * 2 + 1] / L;
    const float4 dq = ld4f(dy + (size_t)img * L + e), xq = ld4f(x + (size_t)img * L + e);
    float dd[4] = {dq.x, dq.y, dq.z, dq.w};
    const float xx[4] = {xq.x, xq.y, xq.z, xq.w};
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (drop_p > 0.f) dd[j] = uniform01(seed, (uint64_t)img * L + e + j) < drop_p ? 0.f : dd[j] * keep_inv;
      const float xh = (xx[j] - mean) * rstd;
      const float g = dd[j] * wv[j];
      o[j] = (float)((double)rstd * ((double)g - m1 - (double)xh * m2));
      aw[j] += dd[j] * xh; ab[j] += dd[j];
    }
    st4f(dx + (size_t)img * L + e, make_float4(o[0], o[1], o[2], o[3]));
  }
  if (gridDim.y == 1) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { dw[e + j] += aw[j]; db[e + j] += ab[j]; }
  } else if (i0 < i1) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { atomicAdd(dw + e + j, aw[j]); atomicAdd(db + e + j, ab[j]); }
  }
}

// ------------------------------------------------------------------------------------------------
// BatchNorm on channels-last [M, C] (row stride ld)
// ------------------------------------------------------------------------------------------------
// per-channel sum and sum of squares (when the producing contraction did not accumulate them itself)
template <typename AT>
__global__ __launch_bounds__(256) void bn_stats_kernel(const AT* __restrict__ x, long long M, int C, int ld,
                                                       double* __restrict__ sums, long long rows_per_block) {
  __shared__ double r1[4][64], r2[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.y * rows_per_block;
  long long r1e = r0 + rows_per_block; if (r1e > M) r1e = M;
  double s1 = 0.0, s2 = 0.0;
  if (c < C) for (long long r = r0 + rl; r < r1e; r += 4) { const double v = ldf(x + (size_t)r * ld + c); s1 += v; s2 += v * v; }
  r1[rl][threadIdx.x & 63] = s1; r2[rl][threadIdx.x & 63] = s2;
  __syncthreads();
  if (rl == 0 && c < C) {
    atomicAdd(sums + c, r1[0][threadIdx.x] + r1[1][threadIdx.x] + r1[2][threadIdx.x] + r1[3][threadIdx.x]);
    atomicAdd(sums + C + c, r2[0][threadIdx.x] + r2[1][threadIdx.x] + r2[2][threadIdx.x] + r2[3][threadIdx.x]);
  }
}

// train: batch mean / biased var -> scale, shift, saved mean/rstd, running-stat update (unbiased var).
// eval : scale/shift from the running statistics.
__global__ void bn_finalize_kernel(const double* __restrict__ sums, double count, const float* __restrict__ gamma,
                                   const float* __restrict__ beta, float* __restrict__ running_mean,
                                   float* __restrict__ running_var, float momentum, float eps, int training,
                                   float* __restrict__ scale, float* __restrict__ shift, float* __restrict__ save_mean,
                                   float* __restrict__ save_rstd, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float mean, var;
  if (training) {   // statistics in double: E[x^2]-mean^2 cancels badly in fp32 (torch's CPU path accumulates in double too)
    double t1 = 0.0, t2 = 0.0;
    for (int sl = 0; sl < SV_BN_SLOTS; ++sl) { t1 += sums[(size_t)sl * 2 * C + c]; t2 += sums[(size_t)sl * 2 * C + C + c]; }
    const double m = t1 / count;
    double v = t2 / count - m * m;
    if (v < 0.0) v = 0.0;
    mean = (float)m; var = (float)v;
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)(v * (count > 1.0 ? count / (count - 1.0) : 1.0));
  } else {
    mean = running_mean[c]; var = running_var[c];
  }
  const float rstd = rsqrtf(var + eps);
  const float sc = gamma[c] * rstd;
  scale[c] = sc; shift[c] = beta[c] - mean * sc;
  save_mean[c] = mean; save_rstd[c] = rstd;
}

// y = act(x*scale[c] + shift[c] (+ residual)): scalar fallback (any C / strides); the vector paths are the *_cg and *_narrow kernels below
template <typename AT>
__global__ __launch_bounds__(256) void scale_shift_act_scalar_kernel(const AT* __restrict__ x, int ldx, const float* __restrict__ scale,
                                                                     const float* __restrict__ shift, const AT* __restrict__ res,
                                                                     int ldr, AT* __restrict__ y, int ldy, long long M, int C,
                                                                     int act, float slope) {
  const long long total = M * C;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long r = i / C; const int c = (int)(i - r * C);
    float o = __fmaf_rn(ldf(x + (size_t)r * ldx + c), scale[c], shift[c]);
    if (res) o += ldf(res + (size_t)r * ldr + c);
    stf(y + (size_t)r * ldy + c, apply_act(o, act, slope));
  }
}

// ------------------------------------------------------------------------------------------------
// Pieces every BatchNorm backward path below shares.  The paths differ in thread mapping (scalar, narrow, vector, the bn3 + down-sampling
// pair, the pool fusions) for measured reasons; the sign-word layout, the mask rule, the apply coefficients and the slot scheme are
// written here once, and a new path uses them.
// ------------------------------------------------------------------------------------------------
// Sign words (optional output of the vector forward passes; G == 64 and C % 256 == 0, so that a wave is the 64 column groups of ONE row):
// bit `lane` of word signs[(row * (C / 256) + blockIdx.x) * 4 + j] = (value of channel 256 blockIdx.x + 4 lane + j before the activation) > 0 -
// the activation mask the backward needs, 1/16 of the bytes of the output it would otherwise re-read.
template <typename W> __device__ __forceinline__ W* bn_sign_words(W* signs, long long row, int C) {
  return signs + ((size_t)row * (C >> 8) + blockIdx.x) * 4;
}
__device__ __forceinline__ void bn_signs_store(unsigned long long* signs, long long row, int C, int gq, const float (&o)[4]) {
  const unsigned long long b0 = __builtin_amdgcn_ballot_w64(o[0] > 0.f), b1 = __builtin_amdgcn_ballot_w64(o[1] > 0.f);
  const unsigned long long b2 = __builtin_amdgcn_ballot_w64(o[2] > 0.f), b3 = __builtin_amdgcn_ballot_w64(o[3] > 0.f);
  if (gq == 0) {
    ulonglong2* w = reinterpret_cast<ulonglong2*>(bn_sign_words(signs, row, C));
    w[0] = make_ulonglong2(b0, b1);
    w[1] = make_ulonglong2(b2, b3);
  }
}
__device__ __forceinline__ void bn_signs_load(const unsigned long long* signs, long long row, int C, unsigned long long (&m)[4]) {
  const ulonglong2* w = reinterpret_cast<const ulonglong2*>(bn_sign_words(signs, row, C));   // the same four words for the whole wave
  const ulonglong2 p0 = w[0], p1 = w[1];
  m[0] = p0.x; m[1] = p0.y; m[2] = p1.x; m[3] = p1.y;
}

// The masked gradient dz' = dz * act'(mask) of N adjacent channels of one row.  The mask comes from the stored output z, from the row's
// sign words (lane gq owns bit gq) or, with neither saved, from the pre-activation recomputed as fma(x, msc, msh) with the forward's
// scale / shift.  bn_mask_load fetches what the source needs (so that a pass can issue it with its other loads), bn_mask_grad applies it.
enum BnMaskSrc { BN_MASK_Z, BN_MASK_X, BN_MASK_SIGNS };
__device__ __forceinline__ BnMaskSrc bn_mask_src(const void* z, const void* signs) { return signs ? BN_MASK_SIGNS : z ? BN_MASK_Z : BN_MASK_X; }
template <int N> struct BnMaskRule {
  int act; float neg; BnMaskSrc src; int gq;
  float msc[N], msh[N];     // BN_MASK_X only (fsc / fsh may be NULL when there is no activation)
};
template <int N> struct BnMask { float z[N]; unsigned long long m[4]; };     // what bn_mask_load fetched for one row

template <int N>
__device__ __forceinline__ void bn_mask_rule(BnMaskRule<N>& m, int act, float slope, BnMaskSrc src, int gq, const float* __restrict__ fsc,
                                             const float* __restrict__ fsh, int c, int nreal = N) {     // nreal < N: padding channels (narrow rows)
  m.act = act; m.neg = act == SV_ACT_LRELU ? slope : 0.f; m.src = src; m.gq = gq;
  if (src == BN_MASK_X && act != SV_ACT_NONE) {      // one branch around all 2 N loads
#pragma unroll
    for (int j = 0; j < N; ++j) { m.msc[j] = j < nreal ? fsc[c + j] : 0.f; m.msh[j] = j < nreal ? fsh[c + j] : 0.f; }
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) { m.msc[j] = 0.f; m.msh[j] = 0.f; }
  }
}
// the rule of channel j alone, for a pass that masks inside its loop over the channels
template <int N> __device__ __forceinline__ BnMaskRule<1> bn_mask_rule_of(const BnMaskRule<N>& m, int j) {
  return BnMaskRule<1>{m.act, m.neg, m.src, m.gq, {m.msc[j]}, {m.msh[j]}};
}
template <int N, typename AT>
__device__ __forceinline__ void bn_mask_load(const BnMaskRule<N>& m, BnMask<N>& k, const AT* __restrict__ z, size_t off,
                                             const unsigned long long* __restrict__ signs, long long row, int C) {
  if (m.act == SV_ACT_NONE) return;
  if (m.src == BN_MASK_Z) { if constexpr (N == 1) k.z[0] = ldf(z + off); else ldnf<N>(z + off, k.z); }
  else if (m.src == BN_MASK_SIGNS) bn_signs_load(signs, row, C, k.m);
}
template <int N>
__device__ __forceinline__ void bn_mask_grad(const BnMaskRule<N>& m, const BnMask<N>& k, float* d, const float* x) {
  if (m.act == SV_ACT_NONE) return;
  if (m.src == BN_MASK_SIGNS) {
#pragma unroll
    for (int j = 0; j < N; ++j) d[j] *= ((k.m[j & 3] >> m.gq) & 1ull) ? 1.f : m.neg;
    return;
  }
  float zz[N];
  if (m.src == BN_MASK_Z) {
#pragma unroll
    for (int j = 0; j < N; ++j) zz[j] = k.z[j];
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) zz[j] = __fmaf_rn(x[j], m.msc[j], m.msh[j]);
  }
#pragma unroll
  for (int j = 0; j < N; ++j) d[j] *= zz[j] > 0.f ? 1.f : m.neg;
}
template <int N> __device__ __forceinline__ void bn_mask_grad(const BnMaskRule<N>& m, float* d, const float* x) {   // BN_MASK_X: nothing was fetched
  BnMask<N> none;
  bn_mask_grad(m, none, d, x);
}
// both steps for a pass with one row in flight (one guard around the fetch and its use: what was fetched does not stay live across a branch)
template <int N, typename AT>
__device__ __forceinline__ void bn_mask_row(const BnMaskRule<N>& m, const AT* __restrict__ z, size_t off, const unsigned long long* __restrict__ signs,
                                            long long row, int C, float* d, const float* x) {
  if (m.act == SV_ACT_NONE) return;
  BnMask<N> k;
  bn_mask_load(m, k, z, off, signs, row, C);
  bn_mask_grad(m, k, d, x);
}

// Apply pass: dx = k1*d - k2 - k3*x with per-channel constants from the folded sums (the image behind the slots), k1 = gamma rstd,
// k3 = k1 rstd sum(dz' xhat)/M, k2 = k1 sum(dz')/M - k3 mean; eval: k2 = k3 = 0.  Double: the mean-removal terms must cancel to
// rounding, otherwise the residual of sum_r dx is amplified by every later reduction over positions (torch's CPU kernel evaluates this
// in double too).
__device__ __forceinline__ const double* bn_bwd_folded(const double* sums, int C) { return sums + (size_t)BN_BWD_SLOTS * 2 * C; }   // written by bn_bwd_fold_kernel
__device__ __forceinline__ void bn_bwd_coef(const float* __restrict__ gamma, const float* __restrict__ mean, const float* __restrict__ rstd,
                                            const double* __restrict__ fin, double invM, int training, int c, int C, double& k1, double& k2,
                                            double& k3) {
  const double gm = gamma[c], rs = rstd[c], mu = mean[c];
  k1 = gm * rs;
  if (training) { const double a = fin[c] * invM, b = fin[C + c] * invM; k3 = gm * rs * b * rs; k2 = gm * rs * a - k3 * mu; }
  else { k2 = 0.0; k3 = 0.0; }
}
__device__ __forceinline__ float bn_bwd_dx(double k1, double k2, double k3, float d, float x) { return (float)(k1 * (double)d - k2 - k3 * (double)x); }

// Reduce pass, vector geometries (G column groups of CV channels x RL = 256 / G row lanes, channel block cb): park the NS * CV per-thread
// double partials (sum s of channel j at [s * CV + j]) in LDS, fold them over the row lanes (thread t folds partial t % NP of column group
// t / NP, l ascending) and hand each total to add(s, index, total), index = the channel's place in slot image `block % BN_BWD_SLOTS`;
// add issues the atomicAdd(s) - which image(s) sum s belongs to is the caller's rule.
template <int CV, int NS, typename Add>
__device__ __forceinline__ void bn_slot_fold(double (*red)[NS * CV + 1], const double (&part)[NS * CV], int G, int RL, int cb, unsigned block, int C,
                                             Add add) {
  constexpr int NP = NS * CV;
#pragma unroll
  for (int j = 0; j < NP; ++j) red[threadIdx.x][j] = part[j];
  __syncthreads();
  for (int t = threadIdx.x; t < NP * G; t += 256) {
    const int q = t / NP, k = t % NP;
    const int cc = (cb * G + q) * CV + k % CV;
    if (cc < C) {
      double a = 0.0;
      for (int l = 0; l < RL; ++l) a += red[l * G + q][k];
      add(k / CV, (size_t)(block % BN_BWD_SLOTS) * 2 * C + cc, a);
    }
  }
}
template <int CV>     // one layer: [sum dz' | sum dz' xhat] into its own image
__device__ __forceinline__ void bn_slot_fold_one(double (*red)[2 * CV + 1], const double (&part)[2 * CV], int G, int RL, int cb, unsigned block, int C, double* __restrict__ sums) {
  bn_slot_fold<CV, 2>(red, part, G, RL, cb, block, C, [&](int s, size_t i, double a) { atomicAdd(sums + i + (size_t)s * C, a); });
}

// fold the BatchNorm backward slots: fin[c] = sum_slot ws[slot][c] (c < 2C), dgamma += fin[C + c], dbeta += fin[c]; blockIdx.y = image
// (gridDim.y = 2 for the two layers of the bn3 + down-sampling pass, 1 otherwise)
__global__ __launch_bounds__(256) void bn_bwd_fold_kernel(double* __restrict__ ws0, double* __restrict__ ws1, int C, float* __restrict__ dgamma0,
                                                          float* __restrict__ dbeta0, float* __restrict__ dgamma1, float* __restrict__ dbeta1) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= 2 * C) return;
  double* ws = blockIdx.y ? ws1 : ws0;
  float* dgamma = blockIdx.y ? dgamma1 : dgamma0;
  float* dbeta = blockIdx.y ? dbeta1 : dbeta0;
  double a = 0.0;
#pragma unroll
  for (int sl = 0; sl < BN_BWD_SLOTS; ++sl) a += ws[(size_t)sl * 2 * C + c];
  ws[(size_t)BN_BWD_SLOTS * 2 * C + c] = a;
  if (c < C) dbeta[c] += (float)a; else dgamma[c - C] += (float)a;
}

// backward pass 1: per channel s1 = sum(dz'), s2 = sum(dz' * xhat), dz' = dz * act'(z) (mask from the OUTPUT z)
template <typename AT>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const AT* __restrict__ dz, int lddz, const AT* __restrict__ z, int ldz,
                                                            const AT* __restrict__ x, int ldx, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, long long M, int C, int act, float slope,
                                                            double* __restrict__ sums, long long rows_per_block, int CW,
                                                            const float* __restrict__ fsc, const float* __restrict__ fsh) {
  // CW (a power of two <= 64) lanes across the channels, 256 / CW row lanes: with one or two channels every thread still works
  __shared__ double r1[256], r2[256];
  const int cl = threadIdx.x & (CW - 1), c = blockIdx.x * CW + cl, rl = threadIdx.x / CW, RL = 256 / CW;
  const long long r0 = (long long)blockIdx.y * rows_per_block;
  long long r1e = r0 + rows_per_block; if (r1e > M) r1e = M;
  double s1 = 0.0, s2 = 0.0;
  if (c < C) {
    const float mu = mean[c], rs = rstd[c];
    BnMaskRule<1> mk;
    bn_mask_rule(mk, act, slope, bn_mask_src(z, nullptr), 0, fsc, fsh, c);
    long long r = r0 + rl;
    for (; r + 3 * RL < r1e; r += 4 * RL) {   // 4 rows in flight per thread (independent loads), then the serial tail
      float d[4], xv[4];
      BnMask<1> zv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        d[u] = ldf(dz + (size_t)(r + RL * u) * lddz + c);
        xv[u] = ldf(x + (size_t)(r + RL * u) * ldx + c);
        bn_mask_load(mk, zv[u], z, (size_t)(r + RL * u) * ldz + c, nullptr, 0, C);
      }
      float f1 = 0.f, f2 = 0.f;               // four rows in fp32, then into the double accumulators
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        bn_mask_grad(mk, zv[u], &d[u], &xv[u]);
        f1 += d[u]; f2 += d[u] * (xv[u] - mu) * rs;
      }
      s1 += (double)f1; s2 += (double)f2;
    }
    for (; r < r1e; r += RL) {
      float d = ldf(dz + (size_t)r * lddz + c);
      const float xq = ldf(x + (size_t)r * ldx + c);
      bn_mask_row(mk, z, (size_t)r * ldz + c, nullptr, 0, C, &d, &xq);
      s1 += (double)d; s2 += (double)(d * (xq - mu) * rs);
    }
  }
  r1[threadIdx.x] = s1; r2[threadIdx.x] = s2;
  __syncthreads();
  if (rl == 0 && c < C) {
    double a = 0.0, b = 0.0;
    for (int l = 0; l < RL; ++l) { a += r1[l * CW + cl]; b += r2[l * CW + cl]; }
    double* slot = sums + (size_t)(blockIdx.y % BN_BWD_SLOTS) * 2 * C;
    atomicAdd(slot + c, a);
    atomicAdd(slot + C + c, b);
  }
}

// backward pass 2: dx = gamma*rstd*(dz' - s1/M - xhat*s2/M) (train) or dz'*gamma*rstd (eval); dres = dz' (optional).  Evaluated per element
// in this association, not as bn_bwd_dx's k1*d - k2 - k3*x: this family carries the largest measured error and keeps its own expression.
template <typename AT>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const AT* __restrict__ dz, int lddz, const AT* __restrict__ z, int ldz,
                                                           const AT* __restrict__ x, int ldx, const float* __restrict__ gamma,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const double* __restrict__ sums, long long M, int C, int act, float slope,
                                                           int training, AT* __restrict__ dx, int lddx, AT* __restrict__ dres,
                                                           int lddres, const float* __restrict__ fsc, const float* __restrict__ fsh) {
  const long long total = M * C;
  const double invM = 1.0 / (double)M;
  sums = bn_bwd_folded(sums, C);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long r = i / C; const int c = (int)(i - r * C);
    float d = ldf(dz + (size_t)r * lddz + c);
    const float xq = ldf(x + (size_t)r * ldx + c);
    BnMaskRule<1> mk;
    bn_mask_rule(mk, act, slope, bn_mask_src(z, nullptr), 0, fsc, fsh, c);
    bn_mask_row(mk, z, (size_t)r * ldz + c, nullptr, 0, C, &d, &xq);
    if (dres) stf(dres + (size_t)r * lddres + c, d);
    const float rs = rstd[c];
    float o;
    if (training) {
      // double arithmetic for the mean-subtraction terms (see bn_bwd_coef)
      const double xh = ((double)xq - (double)mean[c]) * (double)rs;
      o = (float)((double)gamma[c] * (double)rs * ((double)d - sums[c] * invM - xh * (sums[C + c] * invM)));
    } else {
      o = d * gamma[c] * rs;
    }
    stf(dx + (size_t)r * lddx + c, o);
  }
}

// ------------------------------------------------------------------------------------------------
// narrow BatchNorm (C <= 16, every row stride a multiple of 4: the 9/12-channel merger tail): a thread owns ONE 4-channel
// group of a row (g = tid & 3, 64 rows per workgroup pass), so a wave instruction moves 8/16-byte vectors that tile whole
// rows (21 rows x 24 B with 9 channels) instead of one 2-byte element per lane in the generic scalar kernels, and the
// per-channel constants of the group sit in registers.
// ------------------------------------------------------------------------------------------------
constexpr int BN_NARROW_MAXC = 16;

template <typename AT>
__global__ __launch_bounds__(256) void scale_shift_act_narrow_kernel(const AT* __restrict__ x, int ldx, const float* __restrict__ scale,
                                                                     const float* __restrict__ shift, const AT* __restrict__ res, int ldr,
                                                                     AT* __restrict__ y, int ldy, long long M, int C, int act, float slope) {
  const int g = threadIdx.x & 3, rl = threadIdx.x >> 2;
  if (4 * g >= C) return;
  float sc[4], sh[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { const int c = 4 * g + j; sc[j] = c < C ? scale[c] : 0.f; sh[j] = c < C ? shift[c] : 0.f; }
  for (long long r = (long long)blockIdx.x * 64 + rl; r < M; r += (long long)gridDim.x * 64) {
    const float4 xv = ld4f(x + (size_t)r * ldx + 4 * g);
    float o[4] = {xv.x, xv.y, xv.z, xv.w};
    float rr[4] = {0.f, 0.f, 0.f, 0.f};
    if (res) { const float4 rv = ld4f(res + (size_t)r * ldr + 4 * g); rr[0] = rv.x; rr[1] = rv.y; rr[2] = rv.z; rr[3] = rv.w; }
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (4 * g + j < C) ? apply_act(__fmaf_rn(o[j], sc[j], sh[j]) + rr[j], act, slope) : 0.f;
    st4f(y + (size_t)r * ldy + 4 * g, make_float4(o[0], o[1], o[2], o[3]));
  }
}

// pass 1: per-thread fp32 partials over <= rows_per_thread rows, workgroup fold in double, one atomic per channel per workgroup
template <typename AT>
__global__ __launch_bounds__(256) void bn_bwd_reduce_narrow_kernel(const AT* __restrict__ dz, int lddz, const AT* __restrict__ z, int ldz,
                                                                   const AT* __restrict__ x, int ldx, const float* __restrict__ mean,
                                                                   const float* __restrict__ rstd, long long M, int C, int act, float slope,
                                                                   double* __restrict__ sums, int rows_per_thread,
                                                                   const float* __restrict__ fsc, const float* __restrict__ fsh) {
  __shared__ double red[64][9];     // [row lane][4 x s1, 4 x s2] (+1 pad) per group, folded group by group
  const int g = threadIdx.x & 3, rl = threadIdx.x >> 2;
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f}, mu[4], rs[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { const int c = 4 * g + j; mu[j] = c < C ? mean[c] : 0.f; rs[j] = c < C ? rstd[c] : 0.f; }
  BnMaskRule<4> mk;
  bn_mask_rule(mk, act, slope, bn_mask_src(z, nullptr), 0, fsc, fsh, 4 * g, C - 4 * g);
  if (4 * g < C) {
    const long long r0 = (long long)blockIdx.x * 64 * rows_per_thread + rl;
    for (int k = 0; k < rows_per_thread; ++k) {
      const long long r = r0 + (long long)k * 64;
      if (r >= M) break;
      float d[4], xx[4];
      ldnf<4>(dz + (size_t)r * lddz + 4 * g, d); ldnf<4>(x + (size_t)r * ldx + 4 * g, xx);
      bn_mask_row(mk, z, (size_t)r * ldz + 4 * g, nullptr, 0, C, d, xx);
#pragma unroll
      for (int j = 0; j < 4; ++j) { s1[j] += d[j]; s2[j] += d[j] * (xx[j] - mu[j]) * rs[j]; }
    }
  }
  for (int gg = 0; gg < 4; ++gg) {           // fold the 64 row lanes of one channel group at a time
    __syncthreads();
    if (g == gg) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { red[rl][j] = (double)s1[j]; red[rl][4 + j] = (double)s2[j]; }
    }
    __syncthreads();
    if (threadIdx.x < 8) {
      const int c = 4 * gg + (threadIdx.x & 3);
      if (c < C) {
        double a = 0.0;
        for (int l = 0; l < 64; ++l) a += red[l][threadIdx.x];
        atomicAdd(sums + (size_t)(blockIdx.x % BN_BWD_SLOTS) * 2 * C + (threadIdx.x >> 2) * C + c, a);
      }
    }
  }
}

template <typename AT>
__global__ __launch_bounds__(256) void bn_bwd_apply_narrow_kernel(const AT* __restrict__ dz, int lddz, const AT* __restrict__ z, int ldz,
                                                                  const AT* __restrict__ x, int ldx, const float* __restrict__ gamma,
                                                                  const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                  const double* __restrict__ sums, long long M, int C, int act, float slope,
                                                                  int training, AT* __restrict__ dx, int lddx, AT* __restrict__ dres, int lddres,
                                                                  const float* __restrict__ fsc, const float* __restrict__ fsh) {
  const int g = threadIdx.x & 3, rl = threadIdx.x >> 2;
  if (4 * g >= C) return;
  BnMaskRule<4> mk;
  bn_mask_rule(mk, act, slope, bn_mask_src(z, nullptr), 0, fsc, fsh, 4 * g, C - 4 * g);
  double k1[4], k2[4], k3[4];
  const double invM = 1.0 / (double)M;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (4 * g + j < C) bn_bwd_coef(gamma, mean, rstd, bn_bwd_folded(sums, C), invM, training, 4 * g + j, C, k1[j], k2[j], k3[j]);
    else k1[j] = k2[j] = k3[j] = 0.0;
  }
  for (long long r = (long long)blockIdx.x * 64 + rl; r < M; r += (long long)gridDim.x * 64) {
    float d[4], xx[4], o[4];
    ldnf<4>(dz + (size_t)r * lddz + 4 * g, d); ldnf<4>(x + (size_t)r * ldx + 4 * g, xx);
    bn_mask_row(mk, z, (size_t)r * ldz + 4 * g, nullptr, 0, C, d, xx);
#pragma unroll
    for (int j = 0; j < 4; ++j) {   // padding columns: whatever was read (possibly uninitialised memory) is ignored, zero is written
      const bool real = 4 * g + j < C;
      o[j] = real ? bn_bwd_dx(k1[j], k2[j], k3[j], d[j], xx[j]) : 0.f;
      if (!real) d[j] = 0.f;
    }
    if (dres) stnf<4>(dres + (size_t)r * lddres + 4 * g, d);
    stnf<4>(dx + (size_t)r * lddx + 4 * g, o);
  }
}

// vector paths of BatchNorm apply / backward apply (C and every row stride multiples of 4): a thread keeps ONE 4-channel group
// (gq = tid % G) and walks rows (rl = tid / G, step RL = 256 / G), so the per-channel constants live in registers and the loop
// has no 64-bit division (a flat element loop spends as many issue slots on index math and constant reloads as on the data).
template <typename AT>
__global__ __launch_bounds__(256) void scale_shift_act_cg_kernel(const AT* __restrict__ x, int ldx, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift, const AT* __restrict__ res, int ldr,
                                                                 AT* __restrict__ y, int ldy, long long M, int C, int act, float slope,
                                                                 long long rows_per_block, int G, unsigned long long* __restrict__ signs) {
  // signs (optional; G == 64 and C % 256 == 0): the activation mask for the backward, see bn_signs_store
  const int gq = threadIdx.x % G, rl = threadIdx.x / G, RL = 256 / G;
  const int c = (blockIdx.x * G + gq) * 4;
  if (c >= C || rl >= RL) return;
  const float4 sc = *reinterpret_cast<const float4*>(scale + c), sh = *reinterpret_cast<const float4*>(shift + c);
  const long long r0 = (long long)blockIdx.y * rows_per_block;
  long long r1 = r0 + rows_per_block; if (r1 > M) r1 = M;
#pragma unroll 2
  for (long long r = r0 + rl; r < r1; r += RL) {
    const float4 xv = ld4f(x + (size_t)r * ldx + c);
    float o[4] = {__fmaf_rn(xv.x, sc.x, sh.x), __fmaf_rn(xv.y, sc.y, sh.y), __fmaf_rn(xv.z, sc.z, sh.z), __fmaf_rn(xv.w, sc.w, sh.w)};
    if (res) {
      const float4 rv = ld4f(res + (size_t)r * ldr + c);
      o[0] += rv.x; o[1] += rv.y; o[2] += rv.z; o[3] += rv.w;
    }
    if (signs) bn_signs_store(signs, r, C, gq, o);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = apply_act(o[j], act, slope);
    st4f(y + (size_t)r * ldy + c, make_float4(o[0], o[1], o[2], o[3]));
  }
}

// SIGNS: the mask comes from the forward's sign words (G == 64, C % 256 == 0: lane gq owns bit gq of the row's four words)
template <typename AT, bool SIGNS = false>
__global__ __launch_bounds__(256) void bn_bwd_apply_cg_kernel(const AT* __restrict__ dz, int lddz, const AT* __restrict__ z, int ldz,
                                                              const AT* __restrict__ x, int ldx, const float* __restrict__ gamma,
                                                              const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              const double* __restrict__ sums, long long M, int C, int act, float slope,
                                                              int training, AT* __restrict__ dx, int lddx, AT* __restrict__ dres, int lddres,
                                                              const float* __restrict__ fsc, const float* __restrict__ fsh,
                                                              long long rows_per_block, int G,
                                                              const unsigned long long* __restrict__ signs = nullptr) {
  const int gq = threadIdx.x % G, rl = threadIdx.x / G, RL = 256 / G;
  const int c = (blockIdx.x * G + gq) * 4;
  if (c >= C || rl >= RL) return;
  BnMaskRule<4> mk;
  bn_mask_rule(mk, act, slope, SIGNS ? BN_MASK_SIGNS : bn_mask_src(z, nullptr), gq, fsc, fsh, c);
  double k1[4], k2[4], k3[4];
  const double invM = 1.0 / (double)M;
#pragma unroll
  for (int j = 0; j < 4; ++j) bn_bwd_coef(gamma, mean, rstd, bn_bwd_folded(sums, C), invM, training, c + j, C, k1[j], k2[j], k3[j]);
  const long long r0 = (long long)blockIdx.y * rows_per_block;
  long long r1 = r0 + rows_per_block; if (r1 > M) r1 = M;
#pragma unroll 2
  for (long long r = r0 + rl; r < r1; r += RL) {
    float d[4], xx[4], o[4];
    ldnf<4>(dz + (size_t)r * lddz + c, d); ldnf<4>(x + (size_t)r * ldx + c, xx);
    bn_mask_row(mk, z, (size_t)r * ldz + c, signs, r, C, d, xx);
    if (dres) stnf<4>(dres + (size_t)r * lddres + c, d);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = bn_bwd_dx(k1[j], k2[j], k3[j], d[j], xx[j]);
    stnf<4>(dx + (size_t)r * lddx + c, o);
  }
}

// vector variant of pass 1 (C and the row strides multiples of 4): a thread owns 4 adjacent channels of a strided row
// subset; G = min(C/4, 64) column groups x 256/G row lanes per workgroup, row lanes folded through LDS
template <typename AT>
__global__ __launch_bounds__(256) void bn_bwd_reduce_vec_kernel(const AT* __restrict__ dz, int lddz, const AT* __restrict__ z, int ldz,
                                                                const AT* __restrict__ x, int ldx, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, long long M, int C, int act, float slope,
                                                                double* __restrict__ sums, long long rows_per_block, int G,
                                                                const float* __restrict__ fsc, const float* __restrict__ fsh,
                                                                AT* __restrict__ dmask, int lddm, const unsigned long long* __restrict__ signs) {
  // signs (optional, instead of z; G == 64, C % 256 == 0): the forward's activation mask, one bit per element (bn_signs_store)
  // dmask (optional): receives dz' = dz * act'(z) - the gradient of the residual branch AND what pass 2 then reads instead of (dz, z):
  // a BatchNorm in front of a residual sum (bn3 / the down-sampling branch of every bottleneck) saves one read of the widest tensors
  __shared__ double red[256][9];   // [thread][8 partials] (+1 pad)
  const int gq = threadIdx.x % G, rl = threadIdx.x / G, RL = 256 / G;
  const int c = (blockIdx.x * G + gq) * 4;
  const long long r0 = (long long)blockIdx.y * rows_per_block;
  long long r1e = r0 + rows_per_block; if (r1e > M) r1e = M;
  double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // [sum dz' | sum dz' xhat] x 4 channels
  if (c < C && rl < RL) {
    float mm[4], rr[4];
    ldnf<4>(mean + c, mm); ldnf<4>(rstd + c, rr);
    BnMaskRule<4> mk;
    bn_mask_rule(mk, act, slope, bn_mask_src(z, signs), gq, fsc, fsh, c);
    // a row in two steps, so that the loop can issue the loads of both its rows before the arithmetic of either; dz and x of every row
    // go out before the branch on the mask source
    struct Row { float d[4], x[4]; BnMask<4> k; };
    auto load = [&](long long r, Row* w, int n) __attribute__((always_inline)) {     // n rows, RL apart
#pragma unroll
      for (int i = 0; i < n; ++i) ldnf<4>(dz + (size_t)(r + i * RL) * lddz + c, w[i].d);
#pragma unroll
      for (int i = 0; i < n; ++i) ldnf<4>(x + (size_t)(r + i * RL) * ldx + c, w[i].x);
#pragma unroll
      for (int i = 0; i < n; ++i) bn_mask_load(mk, w[i].k, z, (size_t)(r + i * RL) * ldz + c, signs, r + i * RL, C);
    };
    auto terms = [&](long long r, Row& w, float (&t)[8]) __attribute__((always_inline)) {
      bn_mask_grad(mk, w.k, w.d, w.x);
      if (dmask) stnf<4>(dmask + (size_t)r * lddm + c, w.d);
#pragma unroll
      for (int j = 0; j < 4; ++j) { t[j] = w.d[j]; t[4 + j] = w.d[j] * (w.x[j] - mm[j]) * rr[j]; }
    };
    Row w[2];
    float t0[8], t1[8];
    long long r = r0 + rl;
    for (; r + RL < r1e; r += 2 * RL) {   // two rows in flight
      load(r, w, 2);
      terms(r, w[0], t0); terms(r + RL, w[1], t1);
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] += (double)t0[j] + (double)t1[j];
    }
    for (; r < r1e; r += RL) {
      load(r, w, 1);
      terms(r, w[0], t0);
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] += (double)t0[j];
    }
  }
  bn_slot_fold_one<4>(red, s, G, RL, blockIdx.x, blockIdx.y, C, sums);
}

// ------------------------------------------------------------------------------------------------
// The first bottleneck of a ResNet layer: out = relu(bn3(y3) + bn_d(yd)), two BatchNorms on tensors of one shape [M, C] whose outputs are
// only ever summed.  One pass each way handles BOTH layers (C % 256 == 0, G == 64: a wave is the 64 column groups of one row, as in the
// sign-word passes above): the normalised down-sampling branch is never stored, nor is the masked gradient dout * [out > 0] that both
// backwards consume - each pass forms it again from dout and the sign words.
//   forward: t = fma(yd, scale_d, shift_d) rounded to the storage type (what the separate pass stored), o = fma(y3, scale_3, shift_3) + t,
//            sign bit = o > 0, out = relu(o) - the bytes of sv_scale_shift_act (down-sampling layer) + sv_scale_shift_act_signs (bn3)
//   reduce : d = dout * bit; sum d (shared by both layers), sum d xhat_3, sum d xhat_d into the two [slot][2C] images
//   apply  : dy3 = k1 d - k2 - k3 y3 and dyd likewise with each layer's constants (double, see bn_bwd_apply_cg_kernel)
// ------------------------------------------------------------------------------------------------
template <typename AT>
__global__ __launch_bounds__(256) void scale_shift_act2_cg_kernel(const AT* __restrict__ x3, int ldx3, const float* __restrict__ scale3,
                                                                  const float* __restrict__ shift3, const AT* __restrict__ xd, int ldxd,
                                                                  const float* __restrict__ scaled, const float* __restrict__ shiftd,
                                                                  AT* __restrict__ y, int ldy, long long M, int C, long long rows_per_block,
                                                                  unsigned long long* __restrict__ signs) {
  const int gq = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = (blockIdx.x * 64 + gq) * 4;
  const float4 s3 = *reinterpret_cast<const float4*>(scale3 + c), h3 = *reinterpret_cast<const float4*>(shift3 + c);
  const float4 sd = *reinterpret_cast<const float4*>(scaled + c), hd = *reinterpret_cast<const float4*>(shiftd + c);
  const long long r0 = (long long)blockIdx.y * rows_per_block;
  long long r1 = r0 + rows_per_block; if (r1 > M) r1 = M;
#pragma unroll 2
  for (long long r = r0 + rl; r < r1; r += 4) {
    const float4 xv = ld4f(x3 + (size_t)r * ldx3 + c), dv = ld4f(xd + (size_t)r * ldxd + c);
    const float t[4] = {__fmaf_rn(dv.x, sd.x, hd.x), __fmaf_rn(dv.y, sd.y, hd.y), __fmaf_rn(dv.z, sd.z, hd.z), __fmaf_rn(dv.w, sd.w, hd.w)};
    float o[4] = {__fmaf_rn(xv.x, s3.x, h3.x), __fmaf_rn(xv.y, s3.y, h3.y), __fmaf_rn(xv.z, s3.z, h3.z), __fmaf_rn(xv.w, s3.w, h3.w)};
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] += (float)(AT)t[j];
    bn_signs_store(signs, r, C, gq, o);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = apply_act(o[j], SV_ACT_RELU, 0.f);
    st4f(y + (size_t)r * ldy + c, make_float4(o[0], o[1], o[2], o[3]));
  }
}

template <typename AT>
__global__ __launch_bounds__(256) void bn_bwd2_reduce_kernel(const AT* __restrict__ dz, int lddz, const unsigned long long* __restrict__ signs,
                                                             const AT* __restrict__ x3, int ldx3, const float* __restrict__ mean3,
                                                             const float* __restrict__ rstd3, const AT* __restrict__ xd, int ldxd,
                                                             const float* __restrict__ meand, const float* __restrict__ rstdd, long long M, int C,
                                                             double* __restrict__ sums3, double* __restrict__ sumsd, long long rows_per_block) {
  __shared__ double red[256][13];   // [thread][sum d | sum d xhat_3 | sum d xhat_d] x 4 channels (+1 pad)
  const int gq = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = (blockIdx.x * 64 + gq) * 4;
  const long long r0 = (long long)blockIdx.y * rows_per_block;
  long long r1e = r0 + rows_per_block; if (r1e > M) r1e = M;
  double s[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  float m3[4], q3[4], md[4], qd[4];
  ldnf<4>(mean3 + c, m3); ldnf<4>(rstd3 + c, q3); ldnf<4>(meand + c, md); ldnf<4>(rstdd + c, qd);
  BnMaskRule<4> mk;
  bn_mask_rule(mk, SV_ACT_RELU, 0.f, BN_MASK_SIGNS, gq, nullptr, nullptr, c);
  // a row in two steps, as in bn_bwd_reduce_vec_kernel
  struct Row { float d[4], x[4], e[4]; BnMask<4> k; };
  auto load = [&](long long r, Row& w) __attribute__((always_inline)) {
    ldnf<4>(x3 + (size_t)r * ldx3 + c, w.x); ldnf<4>(xd + (size_t)r * ldxd + c, w.e); ldnf<4>(dz + (size_t)r * lddz + c, w.d);
    bn_mask_load(mk, w.k, (const AT*)nullptr, 0, signs, r, C);
  };
  auto terms = [&](Row& w, float (&t)[12]) __attribute__((always_inline)) {
    bn_mask_grad(mk, w.k, w.d, w.x);
#pragma unroll
    for (int j = 0; j < 4; ++j) { t[j] = w.d[j]; t[4 + j] = w.d[j] * (w.x[j] - m3[j]) * q3[j]; t[8 + j] = w.d[j] * (w.e[j] - md[j]) * qd[j]; }
  };
  Row w0, w1;
  float t0[12], t1[12];
  long long r = r0 + rl;
  for (; r + 4 < r1e; r += 8) {   // two rows in flight
    load(r, w0); load(r + 4, w1);
    terms(w0, t0); terms(w1, t1);
#pragma unroll
    for (int j = 0; j < 12; ++j) s[j] += (double)t0[j] + (double)t1[j];
  }
  for (; r < r1e; r += 4) {
    load(r, w0);
    terms(w0, t0);
#pragma unroll
    for (int j = 0; j < 12; ++j) s[j] += (double)t0[j];
  }
  // sum d belongs to both layers' images
  bn_slot_fold<4, 3>(red, s, 64, 4, blockIdx.x, blockIdx.y, C, [&](int k, size_t i, double a) {
    if (k == 0) { atomicAdd(sums3 + i, a); atomicAdd(sumsd + i, a); }
    else if (k == 1) atomicAdd(sums3 + i + C, a);
    else atomicAdd(sumsd + i + C, a);
  });
}

template <typename AT>
__global__ __launch_bounds__(256) void bn_bwd2_apply_kernel(const AT* __restrict__ dz, int lddz, const unsigned long long* __restrict__ signs,
                                                            const AT* __restrict__ x3, int ldx3, const float* __restrict__ gamma3,
                                                            const float* __restrict__ mean3, const float* __restrict__ rstd3,
                                                            const AT* __restrict__ xd, int ldxd, const float* __restrict__ gammad,
                                                            const float* __restrict__ meand, const float* __restrict__ rstdd,
                                                            const double* __restrict__ sums3, const double* __restrict__ sumsd, long long M, int C,
                                                            AT* __restrict__ dx3, int lddx3, AT* __restrict__ dxd, int lddxd, long long rows_per_block) {
  const int gq = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = (blockIdx.x * 64 + gq) * 4;
  BnMaskRule<4> mk;
  bn_mask_rule(mk, SV_ACT_RELU, 0.f, BN_MASK_SIGNS, gq, nullptr, nullptr, c);
  double k1[4], k2[4], k3[4], l1[4], l2[4], l3[4];     // per layer
  const double invM = 1.0 / (double)M;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bn_bwd_coef(gamma3, mean3, rstd3, bn_bwd_folded(sums3, C), invM, 1, c + j, C, k1[j], k2[j], k3[j]);
    bn_bwd_coef(gammad, meand, rstdd, bn_bwd_folded(sumsd, C), invM, 1, c + j, C, l1[j], l2[j], l3[j]);
  }
  const long long r0 = (long long)blockIdx.y * rows_per_block;
  long long r1 = r0 + rows_per_block; if (r1 > M) r1 = M;
#pragma unroll 2
  for (long long r = r0 + rl; r < r1; r += 4) {
    float d[4], xx[4], ee[4], o[4], u[4];
    ldnf<4>(x3 + (size_t)r * ldx3 + c, xx); ldnf<4>(xd + (size_t)r * ldxd + c, ee); ldnf<4>(dz + (size_t)r * lddz + c, d);
    bn_mask_row(mk, (const AT*)nullptr, 0, signs, r, C, d, xx);
#pragma unroll
    for (int j = 0; j < 4; ++j) { o[j] = bn_bwd_dx(k1[j], k2[j], k3[j], d[j], xx[j]); u[j] = bn_bwd_dx(l1[j], l2[j], l3[j], d[j], ee[j]); }
    stnf<4>(dx3 + (size_t)r * lddx3 + c, o);
    stnf<4>(dxd + (size_t)r * lddxd + c, u);
  }
}


// ------------------------------------------------------------------------------------------------
// ResNet stem: BatchNorm + ReLU + MaxPool2d(3, stride 2, padding 1) (reference models/encoder.py:22-23: torchvision resnet50's bn1 / relu /
// maxpool) without the 112 x 112 x 64 activation in between - at 512 images that tensor is 822 MB, written by the normalisation pass, read by
// the pool, written again (as its gradient) by the pool's backward and read twice by the BatchNorm backward.
//   forward : pooled[o] = max over the window of relu(scale * y + shift) (each value rounded to the storage type first, as the separate pass
//             stored it), arg-max tap kept (first maximum in scan order, as torch) - reads y once, writes the 56 x 56 map + 1 byte per element;
//   backward: dz[i] = sum over the <= 2 x 2 windows that contain i of dpooled[o] * [argmax(o) == i] (the pool's gather form), computed on the
//             fly in BOTH passes of the BatchNorm backward (reduce: sums of dz' and dz' * xhat; apply: dy = k1 dz' - k2 - k3 y): neither dz nor
//             the activation is ever stored.
// A thread owns 4 adjacent channels; a workgroup walks whole image rows (no per-position divisions).
// ------------------------------------------------------------------------------------------------
// CV = channels per thread: 8 with bf16 storage (16-byte accesses), else 4
template <int CV> struct TapWord;
template <> struct TapWord<4> { typedef unsigned type; };
template <> struct TapWord<8> { typedef unsigned long long type; };
template <int CV> __device__ __forceinline__ void ld_taps(const uint8_t* p, int (&t)[CV]) {
  const typename TapWord<CV>::type w = *reinterpret_cast<const typename TapWord<CV>::type*>(p);
#pragma unroll
  for (int j = 0; j < CV; ++j) t[j] = (int)((w >> (8 * j)) & 0xff);
}
template <typename AT, int CV>
__global__ __launch_bounds__(256) void bn_act_maxpool_fwd_kernel(const AT* __restrict__ x, const float* __restrict__ fsc, const float* __restrict__ fsh,
                                                                 AT* __restrict__ y, uint8_t* __restrict__ idx, int N, int H, int W, int C, int Ho, int Wo,
                                                                 int act, float slope) {
  const int cv = C / CV;
  const long long total = (long long)N * Ho * Wo * cv;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % cv) * CV; long long t = i / cv;
    const int ow = (int)(t % Wo); t /= Wo; const int oh = (int)(t % Ho); const int n = (int)(t / Ho);
    float s_[CV], h_[CV], best[CV];
    int bi[CV];
#pragma unroll
    for (int j = 0; j < CV; ++j) { s_[j] = fsc[c + j]; h_[j] = fsh[c + j]; best[j] = -3.4e38f; bi[j] = 0; }
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int ih = oh * 2 - 1 + kh, iw = ow * 2 - 1 + kw;
        if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W) {
          float v[CV];
          ldnf<CV>(x + (((size_t)n * H + ih) * W + iw) * C + c, v);
#pragma unroll
          for (int j = 0; j < CV; ++j) {
            const float z = (float)(AT)apply_act(__fmaf_rn(v[j], s_[j], h_[j]), act, slope);   // what scale_shift_act would have stored
            if (z > best[j]) { best[j] = z; bi[j] = kh * 3 + kw; }
          }
        }
      }
    const size_t o = (((size_t)n * Ho + oh) * Wo + ow) * C + c;
    stnf<CV>(y + o, best);
    typename TapWord<CV>::type w = 0;
#pragma unroll
    for (int j = 0; j < CV; ++j) w |= (typename TapWord<CV>::type)bi[j] << (8 * j);
    *reinterpret_cast<typename TapWord<CV>::type*>(idx + o) = w;
  }
}

// The pool's data gradient for the 2 x 2 input block (2a .. 2a + 1, 2b .. 2b + 1), channels c .. c + CV - 1: the block lies in the windows (a, b),
// (a, b + 1), (a + 1, b), (a + 1, b + 1) only, so four pooled gradients + their arg-max taps (tap = 3 kh + kw, input = 2 o - 1 + k) serve four
// positions - and all four loads go out together (the per-position gather form of maxpool2d_bwd_kernel re-reads each pooled element 2.25
// times behind data-dependent loop bounds: 1.57 ms for the two passes against 1.51 for the separate kernels).  d[p][j]: p = 2 * dy + dx.
template <typename AT, int CV>
__device__ __forceinline__ void pool_block_grad(const AT* __restrict__ dmp, const uint8_t* __restrict__ idx, int n, int a, int b, int c, int C, int Ho, int Wo,
                                                float (&d)[4][CV]) {
  const size_t o00 = (((size_t)n * Ho + a) * Wo + b) * C + c;
  const bool vb = b + 1 < Wo, va = a + 1 < Ho;
  const size_t o01 = vb ? o00 + C : o00, o10 = va ? o00 + (size_t)Wo * C : o00, o11 = (va && vb) ? o00 + (size_t)Wo * C + C : o00;
  float g0[CV], g1[CV], g2[CV], g3[CV];
  int i0[CV], i1[CV], i2[CV], i3[CV];
  ldnf<CV>(dmp + o00, g0); ldnf<CV>(dmp + o01, g1); ldnf<CV>(dmp + o10, g2); ldnf<CV>(dmp + o11, g3);
  ld_taps<CV>(idx + o00, i0); ld_taps<CV>(idx + o01, i1); ld_taps<CV>(idx + o10, i2); ld_taps<CV>(idx + o11, i3);
#pragma unroll
  for (int j = 0; j < CV; ++j) {
    const int t1 = vb ? i1[j] : 255, t2 = va ? i2[j] : 255, t3 = (va && vb) ? i3[j] : 255;
    d[0][j] = i0[j] == 4 ? g0[j] : 0.f;
    d[1][j] = (i0[j] == 5 ? g0[j] : 0.f) + (t1 == 3 ? g1[j] : 0.f);
    d[2][j] = (i0[j] == 7 ? g0[j] : 0.f) + (t2 == 1 ? g2[j] : 0.f);
    d[3][j] = (i0[j] == 8 ? g0[j] : 0.f) + (t1 == 6 ? g1[j] : 0.f) + (t2 == 2 ? g2[j] : 0.f) + (t3 == 0 ? g3[j] : 0.f);
  }
}

// G = C / CV column groups x 256 / G block lanes; blockIdx.x owns image-row PAIRS [blockIdx.x * rpb, +rpb) of the N * Ho pairs.
// APPLY = false: pass 1 (sums of dz' and dz' * xhat into slot images); APPLY = true: pass 2 (dx = k1 dz' - k2 - k3 x, dz' gathered again)
template <typename AT, int CV, bool APPLY>
__global__ __launch_bounds__(256) void bn_pool_bwd_kernel(const AT* __restrict__ dmp, const uint8_t* __restrict__ idx, const AT* __restrict__ x,
                                                          const float* __restrict__ gamma, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          const float* __restrict__ fsc, const float* __restrict__ fsh, double* __restrict__ sums,
                                                          AT* __restrict__ dx, int N, int H, int W, int C, int Ho, int Wo, int act, float slope,
                                                          int training, int rpb) {
  __shared__ double red[APPLY ? 1 : 256][2 * CV + 1];
  const int G = C / CV, gq = threadIdx.x % G, rl = threadIdx.x / G, RL = 256 / G, c = gq * CV;
  double s[2 * CV];
#pragma unroll
  for (int j = 0; j < 2 * CV; ++j) s[j] = 0.0;
  if (rl < RL) {
    double k1[CV], k2[CV], k3[CV];     // APPLY
    float mm[CV], rr[CV];              // !APPLY
    BnMaskRule<CV> mk;
    bn_mask_rule(mk, act, slope, BN_MASK_X, 0, fsc, fsh, c);
#pragma unroll
    for (int j = 0; j < CV; ++j) {
      if constexpr (APPLY) bn_bwd_coef(gamma, mean, rstd, bn_bwd_folded(sums, C), 1.0 / ((double)N * H * W), training, c + j, C, k1[j], k2[j], k3[j]);
      else { mm[j] = mean[c + j]; rr[j] = rstd[c + j]; }
    }
    const int rp0 = blockIdx.x * rpb, rp1 = min(rp0 + rpb, N * Ho);
    for (int rp = rp0; rp < rp1; ++rp) {
      const int n = rp / Ho, a = rp - n * Ho;
      float t1[CV], t2[CV];      // one row pair per lane in fp32 (<= 4 Wo / RL terms), then double
#pragma unroll
      for (int j = 0; j < CV; ++j) { t1[j] = 0.f; t2[j] = 0.f; }
      for (int b = rl; b < Wo; b += RL) {
        float d[4][CV];
        pool_block_grad<AT, CV>(dmp, idx, n, a, b, c, C, Ho, Wo, d);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int ih = 2 * a + (p >> 1), iw = 2 * b + (p & 1);
          if (ih < H && iw < W) {
            const size_t o = (((size_t)n * H + ih) * W + iw) * C + c;
            float xx[CV], out[CV];
            ldnf<CV>(x + o, xx);
#pragma unroll
            for (int j = 0; j < CV; ++j) {
              bn_mask_grad(bn_mask_rule_of(mk, j), &d[p][j], &xx[j]);      // per channel: fewer live registers than all CV up front
              if constexpr (APPLY) out[j] = bn_bwd_dx(k1[j], k2[j], k3[j], d[p][j], xx[j]);
              else { t1[j] += d[p][j]; t2[j] += d[p][j] * (xx[j] - mm[j]) * rr[j]; }
            }
            if constexpr (APPLY) stnf<CV>(dx + o, out);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < CV; ++j) { s[j] += (double)t1[j]; s[CV + j] += (double)t2[j]; }
    }
  }
  if constexpr (!APPLY) bn_slot_fold_one<CV>(red, s, G, RL, 0, blockIdx.x, C, sums);
}

// ------------------------------------------------------------------------------------------------
// The same fusion around MaxPool3d(2) (floor: 33 -> 16, 17 -> 8, 9 -> 4) for the three down-sampling layers of the Refiner (reference
// models/refiner.py:21-39: Conv3d -> BatchNorm3d -> LeakyReLU -> MaxPool3d): windows do not overlap, an input position lies in at most one
// window and the last plane of an odd grid in none.  tap = 4 dz + 2 dy + dx (sv_maxpool3d_fwd's numbering).  A thread owns CV channels of one
// window (forward) / of one 2 x 2 x 2 input block, partial blocks at the far faces included (backward: their gradient is -k2 - k3 x).
// ------------------------------------------------------------------------------------------------
template <typename AT, int CV>
__global__ __launch_bounds__(256) void bn_act_maxpool3d_fwd_kernel(const AT* __restrict__ x, const float* __restrict__ fsc, const float* __restrict__ fsh,
                                                                   AT* __restrict__ y, uint8_t* __restrict__ idx, int N, int D, int H, int W, int C,
                                                                   int act, float slope) {
  const int Do = D / 2, Ho = H / 2, Wo = W / 2, cv = C / CV;
  const long long total = (long long)N * Do * Ho * Wo * cv;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % cv) * CV; long long t = i / cv;
    const int ow = (int)(t % Wo); t /= Wo; const int oh = (int)(t % Ho); t /= Ho; const int od = (int)(t % Do); const int n = (int)(t / Do);
    float s_[CV], h_[CV], best[CV];
    int bi[CV];
#pragma unroll
    for (int j = 0; j < CV; ++j) { s_[j] = fsc[c + j]; h_[j] = fsh[c + j]; best[j] = -3.4e38f; bi[j] = 0; }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float v[CV];
      ldnf<CV>(x + ((((size_t)n * D + od * 2 + (k >> 2)) * H + oh * 2 + ((k >> 1) & 1)) * W + ow * 2 + (k & 1)) * C + c, v);
#pragma unroll
      for (int j = 0; j < CV; ++j) {
        const float z = (float)(AT)apply_act(__fmaf_rn(v[j], s_[j], h_[j]), act, slope);   // what scale_shift_act would have stored
        if (z > best[j]) { best[j] = z; bi[j] = k; }
      }
    }
    const size_t o = ((((size_t)n * Do + od) * Ho + oh) * Wo + ow) * C + c;
    stnf<CV>(y + o, best);
    typename TapWord<CV>::type w = 0;
#pragma unroll
    for (int j = 0; j < CV; ++j) w |= (typename TapWord<CV>::type)bi[j] << (8 * j);
    *reinterpret_cast<typename TapWord<CV>::type*>(idx + o) = w;
  }
}

// APPLY = false: pass 1 (sums of dz' and dz' * xhat into slot images); APPLY = true: pass 2 (dx = k1 dz' - k2 - k3 x)
template <typename AT, int CV, bool APPLY>
__global__ __launch_bounds__(256) void bn_pool3d_bwd_kernel(const AT* __restrict__ dmp, const uint8_t* __restrict__ idx, const AT* __restrict__ x,
                                                            const float* __restrict__ gamma, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ fsc, const float* __restrict__ fsh, double* __restrict__ sums,
                                                            AT* __restrict__ dx, int N, int D, int H, int W, int C, int act, float slope, int training,
                                                            long long bpw) {
  __shared__ double red[APPLY ? 1 : 256][2 * CV + 1];
  const int Do = D / 2, Ho = H / 2, Wo = W / 2, BD = (D + 1) / 2, BH = (H + 1) / 2, BW = (W + 1) / 2;
  const int G = C / CV, gq = threadIdx.x % G, rl = threadIdx.x / G, RL = 256 / G, c = gq * CV;
  const long long nblk = (long long)N * BD * BH * BW;
  const long long q0 = (long long)blockIdx.x * bpw, q1 = q0 + bpw < nblk ? q0 + bpw : nblk;
  double s[2 * CV];
#pragma unroll
  for (int j = 0; j < 2 * CV; ++j) s[j] = 0.0;
  if (rl < RL) {
    double k1[CV], k2[CV], k3[CV];     // APPLY
    float mm[CV], rr[CV];              // !APPLY
    BnMaskRule<CV> mk;
    bn_mask_rule(mk, act, slope, BN_MASK_X, 0, fsc, fsh, c);
#pragma unroll
    for (int j = 0; j < CV; ++j) {
      if constexpr (APPLY) bn_bwd_coef(gamma, mean, rstd, bn_bwd_folded(sums, C), 1.0 / ((double)N * D * H * W), training, c + j, C, k1[j], k2[j], k3[j]);
      else { mm[j] = mean[c + j]; rr[j] = rstd[c + j]; }
    }
    for (long long q = q0 + rl; q < q1; q += RL) {
      long long t = q;
      const int bw = (int)(t % BW); t /= BW; const int bh = (int)(t % BH); t /= BH; const int bd = (int)(t % BD); const int n = (int)(t / BD);
      const bool win = bd < Do && bh < Ho && bw < Wo;
      float g[CV];
      int tp[CV];
#pragma unroll
      for (int j = 0; j < CV; ++j) { g[j] = 0.f; tp[j] = 255; }
      if (win) {
        const size_t o = ((((size_t)n * Do + bd) * Ho + bh) * Wo + bw) * C + c;
        ldnf<CV>(dmp + o, g);
        ld_taps<CV>(idx + o, tp);
      }
      float t1[CV], t2[CV];
#pragma unroll
      for (int j = 0; j < CV; ++j) { t1[j] = 0.f; t2[j] = 0.f; }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int id = 2 * bd + (k >> 2), ih = 2 * bh + ((k >> 1) & 1), iw = 2 * bw + (k & 1);
        if (id < D && ih < H && iw < W) {
          const size_t o = ((((size_t)n * D + id) * H + ih) * W + iw) * C + c;
          float xx[CV], dd[CV], out[CV];
          ldnf<CV>(x + o, xx);
#pragma unroll
          for (int j = 0; j < CV; ++j) dd[j] = tp[j] == k ? g[j] : 0.f;
          bn_mask_grad(mk, dd, xx);
#pragma unroll
          for (int j = 0; j < CV; ++j) {
            if constexpr (APPLY) out[j] = bn_bwd_dx(k1[j], k2[j], k3[j], dd[j], xx[j]);
            else { t1[j] += dd[j]; t2[j] += dd[j] * (xx[j] - mm[j]) * rr[j]; }
          }
          if constexpr (APPLY) stnf<CV>(dx + o, out);
        }
      }
#pragma unroll
      for (int j = 0; j < CV; ++j) { s[j] += (double)t1[j]; s[CV + j] += (double)t2[j]; }
    }
  }
  if constexpr (!APPLY) bn_slot_fold_one<CV>(red, s, G, RL, 0, blockIdx.x, C, sums);
}


}  // namespace sv

using namespace sv;

// What a token-LayerNorm call launches, for valid arguments: pure host code behind the four entries and sv_layernorm_plan.  a, b, c = the
// activation tensors of the call (forward: x, y; backward: dy, x, dx), looked at for their alignment only.
static sv_norm_plan ln_plan(bool bwd, long long rows, int C, int merge_H, int act_dtype, const void* a, const void* b, const void* c = nullptr) {
  sv_norm_plan p{};
  p.family = bwd ? SV_NORM_LN_BWD : SV_NORM_LN_FWD; p.merge = merge_H > 0; p.storage = act_dtype;
  // VEC = 8 needs bf16 storage, 8-element channel groups (also of the un-merged map) and 16-byte aligned tensors
  const bool v8 = act_dtype == SV_BF16 && C % 8 == 0 && (merge_H == 0 || (C / 4) % 8 == 0) && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
  p.vec = v8 ? 8 : 4; ln_shape(C / p.vec, p.lanes, p.nv);
  const int rpi = 4 * (64 / p.lanes);                   // rows per workgroup (backward: per workgroup iteration)
  long long rpb = bwd ? rows / 1024 : rpi; if (rpb < rpi) rpb = rpi; if (rpb > 256) rpb = 256;   // backward: >= ~1024 workgroups where the row count allows
  p.rows[0] = rpb = (rpb + rpi - 1) / rpi * rpi;
  p.launch[0] = {cdiv(rows, rpb), 1, 256, bwd ? (int)sizeof(float) * 2 * C : 0};
  p.launch[1] = {cdiv(2 * C, 256), 1, 256, 0}; p.launches = bwd ? 2 : 1;     // ln_bwd_fold_kernel
  return p;
}
// (merge, VEC, storage type) of a plan as MERGE, AT, VEC for the statement: the one selection of the LayerNorm entries
#define SV_LN_SELECT_AT(P_, ...)                                                                       \
  if (P_.vec == 8) { typedef __bf16 AT; constexpr int VEC = 8; __VA_ARGS__ }                           \
  else if (P_.storage == SV_BF16) { typedef __bf16 AT; constexpr int VEC = 4; __VA_ARGS__ }            \
  else { typedef float AT; constexpr int VEC = 4; __VA_ARGS__ }
#define SV_LN_SELECT(P_, ...)                                                                          \
  do {                                                                                                 \
    if (P_.merge) { constexpr bool MERGE = true; SV_LN_SELECT_AT(P_, __VA_ARGS__) }                    \
    else { constexpr bool MERGE = false; SV_LN_SELECT_AT(P_, __VA_ARGS__) }                            \
  } while (0)
// qo: nothing (the plain forward), or the LnQuantOut / LnQuantMxOut of the quantising forms
template <bool MERGE, typename AT, int VEC, typename... QO>
static void ln_fwd_launch(const sv_norm_plan& p, const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, long long rows, int C,
                          float eps, int merge_H, int merge_W, void* stream, QO... qo) {
  const MergeMap mm{merge_H, merge_W, merge_H > 0 ? C / 4 : 0};
  SV_LN_DISPATCH(p.lanes, p.nv, hipLaunchKernelGGL((ln_fwd_kernel<MERGE, AT, VEC, LPR, NV, QO...>), dim3(p.launch[0].grid_x), dim3(256), 0, (hipStream_t)stream,
                                                   static_cast<const AT*>(x), gamma, beta, static_cast<AT*>(y), mean, rstd, rows, C, eps, mm, qo...););
}
// the refusals both forward entries share (everything but the null checks of their outputs); `who` names the entry in the message
static int ln_fwd_check(const char* who, const void* x, const float* gamma, const float* beta, long long rows, int C, int merge_H, int merge_W,
                        int act_dtype) {
  SV_REQUIRE(x && gamma && beta && rows > 0, "%s: null/empty argument", who);
  SV_REQUIRE(C % 4 == 0 && C <= 3072, "%s: C=%d must be a multiple of 4 and <= 3072", who, C);
  SV_REQUIRE(act_dtype == SV_F32 || act_dtype == SV_BF16, "%s: bad activation dtype %d", who, act_dtype);
  SV_REQUIRE((((uintptr_t)gamma | (uintptr_t)beta) & 15) == 0, "%s: gamma/beta must be 16-byte aligned", who);
  if (merge_H > 0) SV_REQUIRE(merge_H % 2 == 0 && merge_W % 2 == 0 && C % 16 == 0, "%s(merge): H,W must be even and C a multiple of 16", who);
  return SV_OK;
}

extern "C" int sv_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                                long long rows, int C, float eps, int merge_H, int merge_W, int act_dtype, void* stream) {
  SV_REQUIRE(y && mean && rstd, "layernorm_fwd: null/empty argument");
  if (const int rc = ln_fwd_check("layernorm_fwd", x, gamma, beta, rows, C, merge_H, merge_W, act_dtype)) return rc;
  const sv_norm_plan p = ln_plan(false, rows, C, merge_H, act_dtype, x, y);
  SV_LN_SELECT(p, ln_fwd_launch<MERGE, AT, VEC>(p, x, gamma, beta, y, mean, rstd, rows, C, eps, merge_H, merge_W, stream););
  return check_launch("sv_layernorm_fwd");
}
// The body of both quantising entries: QO = LnQuantOut (ST = float) or LnQuantMxOut (uint8_t); who / sname name the entry and its scale argument in the messages
template <typename QO, typename ST>
static int ln_quant_fwd(const char* who, const char* sname, std::atomic<long long>& launches, const void* x, const float* gamma, const float* beta, void* y,
                        float* mean, float* rstd, void* q, int Kp, void* scales, long long rows, int C, float eps, int merge_H, int merge_W, int act_dtype, void* stream) {
  SV_REQUIRE(q && scales, "%s: q and %s must not be null", who, sname);
  SV_REQUIRE((mean == nullptr) == (rstd == nullptr), "%s: mean and rstd must be null together", who);
  if (const int rc = ln_fwd_check(who, x, gamma, beta, rows, C, merge_H, merge_W, act_dtype)) return rc;
  SV_REQUIRE(C > 0 && Kp == (C + 127) / 128 * 128, "%s: Kp (%d) must be C (%d) rounded up to a multiple of 128", who, Kp, C);
  SV_REQUIRE(((uintptr_t)q & 15) == 0 && ((uintptr_t)scales & 3) == 0, "%s: q must be 16-byte aligned, %s 4-byte aligned", who, sname);
  const sv_norm_plan p = ln_plan(false, rows, C, merge_H, act_dtype, x, y);
  const QO qo{static_cast<uint8_t*>(q), static_cast<ST*>(scales), Kp};
  SV_LN_SELECT(p, ln_fwd_launch<MERGE, AT, VEC>(p, x, gamma, beta, y, mean, rstd, rows, C, eps, merge_H, merge_W, stream, qo););
  const int rc = check_launch(who);
  if (rc == SV_OK) launches.fetch_add(1, std::memory_order_relaxed);
  return rc;
}
static std::atomic<long long> layernorm_quant_launches{0}, layernorm_quant_mx_launches{0};
extern "C" long long sv_layernorm_quant_launches(void) { return layernorm_quant_launches.load(std::memory_order_relaxed); }
extern "C" long long sv_layernorm_quant_mx_launches(void) { return layernorm_quant_mx_launches.load(std::memory_order_relaxed); }
extern "C" int sv_layernorm_quant_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, void* q, int Kp, float* scales,
                                      long long rows, int C, float eps, int merge_H, int merge_W, int act_dtype, void* stream) {
  return ln_quant_fwd<LnQuantOut, float>("sv_layernorm_quant_fwd", "scales", layernorm_quant_launches, x, gamma, beta, y, mean, rstd, q, Kp, scales,
                                         rows, C, eps, merge_H, merge_W, act_dtype, stream);
}
extern "C" int sv_layernorm_quant_mx_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, void* q, int Kp, void* scales_u8,
                                         long long rows, int C, float eps, int merge_H, int merge_W, int act_dtype, void* stream) {
  return ln_quant_fwd<LnQuantMxOut, uint8_t>("sv_layernorm_quant_mx_fwd", "scales_u8", layernorm_quant_mx_launches, x, gamma, beta, y, mean, rstd, q,
                                             Kp, scales_u8, rows, C, eps, merge_H, merge_W, act_dtype, stream);
}

extern "C" size_t sv_layernorm_bwd_workspace_floats(int C) { return (size_t)LN_BWD_SLOTS * 2 * C + 2; }
// the refusals of the backward; given = every pointer the caller has to pass is there
static int ln_bwd_check(bool given, long long rows, int C, int act_dtype, const float* gamma) {
  SV_REQUIRE(given && rows > 0, "layernorm_bwd: null/empty argument");
  SV_REQUIRE(C % 4 == 0 && C <= 3072, "layernorm_bwd: C=%d unsupported", C);
  SV_REQUIRE_ACT(act_dtype);
  SV_REQUIRE(((uintptr_t)gamma & 15) == 0, "layernorm_bwd: gamma must be 16-byte aligned");
  return SV_OK;
}
extern "C" int sv_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, void* dx, float* dgamma, float* dbeta,
                                float* workspace, long long rows, int C, int merge_H, int merge_W, int accumulate_dx, int act_dtype, void* stream) {
  if (const int rc = ln_bwd_check(dy && x && gamma && mean && rstd && dx && dgamma && dbeta && workspace, rows, C, act_dtype, gamma)) return rc;
  const sv_norm_plan p = ln_plan(true, rows, C, merge_H, act_dtype, dy, x, dx);
  const MergeMap mm{merge_H, merge_W, merge_H > 0 ? C / 4 : 0};
  hipStream_t s = (hipStream_t)stream;
  SV_LN_SELECT(p, SV_LN_DISPATCH(p.lanes, p.nv, hipLaunchKernelGGL((ln_bwd_kernel<MERGE, AT, VEC, LPR, NV>), dim3(p.launch[0].grid_x), dim3(256), p.launch[0].lds_bytes, s,
                                                static_cast<const AT*>(dy), static_cast<const AT*>(x), gamma, mean, rstd, static_cast<AT*>(dx), dgamma, dbeta, rows, C,
                                                mm, accumulate_dx, (int)p.rows[0], workspace);););
  hipLaunchKernelGGL(ln_bwd_fold_kernel, dim3(p.launch[1].grid_x), dim3(256), 0, s, workspace, C, dgamma, dbeta);
  return check_launch("sv_layernorm_bwd");
}
extern "C" int sv_layernorm_plan(int kind, const void* a, const void* b, const void* c, long long rows, int C, int merge_H, int merge_W,
                                 int act_dtype, sv_norm_plan* plan) {
  static const char* const who[3] = {"layernorm_fwd", "sv_layernorm_quant_fwd", "sv_layernorm_quant_mx_fwd"};
  alignas(16) static const float params[4] = {};      // stands in for gamma / beta, which the plan does not depend on
  SV_REQUIRE(plan && kind >= 0 && kind <= 3, "layernorm_plan: null plan or bad kind %d", kind);
  if (const int rc = kind == 3 ? ln_bwd_check(a && b && c, rows, C, act_dtype, params) : ln_fwd_check(who[kind], a, params, params, rows, C, merge_H, merge_W, act_dtype)) return rc;
  *plan = ln_plan(kind == 3, rows, C, merge_H, act_dtype, a, b, kind == 3 ? c : nullptr);
  return SV_OK;
}

// image slices of lnl_bwd_apply_kernel: enough workgroups for ~8 per CU, at least 8 images per slice
static inline int lnl_image_slices(int I, int L) {
  int s = 2048 / cdiv(L, 1024);
  if (s > I / 8) s = I / 8;
  return s < 1 ? 1 : (s > 32 ? 32 : s);
}

extern "C" size_t sv_ln_image_workspace_floats(int I, int L) { return (size_t)I * cdiv(L, LNL_CHUNK) * 2; }

extern "C" int sv_ln_image_fwd(const void* x, const float* w, const float* b, void* y, float* meanrstd, float* workspace,
                               int I, int L, float eps, float drop_p, uint32_t seed, const uint32_t* seed_epoch, int act_dtype, void* stream) {
  SV_REQUIRE(x && w && b && y && meanrstd && workspace && I > 0 && L > 0 && L % 4 == 0, "ln_image_fwd: bad arguments (I=%d L=%d)", I, L);
  SV_REQUIRE_ACT(act_dtype);
  hipStream_t s = (hipStream_t)stream;
  const int nch = cdiv(L, LNL_CHUNK);
  int gx = cdiv(L, 1024); if (gx > 64) gx = 64;
  SV_DISPATCH_ACT(act_dtype,
    hipLaunchKernelGGL(lnl_moments_kernel<AT>, dim3(nch, I), dim3(256), 0, s, static_cast<const AT*>(x), workspace, L, nch);
    hipLaunchKernelGGL(lnl_finalize_kernel, dim3(cdiv(I, 64)), dim3(64), 0, s, workspace, meanrstd, L, nch, eps, I);
    hipLaunchKernelGGL(lnl_apply_kernel<AT>, dim3(gx, I), dim3(256), 0, s, static_cast<const AT*>(x), w, b, meanrstd, static_cast<AT*>(y), L, drop_p, seed, seed_epoch););
  return check_launch("sv_ln_image_fwd");
}

extern "C" int sv_ln_image_bwd(const void* dy, const void* x, const float* w, const float* meanrstd, void* dx, float* dw,
                               float* db, double* sums_ws, int I, int L, float drop_p, uint32_t seed, const uint32_t* seed_epoch, int act_dtype, void* stream) {
  SV_REQUIRE(dy && x && w && meanrstd && dx && dw && db && sums_ws && I > 0 && L > 0 && L % 4 == 0, "ln_image_bwd: bad arguments");
  SV_REQUIRE_ACT(act_dtype);
  hipStream_t s = (hipStream_t)stream;
  (void)hipMemsetAsync(sums_ws, 0, sizeof(double) * 2 * I, s);
  int gx = cdiv(L, 1024); if (gx > 32) gx = 32;
  SV_DISPATCH_ACT(act_dtype,
    hipLaunchKernelGGL(lnl_bwd_reduce_kernel<AT>, dim3(gx, I), dim3(256), 0, s, static_cast<const AT*>(dy), static_cast<const AT*>(x), w, meanrstd, sums_ws, L, drop_p, seed, seed_epoch);
    hipLaunchKernelGGL(lnl_bwd_apply_kernel<AT>, dim3(cdiv(L, 1024), lnl_image_slices(I, L)), dim3(256), 0, s, static_cast<const AT*>(dy), static_cast<const AT*>(x), w, meanrstd, sums_ws,
                       static_cast<AT*>(dx), dw, db, L, I, drop_p, seed, seed_epoch););
  return check_launch("sv_ln_image_bwd");
}

// Rows per workgroup of a BatchNorm pass whose grid is (cg column groups, row blocks): about `target` workgroups in all, but none with less
// than one loop step of `step` rows
static inline long long bn_rows_per_block(long long M, int cg, int target, int step) {
  long long splits = target / cg; if (splits < 1) splits = 1;
  const long long maxs = (M + step - 1) / step; if (splits > maxs) splits = maxs;
  return (M + splits - 1) / splits;
}
// fold the slot images of one layer, or (wsd given) of the two layers of the bn3 + down-sampling pass in one launch
static inline void bn_bwd_fold(hipStream_t s, int C, double* ws, float* dgamma, float* dbeta, double* wsd = nullptr, float* dgammad = nullptr,
                               float* dbetad = nullptr) {
  hipLaunchKernelGGL(bn_bwd_fold_kernel, dim3(cdiv(2 * C, 256), wsd ? 2 : 1), dim3(256), 0, s, ws, wsd, C, dgamma, dbeta, dgammad, dbetad);
}

extern "C" int sv_bn_stats(const void* x, long long M, int C, int ld, double* sums, int act_dtype, void* stream) {
  SV_REQUIRE(x && sums && M > 0 && C > 0 && ld >= C, "bn_stats: bad arguments");
  SV_REQUIRE_ACT(act_dtype);
  const int cg = cdiv(C, 64);
  const long long rpb = bn_rows_per_block(M, cg, 2048, 64);
  SV_DISPATCH_ACT(act_dtype, hipLaunchKernelGGL(bn_stats_kernel<AT>, dim3(cg, cdiv(M, rpb)), dim3(256), 0, (hipStream_t)stream, static_cast<const AT*>(x), M, C, ld, sums, rpb););
  return check_launch("sv_bn_stats");
}

extern "C" int sv_bn_finalize(const double* sums, long long count, const float* gamma, const float* beta, float* running_mean,
                              float* running_var, float momentum, float eps, int training, float* scale, float* shift,
                              float* save_mean, float* save_rstd, int C, void* stream) {
  SV_REQUIRE(gamma && beta && running_mean && running_var && scale && shift && save_mean && save_rstd && C > 0, "bn_finalize: null argument");
  SV_REQUIRE(!training || (sums && count > 0), "bn_finalize: training needs sums and a positive count");
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(cdiv(C, 64)), dim3(64), 0, (hipStream_t)stream, sums, (double)count, gamma, beta,
                     running_mean, running_var, momentum, eps, training, scale, shift, save_mean, save_rstd, C);
  return check_launch("sv_bn_finalize");
}

// vector paths need every activation pointer aligned to 4 elements of the storage type
static inline bool aligned4(int act_dtype, const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr,
                            const void* e = nullptr) {
  const uintptr_t m = act_dtype == SV_BF16 ? 7 : 15;
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e) & m) == 0;
}

// sign words of sv_scale_shift_act_signs / sv_bn_bwd_signs need the wave-per-row mapping of the vector kernels: G == 64 column groups
static inline bool bn_signs_ok(int C) { return C % 256 == 0; }
// ---- launch plans of the per-layer apply and backward: pure host code behind sv_scale_shift_act(_signs), sv_bn_bwd(_signs) and their queries
struct BnRows { const void* p; int ld; };     // an activation tensor of the call and its row stride; p == nullptr: not given
// A plan with the kernel family for rows of C channels: t = the activation tensors of the call, params = the fp32 vectors the vector kernels read as float4, OR-ed.
// Vector and narrow kernels need row strides that are multiples of 4 and 4-element aligned tensors; the narrow ones own the padded row (roundup4(C) columns).
static sv_norm_plan bn_family(int act_dtype, int C, std::initializer_list<BnRows> t, uintptr_t params) {
  const int c4 = (C + 3) & ~3; bool ld4 = true, room = true; uintptr_t ptrs = 0;
  for (const BnRows& r : t) if (r.p) { ld4 = ld4 && r.ld % 4 == 0; room = room && r.ld >= c4; ptrs |= (uintptr_t)r.p; }
  sv_norm_plan p{};
  if (!ld4 || !aligned4(act_dtype, (const void*)ptrs)) p.family = SV_NORM_BN_SCALAR;
  else if (C % 4 == 0 && (params & 15) == 0) p.family = SV_NORM_BN_VECTOR;
  else p.family = C <= BN_NARROW_MAXC && room ? SV_NORM_BN_NARROW : SV_NORM_BN_SCALAR;
  p.storage = act_dtype; p.vec = p.family == SV_NORM_BN_SCALAR ? 1 : 4;
  return p;
}
// vector family: G lanes across a row (4 channels each), RL rows per step of a workgroup, cg column groups along grid x
struct BnVecGeom { int G, RL, cg; };
static inline BnVecGeom bn_vec_geom(int C) { const int G = C / 4 < 64 ? C / 4 : 64; return {G, 256 / G, cdiv(C / 4, G)}; }
static inline dim3 bn_grid(const sv_norm_plan& p, int i) { return dim3(p.launch[i].grid_x, p.launch[i].grid_y); }
// p with launch i, its last = the apply pass of its family, the same grid forward and backward
static sv_norm_plan plan_bn_apply(sv_norm_plan p, int i, long long M, int C) {
  if (p.family == SV_NORM_BN_VECTOR) {
    const BnVecGeom v = bn_vec_geom(C);
    p.lanes = v.G; p.rows[1] = bn_rows_per_block(M, v.cg, 4096, 4 * v.RL);
    p.launch[i] = {v.cg, cdiv(M, p.rows[1]), 256, 0};
  } else {
    long long blocks = p.family == SV_NORM_BN_NARROW ? (M + 63) / 64 : (M * C + 255) / 256; if (blocks > 8192) blocks = 8192;
    p.launch[i] = {(int)blocks, 1, 256, 0};
  }
  p.launches = i + 1;
  return p;
}
static sv_norm_plan plan_scale_shift_act(std::initializer_list<BnRows> t, uintptr_t params, long long M, int C, int act_dtype) {
  return plan_bn_apply(bn_family(act_dtype, C, t, params), 0, M, C);
}
// arguments -> plan -> (query: report it) -> launch; behind sv_scale_shift_act, sv_scale_shift_act_signs and sv_scale_shift_act_plan
static int scale_shift_act_impl(const void* x, int ldx, const float* scale, const float* shift, const void* residual, int ldr, void* y, int ldy,
                                long long M, int C, int act, float slope, void* signs, int act_dtype, hipStream_t s, sv_norm_plan* query) {
  SV_REQUIRE(x && scale && shift && y && M > 0 && C > 0 && ldx >= C && ldy >= C, "scale_shift_act: bad arguments");
  SV_REQUIRE_ACT(act_dtype);
  const sv_norm_plan p = plan_scale_shift_act({{x, ldx}, {y, ldy}, {residual, ldr}}, (uintptr_t)scale | (uintptr_t)shift, M, C, act_dtype);
  SV_REQUIRE(!signs || (p.family == SV_NORM_BN_VECTOR && bn_signs_ok(C) && ((uintptr_t)signs & 15) == 0),
             "scale_shift_act_signs: needs C %% 256 == 0 and 4-aligned rows (C=%d)", C);
  if (query) { *query = p; return SV_OK; }
  SV_DISPATCH_ACT(act_dtype,
    const AT* x_ = static_cast<const AT*>(x); const AT* r_ = static_cast<const AT*>(residual); AT* y_ = static_cast<AT*>(y);
    switch (p.family) {
      case SV_NORM_BN_NARROW:
        hipLaunchKernelGGL(scale_shift_act_narrow_kernel<AT>, bn_grid(p, 0), dim3(256), 0, s, x_, ldx, scale, shift, r_, ldr, y_, ldy, M, C, act, slope);
        break;
      case SV_NORM_BN_VECTOR:
        hipLaunchKernelGGL(scale_shift_act_cg_kernel<AT>, bn_grid(p, 0), dim3(256), 0, s, x_, ldx, scale, shift, r_, ldr, y_, ldy, M, C, act, slope, p.rows[1],
                           p.lanes, static_cast<unsigned long long*>(signs));
        break;
      default:
        hipLaunchKernelGGL(scale_shift_act_scalar_kernel<AT>, bn_grid(p, 0), dim3(256), 0, s, x_, ldx, scale, shift, r_, ldr, y_, ldy, M, C, act, slope);
    });
  return check_launch("sv_scale_shift_act");
}

extern "C" int sv_scale_shift_act(const void* x, int ldx, const float* scale, const float* shift, const void* residual, int ldr,
                                  void* y, int ldy, long long M, int C, int act, float slope, int act_dtype, void* stream) {
  return scale_shift_act_impl(x, ldx, scale, shift, residual, ldr, y, ldy, M, C, act, slope, nullptr, act_dtype, (hipStream_t)stream, nullptr);
}
extern "C" int sv_bn_signs_supported(int C) { return bn_signs_ok(C) ? 1 : 0; }
extern "C" int sv_scale_shift_act_signs(const void* x, int ldx, const float* scale, const float* shift, const void* residual, int ldr,
                                        void* y, int ldy, long long M, int C, int act, float slope, void* signs, int act_dtype, void* stream) {
  SV_REQUIRE(signs, "scale_shift_act_signs: null sign buffer");
  return scale_shift_act_impl(x, ldx, scale, shift, residual, ldr, y, ldy, M, C, act, slope, signs, act_dtype, (hipStream_t)stream, nullptr);
}
extern "C" int sv_scale_shift_act_plan(const void* x, int ldx, const float* scale, const float* shift, const void* residual, int ldr, void* y, int ldy,
                                       long long M, int C, int act, float slope, void* signs, int act_dtype, sv_norm_plan* plan) {
  SV_REQUIRE(plan, "scale_shift_act_plan: null plan");
  return scale_shift_act_impl(x, ldx, scale, shift, residual, ldr, y, ldy, M, C, act, slope, signs, act_dtype, nullptr, plan);
}

// ---- ResNet stem, fused with its max-pool (kernels above).  x = the convolution's output [N, H, W, C] (rows of exactly C elements, C % 4 == 0,
// C <= 256 with 256 % (C / 4) == 0), pooled / idx = [N, Ho, Wo, C] with Ho = (H + 1) / 2, Wo = (W + 1) / 2 (kernel 3, stride 2, padding 1).
static bool bn_pool_shape_ok(int N, int H, int W, int C) {
  return N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && C <= 1024 && 256 % (C / 4) == 0 && (long long)N * H * W * C < (1ll << 40);
}
// 8 channels per thread (16-byte accesses): bf16 storage, C % 8 == 0 with 256 % (C / 8) == 0, 16-byte aligned tensors, 8-byte aligned tap words
static bool bn_pool_cv8(int act_dtype, int C, const void* a, const void* b, const void* c) {
  return act_dtype == SV_BF16 && C % 8 == 0 && 256 % (C / 8) == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}
extern "C" int sv_bn_act_maxpool_fwd(const void* x, const float* scale, const float* shift, void* pooled, void* idx, int N, int H, int W, int C,
                                     int act, float slope, int act_dtype, void* stream) {
  SV_REQUIRE(x && scale && shift && pooled && idx && bn_pool_shape_ok(N, H, W, C), "bn_act_maxpool_fwd: bad arguments (N=%d H=%d W=%d C=%d)", N, H, W, C);
  SV_REQUIRE_ACT(act_dtype);
  SV_REQUIRE(aligned4(act_dtype, x, pooled, nullptr, nullptr, nullptr) && (((uintptr_t)scale | (uintptr_t)shift) & 15) == 0 && ((uintptr_t)idx & 3) == 0,
             "bn_act_maxpool_fwd: misaligned buffers");
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const long long total = (long long)N * Ho * Wo * (C / 4);
  long long blocks = (total + 255) / 256; if (blocks > 16384) blocks = 16384;
  if (bn_pool_cv8(act_dtype, C, x, pooled, idx)) {
    const long long t8 = total / 2;
    long long b8 = (t8 + 255) / 256; if (b8 > 16384) b8 = 16384;
    hipLaunchKernelGGL((bn_act_maxpool_fwd_kernel<__bf16, 8>), dim3((unsigned)b8), dim3(256), 0, (hipStream_t)stream, static_cast<const __bf16*>(x),
                       scale, shift, static_cast<__bf16*>(pooled), static_cast<uint8_t*>(idx), N, H, W, C, Ho, Wo, act, slope);
    return check_launch("sv_bn_act_maxpool_fwd");
  }
  SV_DISPATCH_ACT(act_dtype, hipLaunchKernelGGL((bn_act_maxpool_fwd_kernel<AT, 4>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, static_cast<const AT*>(x),
                                                scale, shift, static_cast<AT*>(pooled), static_cast<uint8_t*>(idx), N, H, W, C, Ho, Wo, act, slope););
  return check_launch("sv_bn_act_maxpool_fwd");
}
/* dpooled [N, Ho, Wo, C] + idx -> dx [N, H, W, C] (gradient w.r.t. the BatchNorm input x), dgamma / dbeta += ; sums_ws as sv_bn_bwd */
extern "C" int sv_bn_maxpool_bwd(const void* dpooled, const void* idx, const void* x, const float* gamma, const float* save_mean, const float* save_rstd,
                                 const float* fwd_scale, const float* fwd_shift, int N, int H, int W, int C, int act, float slope, int training,
                                 void* dx, float* dgamma, float* dbeta, double* sums_ws, int act_dtype, void* stream) {
  SV_REQUIRE(dpooled && idx && x && gamma && save_mean && save_rstd && fwd_scale && fwd_shift && dx && dgamma && dbeta && sums_ws && bn_pool_shape_ok(N, H, W, C),
             "bn_maxpool_bwd: bad arguments (N=%d H=%d W=%d C=%d)", N, H, W, C);
  SV_REQUIRE_ACT(act_dtype);
  SV_REQUIRE(aligned4(act_dtype, dpooled, x, dx, nullptr, nullptr) && (((uintptr_t)save_mean | (uintptr_t)save_rstd | (uintptr_t)fwd_scale | (uintptr_t)fwd_shift) & 15) == 0 &&
             ((uintptr_t)idx & 3) == 0, "bn_maxpool_bwd: misaligned buffers");
  hipStream_t s = (hipStream_t)stream;
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const long long rows = (long long)N * Ho;     // image-row pairs
  SV_REQUIRE(rows < (1ll << 31), "bn_maxpool_bwd: more than 2^31 image rows");
  int rpb = (int)((rows + 2047) / 2048); if (rpb < 1) rpb = 1;
  const unsigned nb = (unsigned)((rows + rpb - 1) / rpb);
  int rpa = (int)((rows + 8191) / 8192); if (rpa < 1) rpa = 1;
  const unsigned na = (unsigned)((rows + rpa - 1) / rpa);
#define SV_POOL_BWD(AT_, CV_)                                                                                                                               \
  hipLaunchKernelGGL((bn_pool_bwd_kernel<AT_, CV_, false>), dim3(nb), dim3(256), 0, s, static_cast<const AT_*>(dpooled), static_cast<const uint8_t*>(idx),     \
                     static_cast<const AT_*>(x), gamma, save_mean, save_rstd, fwd_scale, fwd_shift, sums_ws, static_cast<AT_*>(dx), N, H, W, C, Ho, Wo, act,    \
                     slope, training, rpb);                                                                                                                 \
  bn_bwd_fold(s, C, sums_ws, dgamma, dbeta);                                                                                                                \
  hipLaunchKernelGGL((bn_pool_bwd_kernel<AT_, CV_, true>), dim3(na), dim3(256), 0, s, static_cast<const AT_*>(dpooled), static_cast<const uint8_t*>(idx),      \
                     static_cast<const AT_*>(x), gamma, save_mean, save_rstd, fwd_scale, fwd_shift, sums_ws, static_cast<AT_*>(dx), N, H, W, C, Ho, Wo, act,    \
                     slope, training, rpa);
  if (bn_pool_cv8(act_dtype, C, dpooled, x, dx) && ((uintptr_t)idx & 7) == 0) { SV_POOL_BWD(__bf16, 8) }
  else { SV_DISPATCH_ACT(act_dtype, SV_POOL_BWD(AT, 4)); }
#undef SV_POOL_BWD
  return check_launch("sv_bn_maxpool_bwd");
}

/* Refiner down-sampling layers: BatchNorm3d + activation + MaxPool3d(2) in one pass over the convolution's output x [N, D, H, W, C] (rows of exactly C
 * elements; C % 4 == 0 and 256 % (C / 4) == 0), pooled / idx [N, D/2, H/2, W/2, C] */
extern "C" int sv_bn_act_maxpool3d_fwd(const void* x, const float* scale, const float* shift, void* pooled, void* idx, int N, int D, int H, int W, int C,
                                       int act, float slope, int act_dtype, void* stream) {
  SV_REQUIRE(x && scale && shift && pooled && idx && D > 1 && bn_pool_shape_ok(N, H, W, C) && (long long)N * D * H * W * C < (1ll << 40),
             "bn_act_maxpool3d_fwd: bad arguments (N=%d D=%d H=%d W=%d C=%d)", N, D, H, W, C);
  SV_REQUIRE_ACT(act_dtype);
  SV_REQUIRE(aligned4(act_dtype, x, pooled, nullptr, nullptr, nullptr) && ((uintptr_t)idx & 3) == 0, "bn_act_maxpool3d_fwd: misaligned buffers");
  const long long win = (long long)N * (D / 2) * (H / 2) * (W / 2);
  if (win == 0) return SV_OK;
  hipStream_t s = (hipStream_t)stream;
  if (bn_pool_cv8(act_dtype, C, x, pooled, idx)) {
    long long blocks = (win * (C / 8) + 255) / 256; if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL((bn_act_maxpool3d_fwd_kernel<__bf16, 8>), dim3((unsigned)blocks), dim3(256), 0, s, static_cast<const __bf16*>(x), scale, shift,
                       static_cast<__bf16*>(pooled), static_cast<uint8_t*>(idx), N, D, H, W, C, act, slope);
  } else {
    long long blocks = (win * (C / 4) + 255) / 256; if (blocks > 16384) blocks = 16384;
    SV_DISPATCH_ACT(act_dtype, hipLaunchKernelGGL((bn_act_maxpool3d_fwd_kernel<AT, 4>), dim3((unsigned)blocks), dim3(256), 0, s, static_cast<const AT*>(x), scale, shift,
                                                  static_cast<AT*>(pooled), static_cast<uint8_t*>(idx), N, D, H, W, C, act, slope););
  }
  return check_launch("sv_bn_act_maxpool3d_fwd");
}
extern "C" int sv_bn_maxpool3d_bwd(const void* dpooled, const void* idx, const void* x, const float* gamma, const float* save_mean, const float* save_rstd,
                                   const float* fwd_scale, const float* fwd_shift, int N, int D, int H, int W, int C, int act, float slope, int training,
                                   void* dx, float* dgamma, float* dbeta, double* sums_ws, int act_dtype, void* stream) {
  SV_REQUIRE(dpooled && idx && x && gamma && save_mean && save_rstd && fwd_scale && fwd_shift && dx && dgamma && dbeta && sums_ws && D > 1 &&
             bn_pool_shape_ok(N, H, W, C) && (long long)N * D * H * W * C < (1ll << 40), "bn_maxpool3d_bwd: bad arguments (N=%d D=%d H=%d W=%d C=%d)", N, D, H, W, C);
  SV_REQUIRE_ACT(act_dtype);
  SV_REQUIRE(aligned4(act_dtype, dpooled, x, dx, nullptr, nullptr) && ((uintptr_t)idx & 3) == 0, "bn_maxpool3d_bwd: misaligned buffers");
  hipStream_t s = (hipStream_t)stream;
  const long long nblk = (long long)N * ((D + 1) / 2) * ((H + 1) / 2) * ((W + 1) / 2);
  long long bpr = (nblk + 2047) / 2048, bpa = (nblk + 8191) / 8192;
  const unsigned nr = (unsigned)((nblk + bpr - 1) / bpr), na = (unsigned)((nblk + bpa - 1) / bpa);
#define SV_POOL3D_BWD(AT_, CV_)                                                                                                                             \
  hipLaunchKernelGGL((bn_pool3d_bwd_kernel<AT_, CV_, false>), dim3(nr), dim3(256), 0, s, static_cast<const AT_*>(dpooled), static_cast<const uint8_t*>(idx),   \
                     static_cast<const AT_*>(x), gamma, save_mean, save_rstd, fwd_scale, fwd_shift, sums_ws, static_cast<AT_*>(dx), N, D, H, W, C, act, slope,  \
                     training, bpr);                                                                                                                        \
  bn_bwd_fold(s, C, sums_ws, dgamma, dbeta);                                                                                                                \
  hipLaunchKernelGGL((bn_pool3d_bwd_kernel<AT_, CV_, true>), dim3(na), dim3(256), 0, s, static_cast<const AT_*>(dpooled), static_cast<const uint8_t*>(idx),    \
                     static_cast<const AT_*>(x), gamma, save_mean, save_rstd, fwd_scale, fwd_shift, sums_ws, static_cast<AT_*>(dx), N, D, H, W, C, act, slope,  \
                     training, bpa);
  if (bn_pool_cv8(act_dtype, C, dpooled, x, dx) && ((uintptr_t)idx & 7) == 0) { SV_POOL3D_BWD(__bf16, 8) }
  else { SV_DISPATCH_ACT(act_dtype, SV_POOL3D_BWD(AT, 4)); }
#undef SV_POOL3D_BWD
  return check_launch("sv_bn_maxpool3d_bwd");
}

extern "C" size_t sv_bn_bwd_workspace_doubles(int C) { return (size_t)(BN_BWD_SLOTS + 1) * 2 * C + 2; }
// t = dz, z, x, dx, dres with their row strides; params = save_mean | save_rstd | fwd_scale | fwd_shift, all four read as float4 by the vector kernels
static sv_norm_plan plan_bn_bwd(std::initializer_list<BnRows> t, uintptr_t params, long long M, int C, int act, bool dres, bool signs, int act_dtype) {
  sv_norm_plan p = bn_family(act_dtype, C, t, params);
  if (p.family == SV_NORM_BN_NARROW) { p.rows[0] = 16; p.launch[0] = {cdiv(M, 64 * 16), 1, 256, 0}; }   // 16 rows per thread, 64 row lanes
  else {
    int cg, step;                                           // column groups along grid x, rows of one loop step of a workgroup
    if (p.family == SV_NORM_BN_VECTOR) {
      const BnVecGeom v = bn_vec_geom(C); cg = v.cg; step = 2 * v.RL;
      // with a residual-branch gradient to produce (dres) the reduce pass stores the masked gradient there and the apply pass reads IT,
      // mask-free, instead of (dz, z): 7 instead of 8 passes over the tensor.  The sums are of the fp32 values, the stored ones are
      // rounded to the storage type - as dres always was.  The hand-off needs the stored value to BE the masked gradient: true for ReLU
      // (dz or 0) and for fp32 storage, not for LeakyReLU in bf16, where slope * dz rounds and dx would inherit 2^-9 |gamma rstd dz'| -
      // there the apply pass masks dz itself (from z / x, or from the sign words) and dres only carries the residual branch's gradient.
      const bool premask = dres && act != SV_ACT_NONE && !(act == SV_ACT_LRELU && act_dtype == SV_BF16);
      p.mask = premask ? SV_MASK_PREMASK : signs ? SV_MASK_SIGN_APPLY : SV_MASK_PLAIN;   // SIGN_APPLY: the reduce pass still delivers dres, the apply pass reads (dz, words)
    } else {
      int CW = 1; while (CW < C && CW < 64) CW <<= 1;       // channel lanes: next power of two of C, at most 64
      p.lanes = CW; cg = cdiv(C, CW); step = 4 * (256 / CW);
    }
    p.rows[0] = bn_rows_per_block(M, cg, 2048, step);
    p.launch[0] = {cg, cdiv(M, p.rows[0]), 256, 0};
  }
  p.launch[1] = {cdiv(2 * C, 256), 1, 256, 0};              // bn_bwd_fold
  return plan_bn_apply(p, 2, M, C);
}
// arguments -> plan -> (query: report it) -> launch; behind sv_bn_bwd, sv_bn_bwd_signs and sv_bn_bwd_plan
static int bn_bwd_impl(const void* dz, int lddz, const void* z, int ldz, const void* signs, const void* x, int ldx, const float* gamma, const float* save_mean,
                       const float* save_rstd, long long M, int C, int act, float slope, int training, void* dx, int lddx, void* dres, int lddres, float* dgamma,
                       float* dbeta, double* sums_ws, const float* fsc, const float* fsh, int act_dtype, hipStream_t s, sv_norm_plan* query) {
  SV_REQUIRE(dz && x && gamma && save_mean && save_rstd && dx && dgamma && dbeta && sums_ws && M > 0 && C > 0, "bn_bwd: null/empty argument");
  SV_REQUIRE(act == SV_ACT_NONE || z || signs || (fsc && fsh), "bn_bwd: the activation mask needs the forward output z, its sign words or the forward scale/shift");
  SV_REQUIRE_ACT(act_dtype);             // sums_ws: sv_bn_bwd_workspace_doubles(C) doubles, ZERO on entry (e.g. a slice of one pre-zeroed arena)
  const sv_norm_plan p = plan_bn_bwd({{dz, lddz}, {z, ldz}, {x, ldx}, {dx, lddx}, {dres, lddres}},
                                     (uintptr_t)save_mean | (uintptr_t)save_rstd | (uintptr_t)fsc | (uintptr_t)fsh, M, C, act, dres, signs, act_dtype);
  // sign words: the reduce pass takes the mask from them and hands the masked gradient on through dres (premask) - both vector-path features
  SV_REQUIRE(!signs || (p.family == SV_NORM_BN_VECTOR && bn_signs_ok(C) && dres && act != SV_ACT_NONE && ((uintptr_t)signs & 15) == 0),
             "bn_bwd_signs: needs C %% 256 == 0, 4-aligned rows, an activation and the residual-branch output dres (C=%d)", C);
  if (query) { *query = p; return SV_OK; }
  SV_DISPATCH_ACT(act_dtype,
    const AT* dz_ = static_cast<const AT*>(dz); const AT* z_ = static_cast<const AT*>(z); const AT* x_ = static_cast<const AT*>(x);
    AT* dx_ = static_cast<AT*>(dx); AT* dres_ = static_cast<AT*>(dres); const AT* none = nullptr; const unsigned long long* w = static_cast<const unsigned long long*>(signs);
    const int G = p.lanes; const long long rpb = p.rows[0], arpb = p.rows[1];
    switch (p.family) {
      case SV_NORM_BN_NARROW:
        hipLaunchKernelGGL(bn_bwd_reduce_narrow_kernel<AT>, bn_grid(p, 0), dim3(256), 0, s, dz_, lddz, z_, ldz, x_, ldx, save_mean, save_rstd, M, C, act, slope,
                           sums_ws, (int)rpb, fsc, fsh);
        bn_bwd_fold(s, C, sums_ws, dgamma, dbeta);
        hipLaunchKernelGGL(bn_bwd_apply_narrow_kernel<AT>, bn_grid(p, 2), dim3(256), 0, s, dz_, lddz, z_, ldz, x_, ldx, gamma, save_mean, save_rstd, sums_ws, M, C,
                           act, slope, training, dx_, lddx, dres_, lddres, fsc, fsh);
        break;
      case SV_NORM_BN_VECTOR:
        hipLaunchKernelGGL(bn_bwd_reduce_vec_kernel<AT>, bn_grid(p, 0), dim3(256), 0, s, dz_, lddz, z_, ldz, x_, ldx, save_mean, save_rstd, M, C, act, slope,
                           sums_ws, rpb, G, fsc, fsh, p.mask != SV_MASK_PLAIN ? dres_ : (AT*)nullptr, lddres, w);
        bn_bwd_fold(s, C, sums_ws, dgamma, dbeta);
        if (p.mask == SV_MASK_SIGN_APPLY)
          hipLaunchKernelGGL((bn_bwd_apply_cg_kernel<AT, true>), bn_grid(p, 2), dim3(256), 0, s, dz_, lddz, none, 0, x_, ldx, gamma, save_mean, save_rstd, sums_ws,
                             M, C, act, slope, training, dx_, lddx, (AT*)nullptr, 0, fsc, fsh, arpb, G, w);
        else if (p.mask == SV_MASK_PREMASK)
          hipLaunchKernelGGL(bn_bwd_apply_cg_kernel<AT>, bn_grid(p, 2), dim3(256), 0, s, (const AT*)dres_, lddres, none, 0, x_, ldx, gamma, save_mean, save_rstd,
                             sums_ws, M, C, (int)SV_ACT_NONE, 0.f, training, dx_, lddx, (AT*)nullptr, 0, fsc, fsh, arpb, G);
        else
          hipLaunchKernelGGL(bn_bwd_apply_cg_kernel<AT>, bn_grid(p, 2), dim3(256), 0, s, dz_, lddz, z_, ldz, x_, ldx, gamma, save_mean, save_rstd, sums_ws, M, C,
                             act, slope, training, dx_, lddx, dres_, lddres, fsc, fsh, arpb, G);
        break;
      default:
        hipLaunchKernelGGL(bn_bwd_reduce_kernel<AT>, bn_grid(p, 0), dim3(256), 0, s, dz_, lddz, z_, ldz, x_, ldx, save_mean, save_rstd, M, C, act, slope, sums_ws, rpb, G, fsc, fsh);
        bn_bwd_fold(s, C, sums_ws, dgamma, dbeta);
        hipLaunchKernelGGL(bn_bwd_apply_kernel<AT>, bn_grid(p, 2), dim3(256), 0, s, dz_, lddz, z_, ldz, x_, ldx, gamma, save_mean, save_rstd, sums_ws, M, C,
                           act, slope, training, dx_, lddx, dres_, lddres, fsc, fsh);
    });
  return check_launch("sv_bn_bwd");
}

extern "C" int sv_bn_bwd(const void* dz, int lddz, const void* z, int ldz, const void* x, int ldx, const float* gamma, const float* save_mean, const float* save_rstd,
                         long long M, int C, int act, float slope, int training, void* dx, int lddx, void* dres, int lddres, float* dgamma, float* dbeta,
                         double* sums_ws, const float* fwd_scale, const float* fwd_shift, int act_dtype, void* stream) {
  return bn_bwd_impl(dz, lddz, z, ldz, nullptr, x, ldx, gamma, save_mean, save_rstd, M, C, act, slope, training, dx, lddx, dres, lddres, dgamma, dbeta,
                     sums_ws, fwd_scale, fwd_shift, act_dtype, (hipStream_t)stream, nullptr);
}
extern "C" int sv_bn_bwd_signs(const void* dz, int lddz, const void* signs, const void* x, int ldx, const float* gamma, const float* save_mean, const float* save_rstd,
                               long long M, int C, int act, float slope, int training, void* dx, int lddx, void* dres, int lddres, float* dgamma, float* dbeta,
                               double* sums_ws, int act_dtype, void* stream) {
  SV_REQUIRE(signs, "bn_bwd_signs: null sign buffer");
  return bn_bwd_impl(dz, lddz, nullptr, 0, signs, x, ldx, gamma, save_mean, save_rstd, M, C, act, slope, training, dx, lddx, dres, lddres, dgamma, dbeta,
                     sums_ws, nullptr, nullptr, act_dtype, (hipStream_t)stream, nullptr);
}
extern "C" int sv_bn_bwd_plan(const void* dz, int lddz, const void* z, int ldz, const void* signs, const void* x, int ldx, const float* gamma, const float* save_mean,
                              const float* save_rstd, long long M, int C, int act, float slope, int training, void* dx, int lddx, void* dres, int lddres, float* dgamma,
                              float* dbeta, double* sums_ws, const float* fwd_scale, const float* fwd_shift, int act_dtype, sv_norm_plan* plan) {
  SV_REQUIRE(plan, "bn_bwd_plan: null plan");
  return bn_bwd_impl(dz, lddz, z, ldz, signs, x, ldx, gamma, save_mean, save_rstd, M, C, act, slope, training, dx, lddx, dres, lddres, dgamma, dbeta, sums_ws,
                     fwd_scale, fwd_shift, act_dtype, nullptr, plan);
}

// ---- bn3 + the down-sampling BatchNorm of a ResNet layer's first bottleneck in the same passes (kernels above).  Vector geometry only:
// C % 256 == 0, every row stride a multiple of 4, 4-element aligned tensors, train mode, ReLU; anything else is refused and stays with the
// per-layer entry points.
static bool bn_dual_ok(int act_dtype, int C, const int* lds, int nld, const void* a, const void* b, const void* c, const void* d = nullptr,
                       const void* e = nullptr) {
  if (!bn_signs_ok(C) || C <= 0) return false;
  for (int i = 0; i < nld; ++i) if (lds[i] % 4 != 0 || lds[i] < C) return false;
  return aligned4(act_dtype, a, b, c, d, e);
}

extern "C" int sv_scale_shift_act2_signs(const void* x3, int ldx3, const float* scale3, const float* shift3, const void* xd, int ldxd,
                                         const float* scaled, const float* shiftd, void* y, int ldy, long long M, int C, void* signs,
                                         int act_dtype, void* stream) {
  SV_REQUIRE(x3 && scale3 && shift3 && xd && scaled && shiftd && y && M > 0, "scale_shift_act2_signs: null/empty argument");
  SV_REQUIRE(signs, "scale_shift_act2_signs: null sign buffer");
  SV_REQUIRE_ACT(act_dtype);
  const int lds[3] = {ldx3, ldxd, ldy};
  SV_REQUIRE(bn_dual_ok(act_dtype, C, lds, 3, x3, xd, y) &&
             (((uintptr_t)scale3 | (uintptr_t)shift3 | (uintptr_t)scaled | (uintptr_t)shiftd | (uintptr_t)signs) & 15) == 0,
             "scale_shift_act2_signs: needs C %% 256 == 0 and 4-aligned rows (C=%d)", C);
  const int cg = C / 256;
  const long long rpb = bn_rows_per_block(M, cg, 4096, 16);
  SV_DISPATCH_ACT(act_dtype, hipLaunchKernelGGL(scale_shift_act2_cg_kernel<AT>, dim3(cg, cdiv(M, rpb)), dim3(256), 0, (hipStream_t)stream,
                                                static_cast<const AT*>(x3), ldx3, scale3, shift3, static_cast<const AT*>(xd), ldxd, scaled, shiftd,
                                                static_cast<AT*>(y), ldy, M, C, rpb, static_cast<unsigned long long*>(signs)););
  return check_launch("sv_scale_shift_act2_signs");
}

extern "C" int sv_bn_bwd2_signs(const void* dz, int lddz, const void* signs, const void* x3, int ldx3, const float* gamma3, const float* save_mean3,
                                const float* save_rstd3, const void* xd, int ldxd, const float* gammad, const float* save_meand,
                                const float* save_rstdd, long long M, int C, void* dx3, int lddx3, void* dxd, int lddxd, float* dgamma3,
                                float* dbeta3, float* dgammad, float* dbetad, double* sums_ws3, double* sums_wsd, int act_dtype, void* stream) {
  SV_REQUIRE(dz && x3 && gamma3 && save_mean3 && save_rstd3 && xd && gammad && save_meand && save_rstdd && dx3 && dxd && dgamma3 && dbeta3 &&
             dgammad && dbetad && sums_ws3 && sums_wsd && M > 0, "bn_bwd2_signs: null/empty argument");
  SV_REQUIRE(signs, "bn_bwd2_signs: null sign buffer");
  SV_REQUIRE_ACT(act_dtype);
  const int lds[5] = {lddz, ldx3, ldxd, lddx3, lddxd};
  SV_REQUIRE(bn_dual_ok(act_dtype, C, lds, 5, dz, x3, xd, dx3, dxd) &&
             (((uintptr_t)save_mean3 | (uintptr_t)save_rstd3 | (uintptr_t)save_meand | (uintptr_t)save_rstdd | (uintptr_t)signs) & 15) == 0,
             "bn_bwd2_signs: needs C %% 256 == 0 and 4-aligned rows (C=%d)", C);
  hipStream_t s = (hipStream_t)stream;
  const int cg = C / 256;
  const long long rpb = bn_rows_per_block(M, cg, 2048, 8), arpb = bn_rows_per_block(M, cg, 4096, 16);
  const unsigned long long* w = static_cast<const unsigned long long*>(signs);
  SV_DISPATCH_ACT(act_dtype,
    const AT* dz_ = static_cast<const AT*>(dz); const AT* x3_ = static_cast<const AT*>(x3); const AT* xd_ = static_cast<const AT*>(xd);
    hipLaunchKernelGGL(bn_bwd2_reduce_kernel<AT>, dim3(cg, cdiv(M, rpb)), dim3(256), 0, s, dz_, lddz, w, x3_, ldx3, save_mean3, save_rstd3, xd_, ldxd,
                       save_meand, save_rstdd, M, C, sums_ws3, sums_wsd, rpb);
    bn_bwd_fold(s, C, sums_ws3, dgamma3, dbeta3, sums_wsd, dgammad, dbetad);
    hipLaunchKernelGGL(bn_bwd2_apply_kernel<AT>, dim3(cg, cdiv(M, arpb)), dim3(256), 0, s, dz_, lddz, w, x3_, ldx3, gamma3, save_mean3, save_rstd3, xd_, ldxd,
                       gammad, save_meand, save_rstdd, sums_ws3, sums_wsd, M, C, static_cast<AT*>(dx3), lddx3, static_cast<AT*>(dxd), lddxd, arpb););
  return check_launch("sv_bn_bwd2_signs");
}
