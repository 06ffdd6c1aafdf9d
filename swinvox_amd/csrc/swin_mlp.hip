// Fused Swin MLP branch for gfx950:  x2 = x1 + s * fc2(GELU(fc1(LayerNorm(x1))))   (timm Mlp + norm2 + DropPath behind
// reference models/swin_transformer.py:78), forward, data gradient and weight gradients, with NO hidden activation in HBM.
//
// Unfused, a stage-0 block moves 7.5 GB per step for this branch (the 4C-wide hidden tensor is written twice in the forward -
// pre-activation and GELU output - and read / written four more times in the backward) through kernels that are bound by the
// HBM write stream.  Here the hidden tile never leaves the CU:
//   swin_mlp_fwd_kernel   one wave owns 32 tokens.  H^T chunk [32 hidden x 32 tokens] = W1 chunk . LN(x)^T on MFMA 32x32x16, bias +
//                         GELU on the accumulator, and the accumulator is fed straight back as the B operand of the second product
//                         Y^T += W2 chunk . H^T (an accumulator tile is a valid B fragment when the other operand's k order is permuted to
//                         match - cdna_hip_programming.md "An accumulator tile as the next MFMA's operand").  Weight chunks stream from L2
//                         through a double-buffered LDS ring in FRAGMENT ORDER (sv_swin_mlp_pack), so every A fragment is one
//                         conflict-free ds_read_b128.  Reads x1, writes x2: 4 bytes per element instead of 26.
//   swin_mlp_bwd_kernel   same skeleton, recomputes LN and the pre-activation, dH^T = (W2^T chunk . dy^T) * GELU'(hpre), dLN^T += W1^T chunk . dH^T,
//                         then the LayerNorm backward and the residual add on the accumulator; dgamma / dbeta by DPP row reductions.
//   swin_mlp_wgrad_kernel a workgroup owns a slice of the hidden units (one 16/32-wide chunk per wave) and walks a range of tokens: the
//                         x / dy tiles go to LDS once per 128 tokens and serve every wave; H and dH are recomputed for the wave's chunk
//                         (MFMA 16x16x32, tokens on the accumulator rows) and contracted over the tokens with the transposed tiles read by
//                         ds_read_b64_tr_b16: dW2 += dy^T . H, dW1^T += LN(x)^T . dH.  Accumulators stay in registers for the whole range.
//   swin_mlp_fwd_mx_kernel  opt-in sibling of the forward (sv_swin_mlp_fwd_mx, C = 96, 128): both products on MXFP8 operands quantised in registers,
//                         described in front of the kernel below.  The three kernels above are not touched by it.
//   swin_mlp_bwd_mx_kernel  opt-in sibling of the data gradient (sv_swin_mlp_bwd_mx, C = 96, 128): differentiates that MX forward with all three of its
//                         products on MXFP8 operands, described in front of the kernel below.
//   swin_mlp_wgrad_mx_kernel  opt-in sibling of the weight gradients (sv_swin_mlp_wgrad_mx, C = 96, 128): the unfused MX weight-gradient chain of that
//                         forward (recompute on MX rows, contraction over the tokens on MX columns), described in front of the kernel below.  Where
//                         it is off or says no, the weight gradients stay on swin_mlp_wgrad_kernel.
// bf16 storage + bf16 MFMA only (the exact-fp32 parity mode keeps the unfused chain); C = 96, 128, 192 (Swin-T stages 0-1, Swin-B stage 0).
#include "common.h"
#include "mx_frag.h"
#include <atomic>

namespace sv {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4_t;

struct MlpArgs {
  const __bf16* x1; const __bf16* dx2; __bf16* out;
  const float* ln_g; const float* ln_b; float eps;
  const __bf16* packs;                 // W1F | W2F | W2TF | W1TF, 4C*C elements each (sv_swin_mlp_pack)
  const float* b1; const float* b2;
  const float* row_scale; int rows_per_scale;
  float* dgamma; float* dbeta;
  long long M; int ntiles;
};

// ---- weight packs in MFMA fragment order ------------------------------------------------------------------------------------
// chunk = 32 hidden units.  "row-k" images (A = [32 hidden rows][k = c]):       [chunk][f = c/16][lane][8]   lane = (r, h): hid = 32 chunk + r, c = 16 f + 8 h + j
//                           "k-perm" images (A = [32 c rows][k = hidden, permuted]): [chunk][blk = c/32][s][lane][8] lane = (r, h): c = 32 blk + r,
//                           hid = 32 chunk + 16 s + 8 (j >> 2) + 4 h + (j & 3)  - the k order in which a 32x32 accumulator tile is a B fragment.
__global__ __launch_bounds__(256) void swin_mlp_pack_kernel(const float* __restrict__ w1, const float* __restrict__ w2, __bf16* __restrict__ packs, int C) {
  const int HID = 4 * C;
  const long long n = (long long)HID * C;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < 4 * n; idx += (long long)gridDim.x * 256) {
    const int img = (int)(idx / n);
    const int e = (int)(idx % n);
    const int chunk = e / (32 * C), rem = e % (32 * C);
    const int lane = (rem % 512) / 8, j = rem % 8, r = lane & 31, h = lane >> 5;
    float v;
    if (img == 0 || img == 2) {
      const int f = rem / 512;
      const int hid = 32 * chunk + r, c = 16 * f + 8 * h + j;
      v = img == 0 ? w1[(size_t)hid * C + c] : w2[(size_t)c * HID + hid];
    } else {
      const int blk = rem / 1024, s = (rem % 1024) / 512;
      const int c = 32 * blk + r, hid = 32 * chunk + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3);
      v = img == 1 ? w2[(size_t)c * HID + hid] : w1[(size_t)hid * C + c];
    }
    packs[idx] = (__bf16)v;
  }
}

// GELU and its derivative for the bf16 path: Phi(x) = logistic(x (c0 + c1 x^2 + c2 x^4)) (odd quintic in the logit, minimax-fitted to the
// normal CDF over |x| <= 8; x^2 is clamped at 64, where the logistic has saturated to 1 - 7e-13).  |x Phi(x) - GELU_erf(x)| <= 2.9e-5 and
// |d/dx - GELU_erf'(x)| <= 1.1e-4 everywhere: 1/30 of the bf16 rounding unit of the values that are stored or fed to the matrix pipe.  Cost:
// 6 VALU + v_exp_f32 + v_rcp_f32 against 16 + 2 for erf by Abramowitz-Stegun 7.1.26 - with 16 activations per lane behind every 12 MFMAs
// (C = 96) the GELU stream, not the matrix pipe, paced these kernels (probe: forward 0.36 ms with A&S, 0.22 ms with GELU compiled out).
// The exact-fp32 parity mode never comes here (erff in the unfused chain).
__device__ __forceinline__ f32x2 gelu_pair(f32x2 x) {
#if defined(SV_PROBE_NOGELU)
  return x;
#else
  return gelu_fast2(x);
#endif
}
__device__ __forceinline__ void gelu_both_pair(f32x2 x, f32x2& g, f32x2& dg) {
#if defined(SV_PROBE_NOGELU)
  g = x; dg = (f32x2)(1.f); return;
#else
  gelu_both_fast2(x, g, dg);
#endif
}
__device__ __forceinline__ float gelu_fwd(float x) {
#if defined(SV_PROBE_NOGELU)   // measurement probe only (never built into the library)
  return x;
#else
  const float x2 = fminf(x * x, 64.f);
  const float p = fmaf(x2, fmaf(x2, 9.975397e-04f, -1.0665937e-01f), -2.3012706e+00f);    // -log2(e) * (c0 + c1 x^2 + c2 x^4)
  return x * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(x * p));
#endif
}
__device__ __forceinline__ void gelu_both(float x, float& g, float& dg) {
#if defined(SV_PROBE_NOGELU)
  g = x; dg = 1.f; return;
#endif
  const float x2 = fminf(x * x, 64.f);
  const float p = fmaf(x2, fmaf(x2, 9.975397e-04f, -1.0665937e-01f), -2.3012706e+00f);
  const float s = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(x * p));
  const float qd = fmaf(x2, fmaf(x2, -3.45720919e-03f, 2.21791923e-01f), 1.59511919f);     // d/dx [x (c0 + c1 x^2 + c2 x^4)]
  g = x * s;
  dg = s * fmaf(x * (1.f - s), qd, 1.f);
}

__device__ __forceinline__ bf16x8 pack8(const f32x16& a, int s) {   // registers 8s .. 8s+7 -> one bf16 fragment
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (__bf16)a[8 * s + j];
  return r;
}

// sum over the 32 lanes of each wave half (lanes 0-31 -> lane 31, lanes 32-63 -> lane 63) on the VALU (DPP row shifts + row broadcast)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_shift(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, true));
}
__device__ __forceinline__ float half_wave_total(float v) {
  v += dpp_shift<0x111, 0xf>(v);   // row_shr:1
  v += dpp_shift<0x112, 0xf>(v);   // row_shr:2
  v += dpp_shift<0x114, 0xf>(v);   // row_shr:4
  v += dpp_shift<0x118, 0xf>(v);   // row_shr:8  -> lane 15 of every 16-lane row holds the row total
  v += dpp_shift<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3 -> lanes 31 / 63 hold the totals of lanes 0-31 / 32-63
  return v;
}

// One 64-hidden-unit weight stage (NIMG images, 64 C elements each) HBM/L2 -> LDS by LDS-DMA (global_load_lds_dwordx4): a wave
// instruction moves 1 KB, lane l's 16 bytes landing at (wave-uniform LDS base) + 16 l - exactly the fragment order of the packs, so
// the copy needs no staging registers and runs under the MFMAs of the previous stage.  Completion: the vmcnt(0) that
// __syncthreads() carries while a DMA is in flight.
typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
template <int C, int NW, int NIMG>
__device__ __forceinline__ void stage_dma(const __bf16* const (&img)[NIMG], int pair, __bf16* stage, int wave, int lane) {
  constexpr int PIECES = NIMG * 8 * C / 64;          // 1-KB pieces per stage (8 C / 64 per image)
#pragma unroll
  for (int pc = wave; pc < PIECES; pc += NW) {
    const int im = pc / (8 * C / 64), o = pc % (8 * C / 64);
    const __bf16* src = img[im] + (size_t)pair * 64 * C + o * 512 + lane * 8;
    __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(stage + (size_t)pc * 512), 16, 0, 0);
  }
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
// Workgroups of 4 waves (128 tokens), two per CU: the two run out of phase, so one's prologue (HBM latency of its rows, LayerNorm)
// and store tail hide under the other's MFMA / GELU loop; with one 8-wave workgroup per CU every wave sat in the same phase.
template <int C, int NW, int WPS>
__global__ __launch_bounds__(NW * 64, WPS) void swin_mlp_fwd_kernel(const MlpArgs p) {
  constexpr int NF = C / 16, NB = C / 32, HID = 4 * C, NPAIR = HID / 64, NT = NW * 64;
  constexpr int STAGE = 2 * 64 * C;                      // bf16 elements: W1F pair | W2F pair
  // ONE shared object: with a second one beside the LDS-DMA ring hipcc puts s_waitcnt vmcnt(0) in front of the first ds_read of every
  // stage (it must assume the read aliases the DMA in flight) and the copy no longer runs under the MFMAs (cdna_hip_programming.md 5)
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE * 2 + HID * 4];
  __bf16* wbuf = reinterpret_cast<__bf16*>(smem);
  float* sb1 = reinterpret_cast<float*>(smem + 2 * STAGE * 2);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const long long HC = (long long)HID * C;
  const __bf16* const imgs[2] = {p.packs, p.packs + HC};
  for (int i = tid; i < HID; i += NT) sb1[i] = p.b1[i];

  const long long tok = (long long)blockIdx.x * (NW * 32) + wave * 32 + r;
  const bool valid = tok < p.M;
  // ---- LayerNorm of the wave's 32 token rows, straight into the B fragments of the first product (lane (r, h): 8 consecutive channels)
  bf16x8 xn[NF];
  {
    float xv[NF][8];
    float s = 0.f;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      bf16x8 raw = VecN<__bf16, 8>::zero();
      if (valid) raw = *reinterpret_cast<const bf16x8*>(p.x1 + tok * C + 16 * f + 8 * h);
#pragma unroll
      for (int j = 0; j < 8; ++j) { xv[f][j] = (float)raw[j]; s += xv[f][j]; }
    }
    s = lane_step_add<32>(s);
    const float mean = s * (1.f / C);
    float q = 0.f;
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float d = xv[f][j] - mean; q += d * d; }
    q = lane_step_add<32>(q);
    const float rstd = rsqrtf(q * (1.f / C) + p.eps);
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int c0 = 16 * f + 8 * h;
      const float4 g0 = *reinterpret_cast<const float4*>(p.ln_g + c0), g1 = *reinterpret_cast<const float4*>(p.ln_g + c0 + 4);
      const float4 b0 = *reinterpret_cast<const float4*>(p.ln_b + c0), b1v = *reinterpret_cast<const float4*>(p.ln_b + c0 + 4);
      const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
      const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1v.x, b1v.y, b1v.z, b1v.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) xn[f][j] = (__bf16)((xv[f][j] - mean) * rstd * gg[j] + bb[j]);
    }
  }

  f32x16 acc2[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc2[b][i] = 0.f;

  stage_dma<C, NW, 2>(imgs, 0, wbuf, wave, lane);
#pragma unroll 1
  for (int pr = 0; pr < NPAIR; ++pr) {
    const __bf16* st = wbuf + (pr & 1) * STAGE;
#ifndef SV_PROBE_NODMA
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's pieces of stage pr have landed ...
    __syncthreads();                                     // ... and everybody's; everybody is done with the other buffer
    if (pr + 1 < NPAIR) stage_dma<C, NW, 2>(imgs, pr + 1, wbuf + ((pr + 1) & 1) * STAGE, wave, lane);   // lands under the MFMAs below
#endif
    // the two 32-unit sub-chunks of the stage run interleaved: two independent accumulator chains keep the matrix pipe issuing
    f32x16 acc1[2];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc1[sub][i] = 0.f;
    // every A fragment of the first product is requested before the first MFMA (ds_read latency ~ 4 MFMAs: fetched two at a time in
    // front of their MFMA the matrix pipe idles); the fragments of the second product are requested in front of the GELU block
    bf16x8 wa[2][NF];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) wa[sub][f] = *reinterpret_cast<const bf16x8*>(st + sub * 32 * C + f * 512 + lane * 8);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
        acc1[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa[sub][f], xn[f], acc1[sub], 0, 0, 0);   // H^T chunk: rows = hidden, columns = tokens
    bf16x8 wb[2][2][NB];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int b = 0; b < NB; ++b) wb[sub][s2][b] = *reinterpret_cast<const bf16x8*>(st + 64 * C + sub * 32 * C + (b * 2 + s2) * 512 + lane * 8);
    __builtin_amdgcn_sched_barrier(0);
    bf16x8 hb[2][2];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const int hid0 = (2 * pr + sub) * 32;
#pragma unroll
      for (int i = 0; i < 16; i += 2) {      // pairs: packed fp32 math (common.h gelu_fast2)
        const int hb = hid0 + (i & 3) + 8 * (i >> 2) + 4 * h;
        const f32x2 gl = gelu_pair((f32x2){acc1[sub][i] + sb1[hb], acc1[sub][i + 1] + sb1[hb + 1]});
        acc1[sub][i] = gl[0]; acc1[sub][i + 1] = gl[1];
      }
      hb[sub][0] = pack8(acc1[sub], 0); hb[sub][1] = pack8(acc1[sub], 1);
    }
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int b = 0; b < NB; ++b)
          acc2[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wb[sub][s2][b], hb[sub][s2], acc2[b], 0, 0, 0);   // Y^T: rows = output channels, columns = tokens
  }
  // ---- epilogue: + bias, drop-path scale, + residual; lane (r, h) owns channels 32 b + 8 g + 4 h .. + 3 of token r
  if (valid) {
    const float sc = p.row_scale ? p.row_scale[tok / p.rows_per_scale] : 1.f;
    bf16x4 resv[NB][4];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int g = 0; g < 4; ++g) resv[b][g] = *reinterpret_cast<const bf16x4*>(p.x1 + tok * C + 32 * b + 8 * g + 4 * h);   // all in flight at once
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c0 = 32 * b + 8 * g + 4 * h;
        const float4 bi = *reinterpret_cast<const float4*>(p.b2 + c0);
        const bf16x4 res = resv[b][g];
        bf16x4 o;
        o[0] = (__bf16)((float)res[0] + sc * (acc2[b][4 * g + 0] + bi.x));
        o[1] = (__bf16)((float)res[1] + sc * (acc2[b][4 * g + 1] + bi.y));
        o[2] = (__bf16)((float)res[2] + sc * (acc2[b][4 * g + 2] + bi.z));
        o[3] = (__bf16)((float)res[3] + sc * (acc2[b][4 * g + 3] + bi.w));
#ifdef SV_PROBE_NOSTORE
        if (o[0] == (__bf16)123.f) *reinterpret_cast<bf16x4*>(p.out + tok * C + c0) = o;
#else
        *reinterpret_cast<bf16x4*>(p.out + tok * C + c0) = o;
#endif
      }
  }
}

// ---- data gradient ------------------------------------------------------------------------------------------------------
// dx1 = dx2 + LayerNormBackward( (s * dx2 . W2) * GELU'(hpre) . W1 ),  dgamma / dbeta of the LayerNorm accumulated per workgroup
template <int C, int NW, int WPS>
__global__ __launch_bounds__(NW * 64, WPS) void swin_mlp_bwd_kernel(const MlpArgs p) {
  constexpr int NF = C / 16, NB = C / 32, HID = 4 * C, NPAIR = HID / 64, NT = NW * 64;
  constexpr int STAGE = 3 * 64 * C;                      // W1F pair | W2TF pair | W1TF pair
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE * 2 + (HID + 4 * C) * 4];   // one object (see the forward kernel)
  __bf16* wbuf = reinterpret_cast<__bf16*>(smem);
  float* sb1 = reinterpret_cast<float*>(smem + 2 * STAGE * 2);
  float* sdg = sb1 + HID;
  float* sdb = sdg + C;
  // LayerNorm parameters from LDS: read from global memory they are invariant over the persistent tile loop, hipcc hoists all 3 C / 2
  // per-lane values out of it and spills them around the main loop
  float* sgam = sdb + C;
  float* sbet = sgam + C;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const long long HC = (long long)HID * C;
  const __bf16* const imgs[3] = {p.packs, p.packs + 2 * HC, p.packs + 3 * HC};
  for (int i = tid; i < HID; i += NT) sb1[i] = p.b1[i];
  for (int i = tid; i < C; i += NT) { sdg[i] = 0.f; sdb[i] = 0.f; sgam[i] = p.ln_g[i]; sbet[i] = p.ln_b[i]; }
  __syncthreads();

  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    const long long tok = (long long)tile * (NW * 32) + wave * 32 + r;
    const bool valid = tok < p.M;
    const float sc = (valid && p.row_scale) ? p.row_scale[tok / p.rows_per_scale] : 1.f;
    bf16x8 xn[NF], dyb[NF];
    float mean, rstd;
    {
      float xv[NF][8];
      float s = 0.f;
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        bf16x8 raw = VecN<__bf16, 8>::zero(), dr = VecN<__bf16, 8>::zero();
        if (valid) {
          raw = *reinterpret_cast<const bf16x8*>(p.x1 + tok * C + 16 * f + 8 * h);
          dr = *reinterpret_cast<const bf16x8*>(p.dx2 + tok * C + 16 * f + 8 * h);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) { xv[f][j] = (float)raw[j]; s += xv[f][j]; dyb[f][j] = (__bf16)(sc * (float)dr[j]); }
      }
      s = lane_step_add<32>(s);
      mean = s * (1.f / C);
      float q = 0.f;
#pragma unroll
      for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float d = xv[f][j] - mean; q += d * d; }
      q = lane_step_add<32>(q);
      rstd = rsqrtf(q * (1.f / C) + p.eps);
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const int c0 = 16 * f + 8 * h;
        const float4 g0 = *reinterpret_cast<const float4*>(sgam + c0), g1 = *reinterpret_cast<const float4*>(sgam + c0 + 4);
        const float4 b0 = *reinterpret_cast<const float4*>(sbet + c0), b1v = *reinterpret_cast<const float4*>(sbet + c0 + 4);
        const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
        const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1v.x, b1v.y, b1v.z, b1v.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) xn[f][j] = (__bf16)((xv[f][j] - mean) * rstd * gg[j] + bb[j]);
      }
    }
    f32x16 acc3[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc3[b][i] = 0.f;

    __syncthreads();                                     // previous tile: every wave has left its last stage
    stage_dma<C, NW, 3>(imgs, 0, wbuf, wave, lane);
#pragma unroll 1
    for (int pr = 0; pr < NPAIR; ++pr) {
      const __bf16* st = wbuf + (pr & 1) * STAGE;
#ifndef SV_PROBE_NODMA
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (pr + 1 < NPAIR) stage_dma<C, NW, 3>(imgs, pr + 1, wbuf + ((pr + 1) & 1) * STAGE, wave, lane);
#endif
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        f32x16 acc1, accd;                               // two independent chains (pre-activation, dy . W2) interleave on the matrix pipe
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc1[i] = 0.f; accd[i] = 0.f; }
        const __bf16* w1f = st + sub * 32 * C;
        const __bf16* w2tf = st + 64 * C + sub * 32 * C;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(w1f + f * 512 + lane * 8);
          const bf16x8 at = *reinterpret_cast<const bf16x8*>(w2tf + f * 512 + lane * 8);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, xn[f], acc1, 0, 0, 0);     // pre-activation^T (recomputed)
          accd = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at, dyb[f], accd, 0, 0, 0);   // (dy . W2)^T
        }
        const int hid0 = (2 * pr + sub) * 32;
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
          const int hb = hid0 + (i & 3) + 8 * (i >> 2) + 4 * h;
          f32x2 g, dg;
          gelu_both_pair((f32x2){acc1[i] + sb1[hb], acc1[i + 1] + sb1[hb + 1]}, g, dg);
          accd[i] *= dg[0]; accd[i + 1] *= dg[1];
        }
        const bf16x8 d0 = pack8(accd, 0), d1 = pack8(accd, 1);
        __builtin_amdgcn_sched_barrier(0);               // do not hoist the next fragments above the GELU block (register pressure)
        const __bf16* w1tf = st + 128 * C + sub * 32 * C;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(w1tf + (b * 2 + 0) * 512 + lane * 8);
          acc3[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, d0, acc3[b], 0, 0, 0);  // dLN^T: rows = channels, columns = tokens
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(w1tf + (b * 2 + 1) * 512 + lane * 8);
          acc3[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, d1, acc3[b], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // ---- LayerNorm backward on the accumulator (lane (r, h): channels 32 b + 8 g + 4 h + k of token r)
    // lane offset laundered per tile: otherwise hipcc materialises all 3 C / 2 per-lane LDS addresses of the epilogue once, outside the
    // tile loop, and spills them around the main loop; with an opaque base they stay immediate offsets of the ds instructions
    int lane_off = 4 * h;
    asm volatile("" : "+v"(lane_off));
    float* const lg_ = sgam + lane_off;
    float* const ldg_ = sdg + lane_off;
    float* const ldb_ = sdb + lane_off;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c0 = 32 * b + 8 * g + 4 * h;
        bf16x4 xr = V4<__bf16>::zero();
        if (valid) xr = *reinterpret_cast<const bf16x4*>(p.x1 + tok * C + c0);
        const float4 gm = *reinterpret_cast<const float4*>(lg_ + 32 * b + 8 * g);
        const float gv[4] = {gm.x, gm.y, gm.z, gm.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float xh = valid ? ((float)xr[k] - mean) * rstd : 0.f;
          const float d = valid ? acc3[b][4 * g + k] : 0.f;
          const float gg = d * gv[k];
          s1 += gg; s2 += gg * xh;
          // dgamma / dbeta: totals over the 32 tokens of this lane half arrive in lanes 31 and 63
#ifdef SV_PROBE_NODPP
          const float tb = d, tg = d * xh;
#else
          const float tb = half_wave_total(d), tg = half_wave_total(d * xh);
#endif
          if (r == 31) { atomicAdd(ldb_ + 32 * b + 8 * g + k, tb); atomicAdd(ldg_ + 32 * b + 8 * g + k, tg); }
        }
        __builtin_amdgcn_sched_barrier(0);   // keep the 8 reduction chains of one channel group together (interleaving all 96 spills)
      }
    s1 = lane_step_add<32>(s1);
    s2 = lane_step_add<32>(s2);
    s1 *= (1.f / C); s2 *= (1.f / C);
    if (valid) {
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int c0 = 32 * b + 8 * g + 4 * h;
          const bf16x4 xr = *reinterpret_cast<const bf16x4*>(p.x1 + tok * C + c0);
          const bf16x4 dr = *reinterpret_cast<const bf16x4*>(p.dx2 + tok * C + c0);
          const float4 gm = *reinterpret_cast<const float4*>(lg_ + 32 * b + 8 * g);
          const float gv[4] = {gm.x, gm.y, gm.z, gm.w};
          bf16x4 o;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float xh = ((float)xr[k] - mean) * rstd;
            o[k] = (__bf16)((float)dr[k] + rstd * (acc3[b][4 * g + k] * gv[k] - s1 - xh * s2));
          }
          *reinterpret_cast<bf16x4*>(p.out + tok * C + c0) = o;
        }
    }
  }
  __syncthreads();
  for (int i = tid; i < C; i += NT) { atomicAdd(p.dgamma + i, sdg[i]); atomicAdd(p.dbeta + i, sdb[i]); }
}

// ---- weight gradients --------------------------------------------------------------------------------------------------------
struct MlpWArgs {
  const __bf16* x1; const __bf16* dx2;
  const float* ln_g; const float* ln_b; float eps;
  const __bf16* w1r;   // [4C][C]  fc1 weight rows (forward pack of fc1)
  const __bf16* w2tr;  // [4C][C]  fc2 weight transposed (data-gradient pack of fc2)
  const float* b1; const float* row_scale; int rows_per_scale;
  float* dw1; float* db1; float* dw2; float* db2;     // native layouts [4C][C], [4C], [C][4C], [C]
  long long M; int tok_per_split; int HG;
};

// Tiles: TT token rows of x1 and dx2 per step, DOUBLE-BUFFERED in LDS and filled by LDS-DMA while the previous tile is being
// contracted.  A row record is the C/8 16-byte units of the row plus one pad unit (row stride = 8 banks mod 64: the fragment reads
// below are conflict-free); one DMA instruction moves 64 / (C/8 + 1) whole records (the pad unit re-reads the row's last unit), so
// the records stay contiguous as LDS-DMA requires.  LayerNorm (4 lanes per row) and the drop-path scale of dy then run in place.
template <int C, int NW, int HCW, int TT>
__global__ __launch_bounds__(NW * 64, (NW + 3) / 4) void swin_mlp_wgrad_kernel(const MlpWArgs p) {
  constexpr int NF = C / 32, NCB = C / 16, NHB = HCW / 16, HID = 4 * C, NT = NW * 64;
  constexpr int UPR = C / 8, RU = UPR + 1, LD = RU * 8, RPI = 64 / RU, NGRP = (TT + RPI - 1) / RPI, TILE = TT * LD;
  // ONE shared object (see the forward kernel), and no ordinary global load inside the token loop: hipcc would drain the DMA of the next
  // tile in front of its first use - LayerNorm parameters sit in LDS, the drop-path factors of a tile are fetched before its DMA wait
  __shared__ __attribute__((aligned(16))) char smem_raw[4 * TILE * 2 + 2 * C * 4];
  __bf16* smem = reinterpret_cast<__bf16*>(smem_raw);            // [buffer][x | dy][TT][LD]
  float* sgam = reinterpret_cast<float*>(smem_raw + 4 * TILE * 2);
  float* sbet = sgam + C;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4, q = lr >> 2, pp = lr & 3;
  for (int i = tid; i < C; i += NT) { sgam[i] = p.ln_g[i]; sbet[i] = p.ln_b[i]; }
  const int hg = blockIdx.x % p.HG, split = blockIdx.x / p.HG;
  const int h0 = (hg * NW + wave) * HCW;                         // first hidden unit of this wave
  const long long t_begin = (long long)split * p.tok_per_split;
  long long t_end = t_begin + p.tok_per_split;
  if (t_end > p.M) t_end = p.M;

  auto tile_dma = [&](long long t0, int buf) {
    const int rr = lane / RU, uu = lane % RU;
#pragma unroll 1
    for (int g = wave; g < NGRP; g += NW) {
      const int row = g * RPI + rr;
      if (rr < RPI && row < TT) {
        long long tok = t0 + row;
        if (tok >= t_end) tok = t_end - 1;                       // rows past the end are zeroed by the LayerNorm pass
        const size_t off = (size_t)tok * C + (uu < UPR ? uu : UPR - 1) * 8;
        __bf16* dst = smem + (size_t)(2 * buf) * TILE + (size_t)g * RPI * LD;
        __builtin_amdgcn_global_load_lds((gptr_t)(p.x1 + off), (lptr_t)dst, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gptr_t)(p.dx2 + off), (lptr_t)(dst + TILE), 16, 0, 0);
      }
    }
  };

  // per-wave constant B fragments: W1 rows / W2^T rows of the wave's hidden units (k = channels, 8 consecutive per lane)
  bf16x8 w1b[NHB][NF], w2b[NHB][NF];
  float b1v[NHB];
#pragma unroll
  for (int hb = 0; hb < NHB; ++hb) {
    const int hid = h0 + 16 * hb + lr;
    b1v[hb] = p.b1[hid];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      w1b[hb][f] = *reinterpret_cast<const bf16x8*>(p.w1r + (size_t)hid * C + 32 * f + 8 * lg);
      w2b[hb][f] = *reinterpret_cast<const bf16x8*>(p.w2tr + (size_t)hid * C + 32 * f + 8 * lg);
    }
  }
  f32x4 G2[NCB][NHB], G1[NCB][NHB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
    for (int hb = 0; hb < NHB; ++hb) { G2[cb][hb] = (f32x4){0.f, 0.f, 0.f, 0.f}; G1[cb][hb] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
  float db1acc[NHB];
#pragma unroll
  for (int hb = 0; hb < NHB; ++hb) db1acc[hb] = 0.f;
  float db2acc = 0.f;

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // the fragment loads above are ordinary loads: retire them before any DMA
  tile_dma(t_begin, 0);
  int buf = 0;
#pragma unroll 1
  for (long long t0 = t_begin; t0 < t_end; t0 += TT, buf ^= 1) {
    __bf16* xs = smem + (size_t)(2 * buf) * TILE;
    __bf16* ds = xs + TILE;
    // drop-path factors of this tile: it spans at most two images (rows_per_scale >= TT is checked on the host)
    float sc_lo = 1.f, sc_hi = 1.f;
    long long t_img = t_end;                                     // first token of the second image inside the tile
    if (p.row_scale) {
      const long long i_lo = t0 / p.rows_per_scale;
      long long t_last = t0 + TT - 1; if (t_last >= t_end) t_last = t_end - 1;
      sc_lo = p.row_scale[i_lo]; sc_hi = p.row_scale[t_last / p.rows_per_scale];
      t_img = (i_lo + 1) * (long long)p.rows_per_scale;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // this wave's records of tile t0 have landed ...
    __syncthreads();                                             // ... and everybody's; the other buffer has been consumed
    // ---- in place: LayerNorm of x1 rows (4 lanes per row), drop-path scale of dy rows, zero rows past the end
    for (int row = tid >> 2; row < TT; row += NT / 4) {
      const int part = tid & 3;
      const bool live = t0 + row < t_end;
      __bf16* xr = xs + row * LD + part * (C / 4);
      __bf16* dr = ds + row * LD + part * (C / 4);
      bf16x8 v[C / 32];
      float s1 = 0.f;
#pragma unroll
      for (int u = 0; u < C / 32; ++u) {
        v[u] = *reinterpret_cast<const bf16x8*>(xr + 8 * u);
#pragma unroll
        for (int j = 0; j < 8; ++j) s1 += (float)v[u][j];
      }
      s1 += dpp_move<0xB1>(s1); s1 += dpp_move<0x4E>(s1);
      const float mean = s1 * (1.f / C);
      float s2 = 0.f;
#pragma unroll
      for (int u = 0; u < C / 32; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float d = (float)v[u][j] - mean; s2 += d * d; }
      s2 += dpp_move<0xB1>(s2); s2 += dpp_move<0x4E>(s2);
      const float rstd = rsqrtf(s2 * (1.f / C) + p.eps);
      const float sc = t0 + row < t_img ? sc_lo : sc_hi;
#pragma unroll
      for (int u = 0; u < C / 32; ++u) {
        const int c0 = part * (C / 4) + 8 * u;
        const float4 g0 = *reinterpret_cast<const float4*>(sgam + c0), g1 = *reinterpret_cast<const float4*>(sgam + c0 + 4);
        const float4 b0 = *reinterpret_cast<const float4*>(sbet + c0), b1q = *reinterpret_cast<const float4*>(sbet + c0 + 4);
        const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
        const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1q.x, b1q.y, b1q.z, b1q.w};
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = live ? (__bf16)(((float)v[u][j] - mean) * rstd * gg[j] + bb[j]) : (__bf16)0.f;
        *reinterpret_cast<bf16x8*>(xr + 8 * u) = o;
        if (!live || p.row_scale) {
          bf16x8 d = *reinterpret_cast<const bf16x8*>(dr + 8 * u);
#pragma unroll
          for (int j = 0; j < 8; ++j) d[j] = live ? (__bf16)(sc * (float)d[j]) : (__bf16)0.f;
          *reinterpret_cast<bf16x8*>(dr + 8 * u) = d;
        }
      }
    }
    __syncthreads();
    if (t0 + TT < t_end) tile_dma(t0 + TT, buf ^ 1);             // the next tile lands under the contraction below
    if (hg == 0 && tid < C) {                                    // bias gradient of fc2: column sums of the (scaled) dy tile
      float s = 0.f;
#pragma unroll 8
      for (int row = 0; row < TT; ++row) s += (float)ds[row * LD + tid];
      db2acc += s;
    }
    // ---- the wave's hidden chunk against the 32-token sub-tiles
#pragma unroll 1
    for (int sub = 0; sub < TT / 32; ++sub) {
      f32x4 Hh[2][NHB], Dh[2][NHB];
#pragma unroll
      for (int tb = 0; tb < 2; ++tb) {
        bf16x8 xa[NF], da[NF];
        const int row = 32 * sub + 16 * tb + lr;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          xa[f] = *reinterpret_cast<const bf16x8*>(xs + row * LD + 32 * f + 8 * lg);
          da[f] = *reinterpret_cast<const bf16x8*>(ds + row * LD + 32 * f + 8 * lg);
        }
#pragma unroll
        for (int hb = 0; hb < NHB; ++hb) {
          f32x4 a = (f32x4){0.f, 0.f, 0.f, 0.f}, d = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int f = 0; f < NF; ++f) {
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[f], w1b[hb][f], a, 0, 0, 0);   // rows = tokens, columns = hidden units
            d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da[f], w2b[hb][f], d, 0, 0, 0);
          }
#pragma unroll
          for (int i = 0; i < 4; i += 2) {
            f32x2 g, dg;
            gelu_both_pair((f32x2){a[i] + b1v[hb], a[i + 1] + b1v[hb]}, g, dg);
            a[i] = g[0]; a[i + 1] = g[1];
            d[i] *= dg[0]; d[i + 1] *= dg[1];
            db1acc[hb] += d[i] + d[i + 1];
          }
          Hh[tb][hb] = a; Dh[tb][hb] = d;
        }
      }
      // B fragments of the token contraction: the stacked accumulator blocks (k order {4 lg + i} U {16 + 4 lg + i})
      bf16x8 hB[NHB], dB[NHB];
#pragma unroll
      for (int hb = 0; hb < NHB; ++hb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          hB[hb][i] = (__bf16)Hh[0][hb][i]; hB[hb][4 + i] = (__bf16)Hh[1][hb][i];
          dB[hb][i] = (__bf16)Dh[0][hb][i]; dB[hb][4 + i] = (__bf16)Dh[1][hb][i];
        }
      // A fragments: transposed tiles (rows = channels, k = tokens in the same order) by ds_read_b64_tr_b16
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        const __bf16* sx = xs + (32 * sub + 4 * lg + q) * LD + 16 * cb + 4 * pp;
        const __bf16* sd = ds + (32 * sub + 4 * lg + q) * LD + 16 * cb + 4 * pp;
        const bf16x4 xlo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_t*)(sx));
        const bf16x4 xhi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_t*)(sx + 16 * LD));
        const bf16x4 dlo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_t*)(sd));
        const bf16x4 dhi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_t*)(sd + 16 * LD));
        const bf16x8 xT = __builtin_shufflevector(xlo, xhi, 0, 1, 2, 3, 4, 5, 6, 7);
        const bf16x8 dT = __builtin_shufflevector(dlo, dhi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
        for (int hb = 0; hb < NHB; ++hb) {
          G2[cb][hb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dT, hB[hb], G2[cb][hb], 0, 0, 0);   // dW2[c][hid]
          G1[cb][hb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xT, dB[hb], G1[cb][hb], 0, 0, 0);   // dW1[hid][c], held transposed
        }
      }
    }
  }
  // ---- write out (accumulator: row = channel 16 cb + 4 lg + i, column = hidden unit h0 + 16 hb + lr)
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
    for (int hb = 0; hb < NHB; ++hb)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = 16 * cb + 4 * lg + i, hid = h0 + 16 * hb + lr;
        atomicAdd(p.dw2 + (size_t)c * HID + hid, G2[cb][hb][i]);
        atomicAdd(p.dw1 + (size_t)hid * C + c, G1[cb][hb][i]);
      }
#pragma unroll
  for (int hb = 0; hb < NHB; ++hb) {
    float v = db1acc[hb];
    v = lane_step_add<16>(v);
    v = lane_step_add<32>(v);
    if (lg == 0) atomicAdd(p.db1 + h0 + 16 * hb + lr, v);
  }
  if (hg == 0 && tid < C) atomicAdd(p.db2 + tid, db2acc);
}

static inline bool mlp_supported(int C) { return C == 96 || C == 128 || C == 192; }

// ---- MXFP8 forward (opt-in sibling of swin_mlp_fwd_kernel; sv_swin_mlp_fwd_mx) ---------------------------------------------------------
// The unfused MX chain composed in one kernel: quantising LayerNorm -> fc1 on the block-scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4, e4m3 x e4m3,
// E8M0 block scales) -> + b1, fast GELU, bf16 rounding, MX quantisation of h in blocks of 32 consecutive hidden units -> fc2 on the same MFMA ->
// the epilogue of swin_mlp_fwd_kernel.  Neither h nor any quantised activation reaches HBM.  NORMATIVE recipe: linear_fp8.hip "MX recipe"
// (mx_block_exp / pack4_e4m3_mx of common.h are the only copy of the rounding); the weight bytes are sv_quant_rows_mx_e4m3's.
//   tokens on the columns (B operand): lane l = (t = l & 15, lg = l >> 4) holds token t.  Its data registers 0-3 are k = 16 lg .. + 15 and 4-7 are
//   k = 64 + 16 lg .. + 15 of a 128-wide k-step, its scale byte covers k = 32 lg .. + 31 (linear_fp8.hip, lf_contract).
//   LayerNorm     lane (t, lg) loads exactly those 16 + 16 channels of its token; the row sums cross the four lane groups (two permlane exchanges).
//                 A 32-channel block is the 16 + 16 values of lanes lg and lg ^ 1 (same register half): one permlane16 exchange per maximum.
//                 C = 96: Kp = 128, the upper half of lane groups 2 and 3 is padding - zero bytes, block 3 carries byte 127.
//   fc1           A = 16 rows of W1 per MFMA, one k-step (Kp = 128).  The accumulator leaves as column t, rows 4 lg .. + 3.  Eight row tiles make the 128
//                 hidden units of ONE fc2 k-step; the pack orders W1's rows so that tile j, row r is hidden unit 64 (j >> 2) + 16 (r >> 2) + 4 (j & 3)
//                 + (r & 3) of the group: a lane's 4 x 4 values of tiles 0-3 are its data registers 0-3 of the fc2 operand (k = 16 lg .. + 15), those of
//                 tiles 4-7 its registers 4-7 - no lane movement, and a hardware block is 32 consecutive hidden units, again split over lanes
//                 lg and lg ^ 1.  The scale byte a lane must PASS (block lg) is known to lane group 2 (lg & 1): one ds_bpermute of the two packed bytes.
//   fc2           A = 16 rows of W2 (output channels 16 jc + r), k-step g = hidden units 128 g .. + 127; accumulates over the 4C / 128 groups.
//   weights       resident in LDS for the life of the workgroup, in fragment order (every A fragment is two conflict-free ds_read_b128, its scale one
//                 byte per lane); one persistent workgroup per CU walks 128-token tiles.  NW waves own NTT x 16 tokens each: the library runs
//                 8 x 1 - two waves per SIMD, so the GELU / quantiser VALU stream of one runs beside the MFMAs and LDS reads of the other.  With
//                 NTT = 2 an A fragment read serves two MFMAs, but 4 x 2 leaves one wave per SIMD and 8 x 2 is slower than 8 x 1.
// Pack image (sv_swin_mlp_mx_pack, bytes):  W1F [G][8 tiles][2 halves][64 lanes][16] | W2F [G][C/16][2][64][16] | W1S [G][8][64] | W2S [G][C/16][64],  G = 4C / 128.
// The data gradient (swin_mlp_bwd_mx_kernel) runs the same pieces through the same code: MxImages / mx_pack_hidden_rows / mx_pack_channel_rows (the two
// kinds of image and the only copy of the hidden-unit order), mx_a_frag / mx_a_scale (A fragment read), mx_layernorm (prologue), mx_quant_frag (token
// rows -> B fragment) and mx_quant_acc (accumulator tiles -> elementwise operation -> B fragment).  mx_pack_item, mx_a_frag / mx_a_scale, mx_quant_frag
// and mx_layernorm live in mx_frag.h: the fused attention branch (attn.hip, swin_attn_block_fwd_mx_kernel) runs them too.

// The two kinds of image a pack is made of, for width C (usable at compile time and, in the pack kernels and on the host, at run time).  A
// "hidden-row" image holds a [4C][128] operand (W1, W2^T) as [G][8 tiles][2][64][16] bytes + [G][8][64] scale bytes, a "channel-row" image a [C][4C]
// operand (W2, W1^T) as [G][C/16 tiles][2][64][16] + [G][C/16][64].  Either has one pack item per (tile, lane): two 16-byte pieces and one scale byte.
struct MxImages {
  int HID, G, NJ;
  int HROW_DATA, HROW_SCALES, CROW_DATA, CROW_SCALES;      // bytes; the SCALES counts are the item counts too
  constexpr explicit MxImages(int C)
      : HID(4 * C), G(HID / 128), NJ(C / 16), HROW_DATA(HID * 128), HROW_SCALES(G * 8 * 64), CROW_DATA(C * HID), CROW_SCALES(G * NJ * 64) {}
};

struct MlpMx : MxImages {                                  // the forward's pack: W1F | W2F | W1S | W2S
  int W1F, W2F, W1S, W2S, PACK_BYTES, PACK_ITEMS;
  constexpr explicit MlpMx(int C)
      : MxImages(C), W1F(0), W2F(W1F + HROW_DATA), W1S(W2F + CROW_DATA), W2S(W1S + HROW_SCALES), PACK_BYTES(W2S + CROW_SCALES),
        PACK_ITEMS(HROW_SCALES + CROW_SCALES) {}
};

// hidden-row image of q [4C][128], s [4C][4].  The ONLY copy of the hidden-unit order: tile j, row r of group g is hidden unit `hid`
__device__ __forceinline__ void mx_pack_hidden_rows(const uint8_t* q, const uint8_t* s, uint8_t* data, uint8_t* scales, int e) {
  const int lane = e & 63, j = (e >> 6) & 7, g = e >> 9, r = lane & 15, lg = lane >> 4;
  const int hid = 128 * g + 64 * (j >> 2) + 16 * (r >> 2) + 4 * (j & 3) + (r & 3);
  mx_pack_item(q + (size_t)hid * 128 + 16 * lg, s[hid * 4 + lg], data, scales, e);
}
// channel-row image of q [C][4C], s [C][4C / 32]: tile jc, row r is channel 16 jc + r, k-step g its hidden units 128 g .. + 127
__device__ __forceinline__ void mx_pack_channel_rows(const uint8_t* q, const uint8_t* s, uint8_t* data, uint8_t* scales, int e, const MxImages& I) {
  const int lane = e & 63, t = e >> 6, jc = t % I.NJ, g = t / I.NJ, r = lane & 15, lg = lane >> 4;
  const int row = 16 * jc + r;
  mx_pack_item(q + (size_t)row * I.HID + 128 * g + 16 * lg, s[row * (I.HID / 32) + 4 * g + lg], data, scales, e);
}

struct MlpMxArgs {
  const __bf16* x1; __bf16* out;
  const float* ln_g; const float* ln_b; float eps;
  const uint8_t* packs;
  const float* b1; const float* b2;
  const float* row_scale; int rows_per_scale;
  long long M; int ntiles;
};

__global__ __launch_bounds__(256) void swin_mlp_mx_pack_kernel(const uint8_t* __restrict__ w1q, const uint8_t* __restrict__ w1s, const uint8_t* __restrict__ w2q,
                                                               const uint8_t* __restrict__ w2s, uint8_t* __restrict__ packs, int C) {
  const MlpMx L(C);
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < L.HROW_SCALES) mx_pack_hidden_rows(w1q, w1s, packs + L.W1F, packs + L.W1S, idx);
  else if (idx < L.PACK_ITEMS) mx_pack_channel_rows(w2q, w2s, packs + L.W2F, packs + L.W2S, idx - L.HROW_SCALES, L);
}

// a token's eight accumulator tiles of a group (tile j = 4 hf + jj: hidden units 64 hf + 16 lg + 4 jj .. + 3) -> MX B fragment of k-step g of the next
// product + the scale byte the lane passes.  elem(j) returns tile j's four values after the elementwise operation, rounded to bf16.
template <class Elem>
__device__ __forceinline__ void mx_quant_acc(Elem elem, i32x8& q, int& sbyte, int lane) {
  int e[2];
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) {
    f32x4 v[4];
    float m = 0.f;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      v[jj] = elem(4 * hf + jj);
      m = fmaxf(fmaxf(m, fmaxf(fabsf(v[jj][0]), fabsf(v[jj][1]))), fmaxf(fabsf(v[jj][2]), fabsf(v[jj][3])));
    }
    e[hf] = mx_block_exp(pair16_max(m));
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) q[4 * hf + jj] = (int)pack4_e4m3_mx(v[jj][0], v[jj][1], v[jj][2], v[jj][3], e[hf]);
  }
  sbyte = mx_lane_scale(e[0], e[1], lane);
}

template <int C, int NW, int NTT>
__global__ __launch_bounds__(NW * 64, 1) void swin_mlp_fwd_mx_kernel(const MlpMxArgs p) {
  constexpr MlpMx L(C);
  constexpr int HID = L.HID, G = L.G, NJ = L.NJ, NT = NW * 64, TILE = NW * NTT * 16;
  __shared__ __attribute__((aligned(16))) uint8_t smem[L.PACK_BYTES + (HID + 2 * C) * 4];
  float* sb1 = reinterpret_cast<float*>(smem + L.PACK_BYTES);
  float* sgam = sb1 + HID;
  float* sbet = sgam + C;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = lane & 15, lg = lane >> 4;
  for (int i = tid; i < L.PACK_BYTES / 16; i += NT) reinterpret_cast<i32x4*>(smem)[i] = reinterpret_cast<const i32x4*>(p.packs)[i];
  for (int i = tid; i < HID; i += NT) sb1[i] = p.b1[i];
  for (int i = tid; i < C; i += NT) { sgam[i] = p.ln_g[i]; sbet[i] = p.ln_b[i]; }
  __syncthreads();

#pragma unroll 1
  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    long long tok[NTT]; bool valid[NTT];
    i32x8 xq[NTT]; int xsb[NTT];
    // ---- LayerNorm -> MX B fragments of fc1
#pragma unroll
    for (int tt = 0; tt < NTT; ++tt) {
      tok[tt] = (long long)tile * TILE + wave * (NTT * 16) + tt * 16 + t;
      valid[tt] = tok[tt] < p.M;
      float xv[2][16], mean, rstd;
      mx_layernorm<C, false>(p.x1, tok[tt], valid[tt], lg, sgam, sbet, p.eps, xv, mean, rstd);
      mx_quant_frag(xv, xq[tt], xsb[tt], lane);
    }

    f32x4 acc2[NJ][NTT];
#pragma unroll
    for (int jc = 0; jc < NJ; ++jc)
#pragma unroll
      for (int tt = 0; tt < NTT; ++tt) acc2[jc][tt] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (int g = 0; g < G; ++g) {
      // ---- fc1: the 128 hidden units of group g, as 8 row tiles in the order the fc2 operand wants
      f32x4 acc1[8][NTT];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const i32x8 a = mx_a_frag(smem + L.W1F, g * 8 + j, lane);
        const int sa = mx_a_scale(smem + L.W1S, g * 8 + j, lane);
#pragma unroll
        for (int tt = 0; tt < NTT; ++tt)
          acc1[j][tt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, xq[tt], (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0, sa, 0, xsb[tt]);
      }
      // ---- h = bf16(GELU(acc1 + b1)), MX quantisation in registers: the accumulators become the B fragment of fc2's k-step g
      i32x8 hq[NTT]; int hsb[NTT];
      const float* gb1 = sb1 + 128 * g + 16 * lg;          // the lane's biases: tile j = 4 hf + jj at + 64 hf + 4 jj
#pragma unroll
      for (int tt = 0; tt < NTT; ++tt)
        mx_quant_acc([&](int j) {
          const float4 bi = *reinterpret_cast<const float4*>(gb1 + 64 * (j >> 2) + 4 * (j & 3));
          const f32x2 g0 = gelu_fast2((f32x2){acc1[j][tt][0] + bi.x, acc1[j][tt][1] + bi.y});
          const f32x2 g1 = gelu_fast2((f32x2){acc1[j][tt][2] + bi.z, acc1[j][tt][3] + bi.w});
          return (f32x4){(float)(__bf16)g0[0], (float)(__bf16)g0[1], (float)(__bf16)g1[0], (float)(__bf16)g1[1]};
        }, hq[tt], hsb[tt], lane);
      // ---- fc2: k-step g
#pragma unroll
      for (int jc = 0; jc < NJ; ++jc) {
        const i32x8 a = mx_a_frag(smem + L.W2F, g * NJ + jc, lane);
        const int sa = mx_a_scale(smem + L.W2S, g * NJ + jc, lane);
#pragma unroll
        for (int tt = 0; tt < NTT; ++tt)
          acc2[jc][tt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, hq[tt], acc2[jc][tt], 0, 0, 0, sa, 0, hsb[tt]);
      }
    }
    // ---- epilogue of swin_mlp_fwd_kernel: + bias, drop-path scale, + residual; lane (t, lg) owns channels 16 jc + 4 lg .. + 3 of token t
#pragma unroll
    for (int tt = 0; tt < NTT; ++tt) {
      if (!valid[tt]) continue;
      const float sc = p.row_scale ? p.row_scale[tok[tt] / p.rows_per_scale] : 1.f;
#pragma unroll
      for (int jc = 0; jc < NJ; ++jc) {
        const int c0 = 16 * jc + 4 * lg;
        const float4 bi = *reinterpret_cast<const float4*>(p.b2 + c0);
        const bf16x4 res = *reinterpret_cast<const bf16x4*>(p.x1 + tok[tt] * C + c0);
        bf16x4 o;
        o[0] = (__bf16)((float)res[0] + sc * (acc2[jc][tt][0] + bi.x));
        o[1] = (__bf16)((float)res[1] + sc * (acc2[jc][tt][1] + bi.y));
        o[2] = (__bf16)((float)res[2] + sc * (acc2[jc][tt][2] + bi.z));
        o[3] = (__bf16)((float)res[3] + sc * (acc2[jc][tt][3] + bi.w));
        *reinterpret_cast<bf16x4*>(p.out + tok[tt] * C + c0) = o;
      }
    }
  }
}

static inline bool mlp_mx_supported(int C) { return C == 96 || C == 128; }
static inline long long mlp_mx_pack_bytes(int C) { return mlp_mx_supported(C) ? MlpMx(C).PACK_BYTES : 0; }

// ---- MXFP8 data gradient (opt-in sibling of swin_mlp_bwd_kernel; sv_swin_mlp_bwd_mx) ---------------------------------------------------
// The unfused MX backward chain of the branch composed in one kernel: sv_rowscale -> row quantiser of dy -> sv_linear_mxfp8_dgrad (fc2, GELU' at the
// stored pre-activation) -> row quantiser of dh -> sv_linear_mxfp8_dgrad (fc1) -> sv_layernorm_bwd (+ residual).  The pre-activation is RECOMPUTED as
// swin_mlp_fwd_mx_kernel computes it (quantising LayerNorm, fc1 on the forward's W1 MX rows, bf16(acc + b1)), so GELU' is evaluated where the MX
// forward evaluated GELU.  Neither dy's MX rows, hpre nor dh reach HBM.  Same NORMATIVE recipe (linear_fp8.hip "MX recipe"); the lane maps, the image
// kinds and the helpers that carry them are the forward's (see its comment) - described here is what this kernel does with them:
//   recompute     acc1[j] = W1 row tile j of group g . LN(x)_q: lane (t, lg) holds hidden units 128 g + 64 hf + 16 lg + 4 jj + i (j = 4 hf + jj).
//   fc2 dgrad     accd[j] = W2^T row tile j . dy_q: the W2^T image ([4C][Np = 128], quantize_weight_t_mx(fc2.weight)) has W1's shape and is tiled in W1's
//                 row order, so accd and acc1 hold the same hidden units element for element; dy is quantised as LN(x) is (blocks of 32 channels).
//                 dh = bf16(accd * gelu_grad_fast(bf16(acc1 + b1))) is, without lane movement, the lane's B fragment of k-step g of the next product;
//                 it goes through mx_quant_acc as the forward's h does.
//   fc1 dgrad     dln[jc] += W1^T row tile jc (channels 16 jc + r; [C][4C], quantize_weight_t_mx(fc1.weight): W2's shape, W2's fragment order) . dh_q.
//   epilogue      swin_mlp_bwd_kernel's LayerNorm backward + residual on bf16(dln); lane (t, lg) owns channels 16 jc + 4 lg .. + 3 of token t: the row
//                 sums s1, s2 cross the four lane groups, dgamma / dbeta are sums over the 16 token lanes of a DPP row (row_shr 1/2/4/8), then LDS
//                 atomics and one global atomic per workgroup and channel.
//   weights       C = 96: all three images resident in LDS (139 KB with the scales).  C = 128: W1 and W2^T resident, the W1^T fragments of a group are
//                 16-byte loads from L2 issued in front of the GELU' block (3 x 64 KB do not fit; staging the slice through a 16-KB LDS buffer costs two
//                 workgroup barriers per group and measured 1.28 ms against 1.18 ms).  One persistent workgroup per CU.
// Pack image (sv_swin_mlp_bwd_mx_pack, bytes):  W1F [G][8][2][64][16] | W2TF (same) | W1S [G][8][64] | W2TS (same) | W1TS [G][C/16][64] | W1TF [G][C/16][2][64][16]:
// two hidden-row images (W1, W2^T), then one channel-row image (W1^T), its scales first; everything in front of W1TF is resident for either C.
struct MlpMxB : MxImages {
  int W1F, W2TF, W1S, W2TS, W1TS, W1TF, PACK_BYTES, PACK_ITEMS;
  bool RESIDENT;                                           // W1TF in LDS as well
  int LDS_BYTES;
  constexpr explicit MlpMxB(int C)
      : MxImages(C), W1F(0), W2TF(W1F + HROW_DATA), W1S(W2TF + HROW_DATA), W2TS(W1S + HROW_SCALES), W1TS(W2TS + HROW_SCALES), W1TF(W1TS + CROW_SCALES),
        PACK_BYTES(W1TF + CROW_DATA), PACK_ITEMS(2 * HROW_SCALES + CROW_SCALES), RESIDENT(C <= 96), LDS_BYTES(RESIDENT ? PACK_BYTES : W1TF) {}
};

struct MlpMxBArgs {
  const __bf16* x1; const __bf16* dx2; __bf16* out;
  const float* ln_g; const float* ln_b; float eps;
  const uint8_t* packs;
  const float* b1;
  const float* row_scale; int rows_per_scale;
  float* dgamma; float* dbeta;
  long long M; int ntiles;
};

__global__ __launch_bounds__(256) void swin_mlp_bwd_mx_pack_kernel(const uint8_t* __restrict__ w1q, const uint8_t* __restrict__ w1s, const uint8_t* __restrict__ w2tq,
                                                                   const uint8_t* __restrict__ w2ts, const uint8_t* __restrict__ w1tq, const uint8_t* __restrict__ w1ts,
                                                                   uint8_t* __restrict__ packs, int C) {
  const MlpMxB L(C);
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < L.HROW_SCALES) mx_pack_hidden_rows(w1q, w1s, packs + L.W1F, packs + L.W1S, idx);
  else if (idx < 2 * L.HROW_SCALES) mx_pack_hidden_rows(w2tq, w2ts, packs + L.W2TF, packs + L.W2TS, idx - L.HROW_SCALES);
  else if (idx < L.PACK_ITEMS) mx_pack_channel_rows(w1tq, w1ts, packs + L.W1TF, packs + L.W1TS, idx - 2 * L.HROW_SCALES, L);
}

// total over the 16 lanes of a DPP row, in lane 15 of the row
__device__ __forceinline__ float row16_total(float v) {
  v += dpp_shift<0x111, 0xf>(v);   // row_shr:1
  v += dpp_shift<0x112, 0xf>(v);   // row_shr:2
  v += dpp_shift<0x114, 0xf>(v);   // row_shr:4
  v += dpp_shift<0x118, 0xf>(v);   // row_shr:8
  return v;
}

template <int C, int NW, int NTT>
__global__ __launch_bounds__(NW * 64, 1) void swin_mlp_bwd_mx_kernel(const MlpMxBArgs p) {
  constexpr MlpMxB L(C);
  constexpr int HID = L.HID, G = L.G, NJ = L.NJ, NT = NW * 64, TILE = NW * NTT * 16;
  __shared__ __attribute__((aligned(16))) uint8_t smem[L.LDS_BYTES + (HID + 4 * C) * 4];
  float* sb1 = reinterpret_cast<float*>(smem + L.LDS_BYTES);
  float* sdg = sb1 + HID;
  float* sdb = sdg + C;
  float* sgam = sdb + C;                                   // LayerNorm parameters in LDS: see swin_mlp_bwd_kernel
  float* sbet = sgam + C;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = lane & 15, lg = lane >> 4;
  for (int i = tid; i < L.LDS_BYTES / 16; i += NT) reinterpret_cast<i32x4*>(smem)[i] = reinterpret_cast<const i32x4*>(p.packs)[i];
  for (int i = tid; i < HID; i += NT) sb1[i] = p.b1[i];
  for (int i = tid; i < C; i += NT) { sdg[i] = 0.f; sdb[i] = 0.f; sgam[i] = p.ln_g[i]; sbet[i] = p.ln_b[i]; }
  __syncthreads();

#pragma unroll 1
  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    long long tok[NTT]; bool valid[NTT];
    float mean[NTT], rstd[NTT];
    i32x8 xq[NTT], dq[NTT]; int xsb[NTT], dsb[NTT];
    // ---- LayerNorm -> MX B fragments of the recompute (as swin_mlp_fwd_mx_kernel); dbr = bf16(sc dx2) -> MX B fragments of fc2's data gradient
#pragma unroll
    for (int tt = 0; tt < NTT; ++tt) {
      tok[tt] = (long long)tile * TILE + wave * (NTT * 16) + tt * 16 + t;
      valid[tt] = tok[tt] < p.M;
      const float sc = (valid[tt] && p.row_scale) ? p.row_scale[tok[tt] / p.rows_per_scale] : 1.f;
      float xv[2][16], dv[2][16];
      mx_layernorm<C, true>(p.x1, tok[tt], valid[tt], lg, sgam, sbet, p.eps, xv, mean[tt], rstd[tt], p.dx2, sc, dv);
      mx_quant_frag(xv, xq[tt], xsb[tt], lane);
      mx_quant_frag(dv, dq[tt], dsb[tt], lane);
    }

    f32x4 dln[NJ][NTT];
#pragma unroll
    for (int jc = 0; jc < NJ; ++jc)
#pragma unroll
      for (int tt = 0; tt < NTT; ++tt) dln[jc][tt] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (int g = 0; g < G; ++g) {
      // ---- the 128 hidden units of group g: pre-activation (recomputed) and dy . W2, two independent chains interleaved on the matrix pipe
      f32x4 acc1[8][NTT], accd[8][NTT];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const i32x8 a = mx_a_frag(smem + L.W1F, g * 8 + j, lane), at = mx_a_frag(smem + L.W2TF, g * 8 + j, lane);
        const int sa = mx_a_scale(smem + L.W1S, g * 8 + j, lane), sat = mx_a_scale(smem + L.W2TS, g * 8 + j, lane);
#pragma unroll
        for (int tt = 0; tt < NTT; ++tt) {
          acc1[j][tt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, xq[tt], (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0, sa, 0, xsb[tt]);
          accd[j][tt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(at, dq[tt], (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0, sat, 0, dsb[tt]);
        }
      }
      // W1^T fragments of the group that are not resident (C = 128): requested here, they arrive under the GELU' block
      i32x8 wt[L.RESIDENT ? 1 : NJ];
      if constexpr (!L.RESIDENT) {
#pragma unroll
        for (int jc = 0; jc < NJ; ++jc) wt[jc] = mx_a_frag(p.packs + L.W1TF, g * NJ + jc, lane);
      }
      // ---- dh = bf16(accd * GELU'(bf16(acc1 + b1))), MX quantisation in registers: the B fragment of k-step g of fc1's data gradient
      i32x8 hq[NTT]; int hsb[NTT];
      const float* gb1 = sb1 + 128 * g + 16 * lg;          // the lane's biases: tile j = 4 hf + jj at + 64 hf + 4 jj
#pragma unroll
      for (int tt = 0; tt < NTT; ++tt)
        mx_quant_acc([&](int j) {
          const float4 bi = *reinterpret_cast<const float4*>(gb1 + 64 * (j >> 2) + 4 * (j & 3));
          const f32x2 d0 = gelu_grad_fast2((f32x2){(float)(__bf16)(acc1[j][tt][0] + bi.x), (float)(__bf16)(acc1[j][tt][1] + bi.y)});
          const f32x2 d1 = gelu_grad_fast2((f32x2){(float)(__bf16)(acc1[j][tt][2] + bi.z), (float)(__bf16)(acc1[j][tt][3] + bi.w)});
          return (f32x4){(float)(__bf16)(accd[j][tt][0] * d0[0]), (float)(__bf16)(accd[j][tt][1] * d0[1]),
                         (float)(__bf16)(accd[j][tt][2] * d1[0]), (float)(__bf16)(accd[j][tt][3] * d1[1])};
        }, hq[tt], hsb[tt], lane);
      // ---- fc1 data gradient: k-step g
#pragma unroll
      for (int jc = 0; jc < NJ; ++jc) {
        i32x8 a;
        if constexpr (L.RESIDENT) a = mx_a_frag(smem + L.W1TF, g * NJ + jc, lane);
        else a = wt[jc];
        const int sa = mx_a_scale(smem + L.W1TS, g * NJ + jc, lane);
#pragma unroll
        for (int tt = 0; tt < NTT; ++tt)
          dln[jc][tt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, hq[tt], dln[jc][tt], 0, 0, 0, sa, 0, hsb[tt]);
      }
    }
    // ---- LayerNorm backward + residual on bf16(dln) (swin_mlp_bwd_kernel's epilogue); lane (t, lg): channels 16 jc + 4 lg + k of token t.
    // The lane offset is laundered per tile so that the LDS addresses stay immediate offsets (see swin_mlp_bwd_kernel)
    int lane_off = 4 * lg;
    asm volatile("" : "+v"(lane_off));
    float* const lg_ = sgam + lane_off;
    float* const ldg_ = sdg + lane_off;
    float* const ldb_ = sdb + lane_off;
#pragma unroll
    for (int tt = 0; tt < NTT; ++tt) {
      const bool ok = valid[tt];
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int jc = 0; jc < NJ; ++jc) {
        bf16x4 xr = V4<__bf16>::zero();
        if (ok) xr = *reinterpret_cast<const bf16x4*>(p.x1 + tok[tt] * C + 16 * jc + 4 * lg);
        const float4 gm = *reinterpret_cast<const float4*>(lg_ + 16 * jc);
        const float gv[4] = {gm.x, gm.y, gm.z, gm.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          dln[jc][tt][k] = (float)(__bf16)dln[jc][tt][k];  // the value the unfused fc1 data gradient stores
          const float xh = ok ? ((float)xr[k] - mean[tt]) * rstd[tt] : 0.f;
          const float d = ok ? dln[jc][tt][k] : 0.f;
          const float gg = d * gv[k];
          s1 += gg; s2 += gg * xh;
          const float tb = row16_total(d), tg = row16_total(d * xh);
          if (t == 15) { atomicAdd(ldb_ + 16 * jc + k, tb); atomicAdd(ldg_ + 16 * jc + k, tg); }
        }
        __builtin_amdgcn_sched_barrier(0);                 // keep the 8 reduction chains of one channel group together
      }
      s1 = lane_step_add<16>(s1); s1 = lane_step_add<32>(s1);
      s2 = lane_step_add<16>(s2); s2 = lane_step_add<32>(s2);
      s1 *= (1.f / C); s2 *= (1.f / C);
      if (ok) {
#pragma unroll
        for (int jc = 0; jc < NJ; ++jc) {
          const int c0 = 16 * jc + 4 * lg;
          const bf16x4 xr = *reinterpret_cast<const bf16x4*>(p.x1 + tok[tt] * C + c0);
          const bf16x4 dr = *reinterpret_cast<const bf16x4*>(p.dx2 + tok[tt] * C + c0);
          const float4 gm = *reinterpret_cast<const float4*>(lg_ + 16 * jc);
          const float gv[4] = {gm.x, gm.y, gm.z, gm.w};
          bf16x4 o;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float xh = ((float)xr[k] - mean[tt]) * rstd[tt];
            o[k] = (__bf16)((float)dr[k] + rstd[tt] * (dln[jc][tt][k] * gv[k] - s1 - xh * s2));
          }
          *reinterpret_cast<bf16x4*>(p.out + tok[tt] * C + c0) = o;
        }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < C; i += NT) { atomicAdd(p.dgamma + i, sdg[i]); atomicAdd(p.dbeta + i, sdb[i]); }
}

// C = 128 is served while its instantiation is free of spills and scratch; the host keeps the bf16 backward where this says no
static inline bool mlp_bwd_mx_supported(int C) { return C == 96 || C == 128; }
static inline long long mlp_bwd_mx_pack_bytes(int C) { return mlp_bwd_mx_supported(C) ? MlpMxB(C).PACK_BYTES : 0; }

// ---- MXFP8 weight gradients (opt-in sibling of swin_mlp_wgrad_kernel; sv_swin_mlp_wgrad_mx) ---------------------------------------------
// The unfused MX weight-gradient chain of the branch composed in one kernel: quantising LayerNorm -> fc1 on MX rows (hpre = bf16(acc + b1), h =
// bf16(gelu_fast(acc + b1)) at the fp32 value) -> sv_rowscale -> row quantiser of dbr -> fc2's data gradient on MX rows, dh = bf16(acc *
// gelu_grad_fast(hpre)) -> the four COLUMN quantisers (blocks of 32 consecutive tokens of one column, counted from token 0; rows past M are zero) ->
// dW2[c][hid] += q_cols(dbr)[c] . q_cols(h)[hid], dW1[hid][c] += q_cols(dh)[hid] . q_cols(ln)[c] over the tokens; db2 / db1 are the fp32 column
// sums of the unquantised dbr / dh.  Neither hpre, h, dh nor any quantised operand reaches HBM.  Same NORMATIVE recipe (linear_fp8.hip "MX
// recipe").  K = C <= 128, so fc1 and fc2's data gradient are one scaled MFMA per output tile and hpre, h, dh are the chain's bit for bit; only the
// fp32 order of the sum over token k-steps and token splits differs.  All four products on v_mfma_scale_f32_16x16x128_f8f6f4.
//   skeleton      swin_mlp_wgrad_kernel's: a workgroup of 8 waves owns 128 hidden units (16 per wave) and walks a token range in 128-token tiles (tiles
//                 and splits start at multiples of 128 tokens, so the kernel's 32-token blocks are the chain's); dW accumulators stay in registers over
//                 the range, one float atomicAdd per element at the end (across token splits only).
//   per tile      (1) wave w runs mx_layernorm on tokens 16 w .. + 15 (lane (t, lg), as the other two MX kernels), zeroes rows past the end, and
//                 leaves in LDS: the MX row fragments of ln and dbr (mx_quant_frag; the [tile][2][64][16] + [tile][64] image mx_a_frag reads) and
//                 the bf16 values themselves, LT / DT [128 tokens][C + 8] (16-byte stores).  (2) The 2 C / 16 column fragments (16 channels x 128
//                 tokens of ln^T / dbr^T) are shared among the waves: lane (c, lg) takes tokens 64 hf + 16 lg .. + 15 of its channel out of LT / DT by
//                 ds_read_b64_tr_b16 - with a row of the TRANSPOSED tensor on the lane the column quantiser IS mx_quant_frag - and the fragments go to
//                 LDS once for all waves; workgroups of hidden group 0 add the column sums of DT to db2 (four threads per channel, combined in a fixed
//                 order at the end).  (3) Each wave, for each 16-token tile T: acc1 = ln_q[T] . W1_q[wave's units], accd = dbr_q[T] . W2^T_q[wave's
//                 units] (tokens on the accumulator rows: lane (u, lg) holds tokens 16 T + 4 lg + i of unit u; the W1 / W2^T rows are the lane's B
//                 fragments, read once from the native [4C][128] images), h and dh as above, 8-byte stores into the wave's own [16 units][128 tokens]
//                 bf16 images.  Read back as rows (lane (u, lg): tokens 64 hf + 16 lg .. + 15) they go through mx_quant_frag and are the B fragments
//                 of the two contractions against the C / 16 column fragments of (2).
//   LDS           row fragments 2 x 8 x (2048 + 64), column fragments 2 x C/16 x (2048 + 64), one region that holds LT | DT in (1)-(2) and the waves'
//                 h / dh images in (3) (69 632 bytes), gamma / beta: 126.5 KB (C = 96) / 135 KB (C = 128).  Three workgroup barriers per tile.
struct MlpMxWArgs {
  const __bf16* x1; const __bf16* dx2;
  const float* ln_g; const float* ln_b; float eps;
  const uint8_t* w1q; const uint8_t* w1s;    // [4C][128], [4C][4]  sv_quant_rows_mx_e4m3 of fc1.weight
  const uint8_t* w2tq; const uint8_t* w2ts;  // [4C][128], [4C][4]  sv_quant_cols_mx_e4m3 of fc2.weight
  const float* b1; const float* row_scale; int rows_per_scale;
  float* dw1; float* db1; float* dw2; float* db2;     // native layouts [4C][C], [4C], [C][4C], [C]
  long long M; int tok_per_split; int HG;
};

constexpr int MXW_NW = 8, MXW_TT = 128;
struct MlpMxW {                                            // LDS plan (bytes); LTS / HTS: row strides of the LT | DT tiles ([token][C + 8] bf16) and of a wave's h / dh image
  int NJ, XF, DF, XS, DS, XTF, DTF, XTS, DTS, UN, LTS, HTS, UN_BYTES, PAR, LDS_BYTES;
  constexpr explicit MlpMxW(int C)
      : NJ(C / 16), XF(0), DF(XF + 8 * 2048), XS(DF + 8 * 2048), DS(XS + 8 * 64), XTF(DS + 8 * 64), DTF(XTF + NJ * 2048), XTS(DTF + NJ * 2048),
        DTS(XTS + NJ * 64), UN(DTS + NJ * 64), LTS(2 * C + 16), HTS(2 * MXW_TT + 16),
        UN_BYTES(2 * MXW_TT * LTS > MXW_NW * 2 * 16 * HTS ? 2 * MXW_TT * LTS : MXW_NW * 2 * 16 * HTS), PAR(UN + UN_BYTES), LDS_BYTES(PAR + 2 * C * 4) {}
};

// a fragment (tile `tile` of an image mx_a_frag reads) and its scale bytes into LDS
__device__ __forceinline__ void mx_put_frag(uint8_t* data, uint8_t* scales, int tile, int lane, const i32x8& q, int sbyte) {
  uint8_t* fa = data + (size_t)(tile * 2) * 1024 + lane * 16;
  *reinterpret_cast<i32x4*>(fa) = (i32x4){q[0], q[1], q[2], q[3]};
  *reinterpret_cast<i32x4*>(fa + 1024) = (i32x4){q[4], q[5], q[6], q[7]};
  scales[tile * 64 + lane] = (uint8_t)sbyte;
}

template <int C>
__global__ __launch_bounds__(MXW_NW * 64, 1) void swin_mlp_wgrad_mx_kernel(const MlpMxWArgs p) {
  constexpr MlpMxW L(C);
  constexpr int NW = MXW_NW, TT = MXW_TT, NT = NW * 64, HID = 4 * C, NJ = L.NJ;
  static_assert(TT == NW * 16, "one 16-token tile per wave");
  __shared__ __attribute__((aligned(16))) uint8_t smem[L.LDS_BYTES];
  float* sgam = reinterpret_cast<float*>(smem + L.PAR);
  float* sbet = sgam + C;
  const int tid = threadIdx.x, lane0 = tid & 63, wave = tid >> 6;
  for (int i = tid; i < C; i += NT) { sgam[i] = p.ln_g[i]; sbet[i] = p.ln_b[i]; }
  const int hg = blockIdx.x % p.HG, split = blockIdx.x / p.HG;
  const int hid = (hg * NW + wave) * 16 + (lane0 & 15);    // the lane's hidden unit in phase (3)
  const long long t_begin = (long long)split * p.tok_per_split;
  long long t_end = t_begin + p.tok_per_split;
  if (t_end > p.M) t_end = p.M;

  // per-wave constant B fragments: the MX rows of W1 / W2^T of the wave's hidden units (k = channels) and their block scales
  i32x8 w1b, w2b;
  {
    const int lg = lane0 >> 4;
    const i32x4 a0 = *reinterpret_cast<const i32x4*>(p.w1q + (size_t)hid * 128 + 16 * lg), a1 = *reinterpret_cast<const i32x4*>(p.w1q + (size_t)hid * 128 + 64 + 16 * lg);
    const i32x4 c0 = *reinterpret_cast<const i32x4*>(p.w2tq + (size_t)hid * 128 + 16 * lg), c1 = *reinterpret_cast<const i32x4*>(p.w2tq + (size_t)hid * 128 + 64 + 16 * lg);
    w1b = (i32x8){a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
    w2b = (i32x8){c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]};
  }
  const int w1sb = p.w1s[hid * 4 + (lane0 >> 4)], w2sb = p.w2ts[hid * 4 + (lane0 >> 4)];
  const float b1v = p.b1[hid];

  f32x4 G2[NJ], G1[NJ];
#pragma unroll
  for (int jc = 0; jc < NJ; ++jc) { G2[jc] = (f32x4){0.f, 0.f, 0.f, 0.f}; G1[jc] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
  float db1acc = 0.f, db2acc = 0.f;

  __bf16* const LT = reinterpret_cast<__bf16*>(smem + L.UN);                   // [128 tokens][LTS / 2]  ln of the tile, bf16 (C + 8 elements per row)
  __bf16* const DT = reinterpret_cast<__bf16*>(smem + L.UN + TT * L.LTS);      // [128 tokens][LTS / 2]  dbr
  uint8_t* const hth = smem + L.UN + wave * (2 * 16 * L.HTS);                  // [16][HTS] bytes  the wave's h image (aliases LT | DT)
  uint8_t* const htd = hth + 16 * L.HTS;                                       //                  the wave's dh image

#pragma unroll 1
  for (long long t0 = t_begin; t0 < t_end; t0 += TT) {
    __syncthreads();                                       // the previous tile's fragments and h / dh images have been consumed
    // lane index laundered per tile: otherwise hipcc materialises the ~100 per-lane LDS addresses of the tile once, outside the token loop, and spills
    // them around it; with an opaque lane they stay immediate offsets of the ds instructions (see swin_mlp_bwd_kernel)
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const int t = lane & 15, lg = lane >> 4;
    // ---- (1) LayerNorm and row scale of the wave's 16 tokens -> MX row fragments, bf16 values transposed
    {
      const int tl = 16 * wave + t;
      const long long tok = t0 + tl;
      const bool valid = tok < t_end;
      const float sc = (valid && p.row_scale) ? p.row_scale[tok / p.rows_per_scale] : 1.f;
      float xv[2][16], dv[2][16], mean, rstd;
      mx_layernorm<C, true>(p.x1, tok, valid, lg, sgam, sbet, p.eps, xv, mean, rstd, p.dx2, sc, dv);
      if (!valid) {                                        // rows past the end are zero in every operand (dv already is)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
#pragma unroll
          for (int j = 0; j < 16; ++j) xv[hf][j] = 0.f;
      }
      i32x8 q; int sb;
      mx_quant_frag(xv, q, sb, lane);
      mx_put_frag(smem + L.XF, smem + L.XS, wave, lane, q, sb);
      mx_quant_frag(dv, q, sb, lane);
      mx_put_frag(smem + L.DF, smem + L.DS, wave, lane, q, sb);
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
        if (64 * hf + 16 * lg < C) {
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            bf16x8 xo, dd;
#pragma unroll
            for (int j = 0; j < 8; ++j) { xo[j] = (__bf16)xv[hf][8 * u + j]; dd[j] = (__bf16)dv[hf][8 * u + j]; }   // exact: bf16 values already
            *reinterpret_cast<bf16x8*>(LT + tl * (L.LTS / 2) + 64 * hf + 16 * lg + 8 * u) = xo;
            *reinterpret_cast<bf16x8*>(DT + tl * (L.LTS / 2) + 64 * hf + 16 * lg + 8 * u) = dd;
          }
        }
    }
    __syncthreads();
    // ---- (2) column quantisers of ln and dbr: fragment f = (tensor, 16-channel tile), shared among the waves
#pragma unroll 1
    for (int f = wave; f < 2 * NJ; f += NW) {
      const int which = f / NJ, jc = f % NJ;
      // ds_read_b64_tr_b16: the 16 lanes of a group read a 4-token x 16-channel block (lane: token + (t >> 2), channels 4 (t & 3) .. + 3) and
      // receive it transposed - lane t gets channel t of the block, its 4 tokens (as in swin_mlp_wgrad_kernel)
      const __bf16* src = (which ? DT : LT) + (16 * lg + (t >> 2)) * (L.LTS / 2) + 16 * jc + 4 * (t & 3);
      float v[2][16];
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const bf16x4 r = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_t*)(src + (64 * hf + 4 * u) * (L.LTS / 2)));
#pragma unroll
          for (int k = 0; k < 4; ++k) v[hf][4 * u + k] = (float)r[k];
        }
      i32x8 q; int sb;
      mx_quant_frag(v, q, sb, lane);
      mx_put_frag(smem + (which ? L.DTF : L.XTF), smem + (which ? L.DTS : L.XTS), jc, lane, q, sb);
    }
    if (hg == 0 && tid < 4 * C) {                          // bias gradient of fc2: column sums of the unquantised dbr, 32 tokens per thread
      const __bf16* col = DT + (tid / C) * 32 * (L.LTS / 2) + tid % C;
      float s = 0.f;
#pragma unroll 8
      for (int r = 0; r < 32; ++r) s += (float)col[r * (L.LTS / 2)];
      db2acc += s;
    }
    __syncthreads();                                       // column fragments ready; LT / DT are dead, their space is the waves' h / dh images
    // ---- (3) recompute h and dh of the wave's 16 hidden units, tokens on the accumulator rows
#pragma unroll 2
    for (int T = 0; T < 8; ++T) {
      const i32x8 a = mx_a_frag(smem + L.XF, T, lane), d = mx_a_frag(smem + L.DF, T, lane);
      const int sa = mx_a_scale(smem + L.XS, T, lane), sd = mx_a_scale(smem + L.DS, T, lane);
      const f32x4 acc1 = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, w1b, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0, sa, 0, w1sb);
      const f32x4 accd = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(d, w2b, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0, sd, 0, w2sb);
      const f32x2 p0 = (f32x2){acc1[0] + b1v, acc1[1] + b1v}, p1 = (f32x2){acc1[2] + b1v, acc1[3] + b1v};
      const f32x2 g0 = gelu_fast2(p0), g1 = gelu_fast2(p1);                   // GELU at the fp32 value ...
      const f32x2 e0 = gelu_grad_fast2((f32x2){(float)(__bf16)p0[0], (float)(__bf16)p0[1]});   // ... GELU' at the stored (bf16) pre-activation
      const f32x2 e1 = gelu_grad_fast2((f32x2){(float)(__bf16)p1[0], (float)(__bf16)p1[1]});
      const float hv[4] = {g0[0], g0[1], g1[0], g1[1]};
      const float ev[4] = {e0[0], e0[1], e1[0], e1[1]};
      const long long tk = t0 + 16 * T + 4 * lg;           // the lane's tokens tk .. tk + 3
      bf16x4 hb, db;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        hb[i] = tk + i < t_end ? (__bf16)hv[i] : (__bf16)0.f;   // rows past the end: zero (acc1 = 0 there gives GELU(b1))
        db[i] = (__bf16)(accd[i] * ev[i]);                      // accd = 0 there
        db1acc += (float)db[i];
      }
      *reinterpret_cast<bf16x4*>(hth + t * L.HTS + (16 * T + 4 * lg) * 2) = hb;
      *reinterpret_cast<bf16x4*>(htd + t * L.HTS + (16 * T + 4 * lg) * 2) = db;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // the wave's own stores have landed before its lanes read each other's
    // ---- the token contractions: the wave's h / dh rows (column-quantised: blocks of 32 tokens) against the column fragments of dbr / ln
#pragma unroll
    for (int which = 0; which < 2; ++which) {
      const uint8_t* src = (which ? htd : hth) + t * L.HTS;
      float v[2][16];
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const bf16x8 r = *reinterpret_cast<const bf16x8*>(src + (64 * hf + 16 * lg + 8 * u) * 2);
#pragma unroll
          for (int k = 0; k < 8; ++k) v[hf][8 * u + k] = (float)r[k];
        }
      i32x8 q; int sb;
      mx_quant_frag(v, q, sb, lane);
#pragma unroll
      for (int jc = 0; jc < NJ; ++jc) {
        if (which == 0)   // dW2[c][hid]: rows = channels 16 jc + 4 lg + i, column = the lane's hidden unit
          G2[jc] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(mx_a_frag(smem + L.DTF, jc, lane), q, G2[jc], 0, 0, 0, mx_a_scale(smem + L.DTS, jc, lane), 0, sb);
        else              // dW1[hid][c], held transposed
          G1[jc] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(mx_a_frag(smem + L.XTF, jc, lane), q, G1[jc], 0, 0, 0, mx_a_scale(smem + L.XTS, jc, lane), 0, sb);
      }
    }
  }
  // ---- write out (accumulator: row = channel 16 jc + 4 lg + i, column = hidden unit `hid`)
  const int lg = lane0 >> 4;
#pragma unroll
  for (int jc = 0; jc < NJ; ++jc)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = 16 * jc + 4 * lg + i;
      atomicAdd(p.dw2 + (size_t)c * HID + hid, G2[jc][i]);
      atomicAdd(p.dw1 + (size_t)hid * C + c, G1[jc][i]);
    }
  db1acc = lane_step_add<16>(db1acc);
  db1acc = lane_step_add<32>(db1acc);
  if (lg == 0) atomicAdd(p.db1 + hid, db1acc);
  if (hg == 0) {                                           // the four partial sums of a channel in a fixed order, then one atomic
    float* red = reinterpret_cast<float*>(smem);
    __syncthreads();
    if (tid < 4 * C) red[tid] = db2acc;
    __syncthreads();
    if (tid < C) atomicAdd(p.db2 + tid, (red[tid] + red[C + tid]) + (red[2 * C + tid] + red[3 * C + tid]));
  }
}

// both widths are served while their instantiations are free of spills and scratch; the host keeps swin_mlp_wgrad_kernel where this says no
static inline bool mlp_wgrad_mx_supported(int C) { return C == 96 || C == 128; }

}  // namespace sv

using namespace sv;
#define STREAM static_cast<hipStream_t>(stream)

extern "C" int sv_swin_mlp_supported(int C) { return mlp_supported(C) ? 1 : 0; }

extern "C" int sv_swin_mlp_pack(const float* w1, const float* w2, void* packs, int C, void* stream) {
  SV_REQUIRE(w1 && w2 && packs && mlp_supported(C), "swin_mlp_pack: bad arguments (C=%d)", C);
  const long long total = 16ll * C * C;
  hipLaunchKernelGGL(swin_mlp_pack_kernel, dim3(cdiv(total, 256 * 4)), dim3(256), 0, STREAM, w1, w2, static_cast<__bf16*>(packs), C);
  return check_launch("sv_swin_mlp_pack");
}

static int mlp_check(const void* x1, const void* out, const float* g, const float* b, const void* packs, long long M, int C, int rps) {
  SV_REQUIRE(x1 && out && g && b && packs && M > 0 && M < (1ll << 31) && mlp_supported(C), "swin_mlp: bad arguments (M=%lld C=%d)", M, C);
  SV_REQUIRE((((uintptr_t)x1 | (uintptr_t)out | (uintptr_t)packs) & 15) == 0 && (((uintptr_t)g | (uintptr_t)b) & 15) == 0, "swin_mlp: operands must be 16-byte aligned");
  SV_REQUIRE(rps > 0, "swin_mlp: rows_per_scale must be positive");
  return SV_OK;
}

extern "C" int sv_swin_mlp_fwd(const void* x1, void* x2, const float* ln_g, const float* ln_b, const void* packs, const float* b1,
                               const float* b2, const float* row_scale, int rows_per_scale, long long M, int C, float eps, void* stream) {
  if (int rc = mlp_check(x1, x2, ln_g, ln_b, packs, M, C, rows_per_scale)) return rc;
  SV_REQUIRE(b1 && b2 && (((uintptr_t)b2) & 15) == 0, "swin_mlp_fwd: biases required (16-byte aligned)");
  MlpArgs a{};
  a.x1 = static_cast<const __bf16*>(x1); a.out = static_cast<__bf16*>(x2); a.ln_g = ln_g; a.ln_b = ln_b; a.eps = eps;
  a.packs = static_cast<const __bf16*>(packs); a.b1 = b1; a.b2 = b2; a.row_scale = row_scale; a.rows_per_scale = rows_per_scale; a.M = M;
#define SV_MLP_FWD(CC, NW, WPS) hipLaunchKernelGGL((swin_mlp_fwd_kernel<CC, NW, WPS>), dim3(cdiv(M, NW * 32)), dim3(NW * 64), 0, STREAM, a)
  if (C == 96) SV_MLP_FWD(96, 4, 2);
  else if (C == 128) SV_MLP_FWD(128, 4, 2);
  else SV_MLP_FWD(192, 4, 1);
#undef SV_MLP_FWD
  return check_launch("sv_swin_mlp_fwd");
}

extern "C" int sv_swin_mlp_bwd(const void* x1, const void* dx2, void* dx1, const float* ln_g, const float* ln_b, const void* packs,
                               const float* b1, const float* row_scale, int rows_per_scale, float* dgamma, float* dbeta, long long M, int C,
                               float eps, void* stream) {
  if (int rc = mlp_check(x1, dx1, ln_g, ln_b, packs, M, C, rows_per_scale)) return rc;
  SV_REQUIRE(dx2 && b1 && dgamma && dbeta && (((uintptr_t)dx2) & 15) == 0, "swin_mlp_bwd: bad arguments");
  MlpArgs a{};
  a.x1 = static_cast<const __bf16*>(x1); a.dx2 = static_cast<const __bf16*>(dx2); a.out = static_cast<__bf16*>(dx1);
  a.ln_g = ln_g; a.ln_b = ln_b; a.eps = eps; a.packs = static_cast<const __bf16*>(packs); a.b1 = b1;
  a.row_scale = row_scale; a.rows_per_scale = rows_per_scale; a.dgamma = dgamma; a.dbeta = dbeta; a.M = M;
#define SV_MLP_BWD(CC, NW, WPS)                                                                           \
  do {                                                                                                    \
    a.ntiles = cdiv(M, NW * 32);                                                                          \
    int grid = 256 * WPS; if (grid > a.ntiles) grid = a.ntiles;                                           \
    hipLaunchKernelGGL((swin_mlp_bwd_kernel<CC, NW, WPS>), dim3(grid), dim3(NW * 64), 0, STREAM, a);      \
  } while (0)
  if (C == 96) SV_MLP_BWD(96, 4, 2);
  else if (C == 128) SV_MLP_BWD(128, 4, 1);
  else SV_MLP_BWD(192, 4, 1);
#undef SV_MLP_BWD
  return check_launch("sv_swin_mlp_bwd");
}

extern "C" int sv_swin_mlp_wgrad(const void* x1, const void* dx2, const float* ln_g, const float* ln_b, const void* w1_rows,
                                 const void* w2t_rows, const float* b1, const float* row_scale, int rows_per_scale, float* dw1, float* db1,
                                 float* dw2, float* db2, long long M, int C, float eps, void* stream) {
  SV_REQUIRE(x1 && dx2 && ln_g && ln_b && w1_rows && w2t_rows && b1 && dw1 && db1 && dw2 && db2 && M > 0 && M < (1ll << 31) && mlp_supported(C),
             "swin_mlp_wgrad: bad arguments (M=%lld C=%d)", M, C);
  SV_REQUIRE((((uintptr_t)x1 | (uintptr_t)dx2 | (uintptr_t)w1_rows | (uintptr_t)w2t_rows) & 15) == 0 && rows_per_scale > 0, "swin_mlp_wgrad: alignment");
  SV_REQUIRE(!row_scale || rows_per_scale >= 128, "swin_mlp_wgrad: rows_per_scale (%d) must be >= 128 (a token tile spans at most two scale groups)", rows_per_scale);
  MlpWArgs a{};
  a.x1 = static_cast<const __bf16*>(x1); a.dx2 = static_cast<const __bf16*>(dx2); a.ln_g = ln_g; a.ln_b = ln_b; a.eps = eps;
  a.w1r = static_cast<const __bf16*>(w1_rows); a.w2tr = static_cast<const __bf16*>(w2t_rows); a.b1 = b1;
  a.row_scale = row_scale; a.rows_per_scale = rows_per_scale; a.dw1 = dw1; a.db1 = db1; a.dw2 = dw2; a.db2 = db2; a.M = M;
#define SV_MLP_WG(CC, NW, HCW, TT)                                                                              \
  do {                                                                                                          \
    a.HG = (4 * CC) / (NW * HCW);                                                                               \
    long long splits = 256 / a.HG; if (splits < 1) splits = 1;                                                  \
    long long tps = (M + splits - 1) / splits; tps = (tps + TT - 1) / TT * TT;                                  \
    splits = (M + tps - 1) / tps;                                                                               \
    a.tok_per_split = (int)tps;                                                                                 \
    hipLaunchKernelGGL((swin_mlp_wgrad_kernel<CC, NW, HCW, TT>), dim3((unsigned)(splits * a.HG)), dim3(NW * 64), 0, STREAM, a); \
  } while (0)
  if (C == 96) SV_MLP_WG(96, 6, 32, 128);
  else if (C == 128) SV_MLP_WG(128, 8, 16, 128);
  else SV_MLP_WG(192, 8, 16, 64);
#undef SV_MLP_WG
  return check_launch("sv_swin_mlp_wgrad");
}

// ---- MXFP8: what the forward and the data gradient share on the host -------------------------------------------------------------------
// what sv_swin_mlp_fwd_mx and sv_swin_mlp_bwd_mx ask alike; `who` names the entry point that was called, `widths` what it adds to "unsupported C"
static int mlp_mx_check(const char* who, bool pointers, bool served, const char* widths, uintptr_t aligned16, long long M, int C, int rows_per_scale) {
  SV_REQUIRE(pointers, "%s: null pointer", who);
  SV_REQUIRE(served, "%s: unsupported C=%d%s", who, C, widths);
  SV_REQUIRE(M > 0 && M < (1ll << 31), "%s: M=%lld out of range", who, M);
  SV_REQUIRE((aligned16 & 15) == 0, "%s: operands must be 16-byte aligned", who);
  SV_REQUIRE(rows_per_scale > 0, "%s: rows_per_scale must be positive", who);
  return SV_OK;
}
// 8 waves x 16 tokens: two waves per SIMD, so one wave's GELU / quantiser VALU stream runs beside the other's MFMAs and LDS reads (measured against
// 4 waves x 32 tokens and 8 x 32; in the backward 8 x 32 spills and is slower)
constexpr int MX_NW = 8, MX_NTT = 1;
template <class Args>
static int mlp_mx_launch(const char* who, void (*k96)(Args), void (*k128)(Args), int C, Args& a, hipStream_t stream, std::atomic<long long>& launches) {
  a.ntiles = cdiv(a.M, MX_NW * MX_NTT * 16);
  const int grid = a.ntiles < 256 ? a.ntiles : 256;        // one persistent workgroup per CU: the weights enter LDS once
  hipLaunchKernelGGL(C == 96 ? k96 : k128, dim3(grid), dim3(MX_NW * 64), 0, stream, a);
  const int rc = check_launch(who);
  if (rc == SV_OK) launches.fetch_add(1, std::memory_order_relaxed);
  return rc;
}

// ---- MXFP8 forward ------------------------------------------------------------------------------------------------------------------
static std::atomic<long long> swin_mlp_mx_launches{0};
extern "C" long long sv_swin_mlp_mx_launches(void) { return swin_mlp_mx_launches.load(std::memory_order_relaxed); }
extern "C" int sv_swin_mlp_mx_supported(int C) { return mlp_mx_supported(C) ? 1 : 0; }
extern "C" long long sv_swin_mlp_mx_pack_bytes(int C) { return mlp_mx_pack_bytes(C); }

extern "C" int sv_swin_mlp_mx_pack(const void* w1q, const void* w1s, const void* w2q, const void* w2s, void* packs, int C, void* stream) {
  SV_REQUIRE(w1q && w1s && w2q && w2s && packs, "sv_swin_mlp_mx_pack: null pointer");
  SV_REQUIRE(mlp_mx_supported(C), "sv_swin_mlp_mx_pack: unsupported C=%d (96 or 128)", C);
  SV_REQUIRE((((uintptr_t)w1q | (uintptr_t)w2q | (uintptr_t)packs) & 15) == 0, "sv_swin_mlp_mx_pack: w1q, w2q and packs must be 16-byte aligned");
  hipLaunchKernelGGL(swin_mlp_mx_pack_kernel, dim3(cdiv(MlpMx(C).PACK_ITEMS, 256)), dim3(256), 0, STREAM, static_cast<const uint8_t*>(w1q), static_cast<const uint8_t*>(w1s),
                     static_cast<const uint8_t*>(w2q), static_cast<const uint8_t*>(w2s), static_cast<uint8_t*>(packs), C);
  return check_launch("sv_swin_mlp_mx_pack");
}

extern "C" int sv_swin_mlp_fwd_mx(const void* x1, void* x2, const float* ln_g, const float* ln_b, const void* packs_mx, const float* b1,
                                  const float* b2, const float* row_scale, int rows_per_scale, long long M, int C, float eps, void* stream) {
  if (int rc = mlp_mx_check("sv_swin_mlp_fwd_mx", x1 && x2 && ln_g && ln_b && packs_mx && b1 && b2, mlp_mx_supported(C), " (96 or 128)",
                            (uintptr_t)x1 | (uintptr_t)x2 | (uintptr_t)packs_mx | (uintptr_t)ln_g | (uintptr_t)ln_b | (uintptr_t)b2, M, C, rows_per_scale))
    return rc;
  MlpMxArgs a{};
  a.x1 = static_cast<const __bf16*>(x1); a.out = static_cast<__bf16*>(x2); a.ln_g = ln_g; a.ln_b = ln_b; a.eps = eps;
  a.packs = static_cast<const uint8_t*>(packs_mx); a.b1 = b1; a.b2 = b2; a.row_scale = row_scale; a.rows_per_scale = rows_per_scale; a.M = M;
  return mlp_mx_launch("sv_swin_mlp_fwd_mx", swin_mlp_fwd_mx_kernel<96, MX_NW, MX_NTT>, swin_mlp_fwd_mx_kernel<128, MX_NW, MX_NTT>, C, a, STREAM,
                       swin_mlp_mx_launches);
}

// ---- MXFP8 data gradient ------------------------------------------------------------------------------------------------------------
static std::atomic<long long> swin_mlp_bwd_mx_launches{0};
extern "C" long long sv_swin_mlp_bwd_mx_launches(void) { return swin_mlp_bwd_mx_launches.load(std::memory_order_relaxed); }
extern "C" int sv_swin_mlp_bwd_mx_supported(int C) { return mlp_bwd_mx_supported(C) ? 1 : 0; }
extern "C" long long sv_swin_mlp_bwd_mx_pack_bytes(int C) { return mlp_bwd_mx_pack_bytes(C); }

extern "C" int sv_swin_mlp_bwd_mx_pack(const void* w1q, const void* w1s, const void* w2tq, const void* w2ts, const void* w1tq, const void* w1ts, void* packs,
                                       int C, void* stream) {
  SV_REQUIRE(w1q && w1s && w2tq && w2ts && w1tq && w1ts && packs, "sv_swin_mlp_bwd_mx_pack: null pointer");
  SV_REQUIRE(mlp_bwd_mx_supported(C), "sv_swin_mlp_bwd_mx_pack: unsupported C=%d", C);
  SV_REQUIRE((((uintptr_t)w1q | (uintptr_t)w2tq | (uintptr_t)w1tq | (uintptr_t)packs) & 15) == 0,
             "sv_swin_mlp_bwd_mx_pack: w1q, w2tq, w1tq and packs must be 16-byte aligned");
  hipLaunchKernelGGL(swin_mlp_bwd_mx_pack_kernel, dim3(cdiv(MlpMxB(C).PACK_ITEMS, 256)), dim3(256), 0, STREAM, static_cast<const uint8_t*>(w1q), static_cast<const uint8_t*>(w1s),
                     static_cast<const uint8_t*>(w2tq), static_cast<const uint8_t*>(w2ts), static_cast<const uint8_t*>(w1tq), static_cast<const uint8_t*>(w1ts),
                     static_cast<uint8_t*>(packs), C);
  return check_launch("sv_swin_mlp_bwd_mx_pack");
}

extern "C" int sv_swin_mlp_bwd_mx(const void* x1, const void* dx2, void* dx1, const float* ln_g, const float* ln_b, const void* packs_mx, const float* b1,
                                  const float* row_scale, int rows_per_scale, float* dgamma, float* dbeta, long long M, int C, float eps, void* stream) {
  if (int rc = mlp_mx_check("sv_swin_mlp_bwd_mx", x1 && dx2 && dx1 && ln_g && ln_b && packs_mx && b1 && dgamma && dbeta, mlp_bwd_mx_supported(C), "",
                            (uintptr_t)x1 | (uintptr_t)dx2 | (uintptr_t)dx1 | (uintptr_t)packs_mx | (uintptr_t)ln_g | (uintptr_t)ln_b, M, C, rows_per_scale))
    return rc;
  MlpMxBArgs a{};
  a.x1 = static_cast<const __bf16*>(x1); a.dx2 = static_cast<const __bf16*>(dx2); a.out = static_cast<__bf16*>(dx1);
  a.ln_g = ln_g; a.ln_b = ln_b; a.eps = eps; a.packs = static_cast<const uint8_t*>(packs_mx); a.b1 = b1;
  a.row_scale = row_scale; a.rows_per_scale = rows_per_scale; a.dgamma = dgamma; a.dbeta = dbeta; a.M = M;
  return mlp_mx_launch("sv_swin_mlp_bwd_mx", swin_mlp_bwd_mx_kernel<96, MX_NW, MX_NTT>, swin_mlp_bwd_mx_kernel<128, MX_NW, MX_NTT>, C, a, STREAM,
                       swin_mlp_bwd_mx_launches);
}

// ---- MXFP8 weight gradients ---------------------------------------------------------------------------------------------------------
static std::atomic<long long> swin_mlp_wgrad_mx_launches{0};
extern "C" long long sv_swin_mlp_wgrad_mx_launches(void) { return swin_mlp_wgrad_mx_launches.load(std::memory_order_relaxed); }
extern "C" int sv_swin_mlp_wgrad_mx_supported(int C) { return mlp_wgrad_mx_supported(C) ? 1 : 0; }

extern "C" int sv_swin_mlp_wgrad_mx(const void* x1, const void* dx2, const float* ln_g, const float* ln_b, const void* w1q, const void* w1s, const void* w2tq,
                                    const void* w2ts, const float* b1, const float* row_scale, int rows_per_scale, float* dw1, float* db1, float* dw2,
                                    float* db2, long long M, int C, float eps, void* stream) {
  const char* who = "sv_swin_mlp_wgrad_mx";
  SV_REQUIRE(x1 && dx2 && ln_g && ln_b && w1q && w1s && w2tq && w2ts && b1 && dw1 && db1 && dw2 && db2, "%s: null pointer", who);
  SV_REQUIRE(mlp_wgrad_mx_supported(C), "%s: unsupported C=%d", who, C);
  SV_REQUIRE(M > 0 && M < (1ll << 31), "%s: M=%lld out of range", who, M);
  SV_REQUIRE((((uintptr_t)x1 | (uintptr_t)dx2 | (uintptr_t)w1q | (uintptr_t)w2tq) & 15) == 0, "%s: x1, dx2, w1q and w2tq must be 16-byte aligned", who);
  SV_REQUIRE((((uintptr_t)w1s | (uintptr_t)w2ts) & 3) == 0, "%s: w1s and w2ts must be 4-byte aligned", who);
  SV_REQUIRE(rows_per_scale > 0, "%s: rows_per_scale must be positive", who);
  SV_REQUIRE(!row_scale || rows_per_scale >= 128, "%s: rows_per_scale (%d) must be >= 128 with row_scale (the rule of sv_swin_mlp_wgrad)", who, rows_per_scale);
  MlpMxWArgs a{};
  a.x1 = static_cast<const __bf16*>(x1); a.dx2 = static_cast<const __bf16*>(dx2); a.ln_g = ln_g; a.ln_b = ln_b; a.eps = eps;
  a.w1q = static_cast<const uint8_t*>(w1q); a.w1s = static_cast<const uint8_t*>(w1s); a.w2tq = static_cast<const uint8_t*>(w2tq); a.w2ts = static_cast<const uint8_t*>(w2ts);
  a.b1 = b1; a.row_scale = row_scale; a.rows_per_scale = rows_per_scale; a.dw1 = dw1; a.db1 = db1; a.dw2 = dw2; a.db2 = db2; a.M = M;
  // hidden groups x token splits as sv_swin_mlp_wgrad; splits start at multiples of the 128-token tile, so the 32-token blocks count from token 0
  a.HG = (4 * C) / (MXW_NW * 16);
  long long splits = 256 / a.HG;
  long long tps = (M + splits - 1) / splits; tps = (tps + MXW_TT - 1) / MXW_TT * MXW_TT;
  splits = (M + tps - 1) / tps;
  a.tok_per_split = (int)tps;
  if (C == 96) hipLaunchKernelGGL(swin_mlp_wgrad_mx_kernel<96>, dim3((unsigned)(splits * a.HG)), dim3(MXW_NW * 64), 0, STREAM, a);
  else hipLaunchKernelGGL(swin_mlp_wgrad_mx_kernel<128>, dim3((unsigned)(splits * a.HG)), dim3(MXW_NW * 64), 0, STREAM, a);
  const int rc = check_launch(who);
  if (rc == SV_OK) swin_mlp_wgrad_mx_launches.fetch_add(1, std::memory_order_relaxed);
  return rc;
}
