// Implicit-GEMM contraction engine for gfx950 (MFMA 16x16x4 f32 / 16x16x32 bf16, fp32 accumulate).
//
// One kernel family serves every Linear / Conv2d / Conv3d / ConvTranspose3d of the SwinVox path:
//   igemm_kernel<BF16, TCONV, tile>  out[row, co] = epilogue( sum_k A[row, k] * W[co, k] )
//       A is never materialised: k = (tap, ci) is decoded to a gathered input position on the fly
//       (channels-last activations, so the ci run of one tap is contiguous -> 16-byte loads).  The tap
//       coordinates of a thread's k-chunk advance incrementally from K-step to K-step (no integer division
//       in the main loop).  TCONV = stride-s transposed gather, decomposed into s^3 output parity classes
//       (blockIdx.z) so that only taps that really contribute are visited.
//   wgrad_kernel<BF16, tile>         dw[ca, cg, tap] += sum_r anchor[r, ca] * gathered[pos(r, tap), cg]
//       reduction over positions split across blockIdx.z.  Both operands are stored in LDS as they lie in HBM
//       ([position][channel], 8/16-byte stores); the MFMA fragments, which need 8 consecutive POSITIONS per lane,
//       are produced by the transposing LDS read ds_read_b64_tr_b16 (bf16) or plain strided reads (fp32).
// Tile shapes (256 threads = 4 waves): 128x64 default, 128x128 for wide outputs, 128x16 for the <=16-channel
// 3-D tail (merger / decoder head / refiner head), so that narrow layers do not pay for padded MFMA columns.
// K-step 32 (fp32) or 64 (bf16); global->register prefetch of step k+1 under the MFMAs of step k
// (register-staged: the gather needs per-element predication and an fp32->bf16 conversion).
#include "common.h"
#include "conv_halo.h"
#include <stdlib.h>
#include <atomic>
#include <mutex>

namespace sv {

constexpr int PAD_F32 = 4;   // floats
#ifndef SV_PAD_BF16
#define SV_PAD_BF16 8
#endif
constexpr int PAD_BF16 = SV_PAD_BF16;  // bf16     (both = 16 bytes: keeps every row 16-byte aligned)

struct Geom {
  int N, Di, Hi, Wi, Do, Ho, Wo, Ci, Co, kd, kh, kw, sd, sh, sw, pd, ph, pw, ldi;
};
struct Epi {   // residual / pre_act / act_grad_src are activations (element type AT of the kernel)
  const float* bias; const void* residual; int ldr; const float* row_scale; int rows_per_scale;
  void* pre_act; double* stats; int act; float slope; const void* act_grad_src; int act_grad_kind; int ldc; int col_off;
};
struct ClassInfo {  // one output parity class of a transposed gather
  int o0[3];        // first output index of the class per axis
  int cnt[3];       // outputs of the class per axis
  int ib0[3];       // (o0 + p - r)/s : gathered index for j = 0, t = 0
  int r[3];         // residue = first kernel index of the class
  int T[3];         // taps of the class per axis
};
struct IGemmArgs {
  const void* x; const void* w; void* y;   // x, y: activations (AT); w: packed weights (fp32, or bf16 with bf16 activations)
  Geom g; Epi e;
  int Ktot;         // row length of packed weights = taps_total * Ci
  ClassInfo cls[8];
};

template <bool BF16> struct Cfg {
  typedef float T; static constexpr int BK = 32; static constexpr int PAD = PAD_F32;
};
template <> struct Cfg<true> {
  typedef __bf16 T; static constexpr int BK = 64; static constexpr int PAD = PAD_BF16;
};

// wave grid WM x WN (WM*WN == 4), each wave MT x NT tiles of 16x16
template <int WM_, int WN_, int MT_, int NT_> struct Tile {
  static constexpr int WM = WM_, WN = WN_, MT = MT_, NT = NT_;
  static constexpr int BM = WM_ * MT_ * 16, BN = WN_ * NT_ * 16;
  static constexpr int NW = WM_ * WN_, NTHR = NW * 64;
};
typedef Tile<4, 2, 2, 2> TileDefault;   // 128 x 64, 8 waves of 32x32 (few registers per thread -> 2-3 workgroups per CU)
typedef Tile<2, 4, 4, 2> TileBig;       // 128 x 128, 8 waves (512 threads): halves the A re-reads of TileDefault at equal registers
typedef Tile<4, 1, 2, 1> TileNarrow;    // 128 x 16
typedef Tile<4, 2, 2, 3> Tile96;        // 128 x 96, 8 waves: the Swin channel counts are multiples of 96 (no padded columns for 96 / 192 / 288)

__device__ __forceinline__ void store4(float* dst, float4 v) { *reinterpret_cast<float4*>(dst) = v; }
__device__ __forceinline__ void store4(__bf16* dst, float4 v) {
  bf16x4 b;
  b[0] = (__bf16)v.x; b[1] = (__bf16)v.y; b[2] = (__bf16)v.z; b[3] = (__bf16)v.w;
  *reinterpret_cast<bf16x4*>(dst) = b;
}
__device__ __forceinline__ void store4(__bf16* dst, bf16x4 v) { *reinterpret_cast<bf16x4*>(dst) = v; }   // bf16 storage: no conversion
__device__ __forceinline__ void store4(float* dst, bf16x4 v) {
  *reinterpret_cast<float4*>(dst) = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}
__device__ __forceinline__ void store4(__bf16* dst, bf16x8 v) { *reinterpret_cast<bf16x8*>(dst) = v; }   // 16-byte operand chunk
__device__ __forceinline__ void store4(float* dst, bf16x8 v) {   // never selected (bf16 storage implies bf16 MFMA operands)
#pragma unroll
  for (int i = 0; i < 8; ++i) dst[i] = (float)v[i];
}

// ---- MFMA over one K-step slab, operands stored [row][k] (k contiguous) ---------------------------
// The B fragment goes in as the MFMA's first operand: the accumulator then is the TRANSPOSED 16x16 block, i.e. lane (lr, lg)
// holds C[row = lr][cols lg*4 .. lg*4+3] - four consecutive columns, which the epilogue stages with one 16-byte LDS write.
template <bool BF16, int MT, int NT>
__device__ __forceinline__ void mma_slab(const typename Cfg<BF16>::T* As, const typename Cfg<BF16>::T* Bs,
                                         int arow0, int brow0, int lane, f32x4 (&acc)[MT][NT]) {
  constexpr int BK = Cfg<BF16>::BK, LD = BK + Cfg<BF16>::PAD;
  const int lr = lane & 15, lg = lane >> 4;
  if constexpr (BF16) {
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      bf16x8 a[MT], b[NT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) a[mt] = *reinterpret_cast<const bf16x8*>(As + (arow0 + mt * 16 + lr) * LD + ks * 32 + lg * 8);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) b[nt] = *reinterpret_cast<const bf16x8*>(Bs + (brow0 + nt * 16 + lr) * LD + ks * 32 + lg * 8);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[nt], a[mt], acc[mt][nt], 0, 0, 0);
    }
  } else {
#pragma unroll
    for (int kk = 0; kk < BK / 4; ++kk) {
      float a[MT], b[NT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) a[mt] = As[(arow0 + mt * 16 + lr) * LD + kk * 4 + lg];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) b[nt] = Bs[(brow0 + nt * 16 + lr) * LD + kk * 4 + lg];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[nt], a[mt], acc[mt][nt], 0, 0, 0);
    }
  }
}

// ---- MFMA over one K-step slab, operands stored [k][col] (as they lie in HBM) -----------------------
// bf16: ds_read_b64_tr_b16 delivers, per 16-lane group, a 4(k) x 16(col) block column-major: lane i of the group
// gets column i, rows 0..3; lane 4q+p supplies the address of row q, columns 4p..4p+3.  Two reads give the 8
// consecutive k of the 16x16x32 fragment (k = 8*(lane>>4) + j).
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
template <bool BF16, int MT, int NT, int LDA, int LDB>
__device__ __forceinline__ void mma_slab_km(const typename Cfg<BF16>::T* As, const typename Cfg<BF16>::T* Bs,
                                            int acol0, int bcol0, int lane, f32x4 (&acc)[MT][NT]) {
  constexpr int BK = Cfg<BF16>::BK;
  const int lr = lane & 15, lg = lane >> 4;
  if constexpr (BF16) {
    const int q = lr >> 2, pp = lr & 3;
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      bf16x8 a[MT], b[NT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const __bf16* src = As + (ks * 32 + lg * 8 + q) * LDA + acol0 + mt * 16 + pp * 4;
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(src));
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(src + 4 * LDA));
        a[mt] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const __bf16* src = Bs + (ks * 32 + lg * 8 + q) * LDB + bcol0 + nt * 16 + pp * 4;
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(src));
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(src + 4 * LDB));
        b[nt] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
    }
  } else {
#pragma unroll
    for (int kk = 0; kk < BK / 4; ++kk) {
      float a[MT], b[NT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) a[mt] = As[(kk * 4 + lg) * LDA + acol0 + mt * 16 + lr];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) b[nt] = Bs[(kk * 4 + lg) * LDB + bcol0 + nt * 16 + lr];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
    }
  }
}

// XCD-aware, bijective remap of the linear workgroup id: blocks are dealt round-robin over the 8 XCDs (b and b+8 share an
// L2), so give every XCD one CONTIGUOUS chunk of the logical tile order -> tiles that share an operand panel (all output-
// column tiles of one activation row panel; all (channel, tap) tiles of one position range in wgrad) hit the same L2.
__device__ __forceinline__ int xcd_remap(int bid, int nb) {
  const int q = nb >> 3, r = nb & 7, xcd = bid & 7, idx = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// row index -> (n, d, h, w) of a grid; spatial == 1 (Linear) needs no division at all
__device__ __forceinline__ void decode_row(int m, int c0, int c1, int c2, int& n_, int& d_, int& h_, int& w_) {
  if (c0 * c1 * c2 == 1) { n_ = m; d_ = h_ = w_ = 0; return; }
  w_ = m % c2; int t = m / c2;
  h_ = t % c1; t /= c1;
  d_ = t % c0; n_ = t / c0;
}

// cooperative row pass of the tile epilogue (see tile_epilogue): thread (cr, cw) owns CV consecutive columns of row cr + k*CRPP
template <bool BF16, bool TCONV, typename TL, typename AT, int CV>
__device__ __forceinline__ void epilogue_rows(const IGemmArgs& p, const ClassInfo& ci, int cnt0, int cnt1, int cnt2, const float* Cs, float* red,
                                              int row0, int col0, int Mrows) {
  constexpr int BM = TL::BM, BN = TL::BN, NTHR = TL::NTHR, NW = TL::NW, LDC = BN + 4;
  constexpr int CW = BN / CV, CRPP = NTHR / CW, CPASS = (BM + CRPP - 1) / CRPP;   // 96-wide tile: idle threads past CRPP * CW
  const Geom& g = p.g;
  const Epi& e = p.e;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  AT* __restrict__ Y = static_cast<AT*>(p.y);
  const int cw = tid % CW, cr = tid / CW;
  const int n0 = col0 + cw * CV;
  const bool vec_out = ((e.ldc | e.col_off | g.Co) & (CV - 1)) == 0 && (!e.residual || (e.ldr & (CV - 1)) == 0);
  float bias[CV];
#pragma unroll
  for (int j = 0; j < CV; ++j) bias[j] = (e.bias && n0 + j < g.Co) ? e.bias[n0 + j] : 0.f;
  float s1[CV], s2[CV];
#pragma unroll
  for (int j = 0; j < CV; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
  if (n0 < g.Co && cr < CRPP) {
#pragma unroll 2
    for (int ps_ = 0; ps_ < CPASS; ++ps_) {
      const int row = cr + CRPP * ps_;
      const int m = row0 + row;
      if (row >= BM || m >= Mrows) break;
      int pos = m;
      if constexpr (TCONV) {
        int n_, d_, h_, w_;
        decode_row(m, cnt0, cnt1, cnt2, n_, d_, h_, w_);
        const int od = ci.o0[0] + g.sd * d_, oh = ci.o0[1] + g.sh * h_, ow = ci.o0[2] + g.sw * w_;
        pos = ((n_ * g.Do + od) * g.Ho + oh) * g.Wo + ow;
      }
      float v[CV];
#pragma unroll
      for (int q = 0; q < CV / 4; ++q) {
        const float4 c = *reinterpret_cast<const float4*>(Cs + row * LDC + cw * CV + q * 4);
        v[q * 4] = c.x + bias[q * 4]; v[q * 4 + 1] = c.y + bias[q * 4 + 1]; v[q * 4 + 2] = c.z + bias[q * 4 + 2]; v[q * 4 + 3] = c.w + bias[q * 4 + 3];
      }
      const size_t o = (size_t)pos * e.ldc + e.col_off + n0;
      const float sc = (e.residual && e.row_scale) ? e.row_scale[pos / e.rows_per_scale] : 1.f;
      if (vec_out) {   // Co % CV == 0 => the whole vector is in range
        if (e.act_grad_src) {
          float a[CV];
          ldnf<CV>(static_cast<const AT*>(e.act_grad_src) + o, a);
          if (BF16 && e.act_grad_kind == SV_ACT_GELU) {      // pairs: packed fp32 math (common.h)
#pragma unroll
            for (int j = 0; j < CV; j += 2) {
              const f32x2 dg = gelu_grad_fast2((f32x2){a[j], a[j + 1]});
              v[j] *= dg[0]; v[j + 1] *= dg[1];
            }
          } else {
#pragma unroll
            for (int j = 0; j < CV; ++j) v[j] *= act_grad_t<BF16>(a[j], e.act_grad_kind, e.slope);
          }
        }
        if (e.pre_act) stnf<CV>(static_cast<AT*>(e.pre_act) + o, v);
        if (BF16 && e.act == SV_ACT_GELU) {
#pragma unroll
          for (int j = 0; j < CV; j += 2) {
            const f32x2 gl = gelu_fast2((f32x2){v[j], v[j + 1]});
            v[j] = gl[0]; v[j + 1] = gl[1];
          }
        } else {
#pragma unroll
          for (int j = 0; j < CV; ++j) v[j] = apply_act_t<BF16>(v[j], e.act, e.slope);
        }
        if (e.residual) {
          float r[CV];
          ldnf<CV>(static_cast<const AT*>(e.residual) + (size_t)pos * e.ldr + n0, r);
#pragma unroll
          for (int j = 0; j < CV; ++j) v[j] = r[j] + sc * v[j];
        }
        stnf<CV>(Y + o, v);
#pragma unroll
        for (int j = 0; j < CV; ++j) { s1[j] += v[j]; s2[j] += v[j] * v[j]; }
      } else {
#pragma unroll
        for (int j = 0; j < CV; ++j) {
          if (n0 + j < g.Co) {
            float t = v[j];
            if (e.act_grad_src) t *= act_grad_t<BF16>(ldf(static_cast<const AT*>(e.act_grad_src) + o + j), e.act_grad_kind, e.slope);
            if (e.pre_act) stf(static_cast<AT*>(e.pre_act) + o + j, t);
            t = apply_act_t<BF16>(t, e.act, e.slope);
            if (e.residual) t = ldf(static_cast<const AT*>(e.residual) + (size_t)pos * e.ldr + n0 + j) + sc * t;
            stf(Y + o + j, t);
            s1[j] += t; s2[j] += t * t;
          }
        }
      }
    }
  }
  if (e.stats) {  // per-channel sum / sumsq of what was stored: lanes sharing a column group, then the waves, then ONE
                  // double atomic per column per workgroup into one of SV_BN_SLOTS accumulator slots (spreads contention)
    // lanes that share a column group (lane % CW): DPP row rotations and v_permlane swaps (common.h) - the 2 x CV x log2(64 / CW)
    // __shfl_xor round trips through the LDS crossbar this used to be cost the BatchNorm producers up to 20 % of their time
#pragma unroll
    for (int j = 0; j < CV; ++j) {
      if constexpr (CW <= 1) { s1[j] = lane_step_add<1>(s1[j]); s2[j] = lane_step_add<1>(s2[j]); }
      if constexpr (CW <= 2) { s1[j] = lane_step_add<2>(s1[j]); s2[j] = lane_step_add<2>(s2[j]); }
      if constexpr (CW <= 4) { s1[j] = lane_step_add<4>(s1[j]); s2[j] = lane_step_add<4>(s2[j]); }
      if constexpr (CW <= 8) { s1[j] = lane_step_add<8>(s1[j]); s2[j] = lane_step_add<8>(s2[j]); }
      if constexpr (CW <= 16) { s1[j] = lane_step_add<16>(s1[j]); s2[j] = lane_step_add<16>(s2[j]); }
      if constexpr (CW <= 32) { s1[j] = lane_step_add<32>(s1[j]); s2[j] = lane_step_add<32>(s2[j]); }
    }
    if ((lane / CW) == 0 || CW >= 64) {
#pragma unroll
      for (int j = 0; j < CV; ++j) { red[(wave * BN + cw * CV + j) * 2] = s1[j]; red[(wave * BN + cw * CV + j) * 2 + 1] = s2[j]; }
    }
    __syncthreads();
    if (tid < BN && col0 + tid < g.Co) {
      float a = 0.f, b = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) { a += red[(w * BN + tid) * 2]; b += red[(w * BN + tid) * 2 + 1]; }
      double* st = e.stats + (size_t)((row0 / BM) % SV_BN_SLOTS) * 2 * g.Co;
      atomicAdd(st + col0 + tid, (double)a);
      atomicAdd(st + g.Co + col0 + tid, (double)b);
    }
  }
}

template <int CTRL> __device__ __forceinline__ float gw_dpp_add(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// sum over the 16 lanes of a DPP row; valid in lane 15 of the row (row_shr 1, 2, 4, 8 with zero fill)
__device__ __forceinline__ float row16_total(float v) {
  v = gw_dpp_add<0x111>(v); v = gw_dpp_add<0x112>(v); v = gw_dpp_add<0x114>(v); v = gw_dpp_add<0x118>(v);
  return v;
}
// bf16 rows of the output (and of every tensor the epilogue reads or writes beside it) start on 16-byte boundaries and are whole 8-column pieces
__host__ __device__ __forceinline__ bool rows_16_byte_aligned(const IGemmArgs& p) {
  const Epi& e = p.e;
  return ((e.ldc | e.col_off | p.g.Co) & 7) == 0 && (!e.residual || (e.ldr & 7) == 0) &&
         (((uintptr_t)p.y | (uintptr_t)e.residual | (uintptr_t)e.pre_act | (uintptr_t)e.act_grad_src) & 15) == 0;
}
// ------------------------------------------------------------------------------------------------
// tile epilogue shared by the gather kernels: accumulators -> LDS tile -> cooperative, row-contiguous vector reads/writes with
// the fused bias / activation(-gradient) / residual / pre-activation copy / per-channel statistics.  Every wave must have
// finished reading the operand tiles (Cs aliases them) before the call.
// ------------------------------------------------------------------------------------------------
template <bool BF16, bool TCONV, typename TL, typename AT>
__device__ __forceinline__ void tile_epilogue(const IGemmArgs& p, const ClassInfo& ci, int cnt0, int cnt1, int cnt2, float* Cs, float* red,
                                              const f32x4 (&acc)[TL::MT][TL::NT], int row0, int col0, int Mrows) {
  constexpr int BN = TL::BN, MT = TL::MT, NT = TL::NT, LDC = BN + 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / TL::WN, wn = wave % TL::WN;
  // bf16 storage with 8-aligned rows: 16 bytes per lane
  bool wide = false;
  if constexpr (sizeof(AT) == 2 && BN % 8 == 0) wide = rows_16_byte_aligned(p);
  {
    const int lr = lane & 15, lg = lane >> 4;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        // accumulator layout of mma_slab: row lr, columns lg*4 .. lg*4+3
        *reinterpret_cast<f32x4*>(Cs + ((wm * MT + mt) * 16 + lr) * LDC + (wn * NT + nt) * 16 + lg * 4) = acc[mt][nt];
  }
  __syncthreads();
  // row pass: CV consecutive columns per thread.  bf16 storage with 8-aligned rows moves 16 bytes per lane (half the
  // global-memory instructions, 1 KB per wave store); everything else keeps 4 columns per thread.
  if constexpr (sizeof(AT) == 2 && BN % 8 == 0) {
    if (wide) { epilogue_rows<BF16, TCONV, TL, AT, 8>(p, ci, cnt0, cnt1, cnt2, Cs, red, row0, col0, Mrows); return; }
  }
  epilogue_rows<BF16, TCONV, TL, AT, 4>(p, ci, cnt0, cnt1, cnt2, Cs, red, row0, col0, Mrows);
}

// ------------------------------------------------------------------------------------------------
// forward / data-gradient kernel
// ------------------------------------------------------------------------------------------------
// AT = activation storage type, WT = packed-weight type, VEC = elements per operand load (4, or 8 = 16 bytes of bf16)
template <bool BF16, bool TCONV, typename TL, typename AT, typename WT, int VEC>
__global__ __launch_bounds__(TL::NTHR, TL::NTHR == 512 ? 4 : 2) void igemm_kernel(const IGemmArgs p) {
  typedef typename Cfg<BF16>::T LT;
  typedef typename VecN<AT, VEC>::type AV;
  typedef typename VecN<WT, VEC>::type WV;
  const AT* __restrict__ X = static_cast<const AT*>(p.x);
  const WT* __restrict__ Wt = static_cast<const WT*>(p.w);
  AT* __restrict__ Y = static_cast<AT*>(p.y);
  constexpr int BK = Cfg<BF16>::BK, LD = BK + Cfg<BF16>::PAD;
  constexpr int BM = TL::BM, BN = TL::BN, MT = TL::MT, NT = TL::NT;
  constexpr int TPR = BK / VEC;        // threads per tile row (one VEC-element chunk each)
  constexpr int NTHR = TL::NTHR, NW = TL::NW;
  constexpr int RPP = NTHR / TPR;      // rows per pass
  constexpr int NA = BM / RPP;
  constexpr int NB = (BN + RPP - 1) / RPP;
  constexpr int LDC = BN + 4;          // fp32 staging tile of the epilogue (aliases the operand tiles)
  constexpr int STAGE = (BM + BN) * LD;   // operand tiles are double-buffered: one barrier per K step
  constexpr int AB_BYTES = 2 * STAGE * (int)sizeof(LT), C_BYTES = BM * LDC * 4;
  __shared__ __attribute__((aligned(16))) char smem[AB_BYTES > C_BYTES ? AB_BYTES : C_BYTES];
  __shared__ float red[NW * BN * 2];
  LT* As = reinterpret_cast<LT*>(smem);
  LT* Bs = As + BM * LD;
  float* Cs = reinterpret_cast<float*>(smem);

  const Geom& g = p.g;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / TL::WN, wn = wave % TL::WN;

  int cnt0, cnt1, cnt2, T0, T1, T2;
  ClassInfo ci;
  if constexpr (TCONV) {
    ci = p.cls[blockIdx.y];
    cnt0 = ci.cnt[0]; cnt1 = ci.cnt[1]; cnt2 = ci.cnt[2];
    T0 = ci.T[0]; T1 = ci.T[1]; T2 = ci.T[2];
  } else {
    cnt0 = g.Do; cnt1 = g.Ho; cnt2 = g.Wo;
    T0 = g.kd; T1 = g.kh; T2 = g.kw;
  }
  const int Mrows = g.N * cnt0 * cnt1 * cnt2;
  const int K = T0 * T1 * T2 * g.Ci;
  // logical tile order: output-column tile fastest (the column tiles of one row panel run together and share A in L2)
  const int tiles_n = (g.Co + BN - 1) / BN;
  const int tlin = xcd_remap(blockIdx.x, gridDim.x);
  const int row0 = (tlin / tiles_n) * BM;
  if (row0 >= Mrows) return;
  const int col0 = (tlin % tiles_n) * BN;

  // ---- per-thread loader state -----------------------------------------------------------------
  const int kq = (tid % TPR) * VEC;
  const int rb = tid / TPR;
  int a_n[NA], a_d[NA], a_h[NA], a_w[NA];
  bool a_ok[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    int m = row0 + rb + RPP * i;
    a_ok[i] = m < Mrows;
    if (!a_ok[i]) m = 0;
    int n_, d_, h_, w_;
    decode_row(m, cnt0, cnt1, cnt2, n_, d_, h_, w_);
    a_n[i] = n_;
    if constexpr (TCONV) { a_d[i] = ci.ib0[0] + d_; a_h[i] = ci.ib0[1] + h_; a_w[i] = ci.ib0[2] + w_; }   // gathered idx = this - t
    else { a_d[i] = d_ * g.sd - g.pd; a_h[i] = h_ * g.sh - g.ph; a_w[i] = w_ * g.sw - g.pw; }              // gathered idx = this + t
  }
  const bool vec_ok = (g.Ci % VEC) == 0 && (g.ldi % VEC) == 0;
  // running tap state of this thread's k-chunk (vector path): channel offset kc inside the tap, tap coords
  int kc = 0, tw = 0, th = 0, td = 0, kcur = kq;
  if (vec_ok && K > 0) {
    const int tap = kq / g.Ci;
    kc = kq - tap * g.Ci;
    tw = tap % T2; const int t2 = tap / T2; th = t2 % T1; td = t2 / T1;
  }

  AV ra[NA];
  WV rbv[NB];
  auto load_tile = [&]() {   // loads the tile at the running k position, then advances the state by BK
    if (vec_ok) {
      const bool kok = td < T0;
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        int id, ih, iw;
        if constexpr (TCONV) { id = a_d[i] - td; ih = a_h[i] - th; iw = a_w[i] - tw; }
        else { id = a_d[i] + td; ih = a_h[i] + th; iw = a_w[i] + tw; }
#ifdef SV_IG_PROBE_CHEAPADDR     // probe build (wrong results): what the gather's coordinate / bounds / address arithmetic costs the K loop
        const bool ok = kok && a_ok[i];
        if (ok) {
          const size_t off = (size_t)(row0 + rb + RPP * i) * (size_t)g.ldi + kc;
          (void)id; (void)ih; (void)iw;
          ra[i] = VecN<AT, VEC>::load(X + off);
#else
        const bool ok = kok && a_ok[i] && (unsigned)id < (unsigned)g.Di && (unsigned)ih < (unsigned)g.Hi && (unsigned)iw < (unsigned)g.Wi;
        if (ok) {
          const size_t off = ((((size_t)a_n[i] * g.Di + id) * g.Hi + ih) * g.Wi + iw) * (size_t)g.ldi + kc;
          ra[i] = VecN<AT, VEC>::load(X + off);
#endif
        } else {
          ra[i] = VecN<AT, VEC>::zero();
        }
      }
      // weights: [Co][taps_total][Ci]; TCONV maps the class-local tap to its kernel index
      size_t woff;
      if constexpr (TCONV) {
        const int kd_ = ci.r[0] + g.sd * td, kh_ = ci.r[1] + g.sh * th, kw_ = ci.r[2] + g.sw * tw;
        woff = (size_t)((kd_ * g.kh + kh_) * g.kw + kw_) * g.Ci + kc;
      } else {
        woff = (size_t)kcur;
      }
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int nl = rb + RPP * i, n = col0 + nl;
        if (nl < BN && n < g.Co && kok) rbv[i] = VecN<WT, VEC>::load(Wt + (size_t)n * p.Ktot + woff);
        else rbv[i] = VecN<WT, VEC>::zero();
      }
      // advance
      kcur += BK; kc += BK;
      while (kc >= g.Ci) {
        kc -= g.Ci;
        if (++tw == T2) { tw = 0; if (++th == T1) { th = 0; ++td; } }
      }
    } else if constexpr (VEC == 4) {  // scalar path: any Ci (stem Ci=3, refiner head Ci=1 ...), per-element tap decode
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int kk = kcur + j;
          const int tap = kk / g.Ci, c = kk - tap * g.Ci;
          const int tw_ = tap % T2; const int t2 = tap / T2; const int th_ = t2 % T1; const int td_ = t2 / T1;
          int id, ih, iw;
          if constexpr (TCONV) { id = a_d[i] - td_; ih = a_h[i] - th_; iw = a_w[i] - tw_; }
          else { id = a_d[i] + td_; ih = a_h[i] + th_; iw = a_w[i] + tw_; }
          const bool ok = kk < K && a_ok[i] && (unsigned)id < (unsigned)g.Di && (unsigned)ih < (unsigned)g.Hi && (unsigned)iw < (unsigned)g.Wi;
          v[j] = ok ? ldf(X + ((((size_t)a_n[i] * g.Di + id) * g.Hi + ih) * g.Wi + iw) * (size_t)g.ldi + c) : 0.f;
        }
        ra[i] = VecN<AT, 4>::make(v[0], v[1], v[2], v[3]);
      }
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int nl = rb + RPP * i, n = col0 + nl;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int kk = kcur + j;
          float val = 0.f;
          if (nl < BN && n < g.Co && kk < K) {
            int kidx = kk;
            if constexpr (TCONV) {
              const int tap = kk / g.Ci, c = kk - tap * g.Ci;
              const int tw_ = tap % T2; const int t2 = tap / T2; const int th_ = t2 % T1; const int td_ = t2 / T1;
              const int kd_ = ci.r[0] + g.sd * td_, kh_ = ci.r[1] + g.sh * th_, kw_ = ci.r[2] + g.sw * tw_;
              kidx = ((kd_ * g.kh + kh_) * g.kw + kw_) * g.Ci + c;
            }
            val = (float)Wt[(size_t)n * p.Ktot + kidx];
          }
          v[j] = val;
        }
        rbv[i] = VecN<WT, 4>::make(v[0], v[1], v[2], v[3]);
      }
      kcur += BK;
    }
  };
  auto store_tile = [&](int buf) {
    LT* A_ = As + buf * STAGE;
    LT* B_ = Bs + buf * STAGE;
#pragma unroll
    for (int i = 0; i < NA; ++i) store4(A_ + (rb + RPP * i) * LD + kq, ra[i]);
#pragma unroll
    for (int i = 0; i < NB; ++i)
      if (rb + RPP * i < BN) store4(B_ + (rb + RPP * i) * LD + kq, rbv[i]);
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nk = (K + BK - 1) / BK;
  if (nk > 0) {
    load_tile();
    store_tile(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      if (kt + 1 < nk) load_tile();
      mma_slab<BF16, MT, NT>(As + cur * STAGE, Bs + cur * STAGE, wm * MT * 16, wn * NT * 16, lane, acc);
      if (kt + 1 < nk) store_tile(cur ^ 1);
      __syncthreads();
    }
  }

#ifdef SV_IG_PROBE_NOEPI      // probe build: what the tile costs without its epilogue (one store keeps the accumulators alive)
  if (acc[0][0][0] == 12345.678f) static_cast<AT*>(p.y)[0] = (AT)acc[0][0][1];
  return;
#endif
  tile_epilogue<BF16, TCONV, TL, AT>(p, ci, cnt0, cnt1, cnt2, Cs, red, acc, row0, col0, Mrows);
}

// ------------------------------------------------------------------------------------------------
// persistent dense kernel (bf16 MFMA, bf16 storage): Linear layers and 1x1 / stride-1 convolutions, i.e. gathered row m
// is the row m*ldi of x.  A tile with few K steps spends most of its ~10 us on everything around the MFMA loop
// (workgroup start, first-slab latency, epilogue); here a workgroup walks tiles t = b, b + G, ... and issues the loads of
// the NEXT tile's first operand slab before the epilogue of the current one, so that latency hides behind the epilogue
// and the start-up cost is paid once.  Same tiles, loader mapping, LDS layout and epilogue as igemm_kernel.
// ------------------------------------------------------------------------------------------------
template <typename TL, typename AT, typename WT, int VEC>
__global__ __launch_bounds__(TL::NTHR, TL::NTHR >= 512 ? 4 : 2) void gemm_dense_kernel(const IGemmArgs p, int ntiles) {
  typedef __bf16 LT;
  constexpr int BK = Cfg<true>::BK, LD = BK + Cfg<true>::PAD;
  constexpr int BM = TL::BM, BN = TL::BN, MT = TL::MT, NT = TL::NT;
  constexpr int TPR = BK / VEC, NTHR = TL::NTHR, NW = TL::NW, RPP = NTHR / TPR;
  constexpr int NA = BM / RPP, NB = (BN + RPP - 1) / RPP, LDC = BN + 4;
  constexpr int STAGE = (BM + BN) * LD;
  constexpr int AB_BYTES = 2 * STAGE * (int)sizeof(LT), C_BYTES = BM * LDC * 4;
  __shared__ __attribute__((aligned(16))) char smem[AB_BYTES > C_BYTES ? AB_BYTES : C_BYTES];
  __shared__ float red[NW * BN * 2];
  typedef typename VecN<AT, VEC>::type AV;
  typedef typename VecN<WT, VEC>::type WV;
  LT* As = reinterpret_cast<LT*>(smem);
  LT* Bs = As + BM * LD;
  float* Cs = reinterpret_cast<float*>(smem);
  const AT* __restrict__ X = static_cast<const AT*>(p.x);
  const WT* __restrict__ Wt = static_cast<const WT*>(p.w);
  const Geom& g = p.g;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / TL::WN, wn = wave % TL::WN;
  const int Mrows = g.N * g.Do * g.Ho * g.Wo, K = g.Ci;
  const int tiles_n = (g.Co + BN - 1) / BN, nk = (K + BK - 1) / BK;
  const int kq = (tid % TPR) * VEC, rb = tid / TPR;
  const ClassInfo ci{};

  AV ra[NA];
  WV rbv[NB];
  auto load_slab = [&](int row0, int col0, int k0) {
    const bool kok = k0 + kq < K;                       // K % VEC == 0: a chunk is whole or absent
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int m = row0 + rb + RPP * i;
      ra[i] = (kok && m < Mrows) ? VecN<AT, VEC>::load(X + (size_t)m * g.ldi + k0 + kq) : VecN<AT, VEC>::zero();
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int nl = rb + RPP * i, n = col0 + nl;
      rbv[i] = (kok && nl < BN && n < g.Co) ? VecN<WT, VEC>::load(Wt + (size_t)n * p.Ktot + k0 + kq) : VecN<WT, VEC>::zero();
    }
  };
  auto store_slab = [&](int buf) {
    LT* A_ = As + buf * STAGE;
    LT* B_ = Bs + buf * STAGE;
#pragma unroll
    for (int i = 0; i < NA; ++i) store4(A_ + (rb + RPP * i) * LD + kq, ra[i]);
#pragma unroll
    for (int i = 0; i < NB; ++i)
      if (rb + RPP * i < BN) store4(B_ + (rb + RPP * i) * LD + kq, rbv[i]);
  };
  // tile of this workgroup in window `it` (windows of gridDim.x consecutive tiles, XCD-aware order inside a window)
  auto tile_of = [&](int it, int& row0, int& col0) {
    const int w0 = it * (int)gridDim.x;
    int left = ntiles - w0; if (left > (int)gridDim.x) left = (int)gridDim.x;
    if (left <= 0 || (int)blockIdx.x >= left) return false;
    const int tlin = w0 + xcd_remap(blockIdx.x, left);
    row0 = (tlin / tiles_n) * BM; col0 = (tlin % tiles_n) * BN;
    return true;
  };

  int row0, col0, it = 0;
  bool have = tile_of(0, row0, col0);
  if (have) load_slab(row0, col0, 0);
  while (have) {
    store_slab(0);
    __syncthreads();
    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      if (kt + 1 < nk) load_slab(row0, col0, (kt + 1) * BK);
      mma_slab<true, MT, NT>(As + cur * STAGE, Bs + cur * STAGE, wm * MT * 16, wn * NT * 16, lane, acc);
      if (kt + 1 < nk) store_slab(cur ^ 1);
      __syncthreads();
    }
    int row0n = 0, col0n = 0;
    const bool more = tile_of(++it, row0n, col0n);
    if (more) load_slab(row0n, col0n, 0);                // in flight during the epilogue below
#ifdef SV_IG_PROBE_NOEPI
    if (acc[0][0][0] == 12345.678f) static_cast<AT*>(p.y)[0] = (AT)acc[0][0][1];
#else
    tile_epilogue<true, false, TL, AT>(p, ci, g.Do, g.Ho, g.Wo, Cs, red, acc, row0, col0, Mrows);
    __syncthreads();                                     // the staged tile is consumed: operand slabs may land again
#endif
    have = more; row0 = row0n; col0 = col0n;
  }
}

// ------------------------------------------------------------------------------------------------
// wide dense kernel (bf16 MFMA, bf16 storage) for the deep / wide Linear and 1x1 layers (Swin stages 2-3, ResNet layer 3 1x1s).
// Measured on these shapes (scripts/bench_gemm_wide.py with the SV_GW_PROBE_* builds, scripts/probes/dma_fill_probe.hip): the MFMA + LDS
// part of a 256 x 128 tile runs at ~1.2 PFLOP/s, and what bounds the layer is the L2 -> LDS operand fill: 43-57 GB/s per CU when a wave
// instruction fetches 16 rows x 64 B, 62-84 GB/s with 8 rows x 128 B (whole cache lines) and >= 96 KB in flight per CU.  Hence:
//   * one workgroup per CU owns a 256 x 128 tile: 8 consumer waves (4 x 2, 64 x 64 each; 1.33 x fewer staged bytes per MAC than
//     128 x 128) and 4 producer waves, one per SIMD, that do nothing but issue the operand DMA - an LDS-DMA instruction blocks its wave
//     while the memory pipeline is backed up, and in the consumers' instruction stream that wait would stall the MFMAs behind it
//     (measured: fill alone 106 us, MFMA alone 110 us, both from one instruction stream 174 us on M = 25088, K = 3072, N = 768);
//   * operands go HBM/L2 -> LDS by LDS-DMA (global_load_lds_dwordx4: no staging registers, no ds_write) in 64-deep K slices - every
//     row piece is one whole 128-byte line - into a ring of three 48 KB slots; slice s + 2 is issued right after the barrier of slice
//     s, so two slices (96 KB) are in flight behind the MFMAs (counted vmcnt in the producers, raw s_barrier);
//   * the workgroup is persistent and the slice stream runs ACROSS tiles: the first two slices of the next tile are issued under the
//     last two of the current one, so the DMA queue never runs dry at a tile boundary or during an epilogue;
//   * the epilogue works on the accumulator registers (lane = one row, 4 consecutive columns per 16 x 16 block) - no LDS, no barrier;
//     one barrier per K slice is all the synchronisation there is.
// LDS image of a slice: rows of 64 bf16 (128 B = eight 16-byte slots), a DMA piece = 8 rows (lane l -> row l / 8, slot l % 8); the
// source chunk of (row r, slot s) is s ^ (r / 2 mod 8): with that XOR the four 16-lane groups of a ds_read_b128 fragment read (16
// rows, k chunk = 4 ks + lane / 16) each touch 16 different bank slots (MI355X_MICROARCH.md, LDS).
// Epilogue semantics = epilogue_rows (bias / activation(-gradient) / residual / pre-activation copy / statistics).
// Host-side conditions: K % 64 == 0, K >= 192, 8-aligned rows and columns (gemm_wide_ok).
// ------------------------------------------------------------------------------------------------
constexpr int GW_BN = 128, GW_BK = 64;
constexpr unsigned GW_NODRAW = 0xFFFFFFFFu;   // content of the tile-draw register (v167) while the atomic's return is outstanding
typedef __attribute__((address_space(1))) const void* gw_gptr_t;
typedef __attribute__((address_space(3))) void* gw_lptr_t;

// GENERAL = the epilogue reads a residual and / or an activation-gradient source; false = bias / activation / pre-activation copy / statistics
// WM = consumer wave rows (tile = 64 WM x 128), NPROD producer waves, ring of NST slices.  Built: <4, 4, 3> = 256 x 128, one workgroup per CU.
// Measured and dropped: <2, 2, 2> = 128 x 128 tiles, TWO workgroups per CU (the idea: a short-K layer's time is its output stream, which only
// overlaps with a K loop when another workgroup on the CU runs one) - 1.3-1.6 x SLOWER than <4, 4, 3> on every shape of
// scripts/bench_gemm_wide.py: one slice of lead instead of two and 1.33 x the operand fill per MAC cost more than the overlap returns.
template <bool GENERAL, int WM, int NPROD, int NST>
__global__ __launch_bounds__((2 * WM + NPROD) * 64, 3) void gemm_wide_kernel(const IGemmArgs p, int ntiles, int* __restrict__ ctr) {
  constexpr int GW_NCONS = 2 * WM, GW_BM = 64 * WM, GW_A_BYTES = GW_BM * GW_BK * 2, GW_STAGE_BYTES = (GW_BM + GW_BN) * GW_BK * 2, GW_STAGES = NST;
  constexpr int PA = GW_BM / 8 / NPROD, PB = GW_BN / 8 / NPROD, LEAD = NST - 1;      // DMA pieces per producer and slice; slices in flight
  static_assert(PA % 2 == 0 && PB % 2 == 0 && (NST == 2 || NST == 3), "piece parity / ring depth");
  // ONE object (a second one makes hipcc drain the DMA queue): the ring + the two-word mailbox of the tile scheduler + a 1 KB store patch
  // per consumer wave
  __shared__ __attribute__((aligned(1024))) char smem[GW_STAGES * GW_STAGE_BYTES + 64 + GW_NCONS * 1024];
  const __bf16* __restrict__ X = static_cast<const __bf16*>(p.x);
  const __bf16* __restrict__ Wt = static_cast<const __bf16*>(p.w);
  __bf16* __restrict__ Y = static_cast<__bf16*>(p.y);
  const Geom& g = p.g;
  const Epi& e = p.e;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Mrows = g.N * g.Do * g.Ho * g.Wo, K = g.Ci, nk = K / GW_BK;
  const int tiles_n = (g.Co + GW_BN - 1) / GW_BN;
  // ---- tile scheduler.  Tiles are handed out at run time: with a static share per workgroup a workgroup that gets its CU late (another
  // stream's kernel holds the LDS) makes the whole launch wait for its share (measured beside the ResNet branch: launches of 0.2 ms
  // stretched to 2.6 ms).  The tile space is cut into 8 contiguous chunks, one per XCD (workgroups b, b + 8, ... share an L2, and
  // consecutive tiles share an activation row panel); ctr[x] counts the tiles of chunk x handed out, ctr[8] the workgroups that are done -
  // the last one zeroes the counters for the launch that uses this slot next.  Producer 0 draws the next tile while the current one runs
  // and posts it in the mailbox (two words, by tile parity); everyone reads it behind the barrier of the second K slice.
  const int xcd = blockIdx.x & 7, cq = ntiles >> 3, cr = ntiles & 7;
  const int cbase = xcd * cq + (xcd < cr ? xcd : cr), csize = cq + (xcd < cr ? 1 : 0);
  typedef __attribute__((address_space(3))) int lds_int;   // explicit LDS pointer: a generic (flat) access would be waited for with vmcnt(0)
  lds_int* mbox = (lds_int*)(smem + GW_STAGES * GW_STAGE_BYTES);
  if (tid == 0) {
    const int v = atomicAdd(ctr + xcd, 1);
    mbox[0] = v < csize ? cbase + v : -1;
  }
  __syncthreads();
  int tcur = mbox[0], tnext = -1, it = 0;
  int row0 = (tcur / tiles_n) * GW_BM, col0 = (tcur % tiles_n) * GW_BN, row0n = 0, col0n = 0;
  auto finish = [&]() {   // one thread per workgroup, after its last draw
    if (atomicAdd(ctr + 8, 1) == (int)gridDim.x - 1) {
#pragma unroll
      for (int i = 0; i < 9; ++i) ctr[i] = 0;
    }
  };
  if (tcur < 0) { if (tid == 0) finish(); return; }

  if (wave >= GW_NCONS) {
    // ================= producer wave pw: A pieces 8 pw .. 8 pw + 7, W pieces 4 pw .. 4 pw + 3 of every slice =================
    // lane l of piece q = row 8 q + l / 8, slot l % 8 <- chunk (l % 8) ^ (row / 2 mod 8) = (l % 8) ^ (4 (q & 1) | l / 16)
    const int pw = wave - GW_NCONS;
    const int chunk0 = (lane & 7) ^ (lane >> 4);
    const __bf16* pa[PA];
    const __bf16* pb[PB];
    auto set_sources = [&](int r0, int c0) {
#pragma unroll
      for (int i = 0; i < PA; ++i) {
        int m = r0 + (pw * PA + i) * 8 + (lane >> 3);
        if (m >= Mrows) m = Mrows - 1;                     // rows past the end: any valid row, the epilogue skips them
        pa[i] = X + (size_t)m * g.ldi + (chunk0 ^ ((i & 1) << 2)) * 8;
      }
#pragma unroll
      for (int i = 0; i < PB; ++i) {
        int n = c0 + (pw * PB + i) * 8 + (lane >> 3);
        if (n >= g.Co) n = g.Co - 1;
        pb[i] = Wt + (size_t)n * p.Ktot + (chunk0 ^ ((i & 1) << 2)) * 8;
      }
    };
    auto issue = [&](int kt, int st) {
#ifdef SV_GW_PROBE_NODMA
      return;
#endif
      char* base = smem + st * GW_STAGE_BYTES;
#pragma unroll
      for (int i = 0; i < PA; ++i)
        __builtin_amdgcn_global_load_lds((gw_gptr_t)(pa[i] + kt * GW_BK), (gw_lptr_t)(base + (pw * PA + i) * 1024), 16, 0, 0);
#pragma unroll
      for (int i = 0; i < PB; ++i)
        __builtin_amdgcn_global_load_lds((gw_gptr_t)(pb[i] + kt * GW_BK), (gw_lptr_t)(base + GW_A_BYTES + (pw * PB + i) * 1024), 16, 0, 0);
    };
    static_assert(NST == 2 || PA + PB == 12, "the counted wait below is written for 12 pieces per slice");
    set_sources(row0, col0);
    issue(0, 0);
    if (LEAD == 2) issue(1, 1);                           // nk >= 3
    int st = 0;
    bool have = true;
    while (have) {
      bool more = true;                                   // known from the second slice on (nk >= 3: the last slice is a later one)
      for (int kt = 0; kt < nk; ++kt) {
        // this wave's pieces of the slice have landed (ring of 3: the 12 of the next slice may stay in flight); behind the barrier every
        // producer's have, and every consumer is done reading the previous slice, whose ring slot the next issue overwrites
        if (NST == 3 && (kt + 1 < nk || more)) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (kt == 1 && pw == 0 && lane == 0) {            // the draw of slice 0 is older than the 12 pieces waited past: normally it has returned
          // The atomic's return lands in a FIXED register, v167 (the kernel's budget at 3 waves per SIMD is 168 and the producer path needs
          // far fewer; build/igemm.s shows no other use): a C++ variable tied to the asm statements can be copied by the register
          // allocator between the issue and this read - seen in an experimental gathering variant of this kernel: a loop-carried copy
          // taken right after the issue kept the old value, the return landed in a dead register, and a tile was computed twice
          // (harmless for the output, fatal for the BatchNorm statistics).  The register holds GW_NODRAW until the return arrives - LDS-DMA
          // pieces and an atomic's return take different paths back and need not retire in issue order - in which case the queue is
          // drained once.
          unsigned dv;
          asm volatile("v_mov_b32 %0, v167" : "=v"(dv) :: "memory");
          if (dv == GW_NODRAW) asm volatile("s_waitcnt vmcnt(0)\n\tv_mov_b32 %0, v167" : "=v"(dv) :: "memory");
          const int v = (int)dv;
          mbox[(it + 1) & 1] = v < csize ? cbase + v : -1;
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (kt == 1) {
          tnext = mbox[(it + 1) & 1];
          more = tnext >= 0;
          row0n = (tnext / tiles_n) * GW_BM; col0n = (tnext % tiles_n) * GW_BN;
        }
        if (kt == 0 && pw == 0 && lane == 0)              // draw the next tile: an atomic hipcc does not count (it would drain the DMA queue for it)
          asm volatile("v_mov_b32 v167, -1\n\tglobal_atomic_add v167, %0, %1, off sc0" :: "v"(ctr + xcd), "v"(1u) : "memory", "v167");
        const int st2 = st == 0 ? NST - 1 : st - 1;       // = (st + LEAD) mod NST: the slot consumed a slice ago
        if (kt + LEAD < nk) issue(kt + LEAD, st2);
        else if (more) {
          if (kt + LEAD == nk) set_sources(row0n, col0n); // the current tile's last slice was issued an iteration ago
          issue(kt + LEAD - nk, st2);
        }
        st = st == NST - 1 ? 0 : st + 1;
      }
      have = more; ++it;
    }
    return;
  }

  // ================= consumer waves: WM x 2 grid of 64 x 64 wave tiles =================
  const int wm = wave >> 1, wn = wave & 1, lr = lane & 15, lg = lane >> 4;
  // fragment addresses: row lr of a 16-row block, k chunk 4 ks + lg -> slot (4 ks + lg) ^ (lr / 2)
  int aoff[2], boff[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int slot = (ks * 4 + lg) ^ (lr >> 1);
    aoff[ks] = (wm * 64 + lr) * 128 + slot * 16;
    boff[ks] = GW_A_BYTES + (wn * 64 + lr) * 128 + slot * 16;
  }
  int st = 0;                                             // ring slot of the slice computed next
  bool have = true;
  while (have) {
    f32x4 acc[4][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < nk; ++kt) {
      asm volatile("s_barrier" ::: "memory");             // the slice has landed (the producers waited for it before this barrier)
      if (kt == 1) tnext = mbox[(it + 1) & 1];            // posted by producer 0 in front of this barrier
#ifndef SV_GW_PROBE_NOMMA
      const char* sb = smem + st * GW_STAGE_BYTES;
      bf16x8 a[2][4], b[2][4];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) b[ks][nt] = *reinterpret_cast<const bf16x8*>(sb + boff[ks] + nt * 2048);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) a[ks][mt] = *reinterpret_cast<const bf16x8*>(sb + aoff[ks] + mt * 2048);
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[ks][nt], a[ks][mt], acc[mt][nt], 0, 0, 0);
#endif
      st = st == NST - 1 ? 0 : st + 1;
    }

    // ---- epilogue on the registers: lane (lr, lg) of block (mt, nt) = row mt * 16 + lr, columns nt * 16 + lg * 4 .. + 3.
    // Every global LOAD of the tile (row scales, residual, activation-gradient source) is issued before the first STORE: vmcnt retires
    // in issue order, so a load behind stores could only be waited for by draining the stores (measured: ~2 us per 16-row block).
    {
      const int mbase = row0 + wm * 64 + lr, nbase = col0 + wn * 64 + lg * 4;
      bool colok[4];
      float bias[4][4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        colok[nt] = nbase + nt * 16 < g.Co;                // Co % 8 == 0: a 4-vector is whole or absent
#pragma unroll
        for (int j = 0; j < 4; ++j) bias[nt][j] = (e.bias && colok[nt]) ? e.bias[nbase + nt * 16 + j] : 0.f;
      }
      // the wave-private 8-row x 128-byte LDS patch that turns the accumulator layout (lane = a row, 8 bytes) into whole 128-byte rows
      // (16 bytes per lane) and back: 16-byte pairs XOR-swizzled by the row, conflict-free both ways, no barrier (a wave's LDS operations
      // execute in order)
      typedef __attribute__((address_space(3))) char lds_char;
      lds_char* stg = (lds_char*)(smem + GW_STAGES * GW_STAGE_BYTES + 64) + wave * 1024;
      const int wrow = lr & 7, half_of_lane = lr >> 3, rrow = lane >> 3;
      const int roff = rrow * 128 + (((lane & 7) ^ rrow) << 4);
      const int ncol_s = col0 + wn * 64 + (lane & 7) * 8;
      float rsc[4];
      bf16x8 raw[4][2];                                    // residual OR activation-gradient source rows (gemm_wide_ok: never both), whole lines
      if constexpr (GENERAL) {
        const __bf16* src = e.residual ? static_cast<const __bf16*>(e.residual) + ncol_s : static_cast<const __bf16*>(e.act_grad_src) + e.col_off + ncol_s;
        const int lds_ = e.residual ? e.ldr : e.ldc;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
          const int m = mbase + mt * 16;
          rsc[mt] = (m < Mrows && e.residual && e.row_scale) ? e.row_scale[m / e.rows_per_scale] : 1.f;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int ms = row0 + wm * 64 + mt * 16 + h * 8 + rrow;
            raw[mt][h] = VecN<__bf16, 8>::zero();
            if (ms < Mrows && ncol_s < g.Co) raw[mt][h] = *reinterpret_cast<const bf16x8*>(src + (size_t)ms * lds_);
          }
        }
      }
      float s1[4][4], s2[4][4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int j = 0; j < 4; ++j) { s1[nt][j] = 0.f; s2[nt][j] = 0.f; }
      // stores: through the patch a lane's 8 bytes of a row become 16 bytes per lane, 8 whole 128-byte rows per instruction - a quarter of the
      // cache lines touched per byte of the 8-byte form (measured: the partial-line stores cost as much as the K loop at K = 384); the
      // residual / activation-gradient rows come in the same way (above)
      auto rows_out = [&](__bf16* dst, const bf16x4 (&ob)[4], int mt) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if (half_of_lane == h) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
              *reinterpret_cast<__attribute__((address_space(3))) bf16x4*>(stg + wrow * 128 + (((nt * 4 + lg) ^ (2 * wrow)) << 3)) = ob[nt];
          }
          __builtin_amdgcn_wave_barrier();
          const bf16x8 o16 = *reinterpret_cast<__attribute__((address_space(3))) bf16x8*>(stg + roff);
          __builtin_amdgcn_wave_barrier();
          const int ms = row0 + wm * 64 + mt * 16 + h * 8 + rrow;
#ifdef SV_GW_PROBE_NOSTORE
          if (o16[0] == (__bf16)1234.5f)
#endif
          if (ms < Mrows && ncol_s < g.Co) *reinterpret_cast<bf16x8*>(dst + (size_t)ms * e.ldc + e.col_off + ncol_s) = o16;
        }
      };
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const bool rowok = mbase + mt * 16 < Mrows;
        bf16x4 ob[4], pb[4], aux[4];
        if constexpr (GENERAL) {   // whole rows -> patch -> this lane's four 8-byte pieces
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<__attribute__((address_space(3))) bf16x8*>(stg + roff) = raw[mt][h];
            __builtin_amdgcn_wave_barrier();
            if (half_of_lane == h) {
#pragma unroll
              for (int nt = 0; nt < 4; ++nt)
                aux[nt] = *reinterpret_cast<__attribute__((address_space(3))) bf16x4*>(stg + wrow * 128 + (((nt * 4 + lg) ^ (2 * wrow)) << 3));
            }
            __builtin_amdgcn_wave_barrier();
          }
        }
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          float v[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = acc[mt][nt][j] + bias[nt][j];
          if constexpr (GENERAL) {
            if (e.act_grad_src) {
              if (e.act_grad_kind == SV_ACT_GELU) {        // pairs: packed fp32 math (common.h)
#pragma unroll
                for (int j = 0; j < 4; j += 2) {
                  const f32x2 dg = gelu_grad_fast2((f32x2){(float)aux[nt][j], (float)aux[nt][j + 1]});
                  v[j] *= dg[0]; v[j + 1] *= dg[1];
                }
              } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] *= act_grad_t<true>((float)aux[nt][j], e.act_grad_kind, e.slope);
              }
            }
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) pb[nt][j] = (__bf16)v[j];
          if (e.act == SV_ACT_GELU) {
#pragma unroll
            for (int j = 0; j < 4; j += 2) {
              const f32x2 gl = gelu_fast2((f32x2){v[j], v[j + 1]});
              v[j] = gl[0]; v[j + 1] = gl[1];
            }
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = apply_act_t<true>(v[j], e.act, e.slope);
          }
          if constexpr (GENERAL) {
            if (e.residual) {
#pragma unroll
              for (int j = 0; j < 4; ++j) v[j] = (float)aux[nt][j] + rsc[mt] * v[j];
            }
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) ob[nt][j] = (__bf16)v[j];
          if constexpr (!GENERAL) {
            if (rowok && colok[nt]) {
#pragma unroll
              for (int j = 0; j < 4; ++j) { const float f = (float)ob[nt][j]; s1[nt][j] += f; s2[nt][j] += f * f; }
            }
          }
        }
        if (e.pre_act) rows_out(static_cast<__bf16*>(e.pre_act), pb, mt);
        rows_out(Y, ob, mt);
      }
      if (!GENERAL && e.stats) {   // (gemm_wide_ok: statistics never come with a residual / activation-gradient source) the 16 rows of a lane group, then one double atomic per column and wave (64 rows) into a slot image
        double* stp = e.stats + (size_t)((row0 / 64 + wm) % SV_BN_SLOTS) * 2 * g.Co;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            // the 16 lanes of a row: four DPP row shifts leave the total in lane 15 (a __shfl_xor goes through the LDS crossbar)
            const float a1 = row16_total(s1[nt][j]), a2 = row16_total(s2[nt][j]);
            const int n = nbase + nt * 16 + j;
            if (lr == 15 && n < g.Co) { atomicAdd(stp + n, (double)a1); atomicAdd(stp + g.Co + n, (double)a2); }
          }
      }
    }
    have = tnext >= 0; row0 = (tnext / tiles_n) * GW_BM; col0 = (tnext % tiles_n) * GW_BN; ++it;
  }
  if (tid == 0) finish();
}

// ------------------------------------------------------------------------------------------------
// weight-gradient kernel
// ------------------------------------------------------------------------------------------------
struct WGradArgs {
  const void* anchor; int lda; const void* gathered; float* out;   // anchor/gathered: activations (AT); out = dw (taps == 1) or the packed workspace
  Geom g; int cg_valid; int rows_per_split; int Mrows; int direct;
  float* dbias;     // optional: dbias[ca] += sum_r anchor[r, ca] (bias gradient), folded into the k_out-tile-0 workgroups
};

template <bool BF16, typename TL, typename AT, int VEC>
__global__ __launch_bounds__(TL::NTHR, TL::NTHR == 512 ? 4 : 2) void wgrad_kernel(const WGradArgs p) {
  typedef typename Cfg<BF16>::T LT;
  typedef typename VecN<AT, VEC>::type AV;
  const AT* __restrict__ ANC = static_cast<const AT*>(p.anchor);
  const AT* __restrict__ GAT = static_cast<const AT*>(p.gathered);
  // row stride = 8 banks mod 64 (bf16: +16 elements): the 4 rows a 16-lane group touches in one ds_read_b64_tr_b16 fall
  // into disjoint 8-bank windows (with +8 elements rows q and q+1 overlap by 4 banks -> 2-way conflicts)
  constexpr int BK = Cfg<BF16>::BK, PAD = BF16 ? 16 : Cfg<BF16>::PAD;
  constexpr int BM = TL::BM, BN = TL::BN, MT = TL::MT, NT = TL::NT;
  constexpr int LDA = BM + PAD, LDB = BN + PAD;
  constexpr int NTHR = TL::NTHR;
  constexpr int A4 = BM / VEC, A_RPP = NTHR / A4, A_PASS = (BK + A_RPP - 1) / A_RPP;   // VEC-element columns / rows per pass / passes
  constexpr int B4 = BN / VEC, B_RPP = NTHR / B4, B_PASS = (BK + B_RPP - 1) / B_RPP;
  __shared__ __attribute__((aligned(16))) LT As[2 * BK * LDA];  // [stage][r][ca]     (double-buffered: one barrier / K step)
  __shared__ __attribute__((aligned(16))) LT Bs[2 * BK * LDB];  // [stage][r][k_out]

  const Geom& g = p.g;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / TL::WN, wn = wave % TL::WN;
  const int taps = g.kd * g.kh * g.kw;
  const int Kout = taps * g.Ci;
  const int gx = (g.Co + BM - 1) / BM, gy = (Kout + BN - 1) / BN;
  const int tlin = xcd_remap(blockIdx.x, gridDim.x);          // (ca tile fastest, then k_out tile, then position split)
  const int ca0 = (tlin % gx) * BM, ko0 = ((tlin / gx) % gy) * BN;
  const int r_begin = (tlin / (gx * gy)) * p.rows_per_split;
  int r_end = r_begin + p.rows_per_split;
  if (r_end > p.Mrows) r_end = p.Mrows;
  if (r_begin >= r_end) return;

  const int a_c = (tid % A4) * VEC, a_r = tid / A4;
  const int b_kl = (tid % B4) * VEC, b_k = ko0 + b_kl, b_r = tid / B4;
  const bool avec = (p.lda % VEC) == 0, bvec = (g.Ci % VEC) == 0 && (g.ldi % VEC) == 0;
  const bool dense = (g.Do * g.Ho * g.Wo == 1) && taps == 1;   // Linear: gathered row == anchor row
  int b_c = 0, b_td = 0, b_th = 0, b_tw = 0;
  if (bvec) {
    const int b_tap = b_k / g.Ci; b_c = b_k - b_tap * g.Ci;
    b_tw = b_tap % g.kw; const int t2 = b_tap / g.kw; b_th = t2 % g.kh; b_td = t2 / g.kh;
  }
  // running (n,d,h,w) of the rows this thread gathers for B; advanced by BK per step without division
  int bn_[B_PASS], bd_[B_PASS], bh_[B_PASS], bw_[B_PASS];
#pragma unroll
  for (int i = 0; i < B_PASS; ++i) decode_row(r_begin + b_r + B_RPP * i, g.Do, g.Ho, g.Wo, bn_[i], bd_[i], bh_[i], bw_[i]);

  AV ra[A_PASS], rbv[B_PASS];
  int r0 = r_begin;
  auto load_tile = [&]() {
#pragma unroll
    for (int i = 0; i < A_PASS; ++i) {
      const int rl = a_r + A_RPP * i, r = r0 + rl;
      AV q = VecN<AT, VEC>::zero();
      if (rl < BK && r < r_end) {
        const AT* src = ANC + (size_t)r * p.lda + ca0 + a_c;
        if (avec && ca0 + a_c + VEC - 1 < g.Co) {
          q = VecN<AT, VEC>::load(src);
        } else if constexpr (VEC == 4) {
          float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int j = 0; j < 4; ++j) if (ca0 + a_c + j < g.Co) v[j] = ldf(src + j);
          q = VecN<AT, 4>::make(v[0], v[1], v[2], v[3]);
        }
      }
      ra[i] = q;
    }
#pragma unroll
    for (int i = 0; i < B_PASS; ++i) {
      const int rl = b_r + B_RPP * i, r = r0 + rl;
      AV q = VecN<AT, VEC>::zero();
      if (rl < BK && r < r_end) {
        if (dense) {
          if (bvec) {
            if (b_k < Kout) q = VecN<AT, VEC>::load(GAT + (size_t)r * g.ldi + b_k);
          } else if constexpr (VEC == 4) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) if (b_k + j < Kout) v[j] = ldf(GAT + (size_t)r * g.ldi + b_k + j);
            q = VecN<AT, 4>::make(v[0], v[1], v[2], v[3]);
          }
        } else {
          const int bd = bd_[i] * g.sd - g.pd, bh = bh_[i] * g.sh - g.ph, bw = bw_[i] * g.sw - g.pw;
          if (bvec) {
            const int id = bd + b_td, ih = bh + b_th, iw = bw + b_tw;
            if (b_k < Kout && (unsigned)id < (unsigned)g.Di && (unsigned)ih < (unsigned)g.Hi && (unsigned)iw < (unsigned)g.Wi)
              q = VecN<AT, VEC>::load(GAT + ((((size_t)bn_[i] * g.Di + id) * g.Hi + ih) * g.Wi + iw) * (size_t)g.ldi + b_c);
          } else if constexpr (VEC == 4) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int kk = b_k + j;
              if (kk < Kout) {
                const int tap = kk / g.Ci, c = kk - tap * g.Ci;
                const int tw = tap % g.kw; const int t2 = tap / g.kw; const int th = t2 % g.kh; const int td = t2 / g.kh;
                const int id = bd + td, ih = bh + th, iw = bw + tw;
                if ((unsigned)id < (unsigned)g.Di && (unsigned)ih < (unsigned)g.Hi && (unsigned)iw < (unsigned)g.Wi)
                  v[j] = ldf(GAT + ((((size_t)bn_[i] * g.Di + id) * g.Hi + ih) * g.Wi + iw) * (size_t)g.ldi + c);
              }
            }
            q = VecN<AT, 4>::make(v[0], v[1], v[2], v[3]);
          }
        }
      }
      rbv[i] = q;
    }
    // advance the running row coordinates by BK
    r0 += BK;
    if (!dense) {
#pragma unroll
      for (int i = 0; i < B_PASS; ++i) {
        bw_[i] += BK;
        while (bw_[i] >= g.Wo) {
          bw_[i] -= g.Wo;
          if (++bh_[i] == g.Ho) { bh_[i] = 0; if (++bd_[i] == g.Do) { bd_[i] = 0; ++bn_[i]; } }
        }
      }
    }
  };
  auto store_tile = [&](int buf) {  // natural layout: [position][channel], vector stores
    LT* A_ = As + buf * BK * LDA;
    LT* B_ = Bs + buf * BK * LDB;
#pragma unroll
    for (int i = 0; i < A_PASS; ++i) {
      const int rl = a_r + A_RPP * i;
      if (rl < BK) store4(A_ + rl * LDA + a_c, ra[i]);
    }
#pragma unroll
    for (int i = 0; i < B_PASS; ++i) {
      const int rl = b_r + B_RPP * i;
      if (rl < BK) store4(B_ + rl * LDB + b_kl, rbv[i]);
    }
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const bool do_bias = p.dbias != nullptr && ko0 == 0;
  float bsum = 0.f;
  load_tile();
  store_tile(0);
  __syncthreads();
  int cur = 0;
  for (int rr = r_begin; rr < r_end; rr += BK, cur ^= 1) {
    const bool more = rr + BK < r_end;
    const LT* Ac = As + cur * BK * LDA;
    if (more) load_tile();
    mma_slab_km<BF16, MT, NT, LDA, LDB>(Ac, Bs + cur * BK * LDB, wm * MT * 16, wn * NT * 16, lane, acc);
    if (do_bias && tid < BM) {
      float sb = 0.f;
#pragma unroll 8
      for (int r = 0; r < BK; ++r) sb += (float)Ac[r * LDA + tid];
      bsum += sb;
    }
    if (more) store_tile(cur ^ 1);
    __syncthreads();
  }

  if (do_bias && tid < BM && ca0 + tid < g.Co) atomicAdd(p.dbias + ca0 + tid, bsum);
  const int lr = lane & 15, lg = lane >> 4;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int ko = ko0 + (wn * NT + nt) * 16 + lr;
    if (ko >= Kout) continue;
    const int tap = ko / g.Ci, cg = ko - tap * g.Ci;
    if (cg >= p.cg_valid) continue;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ca = ca0 + (wm * MT + mt) * 16 + lg * 4 + j;
        if (ca < g.Co) {
          // direct: native layout (taps == 1 -> contiguous along cg); else packed workspace [ca][tap][cg] (contiguous along ko)
          const size_t o = p.direct ? ((size_t)ca * p.cg_valid + cg) * taps + tap : (size_t)ca * Kout + ko;
          atomicAdd(p.out + o, acc[mt][nt][j]);
        }
      }
  }
}

// dw[(ca*cgv + cg)*taps + tap] += ws[ca*Kout + tap*Ci + cg]
__global__ void wgrad_unpack_kernel(const float* __restrict__ ws, float* __restrict__ dw, int Co, int Ci, int cgv, int taps) {
  const long long total = (long long)Co * cgv * taps;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int tap = (int)(i % taps); long long t = i / taps;
    const int cg = (int)(t % cgv); const int ca = (int)(t / cgv);
    dw[i] += ws[((size_t)ca * taps + tap) * Ci + cg];
  }
}

// ------------------------------------------------------------------------------------------------
// small helpers: weight repack, column sums
// ------------------------------------------------------------------------------------------------
template <typename WT>
__global__ void pack_weight_kernel(const float* __restrict__ src, WT* __restrict__ dst, int A, int B, int T, int swap,
                                   int rows_out, int inner_out) {
  // dst[rows_out][T][inner_out]; swap=0: rows=A inner=B ; swap=1: rows=B inner=A ; zero beyond the valid range
  const long long total = (long long)rows_out * T * inner_out;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int in_ = (int)(i % inner_out); long long t2 = i / inner_out;
    const int t = (int)(t2 % T); const int ro = (int)(t2 / T);
    const int a = swap ? in_ : ro, b = swap ? ro : in_;
    dst[i] = (WT)((a < A && b < B) ? src[((size_t)a * B + b) * T + t] : 0.f);
  }
}

// every weight pack of a module in ONE launch: workgroup -> descriptor by binary search over the block prefix; a
// workgroup produces PACK_PER_BLOCK consecutive output elements of its descriptor
constexpr int PACK_PER_BLOCK = 2048;
template <typename WT>
__global__ __launch_bounds__(256) void pack_weights_batched_kernel(const sv_pack_desc* __restrict__ descs, int n) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {   // last descriptor with block0 <= blockIdx.x
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const sv_pack_desc d = descs[lo];
  const float* __restrict__ src = d.src;
  WT* __restrict__ dst = static_cast<WT*>(d.dst);
  const long long total = (long long)d.rows_out * d.T * d.inner_out;
  if (d.T == 1 && d.swap && (d.rows_out & 31) == 0 && (d.inner_out & 63) == 0) {
    // data-gradient pack of a Linear / 1x1 layer = a plain matrix transpose dst[b][a] = src[a][b] (most of the 84 M parameters: refiner FC, Swin
    // linears, ResNet 1x1): 32 x 64 tiles through LDS, 128-byte runs on both sides - the element-wise form reads one float per 64-byte line
    // (measured 2.4 GB of traffic per step for 0.7 GB of packs).  Same block count as the element-wise form: 2048 outputs per workgroup.
    __shared__ float tile[32][65];
    const int bl = (int)blockIdx.x - d.block0, tiles_in = d.inner_out >> 6;
    const int b0 = (bl / tiles_in) * 32, a0 = (bl % tiles_in) * 64;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int idx = threadIdx.x + 256 * k, al = idx >> 3, q = idx & 7;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (a0 + al < d.A) v = *reinterpret_cast<const float4*>(src + (size_t)(a0 + al) * d.B + b0 + 4 * q);   // B = rows_out: a multiple of 32
      tile[4 * q][al] = v.x; tile[4 * q + 1][al] = v.y; tile[4 * q + 2][al] = v.z; tile[4 * q + 3][al] = v.w;
    }
    __syncthreads();
    const int brow = threadIdx.x >> 3, ch = (threadIdx.x & 7) * 8;
    WT* o = dst + (size_t)(b0 + brow) * d.inner_out + a0 + ch;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (WT)tile[brow][ch + j];
    return;
  }
  const long long i0 = (long long)(blockIdx.x - d.block0) * PACK_PER_BLOCK;
  for (int k = threadIdx.x; k < PACK_PER_BLOCK; k += 256) {
    const long long i = i0 + k;
    if (i >= total) break;
    const int in_ = (int)(i % d.inner_out); long long t2 = i / d.inner_out;
    const int t = (int)(t2 % d.T); const int ro = (int)(t2 / d.T);
    const int a = d.swap ? in_ : ro, b = d.swap ? ro : in_;
    dst[i] = (WT)((a < d.A && b < d.B) ? src[((size_t)a * d.B + b) * d.T + t] : 0.f);
  }
}

template <typename AT>
__global__ __launch_bounds__(256) void colsum_kernel(const AT* __restrict__ x, long long rows, int cols, int ld,
                                                     float* __restrict__ out, long long rows_per_block) {
  // block = 64 columns x 4 row-lanes; grid.x = column groups, grid.y = row splits
  __shared__ float red[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int rl = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.y * rows_per_block;
  long long r1 = r0 + rows_per_block; if (r1 > rows) r1 = rows;
  float s = 0.f;
  if (c < cols) for (long long r = r0 + rl; r < r1; r += 4) s += ldf(x + (size_t)r * ld + c);
  red[rl][threadIdx.x & 63] = s;
  __syncthreads();
  if (rl == 0 && c < cols) atomicAdd(out + c, red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static Geom to_geom(const sv_geom* g) {
  Geom q{g->N, g->Di, g->Hi, g->Wi, g->Do, g->Ho, g->Wo, g->Ci, g->Co, g->kd, g->kh, g->kw,
         g->sd, g->sh, g->sw, g->pd, g->ph, g->pw, g->ldi};
  return q;
}
static Epi to_epi(const sv_epilogue* e) {
  Epi q{e->bias, e->residual, e->ldr, e->row_scale, e->rows_per_scale > 0 ? e->rows_per_scale : 1, e->pre_act, e->stats,
        e->act, e->slope, e->act_grad_src, e->act_grad_kind, e->ldc, e->col_off};
  return q;
}
static int check_common(const sv_geom* g, const sv_epilogue* e, const void* in, const void* w, const void* out, int act_dtype) {
  SV_REQUIRE(g && e && in && w && out, "igemm: null argument");
  SV_REQUIRE(g->N > 0 && g->Ci > 0 && g->Co > 0, "igemm: N/Ci/Co must be positive (N=%d Ci=%d Co=%d)", g->N, g->Ci, g->Co);
  SV_REQUIRE(g->Di > 0 && g->Hi > 0 && g->Wi > 0 && g->Do > 0 && g->Ho > 0 && g->Wo > 0, "igemm: empty grid");
  SV_REQUIRE(g->kd > 0 && g->kh > 0 && g->kw > 0 && g->sd > 0 && g->sh > 0 && g->sw > 0, "igemm: kernel/stride must be positive");
  SV_REQUIRE(g->ldi >= g->Ci, "igemm: ldi (%d) < Ci (%d)", g->ldi, g->Ci);
  SV_REQUIRE(e->ldc >= e->col_off + g->Co, "igemm: ldc (%d) < col_off+Co (%d)", e->ldc, e->col_off + g->Co);
  SV_REQUIRE(!e->residual || e->ldr >= g->Co, "igemm: ldr (%d) < Co (%d)", e->ldr, g->Co);
  SV_REQUIRE(((uintptr_t)in & (act_dtype == SV_BF16 ? 7 : 15)) == 0 && ((uintptr_t)w & 15) == 0, "igemm: in must be aligned to 4 elements, w to 16 bytes");
  SV_REQUIRE((long long)g->N * g->Do * g->Ho * g->Wo < (1ll << 31) && (long long)g->N * g->Di * g->Hi * g->Wi < (1ll << 31),
             "igemm: more than 2^31 positions");
  return SV_OK;
}

// scheduler counters of the wide kernel: 16 ints per launch slot, zero on entry, zeroed again by the launch's last workgroup.  A slot is
// reused after GW_SLOTS launches of this process - far more than a device queue holds in flight.
constexpr int GW_SLOTS = 4096;
// One buffer PER DEVICE (ops._CallContext allows one thread per device in a process): a launch on device 1 must not hand the scheduler a
// pointer into device 0's memory.  The table is filled lazily under a mutex; the slot cursor is per device too.
struct GwCounters { int* buf = nullptr; bool tried = false; std::atomic<unsigned> next{0}; };
static GwCounters* gemm_wide_counter_table() {
  static GwCounters tab[16];
  static std::mutex mu;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  GwCounters& c = tab[dev];
  if (!c.tried) {
    std::lock_guard<std::mutex> lk(mu);
    if (!c.tried) {
      int* b = nullptr;
      if (hipMalloc(&b, sizeof(int) * 16 * GW_SLOTS) == hipSuccess && hipMemset(b, 0, sizeof(int) * 16 * GW_SLOTS) == hipSuccess) {
        hipDeviceSynchronize();
        c.buf = b;
      }
      c.tried = true;
    }
  }
  return c.buf ? &c : nullptr;
}
static int* gemm_wide_counters() {     // next launch slot of the current device
  GwCounters* c = gemm_wide_counter_table();
  return c ? c->buf + 16 * (c->next.fetch_add(1) % GW_SLOTS) : nullptr;
}

int* tile_draw_counters() { return gemm_wide_counters(); }

// ------------------------------------------------------------------------------------------------
// Launch plans of sv_conv_gather / sv_tconv_gather.  Which kernel, tile, operand variant and grid a call gets is decided HERE, by pure host
// functions (no HIP call); the entry points launch what plan_gather returns and sv_conv_gather_plan reports the same struct.
// ------------------------------------------------------------------------------------------------
enum { TILE_NARROW, TILE_DEFAULT, TILE_96, TILE_BIG };
struct GatherPlan {
  sv_launch_plan q;     // path, tile, operand variant, grid, block: what the query reports
  int tile;             // TILE_* of the dense and the gathering kernels
  int ntiles;           // dense and wide kernels: the tiles their persistent workgroups walk
  bool counters;        // the launch needs a slot of the scheduler counters
  HaloPlan halo;        // halo paths: tile counts of conv_halo.hip
};
template <typename F> static void with_tile(int tile, F&& f) {
  switch (tile) {
    case TILE_NARROW: f(TileNarrow{}); break;
    case TILE_96: f(Tile96{}); break;
    case TILE_BIG: f(TileBig{}); break;
    default: f(TileDefault{}); break;
  }
}

// Halo-tile kernels (conv_halo.hip) take the shapes they are built for - 3 x 3 / stride 1 / 64 k -> 64 k channels (forward and data gradient)
// and the 4 x 4 stem on the space-to-depth image (forward, and its 64 -> 16 data gradient) - when the call is a plain store (+ BatchNorm
// statistics in the forward); kind -1 = not taken
static HaloPlan plan_halo(const IGemmArgs& a, int math, int act, bool dgrad) {
  const Geom& g = a.g;
  const Epi& e = a.e;
  if (math != SV_MATH_BF16 || act != SV_BF16 || !conv_halo_enabled()) return HaloPlan{};
  if (((uintptr_t)a.x | (uintptr_t)a.w | (uintptr_t)a.y) & 15) return HaloPlan{};
  if (g.kd != 1 || g.Di != 1 || g.Do != 1 || g.sd != 1 || g.sh != 1 || g.sw != 1 || g.pd != 0) return HaloPlan{};
  if (g.Hi != g.Ho || g.Wi != g.Wo || g.ldi != g.Ci) return HaloPlan{};
  if (e.bias || e.residual || e.row_scale || e.pre_act || e.act != SV_ACT_NONE || e.act_grad_src || e.ldc != g.Co || e.col_off != 0) return HaloPlan{};
  if (dgrad && e.stats) return HaloPlan{};
  const bool k3 = g.kh == 3 && g.kw == 3 && g.ph == 1 && g.pw == 1, k4 = g.kh == 4 && g.kw == 4 && g.ph == 2 && g.pw == 2;
  // the stem's data gradient (kind 1 backwards: 64 -> 16 channels) on the tile that reads each dy patch once
  if (dgrad && k4 && g.Ci == 64 && g.Co == 16) return conv_halo_plan(2, g.N, g.Hi, g.Wi);
  if (g.Co & 63) return HaloPlan{};
  if (k3) return g.Ci == 64 && g.Co == 64 ? conv_halo_plan(0, g.N, g.Hi, g.Wi) : conv_halo_blocked_plan(g.N, g.Hi, g.Wi, g.Ci, g.Co);   // more channels: blocks of 64 x 64
  if (!dgrad && k4 && g.Ci == 16 && g.Co == 64) return conv_halo_plan(1, g.N, g.Hi, g.Wi);
  return HaloPlan{};
}

// the wide kernel takes the dense layers whose K loop is worth a DMA ring and whose tile count fills the chip;
// SV_GEMM_WIDE=0 in the environment keeps every layer on the 128-wide kernels (A/B measurements)
static bool gemm_wide_ok(const IGemmArgs& a, long long M) {
  static const int enabled = [] { const char* v = getenv("SV_GEMM_WIDE"); return v ? atoi(v) : 1; }();
  const Epi& e = a.e;
  const int K = a.g.Ci, Co = a.g.Co;
  if (!enabled || K % GW_BK || K < 3 * GW_BK || Co < 128 || a.Ktot % 8) return false;
  // where it wins (scripts/bench_gemm_wide.py, M = 25k .. 400k): everything from K = 192 on, except the BatchNorm producers (two double
  // atomics per column and 64 rows), which need a K loop long enough to carry them
  if (enabled == 1 && e.stats && K < 1024) return false;
  if (enabled == 1 && e.act_grad_src && K < 384) return false;   // 192 -> 768 with GELU': 573 us against 522 on the 128-wide kernel
  if (!rows_16_byte_aligned(a) || ((uintptr_t)a.w & 15)) return false;
  // the general epilogue variant keeps no statistics registers and one set of prefetched rows (residual OR activation-gradient source)
  if ((e.stats && (e.residual || e.act_grad_src)) || (e.residual && e.act_grad_src)) return false;
  return (long long)cdiv(M, 256) * cdiv(Co, GW_BN) >= 256;
}

// M = rows of the call (transposed: of its largest parity class), ncls = parity classes (1 unless transposed), counters = a slot of the
// scheduler counters can be had.  Order: halo tiles, wide kernel, dense kernel, gathering kernel.
static GatherPlan plan_gather(const IGemmArgs& a, long long M, int ncls, int math, int act, bool tconv, bool counters) {
  const Geom& g = a.g;
  const int Co = g.Co;
  GatherPlan p{};
  // bf16 storage: weights are bf16 too; 16-byte operand chunks when the gathered rows allow it
  const bool v8 = act == SV_BF16 && (g.Ci % 8) == 0 && (g.ldi % 8) == 0 && ((uintptr_t)a.x & 15) == 0;
  p.q.operands = math != SV_MATH_BF16 ? SV_OPERANDS_F32 : act != SV_BF16 ? SV_OPERANDS_BF16_F32 : SV_OPERANDS_BF16;
  p.q.vec = v8 ? 8 : 4;
  p.q.grid_y = 1;
  if (counters && (p.halo = plan_halo(a, math, act, tconv)).kind >= 0) {
    p.q.path = p.halo.kind < 3 ? SV_PATH_HALO0 + p.halo.kind : p.halo.th == 16 ? SV_PATH_HALO_BLOCKED_16X16 : SV_PATH_HALO_BLOCKED_8X32;
    p.q.tile_rows = p.halo.th; p.q.tile_cols = p.halo.tw; p.q.grid_x = p.halo.grid; p.q.block = 256;
    p.counters = true;
    return p;
  }
  // Linear / 1x1 stride-1 layers with bf16 storage: the wide kernel, or the persistent dense kernel (2 workgroups per CU walk the tiles)
  const bool dense = !tconv && v8 && g.kd * g.kh * g.kw == 1 && g.sd == 1 && g.sh == 1 && g.sw == 1 &&
                     g.pd == 0 && g.ph == 0 && g.pw == 0 && g.Di == g.Do && g.Hi == g.Ho && g.Wi == g.Wo;
  if (dense && counters && gemm_wide_ok(a, M)) {
    p.q.path = a.e.residual || a.e.act_grad_src ? SV_PATH_WIDE_GENERAL : SV_PATH_WIDE;
    p.q.tile_rows = 256; p.q.tile_cols = GW_BN; p.q.grid_x = 256; p.q.block = 768;
    p.ntiles = cdiv(M, 256) * cdiv(Co, GW_BN);
    p.counters = true;
    return p;
  }
  // 96-wide tile for Co = 96 k when it wins the estimate  ceil(tiles / 256 CUs) x tile area x (1 + 2 % per extra pass over A)
  // (the per-channel statistics epilogue needs a power-of-two column-group count, so BatchNorm producers never take it)
  bool use96 = false;
  if (Co % 96 == 0 && !a.e.stats) {
    auto est = [&](int bm, int bn) {
      const long long tn = cdiv(Co, bn), tiles = (long long)cdiv(M, bm) * tn * ncls;
      return (double)((tiles + 255) / 256) * bm * bn * (1.0 + 0.02 * (tn - 1));
    };
    const double e96 = est(128, 96), e64 = est(128, 64), e128 = Co > 64 ? est(128, 128) : 1e300;
    use96 = e96 <= e64 && e96 <= e128;
  }
  // one tile ladder for both kernels (a dense call has one class); 8-wave 128 x 128: one pass over A per 128 output columns
  p.tile = Co <= 16 ? TILE_NARROW : use96 ? TILE_96 : Co > 64 && (long long)cdiv(M, 128) * cdiv(Co, 128) * ncls >= 384 ? TILE_BIG : TILE_DEFAULT;
  with_tile(p.tile, [&](auto tl) {
    typedef decltype(tl) TL;
    const int ntiles = cdiv(M, TL::BM) * cdiv(Co, TL::BN), resident = 256 * (TL::NTHR >= 512 ? 2 : 4);
    p.q.tile_rows = TL::BM; p.q.tile_cols = TL::BN; p.q.block = TL::NTHR;
    if (dense && Co > 16) { p.q.path = SV_PATH_DENSE; p.ntiles = ntiles; p.q.grid_x = resident < ntiles ? resident : ntiles; }
    else { p.q.path = SV_PATH_GATHER; p.q.grid_x = ntiles; p.q.grid_y = ncls; }
  });
  return p;
}

// the one place the gather family is launched: a switch over the plan, no shape condition.  TCONV = transposed gather (the halo kernels then run
// the data gradient: mirrored taps)
template <bool TCONV>
static void launch_gather(const GatherPlan& p, const IGemmArgs& a, int* ctr, hipStream_t s) {
  const dim3 grid(p.q.grid_x, p.q.grid_y), block(p.q.block);
  switch (p.q.path) {
    case SV_PATH_HALO0: case SV_PATH_HALO1: case SV_PATH_HALO2:
      conv_halo_launch(HaloConvArgs{a.x, a.w, a.y, a.e.stats, a.g.N, a.g.Hi, a.g.Wi, TCONV ? 1 : 0}, p.halo, ctr, s);
      return;
    case SV_PATH_HALO_BLOCKED_8X32: case SV_PATH_HALO_BLOCKED_16X16:
      conv_halo_blocked_launch(a.x, a.w, a.y, a.e.stats, a.g.N, a.g.Hi, a.g.Wi, a.g.Ci, a.g.Co, TCONV ? 1 : 0, p.halo, ctr, s);
      return;
    case SV_PATH_WIDE: hipLaunchKernelGGL((gemm_wide_kernel<false, 4, 4, 3>), grid, block, 0, s, a, p.ntiles, ctr); return;
    case SV_PATH_WIDE_GENERAL: hipLaunchKernelGGL((gemm_wide_kernel<true, 4, 4, 3>), grid, block, 0, s, a, p.ntiles, ctr); return;
    default: break;
  }
  with_tile(p.tile, [&](auto tl) {
    typedef decltype(tl) TL;
    if constexpr (!TCONV && TL::BN > 16) {   // the dense kernel is never built for the transposed gather or the 16-column tile
      if (p.q.path == SV_PATH_DENSE) { hipLaunchKernelGGL((gemm_dense_kernel<TL, __bf16, __bf16, 8>), grid, block, 0, s, a, p.ntiles); return; }
    }
    if (p.q.operands == SV_OPERANDS_F32) hipLaunchKernelGGL((igemm_kernel<false, TCONV, TL, float, float, 4>), grid, block, 0, s, a);
    else if (p.q.operands == SV_OPERANDS_BF16_F32) hipLaunchKernelGGL((igemm_kernel<true, TCONV, TL, float, float, 4>), grid, block, 0, s, a);
    else if (p.q.vec == 8) hipLaunchKernelGGL((igemm_kernel<true, TCONV, TL, __bf16, __bf16, 8>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((igemm_kernel<true, TCONV, TL, __bf16, __bf16, 4>), grid, block, 0, s, a);
  });
}

// arguments of a gather call -> plan -> (query: report it) -> launch; behind sv_conv_gather, sv_tconv_gather and sv_conv_gather_plan
static int gather_entry(const void* in, const void* w, void* out, const sv_geom* g, const sv_epilogue* e, int math, int act_dtype, bool transposed,
                        hipStream_t s, sv_launch_plan* query) {
  if (int rc = check_common(g, e, in, w, out, act_dtype)) return rc;
  SV_REQUIRE_ACT(act_dtype);
  SV_REQUIRE(act_dtype == SV_F32 || math == SV_MATH_BF16, "igemm: bf16 activations require SV_MATH_BF16");
  IGemmArgs a{};
  a.x = in; a.w = w; a.y = out; a.g = to_geom(g); a.e = to_epi(e);
  a.Ktot = g->kd * g->kh * g->kw * g->Ci;
  long long M = (long long)g->N * g->Do * g->Ho * g->Wo;
  int ncls = 1;
  if (transposed) {
    SV_REQUIRE(g->sd <= 2 && g->sh <= 2 && g->sw <= 2, "tconv_gather: stride > 2 unsupported (%d,%d,%d)", g->sd, g->sh, g->sw);
    const int O[3] = {g->Do, g->Ho, g->Wo}, S[3] = {g->sd, g->sh, g->sw}, P[3] = {g->pd, g->ph, g->pw}, Kx[3] = {g->kd, g->kh, g->kw};
    ncls = 0; M = 0;
    for (int rd = 0; rd < S[0]; ++rd)
      for (int rh = 0; rh < S[1]; ++rh)
        for (int rw = 0; rw < S[2]; ++rw) {
          const int r[3] = {rd, rh, rw};
          ClassInfo c{};
          long long m = g->N;
          for (int ax = 0; ax < 3; ++ax) {
            c.r[ax] = r[ax];
            c.T[ax] = r[ax] < Kx[ax] ? (Kx[ax] - r[ax] + S[ax] - 1) / S[ax] : 0;
            int o0 = ((r[ax] - P[ax]) % S[ax] + S[ax]) % S[ax];
            c.o0[ax] = o0;
            c.cnt[ax] = o0 < O[ax] ? (O[ax] - o0 + S[ax] - 1) / S[ax] : 0;
            c.ib0[ax] = (o0 + P[ax] - r[ax]) / S[ax];
            m *= c.cnt[ax];
          }
          if (m > M) M = m;
          a.cls[ncls++] = c;
        }
  }
  GatherPlan p = plan_gather(a, M, ncls, math, act_dtype, transposed, true);
  if (query) { *query = p.q; return SV_OK; }
  if (M == 0) return SV_OK;
  // one counter slot per launch, asked for after planning; none to be had: what the plan is without them
  int* ctr = p.counters ? gemm_wide_counters() : nullptr;
  if (p.counters && !ctr) p = plan_gather(a, M, ncls, math, act_dtype, transposed, false);
  if (transposed) launch_gather<true>(p, a, ctr, s);
  else launch_gather<false>(p, a, ctr, s);
  if (p.q.path >= SV_PATH_HALO0) return check_launch(transposed ? "sv_tconv_gather (halo tiles)" : "sv_conv_gather (halo tiles)");
  return check_launch(transposed ? "sv_tconv_gather" : "sv_conv_gather");
}

// ------------------------------------------------------------------------------------------------
// wide weight-gradient kernel of the dense layers (Linear / 1x1 stride-1, bf16 storage):  dW[co][ci] += sum_r dY[r][co] * X[r][ci].
// Same machine as gemm_wide_kernel: one workgroup per CU, 8 consumer waves (4 x 2, 64 x 64 each) on a 256 x 128 tile of dW, 4 producer
// waves that issue the LDS-DMA of 64-row slices of both operands into a ring of three 48 KB slots, one barrier per slice.  The
// contraction runs over ROWS, so both fragments come out of the [row][column] images through ds_read_b64_tr_b16; the 32-byte column
// windows of a row are XOR-swizzled by f(row) = (row & 3) | ((row >> 1) & 4) (applied to the DMA source columns), which spreads the
// 8 rows a 32-lane half reads over all 64 banks.  P = the operand whose columns take the 256-side of the tile (SWAP: X, else dY),
// Q the other; a workgroup owns one tile and a contiguous range of row slices (workgroups of one row range sit on one XCD: they share
// the operand rows through its L2) and adds its fp32 tile into dW once, at the end (16 consecutive floats per lane group).
// Host-side conditions: rows % 64 == 0, 8-aligned columns and row strides, <= 256 tiles (plan_wgrad).
// ------------------------------------------------------------------------------------------------
struct WGradWideArgs {
  const __bf16* P; int ldp; int pcols; const __bf16* Q; int ldq; int qcols;
  float* dw; int ld_dw;                 // dW[co][ci], row stride = Ci
  float* dbias;                         // optional: dbias[co] += sum_r dY[r][co] (the workgroups of ONE column of tiles add them up, from the LDS images)
  int nslices, ntiles, tiles_p, groups; // 64-row slices; tiles = tiles_p x tiles_q; groups = workgroups per tile (grid = ntiles * groups)
};

constexpr int GW_NCONS = 8, GW_NPROD = 4, GW_NTHR = (GW_NCONS + GW_NPROD) * 64, GW_STAGES = 3;                 // geometry of the weight-gradient kernel
constexpr int GW_A_BYTES = 256 * GW_BK * 2, GW_STAGE_BYTES = (256 + GW_BN) * GW_BK * 2;                          // 32 KB + 16 KB
template <bool SWAP>
__global__ __launch_bounds__(GW_NTHR, 3) void wgrad_wide_kernel(const WGradWideArgs p) {
  __shared__ __attribute__((aligned(1024))) char smem[GW_STAGES * GW_STAGE_BYTES];   // ONE object; slot = P image [64][256] | Q image [64][128]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bl = xcd_remap(blockIdx.x, gridDim.x);
  const int tile = bl % p.ntiles, grp = bl / p.ntiles;
  const int p0 = (tile % p.tiles_p) * 256, q0 = (tile / p.tiles_p) * 128;
  const int sbase = p.nslices / p.groups, srem = p.nslices % p.groups;
  const int s0 = grp * sbase + (grp < srem ? grp : srem), nsl = sbase + (grp < srem ? 1 : 0);
  if (nsl <= 0) return;

  if (wave >= GW_NCONS) {
    // ================= producer wave pw: rows 16 pw .. 16 pw + 15 of every slice (8 P pieces of 2 rows, 4 Q pieces of 4 rows) =================
    const int pw = wave - GW_NCONS;
    const __bf16* pp_[8];
    const __bf16* qp_[4];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int b = lane >> 5, cd = lane & 31, R = 16 * pw + 2 * i + b;
      const int fR = (((i & 1) << 1) | b) | (((i >> 2) & 1) << 2);
      int col = p0 + ((((cd >> 1) ^ fR) << 1) | (cd & 1)) * 8;
      if (col > p.pcols - 8) col = p.pcols - 8;          // columns past the operand: any valid chunk, the epilogue skips those outputs
      pp_[i] = p.P + (size_t)(s0 * 64 + R) * p.ldp + col;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int b = lane >> 4, cd = lane & 15, R = 16 * pw + 4 * i + b;
      const int fR = b | (((i >> 1) & 1) << 2);
      int col = q0 + ((((cd >> 1) ^ fR) << 1) | (cd & 1)) * 8;
      if (col > p.qcols - 8) col = p.qcols - 8;
      qp_[i] = p.Q + (size_t)(s0 * 64 + R) * p.ldq + col;
    }
    auto issue = [&](int kt, int st) {
      char* base = smem + st * GW_STAGE_BYTES;
#pragma unroll
      for (int i = 0; i < 8; ++i)
        __builtin_amdgcn_global_load_lds((gw_gptr_t)(pp_[i] + (size_t)kt * 64 * p.ldp), (gw_lptr_t)(base + (pw * 8 + i) * 1024), 16, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        __builtin_amdgcn_global_load_lds((gw_gptr_t)(qp_[i] + (size_t)kt * 64 * p.ldq), (gw_lptr_t)(base + GW_A_BYTES + (pw * 4 + i) * 1024), 16, 0, 0);
    };
    // bias gradient: the dY image of the slice (P, or Q when SWAP) is summed by the producers - each wave its own 16 rows, a lane 4 columns
    // (8-byte reads through the same window swizzle) - while the consumers contract the slice; only the tiles of the first Q (P) column do it
    const bool do_bias = p.dbias != nullptr && (SWAP ? tile % p.tiles_p == 0 : tile / p.tiles_p == 0);
    float bs[4] = {0.f, 0.f, 0.f, 0.f};
    issue(0, 0);
    if (nsl > 1) issue(1, 1);
    int st = 0;
    for (int kt = 0; kt < nsl; ++kt) {
      if (kt + 1 < nsl) asm volatile("s_waitcnt vmcnt(12)\n\ts_barrier" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
      if (kt + 2 < nsl) issue(kt + 2, st == 0 ? 2 : st - 1);
      if (do_bias) {
        const char* sb = smem + st * GW_STAGE_BYTES;
        if constexpr (!SWAP) {
#pragma unroll
          for (int rr = 0; rr < 16; ++rr) {
            const int R = 16 * pw + rr, fR = (R & 3) | ((R >> 1) & 4);
            const bf16x4 v = *reinterpret_cast<const bf16x4*>(sb + R * 512 + (((lane >> 2) ^ fR) << 5) + (lane & 3) * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) bs[j] += (float)v[j];
          }
        } else {
#pragma unroll
          for (int rr = 0; rr < 8; ++rr) {   // 32 lanes cover the 128 columns of a row: two rows per read
            const int R = 16 * pw + 2 * rr + (lane >> 5), fR = (R & 3) | ((R >> 1) & 4);
            const bf16x4 v = *reinterpret_cast<const bf16x4*>(sb + GW_A_BYTES + R * 256 + ((((lane >> 2) & 7) ^ fR) << 5) + (lane & 3) * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) bs[j] += (float)v[j];
          }
        }
      }
      st = st == 2 ? 0 : st + 1;
    }
    if (do_bias) {
      const int c0 = SWAP ? q0 + (lane & 31) * 4 : p0 + lane * 4, ncol = SWAP ? p.qcols : p.pcols;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c0 + j < ncol) atomicAdd(p.dbias + c0 + j, bs[j]);
    }
    return;
  }

  // ================= consumer waves: 4 (P) x 2 (Q) grid of 64 x 64 wave tiles =================
  const int wm = wave >> 1, wn = wave & 1, lr = lane & 15, lg = lane >> 4, q = lr >> 2, pq = lr & 3;
  // fragment (block mt / nt, step ks, half hi) = rows 32 ks + 8 lg + q + 4 hi, 32-byte window (4 wm + mt) ^ f, f = q | (lg & 1) << 2
  int pofs[4], qofs[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    pofs[t] = (lg * 8 + q) * 512 + pq * 8 + ((wm >> 1) * 8 + (((wm & 1) ^ (lg & 1)) * 4) + (t ^ q)) * 32;
    qofs[t] = GW_A_BYTES + (lg * 8 + q) * 256 + pq * 8 + (((wn ^ (lg & 1)) * 4) + (t ^ q)) * 32;
  }
  f32x4 acc[4][4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  int st = 0;
  for (int kt = 0; kt < nsl; ++kt) {
    asm volatile("s_barrier" ::: "memory");               // the slice has landed (the producers waited for it before this barrier)
    const char* sb = smem + st * GW_STAGE_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 pf[4], qf[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const bf16x4 plo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(sb + pofs[t] + ks * 16384));
        const bf16x4 phi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(sb + pofs[t] + ks * 16384 + 2048));
        pf[t] = __builtin_shufflevector(plo, phi, 0, 1, 2, 3, 4, 5, 6, 7);
        const bf16x4 qlo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(sb + qofs[t] + ks * 8192));
        const bf16x4 qhi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(sb + qofs[t] + ks * 8192 + 1024));
        qf[t] = __builtin_shufflevector(qlo, qhi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          acc[mt][nt] = SWAP ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[nt], pf[mt], acc[mt][nt], 0, 0, 0)
                             : __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf[mt], qf[nt], acc[mt][nt], 0, 0, 0);
    }
    st = st == 2 ? 0 : st + 1;
  }
  // ---- one fp32 atomic add per element into dW[co][ci]: a lane group's 16 lanes hit 16 consecutive floats
  //      !SWAP: acc row (4 lg + j) = P column (co), acc column lr = Q column (ci);  SWAP: acc row = Q column (co), acc column = P column (ci)
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int pi = p0 + wm * 64 + mt * 16 + (SWAP ? lr : lg * 4 + j), qi = q0 + wn * 64 + nt * 16 + (SWAP ? lg * 4 + j : lr);
        if (pi < p.pcols && qi < p.qcols) atomicAdd(p.dw + (SWAP ? (size_t)qi * p.ld_dw + pi : (size_t)pi * p.ld_dw + qi), acc[mt][nt][j]);
      }
}

typedef Tile<4, 2, 2, 2> WTileDefault;   // 128 anchor channels x 64 (tap, gathered channel), 8 waves
typedef Tile<1, 4, 1, 2> WTileNarrow;    // 16 x 128 for <=16 anchor channels
typedef Tile<2, 4, 4, 2> WTileWide;      // 128 x 128, 8 waves
typedef Tile<2, 4, 2, 2> WTile64;        // 64 x 128, 8 waves: layers with <= 64 anchor channels (half of a 128-row tile would multiply zeros)
typedef Tile<2, 4, 3, 2> WTile96;        // 96 x 128, 8 waves: anchor channel counts 96 k that are not multiples of 128 (Swin stage 0)

// ---- launch plan of sv_conv_wgrad (pure host function; sv_conv_wgrad_plan reports it).  Order: halo tiles, wide kernel, tiled kernel ----
enum { WTILE_NARROW, WTILE_64, WTILE_96, WTILE_WIDE, WTILE_DEFAULT };
struct WGradPlan {
  sv_launch_plan q;              // path, tile, operand variant, grid, block: what the query reports
  int tile, rows_per_split;      // tiled kernel: WTILE_*, positions per split (grid = tiles x splits)
  int ntiles, tiles_p, groups;   // wide kernel: 256 x 128 tiles, of which tiles_p along the 256-side; workgroups per tile
  HaloPlan halo;                 // halo weight gradient: tile shape, stride, splits
};
template <typename F> static void with_wtile(int tile, F&& f) {
  switch (tile) {
    case WTILE_NARROW: f(WTileNarrow{}); break;
    case WTILE_64: f(WTile64{}); break;
    case WTILE_96: f(WTile96{}); break;
    case WTILE_WIDE: f(WTileWide{}); break;
    default: f(WTileDefault{}); break;
  }
}

static WGradPlan plan_wgrad(const void* anchor, int lda, const void* gathered, const sv_geom* g, int cg_valid, int math, int act) {
  WGradPlan p{};
  const long long Mll = (long long)g->N * g->Do * g->Ho * g->Wo;
  const int Kout = g->kd * g->kh * g->kw * g->Ci;
  const bool bf = math == SV_MATH_BF16, bf16 = bf && act == SV_BF16, aligned16 = (((uintptr_t)anchor | (uintptr_t)gathered) & 15) == 0;
  p.q.operands = !bf ? SV_OPERANDS_F32 : act != SV_BF16 ? SV_OPERANDS_BF16_F32 : SV_OPERANDS_BF16;
  p.q.vec = 8; p.q.grid_y = 1;
  // 3 x 3 / stride 1 or 2 / padding 1 with 64 k channels on both sides and bf16 storage: the halo-tile weight gradient (conv_halo.hip) fills the
  // packed workspace
  if (bf16 && g->kd == 1 && g->kh == 3 && g->kw == 3 && g->sd == 1 && g->sh == g->sw && g->pd == 0 && g->ph == 1 && g->pw == 1 && g->Di == 1 &&
      g->Do == 1 && cg_valid == g->Ci && lda == g->Co && g->ldi == g->Ci && aligned16 &&
      (p.halo = conv_halo_wgrad_plan(g->N, g->Hi, g->Wi, g->Ho, g->Wo, g->sh, g->Ci, g->Co)).kind >= 0) {
    p.q.path = SV_PATH_WGRAD_HALO; p.q.tile_rows = p.halo.th; p.q.tile_cols = p.halo.tw; p.q.grid_x = p.halo.grid; p.q.block = 256;
    return p;
  }
  // dense layers with bf16 storage take the wide weight-gradient kernel (SV_WGRAD_WIDE=0 in the environment keeps the 128-wide one)
  static const int wide_on = [] { const char* v = getenv("SV_WGRAD_WIDE"); return v ? atoi(v) : 1; }();
  const bool same_rows = g->kd * g->kh * g->kw == 1 && g->sd == 1 && g->sh == 1 && g->sw == 1 && g->pd == 0 && g->ph == 0 && g->pw == 0 &&
                         g->Di == g->Do && g->Hi == g->Ho && g->Wi == g->Wo;
  if (wide_on && same_rows && bf16 && cg_valid == g->Ci && Mll % 64 == 0 && Mll >= 16384 && g->Co >= 128 && g->Ci >= 128 &&
      ((g->Co | g->Ci | lda | g->ldi) & 7) == 0 && aligned16) {
    // the 256-side of the tile goes to the operand it wastes less on (dY columns = Co, X columns = Ci)
    const long long w0 = (long long)cdiv(g->Co, 256) * 256 * cdiv(g->Ci, 128) * 128, w1 = (long long)cdiv(g->Ci, 256) * 256 * cdiv(g->Co, 128) * 128;
    const bool swap = w1 < w0;
    const int tiles_p = cdiv(swap ? g->Ci : g->Co, 256);
    const long long ntiles = (long long)tiles_p * cdiv(swap ? g->Co : g->Ci, 128);
    if (ntiles <= 256) {   // one workgroup per CU owns a tile (this also bounds the 128 x 128 blocks of dW by 512, the earlier pre-check)
      p.ntiles = (int)ntiles; p.tiles_p = tiles_p;
      p.groups = 256 / p.ntiles;
      if (p.groups > Mll / 64) p.groups = (int)(Mll / 64);
      p.q.path = swap ? SV_PATH_WGRAD_WIDE_SWAP : SV_PATH_WGRAD_WIDE;
      p.q.tile_rows = 256; p.q.tile_cols = GW_BN; p.q.grid_x = p.ntiles * p.groups; p.q.block = GW_NTHR;
      return p;
    }
  }
  const bool narrow = g->Co <= 16;
  const bool wide = !narrow && Kout >= 128;      // 128 x 128 tile: the anchor operand is re-read once per 128 (tap, channel) columns
  static const int tile64_on = [] { const char* v = getenv("SV_WGRAD_TILE64"); return v ? atoi(v) : 1; }();
  const bool t64 = tile64_on && wide && g->Co <= 64;
  const bool t96 = tile64_on && wide && !t64 && g->Co % 96 == 0 && g->Co % 128 != 0;
  p.tile = narrow ? WTILE_NARROW : t64 ? WTILE_64 : t96 ? WTILE_96 : wide ? WTILE_WIDE : WTILE_DEFAULT;
  with_wtile(p.tile, [&](auto tl) { typedef decltype(tl) TL; p.q.tile_rows = TL::BM; p.q.tile_cols = TL::BN; p.q.block = TL::NTHR; });
  const int BKs = bf ? 64 : 32;
  const int tiles = cdiv(g->Co, p.q.tile_rows) * cdiv(Kout, p.q.tile_cols);
  // at most ONE wave of workgroups (2 resident per CU x 256 CUs = 512 slots) and >= 8 K-steps per split.  Every workgroup
  // does the same amount of work, so tiles * splits must not exceed the slots: rounding the split count UP (e.g. 36 tiles
  // x 15 = 540) leaves a 28-workgroup second wave that costs as much as the first (measured: 173 -> ~90 us for 384x1536 over
  // 50 176 rows).  Fewer, longer splits also halve the fp32 atomic traffic of the epilogue.
  const int slots = 512, min_ksteps = 8;
  long long splits = tiles <= slots ? slots / tiles : 1;
  const long long max_splits = (Mll + min_ksteps * BKs - 1) / (min_ksteps * BKs);
  if (splits > max_splits) splits = max_splits;
  if (splits < 1) splits = 1;
  if (splits > 65535) splits = 65535;
  long long rps = (Mll + splits - 1) / splits;
  rps = (rps + BKs - 1) / BKs * BKs;
  splits = (Mll + rps - 1) / rps;
  p.rows_per_split = (int)rps;
  // 16-byte operand chunks with bf16 storage when every row start and channel count allows it (Co % 8 keeps the edge
  // chunk of the anchor whole; otherwise the 4-element variant with its scalar edge path is used)
  const bool v8 = act == SV_BF16 && (lda % 8) == 0 && (g->Co % 8) == 0 && (g->Ci % 8) == 0 && (g->ldi % 8) == 0 && aligned16;
  p.q.path = SV_PATH_WGRAD_TILED; p.q.vec = v8 ? 8 : 4; p.q.grid_x = (int)(unsigned)(tiles * splits);
  return p;
}

// arguments of a weight-gradient call -> plan -> (query: report it) -> launch; behind sv_conv_wgrad and sv_conv_wgrad_plan
static int wgrad_entry(const void* anchor, int lda, const void* gathered, float* dw, const sv_geom* g, int cg_valid, float* workspace, float* dbias,
                       int math, int act, hipStream_t s, sv_launch_plan* query) {
  SV_REQUIRE(anchor && gathered && g && (dw || query), "wgrad: null argument");
  SV_REQUIRE_ACT(act);
  SV_REQUIRE(act == SV_F32 || math == SV_MATH_BF16, "wgrad: bf16 activations require SV_MATH_BF16");
  SV_REQUIRE(lda >= g->Co && g->ldi >= g->Ci && cg_valid > 0 && cg_valid <= g->Ci, "wgrad: bad strides (lda=%d Co=%d ldi=%d Ci=%d cg_valid=%d)",
             lda, g->Co, g->ldi, g->Ci, cg_valid);
  SV_REQUIRE((((uintptr_t)anchor | (uintptr_t)gathered) & (act == SV_BF16 ? 7 : 15)) == 0, "wgrad: operands must be aligned to 4 elements");
  const long long Mll = (long long)g->N * g->Do * g->Ho * g->Wo;
  SV_REQUIRE(Mll > 0 && Mll < (1ll << 31), "wgrad: row count out of range");
  const int taps = g->kd * g->kh * g->kw;
  const WGradPlan p = plan_wgrad(anchor, lda, gathered, g, cg_valid, math, act);
  if (query) { *query = p.q; return SV_OK; }
  SV_REQUIRE(taps == 1 || workspace, "wgrad: a workspace of sv_conv_wgrad_workspace_floats() floats is required when taps > 1");
  WGradArgs a{};
  a.anchor = anchor; a.lda = lda; a.gathered = gathered; a.g = to_geom(g); a.cg_valid = cg_valid;
  a.Mrows = (int)Mll;
  a.direct = taps == 1;
  a.dbias = dbias;
  a.out = a.direct ? dw : workspace;
  a.rows_per_split = p.rows_per_split;
  if (!a.direct) (void)hipMemsetAsync(workspace, 0, sizeof(float) * (size_t)g->Co * taps * g->Ci, s);
  const dim3 grid(p.q.grid_x), block(p.q.block);
  switch (p.q.path) {
    case SV_PATH_WGRAD_HALO:
      conv_halo_wgrad_launch(gathered, anchor, workspace, dbias, g->N, g->Hi, g->Wi, g->Ho, g->Wo, g->Ci, g->Co, p.halo, s);
      break;
    case SV_PATH_WGRAD_WIDE: case SV_PATH_WGRAD_WIDE_SWAP: {
      const bool swap = p.q.path == SV_PATH_WGRAD_WIDE_SWAP;
      WGradWideArgs wa{};
      wa.P = static_cast<const __bf16*>(swap ? gathered : anchor); wa.ldp = swap ? g->ldi : lda; wa.pcols = swap ? g->Ci : g->Co;
      wa.Q = static_cast<const __bf16*>(swap ? anchor : gathered); wa.ldq = swap ? lda : g->ldi; wa.qcols = swap ? g->Co : g->Ci;
      wa.dw = dw; wa.ld_dw = g->Ci; wa.nslices = (int)(Mll / 64); wa.ntiles = p.ntiles; wa.tiles_p = p.tiles_p; wa.groups = p.groups;
      wa.dbias = dbias;
      if (swap) hipLaunchKernelGGL(wgrad_wide_kernel<true>, grid, block, 0, s, wa);
      else hipLaunchKernelGGL(wgrad_wide_kernel<false>, grid, block, 0, s, wa);
      break;
    }
    default:
      with_wtile(p.tile, [&](auto tl) {
        typedef decltype(tl) TL;
        if (p.q.operands == SV_OPERANDS_F32) hipLaunchKernelGGL((wgrad_kernel<false, TL, float, 4>), grid, block, 0, s, a);
        else if (p.q.operands == SV_OPERANDS_BF16_F32) hipLaunchKernelGGL((wgrad_kernel<true, TL, float, 4>), grid, block, 0, s, a);
        else if (p.q.vec == 8) hipLaunchKernelGGL((wgrad_kernel<true, TL, __bf16, 8>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((wgrad_kernel<true, TL, __bf16, 4>), grid, block, 0, s, a);
      });
  }
  if (!a.direct) {   // the packed workspace of the halo and the tiled kernel -> dw
    const long long total = (long long)g->Co * cg_valid * taps;
    int blocks = cdiv(total, 256); if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(wgrad_unpack_kernel, dim3(blocks), dim3(256), 0, s, workspace, dw, g->Co, g->Ci, cg_valid, taps);
  }
  return check_launch(p.q.path == SV_PATH_WGRAD_HALO ? "sv_conv_wgrad (halo tiles)" : "sv_conv_wgrad");
}

}  // namespace sv

using namespace sv;

extern "C" int sv_conv_gather(const void* in, const void* w, void* out, const sv_geom* g, const sv_epilogue* e,
                              int math, int act_dtype, void* stream) {
  return gather_entry(in, w, out, g, e, math, act_dtype, false, (hipStream_t)stream, nullptr);
}
extern "C" int sv_tconv_gather(const void* in, const void* w, void* out, const sv_geom* g, const sv_epilogue* e,
                               int math, int act_dtype, void* stream) {
  return gather_entry(in, w, out, g, e, math, act_dtype, true, (hipStream_t)stream, nullptr);
}
extern "C" int sv_conv_gather_plan(const void* in, const void* w, void* out, const sv_geom* g, const sv_epilogue* e, int math, int act_dtype,
                                   int transposed, sv_launch_plan* plan) {
  SV_REQUIRE(plan, "conv_gather_plan: null plan");
  return gather_entry(in, w, out, g, e, math, act_dtype, transposed != 0, nullptr, plan);
}
extern "C" int sv_conv_gather_is_wide(const void* in, const void* w, void* out, const sv_geom* g, const sv_epilogue* e, int math, int act_dtype) {
  sv_launch_plan q;
  return sv_conv_gather_plan(in, w, out, g, e, math, act_dtype, 0, &q) == SV_OK && (q.path == SV_PATH_WIDE || q.path == SV_PATH_WIDE_GENERAL);
}

extern "C" size_t sv_conv_wgrad_workspace_floats(const sv_geom* g) {
  const int taps = g->kd * g->kh * g->kw;
  return taps == 1 ? 0 : (size_t)g->Co * taps * g->Ci;
}
extern "C" int sv_conv_wgrad(const void* anchor, int lda, const void* gathered, float* dw, const sv_geom* g, int cg_valid,
                             float* workspace, float* dbias, int math, int act_dtype, void* stream) {
  return wgrad_entry(anchor, lda, gathered, dw, g, cg_valid, workspace, dbias, math, act_dtype, (hipStream_t)stream, nullptr);
}
extern "C" int sv_conv_wgrad_plan(const void* anchor, int lda, const void* gathered, const sv_geom* g, int cg_valid, int math, int act_dtype,
                                  sv_launch_plan* plan) {
  SV_REQUIRE(plan, "conv_wgrad_plan: null plan");
  return wgrad_entry(anchor, lda, gathered, nullptr, g, cg_valid, nullptr, nullptr, math, act_dtype, nullptr, plan);
}
extern "C" int sv_conv_wgrad_is_wide(const void* anchor, int lda, const void* gathered, const sv_geom* g, int cg_valid, int math, int act_dtype) {
  sv_launch_plan q;
  return sv_conv_wgrad_plan(anchor, lda, gathered, g, cg_valid, math, act_dtype, &q) == SV_OK &&
         (q.path == SV_PATH_WGRAD_WIDE || q.path == SV_PATH_WGRAD_WIDE_SWAP);
}

extern "C" int sv_pack_weight(const float* src, void* dst, int A, int B, int T, int swap, int pad_to, int out_dtype, void* stream) {
  SV_REQUIRE(src && dst && A > 0 && B > 0 && T > 0, "pack_weight: bad arguments");
  SV_REQUIRE_ACT(out_dtype);
  const int rows_out = swap ? B : A;
  int inner = swap ? A : B;
  if (pad_to > inner) inner = pad_to;
  const long long total = (long long)rows_out * T * inner;
  int blocks = cdiv(total, 256); if (blocks > 4096) blocks = 4096;
  if (out_dtype == SV_BF16)
    hipLaunchKernelGGL(pack_weight_kernel<__bf16>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, static_cast<__bf16*>(dst), A, B, T, swap, rows_out, inner);
  else
    hipLaunchKernelGGL(pack_weight_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, static_cast<float*>(dst), A, B, T, swap, rows_out, inner);
  return check_launch("sv_pack_weight");
}

extern "C" int sv_pack_weights_block_elems(void) { return PACK_PER_BLOCK; }

extern "C" int sv_pack_weights(const sv_pack_desc* descs_dev, int n, int total_blocks, int out_dtype, void* stream) {
  SV_REQUIRE(descs_dev && n > 0 && total_blocks > 0, "pack_weights: bad arguments");
  SV_REQUIRE_ACT(out_dtype);
  if (out_dtype == SV_BF16) hipLaunchKernelGGL(pack_weights_batched_kernel<__bf16>, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, descs_dev, n);
  else hipLaunchKernelGGL(pack_weights_batched_kernel<float>, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, descs_dev, n);
  return check_launch("sv_pack_weights");
}

extern "C" int sv_colsum(const void* x, int rows, int cols, int ld, float* out, int accumulate, int act_dtype, void* stream) {
  SV_REQUIRE(x && out && rows > 0 && cols > 0 && ld >= cols, "colsum: bad arguments");
  SV_REQUIRE_ACT(act_dtype);
  hipStream_t s = (hipStream_t)stream;
  if (!accumulate) (void)hipMemsetAsync(out, 0, sizeof(float) * cols, s);
  const int cg = cdiv(cols, 64);
  int splits = 2048 / cg; if (splits < 1) splits = 1;
  if (splits > 128) splits = 128;            // every split ends in one atomic per column: keep the contention per address low
  const int maxs = cdiv(rows, 64); if (splits > maxs) splits = maxs;
  const long long rpb = (rows + splits - 1) / splits;
  SV_DISPATCH_ACT(act_dtype, hipLaunchKernelGGL(colsum_kernel<AT>, dim3(cg, cdiv(rows, rpb)), dim3(256), 0, s, static_cast<const AT*>(x),
                                                (long long)rows, cols, ld, out, rpb););
  return check_launch("sv_colsum");
}
