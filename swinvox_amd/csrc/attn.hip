// Attention kernels.
//  * Swin window / shifted-window attention core (timm WindowAttention behind models/swin_transformer.py:78).  The cyclic shift, the
//    7x7 window partition/reverse and the 9-region shift mask are folded into the token index math (no materialised roll); the q/k/v
//    tiles of a window are staged in LDS, every product runs on MFMA, the softmax runs on the accumulator registers.
//      - exact fp32: one WAVE per (image, window, head), the whole 64 x 64 score matrix in registers (win_attn_fwd_kernel / _bwd_kernel);
//      - bf16 and fp8 (e4m3) MFMA: one WORKGROUP per (window, head), each of its 4 waves owns 16 queries (win_attn_*_wg_*kernel);
//      - stage-0 blocks (C = 96): LayerNorm, qkv, attention, projection and residual in one kernel each way (swin_attn_block_*_kernel).
//    A wave's 16 x 64 score strip comes in two layouts.  STRIP (queries 4 lg + j, key 16 nt + lr; fp32 and fp8 kernels) is owned by
//    strip_bias / bias_mask_softmax_strip; QUERY-IN-LANE (query lr, keys 16 nt + 4 lg + j; bf16 and fused kernels) by lane_bias /
//    seam_kdiff / softmax_lane.  dbias_flush takes the bias-table gradient of either layout to HBM.
//  * Cross-view attention core (models/cross_view_attention.py:81-105): one workgroup per (sample, head),
//    V x V scores over 288-long features -- tiny, plain FMA.
#include "common.h"
#include "mx_frag.h"
#include <atomic>

namespace sv {

constexpr int WT = 49;      // tokens per window
constexpr int HD = 32;       // head dim (Swin-T/B: always 32)
constexpr int LDQ_F = 36;    // fp32 row stride of q/k/v tiles
constexpr int LDP_F = 68;    // fp32 row stride of the P tile
constexpr int LDQ_H = 40;    // bf16 row stride of q/k tiles
constexpr int LDP_H = 72;    // bf16 row stride of P and V^T tiles

template <typename AT>
struct WinArgsT {   // AT = storage element of the activations (qkv, out and their gradients)
  const AT* qkv; const float* table; AT* out;   // fwd
  const AT* dout; AT* dqkv; float* dtable;      // bwd
  int I, H, W, C, heads, shift; float scale; int ntasks; int tasks_per_wave;
};
typedef WinArgsT<float> WinArgs;

struct TokMap {  // window -> token rows of the un-shifted [I,H,W] map
  int img, wy, wx, H, W, shift;
  __device__ __forceinline__ long long row(int t) const {
    const int ty = t / 7, tx = t - ty * 7;
    int ys = wy * 7 + ty + shift; if (ys >= H) ys -= H;
    int xs = wx * 7 + tx + shift; if (xs >= W) xs -= W;
    return ((long long)img * H + ys) * W + xs;
  }
  __device__ __forceinline__ int region(int t) const {  // 9-region id in the rolled frame
    const int ty = t / 7, tx = t - ty * 7;
    const int ry = wy * 7 + ty, rx = wx * 7 + tx;
    const int a = ry < H - 7 ? 0 : (ry < H - shift ? 1 : 2);
    const int b = rx < W - 7 ? 0 : (rx < W - shift ? 1 : 2);
    return a * 3 + b;
  }
  // a window touching the rolled seam (last window row / column of a shifted block): tokens of different regions must not attend to each other
  __device__ __forceinline__ bool seam() const { return shift > 0 && (wy == H / 7 - 1 || wx == W / 7 - 1); }
};
__device__ __forceinline__ TokMap task_map(long long task, int nW, int nWx, int H, int W, int shift) {
  TokMap tm;
  tm.img = (int)(task / nW); const int win = (int)(task - (long long)tm.img * nW);
  tm.wy = win / nWx; tm.wx = win - tm.wy * nWx; tm.H = H; tm.W = W; tm.shift = shift;
  return tm;
}
// row of the [169] relative-position-bias table of a head for (query, key) tokens of a window
__device__ __forceinline__ int rel_index(int q, int key) {
  const int qy = q / 7, qx = q - qy * 7, ky = key / 7, kx = key - ky * 7;
  return (qy - ky + 6) * 13 + (qx - kx + 6);
}

// all-reduce over the 16 lanes of a DPP row, every lane gets the result: quad_perm xor 1, xor 2, row_half_mirror (i <-> 7 - i: the two quads
// of a half), row_mirror (i <-> 15 - i: the two halves).  Four VALU DPP moves instead of four ds_bpermute round trips through the LDS crossbar.
template <int CTRL> __device__ __forceinline__ float dpp_mov(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float group16_max(float v) {
  v = fmaxf(v, dpp_mov<0xB1>(v));     // quad_perm [1,0,3,2]
  v = fmaxf(v, dpp_mov<0x4E>(v));     // quad_perm [2,3,0,1]
  v = fmaxf(v, dpp_mov<0x141>(v));    // row_half_mirror
  v = fmaxf(v, dpp_mov<0x140>(v));    // row_mirror
  return v;
}
__device__ __forceinline__ float group16_sum(float v) {
  v += dpp_mov<0xB1>(v); v += dpp_mov<0x4E>(v); v += dpp_mov<0x141>(v); v += dpp_mov<0x140>(v);
  return v;
}

// all-reduce over the four 16-lane groups of a wave (lanes l, l^16, l^32, l^48) on the VALU: the v_permlane16_swap / v_permlane32_swap
// exchanges of common.h (no LDS crossbar round trip as ds_bpermute / __shfl_xor would take)
template <typename OP> __device__ __forceinline__ float lanegroup_allreduce(float v, OP op) {
  float w = v;
  permlane16_pair(v, w);
  v = op(v, w); w = v;
  permlane32_pair(v, w);
  return op(v, w);
}

// scores (+bias, +mask, key padding) -> softmax, all on the 4x4 grid of 16x16 accumulator tiles of one wave.
// element (q = mt*16 + lg*4 + j, key = nt*16 + lr)
__device__ __forceinline__ void bias_mask_softmax(f32x4 (&s)[4][4], const float* bt, const TokMap& tm, int lane, bool shifted) {
  const int lr = lane & 15, lg = lane >> 4;
  int kreg[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int key = nt * 16 + lr;
    kreg[nt] = (shifted && key < WT) ? tm.region(key) : 0;
  }
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = mt * 16 + lg * 4 + j;
      const int qreg = (shifted && q < WT) ? tm.region(q) : 0;
      float mx = -3.0e38f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int key = nt * 16 + lr;
        float v = s[mt][nt][j];
        if (key >= WT) v = -1.0e30f;
        else if (q < WT) {
          v += bt[rel_index(q, key)];
          if (shifted && qreg != kreg[nt]) v += -100.0f;
        }
        s[mt][nt][j] = v;
        mx = fmaxf(mx, v);
      }
      mx = group16_max(mx);
      float sum = 0.f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) { const float e = expf(s[mt][nt][j] - mx); s[mt][nt][j] = e; sum += e; }
      const float inv = 1.f / group16_sum(sum);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) s[mt][nt][j] *= inv;
    }
}

// load one [49(64) x 32] head slice of q, k or v (or dO) into an fp32 LDS tile, rows >= 49 zeroed
template <typename AT>
__device__ __forceinline__ void load_tile_f32(float* dst, const AT* src, int ld, int col, const TokMap& tm, int lane, float mul) {
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int r = (lane >> 3) + 8 * it, ch = (lane & 7) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < WT) {
      v = ld4f(src + (size_t)tm.row(r) * ld + col + ch);
      v.x *= mul; v.y *= mul; v.z *= mul; v.w *= mul;
    }
    *reinterpret_cast<float4*>(dst + r * LDQ_F + ch) = v;
  }
}

// forward (exact fp32 MFMA): one wave per (image, window, head), four waves per workgroup
__global__ __launch_bounds__(256) void win_attn_fwd_kernel(const WinArgs p) {
  constexpr int WAVE_BYTES = 3 * 64 * LDQ_F * 4 + 176 * 4;
  __shared__ __attribute__((aligned(16))) char smem[4 * WAVE_BYTES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int head = blockIdx.y;
  const int nWx = p.W / 7, nW = (p.H / 7) * nWx;
  long long task = (long long)blockIdx.x * 4 + wave;
  const bool active = task < p.ntasks;
  if (!active) task = p.ntasks - 1;
  const TokMap tm = task_map(task, nW, nWx, p.H, p.W, p.shift);
  const int ld = 3 * p.C, colq = head * HD;
  char* base = smem + wave * WAVE_BYTES;
  float* bt = reinterpret_cast<float*>(base + WAVE_BYTES - 176 * 4);
  for (int i = lane; i < 169; i += 64) bt[i] = p.table[i * p.heads + head];

  f32x4 s[4][4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) s[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  f32x4 o[4][2];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) { o[mt][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; o[mt][1] = (f32x4){0.f, 0.f, 0.f, 0.f}; }

  float* Qs = reinterpret_cast<float*>(base);
  float* Ks = Qs + 64 * LDQ_F;
  float* Vs = Ks + 64 * LDQ_F;
  float* Ps = Qs;  // aliases Q,K once the scores are in registers
  load_tile_f32(Qs, p.qkv, ld, colq, tm, lane, p.scale);
  load_tile_f32(Ks, p.qkv, ld, p.C + colq, tm, lane, 1.f);
  load_tile_f32(Vs, p.qkv, ld, 2 * p.C + colq, tm, lane, 1.f);
  __syncthreads();
#pragma unroll
  for (int kk = 0; kk < HD / 4; ++kk) {
    float a[4], b[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { a[t] = Qs[(t * 16 + lr) * LDQ_F + kk * 4 + lg]; b[t] = Ks[(t * 16 + lr) * LDQ_F + kk * 4 + lg]; }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) s[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], b[nt], s[mt][nt], 0, 0, 0);
  }
  bias_mask_softmax(s, bt, tm, lane, p.shift > 0);
  __syncthreads();
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int j = 0; j < 4; ++j) Ps[(mt * 16 + lg * 4 + j) * LDP_F + nt * 16 + lr] = s[mt][nt][j];
  __syncthreads();
#pragma unroll 4
  for (int kk = 0; kk < 16; ++kk) {
    float a[4], b[2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) a[mt] = Ps[(mt * 16 + lr) * LDP_F + kk * 4 + lg];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) b[nt] = Vs[(kk * 4 + lg) * LDQ_F + nt * 16 + lr];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) o[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], b[nt], o[mt][nt], 0, 0, 0);
  }
  if (active) {
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int q = mt * 16 + lg * 4 + j;
        if (q < WT) {
          float* dst = p.out + (size_t)tm.row(q) * p.C + colq;
          dst[lr] = o[mt][0][j]; dst[16 + lr] = o[mt][1][j];
        }
      }
  }
}

// backward (exact fp32 MFMA): recompute P, then dV = P^T dO, dP = dO V^T, dS = P o (dP - rowsum(dP o P)),
// dQ = scale * dS K, dK = dS^T (scale*Q), dtable[idx] += dS.  Two waves per workgroup; a wave walks
// tasks_per_wave windows of ONE head so its relative-position-bias gradient is reduced in LDS first.
constexpr int BWD_WAVE_FLOATS = 4 * 64 * LDQ_F + 64 * LDP_F + 176 + 176;

__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(1, 1))) void win_attn_bwd_kernel(const WinArgs p) {
  __shared__ __attribute__((aligned(16))) float smem[2 * BWD_WAVE_FLOATS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int head = blockIdx.y;
  const int nWx = p.W / 7, nW = (p.H / 7) * nWx;
  float* Qs = smem + wave * BWD_WAVE_FLOATS;
  float* Ks = Qs + 64 * LDQ_F;
  float* Vs = Ks + 64 * LDQ_F;
  float* Ds = Vs + 64 * LDQ_F;
  float* PS = Ds + 64 * LDQ_F;
  float* bt = PS + 64 * LDP_F;
  float* dbt = bt + 176;
  for (int i = lane; i < 176; i += 64) { bt[i] = i < 169 ? p.table[i * p.heads + head] : 0.f; dbt[i] = 0.f; }
  const int ld = 3 * p.C, colq = head * HD;
  const long long task0 = ((long long)blockIdx.x * 2 + wave) * p.tasks_per_wave;

  for (int tt = 0; tt < p.tasks_per_wave; ++tt) {
    long long task = task0 + tt;
    const bool active = task < p.ntasks;   // inactive waves keep running (barriers) on a clamped task, stores suppressed
    if (!active) task = p.ntasks - 1;
    const TokMap tm = task_map(task, nW, nWx, p.H, p.W, p.shift);

    __syncthreads();  // previous task's LDS reads done
    load_tile_f32(Qs, p.qkv, ld, colq, tm, lane, p.scale);
    load_tile_f32(Ks, p.qkv, ld, p.C + colq, tm, lane, 1.f);
    load_tile_f32(Vs, p.qkv, ld, 2 * p.C + colq, tm, lane, 1.f);
    load_tile_f32(Ds, p.dout, p.C, colq, tm, lane, 1.f);
    __syncthreads();

    f32x4 s[4][4], dp[4][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) { s[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f}; dp[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
    for (int kk = 0; kk < HD / 4; ++kk) {
      float a[4], b[4], c[4], d[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int off = (t * 16 + lr) * LDQ_F + kk * 4 + lg;
        a[t] = Qs[off]; b[t] = Ks[off]; c[t] = Ds[off]; d[t] = Vs[off];
      }
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          s[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], b[nt], s[mt][nt], 0, 0, 0);
          dp[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(c[mt], d[nt], dp[mt][nt], 0, 0, 0);
        }
    }
    bias_mask_softmax(s, bt, tm, lane, p.shift > 0);
    // dS = P o (dP - rowsum(dP o P)); kept in dp
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float r = 0.f;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) r += dp[mt][nt][j] * s[mt][nt][j];
        r = group16_sum(r);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) dp[mt][nt][j] = s[mt][nt][j] * (dp[mt][nt][j] - r);
      }
    // relative-position-bias gradient into the wave's LDS table
    if (active) {
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int q = mt * 16 + lg * 4 + j;
          if (q < WT) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
              const int key = nt * 16 + lr;
              if (key < WT) atomicAdd(dbt + rel_index(q, key), dp[mt][nt][j]);
            }
          }
        }
    }
    // ---- dV = P^T dO
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int j = 0; j < 4; ++j) PS[(mt * 16 + lg * 4 + j) * LDP_F + nt * 16 + lr] = s[mt][nt][j];
    __syncthreads();
    {
      f32x4 acc[4][2];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) { acc[mt][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[mt][1] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll 4
      for (int kk = 0; kk < 16; ++kk) {
        float a[4], b[2];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) a[mt] = PS[(kk * 4 + lg) * LDP_F + mt * 16 + lr];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) b[nt] = Ds[(kk * 4 + lg) * LDQ_F + nt * 16 + lr];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
      }
      if (active) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int key = mt * 16 + lg * 4 + j;
            if (key < WT) {
              float* dst = p.dqkv + (size_t)tm.row(key) * ld + 2 * p.C + colq;
              dst[lr] = acc[mt][0][j]; dst[16 + lr] = acc[mt][1][j];
            }
          }
      }
    }
    __syncthreads();
    // ---- dQ = scale * dS K ; dK = dS^T (scale*Q)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int j = 0; j < 4; ++j) PS[(mt * 16 + lg * 4 + j) * LDP_F + nt * 16 + lr] = dp[mt][nt][j];
    __syncthreads();
    {
      f32x4 aq[4][2], ak[4][2];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        aq[mt][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; aq[mt][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
        ak[mt][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; ak[mt][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll 4
      for (int kk = 0; kk < 16; ++kk) {
        float a1[4], a2[4], b1[2], b2[2];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
          a1[mt] = PS[(mt * 16 + lr) * LDP_F + kk * 4 + lg];   // dS[q][key]
          a2[mt] = PS[(kk * 4 + lg) * LDP_F + mt * 16 + lr];   // dS^T[key][q]
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          b1[nt] = Ks[(kk * 4 + lg) * LDQ_F + nt * 16 + lr];
          b2[nt] = Qs[(kk * 4 + lg) * LDQ_F + nt * 16 + lr];
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) {
            aq[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[mt], b1[nt], aq[mt][nt], 0, 0, 0);
            ak[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[mt], b2[nt], ak[mt][nt], 0, 0, 0);
          }
      }
      if (active) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int t = mt * 16 + lg * 4 + j;
            if (t < WT) {
              float* dst = p.dqkv + (size_t)tm.row(t) * ld + colq;
              dst[lr] = aq[mt][0][j] * p.scale; dst[16 + lr] = aq[mt][1][j] * p.scale;
              dst[p.C + lr] = ak[mt][0][j]; dst[p.C + 16 + lr] = ak[mt][1][j];
            }
          }
      }
    }
  }
  __syncthreads();
  for (int i = lane; i < 169; i += 64) {
    const float v = dbt[i];
    if (v != 0.f) atomicAdd(p.dtable + i * p.heads + head, v);
  }
}

// bf16 backward: same algorithm, bf16 MFMA (16x16x32) with fp32 accumulate; the tiles stay row-major [token][32] /
// [q][key] in LDS and every fragment that needs 8 consecutive TOKENS per lane (P^T, dS^T, and the B operands K, Q, dO of
// dQ / dK / dV) is produced by ds_read_b64_tr_b16, so no transposed copies exist.  15.6 KB + 9.2 KB per wave -> 4 waves.
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4_a;

__device__ __forceinline__ bf16x8 tr_frag(const __bf16* tile, int ld, int row0, int col0, int lane) {
  // 8 consecutive rows (row0 + 8*(lane>>4) + j) of column (col0 + (lane&15)): two 4x16 transposing reads
  const int lr = lane & 15, lg = lane >> 4, q = lr >> 2, pp = lr & 3;
  const __bf16* src = tile + (row0 + lg * 8 + q) * ld + col0 + pp * 4;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_a*)(src));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_a*)(src + 4 * ld));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// the same fragment with the columns of a 32-wide head tile permuted: MFMA row lr <- column 8 (lr >> 2) + 4 nt + (lr & 3), so that the two
// 16-column blocks nt = 0, 1 of a transposed accumulator leave the 8 CONSECUTIVE columns 8 lg .. 8 lg + 7 of a row in one lane (16-byte stores)
__device__ __forceinline__ bf16x8 tr_frag_perm(const __bf16* tile, int ld, int row0, int nt, int lane) {
  const int lr = lane & 15, lg = lane >> 4;
  const __bf16* src = tile + (row0 + lg * 8 + (lr >> 2)) * ld + (lr & 3) * 8 + nt * 4;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_a*)(src));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_a*)(src + 4 * ld));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// ------------------------------------------------------------------------------------------------
// cross-view attention core.  qkv: [B*V*P, 3R] channels-last rows (img, pos), R = heads*hd reduced channels;
// feature of (view, head) = all (pos, c) with c in the head's hd channels -> F = P*hd (288).
// ------------------------------------------------------------------------------------------------
constexpr int CVA_MAXV = 32, CVA_MAXF = 288;

template <typename AT>
struct CvaArgsT { const AT* qkv; AT* out; const AT* dout; AT* dqkv; int B, V, P, R, heads, hd, fc; float scale; };

template <typename AT>
__device__ __forceinline__ size_t cva_off(const CvaArgsT<AT>& p, int b, int v, int f, int head, int which, int ld) {
  const int pos = f / p.hd, c = f - pos * p.hd;
  return ((size_t)(b * p.V + v) * p.P + pos) * ld + which * p.R + head * p.hd + c;
}

// Features are walked in chunks of FC = p.fc <= CVA_MAXF per view (whole positions; one chunk for the 3 x 3 grid of the default
// ATT_SPATIAL_DOWNSAMPLE_RATIO = 2, six for the 7 x 7 grid of ratio 1): the V x V scores accumulate over the chunks, the second sweep
// re-loads only when there was more than one chunk.
template <typename AT>
__global__ __launch_bounds__(256) void cva_attn_fwd_kernel(const CvaArgsT<AT> p) {
  __shared__ float q[CVA_MAXV * CVA_MAXF], k[CVA_MAXV * CVA_MAXF], v[CVA_MAXV * CVA_MAXF];
  __shared__ float a[CVA_MAXV * CVA_MAXV];
  const int b = blockIdx.x / p.heads, head = blockIdx.x % p.heads;
  const int F = p.P * p.hd, V = p.V, FC = p.fc;
  const bool single = F <= FC;
  for (int ij = threadIdx.x; ij < V * V; ij += 256) a[ij] = 0.f;
  for (int f0 = 0; f0 < F; f0 += FC) {
    const int fc = min(FC, F - f0);
    __syncthreads();
    for (int i = threadIdx.x; i < V * fc; i += 256) {
      const int vi = i / fc, f = i - vi * fc;
      q[i] = ldf(p.qkv + cva_off(p, b, vi, f0 + f, head, 0, 3 * p.R));
      k[i] = ldf(p.qkv + cva_off(p, b, vi, f0 + f, head, 1, 3 * p.R));
      if (single) v[i] = ldf(p.qkv + cva_off(p, b, vi, f0 + f, head, 2, 3 * p.R));
    }
    __syncthreads();
    for (int ij = threadIdx.x; ij < V * V; ij += 256) {
      const int i = ij / V, j = ij - i * V;
      float s = 0.f;
      for (int f = 0; f < fc; ++f) s += q[i * fc + f] * k[j * fc + f];
      a[ij] += s;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < V; i += 256) {
    float mx = -3.0e38f;
    for (int j = 0; j < V; ++j) { a[i * V + j] *= p.scale; mx = fmaxf(mx, a[i * V + j]); }
    float sum = 0.f;
    for (int j = 0; j < V; ++j) { const float e = expf(a[i * V + j] - mx); a[i * V + j] = e; sum += e; }
    const float inv = 1.f / sum;
    for (int j = 0; j < V; ++j) a[i * V + j] *= inv;
  }
  __syncthreads();
  for (int f0 = 0; f0 < F; f0 += FC) {
    const int fc = min(FC, F - f0);
    if (!single) {
      __syncthreads();
      for (int i = threadIdx.x; i < V * fc; i += 256) {
        const int vi = i / fc, f = i - vi * fc;
        v[i] = ldf(p.qkv + cva_off(p, b, vi, f0 + f, head, 2, 3 * p.R));
      }
      __syncthreads();
    }
    for (int i = threadIdx.x; i < V * fc; i += 256) {
      const int vi = i / fc, f = i - vi * fc;
      float o = 0.f;
      for (int j = 0; j < V; ++j) o += a[vi * V + j] * v[j * fc + f];
      stf(p.out + cva_off(p, b, vi, f0 + f, head, 0, p.R), o);
    }
  }
}

template <typename AT>
__global__ __launch_bounds__(256) void cva_attn_bwd_kernel(const CvaArgsT<AT> p) {
  __shared__ float q[CVA_MAXV * CVA_MAXF], k[CVA_MAXV * CVA_MAXF], v[CVA_MAXV * CVA_MAXF], d[CVA_MAXV * CVA_MAXF];
  __shared__ float a[CVA_MAXV * CVA_MAXV], ds[CVA_MAXV * CVA_MAXV];
  const int b = blockIdx.x / p.heads, head = blockIdx.x % p.heads;
  const int F = p.P * p.hd, V = p.V, FC = p.fc;
  const bool single = F <= FC;
  for (int ij = threadIdx.x; ij < V * V; ij += 256) { a[ij] = 0.f; ds[ij] = 0.f; }
  for (int f0 = 0; f0 < F; f0 += FC) {
    const int fc = min(FC, F - f0);
    __syncthreads();
    for (int i = threadIdx.x; i < V * fc; i += 256) {
      const int vi = i / fc, f = i - vi * fc;
      q[i] = ldf(p.qkv + cva_off(p, b, vi, f0 + f, head, 0, 3 * p.R));
      k[i] = ldf(p.qkv + cva_off(p, b, vi, f0 + f, head, 1, 3 * p.R));
      v[i] = ldf(p.qkv + cva_off(p, b, vi, f0 + f, head, 2, 3 * p.R));
      d[i] = ldf(p.dout + cva_off(p, b, vi, f0 + f, head, 0, p.R));
    }
    __syncthreads();
    for (int ij = threadIdx.x; ij < V * V; ij += 256) {
      const int i = ij / V, j = ij - i * V;
      float s = 0.f, da = 0.f;
      for (int f = 0; f < fc; ++f) { s += q[i * fc + f] * k[j * fc + f]; da += d[i * fc + f] * v[j * fc + f]; }
      a[ij] += s; ds[ij] += da;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < V; i += 256) {
    float mx = -3.0e38f;
    for (int j = 0; j < V; ++j) { a[i * V + j] *= p.scale; mx = fmaxf(mx, a[i * V + j]); }
    float sum = 0.f;
    for (int j = 0; j < V; ++j) { const float e = expf(a[i * V + j] - mx); a[i * V + j] = e; sum += e; }
    const float inv = 1.f / sum;
    float r = 0.f;
    for (int j = 0; j < V; ++j) { a[i * V + j] *= inv; r += a[i * V + j] * ds[i * V + j]; }
    for (int j = 0; j < V; ++j) ds[i * V + j] = a[i * V + j] * (ds[i * V + j] - r) * p.scale;
  }
  __syncthreads();
  for (int f0 = 0; f0 < F; f0 += FC) {
    const int fc = min(FC, F - f0);
    if (!single) {
      __syncthreads();
      for (int i = threadIdx.x; i < V * fc; i += 256) {
        const int vi = i / fc, f = i - vi * fc;
        q[i] = ldf(p.qkv + cva_off(p, b, vi, f0 + f, head, 0, 3 * p.R));
        k[i] = ldf(p.qkv + cva_off(p, b, vi, f0 + f, head, 1, 3 * p.R));
        d[i] = ldf(p.dout + cva_off(p, b, vi, f0 + f, head, 0, p.R));
      }
      __syncthreads();
    }
    for (int i = threadIdx.x; i < V * fc; i += 256) {
      const int vi = i / fc, f = i - vi * fc;
      float dq = 0.f, dk = 0.f, dv = 0.f;
      for (int j = 0; j < V; ++j) {
        dq += ds[vi * V + j] * k[j * fc + f];
        dk += ds[j * V + vi] * q[j * fc + f];
        dv += a[j * V + vi] * d[j * fc + f];
      }
      stf(p.dqkv + cva_off(p, b, vi, f0 + f, head, 0, 3 * p.R), dq);
      stf(p.dqkv + cva_off(p, b, vi, f0 + f, head, 1, 3 * p.R), dk);
      stf(p.dqkv + cva_off(p, b, vi, f0 + f, head, 2, 3 * p.R), dv);
    }
  }
}


// ------------------------------------------------------------------------------------------------
// Workgroup-per-window kernels (bf16 MFMA): the 4 waves of a workgroup split the 64 (49 used) query rows of ONE
// (window, head) task - 16 rows each - and the key rows of the transposed products.  Per-wave state is a 16 x 64 score
// strip (16 accumulator registers) instead of the whole 64 x 64 matrix, so 4-6 workgroups fit a CU (LDS 25 / 41 KB) and
// every SIMD holds 4+ waves to hide LDS / HBM latency (the wave-per-window kernels above run 1 wave per SIMD at 256 VGPRs
// and are kept for exact-fp32 MFMA).  A workgroup walks `tasks_per_wave` windows of one head; the relative-position-bias
// gradient is accumulated in REGISTERS across its windows (the (query, key) -> table index map is the same for all) and
// reaches LDS / HBM once per workgroup.
// ------------------------------------------------------------------------------------------------
// bias + mask + softmax over the keys for ONE 16-row strip (query rows mt*16 + lg*4 + j, keys nt*16 + lr).
// The relative-position bias of this lane's 16 (query, key) slots is the same for every window of a head: it is gathered
// once per workgroup into registers (strip_bias); the shifted-window mask only exists in the last window row / column.
__device__ __forceinline__ void strip_bias(float (&bias)[4][4], const float* bt, int lane, int mt) {
  const int lr = lane & 15, lg = lane >> 4;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int key = nt * 16 + lr;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = mt * 16 + lg * 4 + j;
      bias[nt][j] = key >= WT ? -1.0e30f : (q < WT ? bt[rel_index(q, key)] : 0.f);   // key padding: excluded
    }
  }
}
// The same registers in the QUERY-IN-LANE layout of the transposed score blocks S^T = K Q^T (keys as the first MFMA operand): lane -> query q
// (= 16 wave + lr), keys 16 nt + 4 lg + j.  mul: log2(e) where bt holds the plain table and the softmax runs in the exp2 domain.
__device__ __forceinline__ void lane_bias(float (&bias)[4][4], const float* bt, int q, int lg, float mul = 1.f) {
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int key = nt * 16 + lg * 4 + j;
      bias[nt][j] = key >= WT ? -1.0e30f : (q < WT ? bt[rel_index(q, key)] * mul : 0.f);   // key padding: excluded
    }
}
// seam mask of query q in that layout: bit (4 nt + j) is set where key 16 nt + 4 lg + j lies in another region of the rolled map (TokMap::region)
// than q.  Inside one window the regions split at token row 7 - shift of the last window row and at token column 7 - shift of the last window
// column, so the mask is two window-independent bit sets (key row / column below the split) picked by the window's position.
__device__ __forceinline__ unsigned seam_kdiff(const TokMap& tm, int q, int lg) {
  const int split = 7 - tm.shift, qy = q / 7, qx = q - qy * 7;
  unsigned ylow = 0, xlow = 0, valid = 0;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int key = nt * 16 + lg * 4 + j, ky = key / 7, kx = key - ky * 7;
      const unsigned bit = 1u << (nt * 4 + j);
      if (key < WT) valid |= bit;
      if (ky < split) ylow |= bit;
      if (kx < split) xlow |= bit;
    }
  unsigned kdiff = 0;
  if (tm.wy == tm.H / 7 - 1) kdiff |= qy < split ? ~ylow : ylow;
  if (tm.wx == tm.W / 7 - 1) kdiff |= qx < split ? ~xlow : xlow;
  return q < WT ? kdiff & valid : 0u;
}
struct FMax2 { __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); } };
struct FAdd2 { __device__ __forceinline__ float operator()(float a, float b) const { return a + b; } };
// LOG2: scores and bias arrive multiplied by log2(e) (the forward folds the factor into the scale of Q and into the bias strip), so the
// exponential is one v_exp_f32 without the multiply __expf carries
constexpr float ATTN_LOG2E = 1.4426950408889634f;
template <bool LOG2 = false>
__device__ __forceinline__ void bias_mask_softmax_strip(f32x4 (&s)[4], const float (&bias)[4][4], const TokMap& tm, int lane, bool masked, int mt) {
  const int lr = lane & 15, lg = lane >> 4;
  if (masked) {   // a window touching the rolled seam: tokens of different regions must not attend to each other
    int kreg[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) { const int key = nt * 16 + lr; kreg[nt] = key < WT ? tm.region(key) : 0; }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = mt * 16 + lg * 4 + j;
      const int qreg = q < WT ? tm.region(q) : 0;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        if (q < WT && nt * 16 + lr < WT && qreg != kreg[nt]) s[nt][j] += LOG2 ? -100.0f * ATTN_LOG2E : -100.0f;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float mx = -3.0e38f;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const float v = bias[nt][j] <= -1.0e29f ? -1.0e30f : s[nt][j] + bias[nt][j];
      s[nt][j] = v;
      mx = fmaxf(mx, v);
    }
    mx = group16_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) { const float e = LOG2 ? __builtin_amdgcn_exp2f(s[nt][j] - mx) : __expf(s[nt][j] - mx); s[nt][j] = e; sum += e; }
    const float inv = __builtin_amdgcn_rcpf(group16_sum(sum));   // 1 ulp: the quotient is rounded to bf16 right after (an IEEE division is ~10 instructions)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) s[nt][j] *= inv;
  }
}

// The QUERY-IN-LANE softmax of one query: s = smul * s + bias (smul: what the raw product still owes - 1, or log2(e) where the q tile carries
// the plain softmax scale), seam mask from seam_kdiff (`masked` is uniform over the window), then 16 in-lane values + two lane-group exchanges
// per reduction.  Returns 1 / sum; NORMALISE = false leaves the exponentials unnormalised for a caller that folds the factor into its bf16 pack.
template <bool LOG2, bool NORMALISE>
__device__ __forceinline__ float softmax_lane(f32x4 (&s)[4], const float (&bias)[4][4], float smul, bool masked, unsigned kdiff) {
  float mx = -3.0e38f;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float v = __builtin_fmaf(s[nt][j], smul, bias[nt][j]);   // key padding: bias = -1e30 under finite scores
      s[nt][j] = v;
      mx = fmaxf(mx, v);
    }
  if (masked) {
    mx = -3.0e38f;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (kdiff & (1u << (nt * 4 + j))) s[nt][j] += LOG2 ? -100.0f * ATTN_LOG2E : -100.0f;
        mx = fmaxf(mx, s[nt][j]);
      }
  }
  mx = lanegroup_allreduce(mx, FMax2());
  float sum = 0.f;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int j = 0; j < 4; ++j) { const float e = LOG2 ? __builtin_amdgcn_exp2f(s[nt][j] - mx) : __expf(s[nt][j] - mx); s[nt][j] = e; sum += e; }
  const float inv = __builtin_amdgcn_rcpf(lanegroup_allreduce(sum, FAdd2()));   // 1 ulp: the quotient is rounded to bf16 right after
  if (NORMALISE) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int j = 0; j < 4; ++j) s[nt][j] *= inv;
  }
  return inv;
}

// Relative-position-bias gradient of a workgroup (256 threads): dsum = the sum of dS over the workgroup's windows at each lane's 16 (query,
// key) slots of NH heads, in the STRIP or the query-in-lane layout -> dbt (LDS, [NH][176], zero so far) -> one atomic per non-zero table
// entry into dst[entry * heads + head0 + h] (a slot image of the table, or the table).  Call behind a barrier.
template <bool STRIP, int NH>
__device__ __forceinline__ void dbias_flush(const f32x4 (*dsum)[4], float* dbt, float* dst, int head0, int heads, int lane, int wave) {
  const int lr = lane & 15, lg = lane >> 4;
#pragma unroll
  for (int h = 0; h < NH; ++h)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int q = wave * 16 + (STRIP ? lg * 4 + j : lr), key = nt * 16 + (STRIP ? lr : lg * 4 + j);
        if (q < WT && key < WT) atomicAdd(dbt + h * 176 + rel_index(q, key), dsum[h][nt][j]);
      }
  __syncthreads();
  for (int i = threadIdx.x; i < NH * 169; i += 256) {
    const int h = NH == 1 ? 0 : i / 169, e = i - h * 169;
    const float v = dbt[h * 176 + e];
    if (v != 0.f) atomicAdd(dst + e * heads + head0 + h, v);
  }
}

// fp8 tile scales: m[n] = this thread's maximum of |x| over its piece of N tiles -> 224 / (the workgroup's maximum) (half of e4m3's 448: head
// room for the rounding; 1 for an all-zero tile).  The 4 waves meet in `am` (LDS).  SYNC_FIRST: `am` is single-buffered and may still be
// read for the previous window, so a barrier goes before the write as well.
template <int N, bool SYNC_FIRST>
__device__ __forceinline__ void wg_amax_scale(float (&m)[N], float (*am)[N], int lane, int wave) {
#pragma unroll
  for (int n = 0; n < N; ++n) m[n] = wave_max(m[n]);
  if (SYNC_FIRST) __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int n = 0; n < N; ++n) am[wave][n] = m[n];
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < N; ++n) m[n] = fmaxf(fmaxf(am[0][n], am[1][n]), fmaxf(am[2][n], am[3][n]));
#pragma unroll
  for (int n = 0; n < N; ++n) m[n] = m[n] > 0.f ? 224.f / m[n] : 1.f;
}
__device__ __forceinline__ float amax4(float m, const float4& v) { return fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)))); }

// (window chunk, head) of a workgroup in the 1-D grids of the workgroup-per-window kernels.  A head's slice of a token row is
// 64 bytes - half a cache line - so the `heads` workgroups that walk the same windows must meet in one L2: consecutive
// linear ids are spread round-robin over the 8 XCDs, ids l, l+8, l+16, ... therefore land on the SAME XCD back to back.
// Those carry the heads of one chunk; the row is fetched from HBM once and the other heads hit in that XCD's L2.
// Measured (I = 256): 8 % faster at 3 heads, 2-4 % at 6, and 4 % slower at 12+ heads (a token row is then >= 6 lines and
// the heads of a chunk crowd one XCD), so wide stages keep the head-major order.
__device__ __forceinline__ bool wg_chunk_head(int nchunks, int heads, int& chunk, int& head) {
  const int l = blockIdx.x;
  if (heads <= 6) {
    const int xcd = l & 7, slot = l >> 3;
    head = slot % heads;
    chunk = (slot / heads) * 8 + xcd;
  } else {
    const int n8 = (nchunks + 7) & ~7;
    head = l / n8;
    chunk = l - head * n8;
  }
  return chunk < nchunks;
}
// Windows per workgroup such that the whole grid is ONE resident wave (256 CUs x the kernel's workgroups per CU): every
// workgroup does the same work, so a partially filled second wave costs as much as a full one.
static inline int wg_tasks_per_block(int ntasks, int heads, int blocks_per_cu) {
  int nchunks = 256 * blocks_per_cu / heads;
  if (nchunks < 1) nchunks = 1;
  if (nchunks > ntasks) nchunks = ntasks;
  return (ntasks + nchunks - 1) / nchunks;
}
static inline unsigned wg_grid(int nchunks, int heads) { return 8u * (unsigned)heads * (unsigned)((nchunks + 7) / 8); }

// A thread's piece of a [64 tokens][32 channels] head tile in the cooperative (256-thread) loads: CV consecutive channels of one token row -
// 16 bytes of bf16 rows (one pass over the tile), 4 floats of fp32 rows (two passes)
template <typename AT> struct HeadChunk {
  static constexpr int CV = sizeof(AT) == 2 ? 8 : 4, TPRW = HD / CV, NIT = 64 * TPRW / 256;
  typedef typename VecN<AT, CV>::type RV;
  static __device__ __forceinline__ int row(int tid, int it) { return tid / TPRW + (256 / TPRW) * it; }
  static __device__ __forceinline__ int ch(int tid) { return (tid % TPRW) * CV; }
};
__device__ __forceinline__ void put_chunk(__bf16* dst, const float4& v, float mul) {
  bf16x4 b;
  b[0] = (__bf16)(v.x * mul); b[1] = (__bf16)(v.y * mul); b[2] = (__bf16)(v.z * mul); b[3] = (__bf16)(v.w * mul);
  *reinterpret_cast<bf16x4*>(dst) = b;
}
__device__ __forceinline__ void put_chunk(__bf16* dst, const bf16x8& v, float mul) {
  bf16x8 b;
#pragma unroll
  for (int j = 0; j < 8; ++j) b[j] = (__bf16)((float)v[j] * mul);
  *reinterpret_cast<bf16x8*>(dst) = b;
}

// ---- MX operand rows of the attention output (sv_window_attention_fwd_mxq): the producer side of linear_fp8.hip's MX recipe for att -> proj.
// One head of one token (32 channels) is exactly one MX block.  A lane holds 8 of the 32 channels of query lr as two groups of 4 consecutive
// channels (c0, c1: offsets inside the head); the block maximum of the STORED values (rounded to AT first) is a reduction over the four lg
// groups, lanes lr + 16 lg.  Each lane stores its 2 x 4 bytes, lg == 0 the E8M0 byte at [token][head].  For Kp > C the workgroup of the last
// head writes the zero bytes C .. Kp - 1 and the scale 127 of the padding blocks of its tokens: nothing relies on a pre-zeroed buffer.
// All lanes of a query (the four lg groups) must call it together.
template <typename AT> struct WinMxqArgsT : WinArgsT<AT> { uint8_t* q_out; uint8_t* qs_out; int Kp; };
template <typename AT, bool MXQ> struct WinFwdArgsOf { typedef WinArgsT<AT> type; };
template <typename AT> struct WinFwdArgsOf<AT, true> { typedef WinMxqArgsT<AT> type; };

template <typename AT>
__device__ __forceinline__ void mxq_emit(const WinMxqArgsT<AT>& p, long long row, int head, int lg, const float (&v)[8], int c0, int c1) {
  float t[8], am = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) { t[j] = (float)(AT)v[j]; am = fmaxf(am, fabsf(t[j])); }
  am = fmaxf(am, __shfl_xor(am, 16));
  am = fmaxf(am, __shfl_xor(am, 32));
  const int E = mx_block_exp(am);
  uint8_t* q = p.q_out + (size_t)row * p.Kp + head * HD;
  *reinterpret_cast<uint32_t*>(q + c0) = pack4_e4m3_mx(t[0], t[1], t[2], t[3], E);
  *reinterpret_cast<uint32_t*>(q + c1) = pack4_e4m3_mx(t[4], t[5], t[6], t[7], E);
  uint8_t* qs = p.qs_out + (size_t)row * (p.Kp >> 5);
  if (lg == 0) qs[head] = (uint8_t)(E + 127);
  if (head == p.heads - 1 && p.C + 32 * lg < p.Kp) {       // padding block lg of this token: 32 zero bytes, scale 1.0
    uint4* z = reinterpret_cast<uint4*>(p.q_out + (size_t)row * p.Kp + p.C + 32 * lg);
    z[0] = make_uint4(0u, 0u, 0u, 0u); z[1] = make_uint4(0u, 0u, 0u, 0u);
    qs[(p.C >> 5) + lg] = 127;
  }
}

template <typename AT, bool MXQ = false>
__global__ __launch_bounds__(256, 4) void win_attn_fwd_wg_kernel(const typename WinFwdArgsOf<AT, MXQ>::type p) {
  // q (scaled) | k | v of the window's head, row-major [token][32 (+8)] bf16.  The products are taken with swapped operands (keys / V^T as
  // the first MFMA operand): S^T = K Q^T leaves the 16 keys (16 nt + 4 lg + j) of query lr in one lane, so the softmax of a query is 16
  // in-lane values + two lane-group exchanges, and the probabilities go into P V from the registers they are in (the contraction index of
  // an MFMA may be permuted freely as long as both operands agree: the V^T fragment is fetched with ds_read_b64_tr_b16 from exactly those
  // key rows) - no P tile, no transposed V copy, one barrier less per window than the first version of this kernel.
  __shared__ __attribute__((aligned(16))) __bf16 Qs[64 * LDQ_H], Ks[64 * LDQ_H], Vs[64 * LDQ_H];
  __shared__ float bt[176];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  int chunk, head;
  if (!wg_chunk_head((p.ntasks + p.tasks_per_wave - 1) / p.tasks_per_wave, p.heads, chunk, head)) return;   // uniform over the workgroup
  const int nWx = p.W / 7, nW = (p.H / 7) * nWx;
  const int ld = 3 * p.C, colq = head * HD;
  for (int i = tid; i < 169; i += 256) bt[i] = p.table[i * p.heads + head] * ATTN_LOG2E;
  __syncthreads();
  const int q = wave * 16 + lr;                      // the query of this lane
  const bool qok = q < WT;
  float bias[4][4];                                  // relative-position bias of this lane's 16 (query, key) slots: the same for every window
  lane_bias(bias, bt, q, lg);
  const float qscale = p.scale * ATTN_LOG2E;      // scores come out of the MFMA in log2 units
  const long long task0 = (long long)chunk * p.tasks_per_wave;
  for (int tt = 0; tt < p.tasks_per_wave; ++tt) {
    const long long task = task0 + tt;
    if (task >= p.ntasks) break;                                         // uniform over the workgroup
    const TokMap tm = task_map(task, nW, nWx, p.H, p.W, p.shift);
    __syncthreads();                                                     // previous window's tiles are consumed
    typedef HeadChunk<AT> HC;
#pragma unroll
    for (int it = 0; it < HC::NIT; ++it) {
      const int r = HC::row(tid, it), ch = HC::ch(tid);
      typename HC::RV q4 = VecN<AT, HC::CV>::zero(), k4 = q4, v4 = q4;   // rows >= 49: zeros (finite values under zero probabilities)
      if (r < WT) {
        const AT* src = p.qkv + (size_t)tm.row(r) * ld + colq + ch;
        q4 = VecN<AT, HC::CV>::load(src); k4 = VecN<AT, HC::CV>::load(src + p.C); v4 = VecN<AT, HC::CV>::load(src + 2 * p.C);
      }
      put_chunk(Qs + r * LDQ_H + ch, q4, qscale);
      put_chunk(Ks + r * LDQ_H + ch, k4, 1.f);
      put_chunk(Vs + r * LDQ_H + ch, v4, 1.f);
    }
    __syncthreads();
    f32x4 s[4];
    {
      const bf16x8 qf = *reinterpret_cast<const bf16x8*>(Qs + q * LDQ_H + lg * 8);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + (nt * 16 + lr) * LDQ_H + lg * 8);
        s[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);   // lane: query lr, keys 16 nt + 4 lg + j
      }
    }
    const bool masked = tm.seam();
    const float inv = softmax_lane<true, false>(s, bias, 1.f, masked, masked ? seam_kdiff(tm, q, lg) : 0u);
    bf16x8 pf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int j = 0; j < 4; ++j) { pf[ks][j] = (__bf16)(s[2 * ks][j] * inv); pf[ks][4 + j] = (__bf16)(s[2 * ks + 1][j] * inv); }
    f32x4 o[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        // V^T fragment of block nt: MFMA row lr <- head channel 8 (lr >> 2) + 4 nt + (lr & 3) (the lanes with lr & 3 = c supply the 4-column
        // group that the lanes with lr >> 2 = c receive), keys 32 ks + 4 lg .. + 3 and 32 ks + 16 + 4 lg .. + 3: the order of the P fragment
        const __bf16* src = Vs + (2 * ks * 16 + lg * 4 + (lr >> 2)) * LDQ_H + (lr & 3) * 8 + nt * 4;
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_a*)(src));
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_a*)(src + 16 * LDQ_H));
        const bf16x8 vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        o[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[ks], o[nt], 0, 0, 0);
      }
    if (qok) {   // lane: query lr, head channels 8 lg .. 8 lg + 7 (block nt holds 8 lg + 4 nt + j): one 16-byte vector of bf16 rows
      const float ov[8] = {o[0][0], o[0][1], o[0][2], o[0][3], o[1][0], o[1][1], o[1][2], o[1][3]};
      if (!MXQ || p.out) stnf<8>(p.out + (size_t)tm.row(q) * p.C + colq + lg * 8, ov);
      if constexpr (MXQ) mxq_emit<AT>(p, tm.row(q), head, lg, ov, lg * 8, lg * 8 + 4);
    }
  }
}

// ---- fp8 (OCP e4m3) variant of the forward core: BASELINE configuration 5 ("fp8 MFMA QK/AV") -------------------------------------
// q (already times head_dim^-0.5), k, v and the softmax probabilities go to the matrix pipe as e4m3 (v_mfma_f32_16x16x32_fp8_fp8,
// fp32 accumulate).  Scales are per (window, head) TILE - finer than per tensor and free of an extra pass over HBM: the workgroup takes
// the absolute maximum of its q / k / v tile while the rows travel through registers and maps it to 224 (half of e4m3's 448, head room
// for the rounding); probabilities (<= 1) are scaled by 256, so that everything above 2^-17 survives as a subnormal.  Scores and
// outputs are rescaled in fp32; bias, mask and softmax stay fp32.  The backward of SV_MATH_FP8 keeps bf16 operands and recomputes P from
// bf16 q / k; SV_MATH_FP8_FULL differentiates this very function on e4m3 operands (win_attn_bwd_wg_fp8_kernel).
constexpr int LDQ_8 = 40;    // byte row stride of the fp8 q / k tiles (32 + 8: 8-byte fragment reads, rows 10 banks apart)
constexpr int LDP_8 = 72;    // byte row stride of the fp8 P and V^T tiles
__device__ __forceinline__ uint32_t pack4_fp8(float a, float b, float c, float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return (uint32_t)w;
}
__device__ __forceinline__ uint8_t one_fp8(float a) { return (uint8_t)(__builtin_amdgcn_cvt_pk_fp8_f32(a, 0.f, 0, false) & 0xff); }

template <typename AT, bool MXQ = false>
__global__ __launch_bounds__(256, 4) void win_attn_fwd_wg_fp8_kernel(const typename WinFwdArgsOf<AT, MXQ>::type p) {
  __shared__ __attribute__((aligned(16))) uint8_t Qs[64 * LDQ_8], Ks[64 * LDQ_8], Vt[HD * LDP_8], Ps[64 * LDP_8];
  __shared__ float bt[176];
  __shared__ float amax[4][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  int chunk, head;
  if (!wg_chunk_head((p.ntasks + p.tasks_per_wave - 1) / p.tasks_per_wave, p.heads, chunk, head)) return;   // uniform over the workgroup
  const int nWx = p.W / 7, nW = (p.H / 7) * nWx;
  const int ld = 3 * p.C, colq = head * HD;
  for (int i = tid; i < 169; i += 256) bt[i] = p.table[i * p.heads + head];
  for (int i = tid; i < HD * LDP_8; i += 256) Vt[i] = 0;               // key columns >= 49 stay zero
  __syncthreads();
  float bias[4][4];
  strip_bias(bias, bt, lane, wave);
  const long long task0 = (long long)chunk * p.tasks_per_wave;
  for (int tt = 0; tt < p.tasks_per_wave; ++tt) {
    const long long task = task0 + tt;
    if (task >= p.ntasks) break;                                         // uniform over the workgroup
    const TokMap tm = task_map(task, nW, nWx, p.H, p.W, p.shift);
    float4 q4[2], k4[2], v4[2];
    float sc[3] = {0.f, 0.f, 0.f};                                       // maxima, then scales, of the q' / k / v tile
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int r = (tid >> 3) + 32 * it, ch = (tid & 7) * 4;
      q4[it] = make_float4(0.f, 0.f, 0.f, 0.f); k4[it] = q4[it]; v4[it] = q4[it];
      if (r < WT) {
        const AT* src = p.qkv + (size_t)tm.row(r) * ld + colq + ch;
        q4[it] = ld4f(src); k4[it] = ld4f(src + p.C); v4[it] = ld4f(src + 2 * p.C);
      }
      q4[it].x *= p.scale; q4[it].y *= p.scale; q4[it].z *= p.scale; q4[it].w *= p.scale;
      sc[0] = amax4(sc[0], q4[it]); sc[1] = amax4(sc[1], k4[it]); sc[2] = amax4(sc[2], v4[it]);
    }
    wg_amax_scale<3, true>(sc, amax, lane, wave);                        // its first barrier: the previous window's tiles (and maxima) are consumed
    const float sq = sc[0], sk = sc[1], sv = sc[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int r = (tid >> 3) + 32 * it, ch = (tid & 7) * 4;
      *reinterpret_cast<uint32_t*>(Qs + r * LDQ_8 + ch) = pack4_fp8(q4[it].x * sq, q4[it].y * sq, q4[it].z * sq, q4[it].w * sq);
      *reinterpret_cast<uint32_t*>(Ks + r * LDQ_8 + ch) = pack4_fp8(k4[it].x * sk, k4[it].y * sk, k4[it].z * sk, k4[it].w * sk);
      if (r < WT) {
        const uint32_t w = pack4_fp8(v4[it].x * sv, v4[it].y * sv, v4[it].z * sv, v4[it].w * sv);
        Vt[(ch + 0) * LDP_8 + r] = (uint8_t)(w & 0xff); Vt[(ch + 1) * LDP_8 + r] = (uint8_t)((w >> 8) & 0xff);
        Vt[(ch + 2) * LDP_8 + r] = (uint8_t)((w >> 16) & 0xff); Vt[(ch + 3) * LDP_8 + r] = (uint8_t)(w >> 24);
      }
    }
    __syncthreads();
    f32x4 s[4];
    {
      const long a = *reinterpret_cast<const long*>(Qs + (wave * 16 + lr) * LDQ_8 + lg * 8);
      const float un = 1.f / (sq * sk);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const long b = *reinterpret_cast<const long*>(Ks + (nt * 16 + lr) * LDQ_8 + lg * 8);
        s[nt] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) s[nt][j] *= un;
      }
    }
    bias_mask_softmax_strip(s, bias, tm, lane, tm.seam(), wave);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int j = 0; j < 4; ++j) Ps[(wave * 16 + lg * 4 + j) * LDP_8 + nt * 16 + lr] = one_fp8(s[nt][j] * 256.f);
    __syncthreads();
    f32x4 o[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const long a = *reinterpret_cast<const long*>(Ps + (wave * 16 + lr) * LDP_8 + ks * 32 + lg * 8);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const long b = *reinterpret_cast<const long*>(Vt + (nt * 16 + lr) * LDP_8 + ks * 32 + lg * 8);
        o[nt] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(b, a, o[nt], 0, 0, 0);   // transposed block: O[q = lr][d = lg*4 + j]
      }
    }
    {
      const int q = wave * 16 + lr;
      const float un = 1.f / (256.f * sv);
      if (q < WT) {
        if (!MXQ || p.out) {
          AT* dst = p.out + (size_t)tm.row(q) * p.C + colq + lg * 4;
          st4f(dst, make_float4(o[0][0] * un, o[0][1] * un, o[0][2] * un, o[0][3] * un));
          st4f(dst + 16, make_float4(o[1][0] * un, o[1][1] * un, o[1][2] * un, o[1][3] * un));
        }
        if constexpr (MXQ) {   // the lane's channels: 4 lg .. + 3 and 16 + 4 lg .. + 3 of the head
          const float ov[8] = {o[0][0] * un, o[0][1] * un, o[0][2] * un, o[0][3] * un, o[1][0] * un, o[1][1] * un, o[1][2] * un, o[1][3] * un};
          mxq_emit<AT>(p, tm.row(q), head, lg, ov, lg * 4, 16 + lg * 4);
        }
      }
    }
  }
}

constexpr int ATTN_DT_SLOTS = 16;   // slot images of the relative-position-bias gradient (see sv_window_attention_bwd)

template <typename AT>
__global__ __launch_bounds__(256, 3) void win_attn_bwd_wg_kernel(const WinArgsT<AT> p, float* __restrict__ dt_ws) {
  __shared__ __attribute__((aligned(16))) __bf16 Qs[64 * LDQ_H], Ks[64 * LDQ_H], Vs[64 * LDQ_H], Ds[64 * LDQ_H];
  __shared__ __attribute__((aligned(16))) __bf16 Ps[64 * LDP_H], Ss[64 * LDP_H];   // P and dS, [query][key]
  __shared__ float bt[176], dbt[176];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  int chunk, head;
  if (!wg_chunk_head((p.ntasks + p.tasks_per_wave - 1) / p.tasks_per_wave, p.heads, chunk, head)) return;   // uniform over the workgroup
  const int nWx = p.W / 7, nW = (p.H / 7) * nWx;
  const int ld = 3 * p.C, colq = head * HD;
  for (int i = tid; i < 176; i += 256) { bt[i] = i < 169 ? p.table[i * p.heads + head] : 0.f; dbt[i] = 0.f; }
  __syncthreads();
  // Score blocks are taken transposed (keys as the first MFMA operand): lane -> query 16 wave + lr, keys 16 nt + 4 lg + j.  The softmax and
  // the row sum of dP o P of a query are then 16 in-lane values + two lane-group exchanges (the first version reduced every accumulator
  // row over 16 lanes), P and dS reach their LDS tiles as 8-byte row vectors instead of 2-byte scatters, and dQ = dS K takes dS from the
  // registers it is in (K^T fragments by ds_read_b64_tr_b16 in the key order of those registers, as the forward kernel does with V).
  const int qrow = wave * 16 + lr;
  const bool qrow_ok = qrow < WT;
  float bias[4][4];
  lane_bias(bias, bt, qrow, lg);
  f32x4 dsum[4];                                  // sum over this workgroup's windows of dS at this lane's (query, key) slots
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) dsum[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const long long task0 = (long long)chunk * p.tasks_per_wave;
  // the next window's q / k / v / dO vectors travel in registers while this window is contracted: a window is
  // load -> barrier -> MFMA -> softmax -> barrier -> MFMA -> store, and three workgroups per CU do not hide a global round trip
  typedef HeadChunk<AT> HC;
  typedef typename HC::RV RV;
  RV rq[HC::NIT], rk[HC::NIT], rv[HC::NIT], rd[HC::NIT];
  auto fetch = [&](long long task) {
    const TokMap tn = task_map(task, nW, nWx, p.H, p.W, p.shift);
#pragma unroll
    for (int it = 0; it < HC::NIT; ++it) {
      const int r = HC::row(tid, it), ch = HC::ch(tid);
      rq[it] = VecN<AT, HC::CV>::zero(); rk[it] = rq[it]; rv[it] = rq[it]; rd[it] = rq[it];
      if (r < WT) {
        const size_t row = tn.row(r);
        const AT* src = p.qkv + row * ld + colq + ch;
        rq[it] = VecN<AT, HC::CV>::load(src); rk[it] = VecN<AT, HC::CV>::load(src + p.C); rv[it] = VecN<AT, HC::CV>::load(src + 2 * p.C);
        rd[it] = VecN<AT, HC::CV>::load(p.dout + row * p.C + colq + ch);
      }
    }
  };
  auto put = [&](__bf16* dst, const RV& v, int it, float mul) { put_chunk(dst + HC::row(tid, it) * LDQ_H + HC::ch(tid), v, mul); };
  if (task0 < p.ntasks) fetch(task0);
  for (int tt = 0; tt < p.tasks_per_wave; ++tt) {
    const long long task = task0 + tt;
    if (task >= p.ntasks) break;
    const TokMap tm = task_map(task, nW, nWx, p.H, p.W, p.shift);
    __syncthreads();
#pragma unroll
    for (int it = 0; it < HC::NIT; ++it) { put(Qs, rq[it], it, p.scale); put(Ks, rk[it], it, 1.f); put(Vs, rv[it], it, 1.f); put(Ds, rd[it], it, 1.f); }
    __syncthreads();
    if (tt + 1 < p.tasks_per_wave && task + 1 < p.ntasks) fetch(task + 1);
    // ---- this wave's 16 queries: S^T = K (scale Q)^T, dP^T = V dO^T, P = softmax, dS = P o (dP - rowsum(dP o P))
    f32x4 s[4], dp[4];
    {
      const int off = qrow * LDQ_H + lg * 8;
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(Qs + off), c = *reinterpret_cast<const bf16x8*>(Ds + off);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int offb = (nt * 16 + lr) * LDQ_H + lg * 8;
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(Ks + offb), d = *reinterpret_cast<const bf16x8*>(Vs + offb);
        s[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, a, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        dp[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(d, c, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      }
    }
    const bool masked = tm.seam();
    softmax_lane<false, true>(s, bias, 1.f, masked, masked ? seam_kdiff(tm, qrow, lg) : 0u);
    {
      float r = 0.f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int j = 0; j < 4; ++j) r += dp[nt][j] * s[nt][j];
      r = lanegroup_allreduce(r, FAdd2());
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float dsv = s[nt][j] * (dp[nt][j] - r);
          dp[nt][j] = dsv;
          if (qrow_ok && nt * 16 + lg * 4 + j < WT) dsum[nt][j] += dsv;
        }
    }
    bf16x8 dsf[2];                                   // dS of this query as the second operand of dQ = dS K: keys 32 ks + 4 lg .. + 3, 32 ks + 16 + 4 lg .. + 3
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      bf16x4 pb, sb;
#pragma unroll
      for (int j = 0; j < 4; ++j) { pb[j] = (__bf16)s[nt][j]; sb[j] = (__bf16)dp[nt][j]; dsf[nt >> 1][(nt & 1) * 4 + j] = sb[j]; }
      *reinterpret_cast<bf16x4*>(Ps + qrow * LDP_H + nt * 16 + lg * 4) = pb;     // [query][key] rows: four consecutive keys per lane
      *reinterpret_cast<bf16x4*>(Ss + qrow * LDP_H + nt * 16 + lg * 4) = sb;
    }
    // ---- dQ = scale dS K for this wave's queries, from the registers: lane -> query lr, head channels 8 lg + 4 nt + j
    f32x4 aq[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const __bf16* src = Ks + (2 * ks * 16 + lg * 4 + (lr >> 2)) * LDQ_H + (lr & 3) * 8 + nt * 4;
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_a*)(src));
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_a*)(src + 16 * LDQ_H));
        const bf16x8 kT = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        aq[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kT, dsf[ks], aq[nt], 0, 0, 0);
      }
    if (qrow_ok) {
      const float qv[8] = {aq[0][0] * p.scale, aq[0][1] * p.scale, aq[0][2] * p.scale, aq[0][3] * p.scale,
                           aq[1][0] * p.scale, aq[1][1] * p.scale, aq[1][2] * p.scale, aq[1][3] * p.scale};
      stnf<8>(p.dqkv + (size_t)tm.row(qrow) * ld + colq + lg * 8, qv);
    }
    __syncthreads();
    // ---- this wave's 16 KEYS: dV = P^T dO and dK = dS^T (scale Q), contractions over all 64 queries of the tiles
    f32x4 av[2], ak[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) { av[nt] = (f32x4){0.f, 0.f, 0.f, 0.f}; ak[nt] = av[nt]; }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 pT = tr_frag(Ps, LDP_H, ks * 32, wave * 16, lane);        // A[key][q]
      const bf16x8 sT = tr_frag(Ss, LDP_H, ks * 32, wave * 16, lane);        // A[key][q]
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const bf16x8 bd = tr_frag_perm(Ds, LDQ_H, ks * 32, nt, lane);        // dO[q][d]
        const bf16x8 bq = tr_frag_perm(Qs, LDQ_H, ks * 32, nt, lane);        // (scale Q)[q][d]
        // operands swapped: the accumulators are the transposed blocks, X[row = lr][d = 8 lg + 4 nt + j] (16-byte stores below)
        av[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bd, pT, av[nt], 0, 0, 0);
        ak[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bq, sT, ak[nt], 0, 0, 0);
      }
    }
    {
      const int t = wave * 16 + lr;               // a key row
      if (t < WT) {
        AT* dst = p.dqkv + (size_t)tm.row(t) * ld + colq + lg * 8;
        const float kv[8] = {ak[0][0], ak[0][1], ak[0][2], ak[0][3], ak[1][0], ak[1][1], ak[1][2], ak[1][3]};
        const float vv[8] = {av[0][0], av[0][1], av[0][2], av[0][3], av[1][0], av[1][1], av[1][2], av[1][3]};
        stnf<8>(dst + p.C, kv);
        stnf<8>(dst + 2 * p.C, vv);
      }
    }
  }
  // ---- relative-position-bias gradient: registers -> LDS (once per workgroup) -> one atomic per table entry
  __syncthreads();
  dbias_flush<false, 1>(&dsum, dbt, dt_ws ? dt_ws + (size_t)(chunk % ATTN_DT_SLOTS) * 169 * p.heads : p.dtable, head, p.heads, lane, wave);
}
// ---- fp8 (OCP e4m3) backward of the window-attention core (SV_MATH_FP8_FULL) ----------------------------------------------------------
// The gradient of exactly the function win_attn_fwd_wg_fp8_kernel evaluates, every quantiser taken as the identity (straight-through).
// Per (window, head) tile: q' = scale q; sq, sk, sv, so = 224 / amax of q', k, v, dO (1 for an all-zero tile); Qq, Kq, Vq, dOq = e4m3 of
// the scaled tiles (pack4_fp8, the forward's conversions in the forward's order).  S = Qq Kq^T / (sq sk) (+ bias, + mask) and P = softmax(S)
// are recomputed exactly as the forward computes them (same MFMA operands and strip layout, bias_mask_softmax_strip), Pq = e4m3(256 P).
//   dV = Pq^T dOq / (256 so),  dP = dOq Vq^T / (so sv),  dS = P o (dP - rowsum(dP o P)) (fp32; the bias-table gradient sums this dS),
//   ss = 224 / amax(dS) over the tile (one scale: dK contracts over the queries), dSq = e4m3(ss dS),
//   dQ = scale dSq Kq / (ss sk),  dK = dSq^T Qq / (ss sq).
// All five contractions are v_mfma_f32_16x16x32_fp8_fp8.  Both operands of that MFMA take 8 consecutive bytes along the contraction
// index.  The q / k / v / dO tiles stay row-major [token][d] in LDS; the contractions over tokens (dQ, dK, dV) take them through
// ds_read_b64_tr_b8 (tr8_frag).  P and dS go to LDS as [key][query] (four consecutive queries of one key per lane: one 32-bit write); dK / dV
// read them as they are, dQ reads dS transposed.
// Phase 1: wave w owns queries 16 w .. 16 w + 15 (strip layout: lane -> queries 16 w + 4 lg + j, key 16 nt + lr).  Phase 2: wave w owns
// queries 16 w + lr for dQ and keys 16 w + lr for dK / dV; the transposed products leave 4 consecutive channels per lane (8 / 16-byte stores).
constexpr int LDT_8 = 72;    // byte row stride of the [key][query] fp8 tiles (64 + 8)
// a thread's piece of a window's q / k / v / dO head tiles: 4 channels (ch .. ch + 3) of rows r0 and r0 + 32, zeros for rows >= 49
template <typename AT>
__device__ __forceinline__ void fetch_rows(const WinArgsT<AT>& p, const TokMap& tn, int colq, int r0, int ch, float4 (&rq)[2], float4 (&rk)[2],
                                           float4 (&rv)[2], float4 (&rd)[2]) {
  const int ld = 3 * p.C;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int r = r0 + 32 * it;
    rq[it] = make_float4(0.f, 0.f, 0.f, 0.f); rk[it] = rq[it]; rv[it] = rq[it]; rd[it] = rq[it];
    if (r < WT) {
      const size_t row = tn.row(r);
      const AT* src = p.qkv + row * ld + colq + ch;
      rq[it] = ld4f(src); rk[it] = ld4f(src + p.C); rv[it] = ld4f(src + 2 * p.C);
      rd[it] = ld4f(p.dout + row * p.C + colq + ch);
    }
  }
}
// e4m3(s v) as 4 row-major bytes at [r][ch]
__device__ __forceinline__ void put_fp8(uint8_t* rowm, int r, int ch, const float4& v, float s) {
  *reinterpret_cast<uint32_t*>(rowm + r * LDQ_8 + ch) = pack4_fp8(v.x * s, v.y * s, v.z * s, v.w * s);
}
// fp8 MFMA operand along a tile's ROWS: lane -> column col0 + (lane & 15), rows row0 + 8 (lane >> 4) + j (j = 0..7, one byte each).
// ds_read_b64_tr_b8 transposes an 8 x 16-byte block among 16 lanes: lanes 2 j and 2 j + 1 fetch the two 8-byte halves of row j, lane i
// receives column i.
typedef int i32x2_tr __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) i32x2_tr lds_i32x2_a;
__device__ __forceinline__ long tr8_frag(const uint8_t* tile, int ld, int row0, int col0, int lane) {
  const int lr = lane & 15, lg = lane >> 4;
  const uint8_t* src = tile + (row0 + lg * 8 + (lr >> 1)) * ld + col0 + (lr & 1) * 8;
  return __builtin_bit_cast(long, __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2_a*)(src)));
}
template <typename AT>
__global__ __launch_bounds__(256, 3) void win_attn_bwd_wg_fp8_kernel(const WinArgsT<AT> p, float* __restrict__ dt_ws) {
  __shared__ __attribute__((aligned(16))) uint8_t Qs[64 * LDQ_8], Ks[64 * LDQ_8], Vs[64 * LDQ_8], Ds[64 * LDQ_8];   // [token][d]
  __shared__ __attribute__((aligned(16))) uint8_t Pt[64 * LDT_8], St[64 * LDT_8];                                   // Pq, dSq [key][q]
  __shared__ float bt[176], dbt[176];
  __shared__ float amax[2][4][4], amaxs[4][1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  int chunk, head;
  if (!wg_chunk_head((p.ntasks + p.tasks_per_wave - 1) / p.tasks_per_wave, p.heads, chunk, head)) return;   // uniform over the workgroup
  const int nWx = p.W / 7, nW = (p.H / 7) * nWx;
  const int ld = 3 * p.C, colq = head * HD;
  for (int i = tid; i < 176; i += 256) { bt[i] = i < 169 ? p.table[i * p.heads + head] : 0.f; dbt[i] = 0.f; }
  __syncthreads();
  float bias[4][4];
  strip_bias(bias, bt, lane, wave);
  f32x4 dsum[4];                                  // sum over this workgroup's windows of dS at this lane's (query, key) slots
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) dsum[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // the next window's rows travel in registers while this window is contracted
  const int r0 = tid >> 3, ch = (tid & 7) * 4;
  float4 rq[2], rk[2], rv[2], rd[2];
  const long long task0 = (long long)chunk * p.tasks_per_wave;
  if (task0 < p.ntasks) fetch_rows(p, task_map(task0, nW, nWx, p.H, p.W, p.shift), colq, r0, ch, rq, rk, rv, rd);
  for (int tt = 0; tt < p.tasks_per_wave; ++tt) {
    const long long task = task0 + tt;
    if (task >= p.ntasks) break;                                         // uniform over the workgroup
    const TokMap tm = task_map(task, nW, nWx, p.H, p.W, p.shift);
    // ---- per-tile scales: q' = scale q first (the forward's order), then the workgroup maximum of |q'|, |k|, |v|, |dO|
    float sc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      rq[it].x *= p.scale; rq[it].y *= p.scale; rq[it].z *= p.scale; rq[it].w *= p.scale;
      sc[0] = amax4(sc[0], rq[it]); sc[1] = amax4(sc[1], rk[it]); sc[2] = amax4(sc[2], rv[it]); sc[3] = amax4(sc[3], rd[it]);
    }
    // double-buffered maxima: no barrier between two windows' maxima; the helper's barrier also ends the reads of the previous window's tiles
    wg_amax_scale<4, false>(sc, amax[tt & 1], lane, wave);
    const float sq = sc[0], sk = sc[1], sv = sc[2], so = sc[3];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int r = r0 + 32 * it;                                        // rows >= 49 hold zeros (registers were zeroed)
      put_fp8(Qs, r, ch, rq[it], sq); put_fp8(Ks, r, ch, rk[it], sk); put_fp8(Vs, r, ch, rv[it], sv); put_fp8(Ds, r, ch, rd[it], so);
    }
    __syncthreads();
    if (tt + 1 < p.tasks_per_wave && task + 1 < p.ntasks)
      fetch_rows(p, task_map(task + 1, nW, nWx, p.H, p.W, p.shift), colq, r0, ch, rq, rk, rv, rd);
    // ---- phase 1, this wave's 16 queries: S and dP in the forward's strip layout (element (q = 16 wave + 4 lg + j, key = 16 nt + lr))
    f32x4 s[4], dp[4];
    {
      const int off = (wave * 16 + lr) * LDQ_8 + lg * 8;
      const long a = *reinterpret_cast<const long*>(Qs + off), c = *reinterpret_cast<const long*>(Ds + off);
      const float un = 1.f / (sq * sk), unp = 1.f / (so * sv);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int offb = (nt * 16 + lr) * LDQ_8 + lg * 8;
        const long b = *reinterpret_cast<const long*>(Ks + offb), d = *reinterpret_cast<const long*>(Vs + offb);
        s[nt] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        dp[nt] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(c, d, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) { s[nt][j] *= un; dp[nt][j] *= unp; }
      }
    }
    bias_mask_softmax_strip(s, bias, tm, lane, tm.seam(), wave);
    float ms = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = wave * 16 + lg * 4 + j;
      float r = 0.f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) r += dp[nt][j] * s[nt][j];
      r = group16_sum(r);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const float dsv = s[nt][j] * (dp[nt][j] - r);
        dp[nt][j] = dsv;
        ms = fmaxf(ms, fabsf(dsv));
        if (q < WT && nt * 16 + lr < WT) dsum[nt][j] += dsv;
      }
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)     // Pq as [key][query]: the four queries of this lane are consecutive
      *reinterpret_cast<uint32_t*>(Pt + (nt * 16 + lr) * LDT_8 + wave * 16 + lg * 4) =
          pack4_fp8(s[nt][0] * 256.f, s[nt][1] * 256.f, s[nt][2] * 256.f, s[nt][3] * 256.f);
    float ssc[1] = {ms};
    wg_amax_scale<1, false>(ssc, amaxs, lane, wave);   // amaxs was last read before this window's two barriers
    const float ss = ssc[0];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
      *reinterpret_cast<uint32_t*>(St + (nt * 16 + lr) * LDT_8 + wave * 16 + lg * 4) =
          pack4_fp8(dp[nt][0] * ss, dp[nt][1] * ss, dp[nt][2] * ss, dp[nt][3] * ss);
    __syncthreads();
    // ---- phase 2: transposed products X^T[d = 16 nt + 4 lg + j][token = 16 wave + lr], contraction over 64 keys (dQ) or queries (dK, dV)
    f32x4 aq[2], ak[2], av[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) { aq[nt] = (f32x4){0.f, 0.f, 0.f, 0.f}; ak[nt] = aq[nt]; av[nt] = aq[nt]; }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int off = (wave * 16 + lr) * LDT_8 + ks * 32 + lg * 8;
      const long bs = tr8_frag(St, LDT_8, ks * 32, wave * 16, lane);    // dSq[q = 16 wave + lr][keys 32 ks + 8 lg ..]
      const long bst = *reinterpret_cast<const long*>(St + off);         // dSq[queries 32 ks + 8 lg ..][key = 16 wave + lr]
      const long bpt = *reinterpret_cast<const long*>(Pt + off);         // Pq [queries ..][key]
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {                                   // K^T, Q^T, dO^T fragments: [d = 16 nt + lr][tokens 32 ks + 8 lg ..]
        aq[nt] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(tr8_frag(Ks, LDQ_8, ks * 32, nt * 16, lane), bs, aq[nt], 0, 0, 0);
        ak[nt] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(tr8_frag(Qs, LDQ_8, ks * 32, nt * 16, lane), bst, ak[nt], 0, 0, 0);
        av[nt] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(tr8_frag(Ds, LDQ_8, ks * 32, nt * 16, lane), bpt, av[nt], 0, 0, 0);
      }
    }
    {
      const int t = wave * 16 + lr;                // the query of dQ and the key of dK / dV
      if (t < WT) {
        const float uq = p.scale / (ss * sk), uk = 1.f / (ss * sq), uv = 1.f / (256.f * so);
        AT* dst = p.dqkv + (size_t)tm.row(t) * ld + colq + lg * 4;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          st4f(dst + nt * 16, make_float4(aq[nt][0] * uq, aq[nt][1] * uq, aq[nt][2] * uq, aq[nt][3] * uq));
          st4f(dst + p.C + nt * 16, make_float4(ak[nt][0] * uk, ak[nt][1] * uk, ak[nt][2] * uk, ak[nt][3] * uk));
          st4f(dst + 2 * p.C + nt * 16, make_float4(av[nt][0] * uv, av[nt][1] * uv, av[nt][2] * uv, av[nt][3] * uv));
        }
      }
    }
  }
  // ---- relative-position-bias gradient: registers -> LDS (once per workgroup) -> slot image or table (as win_attn_bwd_wg_kernel)
  __syncthreads();
  dbias_flush<true, 1>(&dsum, dbt, dt_ws ? dt_ws + (size_t)(chunk % ATTN_DT_SLOTS) * 169 * p.heads : p.dtable, head, p.heads, lane, wave);
}

__global__ __launch_bounds__(256) void attn_dtable_fold_kernel(const float* __restrict__ ws, float* __restrict__ dtable, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float a = 0.f;
#pragma unroll
  for (int sl = 0; sl < ATTN_DT_SLOTS; ++sl) a += ws[(size_t)sl * n + i];
  dtable[i] += a;
}


// ---- fused attention branch of a stage-0 Swin block (C = 96, 3 heads) ----------------------------------------------------------------
// x1 = x + s * proj(window_attention(qkv(LayerNorm(x)))) in ONE kernel (timm SwinTransformerBlock behind models/swin_transformer.py:78:
// norm1 -> roll / partition -> qkv -> per-head softmax(q k^T * scale + bias (+ mask)) v -> proj -> reverse / roll -> drop-path -> + x).
// At C = 96 both weight matrices fit LDS as bf16 (288 x 96 + 96 x 96 = 72 KB), so a workgroup stages them once and then walks windows:
// 8 waves = 2 windows in flight, the 4 waves of a window own 16 token rows each (49 tokens padded to 64).
//  * LayerNorm runs on the MFMA operand layout itself: a lane loads the 16-byte chunks (token lr, channels 32 ks + 8 lg ..) that ARE its
//    fragment of the qkv GEMM, the row sums cross the four lane groups with two shuffles - the normalised rows never touch LDS.
//  * every product is taken with the operands swapped (weights / keys / V^T as the first MFMA operand), so the accumulator of a lane is
//    4 consecutive channels (or keys) of ONE token: q | k | v go to the LDS tile and to HBM as 8-byte vectors, and the softmax of a query
//    is 16 in-lane values + two shuffles across the lane groups instead of 16-lane reductions per accumulator row.
//  * the probabilities never leave registers: S^T = K Q^T leaves keys (16 nt + 4 lg + j) in the lane that, as the second operand of
//    P V, must supply 8 keys per K step - the contraction index of an MFMA may be permuted freely as long as both operands agree, so the
//    V^T fragment is fetched with ds_read_b64_tr_b16 from exactly those key rows (two 4-row blocks of the row-major V tile).
//  * the head outputs overwrite the (wave-private) q columns of the tile and become the operand of the projection; the residual, the
//    projection bias and the per-image drop-path factor are applied on the accumulators.
// Training needs the intermediate tensors of the unfused chain for its backward (LayerNorm output + statistics, qkv, attention output):
// they are written as side outputs when their pointers are given, bit-identical to what the unfused kernels store (q is rounded to bf16
// before the softmax scale is applied, as the core kernel does with the q it reads back), 7 instead of 13 passes over the token map;
// without them (inference) the kernel reads x and writes x1.  Two barriers per window; the next window's rows are prefetched into
// registers before the attention phase.
constexpr int FB_C = 96, FB_HEADS = 3;
constexpr int FB_LDT = 296;   // bf16 row stride of the q | k | v tile: 592 bytes = 37 x 16, odd -> 16-byte fragment reads of 16 rows spread over all bank groups
constexpr int FB_LDW = 104;   // bf16 row stride of the weight images: 208 bytes = 13 x 16
struct BlockFwdArgs {
  const __bf16* x; const float *ln_g, *ln_b, *wqkv, *bqkv, *table, *wproj, *bproj, *row_scale;
  __bf16 *x1, *ln1, *qkv, *att; float *mean, *rstd;
  int I, H, W, shift; float eps, scale; int ntasks, tasks_per_group;
};
constexpr int FB_SMEM = (288 + 96) * FB_LDW * 2 + 2 * 64 * FB_LDT * 2 + (3 * 176 + 288 + 3 * 96) * 4;

// The three sections of swin_attn_block_fwd_kernel that its MXFP8 sibling (swin_attn_block_fwd_mx_kernel) runs expression for expression, on a lane
// that holds token q = 16 wave + lr and, of a 32-column chunk ck, the 8 consecutive columns n0 = 32 ck + 8 lg .. + 7 in the two accumulator blocks
// acc[0] | acc[1].  The bf16 kernel keeps its own text: calling these from it moves its register allocation (182 -> 178 VGPRs) and the kernel of the
// default step is pinned, resource row included; a change to either copy belongs in both.
// qkv chunk ck: + bias, bf16 rounding, side output, the softmax scale on the bf16 q, the window tile
__device__ __forceinline__ void fb_put_qkv(const f32x4 (&acc)[2], int ck, const float* bq, __bf16* T, int q, int lg, float qscale, bool store, __bf16* qkv, size_t row) {
  const int n0 = ck * 32 + lg * 8;
  const float4 b0 = *reinterpret_cast<const float4*>(bq + n0), b1 = *reinterpret_cast<const float4*>(bq + n0 + 4);
  bf16x8 o;
  o[0] = (__bf16)(acc[0][0] + b0.x); o[1] = (__bf16)(acc[0][1] + b0.y); o[2] = (__bf16)(acc[0][2] + b0.z); o[3] = (__bf16)(acc[0][3] + b0.w);
  o[4] = (__bf16)(acc[1][0] + b1.x); o[5] = (__bf16)(acc[1][1] + b1.y); o[6] = (__bf16)(acc[1][2] + b1.z); o[7] = (__bf16)(acc[1][3] + b1.w);
  if (store) *reinterpret_cast<bf16x8*>(qkv + row * (3 * FB_C) + n0) = o;
  if (ck < 3) {   // q: the softmax scale (and log2 e) goes onto the bf16 value, as the core kernel applies it to the q it reads from HBM
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (__bf16)((float)o[e] * qscale);
  }
  *reinterpret_cast<bf16x8*>(T + q * FB_LDT + n0) = o;
}
// attention of one window on its tile, one head at a time; lane -> query lr, keys nt*16 + lg*4 + j.  The head outputs overwrite the q columns.
__device__ __forceinline__ void fb_attention(__bf16* T, const float (&bias)[FB_HEADS][4][4], const TokMap& tm, int q, int lr, int lg, bool store,
                                             __bf16* att, size_t row) {
  const bool masked = tm.seam();                                       // uniform over the window
  const unsigned kdiff = masked ? seam_kdiff(tm, q, lg) : 0u;
#pragma unroll
  for (int h = 0; h < FB_HEADS; ++h) {
    f32x4 s[4];
    {
      const bf16x8 qf = *reinterpret_cast<const bf16x8*>(T + q * FB_LDT + h * HD + lg * 8);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(T + (nt * 16 + lr) * FB_LDT + FB_C + h * HD + lg * 8);
        s[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      }
    }
    // key padding: bias = -1e30 and the padded K rows are finite (LayerNorm of a zero row = beta)
    const float inv = softmax_lane<true, false>(s, bias[h], 1.f, masked, kdiff);
    bf16x8 pf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int j = 0; j < 4; ++j) { pf[ks][j] = (__bf16)(s[2 * ks][j] * inv); pf[ks][4 + j] = (__bf16)(s[2 * ks + 1][j] * inv); }
    f32x4 o[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        // V^T fragment of block nt: MFMA row lr <- head channel 8 (lr >> 2) + 4 nt + (lr & 3) (the chunk permutation of the weight rows: the
        // lanes with lr & 3 = c supply the 4-column group that the lanes with lr >> 2 = c receive), the 8 keys of this lane group in the order
        // the P fragment holds them: keys 32 ks + 4 lg .. + 3 and 32 ks + 16 + 4 lg .. + 3
        const __bf16* src = T + (2 * ks * 16 + lg * 4 + (lr >> 2)) * FB_LDT + 2 * FB_C + h * HD + (lr & 3) * 8 + nt * 4;
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_a*)(src));
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_a*)(src + 16 * FB_LDT));
        const bf16x8 vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        o[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[ks], o[nt], 0, 0, 0);
      }
    bf16x8 ob;                                                         // lane -> query lr, head channels 8 lg .. 8 lg + 7
#pragma unroll
    for (int j = 0; j < 4; ++j) { ob[j] = (__bf16)o[0][j]; ob[4 + j] = (__bf16)o[1][j]; }
    if (store) *reinterpret_cast<bf16x8*>(att + row * FB_C + h * HD + lg * 8) = ob;
    *reinterpret_cast<bf16x8*>(T + q * FB_LDT + h * HD + lg * 8) = ob;   // over this wave's own q rows
  }
}
// x1 chunk ck = x + s * (acc + bp)
__device__ __forceinline__ void fb_put_x1(const f32x4 (&acc)[2], int ck, const float* bp, int lg, float sc, const bf16x8& xr, __bf16* x1_row) {
  const int n0 = ck * 32 + lg * 8;
  const float4 b0 = *reinterpret_cast<const float4*>(bp + n0), b1 = *reinterpret_cast<const float4*>(bp + n0 + 4);
  const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
  bf16x8 y;
#pragma unroll
  for (int e = 0; e < 8; ++e) y[e] = (__bf16)((float)xr[e] + sc * (acc[e >> 2][e & 3] + bb[e]));
  *reinterpret_cast<bf16x8*>(x1_row + n0) = y;
}

__global__ __launch_bounds__(512, 1) void swin_attn_block_fwd_kernel(const BlockFwdArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned char fb_smem[FB_SMEM];
  __bf16* Wq = reinterpret_cast<__bf16*>(fb_smem);          // [288][FB_LDW]  qkv.weight rows (out, in), rows permuted inside 32-row chunks (below)
  __bf16* Wp = Wq + 288 * FB_LDW;                            // [96][FB_LDW]   proj.weight rows, same permutation
  __bf16* Tb = Wp + 96 * FB_LDW;                             // 2 x [64][FB_LDT]  q (-> O) | k | v of the two windows in flight
  float* bt = reinterpret_cast<float*>(Tb + 2 * 64 * FB_LDT);   // [3][176] relative-position bias table per head, times log2 e
  float* bq = bt + 3 * 176;                                  // [288] qkv bias
  float* bp = bq + 288;                                      // [96] proj bias
  float* lng = bp + 96;                                      // [96] norm1 weight
  float* lnb = lng + 96;                                     // [96] norm1 bias
  const int tid = threadIdx.x, lane = tid & 63, wave = (tid >> 6) & 3, grp = tid >> 8;
  const int lr = lane & 15, lg = lane >> 4;
  // A transposed 16 x 16 accumulator block leaves MFMA row i = 4 lg + j in register j of lane group lg.  Feeding the weight rows of a
  // 32-column chunk in the order  block `half`, MFMA row i  <-  output column 8 (i >> 2) + 4 half + (i & 3)  makes the two blocks of a
  // chunk hold the 8 CONSECUTIVE columns 8 lg .. 8 lg + 7 of a token in one lane: every global access of the kernel is a 16-byte vector
  // in the layout of the LayerNorm loads (4 lanes = 64 contiguous bytes of a token row).  The permutation is applied once, here.
  for (int i = tid; i < (288 + 96) * 24; i += 512) {
    const int R = i / 24, c4 = (i - R * 24) * 4;            // LDS row R = 32 chunk + 16 half + i
    const int ii = R & 15, n = (R & ~31) + 8 * (ii >> 2) + 4 * ((R >> 4) & 1) + (ii & 3);
    const float4 w = ld4f(R < 288 ? p.wqkv + n * FB_C + c4 : p.wproj + (n - 288) * FB_C + c4);
    bf16x4 b; b[0] = (__bf16)w.x; b[1] = (__bf16)w.y; b[2] = (__bf16)w.z; b[3] = (__bf16)w.w;
    *reinterpret_cast<bf16x4*>(Wq + R * FB_LDW + c4) = b;    // Wp follows Wq
  }
  for (int i = tid; i < 3 * 169; i += 512) { const int h = i / 169, e = i - h * 169; bt[h * 176 + e] = p.table[e * FB_HEADS + h] * ATTN_LOG2E; }
  for (int i = tid; i < 288; i += 512) bq[i] = p.bqkv[i];
  if (tid < 96) { bp[tid] = p.bproj[tid]; lng[tid] = p.ln_g[tid]; lnb[tid] = p.ln_b[tid]; }
  __syncthreads();

  const int q = wave * 16 + lr;                      // the token (query) of this lane in every transposed accumulator
  const bool qok = q < WT;
  // relative-position bias of this lane's 16 (query, key) slots per head: the same for every window
  float bias[FB_HEADS][4][4];
#pragma unroll
  for (int h = 0; h < FB_HEADS; ++h) lane_bias(bias[h], bt + h * 176, q, lg);
  __bf16* T = Tb + grp * 64 * FB_LDT;
  const int nWx = p.W / 7, nW = (p.H / 7) * nWx;
  const long long task0 = ((long long)blockIdx.x * 2 + grp) * p.tasks_per_group;
  const float qscale = p.scale * ATTN_LOG2E;
  const bf16x8 zero8 = {(__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f};

  // the windows of a group are consecutive: (image, window row, window column) advance by increments, one division at the start
  TokMap tnext = task_map(task0 < p.ntasks ? task0 : 0, nW, nWx, p.H, p.W, p.shift);
  const int qty = (qok ? q : 0) / 7, qtx = (qok ? q : 0) - qty * 7;       // this lane's token inside the window
  auto token_row = [&](const TokMap& t) -> size_t {
    int ys = t.wy * 7 + qty + t.shift; if (ys >= t.H) ys -= t.H;
    int xs = t.wx * 7 + qtx + t.shift; if (xs >= t.W) xs -= t.W;
    return ((size_t)t.img * t.H + ys) * t.W + xs;
  };
  bf16x8 xn[3] = {zero8, zero8, zero8};              // prefetched rows of the NEXT window
  auto fetch = [&](bool in_range) {                   // this lane's three 16-byte chunks of its token row of window `tnext`
    xn[0] = zero8; xn[1] = zero8; xn[2] = zero8;
    if (in_range && qok) {
      const __bf16* src = p.x + token_row(tnext) * FB_C + lg * 8;
      xn[0] = *reinterpret_cast<const bf16x8*>(src); xn[1] = *reinterpret_cast<const bf16x8*>(src + 32); xn[2] = *reinterpret_cast<const bf16x8*>(src + 64);
    }
  };
  fetch(task0 < p.ntasks);
  for (int tt = 0; tt < p.tasks_per_group; ++tt) {
    const long long task = task0 + tt;
    const bool live = task < p.ntasks;                                   // uniform over the 4 waves of a window
    const TokMap tm = tnext;
    const bool valid = live && qok;
    const size_t row = token_row(tm);
    const bf16x8 xr[3] = {xn[0], xn[1], xn[2]};                          // kept for the residual: the projection's columns come out in this layout
    if (++tnext.wx == nWx) { tnext.wx = 0; if (++tnext.wy == p.H / 7) { tnext.wy = 0; ++tnext.img; } }
    fetch(tt + 1 < p.tasks_per_group && task + 1 < p.ntasks);           // issued before any store of this window, lands during its GEMMs
    // ---- LayerNorm of the wave's 16 rows, on the operand layout
    bf16x8 xf[3];
    {
      float xv[3][8];
      float s = 0.f;
#pragma unroll
      for (int ks = 0; ks < 3; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) { xv[ks][e] = (float)xr[ks][e]; s += xv[ks][e]; }
      const float mean = lanegroup_allreduce(s, FAdd2()) * (1.f / FB_C);
      float v2 = 0.f;
#pragma unroll
      for (int ks = 0; ks < 3; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float a = xv[ks][e] - mean; v2 += a * a; }
      const float rstd = rsqrtf(lanegroup_allreduce(v2, FAdd2()) * (1.f / FB_C) + p.eps);
#pragma unroll
      for (int ks = 0; ks < 3; ++ks) {
        const float4 g0 = *reinterpret_cast<const float4*>(lng + ks * 32 + lg * 8), g1 = *reinterpret_cast<const float4*>(lng + ks * 32 + lg * 8 + 4);
        const float4 b0 = *reinterpret_cast<const float4*>(lnb + ks * 32 + lg * 8), b1 = *reinterpret_cast<const float4*>(lnb + ks * 32 + lg * 8 + 4);
        const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w}, b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) xf[ks][e] = (__bf16)((xv[ks][e] - mean) * rstd * g[e] + b[e]);
      }
      if (valid && p.ln1) {
        __bf16* dst = p.ln1 + row * FB_C + lg * 8;
        *reinterpret_cast<bf16x8*>(dst) = xf[0]; *reinterpret_cast<bf16x8*>(dst + 32) = xf[1]; *reinterpret_cast<bf16x8*>(dst + 64) = xf[2];
        if (lg == 0) { p.mean[row] = mean; p.rstd[row] = rstd; }
      }
    }
    // ---- qkv = LN(x) W^T + b, one 32-column chunk (= one head of q, k or v) at a time: lane -> token lr, columns 32 ck + 8 lg .. + 7
#pragma unroll 3
    for (int ck = 0; ck < 9; ++ck) {
      f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int ks = 0; ks < 3; ++ks)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(Wq + (ck * 32 + hf * 16 + lr) * FB_LDW + ks * 32 + lg * 8);
          acc[hf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, xf[ks], acc[hf], 0, 0, 0);
        }
      const int n0 = ck * 32 + lg * 8;
      const float4 b0 = *reinterpret_cast<const float4*>(bq + n0), b1 = *reinterpret_cast<const float4*>(bq + n0 + 4);
      bf16x8 o;
      o[0] = (__bf16)(acc[0][0] + b0.x); o[1] = (__bf16)(acc[0][1] + b0.y); o[2] = (__bf16)(acc[0][2] + b0.z); o[3] = (__bf16)(acc[0][3] + b0.w);
      o[4] = (__bf16)(acc[1][0] + b1.x); o[5] = (__bf16)(acc[1][1] + b1.y); o[6] = (__bf16)(acc[1][2] + b1.z); o[7] = (__bf16)(acc[1][3] + b1.w);
      if (valid && p.qkv) *reinterpret_cast<bf16x8*>(p.qkv + row * (3 * FB_C) + n0) = o;
      if (ck < 3) {   // q: the softmax scale (and log2 e) goes onto the bf16 value, as the core kernel applies it to the q it reads from HBM
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (__bf16)((float)o[e] * qscale);
      }
      *reinterpret_cast<bf16x8*>(T + q * FB_LDT + n0) = o;
    }
    __syncthreads();                                                     // all key / value rows of both windows are in LDS
    // ---- attention, one head at a time; lane -> query lr, keys nt*16 + lg*4 + j
    const bool masked = tm.seam();                                       // uniform over the window
    const unsigned kdiff = masked ? seam_kdiff(tm, q, lg) : 0u;
#pragma unroll
    for (int h = 0; h < FB_HEADS; ++h) {
      f32x4 s[4];
      {
        const bf16x8 qf = *reinterpret_cast<const bf16x8*>(T + q * FB_LDT + h * HD + lg * 8);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(T + (nt * 16 + lr) * FB_LDT + FB_C + h * HD + lg * 8);
          s[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        }
      }
      // key padding: bias = -1e30 and the padded K rows are finite (LayerNorm of a zero row = beta)
      const float inv = softmax_lane<true, false>(s, bias[h], 1.f, masked, kdiff);
      bf16x8 pf[2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int j = 0; j < 4; ++j) { pf[ks][j] = (__bf16)(s[2 * ks][j] * inv); pf[ks][4 + j] = (__bf16)(s[2 * ks + 1][j] * inv); }
      f32x4 o[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          // V^T fragment of block nt: MFMA row lr <- head channel 8 (lr >> 2) + 4 nt + (lr & 3) (the chunk permutation above: the lanes with
          // lr & 3 = c supply the 4-column group that the lanes with lr >> 2 = c receive), the 8 keys of this lane group in the order the P
          // fragment holds them: keys 32 ks + 4 lg .. + 3 and 32 ks + 16 + 4 lg .. + 3
          const __bf16* src = T + (2 * ks * 16 + lg * 4 + (lr >> 2)) * FB_LDT + 2 * FB_C + h * HD + (lr & 3) * 8 + nt * 4;
          const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_a*)(src));
          const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_a*)(src + 16 * FB_LDT));
          const bf16x8 vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
          o[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[ks], o[nt], 0, 0, 0);
        }
      bf16x8 ob;                                                         // lane -> query lr, head channels 8 lg .. 8 lg + 7
#pragma unroll
      for (int j = 0; j < 4; ++j) { ob[j] = (__bf16)o[0][j]; ob[4 + j] = (__bf16)o[1][j]; }
      if (valid && p.att) *reinterpret_cast<bf16x8*>(p.att + row * FB_C + h * HD + lg * 8) = ob;
      *reinterpret_cast<bf16x8*>(T + q * FB_LDT + h * HD + lg * 8) = ob;   // over this wave's own q rows
    }
    __syncthreads();                                                     // keys / values are consumed: the next window may overwrite them
    // ---- x1 = x + s * (O Wp^T + bp), lane -> token lr, channels 32 ck + 8 lg .. + 7: the layout x was loaded in
    {
      const float sc = p.row_scale ? p.row_scale[tm.img] : 1.f;
      bf16x8 of[3];
#pragma unroll
      for (int ks = 0; ks < 3; ++ks) of[ks] = *reinterpret_cast<const bf16x8*>(T + q * FB_LDT + ks * 32 + lg * 8);
#pragma unroll
      for (int ck = 0; ck < 3; ++ck) {
        f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int ks = 0; ks < 3; ++ks)
#pragma unroll
          for (int hf = 0; hf < 2; ++hf) {
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(Wp + (ck * 32 + hf * 16 + lr) * FB_LDW + ks * 32 + lg * 8);
            acc[hf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, of[ks], acc[hf], 0, 0, 0);
          }
        if (valid) {
          const int n0 = ck * 32 + lg * 8;
          const float4 b0 = *reinterpret_cast<const float4*>(bp + n0), b1 = *reinterpret_cast<const float4*>(bp + n0 + 4);
          const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
          bf16x8 y;
#pragma unroll
          for (int e = 0; e < 8; ++e) y[e] = (__bf16)((float)xr[ck][e] + sc * (acc[e >> 2][e & 3] + bb[e]));
          *reinterpret_cast<bf16x8*>(p.x1 + row * FB_C + n0) = y;
        }
      }
    }
  }
}

// ---- MXFP8 forward of the same branch (opt-in sibling of swin_attn_block_fwd_kernel; sv_swin_attn_block_fwd_mx) --------------------------------
// The unfused MX chain composed in one kernel: sv_layernorm_quant_mx_fwd -> sv_linear_mxfp8 (bias) -> sv_window_attention_fwd_mxq (bf16 core) ->
// sv_linear_mxfp8 (bias, residual x, row_scale per image).  qkv and proj run on v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 x e4m3, cbsz = blgp = 0,
// E8M0 block scales as the two scale operands), ONE scaled MFMA per 16-column tile: Kp = roundup(96, 128) = 128 is a single k-step, bytes 96 .. 127
// are zero and block 3 carries scale byte 127.  No quantiser pass: LN(x) is quantised in the registers it is computed in, the head outputs from
// the wave's own rows of the LDS tile - one head of one token (32 channels) is exactly one MX block.  NORMATIVE recipe: linear_fp8.hip "MX recipe";
// the rounding is mx_block_exp / pack4_e4m3_mx (common.h), the quantiser, the prologue and the fragment reads are mx_frag.h's.
//   lanes         token q = 16 wave + t on lane (t, lg) everywhere (geometry, window walk and barriers of the bf16 kernel: 512 threads, two window
//                 groups, 4 waves x 16 rows per window).  B operand (mx_frag.h): the lane holds channels 16 lg .. + 15 and 64 + 16 lg .. + 15 of its
//                 token, lane groups 2 and 3 zeros in the upper half.  A operand: 16 weight rows per tile; tile 2 ck + hf, MFMA row i is output column
//                 32 ck + 8 (i >> 2) + 4 hf + (i & 3) (fbm_pack_row: the bf16 kernel's order), so the accumulators of a chunk's two tiles are the 8
//                 consecutive columns 32 ck + 8 lg .. + 7 of the lane's token: qkv, att and x1 keep the 16-byte accesses and the epilogues
//                 (fb_put_qkv, fb_put_x1) and the attention core (fb_attention) of the bf16 kernel.
//   LayerNorm     mx_layernorm on the B-operand layout (ln1 leaves as two + two 16-byte vectors), then mx_quant_frag.
//   proj operand  att (bf16, in the q columns of the wave's own tile rows) is read back in the B-operand layout - 2 + 2 ds_read_b128 - and goes
//                 through mx_quant_frag: blocks 0 / 1 / 2 are heads 0 / 1 / 2.
//   x             each window's rows are loaded where mx_layernorm needs them.  Fetching the NEXT window's rows ahead (as the bf16 kernel does) was
//                 built and measured: 208 VGPRs instead of 176 and 9 % SLOWER in the training form, level in the inference form - the
//                 kernel is not waiting for x.
//   residual      x arrives in the B-operand layout but x1 leaves in the chunk layout, so the residual is RE-READ from x in front of the projection
//                 epilogue: 3 x 16 bytes per lane = 192 bytes per token from L2 (the row was fetched by this very wave earlier in the window).
//                 Carrying it across would cost a second tile (64 x 96 bf16 = 12 KB per window) and a write + read of LDS per token.
//   weights       resident in LDS for the life of the workgroup in fragment order (every A fragment: two ds_read_b128, its scale one byte per lane).
// Pack image (sv_swin_attn_block_mx_pack, bytes):  WF [24 tiles][2 halves][64 lanes][16] | WS [24 tiles][64 lanes]; tiles 0 - 17 are qkv.weight's
// rows, tiles 18 - 23 proj.weight's; lane (r, lg) of tile T holds row fbm_pack_row(T, r), its bytes k = 16 lg .. + 15 (half 0) and 64 + 16 lg ..
// + 15 (half 1), and that row's scale byte lg.  The bytes are sv_quant_rows_mx_e4m3's, re-ordered, never re-quantised.
// LDS: 48 KB fragments + 1.5 KB scale bytes + 2 x 37 KB q | k | v tiles (FB_LDT) + 4.3 KB tables = 127.8 KB.
constexpr int FBM_QKV_TILES = 18, FBM_TILES = 24;
constexpr int FBM_WS = FBM_TILES * 2048, FBM_PACK_BYTES = FBM_WS + FBM_TILES * 64;
constexpr int FBM_SMEM = FBM_PACK_BYTES + 2 * 64 * FB_LDT * 2 + (3 * 176 + 288 + 3 * 96) * 4;
struct BlockFwdMxArgs : BlockFwdArgs { const uint8_t* packs; };   // wqkv / wproj stay NULL

// The ONLY copy of the row order of the image: output column (0 .. 287 of qkv, then 288 + 0 .. 95 of proj) of MFMA row r of tile T
__host__ __device__ __forceinline__ int fbm_pack_row(int T, int r) { return 32 * (T >> 1) + 8 * (r >> 2) + 4 * (T & 1) + (r & 3); }

__global__ __launch_bounds__(256) void swin_attn_block_mx_pack_kernel(const uint8_t* __restrict__ wqkv_q, const uint8_t* __restrict__ wqkv_s,
                                                                      const uint8_t* __restrict__ wproj_q, const uint8_t* __restrict__ wproj_s,
                                                                      uint8_t* __restrict__ packs) {
  const int e = blockIdx.x * 256 + threadIdx.x;              // item (tile, lane)
  if (e >= FBM_TILES * 64) return;
  const int T = e >> 6, lane = e & 63, lg = lane >> 4;
  const int n = fbm_pack_row(T, lane & 15);
  const bool proj = T >= FBM_QKV_TILES;
  const uint8_t* q = proj ? wproj_q + (size_t)(n - 3 * FB_C) * 128 : wqkv_q + (size_t)n * 128;
  const uint8_t* s = proj ? wproj_s + (n - 3 * FB_C) * 4 : wqkv_s + n * 4;
  mx_pack_item(q + 16 * lg, s[lg], packs, packs + FBM_WS, e);
}

__global__ __launch_bounds__(512, 1) void swin_attn_block_fwd_mx_kernel(const BlockFwdMxArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned char fbm_smem[FBM_SMEM];
  const uint8_t* WF = fbm_smem;                              // [24][2][64][16] weight fragments
  const uint8_t* WS = fbm_smem + FBM_WS;                     // [24][64] their scale bytes
  __bf16* Tb = reinterpret_cast<__bf16*>(fbm_smem + FBM_PACK_BYTES);   // 2 x [64][FB_LDT]  q (-> O) | k | v of the two windows in flight
  float* bt = reinterpret_cast<float*>(Tb + 2 * 64 * FB_LDT);   // [3][176] relative-position bias table per head, times log2 e
  float* bq = bt + 3 * 176;                                  // [288] qkv bias
  float* bp = bq + 288;                                      // [96] proj bias
  float* lng = bp + 96;                                      // [96] norm1 weight
  float* lnb = lng + 96;                                     // [96] norm1 bias
  const int tid = threadIdx.x, lane = tid & 63, wave = (tid >> 6) & 3, grp = tid >> 8;
  const int lr = lane & 15, lg = lane >> 4;
  for (int i = tid; i < FBM_PACK_BYTES / 16; i += 512) reinterpret_cast<i32x4*>(fbm_smem)[i] = reinterpret_cast<const i32x4*>(p.packs)[i];
  for (int i = tid; i < 3 * 169; i += 512) { const int h = i / 169, e = i - h * 169; bt[h * 176 + e] = p.table[e * FB_HEADS + h] * ATTN_LOG2E; }
  for (int i = tid; i < 288; i += 512) bq[i] = p.bqkv[i];
  if (tid < 96) { bp[tid] = p.bproj[tid]; lng[tid] = p.ln_g[tid]; lnb[tid] = p.ln_b[tid]; }
  __syncthreads();

  const int q = wave * 16 + lr;                      // the token (query) of this lane: B-operand column and transposed accumulator alike
  const bool qok = q < WT;
  float bias[FB_HEADS][4][4];
#pragma unroll
  for (int h = 0; h < FB_HEADS; ++h) lane_bias(bias[h], bt + h * 176, q, lg);
  __bf16* T = Tb + grp * 64 * FB_LDT;
  const int nWx = p.W / 7, nW = (p.H / 7) * nWx;
  const long long task0 = ((long long)blockIdx.x * 2 + grp) * p.tasks_per_group;
  const float qscale = p.scale * ATTN_LOG2E;
  const bool hi_live = lg < 2;                       // channels 64 + 16 lg .. + 15 exist (C = 96)
  auto to_bf16x8 = [](const float* v) { bf16x8 b; for (int e = 0; e < 8; ++e) b[e] = (__bf16)v[e]; return b; };

  TokMap tm = task_map(task0 < p.ntasks ? task0 : 0, nW, nWx, p.H, p.W, p.shift);
  const int qty = (qok ? q : 0) / 7, qtx = (qok ? q : 0) - qty * 7;       // this lane's token inside the window
  for (int tt = 0; tt < p.tasks_per_group; ++tt) {
    const bool valid = task0 + tt < p.ntasks && qok;                     // a dead window is uniform over its 4 waves
    int ys = tm.wy * 7 + qty + tm.shift; if (ys >= tm.H) ys -= tm.H;
    int xs = tm.wx * 7 + qtx + tm.shift; if (xs >= tm.W) xs -= tm.W;
    const size_t row = ((size_t)tm.img * tm.H + ys) * tm.W + xs;
    // ---- LayerNorm of the lane's token on the B-operand layout -> MX fragment of qkv; padded tokens load zeros (LayerNorm = beta: finite keys)
    i32x8 xq; int xsb;
    {
      float xv[2][16], mean, rstd;
      mx_layernorm<FB_C, false>(p.x, (long long)row, valid, lg, lng, lnb, p.eps, xv, mean, rstd);
      if (valid && p.ln1) {
        __bf16* dst = p.ln1 + row * FB_C + 16 * lg;
        *reinterpret_cast<bf16x8*>(dst) = to_bf16x8(xv[0]); *reinterpret_cast<bf16x8*>(dst + 8) = to_bf16x8(xv[0] + 8);
        if (hi_live) { *reinterpret_cast<bf16x8*>(dst + 64) = to_bf16x8(xv[1]); *reinterpret_cast<bf16x8*>(dst + 72) = to_bf16x8(xv[1] + 8); }
        if (lg == 0) { p.mean[row] = mean; p.rstd[row] = rstd; }
      }
      mx_quant_frag(xv, xq, xsb, lane);
    }
    // ---- qkv = bf16(acc + b), one 32-column chunk (= one head of q, k or v) = two scaled MFMAs at a time
#pragma unroll 3
    for (int ck = 0; ck < 9; ++ck) {
      f32x4 acc[2];
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
        acc[hf] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(mx_a_frag(WF, 2 * ck + hf, lane), xq, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0,
                                                                   mx_a_scale(WS, 2 * ck + hf, lane), 0, xsb);
      fb_put_qkv(acc, ck, bq, T, q, lg, qscale, valid && p.qkv, p.qkv, row);
    }
    __syncthreads();                                                     // all key / value rows of both windows are in LDS
    fb_attention(T, bias, tm, q, lr, lg, valid && p.att, p.att, row);
    __syncthreads();                                                     // keys / values are consumed: the next window may overwrite them
    // ---- x1 = x + s * (att_q Wp_q^T + bp): att from the wave's own tile rows, one block per head
    {
      float av[2][16];
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          bf16x8 raw = VecN<__bf16, 8>::zero();
          if (hf == 0 || hi_live) raw = *reinterpret_cast<const bf16x8*>(T + q * FB_LDT + 64 * hf + 16 * lg + 8 * u);
#pragma unroll
          for (int e = 0; e < 8; ++e) av[hf][8 * u + e] = (float)raw[e];
        }
      i32x8 aq; int asb;
      mx_quant_frag(av, aq, asb, lane);
      const float sc = valid && p.row_scale ? p.row_scale[tm.img] : 1.f;
#pragma unroll
      for (int ck = 0; ck < 3; ++ck) {
        f32x4 acc[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
          acc[hf] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(mx_a_frag(WF, FBM_QKV_TILES + 2 * ck + hf, lane), aq, (f32x4){0.f, 0.f, 0.f, 0.f},
                                                                     0, 0, 0, mx_a_scale(WS, FBM_QKV_TILES + 2 * ck + hf, lane), 0, asb);
        if (valid) fb_put_x1(acc, ck, bp, lg, sc, *reinterpret_cast<const bf16x8*>(p.x + row * FB_C + ck * 32 + lg * 8), p.x1 + row * FB_C);
      }
    }
    if (++tm.wx == nWx) { tm.wx = 0; if (++tm.wy == p.H / 7) { tm.wy = 0; ++tm.img; } }
  }
}


// ---- fused BACKWARD of the attention branch of a stage-0 Swin block (C = 96, 3 heads) ------------------------------------------------
// x1 = x + s * proj(window_attention(qkv(LayerNorm(x)))).  The unfused chain of this backward is four kernels over the token map - projection
// data gradient, attention core backward, qkv data gradient, LayerNorm backward + residual - with datt, dqkv and dln1 going through HBM in
// between: 17 passes over an [M, 96] tensor.  Here the data path is ONE kernel, 9 passes: it reads dx1, qkv (saved by the forward), x (+ the
// saved LayerNorm statistics) and writes dqkv (the weight-gradient kernels of the engine need it in HBM) and dx.
// One workgroup = 4 waves = one window at a time (49 tokens padded to 64; wave w owns token rows 16 w .. 16 w + 15 wherever rows are
// owned); both weight matrices sit in LDS in DATA-GRADIENT orientation:
//   P1  datt = (s dx1) Wproj          A rows = input channel j of proj, k = output channel   [96][96]
//   P2  per head: the body of win_attn_bwd_wg_kernel (P recomputed) on the q | k | v columns of the window tile; dq / dk / dv leave for HBM
//       as 16-byte row vectors and overwrite the head's q | k | v columns of the tile once every wave is done reading them
//   P3  dln = dqkv Wqkv               A rows = input channel c of qkv, k = output column     [96][288]
//   P4  LayerNorm backward + residual on the accumulators: dx = dx1 + rstd (g - mean(g) - xhat mean(g xhat)), g = dln gamma
// Every product takes the weights as the FIRST MFMA operand with the row permutation of the forward kernel, so a lane's accumulators are
// the 8 consecutive channels 32 ck + 8 lg .. + 7 of ONE token: every global access is a 16-byte vector in one layout (dx1, x, qkv, dqkv, dx),
// and the LayerNorm row sums are 24 in-lane values + two lane-group exchanges.  dgamma / dbeta and the bias-table gradient stay in
// registers over all windows of the workgroup.  The next window's dx1 and qkv rows are prefetched into registers during the current one.
struct BlockBwdArgs {
  const __bf16 *dx1, *qkv, *x; const float *mean, *rstd, *ln_g, *wqkv, *wproj, *table, *row_scale;
  __bf16 *dqkv, *dx, *dbr; float *dgamma, *dbeta, *dt_ws;
  int I, H, W, shift; float scale; int ntasks, tasks_per_group;
};
constexpr int BB_LDT = 296;   // bf16 row stride of the q | k | v (then dq | dk | dv) tile and of the qkv weight image: 592 bytes = 37 x 16
constexpr int BB_LDD = 104;   // bf16 row stride of the s dx1 (then datt) tile and of the proj weight image: 208 bytes = 13 x 16
constexpr int BB_SMEM = 96 * BB_LDT * 2 + 96 * BB_LDD * 2 + 64 * BB_LDT * 2 + 64 * BB_LDD * 2 + 2 * 64 * LDP_H * 2 + (3 * 176 * 2 + 96 + 2 * 96) * 4;

__global__ __launch_bounds__(256, 1) void swin_attn_block_bwd_kernel(const BlockBwdArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned char bb_smem[BB_SMEM];
  __bf16* Wq = reinterpret_cast<__bf16*>(bb_smem);          // [96][BB_LDT]  row R (permuted input channel c): Wqkv[k][c], k = 0 .. 287
  __bf16* Wp = Wq + 96 * BB_LDT;                             // [96][BB_LDD]  row R (permuted input channel j): Wproj[i][j], i = 0 .. 95
  __bf16* T = Wp + 96 * BB_LDD;                              // [64][BB_LDT]  scale q | k | v, then dq | dk | dv
  __bf16* D = T + 64 * BB_LDT;                               // [64][BB_LDD]  s dx1, then datt
  __bf16* Ps = D + 64 * BB_LDD;                              // [64][LDP_H]   P  [query][key]
  __bf16* Ss = Ps + 64 * LDP_H;                              // [64][LDP_H]   dS [query][key]
  float* bt = reinterpret_cast<float*>(Ss + 64 * LDP_H);     // [3][176] bias table per head
  float* dbt = bt + 3 * 176;                                 // [3][176] its gradient (filled once, at the end)
  float* lng = dbt + 3 * 176;                                // [96] norm1 weight
  float* red = lng + 96;                                     // [2][96] dgamma / dbeta of the workgroup
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  // weight images, transposed from the native [out][in] layouts; LDS row R = 32 chunk + 16 half + ii <- channel 32 chunk + 8 (ii >> 2) + 4 half + (ii & 3)
  for (int i = tid; i < 96 * 288; i += 256) {
    const int R = i / 288, k = i - R * 288, ii = R & 15, c = (R & ~31) + 8 * (ii >> 2) + 4 * ((R >> 4) & 1) + (ii & 3);
    Wq[R * BB_LDT + k] = (__bf16)p.wqkv[k * FB_C + c];
  }
  for (int i = tid; i < 96 * 96; i += 256) {
    const int R = i / 96, k = i - R * 96, ii = R & 15, c = (R & ~31) + 8 * (ii >> 2) + 4 * ((R >> 4) & 1) + (ii & 3);
    Wp[R * BB_LDD + k] = (__bf16)p.wproj[k * FB_C + c];
  }
  for (int i = tid; i < 3 * 176; i += 256) { const int h = i / 176, e = i - h * 176; bt[i] = e < 169 ? p.table[e * FB_HEADS + h] : 0.f; dbt[i] = 0.f; }
  if (tid < 96) { lng[tid] = p.ln_g[tid]; red[tid] = 0.f; red[96 + tid] = 0.f; }
  __syncthreads();

  const int q = wave * 16 + lr;                      // the token of this lane wherever rows are owned (queries of P2, keys of its second half)
  const bool qok = q < WT;
  float bias[FB_HEADS][4][4];
#pragma unroll
  for (int h = 0; h < FB_HEADS; ++h) lane_bias(bias[h], bt + h * 176, q, lg, ATTN_LOG2E);   // exp2 domain
  const bf16x8 zero8 = {(__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f};
  f32x4 dsum[FB_HEADS][4];                           // bias-table gradient at this lane's (query, key) slots, over all windows
#pragma unroll
  for (int h = 0; h < FB_HEADS; ++h)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) dsum[h][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float dgam[3][8], dbet[3][8];                      // LayerNorm parameter gradients of this lane's channels 32 ck + 8 lg + e, over all windows
#pragma unroll
  for (int ck = 0; ck < 3; ++ck)
#pragma unroll
    for (int e = 0; e < 8; ++e) { dgam[ck][e] = 0.f; dbet[ck][e] = 0.f; }

  const int nWx = p.W / 7, nW = (p.H / 7) * nWx;
  const long long task0 = (long long)blockIdx.x * p.tasks_per_group;
  TokMap tnext = task_map(task0 < p.ntasks ? task0 : 0, nW, nWx, p.H, p.W, p.shift);
  const int qty = (qok ? q : 0) / 7, qtx = (qok ? q : 0) - qty * 7;
  auto token_row = [&](const TokMap& t) -> size_t {
    int ys = t.wy * 7 + qty + t.shift; if (ys >= t.H) ys -= t.H;
    int xs = t.wx * 7 + qtx + t.shift; if (xs >= t.W) xs -= t.W;
    return ((size_t)t.img * t.H + ys) * t.W + xs;
  };
  bf16x8 nd[3], nq[9];                               // the NEXT window's dx1 and qkv chunks of this lane's token
  auto fetch = [&](bool in_range) {
#pragma unroll
    for (int i = 0; i < 3; ++i) nd[i] = zero8;
#pragma unroll
    for (int i = 0; i < 9; ++i) nq[i] = zero8;
    if (in_range && qok) {
      const size_t row = token_row(tnext);
      const __bf16* sd = p.dx1 + row * FB_C + lg * 8;
      const __bf16* sq = p.qkv + row * (3 * FB_C) + lg * 8;
#pragma unroll
      for (int i = 0; i < 3; ++i) nd[i] = *reinterpret_cast<const bf16x8*>(sd + 32 * i);
#pragma unroll
      for (int i = 0; i < 9; ++i) nq[i] = *reinterpret_cast<const bf16x8*>(sq + 32 * i);
    }
  };
  fetch(task0 < p.ntasks);
  for (int tt = 0; tt < p.tasks_per_group; ++tt) {
    const long long task = task0 + tt;
    if (task >= p.ntasks) break;                     // uniform over the workgroup
    const TokMap tm = tnext;
    const bool valid = qok;
    const size_t row = token_row(tm);
    bf16x8 dxr[3], xr[3];                            // dx1 (unscaled, for the residual) and x of this lane's token
    const float sc = p.row_scale ? p.row_scale[tm.img] : 1.f;
    float mean = 0.f, rstd = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) { dxr[i] = nd[i]; xr[i] = zero8; }
    if (valid) {
      const __bf16* sx = p.x + row * FB_C + lg * 8;
#pragma unroll
      for (int i = 0; i < 3; ++i) xr[i] = *reinterpret_cast<const bf16x8*>(sx + 32 * i);       // consumed in P4: lands during P1 - P3
      mean = p.mean[row]; rstd = p.rstd[row];
    }
    __syncthreads();                                 // the previous window's tiles are consumed
    // ---- tiles: s dx1 -> D, scale q | k | v -> T (q is rounded to bf16 AFTER the scale goes on, as the unfused core does with the q it reads)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (__bf16)(sc * (float)dxr[i][e]);
      *reinterpret_cast<bf16x8*>(D + q * BB_LDD + 32 * i + lg * 8) = o;
      if (p.dbr && valid) *reinterpret_cast<bf16x8*>(p.dbr + row * FB_C + 32 * i + lg * 8) = o;   // for the projection's weight gradient
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      bf16x8 o = nq[i];
      if (i < 3) {
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (__bf16)((float)o[e] * p.scale);
      }
      *reinterpret_cast<bf16x8*>(T + q * BB_LDT + 32 * i + lg * 8) = o;
    }
    if (++tnext.wx == nWx) { tnext.wx = 0; if (++tnext.wy == p.H / 7) { tnext.wy = 0; ++tnext.img; } }
    fetch(tt + 1 < p.tasks_per_group && task + 1 < p.ntasks);
    // ---- P1: datt = (s dx1) Wproj for this wave's 16 tokens (its own rows of D: no barrier), written back over them
    {
      bf16x8 df[3];
#pragma unroll
      for (int ks = 0; ks < 3; ++ks) df[ks] = *reinterpret_cast<const bf16x8*>(D + q * BB_LDD + ks * 32 + lg * 8);
#pragma unroll
      for (int ck = 0; ck < 3; ++ck) {
        f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int ks = 0; ks < 3; ++ks)
#pragma unroll
          for (int hf = 0; hf < 2; ++hf) {
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(Wp + (ck * 32 + hf * 16 + lr) * BB_LDD + ks * 32 + lg * 8);
            acc[hf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, df[ks], acc[hf], 0, 0, 0);
          }
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (__bf16)acc[e >> 2][e & 3];
        *reinterpret_cast<bf16x8*>(D + q * BB_LDD + ck * 32 + lg * 8) = o;
      }
    }
    __syncthreads();                                 // every row of T and of D (= datt) is in LDS
    const bool masked = tm.seam();                   // uniform over the workgroup
    const unsigned kdiff = masked ? seam_kdiff(tm, q, lg) : 0u;
    // ---- P2: attention backward, one head at a time (win_attn_bwd_wg_kernel's body on the tile columns of the head)
#pragma unroll
    for (int h = 0; h < FB_HEADS; ++h) {
      const __bf16* Qs = T + h * HD;
      const __bf16* Ks = T + FB_C + h * HD;
      const __bf16* Vs = T + 2 * FB_C + h * HD;
      const __bf16* Ds = D + h * HD;
      f32x4 s[4], dp[4];
      {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(Qs + q * BB_LDT + lg * 8), c = *reinterpret_cast<const bf16x8*>(Ds + q * BB_LDD + lg * 8);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const bf16x8 b = *reinterpret_cast<const bf16x8*>(Ks + (nt * 16 + lr) * BB_LDT + lg * 8);
          const bf16x8 d = *reinterpret_cast<const bf16x8*>(Vs + (nt * 16 + lr) * BB_LDT + lg * 8);
          s[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, a, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          dp[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(d, c, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        }
      }
      {
        // scores in the exp2 domain: log2 e rides on the bias (above) and on the raw product here (Q carries the plain softmax scale, as the
        // dK product needs it)
        softmax_lane<true, true>(s, bias[h], ATTN_LOG2E, masked, kdiff);
        float r = 0.f;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int j = 0; j < 4; ++j) r += dp[nt][j] * s[nt][j];
        r = lanegroup_allreduce(r, FAdd2());
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float dsv = s[nt][j] * (dp[nt][j] - r);
            dp[nt][j] = dsv;
            if (qok && nt * 16 + lg * 4 + j < WT) dsum[h][nt][j] += dsv;
          }
      }
      bf16x8 dsf[2];                                 // dS of this query as the second operand of dQ = dS K
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        bf16x4 pb, sb;
#pragma unroll
        for (int j = 0; j < 4; ++j) { pb[j] = (__bf16)s[nt][j]; sb[j] = (__bf16)dp[nt][j]; dsf[nt >> 1][(nt & 1) * 4 + j] = sb[j]; }
        *reinterpret_cast<bf16x4*>(Ps + q * LDP_H + nt * 16 + lg * 4) = pb;
        *reinterpret_cast<bf16x4*>(Ss + q * LDP_H + nt * 16 + lg * 4) = sb;
      }
      f32x4 aq[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};   // dQ = scale dS K: lane -> query lr, head channels 8 lg + 4 nt + j
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          const __bf16* src = Ks + (2 * ks * 16 + lg * 4 + (lr >> 2)) * BB_LDT + (lr & 3) * 8 + nt * 4;
          const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_a*)(src));
          const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_a*)(src + 16 * BB_LDT));
          const bf16x8 kT = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
          aq[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kT, dsf[ks], aq[nt], 0, 0, 0);
        }
      __syncthreads();                               // P and dS of all 64 queries are in LDS
      f32x4 av[2], ak[2];                            // this wave's 16 KEYS: dV = P^T dO, dK = dS^T (scale Q)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) { av[nt] = (f32x4){0.f, 0.f, 0.f, 0.f}; ak[nt] = av[nt]; }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 pT = tr_frag(Ps, LDP_H, ks * 32, wave * 16, lane);
        const bf16x8 sT = tr_frag(Ss, LDP_H, ks * 32, wave * 16, lane);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          const bf16x8 bd = tr_frag_perm(Ds, BB_LDD, ks * 32, nt, lane);
          const bf16x8 bq = tr_frag_perm(Qs, BB_LDT, ks * 32, nt, lane);
          av[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bd, pT, av[nt], 0, 0, 0);
          ak[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bq, sT, ak[nt], 0, 0, 0);
        }
      }
      bf16x8 oq, ok_, ov;
#pragma unroll
      for (int e = 0; e < 8; ++e) { oq[e] = (__bf16)(aq[e >> 2][e & 3] * p.scale); ok_[e] = (__bf16)ak[e >> 2][e & 3]; ov[e] = (__bf16)av[e >> 2][e & 3]; }
      if (valid) {
        __bf16* dst = p.dqkv + row * (3 * FB_C) + h * HD + lg * 8;
        *reinterpret_cast<bf16x8*>(dst) = oq;
        *reinterpret_cast<bf16x8*>(dst + FB_C) = ok_;
        *reinterpret_cast<bf16x8*>(dst + 2 * FB_C) = ov;
      }
      __syncthreads();                               // every wave is done with this head's q | k | v, P and dS
      {
        __bf16* dstl = T + q * BB_LDT + h * HD + lg * 8;     // this wave's own rows: dq | dk | dv become the operand of P3 (zero rows for the padding)
        *reinterpret_cast<bf16x8*>(dstl) = valid ? oq : zero8;
        *reinterpret_cast<bf16x8*>(dstl + FB_C) = valid ? ok_ : zero8;
        *reinterpret_cast<bf16x8*>(dstl + 2 * FB_C) = valid ? ov : zero8;
      }
    }
    // ---- P3: dln = dqkv Wqkv for this wave's 16 tokens (its own rows of T), P4: LayerNorm backward + residual on the accumulators
    {
      bf16x8 gf[9];
#pragma unroll
      for (int ks = 0; ks < 9; ++ks) gf[ks] = *reinterpret_cast<const bf16x8*>(T + q * BB_LDT + ks * 32 + lg * 8);
      float dl[3][8], xh[3][8];
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int ck = 0; ck < 3; ++ck) {
        f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int ks = 0; ks < 9; ++ks)
#pragma unroll
          for (int hf = 0; hf < 2; ++hf) {
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(Wq + (ck * 32 + hf * 16 + lr) * BB_LDT + ks * 32 + lg * 8);
            acc[hf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, gf[ks], acc[hf], 0, 0, 0);
          }
        const float4 g0 = *reinterpret_cast<const float4*>(lng + ck * 32 + lg * 8), g1 = *reinterpret_cast<const float4*>(lng + ck * 32 + lg * 8 + 4);
        const float gm[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          // the unfused chain stores dln1 as bf16 between the qkv data gradient and the LayerNorm backward: the same rounding here
          const float d = valid ? (float)(__bf16)acc[e >> 2][e & 3] : 0.f;
          const float xv = valid ? ((float)xr[ck][e] - mean) * rstd : 0.f;
          dbet[ck][e] += d; dgam[ck][e] += d * xv;
          const float g = d * gm[e];
          dl[ck][e] = g; xh[ck][e] = xv;
          s1 += g;
          // g xhat is rounded before it is summed: left to the compiler, whether the product is fused into the sum follows from how the loop
          // happens to be vectorised, and dx changes in its last bit with unrelated edits of this kernel
          {
#pragma clang fp contract(off)
            s2 += g * xv;
          }
        }
      }
      s1 = lanegroup_allreduce(s1, FAdd2()) * (1.f / FB_C);
      s2 = lanegroup_allreduce(s2, FAdd2()) * (1.f / FB_C);
      if (valid) {
#pragma unroll
        for (int ck = 0; ck < 3; ++ck) {
          bf16x8 o;
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = (__bf16)((float)dxr[ck][e] + rstd * (dl[ck][e] - s1 - xh[ck][e] * s2));
          *reinterpret_cast<bf16x8*>(p.dx + row * FB_C + ck * 32 + lg * 8) = o;
        }
      }
    }
  }
  // ---- parameter gradients: registers -> LDS (once per workgroup) -> atomics
  __syncthreads();
#pragma unroll
  for (int ck = 0; ck < 3; ++ck)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float a = group16_sum(dgam[ck][e]), b = group16_sum(dbet[ck][e]);      // the 16 tokens of a lane group
      if (lr == 0) { atomicAdd(red + ck * 32 + lg * 8 + e, a); atomicAdd(red + 96 + ck * 32 + lg * 8 + e, b); }
    }
  dbias_flush<false, FB_HEADS>(dsum, dbt, p.dt_ws + (size_t)(blockIdx.x % ATTN_DT_SLOTS) * 169 * FB_HEADS, 0, FB_HEADS, lane, wave);
  if (tid < 96) { atomicAdd(p.dgamma + tid, red[tid]); atomicAdd(p.dbeta + tid, red[96 + tid]); }   // behind the barrier of the flush
}

}  // namespace sv

using namespace sv;

// the window geometry every entry point of the window kernels requires; `who` names the entry point in the message
static int win_geom_check(const char* who, int H, int W, int shift) {
  SV_REQUIRE(H % 7 == 0 && W % 7 == 0 && H >= 7 && W >= 7, "%s: map %dx%d is not a multiple of the 7x7 window", who, H, W);
  SV_REQUIRE(shift >= 0 && shift < 7 && (shift == 0 || (H > 7 && W > 7)), "%s: bad shift %d for map %dx%d", who, shift, H, W);
  return SV_OK;
}

static int win_check(const void* qkv, const float* table, int I, int H, int W, int C, int heads, int shift, int math, int act_dtype) {
  SV_REQUIRE(qkv && table && I > 0, "window_attention: null/empty argument");
  if (int rc = win_geom_check("window_attention", H, W, shift)) return rc;
  SV_REQUIRE(C == heads * HD, "window_attention: C (%d) must equal heads (%d) * 32", C, heads);
  SV_REQUIRE(((uintptr_t)qkv & 15) == 0, "window_attention: qkv must be 16-byte aligned");
  SV_REQUIRE_ACT(act_dtype);
  SV_REQUIRE(act_dtype == SV_F32 || math == SV_MATH_BF16 || math == SV_MATH_FP8 || math == SV_MATH_FP8_FULL,
             "window_attention: bf16 activations require SV_MATH_BF16 / SV_MATH_FP8 / SV_MATH_FP8_FULL");
  return SV_OK;
}

// the arguments of sv_window_attention_fwd / _bwd, as they arrive
struct WinCall {
  const void* qkv; const float* table; void* out; const void* dout; void* dqkv; float* dtable;
  int I, H, W, C, heads, shift;
  int ntasks() const { return I * (H / 7) * (W / 7); }
};
template <typename AT>
static WinArgsT<AT> win_args(const WinCall& c, int tasks_per_wave) {
  WinArgsT<AT> a{};
  a.qkv = static_cast<const AT*>(c.qkv); a.table = c.table; a.out = static_cast<AT*>(c.out);
  a.dout = static_cast<const AT*>(c.dout); a.dqkv = static_cast<AT*>(c.dqkv); a.dtable = c.dtable;
  a.I = c.I; a.H = c.H; a.W = c.W; a.C = c.C; a.heads = c.heads; a.shift = c.shift;
  a.scale = 1.0f / sqrtf((float)HD);
  a.ntasks = c.ntasks();
  a.tasks_per_wave = tasks_per_wave;
  return a;
}

static void launch_dtable_fold(float* workspace, float* dtable, int heads, hipStream_t s) {
  hipLaunchKernelGGL(attn_dtable_fold_kernel, dim3(cdiv(169 * heads, 256)), dim3(256), 0, s, workspace, dtable, 169 * heads);
}

// Consecutive windows of one head per workgroup (per wave in the exact-fp32 kernels) of the launch for these arguments: the launches below
// and sv_window_attention_windows_per_group both take it from here.
//  * bf16 / fp8 forward: >= ~2048 short workgroups (the forward task is brief, oversubscribing the CUs balances better than one exact wave
//    - measured);
//  * bf16 / fp8 backward: one resident wave of workgroups, 3 per CU;
//  * exact fp32: wave per window; the backward walks several windows per wave so the bias gradient is reduced on chip.
static int win_share(int ntasks, int heads, int math, bool bwd) {
  if (math == SV_MATH_BF16 || math == SV_MATH_FP8 || math == SV_MATH_FP8_FULL) {
    if (bwd) return wg_tasks_per_block(ntasks, heads, 3);
    int tpb = (int)((long long)ntasks * heads / 2048);
    if (tpb < 1) tpb = 1;
    if (tpb > 8) tpb = 8;
    return tpb;
  }
  int tpw = 1;
  while (bwd && tpw < 8 && (long long)ntasks * heads / (tpw * 2) > 2048) tpw *= 2;
  return tpw;
}
// Fused stage-0 block, windows per window group.  Forward: one workgroup (two window groups) per CU, every group the same share;
// backward: one workgroup (one group) per CU, every workgroup the same share of consecutive windows.
static int block_share(int ntasks, bool bwd) { return cdiv(ntasks, bwd ? 256 : 512); }

// The four workgroup-per-window kernels: a workgroup walks tpb windows of one head.  Backward: the bias-table gradient goes to the slot
// images of `workspace` (folded into dtable by a second launch) or, without a workspace, straight to dtable.
static void launch_win_wg(bool bwd, bool fp8, int act_dtype, const WinCall& c, int tpb, float* workspace, hipStream_t s) {
  const int ntasks = c.ntasks();
  const dim3 grid(wg_grid(cdiv(ntasks, tpb), c.heads));
  SV_DISPATCH_ACT(act_dtype,
    const WinArgsT<AT> a = win_args<AT>(c, tpb);
    if (!bwd && !fp8) hipLaunchKernelGGL(win_attn_fwd_wg_kernel<AT>, grid, dim3(256), 0, s, a);
    else if (!bwd) hipLaunchKernelGGL(win_attn_fwd_wg_fp8_kernel<AT>, grid, dim3(256), 0, s, a);
    else if (!fp8) hipLaunchKernelGGL(win_attn_bwd_wg_kernel<AT>, grid, dim3(256), 0, s, a, workspace);
    else hipLaunchKernelGGL(win_attn_bwd_wg_fp8_kernel<AT>, grid, dim3(256), 0, s, a, workspace););
  if (bwd && workspace) launch_dtable_fold(workspace, c.dtable, c.heads, s);
}

extern "C" int sv_window_attention_fwd(const void* qkv, const float* table, void* out, int I, int H, int W, int C, int heads,
                                       int shift, int math, int act_dtype, void* stream) {
  if (int rc = win_check(qkv, table, I, H, W, C, heads, shift, math, act_dtype)) return rc;
  SV_REQUIRE(out, "window_attention_fwd: null out");
  const WinCall c{qkv, table, out, nullptr, nullptr, nullptr, I, H, W, C, heads, shift};
  hipStream_t s = (hipStream_t)stream;
  const bool fp8 = math == SV_MATH_FP8 || math == SV_MATH_FP8_FULL;   // e4m3 operands for QK^T and PV (the backward of SV_MATH_FP8 is bf16)
  const int share = win_share(c.ntasks(), heads, math, false);
  if (fp8 || math == SV_MATH_BF16) launch_win_wg(false, fp8, act_dtype, c, share, nullptr, s);
  else   // exact-fp32 MFMA: wave per window
    hipLaunchKernelGGL(win_attn_fwd_kernel, dim3(cdiv(c.ntasks(), 4), heads), dim3(256), 0, s, win_args<float>(c, share));
  return check_launch("sv_window_attention_fwd");
}

extern "C" int sv_window_attention_fwd_mxq(const void* qkv, const float* table, void* out, int I, int H, int W, int C, int heads, int shift, int math,
                                           void* q_out, int Kp, void* qs_out, int act_dtype, void* stream) {
  if (int rc = win_check(qkv, table, I, H, W, C, heads, shift, math, act_dtype)) return rc;
  SV_REQUIRE(math == SV_MATH_BF16 || math == SV_MATH_FP8 || math == SV_MATH_FP8_FULL,
             "window_attention_fwd_mxq: served by the bf16 and fp8 workgroup kernels only (math %d)", math);
  SV_REQUIRE(q_out && qs_out, "window_attention_fwd_mxq: null q_out / qs_out");
  SV_REQUIRE(Kp == cdiv(C, 128) * 128, "window_attention_fwd_mxq: Kp (%d) must be C (%d) rounded up to a multiple of 128", Kp, C);
  SV_REQUIRE(((uintptr_t)q_out & 15) == 0 && ((uintptr_t)qs_out & 3) == 0, "window_attention_fwd_mxq: q_out must be 16-byte, qs_out 4-byte aligned");
  const WinCall c{qkv, table, out, nullptr, nullptr, nullptr, I, H, W, C, heads, shift};
  hipStream_t s = (hipStream_t)stream;
  const bool fp8 = math != SV_MATH_BF16;
  const int tpb = win_share(c.ntasks(), heads, math, false);
  const dim3 grid(wg_grid(cdiv(c.ntasks(), tpb), heads));
  SV_DISPATCH_ACT(act_dtype,
    WinMxqArgsT<AT> a{};
    static_cast<WinArgsT<AT>&>(a) = win_args<AT>(c, tpb);
    a.q_out = static_cast<uint8_t*>(q_out); a.qs_out = static_cast<uint8_t*>(qs_out); a.Kp = Kp;
    if (!fp8) hipLaunchKernelGGL((win_attn_fwd_wg_kernel<AT, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((win_attn_fwd_wg_fp8_kernel<AT, true>), grid, dim3(256), 0, s, a););
  return check_launch("sv_window_attention_fwd_mxq");
}

extern "C" int sv_window_attention_windows_per_group(int I, int H, int W, int heads, int math, int backward) {
  SV_REQUIRE(I > 0 && heads > 0, "window_attention_windows_per_group: I (%d) and heads (%d) must be positive", I, heads);
  SV_REQUIRE(math == SV_MATH_F32 || math == SV_MATH_BF16 || math == SV_MATH_FP8 || math == SV_MATH_FP8_FULL,
             "window_attention_windows_per_group: unknown math mode %d", math);
  if (int rc = win_geom_check("window_attention_windows_per_group", H, W, 0)) return rc;
  return win_share(I * (H / 7) * (W / 7), heads, math, backward != 0);
}

extern "C" size_t sv_window_attention_bwd_workspace_floats(int heads) { return (size_t)ATTN_DT_SLOTS * 169 * heads; }

extern "C" int sv_window_attention_bwd(const void* qkv, const float* table, const void* dout, void* dqkv, float* dtable, float* workspace,
                                       int I, int H, int W, int C, int heads, int shift, int math, int act_dtype, void* stream) {
  if (int rc = win_check(qkv, table, I, H, W, C, heads, shift, math, act_dtype)) return rc;
  SV_REQUIRE(dout && dqkv && dtable && ((uintptr_t)dout & 15) == 0, "window_attention_bwd: null/unaligned argument");
  const WinCall c{qkv, table, nullptr, dout, dqkv, dtable, I, H, W, C, heads, shift};
  hipStream_t s = (hipStream_t)stream;
  const int share = win_share(c.ntasks(), heads, math, true);
  if (math == SV_MATH_BF16 || math == SV_MATH_FP8 || math == SV_MATH_FP8_FULL) {
    // SV_MATH_FP8_FULL: e4m3 operands for all five contractions, the gradient of the SV_MATH_FP8 forward; SV_MATH_FP8: the bf16 backward
    launch_win_wg(true, math == SV_MATH_FP8_FULL, act_dtype, c, share, workspace, s);
  } else {
    // exact-fp32 MFMA: wave per window, several windows per wave (same head) so the bias gradient is reduced on chip
    const int tpw = share;
    hipLaunchKernelGGL(win_attn_bwd_kernel, dim3(cdiv(c.ntasks(), 2 * tpw), heads), dim3(128), 0, s, win_args<float>(c, tpw));
  }
  return check_launch("sv_window_attention_bwd");
}

static int cva_check(int B, int V, int P, int R, int heads) {
  SV_REQUIRE(B > 0 && V > 0 && V <= CVA_MAXV, "cross_view_attention: n_views=%d unsupported (max %d)", V, CVA_MAXV);
  SV_REQUIRE(heads > 0 && R % heads == 0 && P > 0 && R / heads <= CVA_MAXF, "cross_view_attention: head_dim %d exceeds %d",
             R / (heads > 0 ? heads : 1), CVA_MAXF);
  return SV_OK;
}
// features per chunk: whole positions, as many as the LDS arrays hold
static int cva_chunk(int P, int R, int heads) { const int hd = R / heads; return min(P, CVA_MAXF / hd) * hd; }

extern "C" int sv_cross_view_attention_fwd(const void* qkv, void* out, int B, int V, int P, int R, int heads, int act_dtype, void* stream) {
  SV_REQUIRE(qkv && out, "cross_view_attention_fwd: null argument");
  SV_REQUIRE_ACT(act_dtype);
  if (int rc = cva_check(B, V, P, R, heads)) return rc;
  SV_DISPATCH_ACT(act_dtype,
    CvaArgsT<AT> a{static_cast<const AT*>(qkv), static_cast<AT*>(out), nullptr, nullptr, B, V, P, R, heads, R / heads, cva_chunk(P, R, heads), 1.0f / sqrtf((float)(R / heads) * (float)V)};
    hipLaunchKernelGGL(cva_attn_fwd_kernel<AT>, dim3(B * heads), dim3(256), 0, (hipStream_t)stream, a););
  return check_launch("sv_cross_view_attention_fwd");
}

extern "C" int sv_cross_view_attention_bwd(const void* qkv, const void* dout, void* dqkv, int B, int V, int P, int R, int heads,
                                           int act_dtype, void* stream) {
  SV_REQUIRE(qkv && dout && dqkv, "cross_view_attention_bwd: null argument");
  SV_REQUIRE_ACT(act_dtype);
  if (int rc = cva_check(B, V, P, R, heads)) return rc;
  SV_DISPATCH_ACT(act_dtype,
    CvaArgsT<AT> a{static_cast<const AT*>(qkv), nullptr, static_cast<const AT*>(dout), static_cast<AT*>(dqkv), B, V, P, R, heads, R / heads,
                   cva_chunk(P, R, heads), 1.0f / sqrtf((float)(R / heads) * (float)V)};
    hipLaunchKernelGGL(cva_attn_bwd_kernel<AT>, dim3(B * heads), dim3(256), 0, (hipStream_t)stream, a););
  return check_launch("sv_cross_view_attention_bwd");
}

// ---- fused attention branch of a stage-0 Swin block ------------------------------------------------------------------------------------
extern "C" int sv_swin_attn_block_supported(int C, int heads, int act_dtype, int math) {
  return C == FB_C && heads == FB_HEADS && act_dtype == SV_BF16 && math == SV_MATH_BF16;
}

// What sv_swin_attn_block_fwd and sv_swin_attn_block_fwd_mx ask alike, and the arguments and launch geometry they share; `who` names the entry
// that was called, `weights` are its weight operands (fp32 matrices or the MX pack): all present, or-ed together for the alignment rule.
static int block_fwd_args(const char* who, BlockFwdArgs& a, bool weights, uintptr_t weight_bits, const void* x, const float* ln_g, const float* ln_b,
                          const float* bqkv, const float* table, const float* bproj, const float* row_scale, void* x1, void* ln1, float* mean,
                          float* rstd, void* qkv, void* att, int I, int H, int W, int C, int heads, int shift, float eps, int act_dtype) {
  SV_REQUIRE(x && ln_g && ln_b && weights && bqkv && table && bproj && x1 && I > 0, "%s: null/empty argument", who);
  SV_REQUIRE(C == FB_C && heads == FB_HEADS && act_dtype == SV_BF16, "%s: built for C = 96, 3 heads, bf16 token rows (got C=%d heads=%d dtype=%d)", who,
             C, heads, act_dtype);
  if (int rc = win_geom_check(who, H, W, shift)) return rc;
  const bool side = ln1 || mean || rstd || qkv || att;
  SV_REQUIRE(!side || (ln1 && mean && rstd && qkv && att), "%s: the side outputs (ln1, mean, rstd, qkv, att) come all or none", who);
  SV_REQUIRE((((uintptr_t)x | (uintptr_t)x1 | (uintptr_t)ln1 | (uintptr_t)qkv | (uintptr_t)att | weight_bits) & 15) == 0,
             "%s: tensors must be 16-byte aligned", who);
  a.x = static_cast<const __bf16*>(x); a.ln_g = ln_g; a.ln_b = ln_b; a.bqkv = bqkv; a.table = table; a.bproj = bproj;
  a.row_scale = row_scale; a.x1 = static_cast<__bf16*>(x1); a.ln1 = static_cast<__bf16*>(ln1); a.qkv = static_cast<__bf16*>(qkv);
  a.att = static_cast<__bf16*>(att); a.mean = mean; a.rstd = rstd;
  a.I = I; a.H = H; a.W = W; a.shift = shift; a.eps = eps; a.scale = 1.0f / sqrtf((float)HD);
  a.ntasks = I * (H / 7) * (W / 7);
  a.tasks_per_group = block_share(a.ntasks, false);
  return SV_OK;
}
static inline unsigned block_fwd_grid(const BlockFwdArgs& a) { return (unsigned)cdiv(a.ntasks, 2 * a.tasks_per_group); }

extern "C" int sv_swin_attn_block_fwd(const void* x, const float* ln_g, const float* ln_b, const float* wqkv, const float* bqkv, const float* table,
                                      const float* wproj, const float* bproj, const float* row_scale, void* x1, void* ln1, float* mean,
                                      float* rstd, void* qkv, void* att, int I, int H, int W, int C, int heads, int shift, float eps,
                                      int act_dtype, void* stream) {
  BlockFwdArgs a{};
  if (int rc = block_fwd_args("swin_attn_block_fwd", a, wqkv && wproj, (uintptr_t)wqkv | (uintptr_t)wproj, x, ln_g, ln_b, bqkv, table, bproj, row_scale,
                              x1, ln1, mean, rstd, qkv, att, I, H, W, C, heads, shift, eps, act_dtype))
    return rc;
  a.wqkv = wqkv; a.wproj = wproj;
  hipLaunchKernelGGL(swin_attn_block_fwd_kernel, dim3(block_fwd_grid(a)), dim3(512), 0, (hipStream_t)stream, a);
  return check_launch("sv_swin_attn_block_fwd");
}

// ---- MXFP8 forward of the branch (swin_attn_block_fwd_mx_kernel) ------------------------------------------------------------------------
static inline bool block_mx_supported(int C, int heads) { return C == FB_C && heads == FB_HEADS; }
static std::atomic<long long> swin_attn_block_mx_launches{0};
extern "C" long long sv_swin_attn_block_mx_launches(void) { return swin_attn_block_mx_launches.load(std::memory_order_relaxed); }
extern "C" int sv_swin_attn_block_mx_supported(int C, int heads) { return block_mx_supported(C, heads) ? 1 : 0; }
extern "C" long long sv_swin_attn_block_mx_pack_bytes(int C) { return C == FB_C ? FBM_PACK_BYTES : 0; }

extern "C" int sv_swin_attn_block_mx_pack(const void* wqkv_q, const void* wqkv_s, const void* wproj_q, const void* wproj_s, void* packs, int C,
                                          void* stream) {
  SV_REQUIRE(wqkv_q && wqkv_s && wproj_q && wproj_s && packs, "sv_swin_attn_block_mx_pack: null pointer");
  SV_REQUIRE(C == FB_C, "sv_swin_attn_block_mx_pack: unsupported C=%d (96)", C);
  SV_REQUIRE((((uintptr_t)wqkv_q | (uintptr_t)wproj_q | (uintptr_t)packs) & 15) == 0,
             "sv_swin_attn_block_mx_pack: wqkv_q, wproj_q and packs must be 16-byte aligned");
  hipLaunchKernelGGL(swin_attn_block_mx_pack_kernel, dim3(cdiv(FBM_TILES * 64, 256)), dim3(256), 0, (hipStream_t)stream,
                     static_cast<const uint8_t*>(wqkv_q), static_cast<const uint8_t*>(wqkv_s), static_cast<const uint8_t*>(wproj_q),
                     static_cast<const uint8_t*>(wproj_s), static_cast<uint8_t*>(packs));
  return check_launch("sv_swin_attn_block_mx_pack");
}

extern "C" int sv_swin_attn_block_fwd_mx(const void* x, const float* ln_g, const float* ln_b, const void* packs_mx, const float* bqkv,
                                         const float* table, const float* bproj, const float* row_scale, void* x1, void* ln1, float* mean,
                                         float* rstd, void* qkv, void* att, int I, int H, int W, int C, int heads, int shift, float eps,
                                         int act_dtype, void* stream) {
  BlockFwdMxArgs a{};
  if (int rc = block_fwd_args("sv_swin_attn_block_fwd_mx", a, packs_mx != nullptr, (uintptr_t)packs_mx, x, ln_g, ln_b, bqkv, table, bproj, row_scale,
                              x1, ln1, mean, rstd, qkv, att, I, H, W, C, heads, shift, eps, act_dtype))
    return rc;
  a.packs = static_cast<const uint8_t*>(packs_mx);
  hipLaunchKernelGGL(swin_attn_block_fwd_mx_kernel, dim3(block_fwd_grid(a)), dim3(512), 0, (hipStream_t)stream, a);
  const int rc = check_launch("sv_swin_attn_block_fwd_mx");
  if (rc == SV_OK) swin_attn_block_mx_launches.fetch_add(1, std::memory_order_relaxed);
  return rc;
}

extern "C" int sv_swin_attn_block_windows_per_group(int I, int H, int W, int backward) {
  SV_REQUIRE(I > 0, "swin_attn_block_windows_per_group: I (%d) must be positive", I);
  if (int rc = win_geom_check("swin_attn_block_windows_per_group", H, W, 0)) return rc;
  return block_share(I * (H / 7) * (W / 7), backward != 0);
}

/* Fused backward of the attention branch of a stage-0 block (see swin_attn_block_bwd_kernel).  dgamma / dbeta / dtable are accumulated into;
 * workspace = sv_window_attention_bwd_workspace_floats(heads) floats, zero on entry. */
extern "C" int sv_swin_attn_block_bwd(const void* dx1, const void* qkv, const void* x, const float* mean, const float* rstd, const float* ln_g,
                                      const float* wqkv, const float* wproj, const float* table, const float* row_scale, void* dqkv, void* dx,
                                      void* dbr, float* dgamma, float* dbeta, float* dtable, float* workspace, int I, int H, int W, int C,
                                      int heads, int shift, int act_dtype, void* stream) {
  SV_REQUIRE(dx1 && qkv && x && mean && rstd && ln_g && wqkv && wproj && table && dqkv && dx && dgamma && dbeta && dtable && workspace && I > 0,
             "swin_attn_block_bwd: null/empty argument");
  SV_REQUIRE(C == FB_C && heads == FB_HEADS && act_dtype == SV_BF16, "swin_attn_block_bwd: built for C = 96, 3 heads, bf16 token rows (got C=%d heads=%d dtype=%d)",
             C, heads, act_dtype);
  if (int rc = win_geom_check("swin_attn_block_bwd", H, W, shift)) return rc;
  SV_REQUIRE((((uintptr_t)dx1 | (uintptr_t)qkv | (uintptr_t)x | (uintptr_t)dqkv | (uintptr_t)dx | (uintptr_t)dbr) & 15) == 0,
             "swin_attn_block_bwd: tensors must be 16-byte aligned");
  BlockBwdArgs a{};
  a.dx1 = static_cast<const __bf16*>(dx1); a.qkv = static_cast<const __bf16*>(qkv); a.x = static_cast<const __bf16*>(x);
  a.mean = mean; a.rstd = rstd; a.ln_g = ln_g; a.wqkv = wqkv; a.wproj = wproj; a.table = table; a.row_scale = row_scale;
  a.dqkv = static_cast<__bf16*>(dqkv); a.dx = static_cast<__bf16*>(dx); a.dbr = static_cast<__bf16*>(dbr);
  a.dgamma = dgamma; a.dbeta = dbeta; a.dt_ws = workspace;
  a.I = I; a.H = H; a.W = W; a.shift = shift; a.scale = 1.0f / sqrtf((float)HD);
  a.ntasks = I * (H / 7) * (W / 7);
  a.tasks_per_group = block_share(a.ntasks, true);
  const int nblocks = cdiv(a.ntasks, a.tasks_per_group);
  hipLaunchKernelGGL(swin_attn_block_bwd_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, a);
  launch_dtable_fold(workspace, dtable, heads, (hipStream_t)stream);
  return check_launch("sv_swin_attn_block_bwd");
}
