// Halo-tile convolution (conv_halo.hip): the interface igemm.hip dispatches through.  Internal header - not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

namespace sv {

struct HaloConvArgs {
  const void* x;      // [N][H][W][CI] bf16, rows of exactly CI elements
  const void* w;      // packed weights [64][taps][CI] bf16 (forward pack, or the data-gradient pack with flip = 1)
  void* y;            // [N][H][W][64] bf16, rows of exactly 64 elements
  double* stats;      // optional [SV_BN_SLOTS][2 * 64]: per-channel sum / sum of squares of the stored (bf16-rounded) results
  int N, H, W;
  int flip;           // 1: tap t of the pack is applied at the mirrored offset (data gradient of a stride-1 convolution)
};

// Which halo-tile kernel a call gets, and its launch geometry.  The *_plan functions are pure host functions of the shape and of the current
// halo mode (sv_set_conv_halo / sv_set_conv_halo_wgrad) - every shape condition of the halo route lives in them; the launch functions take a
// finished plan and decide nothing.  The engine's plans (igemm.hip) call them.
struct HaloPlan {     // HaloPlan{} = not taken
  int kind = -1;      // -1: not taken (the caller goes on with the engine); 0, 1, 2: resident-weights kernels (below); 3: blocked; 4: weight gradient
  int th = 0, tw = 0; // output positions of a tile
  int stride = 0;     // weight gradient: 1 or 2
  int tiles_h = 0, tiles_w = 0;
  int nitems = 0;     // tiles (kind 3: tiles x blocks of 64 output channels) the launch hands out
  int nsplit = 0;     // weight gradient: position splits per (co, ci) block
  int grid = 0;       // workgroups of 256 threads
};
// kind: 0 = 3 x 3, padding 1, CI = 64;  1 = 4 x 4, padding (2, 1), CI = 16 (the ResNet stem on the space-to-depth image);
//       2 = kind 1's data gradient: x = dy [N][H][W][64], w = its data-gradient pack [16][16 taps][64], y = [N][H][W][16] (flip = 1)
HaloPlan conv_halo_plan(int kind, int N, int H, int W);
// the same convolution (3 x 3 / stride 1 / padding 1, plain store + optional statistics) with Ci, Co multiples of 64 up to 512: work items of 256
// positions x 64 output channels with a K loop over blocks of 64 input channels; w = the [Co][9][Ci] pack (data-gradient pack with flip = 1)
HaloPlan conv_halo_blocked_plan(int N, int H, int W, int Ci, int Co);
// 3 x 3 / padding 1 / stride 1 or 2 weight gradient (Ci, Co multiples of 64, rows of exactly Ci / Co elements)
HaloPlan conv_halo_wgrad_plan(int N, int H, int W, int Ho, int Wo, int stride, int Ci, int Co);
bool conv_halo_enabled();

// launches of a taken plan on `stream`; ctr = a slot of tile_draw_counters()
void conv_halo_launch(const HaloConvArgs& a, const HaloPlan& p, int* ctr, hipStream_t stream);
void conv_halo_blocked_launch(const void* x, const void* w, void* y, double* stats, int N, int H, int W, int Ci, int Co, int flip, const HaloPlan& p,
                              int* ctr, hipStream_t stream);
// into the packed workspace ws [Co][9][Ci] fp32 (zero on entry), dbias (optional) += column sums of dy
void conv_halo_wgrad_launch(const void* x, const void* dy, float* ws, float* dbias, int N, int H, int W, int Ho, int Wo, int Ci, int Co, const HaloPlan& p,
                            hipStream_t stream);

// launch slot of the run-time tile schedulers (igemm.hip): 16 ints, zero on entry, zeroed again by the launch's last workgroup
int* tile_draw_counters();

}  // namespace sv
