// Which lane's scale byte does v_mfma_scale_f32_16x16x128_f8f6f4 apply to which (row, 32-wide k-block)?  One wave, e4m3 operands of ones.
// For every "hot" lane h and lane group g: the probed operand holds ones only in the lanes of group g (k-block g under the data map
// "lane l holds row l & 15, k = 32 (l >> 4) .. + 31"), the other operand is all ones, every scale is 1.0 except lane h's, which is 2.0.
// D is 32 everywhere except where lane h's scale reached the block: 64.  Prints, per hot lane, the (group, row) it scaled; side A = first
// operand (rows of D), side B = second operand (columns of D), and side A again with the scale in byte 1 of the register and op-sel 1.
//   hipcc --offload-arch=gfx950 -O2 mfma_scale_lane_probe.hip -o mfma_scale_lane_probe && ./mfma_scale_lane_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ void probe(float* out) {
  const int lane = threadIdx.x, lr = lane & 15, lg = lane >> 4;
  const int one = 0x38383838;                              // four e4m3 1.0
  const i32x8 ones = {one, one, one, one, one, one, one, one}, zeros = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int side = 0; side < 3; ++side)
    for (int h = 0; h < 64; ++h)
      for (int g = 0; g < 4; ++g) {
        const i32x8 hot = lg == g ? ones : zeros;
        const int s = lane == h ? 128 : 127;
        f32x4 d = {0.f, 0.f, 0.f, 0.f};
        if (side == 0) d = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(hot, ones, d, 0, 0, 0, s, 0, 0x7f7f7f7f);
        else if (side == 1) d = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(ones, hot, d, 0, 0, 0, 0x7f7f7f7f, 0, s);
        else d = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(hot, ones, d, 0, 0, 1, (s << 8) | 0x78780078, 0, 0x7f7f7f7f);
        float* o = out + (size_t)((side * 64 + h) * 4 + g) * 256;
        for (int r = 0; r < 4; ++r) o[(4 * lg + r) * 16 + lr] = d[r];   // C/D map: row 4 (lane >> 4) + r, column lane & 15
      }
}

int main() {
  const size_t n = 3 * 64 * 4 * 256;
  float* d;
  if (hipMalloc(&d, n * sizeof(float)) != hipSuccess) { printf("hipMalloc failed\n"); return 1; }
  hipMemset(d, 0, n * sizeof(float));
  hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, d);
  std::vector<float> h(n);
  if (hipMemcpy(h.data(), d, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) { printf("kernel or copy failed\n"); return 1; }
  const char* names[3] = {"A (byte 0, op-sel 0)", "B (byte 0, op-sel 0)", "A (byte 1, op-sel 1)"};
  for (int side = 0; side < 3; ++side) {
    printf("side %s: hot lane -> (lane group of the data, row%s) it scaled\n", names[side], side == 1 ? " = column of D" : "");
    int expected = 0;
    for (int hl = 0; hl < 64; ++hl) {
      printf("  lane %2d:", hl);
      for (int g = 0; g < 4; ++g) {
        const float* o = h.data() + (size_t)((side * 64 + hl) * 4 + g) * 256;
        for (int i = 0; i < 16; ++i) {
          const float v = side == 1 ? o[i] : o[i * 16];                      // row 0 along the columns / column 0 along the rows
          if (v != 32.f) { printf(" (g %d, %2d: %g)", g, i, v); expected += (g == (hl >> 4) && i == (hl & 15) && v == 64.f); }
        }
      }
      printf("\n");
    }
    printf("  lanes that scale exactly their own (l >> 4, l & 15): %d of 64\n", expected);
  }
  hipFree(d);
  return 0;
}
