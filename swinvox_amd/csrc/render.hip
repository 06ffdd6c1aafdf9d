// Volume views on the device: the picture the reference's evaluation loop draws of every reconstruction (utils/helpers.py:50-88,
// get_volume_views -> Axes3D.voxels at elev 30 / azim 45, called from core/test.py:178-187; utils/binvox_rw.py:306-343 draws it
// orthographically) as a ray-cast through the volume's bit mask.  The rule is written out in include/swinvox_hip.h (sv_render_volumes)
// and restated in numpy in tests/volume_view_ref.py; the arithmetic below follows it operation for operation, so the ids are meant to be
// equal, not close.
//
//   pack      occupancy (the voxel_set predicate of the other exports) -> one or two 32-bit words per (i, j) row, by ballot
//   ray-cast  16 x 16-pixel tiles x cameras x volumes; slab test, then Amanatides-Woo stepping against the mask in LDS -> one id per pixel
//   shade     ids -> uint8 planes: edge / face / background colours, an integer rule on the ids
#include <cmath>
#include "common.h"

namespace sv {

// ---- pack: a wave owns 64 consecutive lanes of padded rows - two rows of <= 32 voxels or one row of <= 64 ------------------------------
__global__ void __launch_bounds__(256) render_pack_kernel(const void* __restrict__ vol, int dtype, long long rows, int d2, int nw, float th,
                                                          unsigned int* __restrict__ mask) {
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long long row = nw == 1 ? wave * 2 + (lane >> 5) : wave;              // wave-uniform trip: every lane takes part in the ballot
  const int k = nw == 1 ? (lane & 31) : lane;
  const bool in = row < rows && k < d2;
  const unsigned long long m = __ballot(in && voxel_set(vol, dtype, in ? (size_t)row * d2 + k : 0, th));
  if (lane == 0) {
    if (nw == 1) {
      if (wave * 2 < rows) mask[wave * 2] = (unsigned int)m;
      if (wave * 2 + 1 < rows) mask[wave * 2 + 1] = (unsigned int)(m >> 32);
    } else if (wave < rows) {
      mask[wave * 2] = (unsigned int)m;
      mask[wave * 2 + 1] = (unsigned int)(m >> 32);
    }
  }
}

// ---- ray-cast --------------------------------------------------------------------------------------------------------------------------
// One step at a time in fp32, as the numpy restatement takes them: no contraction into fma, IEEE division (hipcc's default for fp32), no
// reciprocal approximations.
#pragma clang fp contract(off)

struct RayAxis {
  float o, d, tnear, tfar;
};

__device__ __forceinline__ RayAxis ray_axis(const float* __restrict__ c, int a, float px, float py, int D) {
  RayAxis r;
  r.o = (c[a] + px * c[3 + a]) + py * c[6 + a];                               // o0 + (col + 0.5) ox + (row + 0.5) oy
  r.d = (c[9 + a] + px * c[12 + a]) + py * c[15 + a];
  if (r.d != 0.f) {
    const float t0 = (0.f - r.o) / r.d, t1 = ((float)D - r.o) / r.d;
    r.tnear = fminf(t0, t1);
    r.tfar = fmaxf(t0, t1);
  } else {
    const bool inside = r.o >= 0.f && r.o < (float)D;
    r.tnear = inside ? -INFINITY : INFINITY;
    r.tfar = inside ? INFINITY : -INFINITY;
  }
  return r;
}

template <int LDSW>
__global__ void __launch_bounds__(256) render_cast_kernel(const unsigned int* __restrict__ mask, const sv_view_camera* __restrict__ cams, int d0,
                                                          int d1, int d2, int nw, int H, int W, int tiles_x, int* __restrict__ ids) {
  __shared__ unsigned int occ[LDSW];
  const int tid = threadIdx.x, cam = blockIdx.y, b = blockIdx.z;
  const int col = (blockIdx.x % tiles_x) * 16 + (tid & 15), row = (blockIdx.x / tiles_x) * 16 + (tid >> 4);
  const bool in_image = col < W && row < H;
  const float* c = reinterpret_cast<const float*>(cams + cam);
  const float px = (float)col + 0.5f, py = (float)row + 0.5f;
  const int D[3] = {d0, d1, d2};
  RayAxis ax[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) ax[a] = ray_axis(c, a, px, py, D[a]);
  int e = 0;                                                                  // first arg-max of tnear: x before y before z
  float tin = ax[0].tnear;
  if (ax[1].tnear > tin) { tin = ax[1].tnear; e = 1; }
  if (ax[2].tnear > tin) { tin = ax[2].tnear; e = 2; }
  const float tout = fminf(fminf(ax[0].tfar, ax[1].tfar), ax[2].tfar);
  const bool hit = in_image && tin < tout && tin > 0.f;
  int* out = ids + (((size_t)b * gridDim.y + cam) * H + (in_image ? row : 0)) * (size_t)W + (in_image ? col : 0);
  if (!__syncthreads_or(hit)) {                                               // no ray of the tile reaches the box: the mask is not touched
    if (in_image) *out = -1;
    return;
  }
  const int words = d0 * d1 * nw;                                             // <= LDSW: the host picks the instance
  const unsigned int* m = mask + (size_t)b * words;
  for (int i = tid; i < words && i < LDSW; i += 256) occ[i] = m[i];
  __syncthreads();
  int id = -1;
  if (hit) {
    int cell[3], step[3];
    float tmax[3], tdelta[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float p = ax[a].o + ax[a].d * tin;
      const bool pos = ax[a].d > 0.f;
      int cc = (int)fminf(fmaxf(floorf(p), 0.f), (float)(D[a] - 1));
      if (a == e) cc = pos ? 0 : D[a] - 1;
      cell[a] = cc;
      if (ax[a].d != 0.f) {
        step[a] = pos ? 1 : -1;
        tmax[a] = ((float)(cc + (pos ? 1 : 0)) - ax[a].o) / ax[a].d;
        tdelta[a] = fabsf(1.f / ax[a].d);
      } else {
        step[a] = 0;
        tmax[a] = INFINITY;
        tdelta[a] = INFINITY;
      }
    }
    int face = 2 * e + (step[e] < 0 ? 1 : 0);
    for (int it = 0; it < d0 + d1 + d2; ++it) {                               // a ray crosses fewer cells than that
      const int w = (cell[0] * d1 + cell[1]) * nw + (cell[2] >> 5);           // cells stay inside the grid, so w < words
      if ((occ[w] >> (cell[2] & 31)) & 1u) {
        id = ((cell[0] * d1 + cell[1]) * d2 + cell[2]) * 6 + face;
        break;
      }
      int a = 0;                                                              // first arg-min of tmax
      float tm = tmax[0];
      if (tmax[1] < tm) { tm = tmax[1]; a = 1; }
      if (tmax[2] < tm) { a = 2; }
      int nc, lim, st;
      if (a == 0) { nc = cell[0] += step[0]; tmax[0] += tdelta[0]; lim = d0; st = step[0]; }
      else if (a == 1) { nc = cell[1] += step[1]; tmax[1] += tdelta[1]; lim = d1; st = step[1]; }
      else { nc = cell[2] += step[2]; tmax[2] += tdelta[2]; lim = d2; st = step[2]; }
      if (nc < 0 || nc >= lim || st == 0) break;
      face = 2 * a + (st < 0 ? 1 : 0);
    }
  }
  if (in_image) *out = id;
}

// ---- shade: an integer rule on the ids (no floating point) -----------------------------------------------------------------------------------------------------
struct ShadeColours {
  unsigned char face[18], edge[3], bg[3];
};

__global__ void __launch_bounds__(256) render_shade_kernel(const int* __restrict__ ids, int H, int W, ShadeColours col,
                                                           const unsigned char* __restrict__ plate, unsigned char* __restrict__ rgb) {
  const int p = blockIdx.x * 256 + threadIdx.x, hw = H * W;
  if (p >= hw) return;
  const size_t img = (size_t)blockIdx.z * gridDim.y + blockIdx.y;
  const int* im = ids + img * hw;
  const int y = p / W, x = p - y * W;
  const int id = im[p], right = x + 1 < W ? im[p + 1] : id, below = y + 1 < H ? im[p + W] : id;
  unsigned char* o = rgb + img * 3 * (size_t)hw + p;
  const bool edge = id != right || id != below;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    unsigned char v;
    if (edge) v = col.edge[ch];
    else if (id >= 0) v = col.face[(id % 6) * 3 + ch];
    else v = plate ? plate[(size_t)ch * hw + p] : col.bg[ch];
    o[(size_t)ch * hw] = v;
  }
}

}  // namespace sv

using namespace sv;
#define STREAM static_cast<hipStream_t>(stream)

extern "C" int sv_render_volumes(const void* vol, int dtype, int B, int d0, int d1, int d2, float threshold, const sv_view_camera* cams_host,
                                 int n_cams, sv_view_camera* cams_dev_ws, int H, int W, const unsigned char* face_rgb,
                                 const unsigned char* edge_rgb, const unsigned char* background_rgb, const unsigned char* plate_dev,
                                 unsigned int* mask_ws, int* ids, unsigned char* rgb, void* stream) {
  SV_REQUIRE(vol && cams_host && cams_dev_ws && face_rgb && edge_rgb && background_rgb && mask_ws && ids, "sv_render_volumes: bad arguments");
  SV_REQUIRE(B >= 1 && B <= 65535 && n_cams >= 1 && n_cams <= 65535, "sv_render_volumes: %d volumes x %d cameras (1 .. 65535 each)", B, n_cams);
  SV_REQUIRE(d0 >= 1 && d0 <= 64 && d1 >= 1 && d1 <= 64 && d2 >= 1 && d2 <= 64, "sv_render_volumes: dims %d x %d x %d, every dim must lie in 1 .. 64",
             d0, d1, d2);
  SV_REQUIRE(H >= 1 && W >= 1 && (long long)H * W <= (1ll << 24), "sv_render_volumes: image %d x %d (at least 1 x 1, at most 2^24 pixels)", H, W);
  SV_REQUIRE(dtype == 0 || dtype == 1, "sv_render_volumes: dtype %d is neither 0 (float32) nor 1 (uint8)", dtype);
  SV_REQUIRE(threshold < 0.f || (threshold > 0.f && threshold < 1.f), "sv_render_volumes: threshold must be negative (occupancy input) or in (0, 1)");
  SV_REQUIRE(threshold < 0.f || dtype == 0, "sv_render_volumes: a sigmoid threshold needs float32 logits");
  const float dims[3] = {(float)d0, (float)d1, (float)d2};
  for (int c = 0; c < n_cams; ++c) {                                          // every camera, on the host, before anything is launched
    const float* f = reinterpret_cast<const float*>(cams_host + c);
    bool persp = true, on_box = true;
    for (int i = 0; i < 18; ++i) SV_REQUIRE(std::isfinite(f[i]),"sv_render_volumes: camera %d holds a number that is not finite", c);
    for (int i = 3; i < 9; ++i) persp = persp && f[i] == 0.f;                 // ox = oy = 0: one eye for all rays
    for (int a = 0; a < 3; ++a) on_box = on_box && f[a] >= 0.f && f[a] <= dims[a];
    SV_REQUIRE(!(persp && on_box), "sv_render_volumes: the eye of camera %d (%g, %g, %g) lies inside or on the volume's box", c, f[0], f[1], f[2]);
  }
  const int nw = d2 <= 32 ? 1 : 2;
  const long long rows = (long long)B * d0 * d1;
  // pageable host memory: the copy has read cams_host when the call returns
  hipError_t err = hipMemcpyAsync(cams_dev_ws, cams_host, sizeof(sv_view_camera) * (size_t)n_cams, hipMemcpyHostToDevice, STREAM);
  if (err != hipSuccess) { set_error("sv_render_volumes: camera copy failed: %s", hipGetErrorString(err)); return SV_ERR_LAUNCH; }
  hipLaunchKernelGGL(render_pack_kernel, dim3(cdiv(nw == 1 ? (rows + 1) / 2 : rows, 4)), dim3(256), 0, STREAM, vol, dtype, rows, d2, nw, threshold,
                     mask_ws);
  const int tiles_x = cdiv(W, 16), tiles_y = cdiv(H, 16);
  const dim3 grid(tiles_x * tiles_y, n_cams, B);
  if (d0 * d1 * nw <= 1024)
    hipLaunchKernelGGL(render_cast_kernel<1024>, grid, dim3(256), 0, STREAM, mask_ws, cams_dev_ws, d0, d1, d2, nw, H, W, tiles_x, ids);
  else
    hipLaunchKernelGGL(render_cast_kernel<8192>, grid, dim3(256), 0, STREAM, mask_ws, cams_dev_ws, d0, d1, d2, nw, H, W, tiles_x, ids);
  if (rgb) {
    ShadeColours col;
    for (int i = 0; i < 18; ++i) col.face[i] = face_rgb[i];
    for (int i = 0; i < 3; ++i) { col.edge[i] = edge_rgb[i]; col.bg[i] = background_rgb[i]; }
    hipLaunchKernelGGL(render_shade_kernel, dim3(cdiv((long long)H * W, 256), n_cams, B), dim3(256), 0, STREAM, ids, H, W, col, plate_dev, rgb);
  }
  return check_launch("sv_render_volumes");
}
