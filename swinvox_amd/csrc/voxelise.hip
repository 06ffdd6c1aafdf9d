// Mesh voxelisation on the device: triangle meshes -> occupancy volumes, the step the reference leaves to the external `binvox` program
// (utils/binvox_converter.py and the notebook's convert_obj_to_binvox shell out to it).  The rule is written out in include/swinvox_hip.h
// (sv_voxelise_meshes) and restated in numpy in tests/mesh_voxel_ref.py.  Every decision below is made in integers on coordinates snapped to
// 1 / 1024 of a voxel: there is no floating point in this file, so the volumes are meant to be equal to the restatement, not close.
//
//   accumulate  grid (triangle chunks, meshes); a workgroup keeps two bit masks of the volume in LDS (bits along z, one or two 32-bit words
//               per (i, j) row - render.hip's layout): `solid` collects parity toggles with atomicXor, `surface` cube hits with atomicOr;
//               both are then merged into the mesh's masks in the workspace with global atomicXor / atomicOr.  XOR and OR commute, so
//               neither the triangle order nor the split into chunks shows in the result.
//   expand      surface | solid -> float32 or uint8 [B][d0][d1][d2]
#include "common.h"

namespace sv {

constexpr int VOX_S = 1024, VOX_H = 512;        // units per voxel; a voxel centre is an odd multiple of VOX_H
constexpr int VOX_NT = 256;
constexpr int VOX_CHUNK = 1024;                 // triangles per workgroup: four per thread
// A triangle whose clipped bounding box holds more candidate voxels (surface) or columns (solid) than this leaves the one-per-thread
// pass for the workgroup's LDS list and is then worked on by all 256 threads: one triangle across a 64^3 grid is 262 144 candidates.
constexpr int VOX_COOP_CANDIDATES = 256;

__device__ __forceinline__ int floor_div_s(int x) { return (x >= 0 ? x : x - (VOX_S - 1)) / VOX_S; }
__device__ __forceinline__ int ceil_div_s(int x) { return -floor_div_s(-x); }
__device__ __forceinline__ long long floor_div64(long long x, long long y) {   // y > 0
  long long q = x / y;
  if (x % y != 0 && x < 0) --q;
  return q;
}
__device__ __forceinline__ long long abs64(long long x) { return x < 0 ? -x : x; }
__device__ __forceinline__ int min3(int a, int b, int c) { return min(a, min(b, c)); }
__device__ __forceinline__ int max3(int a, int b, int c) { return max(a, max(b, c)); }

struct VoxTri {
  int a[3], b[3], c[3];
  long long n[3];                                // (b - a) x (c - a): components below 2^37
};

// 0: loaded; 1: an index outside the mesh's vertices (nothing was dereferenced); 2: zero normal
__device__ __forceinline__ int vox_load_tri(const int* __restrict__ verts, const int* __restrict__ tris, long long n_verts, long long t, VoxTri& T) {
  const int* ix = tris + 3 * t;
  const int i0 = ix[0], i1 = ix[1], i2 = ix[2];
  if (i0 < 0 || i0 >= n_verts || i1 < 0 || i1 >= n_verts || i2 < 0 || i2 >= n_verts) return 1;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    T.a[q] = verts[3 * (long long)i0 + q];
    T.b[q] = verts[3 * (long long)i1 + q];
    T.c[q] = verts[3 * (long long)i2 + q];
  }
  const long long e1x = T.b[0] - T.a[0], e1y = T.b[1] - T.a[1], e1z = T.b[2] - T.a[2];
  const long long e2x = T.c[0] - T.a[0], e2y = T.c[1] - T.a[1], e2z = T.c[2] - T.a[2];
  T.n[0] = e1y * e2z - e1z * e2y;
  T.n[1] = e1z * e2x - e1x * e2z;
  T.n[2] = e1x * e2y - e1y * e2x;                // = A2 of the solid rule
  return (T.n[0] | T.n[1] | T.n[2]) == 0 ? 2 : 0;
}

// ---- solid: parity along z ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool vox_edge_inside(int ux, int uy, int vx, int vy, int Px, int Py) {
  const int dx = vx - ux, dy = vy - uy;
  const long long E = (long long)dx * (Py - uy) - (long long)dy * (Px - ux);
  return E > 0 || (E == 0 && (dy < 0 || (dy == 0 && dx < 0)));
}

__device__ __forceinline__ bool vox_column_covered(const VoxTri& T, int Px, int Py) {
  const bool flip = T.n[2] < 0;                  // counter-clockwise in the xy projection for the edge tests
  const int bx = flip ? T.c[0] : T.b[0], by = flip ? T.c[1] : T.b[1], cx = flip ? T.b[0] : T.c[0], cy = flip ? T.b[1] : T.c[1];
  return vox_edge_inside(T.a[0], T.a[1], bx, by, Px, Py) && vox_edge_inside(bx, by, cx, cy, Px, Py) && vox_edge_inside(cx, cy, T.a[0], T.a[1], Px, Py);
}

// first k in 0 .. d2 whose centre lies strictly above the triangle's crossing of the column: with s = sgn(n.z),
// s (n.x (Px - a.x) + n.y (Py - a.y) + n.z ((2k + 1) H - a.z)) > 0  <=>  k > (R - H |n.z|) / (S |n.z|),  R = |n.z| a.z - s (n.x (Px - a.x) + n.y (Py - a.y))
__device__ __forceinline__ int vox_first_toggled(const VoxTri& T, int Px, int Py, int d2) {
  const long long anz = abs64(T.n[2]);
  const long long lat = T.n[0] * (Px - T.a[0]) + T.n[1] * (Py - T.a[1]);
  const long long R = anz * T.a[2] - (T.n[2] > 0 ? lat : -lat);
  const long long k = floor_div64(R - VOX_H * anz, VOX_S * anz) + 1;
  return (int)(k < 0 ? 0 : (k > d2 ? d2 : k));
}

__device__ __forceinline__ void vox_solid_column(unsigned int* sol, const VoxTri& T, int i, int j, int d1, int d2, int nw) {
  const int Px = (2 * i + 1) * VOX_H, Py = (2 * j + 1) * VOX_H;
  if (!vox_column_covered(T, Px, Py)) return;
  const int k0 = vox_first_toggled(T, Px, Py, d2);
  if (k0 >= d2) return;                          // k0 <= 63 below
  const unsigned long long bits = (~0ull << k0) & (d2 == 64 ? ~0ull : ((1ull << d2) - 1ull));
  unsigned int* row = sol + (i * d1 + j) * nw;   // i < d0, j < d1: inside the d0 * d1 * nw words of the mask
  if ((unsigned int)bits) atomicXor(row, (unsigned int)bits);
  if (nw == 2 && (unsigned int)(bits >> 32)) atomicXor(row + 1, (unsigned int)(bits >> 32));
}

// ---- surface: closed cube against closed triangle, 13 separating axes --------------------------------------------------------------------
// One of the nine axes e_i x f: q0 .. q2 are the projections of the translated vertices, r the cube's radius along the axis.
__device__ __forceinline__ bool vox_axis_separates(long long q0, long long q1, long long q2, long long r) {
  const long long lo = q0 < q1 ? (q0 < q2 ? q0 : q2) : (q1 < q2 ? q1 : q2);
  const long long hi = q0 > q1 ? (q0 > q2 ? q0 : q2) : (q1 > q2 ? q1 : q2);
  return lo > r || hi < -r;
}

__device__ __forceinline__ bool vox_tri_cube(const VoxTri& T, int i, int j, int k) {
  const int cx = (2 * i + 1) * VOX_H, cy = (2 * j + 1) * VOX_H, cz = (2 * k + 1) * VOX_H;
  long long p[3][3];                             // vertices relative to the cube's centre
  p[0][0] = T.a[0] - cx; p[0][1] = T.a[1] - cy; p[0][2] = T.a[2] - cz;
  p[1][0] = T.b[0] - cx; p[1][1] = T.b[1] - cy; p[1][2] = T.b[2] - cz;
  p[2][0] = T.c[0] - cx; p[2][1] = T.c[1] - cy; p[2][2] = T.c[2] - cz;
#pragma unroll
  for (int q = 0; q < 3; ++q)                    // the cube's three face normals
    if (vox_axis_separates(p[0][q], p[1][q], p[2][q], VOX_H)) return false;
  const long long dn = T.n[0] * p[0][0] + T.n[1] * p[0][1] + T.n[2] * p[0][2];   // the triangle's normal: all three vertices project alike
  const long long rn = VOX_H * (abs64(T.n[0]) + abs64(T.n[1]) + abs64(T.n[2]));
  if (dn > rn || dn < -rn) return false;
#pragma unroll
  for (int e = 0; e < 3; ++e) {                  // e_x x f = (0, -f.z, f.y), e_y x f = (f.z, 0, -f.x), e_z x f = (-f.y, f.x, 0)
    const int e1 = (e + 1) % 3;
    const long long fx = p[e1][0] - p[e][0], fy = p[e1][1] - p[e][1], fz = p[e1][2] - p[e][2];
    if (vox_axis_separates(fy * p[0][2] - fz * p[0][1], fy * p[1][2] - fz * p[1][1], fy * p[2][2] - fz * p[2][1], VOX_H * (abs64(fy) + abs64(fz)))) return false;
    if (vox_axis_separates(fz * p[0][0] - fx * p[0][2], fz * p[1][0] - fx * p[1][2], fz * p[2][0] - fx * p[2][2], VOX_H * (abs64(fz) + abs64(fx)))) return false;
    if (vox_axis_separates(fx * p[0][1] - fy * p[0][0], fx * p[1][1] - fy * p[1][0], fx * p[2][1] - fy * p[2][0], VOX_H * (abs64(fx) + abs64(fy)))) return false;
  }
  return true;
}

__device__ __forceinline__ void vox_surface_row(unsigned int* srf, const VoxTri& T, int i, int j, int k_lo, int k_hi, int d1, int nw) {
  unsigned long long bits = 0ull;
  for (int k = k_lo; k <= k_hi; ++k)             // 0 <= k_lo, k_hi <= d2 - 1 <= 63
    if (vox_tri_cube(T, i, j, k)) bits |= 1ull << k;
  unsigned int* row = srf + (i * d1 + j) * nw;
  if ((unsigned int)bits) atomicOr(row, (unsigned int)bits);
  if (nw == 2 && (unsigned int)(bits >> 32)) atomicOr(row + 1, (unsigned int)(bits >> 32));
}

// inclusive index ranges of a triangle's bounding box, clipped to the grid (empty when hi < lo)
struct VoxRange {
  int lo[3], hi[3];
  __device__ __forceinline__ int extent(int q) const { return hi[q] >= lo[q] ? hi[q] - lo[q] + 1 : 0; }
};
// columns whose centre (2i + 1) H lies inside [min, max] of x and y
__device__ __forceinline__ VoxRange vox_column_range(const VoxTri& T, int d0, int d1) {
  VoxRange r;
  const int D[2] = {d0, d1};
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    r.lo[q] = max(0, ceil_div_s(min3(T.a[q], T.b[q], T.c[q]) - VOX_H));
    r.hi[q] = min(D[q] - 1, floor_div_s(max3(T.a[q], T.b[q], T.c[q]) - VOX_H));
  }
  r.lo[2] = r.hi[2] = 0;
  return r;
}
// voxels whose closed cube [iS, (i + 1) S] meets [min, max] on every axis
__device__ __forceinline__ VoxRange vox_voxel_range(const VoxTri& T, int d0, int d1, int d2) {
  VoxRange r;
  const int D[3] = {d0, d1, d2};
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    r.lo[q] = max(0, ceil_div_s(min3(T.a[q], T.b[q], T.c[q])) - 1);
    r.hi[q] = min(D[q] - 1, floor_div_s(max3(T.a[q], T.b[q], T.c[q])));
  }
  return r;
}

template <int LDSW>
__global__ void __launch_bounds__(VOX_NT) voxelise_accumulate_kernel(const int* __restrict__ verts, const int* __restrict__ tris,
                                                                     const long long* __restrict__ table, int d0, int d1, int d2, int nw, int mode,
                                                                     unsigned int* __restrict__ masks, int* __restrict__ bad) {
  __shared__ unsigned int sol[LDSW], srf[LDSW];
  __shared__ unsigned short coop[VOX_CHUNK];
  __shared__ int n_coop;
  const int tid = threadIdx.x, b = blockIdx.y;
  const long long v_off = table[4 * b], n_verts = table[4 * b + 1], t_off = table[4 * b + 2], n_tris = table[4 * b + 3];
  const long long first = (long long)blockIdx.x * VOX_CHUNK;
  if (first >= n_tris) return;                   // the whole workgroup: the grid is sized for the largest mesh of the batch
  const int words = d0 * d1 * nw;                // <= LDSW: the host picks the instance
  for (int w = tid; w < words && w < LDSW; w += VOX_NT) { sol[w] = 0u; srf[w] = 0u; }
  if (tid == 0) n_coop = 0;
  __syncthreads();
  const int* mv = verts + 3 * v_off;
  const int* mt = tris + 3 * t_off;
  const int count = (int)(n_tris - first < VOX_CHUNK ? n_tris - first : VOX_CHUNK);
  const bool do_solid = mode != SV_VOXELISE_SURFACE, do_surface = mode != SV_VOXELISE_SOLID;
  int n_bad = 0;
  for (int l = tid; l < count; l += VOX_NT) {    // one triangle per thread
    VoxTri T;
    const int st = vox_load_tri(mv, mt, n_verts, first + l, T);
    if (st == 1) ++n_bad;
    if (st != 0) continue;
    const bool solid = do_solid && T.n[2] != 0;
    const VoxRange cr = vox_column_range(T, d0, d1), vr = vox_voxel_range(T, d0, d1, d2);
    const int cols = solid ? cr.extent(0) * cr.extent(1) : 0;
    const int vox = do_surface ? vr.extent(0) * vr.extent(1) * vr.extent(2) : 0;
    if (cols > VOX_COOP_CANDIDATES || vox > VOX_COOP_CANDIDATES) {
      coop[atomicAdd(&n_coop, 1)] = (unsigned short)l;   // at most `count` <= VOX_CHUNK entries
      continue;
    }
    if (cols > 0)
      for (int i = cr.lo[0]; i <= cr.hi[0]; ++i)
        for (int j = cr.lo[1]; j <= cr.hi[1]; ++j) vox_solid_column(sol, T, i, j, d1, d2, nw);
    if (vox > 0)
      for (int i = vr.lo[0]; i <= vr.hi[0]; ++i)
        for (int j = vr.lo[1]; j <= vr.hi[1]; ++j) vox_surface_row(srf, T, i, j, vr.lo[2], vr.hi[2], d1, nw);
  }
  if (n_bad) atomicAdd(bad + b, n_bad);
  __syncthreads();
  const int nc = n_coop;
  for (int e = 0; e < nc; ++e) {                 // the large triangles, each by the whole workgroup
    VoxTri T;
    vox_load_tri(mv, mt, n_verts, first + coop[e], T);   // passed both checks above
    if (do_solid && T.n[2] != 0) {
      const VoxRange cr = vox_column_range(T, d0, d1);
      const int nj = cr.extent(1), cols = cr.extent(0) * nj;
      for (int c = tid; c < cols; c += VOX_NT) vox_solid_column(sol, T, cr.lo[0] + c / nj, cr.lo[1] + c % nj, d1, d2, nw);
    }
    if (do_surface) {
      const VoxRange vr = vox_voxel_range(T, d0, d1, d2);
      const int nj = vr.extent(1), rows = vr.extent(2) > 0 ? vr.extent(0) * nj : 0;
      for (int c = tid; c < rows; c += VOX_NT) vox_surface_row(srf, T, vr.lo[0] + c / nj, vr.lo[1] + c % nj, vr.lo[2], vr.hi[2], d1, nw);
    }
  }
  __syncthreads();
  unsigned int* g_sol = masks + (size_t)b * 2 * words;
  unsigned int* g_srf = g_sol + words;
  for (int w = tid; w < words && w < LDSW; w += VOX_NT) {
    const unsigned int s = sol[w], f = srf[w];
    if (s) atomicXor(g_sol + w, s);
    if (f) atomicOr(g_srf + w, f);
  }
}

__global__ void __launch_bounds__(256) voxelise_expand_kernel(const unsigned int* __restrict__ masks, int rows_per_mesh, int d2, int nw, int out_dtype,
                                                              long long total, void* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int k = (int)(idx % d2);
  const long long row = idx / d2;
  const long long b = row / rows_per_mesh;
  const int r = (int)(row % rows_per_mesh), words = rows_per_mesh * nw, w = r * nw + (k >> 5);
  const unsigned int* m = masks + (size_t)b * 2 * words;
  const unsigned int bit = ((m[w] | m[words + w]) >> (k & 31)) & 1u;   // a mode's unused mask stays cleared
  if (out_dtype == 0) static_cast<float*>(out)[idx] = bit ? 1.f : 0.f;
  else static_cast<unsigned char*>(out)[idx] = (unsigned char)bit;
}

static inline bool vox_dims_ok(int B, int d0, int d1, int d2) {
  return B >= 1 && B <= 65535 && d0 >= 1 && d0 <= 64 && d1 >= 1 && d1 <= 64 && d2 >= 1 && d2 <= 64;
}
static inline size_t vox_table_bytes(int B) { return sizeof(long long) * 4 * (size_t)B; }
static inline size_t vox_counter_bytes(int B) { return (sizeof(int) * (size_t)B + 7) & ~(size_t)7; }

}  // namespace sv

using namespace sv;
#define STREAM static_cast<hipStream_t>(stream)

extern "C" size_t sv_voxelise_meshes_workspace_bytes(int B, int d0, int d1, int d2) {
  if (!vox_dims_ok(B, d0, d1, d2)) return 0;
  return vox_table_bytes(B) + vox_counter_bytes(B) + sizeof(unsigned int) * 2 * (size_t)B * d0 * d1 * (d2 <= 32 ? 1 : 2);
}

extern "C" int sv_voxelise_meshes(const int* verts, long long total_verts, const int* tris, long long total_tris, const long long* mesh_table, int B,
                                  int d0, int d1, int d2, int mode, int out_dtype, void* out, void* workspace, void* stream) {
  SV_REQUIRE(mesh_table && out && workspace, "sv_voxelise_meshes: bad arguments");
  SV_REQUIRE(B >= 1 && B <= 65535, "sv_voxelise_meshes: %d meshes (1 .. 65535 per call)", B);
  SV_REQUIRE(vox_dims_ok(B, d0, d1, d2), "sv_voxelise_meshes: dims %d x %d x %d, every dim must lie in 1 .. 64", d0, d1, d2);
  SV_REQUIRE(mode == SV_VOXELISE_SOLID || mode == SV_VOXELISE_SURFACE || mode == SV_VOXELISE_BOTH,
             "sv_voxelise_meshes: mode %d is none of 0 (solid), 1 (surface), 2 (both)", mode);
  SV_REQUIRE(out_dtype == 0 || out_dtype == 1, "sv_voxelise_meshes: out_dtype %d is neither 0 (float32) nor 1 (uint8)", out_dtype);
  SV_REQUIRE(total_verts >= 0 && total_tris >= 0 && (verts || total_verts == 0) && (tris || total_tris == 0),
             "sv_voxelise_meshes: buffers of %lld vertices and %lld triangles", total_verts, total_tris);
  SV_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "sv_voxelise_meshes: the workspace must be 8-byte aligned");
  long long most = 0;
  for (int b = 0; b < B; ++b) {                                               // the whole table, on the host, before anything is launched
    const long long vo = mesh_table[4 * b], nv = mesh_table[4 * b + 1], to = mesh_table[4 * b + 2], nt = mesh_table[4 * b + 3];
    SV_REQUIRE(vo >= 0 && nv >= 0 && vo <= total_verts && nv <= total_verts - vo,
               "sv_voxelise_meshes: mesh %d (vertex offset %lld, %lld vertices) does not lie inside the %lld vertices of the buffer", b, vo, nv, total_verts);
    SV_REQUIRE(to >= 0 && nt >= 0 && to <= total_tris && nt <= total_tris - to,
               "sv_voxelise_meshes: mesh %d (triangle offset %lld, %lld triangles) does not lie inside the %lld triangles of the buffer", b, to, nt,
               total_tris);
    SV_REQUIRE(nv <= 0x7fffffffll && nt <= 0x7fffffffll, "sv_voxelise_meshes: mesh %d has %lld vertices and %lld triangles (at most 2^31 - 1 each)", b, nv,
               nt);
    most = nt > most ? nt : most;
  }
  const int nw = d2 <= 32 ? 1 : 2, words = d0 * d1 * nw;
  char* ws = static_cast<char*>(workspace);
  long long* table_dev = reinterpret_cast<long long*>(ws);
  int* bad = reinterpret_cast<int*>(ws + vox_table_bytes(B));
  unsigned int* masks = reinterpret_cast<unsigned int*>(ws + vox_table_bytes(B) + vox_counter_bytes(B));
  // pageable host memory: the copy has read mesh_table when the call returns
  hipError_t e = hipMemcpyAsync(table_dev, mesh_table, vox_table_bytes(B), hipMemcpyHostToDevice, STREAM);
  if (e != hipSuccess) { set_error("sv_voxelise_meshes: table copy failed: %s", hipGetErrorString(e)); return SV_ERR_LAUNCH; }
  e = hipMemsetAsync(bad, 0, vox_counter_bytes(B) + sizeof(unsigned int) * 2 * (size_t)B * words, STREAM);
  if (e != hipSuccess) { set_error("sv_voxelise_meshes: memset failed: %s", hipGetErrorString(e)); return SV_ERR_LAUNCH; }
  if (most > 0) {
    const dim3 grid(cdiv(most, VOX_CHUNK), B);
    if (words <= 1024)
      hipLaunchKernelGGL(voxelise_accumulate_kernel<1024>, grid, dim3(VOX_NT), 0, STREAM, verts, tris, table_dev, d0, d1, d2, nw, mode, masks, bad);
    else
      hipLaunchKernelGGL(voxelise_accumulate_kernel<8192>, grid, dim3(VOX_NT), 0, STREAM, verts, tris, table_dev, d0, d1, d2, nw, mode, masks, bad);
  }
  const long long total = (long long)B * d0 * d1 * d2;
  hipLaunchKernelGGL(voxelise_expand_kernel, dim3(cdiv(total, 256)), dim3(256), 0, STREAM, masks, d0 * d1, d2, nw, out_dtype, total, out);
  return check_launch("sv_voxelise_meshes");
}
