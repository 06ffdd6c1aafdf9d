// Input preparation on the device: the reference does this per sample in DataLoader workers with numpy/cv2
// (utils/data_loaders.py:52-88, utils/data_transforms.py, utils/binvox_rw.py:118-149); at thousands of views per second that
// CPU path is the bottleneck, so the raw bytes (RLE voxel runs, 8-bit renderings) are shipped and expanded here.
//
//   sv_binvox_decode  run-length (value, count) byte pairs -> dense float occupancy, xzy -> xyz transposition
//   sv_binvox_encode  the way back (utils/binvox_rw.py:239-292): dense occupancy or thresholded logits -> the writer's byte pairs
//   sv_voxel_surface  the exposed voxel faces the reference draws (utils/helpers.py:50-88, core/test.py:178-187) as an indexed quad mesh
//   sv_augment_views  crop -> bilinear resize -> background composite -> colour jitter -> PCA noise -> normalise ->
//                     flip -> channel permutation -> CHW float, two launches (grey means for the contrast step, then the image)
//   sv_augment_images the same for a ragged batch of photographs, each cropped to its bounding box with edge padding
//                     (utils/data_transforms.py:93-136, :187-232): one launch pair, a descriptor per image
//   sv_augment_views_bg  sv_augment_views with RandomBackground's folder (:415-452): per image a photograph of a bank, or the flat colour
#include "common.h"

namespace sv {

// ---- binvox: one workgroup per volume; runs are placed with a running prefix sum over the counts -------------------------
__global__ void __launch_bounds__(256) binvox_decode_kernel(const unsigned char* __restrict__ rle, const long long* __restrict__ pair_off, int d0, int d1,
                                                            int d2, int fix_coords, float* __restrict__ out, int* __restrict__ decoded) {
  __shared__ int wsum[4];
  __shared__ int running_s;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long p0 = pair_off[b], p1 = pair_off[b + 1];
  const int total = d0 * d1 * d2;
  float* o = out + (size_t)b * total;
  if (tid == 0) running_s = 0;
  __syncthreads();
  for (long long base = p0; base < p1; base += 256) {
    const long long p = base + tid;
    int val = 0, cnt = 0;
    if (p < p1) {
      val = rle[2 * p];
      cnt = rle[2 * p + 1];
    }
    int inc = cnt;                               // inclusive scan inside the wave, then across the four waves
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(inc, d, 64);
      if (lane >= d) inc += t;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int start = running_s + inc - cnt;
    for (int i = 0; i < w; ++i) start += wsum[i];
    const float v = val ? 1.f : 0.f;             // .astype(bool)
    for (int t = 0; t < cnt; ++t) {
      const int f = start + t;
      if (f >= total) break;                     // malformed stream: the host sees decoded != total
      if (fix_coords) {                          // file order is [x][z][y]; np.transpose(data, (0, 2, 1)) -> [x][y][z]
        const int k = f % d2, j = (f / d2) % d1, i = f / (d1 * d2);
        o[((size_t)i * d2 + k) * d1 + j] = v;
      } else {
        o[f] = v;
      }
    }
    __syncthreads();
    if (tid == 0) running_s += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
  if (tid == 0) decoded[b] = running_s;
}

// ---- binvox writer (utils/binvox_rw.py:239-292): one workgroup per volume, file-order chunks of ENC_CHUNK voxels --------------
// A chunk is first reduced to a bit mask in LDS, in file order: the input is read along its own fastest axis and the (0, 2, 1)
// transposition happens in the scatter of the bits.  The reference's (state, ctr) loop is then restated per voxel, 256 voxels per pass:
//   start  = the voxel differs from its predecessor in file order (or is the first voxel)
//   t      = 1-based offset of the voxel in its run (max-scan of the start positions; a run open from earlier passes continues `run`)
//   a start other than voxel 0 emits (previous value, previous t % 255) - the "switch state" dump, a zero count included, which is what
//            the reference writes when the switch comes right after a dump at 255
//   t % 255 == 0 emits (value, 255)
//   the tail emits (value, run % 255) when that is non-zero
// and a sum-scan of the 0 / 1 / 2 emissions per voxel gives the output slots.  Carried between passes: the run length so far, the pairs
// written so far, and (between chunks) the last value.  A run of n >= 1 voxels emits at most n / 255 + 1 <= n pairs, so a volume never
// emits more pairs than it has voxels; every store is bounded by `cap` regardless.
constexpr int ENC_CHUNK = 1024;

__global__ void __launch_bounds__(256) binvox_encode_kernel(const void* __restrict__ vol, int dtype, int d0, int d1, int d2, int fix_coords, float th,
                                                            unsigned char* __restrict__ pairs, long long cap, int* __restrict__ n_pairs) {
  __shared__ unsigned int bits[ENC_CHUNK / 32];
  __shared__ int tl[256];
  __shared__ int wmax[4], wsum[4];
  __shared__ int run_s, np_s;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int total = d0 * d1 * d2, slab = d1 * d2;
  const size_t vbase = (size_t)b * total;
  unsigned char* o = pairs + (size_t)b * 2 * (size_t)cap;
  auto getbit = [&](int p) -> int { return (bits[p >> 5] >> (p & 31)) & 1; };
  auto put = [&](int slot, int v, int c) {
    if (slot < cap) {
      o[2 * (size_t)slot] = (unsigned char)v;
      o[2 * (size_t)slot + 1] = (unsigned char)c;
    }
  };
  if (tid == 0) { run_s = 0; np_s = 0; }
  int pv = 0;                                    // value of the voxel before the chunk
  for (int c0 = 0; c0 < total; c0 += ENC_CHUNK) {
    const int n = min(ENC_CHUNK, total - c0);
    __syncthreads();                             // the previous chunk's mask has been read
    if (tid < ENC_CHUNK / 32) bits[tid] = 0u;
    __syncthreads();
    if (fix_coords) {                            // file (i, j, k) = vol[(i * d2 + k) * d1 + j]: per slab i, walk the rows j the chunk touches with j fastest
      for (int i = c0 / slab; i <= (c0 + n - 1) / slab; ++i) {
        const int s0 = max(c0 - i * slab, 0), s1 = min(c0 + n - i * slab, slab);   // the chunk's part of the slab, in file order
        const int jlo = s0 / d2, nj = (s1 - 1) / d2 - jlo + 1;
        const int klo = nj == 1 ? s0 % d2 : 0, nk = nj == 1 ? s1 - s0 : d2;
        for (int q = tid; q < nj * nk; q += 256) {
          const int k = klo + q / nj, j = jlo + q % nj, s = j * d2 + k;
          if (s >= s0 && s < s1 && voxel_set(vol, dtype, vbase + ((size_t)i * d2 + k) * d1 + j, th)) {
            const int p = i * slab + s - c0;
            atomicOr(&bits[p >> 5], 1u << (p & 31));
          }
        }
      }
    } else {
      for (int q = 0; q < n; q += 256) {         // wave-uniform trip count: every lane takes part in the ballot
        const int p = q + tid;
        const unsigned long long m = __ballot(p < n && voxel_set(vol, dtype, vbase + c0 + p, th));
        if (lane == 0) {
          bits[(q >> 5) + 2 * w] = (unsigned int)m;
          bits[(q >> 5) + 2 * w + 1] = (unsigned int)(m >> 32);
        }
      }
    }
    __syncthreads();
    for (int q = 0; q < n; q += 256) {
      const int p = q + tid;
      const bool valid = p < n;
      const int bit = valid ? getbit(p) : 0;
      const int prev = p > 0 ? getbit(p - 1) : pv;
      const bool start = valid && (c0 + p == 0 || bit != prev);
      int ms = start ? tid : -1;                 // inclusive max-scan: position of the latest run start at or before this voxel
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(ms, d, 64);
        if (lane >= d) ms = max(ms, t);
      }
      if (lane == 63) wmax[w] = ms;
      __syncthreads();
      for (int i = 0; i < w; ++i) ms = max(ms, wmax[i]);
      const int t = valid ? (ms >= 0 ? tid - ms + 1 : run_s + tid + 1) : 0;
      tl[tid] = t;
      const int ea = (start && c0 + p > 0) ? 1 : 0, eb = (valid && t % 255 == 0) ? 1 : 0;
      int inc = ea + eb;                         // inclusive sum-scan of the emissions
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(inc, d, 64);
        if (lane >= d) inc += u;
      }
      if (lane == 63) wsum[w] = inc;
      __syncthreads();
      int slot = np_s + inc - ea - eb;
      for (int i = 0; i < w; ++i) slot += wsum[i];
      if (ea) put(slot, prev, (tid > 0 ? tl[tid - 1] : run_s) % 255);
      if (eb) put(slot + ea, bit, 255);
      __syncthreads();
      if (tid == 0) {
        np_s += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        run_s = tl[min(256, n - q) - 1];
      }
      __syncthreads();
    }
    pv = getbit(n - 1);
  }
  if (tid == 0) {
    int np = np_s;
    if (run_s % 255 > 0) put(np++, pv, run_s % 255);   // "flush out remainders"
    n_pairs[b] = np;
  }
}

// ---- exposed voxel faces (utils/helpers.py:50-88 -> Axes3D.voxels; utils/binvox_rw.py:306-343): one workgroup per volume ---------
// The quads that separate a filled voxel from an empty one or from the outside, as an indexed mesh in a fixed order (no atomics):
//   (a) occupancy bit mask `occ` in LDS, bit p = voxel (x * d1 + y) * d2 + z, from a ballot over the input;
//   (b) lattice "used" bit mask: point (i, j, k) of [0..d0] x [0..d1] x [0..d2] is a corner of an exposed face iff its 8 surrounding cells
//       (outside = empty) are neither all filled nor all empty; `pre[w]` = used points in the words before w (workgroup sum-scan of the
//       popcounts), so vertex id of lattice point l = pre[l >> 5] + popcount(used[l >> 5] & lower bits) - lattice rows are d2 + 1 points long,
//       so a row's vertex run straddles words and nothing below assumes otherwise;
//   (c) vertex list: the used lattice indices, ascending;
//   (d) faces: every thread owns a contiguous run of voxels, counts their exposed faces (directions -x +x -y +y -z +z), one workgroup
//       sum-scan gives its first slot, and each face is one 16-byte store of four vertex ids (corners counter-clockwise seen from outside).
// LDS at MAXD = 64: 8192 + 2 * 8583 words = 101 432 B (one static block, as the fused kernels of attn.hip hold theirs); at MAXD = 32: 13 088 B.
// Every global store is bounded by the capacities; every LDS word index by the word counts of the template's MAXD.
constexpr int SURF_NT = 1024;

template <int MAXD>
struct SurfLds {
  static constexpr int OCC_W = MAXD * MAXD * MAXD / 32;
  static constexpr int LAT_W = ((MAXD + 1) * (MAXD + 1) * (MAXD + 1) + 31) / 32;
};

// exclusive sum-scan over the workgroup in thread order; `total` receives the workgroup's sum.  wsum is [SURF_NT / 64] in LDS.
__device__ __forceinline__ int surf_scan(int v, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(inc, d, 64);
    if (lane >= d) inc += u;
  }
  __syncthreads();                               // the previous scan's wsum has been read
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  int excl = inc - v, t = 0;
  for (int i = 0; i < SURF_NT / 64; ++i) {
    const int s = wsum[i];
    if (i < w) excl += s;
    t += s;
  }
  total = t;
  return excl;
}

template <int MAXD>
__global__ void __launch_bounds__(SURF_NT) voxel_surface_kernel(const void* __restrict__ vol, int dtype, int d0, int d1, int d2, float th,
                                                                unsigned int* __restrict__ verts, long long vcap, unsigned int* __restrict__ faces,
                                                                long long fcap, int* __restrict__ counts) {
  constexpr int OCC_W = SurfLds<MAXD>::OCC_W, LAT_W = SurfLds<MAXD>::LAT_W;
  __shared__ __attribute__((aligned(16))) unsigned int surf_smem[OCC_W + 2 * LAT_W];
  __shared__ int wsum[SURF_NT / 64];
  unsigned int* occ = surf_smem;                 // [OCC_W]
  unsigned int* used = occ + OCC_W;              // [LAT_W]
  unsigned int* pre = used + LAT_W;              // [LAT_W]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int total = d0 * d1 * d2, slab = d1 * d2;
  const int e1 = d1 + 1, e2 = d2 + 1, lslab = e1 * e2, ltotal = (d0 + 1) * lslab, lwords = (ltotal + 31) >> 5;
  const size_t vbase = (size_t)b * total;
  unsigned int* vo = verts + (size_t)b * (size_t)vcap;
  uint4* fo = reinterpret_cast<uint4*>(faces) + (size_t)b * (size_t)fcap;
  auto filled = [&](int p) -> bool { return (occ[p >> 5] >> (p & 31)) & 1u; };
  // corners of the six directions, counter-clockwise seen from outside; a corner is (dx << 2) | (dy << 1) | dz
  constexpr int CORNER[6][4] = {{0, 1, 3, 2}, {4, 6, 7, 5}, {0, 4, 5, 1}, {2, 3, 7, 6}, {0, 2, 6, 4}, {1, 5, 7, 3}};

  // (a) occupancy mask; the trip count is wave-uniform, so every lane takes part in the ballot
  for (int q = 0; q < total; q += SURF_NT) {
    const int p = q + tid;
    const unsigned long long m = __ballot(p < total && voxel_set(vol, dtype, vbase + p, th));
    const int wi = (q >> 5) + 2 * w;
    if (lane == 0 && wi + 1 < OCC_W) {           // always true for total <= MAXD^3 (a multiple of SURF_NT); the LDS bound all the same
      occ[wi] = (unsigned int)m;
      occ[wi + 1] = (unsigned int)(m >> 32);
    }
  }
  __syncthreads();

  // (b) used mask from the 8-cell rule
  for (int q = 0; q < ltotal; q += SURF_NT) {
    const int l = q + tid;
    bool u = false;
    if (l < ltotal) {
      const int i = l / lslab, r = l - i * lslab, j = r / e2, k = r - j * e2;
      int n = 0;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int x = i - 1 + (c >> 2), y = j - 1 + ((c >> 1) & 1), z = k - 1 + (c & 1);
        if (x >= 0 && x < d0 && y >= 0 && y < d1 && z >= 0 && z < d2) n += filled(x * slab + y * d2 + z) ? 1 : 0;
      }
      u = n > 0 && n < 8;
    }
    const unsigned long long m = __ballot(u);
    const int wi = (q >> 5) + 2 * w;
    if (lane == 0) {
      if (wi < lwords) used[wi] = (unsigned int)m;
      if (wi + 1 < lwords) used[wi + 1] = (unsigned int)(m >> 32);
    }
  }
  __syncthreads();
  int n_verts;
  {
    const int per = (lwords + SURF_NT - 1) / SURF_NT, w0 = min(tid * per, lwords), w1 = min(w0 + per, lwords);
    int s = 0;
    for (int i = w0; i < w1; ++i) s += __popc(used[i]);
    int run = surf_scan(s, wsum, n_verts);
    for (int i = w0; i < w1; ++i) {
      pre[i] = (unsigned int)run;
      run += __popc(used[i]);
    }
  }
  __syncthreads();
  auto vid = [&](int l) -> unsigned int { return pre[l >> 5] + __popc(used[l >> 5] & ((1u << (l & 31)) - 1u)); };

  // (c) vertex list
  for (int l = tid; l < ltotal; l += SURF_NT) {
    if ((used[l >> 5] >> (l & 31)) & 1u) {
      const unsigned int id = vid(l);
      if ((long long)id < vcap) vo[id] = (unsigned int)l;
    }
  }

  // (d) faces
  const int per = (total + SURF_NT - 1) / SURF_NT, p0 = min(tid * per, total), p1 = min(p0 + per, total);
  auto exposure = [&](int p, int x, int y, int z) -> unsigned int {
    if (!filled(p)) return 0u;
    unsigned int e = 0u;
    if (x == 0 || !filled(p - slab)) e |= 1u;
    if (x == d0 - 1 || !filled(p + slab)) e |= 2u;
    if (y == 0 || !filled(p - d2)) e |= 4u;
    if (y == d1 - 1 || !filled(p + d2)) e |= 8u;
    if (z == 0 || !filled(p - 1)) e |= 16u;
    if (z == d2 - 1 || !filled(p + 1)) e |= 32u;
    return e;
  };
  const int x0 = p0 / slab, r0 = p0 - x0 * slab, y0 = r0 / d2, z0 = r0 - y0 * d2;
  int nf = 0;
  for (int p = p0, x = x0, y = y0, z = z0; p < p1; ++p) {
    nf += __popc(exposure(p, x, y, z));
    if (++z == d2) { z = 0; if (++y == d1) { y = 0; ++x; } }
  }
  int n_faces;
  long long slot = surf_scan(nf, wsum, n_faces);
  for (int p = p0, x = x0, y = y0, z = z0; p < p1; ++p) {
    const unsigned int e = exposure(p, x, y, z);
    if (e) {
      const int l = (x * e1 + y) * e2 + z;
      unsigned int c[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) c[q] = vid(l + (q >> 2) * lslab + ((q >> 1) & 1) * e2 + (q & 1));
#pragma unroll
      for (int d = 0; d < 6; ++d)
        if ((e >> d) & 1u) {
          if (slot < fcap) fo[slot] = make_uint4(c[CORNER[d][0]], c[CORNER[d][1]], c[CORNER[d][2]], c[CORNER[d][3]]);
          ++slot;
        }
    }
    if (++z == d2) { z = 0; if (++y == d1) { y = 0; ++x; } }
  }
  if (tid == 0) {
    counts[2 * b] = n_verts;
    counts[2 * b + 1] = n_faces;
  }
}

// ---- view augmentation -----------------------------------------------------------------------------------------------------
struct AugGeom {
  int I, V, Hs, Ws, C, x0, y0, cw, ch, Ho, Wo;
};

// cv2.resize(..., INTER_LINEAR) source coordinate of a destination index (float arithmetic as in OpenCV's resize.cpp)
__device__ __forceinline__ void lin_coord(int d, double scale, int ssize, int& s, float& f) {
  float fx = (float)((d + 0.5) * scale - 0.5);
  s = (int)floorf(fx);
  fx -= (float)s;
  if (s < 0) { fx = 0.f; s = 0; }
  if (s >= ssize - 1) { fx = 0.f; s = ssize - 1; }
  f = fx;
}

// the four taps of one resized pixel (rows r0 / r1, pixel columns x0 / x1 in them): horizontal pass on the two source rows, then the
// vertical pass; products and sums are rounded separately (no fused multiply-add) so that the CPU restatement reproduces them bit for bit
__device__ __forceinline__ void blend_taps(const unsigned char* __restrict__ r0, const unsigned char* __restrict__ r1, int x0, int x1, int C, float fx,
                                           float fy, float px[4]) {
  const float a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy;
  for (int c = 0; c < C; ++c) {
    const float t00 = (float)r0[x0 * C + c] / 255.f, t01 = (float)r0[x1 * C + c] / 255.f;
    const float t10 = (float)r1[x0 * C + c] / 255.f, t11 = (float)r1[x1 * C + c] / 255.f;
    const float h0 = __fadd_rn(__fmul_rn(t00, a0), __fmul_rn(t01, a1));
    const float h1 = __fadd_rn(__fmul_rn(t10, a0), __fmul_rn(t11, a1));
    px[c] = __fadd_rn(__fmul_rn(h0, b0), __fmul_rn(h1, b1));
  }
}

// resized crop at (oy, ox)
__device__ __forceinline__ void sample_pixel(const unsigned char* __restrict__ img, const AugGeom& g, int oy, int ox, float px[4]) {
  int sx, sy;
  float fx, fy;
  lin_coord(ox, (double)g.cw / g.Wo, g.cw, sx, fx);
  lin_coord(oy, (double)g.ch / g.Ho, g.ch, sy, fy);
  const int sx1 = min(sx + 1, g.cw - 1), sy1 = min(sy + 1, g.ch - 1);
  const unsigned char* r0 = img + ((size_t)(g.y0 + sy) * g.Ws + g.x0) * g.C;
  const unsigned char* r1 = img + ((size_t)(g.y0 + sy1) * g.Ws + g.x0) * g.C;
  blend_taps(r0, r1, sx, sx1, g.C, fx, fy, px);
}

// RandomBackground: pixels whose (resized) alpha is exactly zero take the background colour
__device__ __forceinline__ void composite(float px[4], int C, const float bg[3]) {
  if (C == 4 && px[3] == 0.f) {
    px[0] = bg[0];
    px[1] = bg[1];
    px[2] = bg[2];
  }
}
__device__ __forceinline__ float grey_of(const float px[4]) { return 0.114f * px[0] + 0.587f * px[1] + 0.299f * px[2]; }

__global__ void __launch_bounds__(256) augment_grey_mean_kernel(const unsigned char* __restrict__ src, AugGeom g, const sv_aug_sample* __restrict__ prm,
                                                                double* __restrict__ grey_sum) {
  __shared__ float red[4];
  const int img = blockIdx.y;
  const sv_aug_sample& P = prm[img / g.V];
  const unsigned char* s = src + (size_t)img * g.Hs * g.Ws * g.C;
  const int npix = g.Ho * g.Wo;
  float acc = 0.f;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < npix; p += gridDim.x * 256) {
    float px[4];
    sample_pixel(s, g, p / g.Wo, p % g.Wo, px);
    composite(px, g.C, P.bg);
    acc += grey_of(px);
  }
  const float r = block_sum<4>(acc, red);
  if (threadIdx.x == 0) atomicAdd(&grey_sum[img], (double)r);
}

__global__ void __launch_bounds__(256) augment_apply_kernel(const unsigned char* __restrict__ src, AugGeom g, const sv_aug_sample* __restrict__ prm,
                                                            const unsigned char* __restrict__ flip, const double* __restrict__ grey_sum,
                                                            float* __restrict__ out) {
  const int img = blockIdx.y;
  const sv_aug_sample P = prm[img / g.V];
  const unsigned char* s = src + (size_t)img * g.Hs * g.Ws * g.C;
  const int npix = g.Ho * g.Wo;
  const bool fl = flip != nullptr && flip[img] != 0;
  float mean_grey = (float)(grey_sum[img] / (double)npix);
  // the contrast step blends with the mean grey of the image as it is at that point of the jitter order: brightness scales it,
  // saturation and contrast itself leave it unchanged
  float contrast_mean = mean_grey;
  for (int k = 0; k < 3; ++k) {
    if (P.jitter_order[k] == 1) break;
    if (P.jitter_order[k] == 0) contrast_mean *= P.jitter_value[0];
  }
  float* o = out + (size_t)img * 3 * npix;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < npix; p += gridDim.x * 256) {
    const int oy = p / g.Wo, ox = p % g.Wo;
    float px[4];
    sample_pixel(s, g, oy, fl ? g.Wo - 1 - ox : ox, px);           // np.fliplr of the finished image = sampling the mirrored column
    composite(px, g.C, P.bg);
#pragma unroll
    for (int k = 0; k < 3; ++k) {                                  // ColorJitter: 0 brightness, 1 contrast, 2 saturation
      const int kind = P.jitter_order[k];
      const float a = P.jitter_value[kind];
      const float other = kind == 0 ? 0.f : (kind == 1 ? contrast_mean : grey_of(px));
#pragma unroll
      for (int c = 0; c < 3; ++c) px[c] = a * px[c] + (1.f - a) * other;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = (px[c] + P.noise[c] - P.mean[c]) / P.std[c];   // RandomNoise (already in channel order), Normalize
#pragma unroll
    for (int c = 0; c < 3; ++c) o[(size_t)c * npix + p] = px[P.perm[c]];                // RandomPermuteRGB, ToTensor (HWC -> CHW)
  }
}

// ---- ragged form of the two kernels above (sv_augment_images): grid (blocks, I), image blockIdx.y described by images[blockIdx.y], one
// sv_aug_sample and one flip byte per image.  The two paths share lin_coord, blend_taps, composite and grey_of.  The kernel bodies mirror
// the dense ones statement for statement instead of sharing a function: the jitter and normalise expressions are left to the compiler's
// contraction, and moving them into a shared function changed which products it fuses in augment_apply_kernel (last-bit changes in
// sv_augment_views).  Mirrored, the dense kernels compile to the instructions they had before, and an unboxed batch of equal sizes gives
// the bits of sv_augment_views (tests/test_gpu_bbox_crop.py).
struct BoxGeom {
  int Ws, C, cw, ch, Ho, Wo;
  int xo, yo;                   // source coordinate of padded coordinate 0 (x_left - pad_l, y_top - pad_t; negative inside the padding)
  int xl, xr, yt, yb;           // kept rectangle, inclusive
};
__device__ __forceinline__ BoxGeom box_geom(const sv_aug_image& d, int C, int Ho, int Wo) {
  BoxGeom g;
  g.Ws = d.Ws; g.C = C; g.Ho = Ho; g.Wo = Wo;
  g.cw = d.pad_l + (d.x_right - d.x_left + 1) + d.pad_r;
  g.ch = d.pad_t + (d.y_bottom - d.y_top + 1) + d.pad_b;
  g.xo = d.x_left - d.pad_l; g.yo = d.y_top - d.pad_t;
  g.xl = d.x_left; g.xr = d.x_right; g.yt = d.y_top; g.yb = d.y_bottom;
  return g;
}

// lin_coord runs in the coordinates of the padded crop (cw x ch); np.pad(..., mode='edge') is the clamp of a padded coordinate onto the
// kept rectangle, so no padded copy exists.  Bytes only: an image starts wherever the one before it ended.
__device__ __forceinline__ void sample_pixel(const unsigned char* __restrict__ img, const BoxGeom& g, int oy, int ox, float px[4]) {
  int sx, sy;
  float fx, fy;
  lin_coord(ox, (double)g.cw / g.Wo, g.cw, sx, fx);
  lin_coord(oy, (double)g.ch / g.Ho, g.ch, sy, fy);
  const int sx1 = min(sx + 1, g.cw - 1), sy1 = min(sy + 1, g.ch - 1);
  const int x0 = min(max(g.xo + sx, g.xl), g.xr), x1 = min(max(g.xo + sx1, g.xl), g.xr);
  const int y0 = min(max(g.yo + sy, g.yt), g.yb), y1 = min(max(g.yo + sy1, g.yt), g.yb);
  blend_taps(img + (size_t)y0 * g.Ws * g.C, img + (size_t)y1 * g.Ws * g.C, x0, x1, g.C, fx, fy, px);
}

__global__ void __launch_bounds__(256) augment_images_grey_mean_kernel(const unsigned char* __restrict__ src, const sv_aug_image* __restrict__ images,
                                                                       int C, int Ho, int Wo, const sv_aug_sample* __restrict__ prm,
                                                                       double* __restrict__ grey_sum) {
  __shared__ float red[4];
  const int img = blockIdx.y;
  const sv_aug_sample& P = prm[img];
  const BoxGeom g = box_geom(images[img], C, Ho, Wo);
  const unsigned char* s = src + images[img].offset;
  const int npix = g.Ho * g.Wo;
  float acc = 0.f;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < npix; p += gridDim.x * 256) {
    float px[4];
    sample_pixel(s, g, p / g.Wo, p % g.Wo, px);
    composite(px, g.C, P.bg);
    acc += grey_of(px);
  }
  const float r = block_sum<4>(acc, red);
  if (threadIdx.x == 0) atomicAdd(&grey_sum[img], (double)r);
}

__global__ void __launch_bounds__(256) augment_images_apply_kernel(const unsigned char* __restrict__ src, const sv_aug_image* __restrict__ images, int C,
                                                                   int Ho, int Wo, const sv_aug_sample* __restrict__ prm,
                                                                   const unsigned char* __restrict__ flip, const double* __restrict__ grey_sum,
                                                                   float* __restrict__ out) {
  const int img = blockIdx.y;
  const sv_aug_sample P = prm[img];
  const BoxGeom g = box_geom(images[img], C, Ho, Wo);
  const unsigned char* s = src + images[img].offset;
  const int npix = g.Ho * g.Wo;
  const bool fl = flip != nullptr && flip[img] != 0;
  float mean_grey = (float)(grey_sum[img] / (double)npix);
  float contrast_mean = mean_grey;                                 // as in augment_apply_kernel
  for (int k = 0; k < 3; ++k) {
    if (P.jitter_order[k] == 1) break;
    if (P.jitter_order[k] == 0) contrast_mean *= P.jitter_value[0];
  }
  float* o = out + (size_t)img * 3 * npix;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < npix; p += gridDim.x * 256) {
    const int oy = p / g.Wo, ox = p % g.Wo;
    float px[4];
    sample_pixel(s, g, oy, fl ? g.Wo - 1 - ox : ox, px);
    composite(px, g.C, P.bg);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int kind = P.jitter_order[k];
      const float a = P.jitter_value[kind];
      const float other = kind == 0 ? 0.f : (kind == 1 ? contrast_mean : grey_of(px));
#pragma unroll
      for (int c = 0; c < 3; ++c) px[c] = a * px[c] + (1.f - a) * other;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = (px[c] + P.noise[c] - P.mean[c]) / P.std[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) o[(size_t)c * npix + p] = px[P.perm[c]];
  }
}

// ---- photograph backgrounds (sv_augment_views_bg): the dense pair once more, mirrored for the reason given above, with the composite
// that RandomBackground makes when it has a folder (utils/data_transforms.py:437-448): image blockIdx.y takes photograph bg_index[img] of
// the bank ([n_bank][Ho][Wo][3] bytes) where its resized alpha is exactly zero, or the flat colour when the index is -1.  The reference's
// alpha * bg + (1 - alpha) * img with alpha in {0, 1} is a select.  The photograph has the size of the output, so its pixel is read at the
// output row and at the column the source is sampled at: RandomFlip mirrors the finished image, photograph included.  One byte-triple per
// transparent pixel, consecutive lanes on consecutive triples (mirrored: descending).  The entry has checked every index against n_bank.
__device__ __forceinline__ void composite_photo(float px[4], int C, const float bg[3], const unsigned char* __restrict__ photo, int pix) {
  if (C == 4 && px[3] == 0.f) {
    if (photo != nullptr) {
      const unsigned char* t = photo + (size_t)pix * 3;
      px[0] = (float)t[0] / 255.f;               // cv2.imread(...).astype(np.float32) / 255.
      px[1] = (float)t[1] / 255.f;
      px[2] = (float)t[2] / 255.f;
    } else {
      px[0] = bg[0];
      px[1] = bg[1];
      px[2] = bg[2];
    }
  }
}

__global__ void __launch_bounds__(256) augment_bg_grey_mean_kernel(const unsigned char* __restrict__ src, AugGeom g, const sv_aug_sample* __restrict__ prm,
                                                                   const unsigned char* __restrict__ bank, const int* __restrict__ bg_index,
                                                                   double* __restrict__ grey_sum) {
  __shared__ float red[4];
  const int img = blockIdx.y;
  const sv_aug_sample& P = prm[img / g.V];
  const unsigned char* s = src + (size_t)img * g.Hs * g.Ws * g.C;
  const int npix = g.Ho * g.Wo;
  const int bi = bg_index[img];
  const unsigned char* photo = bi >= 0 ? bank + (size_t)bi * npix * 3 : nullptr;
  float acc = 0.f;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < npix; p += gridDim.x * 256) {
    float px[4];
    sample_pixel(s, g, p / g.Wo, p % g.Wo, px);
    composite_photo(px, g.C, P.bg, photo, p);
    acc += grey_of(px);
  }
  const float r = block_sum<4>(acc, red);
  if (threadIdx.x == 0) atomicAdd(&grey_sum[img], (double)r);
}

__global__ void __launch_bounds__(256) augment_bg_apply_kernel(const unsigned char* __restrict__ src, AugGeom g, const sv_aug_sample* __restrict__ prm,
                                                               const unsigned char* __restrict__ flip, const unsigned char* __restrict__ bank,
                                                               const int* __restrict__ bg_index, const double* __restrict__ grey_sum,
                                                               float* __restrict__ out) {
  const int img = blockIdx.y;
  const sv_aug_sample P = prm[img / g.V];
  const unsigned char* s = src + (size_t)img * g.Hs * g.Ws * g.C;
  const int npix = g.Ho * g.Wo;
  const bool fl = flip != nullptr && flip[img] != 0;
  const int bi = bg_index[img];
  const unsigned char* photo = bi >= 0 ? bank + (size_t)bi * npix * 3 : nullptr;
  float mean_grey = (float)(grey_sum[img] / (double)npix);
  float contrast_mean = mean_grey;                                 // as in augment_apply_kernel
  for (int k = 0; k < 3; ++k) {
    if (P.jitter_order[k] == 1) break;
    if (P.jitter_order[k] == 0) contrast_mean *= P.jitter_value[0];
  }
  float* o = out + (size_t)img * 3 * npix;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < npix; p += gridDim.x * 256) {
    const int oy = p / g.Wo, ox = p % g.Wo;
    const int sx = fl ? g.Wo - 1 - ox : ox;
    float px[4];
    sample_pixel(s, g, oy, sx, px);
    composite_photo(px, g.C, P.bg, photo, oy * g.Wo + sx);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int kind = P.jitter_order[k];
      const float a = P.jitter_value[kind];
      const float other = kind == 0 ? 0.f : (kind == 1 ? contrast_mean : grey_of(px));
#pragma unroll
      for (int c = 0; c < 3; ++c) px[c] = a * px[c] + (1.f - a) * other;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = (px[c] + P.noise[c] - P.mean[c]) / P.std[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) o[(size_t)c * npix + p] = px[P.perm[c]];
  }
}

}  // namespace sv

using namespace sv;
#define STREAM static_cast<hipStream_t>(stream)

extern "C" int sv_binvox_decode(const unsigned char* rle, const long long* pair_offsets, int B, int d0, int d1, int d2, int fix_coords,
                                float* out, int* decoded, void* stream) {
  SV_REQUIRE(rle && pair_offsets && out && decoded && B > 0 && d0 > 0 && d1 > 0 && d2 > 0, "binvox_decode: bad arguments");
  SV_REQUIRE((long long)d0 * d1 * d2 < (1ll << 30), "binvox_decode: volume too large");
  hipLaunchKernelGGL(binvox_decode_kernel, dim3(B), dim3(256), 0, STREAM, rle, pair_offsets, d0, d1, d2, fix_coords, out, decoded);
  return check_launch("sv_binvox_decode");
}

extern "C" int sv_binvox_encode(const void* vol, int dtype, int B, int d0, int d1, int d2, int fix_coords, float threshold, unsigned char* pairs,
                                long long pair_capacity, int* n_pairs, void* stream) {
  SV_REQUIRE(vol && pairs && n_pairs && B > 0 && d0 > 0 && d1 > 0 && d2 > 0, "sv_binvox_encode: bad arguments");
  SV_REQUIRE((long long)d0 * d1 * d2 < (1ll << 30), "sv_binvox_encode: volume too large");
  SV_REQUIRE(dtype == 0 || dtype == 1, "sv_binvox_encode: dtype %d is neither 0 (float32) nor 1 (uint8)", dtype);
  SV_REQUIRE(threshold < 0.f || (threshold > 0.f && threshold < 1.f), "sv_binvox_encode: threshold must be negative (occupancy input) or in (0, 1)");
  SV_REQUIRE(threshold < 0.f || dtype == 0, "sv_binvox_encode: a sigmoid threshold needs float32 logits");
  SV_REQUIRE(pair_capacity >= (long long)d0 * d1 * d2, "sv_binvox_encode: pair_capacity %lld is below the %lld voxels of a volume", pair_capacity,
             (long long)d0 * d1 * d2);
  hipLaunchKernelGGL(binvox_encode_kernel, dim3(B), dim3(256), 0, STREAM, vol, dtype, d0, d1, d2, fix_coords, threshold, pairs, pair_capacity, n_pairs);
  return check_launch("sv_binvox_encode");
}

extern "C" int sv_voxel_surface(const void* vol, int dtype, int B, int d0, int d1, int d2, float threshold, unsigned int* verts, long long vert_capacity,
                                unsigned int* faces, long long face_capacity, int* counts, void* stream) {
  SV_REQUIRE(vol && verts && faces && counts && B > 0, "sv_voxel_surface: bad arguments");
  SV_REQUIRE(d0 >= 1 && d0 <= 64 && d1 >= 1 && d1 <= 64 && d2 >= 1 && d2 <= 64, "sv_voxel_surface: dims %d x %d x %d, every dim must lie in 1 .. 64", d0,
             d1, d2);
  SV_REQUIRE(dtype == 0 || dtype == 1, "sv_voxel_surface: dtype %d is neither 0 (float32) nor 1 (uint8)", dtype);
  SV_REQUIRE(threshold < 0.f || (threshold > 0.f && threshold < 1.f), "sv_voxel_surface: threshold must be negative (occupancy input) or in (0, 1)");
  SV_REQUIRE(threshold < 0.f || dtype == 0, "sv_voxel_surface: a sigmoid threshold needs float32 logits");
  const long long vmax = (long long)(d0 + 1) * (d1 + 1) * (d2 + 1), fmax = 3ll * d0 * d1 * d2 + (long long)d0 * d1 + (long long)d1 * d2 + (long long)d0 * d2;
  SV_REQUIRE(vert_capacity >= vmax, "sv_voxel_surface: vert_capacity %lld is below the %lld lattice points of a volume", vert_capacity, vmax);
  SV_REQUIRE(face_capacity >= fmax, "sv_voxel_surface: face_capacity %lld is below the %lld lattice faces of a volume", face_capacity, fmax);
  SV_REQUIRE((reinterpret_cast<uintptr_t>(faces) & 15) == 0, "sv_voxel_surface: faces must be 16-byte aligned");
  if (d0 <= 32 && d1 <= 32 && d2 <= 32)
    hipLaunchKernelGGL(voxel_surface_kernel<32>, dim3(B), dim3(SURF_NT), 0, STREAM, vol, dtype, d0, d1, d2, threshold, verts, vert_capacity, faces,
                       face_capacity, counts);
  else
    hipLaunchKernelGGL(voxel_surface_kernel<64>, dim3(B), dim3(SURF_NT), 0, STREAM, vol, dtype, d0, d1, d2, threshold, verts, vert_capacity, faces,
                       face_capacity, counts);
  return check_launch("sv_voxel_surface");
}

extern "C" int sv_augment_views(const unsigned char* src, int I, int V, int Hs, int Ws, int C, int crop_h, int crop_w, int out_h, int out_w,
                                const sv_aug_sample* params_dev, const unsigned char* flip_dev, double* grey_sum_ws, float* out, void* stream) {
  SV_REQUIRE(src && params_dev && grey_sum_ws && out, "augment_views: bad arguments");
  SV_REQUIRE(I > 0 && V > 0 && I % V == 0 && (C == 3 || C == 4) && Hs > 0 && Ws > 0 && out_h > 0 && out_w > 0, "augment_views: bad shapes");
  AugGeom g;
  g.I = I; g.V = V; g.Hs = Hs; g.Ws = Ws; g.C = C; g.Ho = out_h; g.Wo = out_w;
  if (Hs > crop_h && Ws > crop_w && crop_h > 0 && crop_w > 0) {      // centre crop (data_transforms.py:135-139 / :222-226, no bounding box)
    g.x0 = (Ws - crop_w) / 2; g.y0 = (Hs - crop_h) / 2; g.cw = crop_w; g.ch = crop_h;
  } else {
    g.x0 = 0; g.y0 = 0; g.cw = Ws; g.ch = Hs;
  }
  hipError_t e = hipMemsetAsync(grey_sum_ws, 0, sizeof(double) * (size_t)I, STREAM);
  if (e != hipSuccess) { set_error("augment_views: memset failed: %s", hipGetErrorString(e)); return SV_ERR_LAUNCH; }
  const int bx = cdiv((long long)out_h * out_w, 256 * 4);
  hipLaunchKernelGGL(augment_grey_mean_kernel, dim3(bx, I), dim3(256), 0, STREAM, src, g, params_dev, grey_sum_ws);
  hipLaunchKernelGGL(augment_apply_kernel, dim3(bx, I), dim3(256), 0, STREAM, src, g, params_dev, flip_dev, grey_sum_ws, out);
  return check_launch("sv_augment_views");
}

// sv_augment_views with RandomBackground's folder (data_transforms.py:437-448): a photograph of the bank, or the flat colour, per image
extern "C" int sv_augment_views_bg(const unsigned char* src, int I, int V, int Hs, int Ws, int C, int crop_h, int crop_w, int out_h, int out_w,
                                   const sv_aug_sample* params_dev, const unsigned char* flip_dev, const unsigned char* bank, int n_bank,
                                   const int* bg_index_host, int* bg_index_dev_ws, double* grey_sum_ws, float* out, void* stream) {
  SV_REQUIRE(src && params_dev && grey_sum_ws && out && bg_index_host && bg_index_dev_ws, "augment_views_bg: bad arguments");
  SV_REQUIRE(I > 0 && V > 0 && I % V == 0 && (C == 3 || C == 4) && Hs > 0 && Ws > 0 && out_h > 0 && out_w > 0, "augment_views_bg: bad shapes");
  SV_REQUIRE(I <= 65535, "augment_views_bg: %d images (1 ... 65535 per call)", I);
  SV_REQUIRE((long long)out_h * out_w < (1ll << 30), "augment_views_bg: bad output size %d x %d", out_h, out_w);
  SV_REQUIRE(n_bank >= 0, "augment_views_bg: a bank of %d photographs", n_bank);
  for (int i = 0; i < I; ++i) {                                      // the whole table, on the host, before anything is launched
    const int idx = bg_index_host[i];
    SV_REQUIRE(idx >= -1 && idx < n_bank, "augment_views_bg: image %d asks for photograph %d of a bank of %d (-1 = the flat colour)", i, idx, n_bank);
    SV_REQUIRE(idx < 0 || bank != nullptr, "augment_views_bg: image %d asks for photograph %d and the bank is NULL", i, idx);
  }
  AugGeom g;
  g.I = I; g.V = V; g.Hs = Hs; g.Ws = Ws; g.C = C; g.Ho = out_h; g.Wo = out_w;
  if (Hs > crop_h && Ws > crop_w && crop_h > 0 && crop_w > 0) {      // as in sv_augment_views
    g.x0 = (Ws - crop_w) / 2; g.y0 = (Hs - crop_h) / 2; g.cw = crop_w; g.ch = crop_h;
  } else {
    g.x0 = 0; g.y0 = 0; g.cw = Ws; g.ch = Hs;
  }
  // pageable host memory: the copy has read bg_index_host when the call returns
  hipError_t e = hipMemcpyAsync(bg_index_dev_ws, bg_index_host, sizeof(int) * (size_t)I, hipMemcpyHostToDevice, STREAM);
  if (e != hipSuccess) { set_error("augment_views_bg: index copy failed: %s", hipGetErrorString(e)); return SV_ERR_LAUNCH; }
  e = hipMemsetAsync(grey_sum_ws, 0, sizeof(double) * (size_t)I, STREAM);
  if (e != hipSuccess) { set_error("augment_views_bg: memset failed: %s", hipGetErrorString(e)); return SV_ERR_LAUNCH; }
  const int bx = cdiv((long long)out_h * out_w, 256 * 4);
  hipLaunchKernelGGL(augment_bg_grey_mean_kernel, dim3(bx, I), dim3(256), 0, STREAM, src, g, params_dev, bank, bg_index_dev_ws, grey_sum_ws);
  hipLaunchKernelGGL(augment_bg_apply_kernel, dim3(bx, I), dim3(256), 0, STREAM, src, g, params_dev, flip_dev, bank, bg_index_dev_ws, grey_sum_ws, out);
  return check_launch("sv_augment_views_bg");
}

// CenterCrop / RandomCrop with a bounding box (data_transforms.py:93-136 / :187-232) for a ragged batch, then the list of sv_augment_views
extern "C" int sv_augment_images(const unsigned char* src, long long src_bytes, int I, int C, const sv_aug_image* images_host,
                                 sv_aug_image* images_dev_ws, int out_h, int out_w, const sv_aug_sample* params_dev, const unsigned char* flip_dev,
                                 double* grey_sum_ws, float* out, void* stream) {
  SV_REQUIRE(src && images_host && images_dev_ws && params_dev && grey_sum_ws && out, "augment_images: bad arguments");
  SV_REQUIRE(I > 0 && I <= 65535, "augment_images: %d images (1 ... 65535 per call)", I);
  SV_REQUIRE(C == 3 || C == 4, "augment_images: %d channels (3 or 4)", C);
  SV_REQUIRE(out_h > 0 && out_w > 0 && (long long)out_h * out_w < (1ll << 30), "augment_images: bad output size %d x %d", out_h, out_w);
  SV_REQUIRE(src_bytes > 0, "augment_images: empty source buffer");
  constexpr int LIM = 1 << 24;                                       // keeps every coordinate sum and Hs*Ws*C far from overflow
  for (int i = 0; i < I; ++i) {                                      // the whole table, on the host, before anything is launched
    const sv_aug_image& d = images_host[i];
    SV_REQUIRE(d.Hs > 0 && d.Ws > 0 && d.Hs <= LIM && d.Ws <= LIM, "augment_images: image %d has size %d x %d", i, d.Hs, d.Ws);
    SV_REQUIRE(d.offset >= 0 && d.offset <= src_bytes && (long long)d.Hs * d.Ws * C <= src_bytes - d.offset,
               "augment_images: image %d (offset %lld, %d x %d x %d) does not lie inside the %lld bytes of the source buffer", i, d.offset, d.Hs, d.Ws,
               C, src_bytes);
    SV_REQUIRE(d.x_left >= 0 && d.x_left <= d.x_right && d.x_right < d.Ws && d.y_top >= 0 && d.y_top <= d.y_bottom && d.y_bottom < d.Hs,
               "augment_images: image %d keeps columns [%d, %d] and rows [%d, %d]: empty or outside its %d x %d pixels", i, d.x_left, d.x_right,
               d.y_top, d.y_bottom, d.Hs, d.Ws);
    SV_REQUIRE(d.pad_l >= 0 && d.pad_r >= 0 && d.pad_t >= 0 && d.pad_b >= 0, "augment_images: image %d has a negative pad (%d, %d, %d, %d)", i,
               d.pad_l, d.pad_r, d.pad_t, d.pad_b);
    SV_REQUIRE(d.pad_l <= LIM && d.pad_r <= LIM && d.pad_t <= LIM && d.pad_b <= LIM &&
                   (long long)d.pad_l + (d.x_right - d.x_left + 1) + d.pad_r <= LIM && (long long)d.pad_t + (d.y_bottom - d.y_top + 1) + d.pad_b <= LIM,
               "augment_images: the padded crop of image %d is larger than %d", i, LIM);
  }
  // pageable host memory: the copy has read images_host when the call returns
  hipError_t e = hipMemcpyAsync(images_dev_ws, images_host, sizeof(sv_aug_image) * (size_t)I, hipMemcpyHostToDevice, STREAM);
  if (e != hipSuccess) { set_error("augment_images: descriptor copy failed: %s", hipGetErrorString(e)); return SV_ERR_LAUNCH; }
  e = hipMemsetAsync(grey_sum_ws, 0, sizeof(double) * (size_t)I, STREAM);
  if (e != hipSuccess) { set_error("augment_images: memset failed: %s", hipGetErrorString(e)); return SV_ERR_LAUNCH; }
  const int bx = cdiv((long long)out_h * out_w, 256 * 4);
  hipLaunchKernelGGL(augment_images_grey_mean_kernel, dim3(bx, I), dim3(256), 0, STREAM, src, images_dev_ws, C, out_h, out_w, params_dev, grey_sum_ws);
  hipLaunchKernelGGL(augment_images_apply_kernel, dim3(bx, I), dim3(256), 0, STREAM, src, images_dev_ws, C, out_h, out_w, params_dev, flip_dev,
                     grey_sum_ws, out);
  return check_launch("sv_augment_images");
}
