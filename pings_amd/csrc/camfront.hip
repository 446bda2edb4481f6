// Camera frame front-end on the device, for gfx950.
//
// The image pyramids of `CamImage.__init__` (gaussian_splatting/utils/cameras.py:39, :116-182): the RGB image, the depth
// image, the sky mask and the normal image of every camera of a frame, four levels each, in ONE launch.
//   camfront_pyramid      a table of up to PINGS_CAMFRONT_MAX_MAPS maps travels in the kernel arguments.  A workgroup takes
//                         one 128 x 32 tile of one map; a lane owns 8 x 2 level-0 pixels, so a wave owns 128 x 8 and holds
//                         one complete level-3 row.  Level 1 is formed in the lane's registers, levels 2 and 3 from the
//                         lanes 16 and 32 further on (the rows below) with cross-lane moves: no level is read back from
//                         memory, and no LDS or scratch is used.
//     bilinear (RGB, normal)   0.5 (0.5 a + 0.5 b) + 0.5 (0.5 c + 0.5 d), rounded to fp32 at every level: what
//                              F.interpolate(scale_factor=0.5, mode='bilinear', align_corners=False) evaluates on the
//                              device.  The products by 0.5 are exact, so a fused multiply-add rounds the same.
//     nearest-exact (depth)    level k takes level-0 pixel (2^k y + 2^k - 1, 2^k x + 2^k - 1)
//     nearest (sky mask)       level k takes level-0 pixel (2^k y, 2^k x)
//   A map whose width is a multiple of 16 and whose pointers are 16-byte aligned moves 8-byte words of the uint8 rows and
//   16-, 16-, 8- and 8-byte words of the fp32 levels 0..3 per lane; any other map takes element accesses.
// and the mono-depth cloud of dataset/slam_dataset.py:366-477:
//   camfront_align        the least-squares line LiDAR depth = k * predicted depth + b over the pixels both cover: fp64
//                         sums per workgroup in a fixed order, then a one-workgroup launch that adds the partials in
//                         index order and solves the 2 x 2 system about the means.  A launch boundary, not a ticket,
//                         separates the two stages.
//   camfront_mono_cloud   per camera: the fitted depth, the sky mask, the range gates, the back-projection and the
//                         colours of the kept pixels as [., 6] rows in row-major pixel order: flag, scan (devprim),
//                         scatter.  The count stays on the device.
//   The coloured voxel average that follows it is an instance of the centroid kernels of eval.hip and lives there.
// Plain stores only, no float atomics: every output is bitwise the same from run to run.
#include <cmath>

#include "common.hpp"
#include "devprim.hpp"

namespace {

using i64 = long long;

constexpr int kMaxMaps = PINGS_CAMFRONT_MAX_MAPS;
constexpr int kTileW = PINGS_CAMFRONT_TILE_W;
constexpr int kTileH = PINGS_CAMFRONT_TILE_H;
static_assert(kTileW == 128 && kTileH == 32, "a wave is 16 x 4 lanes of 8 x 2 pixels, a workgroup four waves stacked");

struct MapK {
  const void* src;
  void* lv[4];
  i64 sc, sy, sx;              // element strides of src (channel, row, pixel); unused for the uint8 HWC image
  int H, W, kind, vec;
  int tile0, tiles_x;          // first workgroup of this map, tiles per tile row
};
struct PyramidK {
  int n;
  MapK map[kMaxMaps];
};

template <typename T, int N>
struct alignas(sizeof(T) * N) Pack {
  T a[N];
};

template <typename T, int N>
__device__ inline void store_pack(T* d, const T* v) {
  Pack<T, N> p;
#pragma unroll
  for (int i = 0; i < N; ++i) p.a[i] = v[i];
  *reinterpret_cast<Pack<T, N>*>(d) = p;
}

template <typename T, int N>
__device__ inline void load_pack(const T* s, T* v) {
  const Pack<T, N> p = *reinterpret_cast<const Pack<T, N>*>(s);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = p.a[i];
}

__device__ inline float half_sum(float a, float b, float c, float d) {
  return 0.5f * (0.5f * a + 0.5f * b) + 0.5f * (0.5f * c + 0.5f * d);
}

// RGB (uint8 HWC or fp32 with strides) and normal image.  Every lane of the wave runs the whole function: the cross-lane
// moves need the lanes outside the image too, which carry zeros that no pixel inside ever reads.
template <bool U8>
__device__ inline void bilinear_lane(const MapK& m, int x0, int y0, int tx, int ty) {
  const int H = m.H, W = m.W;
  const int H1 = H >> 1, W1 = W >> 1, H2 = H >> 2, W2 = W >> 2, H3 = H >> 3, W3 = W >> 3;
  const bool vec = m.vec != 0, in_x = x0 < W;                  // vec: W % 16 == 0, so a lane is inside or outside whole
  const bool clamp = m.kind == PINGS_CAMFRONT_RGB_F32;
  float* const o0 = static_cast<float*>(m.lv[0]);
  float* const o1 = static_cast<float*>(m.lv[1]);
  float* const o2 = static_cast<float*>(m.lv[2]);
  float* const o3 = static_cast<float*>(m.lv[3]);
  uint32_t raw[2][6] = {};
  if (U8 && vec) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (y0 + r < H && in_x) {
        const uint8_t* p = static_cast<const uint8_t*>(m.src) + ((i64)(y0 + r) * W + x0) * 3;
        load_pack<uint32_t, 2>(reinterpret_cast<const uint32_t*>(p), &raw[r][0]);
        load_pack<uint32_t, 2>(reinterpret_cast<const uint32_t*>(p) + 2, &raw[r][2]);
        load_pack<uint32_t, 2>(reinterpret_cast<const uint32_t*>(p) + 4, &raw[r][4]);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v[2][8];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int y = y0 + r;
      const bool row_ok = y < H;
      if (U8) {
        if (vec) {
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int b = 3 * i + c;
            v[r][i] = (float)((raw[r][b >> 2] >> (8 * (b & 3))) & 255u) / 255.0f;
          }
        } else {
          const uint8_t* s = static_cast<const uint8_t*>(m.src) + (i64)y * W * 3 + c;
#pragma unroll
          for (int i = 0; i < 8; ++i)
            v[r][i] = (row_ok && x0 + i < W) ? (float)s[(i64)(x0 + i) * 3] / 255.0f : 0.f;
        }
      } else {
        const float* s = static_cast<const float*>(m.src) + c * m.sc + y * m.sy;
        if (vec) {
          if (row_ok && in_x) {
            load_pack<float, 4>(s + x0, &v[r][0]);
            load_pack<float, 4>(s + x0 + 4, &v[r][4]);
          } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[r][i] = 0.f;
          }
        } else {
#pragma unroll
          for (int i = 0; i < 8; ++i) v[r][i] = (row_ok && x0 + i < W) ? s[(x0 + i) * m.sx] : 0.f;
        }
        if (clamp) {                                           // torch.clamp: a NaN fails both comparisons and stays
#pragma unroll
          for (int i = 0; i < 8; ++i) v[r][i] = v[r][i] < 0.f ? 0.f : (v[r][i] > 1.f ? 1.f : v[r][i]);
        }
      }
      if (o0 && row_ok) {
        float* d = o0 + ((i64)c * H + y) * W + x0;
        if (vec) {
          if (in_x) {
            store_pack<float, 4>(d, &v[r][0]);
            store_pack<float, 4>(d + 4, &v[r][4]);
          }
        } else {
#pragma unroll
          for (int i = 0; i < 8; ++i)
            if (x0 + i < W) d[i] = v[r][i];
        }
      }
    }
    float l1[4], p1[4], l2[2], p2[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) l1[i] = half_sum(v[0][2 * i], v[0][2 * i + 1], v[1][2 * i], v[1][2 * i + 1]);
    const int y1 = y0 >> 1, x1 = x0 >> 1;
    if (o1 && y1 < H1) {
      float* d = o1 + ((i64)c * H1 + y1) * W1 + x1;
      if (vec) {
        if (in_x) store_pack<float, 4>(d, l1);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (x1 + i < W1) d[i] = l1[i];
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) p1[i] = __shfl_xor(l1[i], 16, 64);          // the level-1 row below (even ty)
#pragma unroll
    for (int i = 0; i < 2; ++i) l2[i] = half_sum(l1[2 * i], l1[2 * i + 1], p1[2 * i], p1[2 * i + 1]);
    const int y2 = y0 >> 2, x2 = x0 >> 2;
    if (o2 && !(ty & 1) && y2 < H2) {
      float* d = o2 + ((i64)c * H2 + y2) * W2 + x2;
      if (vec) {
        if (in_x) store_pack<float, 2>(d, l2);
      } else {
#pragma unroll
        for (int i = 0; i < 2; ++i)
          if (x2 + i < W2) d[i] = l2[i];
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) p2[i] = __shfl_xor(l2[i], 32, 64);          // the level-2 row below (ty == 0)
    float l3[2];
    l3[0] = half_sum(l2[0], l2[1], p2[0], p2[1]);
    l3[1] = __shfl_xor(l3[0], 1, 64);                                       // the next lane's, for an 8-byte store
    const int y3 = y0 >> 3, x3 = x0 >> 3;
    if (o3 && ty == 0 && y3 < H3) {
      float* d = o3 + ((i64)c * H3 + y3) * W3 + x3;
      if (vec) {
        if (in_x && !(tx & 1)) store_pack<float, 2>(d, l3);
      } else if (x3 < W3) {
        d[0] = l3[0];
      }
    }
  }
}

// depth (fp32, EXACT) and sky mask (bytes): levels 1..3 pick pixels of one of the lane's two rows, nothing is computed
template <typename T, bool EXACT>
__device__ inline void nearest_lane(const MapK& m, int x0, int y0, int tx, int ty) {
  const int H = m.H, W = m.W;
  const bool vec = m.vec != 0, in_x = x0 < W;
  const int y = y0 + (EXACT ? 1 : 0);
  const bool row_ok = y < H;
  T v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = T(0);
  const T* s = static_cast<const T*>(m.src) + y * m.sy;
  if (vec) {
    if (row_ok && in_x) {
      if constexpr (sizeof(T) == 4) {
        load_pack<T, 4>(s + x0, &v[0]);
        load_pack<T, 4>(s + x0 + 4, &v[4]);
      } else {
        load_pack<T, 8>(s + x0, &v[0]);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (row_ok && x0 + i < W) v[i] = s[(x0 + i) * m.sx];
  }
  T next3 = T(0);
  if constexpr (sizeof(T) == 4) next3 = __shfl_xor(v[EXACT ? 7 : 0], 1, 64);
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    const int step = 1 << k, off = EXACT ? step - 1 : 0, n = 8 >> k;
    const int Hk = H >> k, Wk = W >> k, yk = y >> k, xk = x0 >> k;
    T* const o = static_cast<T*>(m.lv[k]);
    if (!o || ((y - off) & (step - 1)) != 0 || yk >= Hk) continue;
    T pick[4] = {T(0), T(0), T(0), T(0)};
#pragma unroll
    for (int i = 0; i < n; ++i) pick[i] = v[off + i * step];
    T* d = o + (i64)yk * Wk + xk;
    if (!vec) {
#pragma unroll
      for (int i = 0; i < n; ++i)
        if (xk + i < Wk) d[i] = pick[i];
    } else if (in_x) {
      if (k == 1) store_pack<T, 4>(d, pick);
      if (k == 2) store_pack<T, 2>(d, pick);
      if (k == 3) {
        if constexpr (sizeof(T) == 4) {
          pick[1] = next3;
          if (!(tx & 1)) store_pack<T, 2>(d, pick);
        } else {
          d[0] = pick[0];
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void pyramid_kernel(PyramidK k) {
  int j = 0;
  while (j + 1 < k.n && (int)blockIdx.x >= k.map[j + 1].tile0) ++j;
  const MapK& m = k.map[j];
  const int t = (int)blockIdx.x - m.tile0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tx = lane & 15, ty = lane >> 4;
  const int x0 = (t % m.tiles_x) * kTileW + 8 * tx;
  const int y0 = (t / m.tiles_x) * kTileH + 8 * wave + 2 * ty;
  switch (m.kind) {                                            // the same for every lane of the workgroup
    case PINGS_CAMFRONT_RGB_U8: bilinear_lane<true>(m, x0, y0, tx, ty); break;
    case PINGS_CAMFRONT_RGB_F32:
    case PINGS_CAMFRONT_NORMAL: bilinear_lane<false>(m, x0, y0, tx, ty); break;
    case PINGS_CAMFRONT_DEPTH: nearest_lane<float, true>(m, x0, y0, tx, ty); break;
    default: nearest_lane<uint8_t, false>(m, x0, y0, tx, ty); break;
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ------------------------------------------------------------------ the fit of the mono depth to the LiDAR depth
constexpr int kBlock = 256;
constexpr int kFitBlocks = 256;                                // workgroups of the partial sums (grid-stride above that)
constexpr int kFitSums = 7;                                    // n, Sx, Sy, Sxx, Sxy, Syy, S(x - y)^2

inline unsigned blocks_for(i64 n) { return (unsigned)((n + kBlock - 1) / kBlock); }

__global__ __launch_bounds__(kBlock) void fit_partial_kernel(const float* __restrict__ pred,
                                                             const float* __restrict__ lidar, i64 n, float lo, float hi,
                                                             double* __restrict__ part) {
  __shared__ double red[kFitSums][kBlock / 64];
  double acc[kFitSums];
#pragma unroll
  for (int k = 0; k < kFitSums; ++k) acc[k] = 0.0;
  for (i64 i = (i64)blockIdx.x * kBlock + threadIdx.x; i < n; i += (i64)gridDim.x * kBlock) {
    const float xf = pred[i], yf = lidar[i];
    if (yf > lo && xf > lo && yf < hi) {                       // slam_dataset.py:370, in fp32 as numpy compares
      const double x = (double)xf, y = (double)yf, e = x - y;
      acc[0] += 1.0; acc[1] += x; acc[2] += y; acc[3] += x * x; acc[4] += x * y; acc[5] += y * y; acc[6] += e * e;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kFitSums; ++k) {
    double s = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);     // a fixed tree: the same sum in every run
    if (lane == 0) red[k][wave] = s;
  }
  __syncthreads();
  if (threadIdx.x < kFitSums) {
    double s = red[threadIdx.x][0];
    for (int w = 1; w < kBlock / 64; ++w) s += red[threadIdx.x][w];
    part[(i64)blockIdx.x * kFitSums + threadIdx.x] = s;
  }
}

// one workgroup: the partials added in index order, then the 2 x 2 normal equations about the means
__global__ __launch_bounds__(64) void fit_solve_kernel(const double* __restrict__ part, int nparts,
                                                       double* __restrict__ rec) {
  __shared__ double tot[kFitSums];
  if (threadIdx.x < kFitSums) {
    double s = 0.0;
    for (int b = 0; b < nparts; ++b) s += part[(i64)b * kFitSums + threadIdx.x];
    tot[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double n = tot[0], Sx = tot[1], Sy = tot[2], Sxx = tot[3], Sxy = tot[4], Syy = tot[5];
  double k = 1.0, b = 0.0, after = NAN;
  if (n > (double)PINGS_CAMFRONT_MIN_FIT) {
    const double mx = Sx / n, my = Sy / n;
    k = (Sxy - n * mx * my) / (Sxx - n * mx * mx);
    b = my - k * mx;
    const double res = Syy - 2.0 * k * Sxy - 2.0 * b * Sy + k * k * Sxx + 2.0 * k * b * Sx + n * b * b;
    after = sqrt(fmax(res, 0.0) / n);
  }
  rec[0] = n;
  rec[1] = k;
  rec[2] = b;
  rec[3] = sqrt(tot[6] / n);                                   // no pixel: 0 / 0 = NaN, as np.mean of nothing
  rec[4] = after;
}

// ------------------------------------------------------------------ the mono-depth cloud of one camera
struct CloudArgs {
  const float* pred;
  const uint8_t* image;
  const double* record;        // DEVICE {count, k, b, ...} or null: k = 1, b = 0
  i64 hw;
  int width, high_z;
  float sky, far, near;        // thresholds, each rounded to fp32 once
  double fx, fy, cx, cy, trunc;
  double T[12];                // camera -> LiDAR, rows of [R | t]
};

// slam_dataset.py:388-436 for one pixel, in the reference's order; every comparison strict, a NaN passes them all
__device__ __forceinline__ float gated_depth(const CloudArgs& a, i64 i, bool* sky) {
  const double k = a.record ? a.record[1] : 1.0, b = a.record ? a.record[2] : 0.0;
  float d = (float)(k * (double)a.pred[i] + b);
  *sky = d > a.sky;
  if (*sky) d = 0.f;
  if (a.high_z && d > a.far) d = 0.f;
  if (d < a.near) d = 0.f;
  return d;
}

__device__ __forceinline__ bool gives_row(const CloudArgs& a, float d) {
  return (double)d > 0.0 && (double)d < a.trunc;               // the rule of pings_eval_backproject
}

__global__ __launch_bounds__(kBlock) void cloud_count_kernel(CloudArgs a, int* __restrict__ cnt) {
  const i64 i = (i64)blockIdx.x * kBlock + threadIdx.x;
  bool sky;
  const bool keep = i < a.hw && gives_row(a, gated_depth(a, i, &sky));
  int tot;
  pings::block_exclusive_scan<kBlock>(keep ? 1 : 0, &tot);
  if (threadIdx.x == 0) cnt[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kBlock) void cloud_emit_kernel(CloudArgs a, const int* __restrict__ off, int nb,
                                                            uint8_t* __restrict__ sky_out, float* __restrict__ gated,
                                                            float* __restrict__ rows, int64_t* __restrict__ count) {
  const i64 i = (i64)blockIdx.x * kBlock + threadIdx.x;
  bool sky = false;
  const float d = i < a.hw ? gated_depth(a, i, &sky) : 0.f;
  const bool keep = i < a.hw && gives_row(a, d);
  int tot;
  const int r0 = pings::block_exclusive_scan<kBlock>(keep ? 1 : 0, &tot);
  if (i == 0) *count = (int64_t)off[nb - 1];
  if (i >= a.hw) return;
  sky_out[i] = sky ? 1 : 0;
  if (gated) gated[i] = d;
  if (!keep) return;
  const i64 o = (i64)(blockIdx.x ? off[blockIdx.x - 1] : 0) + r0;           // o < kept total <= hw
  const double z = (double)d;
  const double u = (double)(i % a.width), v = (double)(i / a.width);
  const double x = (u - a.cx) * z / a.fx, y = (v - a.cy) * z / a.fy;
  float* row = rows + 6 * o;
#pragma unroll
  for (int r = 0; r < 3; ++r)
    row[r] = (float)(a.T[4 * r] * x + a.T[4 * r + 1] * y + a.T[4 * r + 2] * z + a.T[4 * r + 3]);
#pragma unroll
  for (int c = 0; c < 3; ++c) row[3 + c] = (float)((double)a.image[3 * i + c] / 255.0);   // Open3D's uint8 / 255.0
}

struct CloudScratch {
  int *cnt, *off;              // per block: rows kept, their inclusive scan
  void* temp;
  size_t temp_bytes, total;
};
CloudScratch carve_cloud(void* base, i64 hw) {
  pings::Carver c(base);
  CloudScratch s;
  const size_t nb = (size_t)blocks_for(hw);
  s.cnt = c.take<int>(nb);
  s.off = c.take<int>(nb);
  s.temp_bytes = pings::devprim::inclusive_sum_i32_temp_bytes((i64)nb);
  s.temp = c.take<char>(s.temp_bytes);
  s.total = c.total();
  return s;
}

inline bool image_ok(int H, int W) { return H > 0 && W > 0 && (int64_t)H * W < (int64_t)0x7FFFFFF0 / 6; }

}  // namespace

PINGS_API int pings_camfront_pyramid(const pings_camfront_map* maps, int32_t nmaps, int32_t* launches_out,
                                     void* stream) {
  if (launches_out) *launches_out = 0;
  PINGS_ARG_CHECK(maps && nmaps > 0 && nmaps <= kMaxMaps, "1..32 maps");
  PyramidK k;
  k.n = nmaps;
  int tiles = 0;
  for (int j = 0; j < kMaxMaps; ++j) {
    MapK& m = k.map[j];
    if (j >= nmaps) {
      m = MapK{nullptr, {nullptr, nullptr, nullptr, nullptr}, 0, 0, 0, 0, 0, 0, 0, tiles, 1};
      continue;
    }
    const pings_camfront_map& a = maps[j];
    PINGS_ARG_CHECK(a.src, "null pointer in map");
    PINGS_ARG_CHECK(a.kind >= PINGS_CAMFRONT_RGB_U8 && a.kind <= PINGS_CAMFRONT_SKY, "unknown kind of map");
    PINGS_ARG_CHECK(a.H > 0 && a.W > 0 && (int64_t)a.H * a.W < (int64_t)0x7FFFFFF0 / 3, "bad image size");
    const bool planar = a.kind != PINGS_CAMFRONT_RGB_U8;
    PINGS_ARG_CHECK(!planar || (a.stride_y >= 0 && a.stride_x >= 0 && a.stride_c >= 0), "negative stride");
    m.src = a.src;
    m.lv[0] = a.l0; m.lv[1] = a.l1; m.lv[2] = a.l2; m.lv[3] = a.l3;
    m.sc = planar ? a.stride_c : 1;
    m.sy = planar ? a.stride_y : 3 * (i64)a.W;
    m.sx = planar ? a.stride_x : 3;
    m.H = a.H;
    m.W = a.W;
    m.kind = a.kind;
    bool vec = a.W % 16 == 0 && aligned16(a.src) && aligned16(a.l0) && aligned16(a.l1) && aligned16(a.l2) &&
               aligned16(a.l3);
    if (planar) vec = vec && a.stride_x == 1 && a.stride_y % 16 == 0 && a.stride_c % 16 == 0;
    m.vec = vec ? 1 : 0;
    m.tile0 = tiles;
    m.tiles_x = (a.W + kTileW - 1) / kTileW;
    tiles += m.tiles_x * ((a.H + kTileH - 1) / kTileH);
  }
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("camfront_pyramid", st);
  if (int e = pings::launch(pyramid_kernel, dim3((unsigned)tiles), 256, 0, st, k)) return e;
  if (launches_out) *launches_out = 1;
  return PINGS_OK;
}

PINGS_API size_t pings_camfront_align_scratch_bytes(void) {
  pings::Carver c(nullptr);
  c.take<double>((size_t)kFitBlocks * kFitSums);
  return c.total();
}

PINGS_API int pings_camfront_align(const float* pred, const float* lidar_depth, int64_t n, double min_range,
                                   double max_range, void* scratch, double* record, void* stream) {
  PINGS_ARG_CHECK(pred && lidar_depth && scratch && record, "null pointer");
  PINGS_ARG_CHECK(n > 0 && n < (int64_t)0x7FFFFFF0, "empty or oversized image");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("camfront_align", st);
  pings::Carver c(scratch);
  double* part = c.take<double>((size_t)kFitBlocks * kFitSums);
  const unsigned nb = blocks_for(n) < (unsigned)kFitBlocks ? blocks_for(n) : (unsigned)kFitBlocks;
  if (int e = pings::launch(fit_partial_kernel, dim3(nb), kBlock, 0, st, pred, lidar_depth, (i64)n, (float)min_range,
                            (float)(0.8 * max_range), part))
    return e;
  return pings::launch(fit_solve_kernel, dim3(1), 64, 0, st, (const double*)part, (int)nb, record);
}

PINGS_API size_t pings_camfront_cloud_scratch_bytes(int64_t hw) {
  return hw > 0 && hw < (int64_t)0x7FFFFFF0 / 6 ? carve_cloud(nullptr, hw).total : 0;
}

PINGS_API int pings_camfront_mono_cloud(const float* pred, const uint8_t* image, int32_t H, int32_t W,
                                        const double* record, const double* intrinsic, const double* cam_to_lidar,
                                        double min_range, double max_range, double depth_trunc, int32_t high_z,
                                        void* scratch, uint8_t* sky, float* gated, float* rows, int64_t* count,
                                        void* stream) {
  PINGS_ARG_CHECK(pred && image && intrinsic && cam_to_lidar && scratch && sky && rows && count, "null pointer");
  PINGS_ARG_CHECK(image_ok(H, W), "empty or oversized image");
  PINGS_ARG_CHECK(intrinsic[0] != 0.0 && intrinsic[1] != 0.0, "zero focal length");
  hipStream_t st = pings::as_stream(stream);
  CloudArgs a{};
  a.pred = pred;
  a.image = image;
  a.record = record;
  a.hw = (i64)H * W;
  a.width = W;
  a.high_z = high_z ? 1 : 0;
  a.sky = (float)(1.2 * max_range);
  a.far = (float)(0.8 * max_range);
  a.near = high_z ? (float)(2.0 * min_range) : (float)(0.2 * max_range);
  a.fx = intrinsic[0]; a.fy = intrinsic[1]; a.cx = intrinsic[2]; a.cy = intrinsic[3];
  a.trunc = depth_trunc;
  for (int k = 0; k < 12; ++k) a.T[k] = cam_to_lidar[k];
  const int nb = (int)blocks_for(a.hw);
  const CloudScratch s = carve_cloud(scratch, a.hw);
  pings::prof::Scope ps("camfront_mono_cloud", st);
  if (int e = pings::launch(cloud_count_kernel, dim3(nb), kBlock, 0, st, a, s.cnt)) return e;
  if (int e = pings::devprim::inclusive_sum_i32(s.temp, s.temp_bytes, s.cnt, s.off, nb, st)) return e;
  return pings::launch(cloud_emit_kernel, dim3(nb), kBlock, 0, st, a, (const int*)s.off, nb, sky, gated, rows, count);
}
