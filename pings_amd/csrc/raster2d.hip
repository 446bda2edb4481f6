// 2D Gaussian splatting (ray-splat intersection) rasteriser, forward and backward, for gfx950.
//
// The `diff_surfel_rasterization` backend of the reference (gaussian_renderer/__init__.py:88-89,167-181,349-409).
// Semantics: Huang et al., "2D Gaussian Splatting for Geometrically Accurate Radiance Fields" (SIGGRAPH 2024), as
// restated in tests/raster2d_ref.py and DESIGN.md §2.1b / §3 (assumptions 2D-1 .. 2D-9).
//
// Pipeline (one stream; one host read-back, the instance count):
//   preprocess2d_kernel   per Gaussian: splat-to-pixel matrix T (3x3), screen centre mu, radius, published getRect
//                         square, camera-frame normal, fp32 depth key                          [44 B in, 112 B out]
//   inclusive scan        tiles per Gaussian (Gaussian-index order) -> instance slots
//   duplicate2d_kernel    one (tile << 32 | depth bits, slot) pair per covered tile                     [12 B out]
//   radix sort (I)        64-bit keys, 32 + ceil(log2 tiles) bits; radix sort is stable, so ties of (tile, depth)
//                         stay in slot order = Gaussian index order
//   tile_ranges2d_kernel  [start, end) of every tile
//   blend2d_fwd_kernel    one 256-thread workgroup per 16x16 tile, one wave per 8x8 quadrant; 256 records per round
//                         staged in LDS; front to back; writes image, allmap[7], final T, last / median contributor and
//                         the final M1 / M2 the backward pass needs for the distortion term
//   blend2d_bwd_kernel    same geometry, back to front; one 18-float gradient row per (instance, wave), summed over
//                         the wave with DPP (no float atomics)
//   fold2d_kernel         per instance: the four wave rows -> one row (fixed order)
//   gaussian_sum2d_kernel per (Gaussian, column): its instances' rows, in slot order
//   gaussian2d_bwd_kernel per Gaussian: (T, mu, n_c) -> (p, t_u, t_v, n) -> means3D, scales, rotations
//
// The preprocess arithmetic follows tests/raster2d_ref.py:preprocess32 op for op (-ffp-contract=off, IEEE divide /
// sqrt), so radii, tile squares and sort order match the fp32 restatement bit for bit.  The forward and backward
// blend kernels evaluate a (pixel, splat) pair through the same inline function, so both take the same skip / stop /
// branch decisions.
#include <algorithm>

#include "devprim.hpp"
#include "raster_common.hpp"

namespace pings {
namespace raster2d {

using raster::wave_reduce_sum_dpp;

constexpr int TILE = 16;
constexpr int BLOCK = TILE * TILE;
constexpr float NEAR_Z = 0.2f;
constexpr float FAR_Z = 100.0f;
constexpr float ALPHA_MAX = 0.99f;
constexpr float ALPHA_MIN = 1.0f / 255.0f;
constexpr float T_EPS = 1e-4f;
constexpr float CUTOFF2 = 9.0f;                   // c^2, c = 3
constexpr float FILTER_R = 2.12132034f;           // c sqrt(2) / 2: smallest radius of the published rule
constexpr float LOWPASS_INV2 = 2.0f;              // rho2 = 2 |mu - pixel|^2
constexpr uint32_t CULLED_KEY = 0xFFFFFFFFu;
constexpr int REC = 5;                            // float4 per record
constexpr int GROW = 18;                          // floats per gradient row
// gradient row: dT[9] (row-major), dmu[2], dopacity, dcolour[3], dnormal[3]
enum { R_T = 0, R_MX = 9, R_MY = 10, R_O = 11, R_C = 12, R_N = 15 };

struct Params {
  int P, W, H, gx, gy;
  float scale_mod;
  const float* view;
  const float* proj;
  const float* bg;
  const int32_t* live;
  int dyn_rows;
};

struct Geom {
  float4* rec;         // [P][5] {T00 T01 T02 T10} {T11 T12 T20 T21} {T22 mx my opacity} {r g b ncx} {ncy ncz sign -}
  uint4* rect;         // [P] xmin, ymin, xmax, ymax (tiles)
  uint32_t* tiles;     // [P] tiles of the square (0 = culled)
  uint32_t* offsets;   // [P] inclusive scan of tiles
  uint32_t* key;       // [P] fp32 view depth bits
  unsigned long long* count;  // [1] instance count in 64 bits (what the read-back fetches: the uint32 scan may wrap)
  void* temp;
  size_t temp_bytes;
  size_t total;
};

struct Bins {
  unsigned long long *keys, *keys_sorted;
  uint32_t *slots, *point_list;   // point_list[i] = slot of the i-th instance in (tile, depth, index) order
  uint32_t* slot_g;               // [I] Gaussian of every slot
  uint2* ranges;                  // [num_tiles]
  void* temp;
  size_t temp_bytes;
  size_t total;
};

struct Img {
  float* final_T;
  uint32_t* n_contrib;  // list position (relative to the tile range) + 1 of the last blended pair
  int32_t* median;      // list position of the median contributor, -1 = none
  float *M1, *M2;       // final sums of w m and w m^2 (distortion backward)
  size_t total;
};

static int tile_bits(int nt) {
  int b = 1;
  while ((1 << b) < nt) ++b;
  return b;
}

static Geom carve_geom(void* blob, int P) {
  Carver c(blob);
  Geom g;
  const size_t n = (size_t)(P > 0 ? P : 1);
  g.rec = c.take<float4>(REC * n);
  g.rect = c.take<uint4>(n);
  g.tiles = c.take<uint32_t>(n);
  g.offsets = c.take<uint32_t>(n);
  g.key = c.take<uint32_t>(n);
  g.count = c.take<unsigned long long>(1);
  g.temp_bytes = devprim::inclusive_sum_u32_temp_bytes(P);
  g.temp = c.take<char>(g.temp_bytes);
  g.total = c.total();
  return g;
}

static Bins carve_bins(void* blob, int64_t I, int nt) {
  Carver c(blob);
  Bins b;
  const size_t n = (size_t)(I > 0 ? I : 1);
  b.keys = c.take<unsigned long long>(n);
  b.keys_sorted = c.take<unsigned long long>(n);
  b.slots = c.take<uint32_t>(n);
  b.point_list = c.take<uint32_t>(n);
  b.slot_g = c.take<uint32_t>(n);
  b.ranges = c.take<uint2>((size_t)nt);
  b.temp_bytes = devprim::sort_pairs_u64_u32_temp_bytes(I);
  b.temp = c.take<char>(b.temp_bytes);
  b.total = c.total();
  return b;
}

static Img carve_img(void* blob, int W, int H) {
  Carver c(blob);
  Img im;
  const size_t n = (size_t)W * H;
  im.final_T = c.take<float>(n);
  im.n_contrib = c.take<uint32_t>(n);
  im.median = c.take<int32_t>(n);
  im.M1 = c.take<float>(n);
  im.M2 = c.take<float>(n);
  im.total = c.total();
  return im;
}

struct Bwd {
  float *parts, *rows, *gsum;   // gradient rows per (instance, wave), per instance, per Gaussian
  size_t total;
};

static Bwd carve_bwd(void* blob, int P, int64_t I) {
  Carver c(blob);
  Bwd b;
  const size_t n = (size_t)(I > 0 ? I : 1);
  b.parts = c.take<float>(n * 4 * GROW);
  b.rows = c.take<float>(n * GROW);
  b.gsum = c.take<float>((size_t)(P > 0 ? P : 1) * GROW);
  b.total = c.total();
  return b;
}

// ---------------------------------------------------------------- preprocess
// clip-space row (a, a3) . projmatrix, then the clip-to-pixel map N: (u w, v w, w)
__device__ inline void to_pixel_h(const float* __restrict__ Pm, float a0, float a1, float a2, bool homog, float hw,
                                  float hw1, float hh, float hh1, float& h0, float& h1, float& h2) {
  float c0 = (a0 * Pm[0] + a1 * Pm[4]) + a2 * Pm[8];
  float c1 = (a0 * Pm[1] + a1 * Pm[5]) + a2 * Pm[9];
  float c3 = (a0 * Pm[3] + a1 * Pm[7]) + a2 * Pm[11];
  if (homog) {
    c0 = c0 + Pm[12];
    c1 = c1 + Pm[13];
    c3 = c3 + Pm[15];
  }
  h0 = hw * c0 + hw1 * c3;
  h1 = hh * c1 + hh1 * c3;
  h2 = c3;
}

__device__ inline int rect_lo(float v, int g) {   // published getRect lower bound: (int) truncation, clamped
  return v <= 0.0f ? 0 : (v >= (float)g ? g : (int)v);
}

__global__ __launch_bounds__(256) void preprocess2d_kernel(
    Params p, const float* __restrict__ means3D, const float* __restrict__ colors,
    const float* __restrict__ opacities, const float* __restrict__ scales, const float* __restrict__ rotations,
    float4* __restrict__ rec, uint4* __restrict__ rect, uint32_t* __restrict__ tiles_out,
    uint32_t* __restrict__ key_out, int32_t* __restrict__ radii) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= p.P) return;
  const float* V = p.view;
  const float* Pm = p.proj;
  uint32_t key = CULLED_KEY, tiles = 0u;
  uint4 rc = make_uint4(0u, 0u, 0u, 0u);
  int rad = 0;

  const float x = means3D[3 * g], y = means3D[3 * g + 1], z = means3D[3 * g + 2];
  const float px = ((V[0] * x + V[4] * y) + V[8] * z) + V[12];
  const float py = ((V[1] * x + V[5] * y) + V[9] * z) + V[13];
  const float pz = ((V[2] * x + V[6] * y) + V[10] * z) + V[14];
  bool ok = pz > NEAR_Z;
  if (p.live && g < p.dyn_rows && g >= *p.live) ok = false;   // rows behind the producer's device count

  const float qr = rotations[4 * g], qx = rotations[4 * g + 1], qy = rotations[4 * g + 2], qz = rotations[4 * g + 3];
  const float R00 = 1.0f - 2.0f * (qy * qy + qz * qz), R01 = 2.0f * (qx * qy - qr * qz),
              R02 = 2.0f * (qx * qz + qr * qy);
  const float R10 = 2.0f * (qx * qy + qr * qz), R11 = 1.0f - 2.0f * (qx * qx + qz * qz),
              R12 = 2.0f * (qy * qz - qr * qx);
  const float R20 = 2.0f * (qx * qz - qr * qy), R21 = 2.0f * (qy * qz + qr * qx),
              R22 = 1.0f - 2.0f * (qx * qx + qy * qy);
  const float s0 = p.scale_mod * scales[2 * g], s1 = p.scale_mod * scales[2 * g + 1];

  const float hw = 0.5f * (float)p.W, hw1 = 0.5f * ((float)p.W - 1.0f);
  const float hh = 0.5f * (float)p.H, hh1 = 0.5f * ((float)p.H - 1.0f);
  float T[9];
  to_pixel_h(Pm, R00 * s0, R10 * s0, R20 * s0, false, hw, hw1, hh, hh1, T[0], T[1], T[2]);
  to_pixel_h(Pm, R01 * s1, R11 * s1, R21 * s1, false, hw, hw1, hh, hh1, T[3], T[4], T[5]);
  to_pixel_h(Pm, x, y, z, true, hw, hw1, hh, hh1, T[6], T[7], T[8]);

  // centre and extent of the c = 3 bounding quadric (t = (c^2, c^2, -1))
  const float d = (CUTOFF2 * (T[2] * T[2]) + CUTOFF2 * (T[5] * T[5])) + (-1.0f) * (T[8] * T[8]);
  ok = ok && d != 0.0f;
  const float dd = d != 0.0f ? d : 1.0f;
  const float f0 = CUTOFF2 / dd, f1 = CUTOFF2 / dd, f2 = -1.0f / dd;
  const float mx = ((f0 * T[0]) * T[2] + (f1 * T[3]) * T[5]) + (f2 * T[6]) * T[8];
  const float my = ((f0 * T[1]) * T[2] + (f1 * T[4]) * T[5]) + (f2 * T[7]) * T[8];
  const float sx = ((f0 * T[0]) * T[0] + (f1 * T[3]) * T[3]) + (f2 * T[6]) * T[6];
  const float sy = ((f0 * T[1]) * T[1] + (f1 * T[4]) * T[4]) + (f2 * T[7]) * T[7];
  const float ex = sqrtf(fmaxf(1e-4f, mx * mx - sx));
  const float ey = sqrtf(fmaxf(1e-4f, my * my - sy));
  const float radius = ceilf(fmaxf(fmaxf(ex, ey), FILTER_R));
  ok = ok && isfinite(mx) && isfinite(my) && isfinite(radius);

  // camera-frame normal, flipped towards the camera
  float nx = (V[0] * R02 + V[4] * R12) + V[8] * R22;
  float ny = (V[1] * R02 + V[5] * R12) + V[9] * R22;
  float nz = (V[2] * R02 + V[6] * R12) + V[10] * R22;
  const float cosv = (nx * px + ny * py) + nz * pz;
  ok = ok && cosv != 0.0f;
  const float sign = cosv > 0.0f ? -1.0f : 1.0f;
  nx = sign * nx; ny = sign * ny; nz = sign * nz;

  if (ok) {
    const int xmin = rect_lo((mx - radius) / (float)TILE, p.gx);
    const int ymin = rect_lo((my - radius) / (float)TILE, p.gy);
    const int xmax = rect_lo(((mx + radius) + (float)(TILE - 1)) / (float)TILE, p.gx);
    const int ymax = rect_lo(((my + radius) + (float)(TILE - 1)) / (float)TILE, p.gy);
    const int nt = (xmax - xmin) * (ymax - ymin);
    if (nt > 0) {
      key = __float_as_uint(pz);
      tiles = (uint32_t)nt;
      rc = make_uint4((uint32_t)xmin, (uint32_t)ymin, (uint32_t)xmax, (uint32_t)ymax);
      rad = (int)radius;
      rec[REC * g + 0] = make_float4(T[0], T[1], T[2], T[3]);
      rec[REC * g + 1] = make_float4(T[4], T[5], T[6], T[7]);
      rec[REC * g + 2] = make_float4(T[8], mx, my, opacities[g]);
      rec[REC * g + 3] = make_float4(colors[3 * g], colors[3 * g + 1], colors[3 * g + 2], nx);
      rec[REC * g + 4] = make_float4(ny, nz, sign, 0.0f);
    }
  }
  key_out[g] = key;
  tiles_out[g] = tiles;
  rect[g] = rc;
  radii[g] = rad;
}

__global__ __launch_bounds__(256) void duplicate2d_kernel(int P, int gx, const uint4* __restrict__ rect,
                                                           const uint32_t* __restrict__ tiles,
                                                           const uint32_t* __restrict__ offsets,
                                                           const uint32_t* __restrict__ key,
                                                           unsigned long long* __restrict__ keys,
                                                           uint32_t* __restrict__ slots, uint32_t* __restrict__ slot_g) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= P) return;
  const uint32_t n = tiles[g];
  if (n == 0u) return;
  const uint4 r = rect[g];
  uint32_t s = offsets[g] - n;
  const unsigned long long k = (unsigned long long)key[g];
  for (uint32_t ty = r.y; ty < r.w; ++ty)
    for (uint32_t tx = r.x; tx < r.z; ++tx) {
      keys[s] = ((unsigned long long)(ty * (uint32_t)gx + tx) << 32) | k;
      slots[s] = s;
      slot_g[s] = (uint32_t)g;
      ++s;
    }
}

__global__ __launch_bounds__(256) void tile_ranges2d_kernel(int64_t I, const unsigned long long* __restrict__ keys,
                                                             uint2* __restrict__ ranges) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= I) return;
  const uint32_t t = (uint32_t)(keys[i] >> 32);
  if (i == 0 || (uint32_t)(keys[i - 1] >> 32) != t) ranges[t].x = (uint32_t)i;
  if (i == I - 1 || (uint32_t)(keys[i + 1] >> 32) != t) ranges[t].y = (uint32_t)(i + 1);
}

// Sum of tiles[] in 64 bits (integer atomics: order independent).  The instance offsets are a uint32 scan; a total at or
// beyond 2^31 (the sort's int range) is refused from this sum, which a wrapped scan could not reveal.
__global__ __launch_bounds__(256) void total2d_kernel(int P, const uint32_t* __restrict__ tiles,
                                                     unsigned long long* __restrict__ out) {
  __shared__ unsigned long long s;
  if (threadIdx.x == 0) s = 0ull;
  __syncthreads();
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < P && tiles[g]) atomicAdd(&s, (unsigned long long)tiles[g]);
  __syncthreads();
  if (threadIdx.x == 0 && s) atomicAdd(out, s);
}

// ---------------------------------------------------------------- one (pixel, splat) pair
struct Pair {
  float k0, k1, k2, l0, l1, l2;   // k = x T_w - T_u, l = y T_w - T_v
  float iqz, su, sv;              // 1 / q_z, splat-plane coordinates of the ray's hit
  float dx, dy;                   // mu - pixel
  bool on_splat;                  // rho3 <= rho2 (ray-splat branch)
  float depth, G, alpha;
  bool clamped;                   // alpha hit ALPHA_MAX
};

// false = the pair is skipped (q_z = 0, depth < near, power > 0, alpha < 1/255)
__device__ __forceinline__ bool eval_pair(const float* __restrict__ t, float mx, float my, float opac, float x,
                                          float y, Pair& e) {
  e.k0 = x * t[2] - t[0]; e.k1 = x * t[5] - t[3]; e.k2 = x * t[8] - t[6];
  e.l0 = y * t[2] - t[1]; e.l1 = y * t[5] - t[4]; e.l2 = y * t[8] - t[7];
  const float qx = e.k1 * e.l2 - e.k2 * e.l1;
  const float qy = e.k2 * e.l0 - e.k0 * e.l2;
  const float qz = e.k0 * e.l1 - e.k1 * e.l0;
  if (qz == 0.0f) return false;
  e.iqz = 1.0f / qz;
  e.su = qx * e.iqz;
  e.sv = qy * e.iqz;
  const float rho3 = e.su * e.su + e.sv * e.sv;
  e.dx = mx - x;
  e.dy = my - y;
  const float rho2 = LOWPASS_INV2 * (e.dx * e.dx + e.dy * e.dy);
  e.on_splat = rho3 <= rho2;
  const float rho = e.on_splat ? rho3 : rho2;
  e.depth = e.on_splat ? (e.su * t[2] + e.sv * t[5]) + t[8] : t[8];
  if (!(e.depth >= NEAR_Z)) return false;
  const float power = -0.5f * rho;
  if (power > 0.0f) return false;
  e.G = expf(power);
  const float a = opac * e.G;
  e.clamped = a > ALPHA_MAX;
  e.alpha = e.clamped ? ALPHA_MAX : a;
  return e.alpha >= ALPHA_MIN;
}

__device__ __forceinline__ float map_m(float depth) {   // NDC-like depth of the distortion term
  return (FAR_Z / (FAR_Z - NEAR_Z)) * (1.0f - NEAR_Z / depth);
}

struct SharedRec {
  float4 r[REC][BLOCK];
  uint32_t slot[BLOCK];
};

__device__ inline void stage_records(SharedRec& sh, const float4* __restrict__ rec, const uint32_t* __restrict__ list,
                                     const uint32_t* __restrict__ slot_g, uint32_t begin, uint32_t j, uint32_t end) {
  const int tid = threadIdx.x;
  if (j < end) {
    const uint32_t slot = list[begin + j];
    const uint32_t g = slot_g[slot];
    sh.slot[tid] = slot;
#pragma unroll
    for (int c = 0; c < REC; ++c) sh.r[c][tid] = rec[(size_t)REC * g + c];
  }
}

__device__ inline void load_t(const SharedRec& sh, int k, float (&t)[9], float& mx, float& my, float& o) {
  const float4 a = sh.r[0][k], b = sh.r[1][k], c = sh.r[2][k];
  t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w;
  t[4] = b.x; t[5] = b.y; t[6] = b.z; t[7] = b.w;
  t[8] = c.x; mx = c.y; my = c.z; o = c.w;
}

// pixel of thread `tid`: wave w owns the 8x8 quadrant (w & 1, w >> 1) of the tile
__device__ inline void pixel_of(int tile, int gx, int& px, int& py) {
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  px = (tile % gx) * TILE + 8 * (w & 1) + (lane & 7);
  py = (tile / gx) * TILE + 8 * (w >> 1) + (lane >> 3);
}

// ---------------------------------------------------------------- forward blend
__global__ __launch_bounds__(BLOCK) void blend2d_fwd_kernel(int W, int H, int gx, const float* __restrict__ bg,
                                                            const uint2* __restrict__ ranges,
                                                            const uint32_t* __restrict__ list,
                                                            const uint32_t* __restrict__ slot_g,
                                                            const float4* __restrict__ rec, Img im,
                                                            float* __restrict__ out_color,
                                                            float* __restrict__ out_all) {
  __shared__ SharedRec sh;
  const int tile = blockIdx.x;
  int px, py;
  pixel_of(tile, gx, px, py);
  const bool inside = px < W && py < H;
  const uint2 rg = ranges[tile];
  const uint32_t n = rg.y - rg.x;
  const float x = (float)px, y = (float)py;

  bool done = !inside;
  float T = 1.0f, C0 = 0.f, C1 = 0.f, C2 = 0.f, D = 0.f, N0 = 0.f, N1 = 0.f, N2 = 0.f;
  float dist = 0.f, M1 = 0.f, M2 = 0.f, med_depth = 0.f;
  int med = -1;
  uint32_t last = 0u;
  for (uint32_t b = 0; b < n; b += BLOCK) {
    if (__syncthreads_count(done) == BLOCK) break;
    stage_records(sh, rec, list, slot_g, rg.x, b + threadIdx.x, n);
    __syncthreads();
    const int cnt = (int)min((uint32_t)BLOCK, n - b);
    for (int k = 0; k < cnt && !done; ++k) {
      float t[9], mx, my, o;
      load_t(sh, k, t, mx, my, o);
      Pair e;
      if (!eval_pair(t, mx, my, o, x, y, e)) continue;
      const float test_T = T * (1.0f - e.alpha);
      if (test_T < T_EPS) { done = true; break; }
      const float w = e.alpha * T;
      const float4 cr = sh.r[3][k], nr = sh.r[4][k];
      const float m = map_m(e.depth);
      const float A = 1.0f - T;
      C0 += w * cr.x; C1 += w * cr.y; C2 += w * cr.z;
      D += w * e.depth;
      N0 += w * cr.w; N1 += w * nr.x; N2 += w * nr.y;
      dist += w * ((m * m * A + M2) - 2.0f * m * M1);
      M1 += w * m;
      M2 += w * m * m;
      if (T > 0.5f) { med_depth = e.depth; med = (int)(b + k); }
      T = test_T;
      last = b + k + 1;
    }
  }
  if (!inside) return;
  const size_t HW = (size_t)W * H, pix = (size_t)py * W + px;
  im.final_T[pix] = T;
  im.n_contrib[pix] = last;
  im.median[pix] = med;
  im.M1[pix] = M1;
  im.M2[pix] = M2;
  out_color[pix] = C0 + T * bg[0];
  out_color[HW + pix] = C1 + T * bg[1];
  out_color[2 * HW + pix] = C2 + T * bg[2];
  out_all[pix] = D;
  out_all[HW + pix] = 1.0f - T;
  out_all[2 * HW + pix] = N0;
  out_all[3 * HW + pix] = N1;
  out_all[4 * HW + pix] = N2;
  out_all[5 * HW + pix] = med_depth;
  out_all[6 * HW + pix] = dist;
}

// ---------------------------------------------------------------- backward blend
__device__ inline float g_at(const float* __restrict__ g, size_t off) { return g ? g[off] : 0.0f; }

__global__ __launch_bounds__(BLOCK) void blend2d_bwd_kernel(int W, int H, int gx, const float* __restrict__ bg,
                                                            const uint2* __restrict__ ranges,
                                                            const uint32_t* __restrict__ list,
                                                            const uint32_t* __restrict__ slot_g,
                                                            const float4* __restrict__ rec, Img im,
                                                            const float* __restrict__ dL_dcolor,
                                                            const float* __restrict__ dL_dall,
                                                            float* __restrict__ parts) {
  __shared__ SharedRec sh;
  __shared__ int s_last[BLOCK / 64 + 1];
  const int tile = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int px, py;
  pixel_of(tile, gx, px, py);
  const bool inside = px < W && py < H;
  const uint2 rg = ranges[tile];
  const float x = (float)px, y = (float)py;
  const size_t HW = (size_t)W * H, pix = inside ? (size_t)py * W + px : 0;

  float T = 1.0f, M1 = 0.f, M2 = 0.f, gC0 = 0.f, gC1 = 0.f, gC2 = 0.f, gD = 0.f, gA = 0.f;
  float gN0 = 0.f, gN1 = 0.f, gN2 = 0.f, gMed = 0.f, gDist = 0.f;
  int last = 0, med = -1;
  if (inside) {
    T = im.final_T[pix];
    last = (int)im.n_contrib[pix];
    med = im.median[pix];
    M1 = im.M1[pix];
    M2 = im.M2[pix];
    gC0 = g_at(dL_dcolor, pix); gC1 = g_at(dL_dcolor, HW + pix); gC2 = g_at(dL_dcolor, 2 * HW + pix);
    gD = g_at(dL_dall, pix); gA = g_at(dL_dall, HW + pix);
    gN0 = g_at(dL_dall, 2 * HW + pix); gN1 = g_at(dL_dall, 3 * HW + pix); gN2 = g_at(dL_dall, 4 * HW + pix);
    gMed = g_at(dL_dall, 5 * HW + pix); gDist = g_at(dL_dall, 6 * HW + pix);
  }
  if (tid <= BLOCK / 64) s_last[tid] = 0;
  __syncthreads();
  atomicMax(&s_last[wave], last);
  atomicMax(&s_last[BLOCK / 64], last);
  __syncthreads();
  const int wave_last = s_last[wave];
  const int block_last = s_last[BLOCK / 64];
  const float A = 1.0f - T;                        // sum of the blend weights
  float S = (gC0 * bg[0] + gC1 * bg[1]) + gC2 * bg[2];   // d(outputs behind the pair) / d(its transmittance)
  constexpr float MK = FAR_Z / (FAR_Z - NEAR_Z);

  for (int b = block_last > 0 ? ((block_last - 1) / BLOCK) * BLOCK : -1; b >= 0; b -= BLOCK) {
    __syncthreads();
    stage_records(sh, rec, list, slot_g, rg.x, (uint32_t)(b + tid), (uint32_t)block_last);
    __syncthreads();
    const int top = min(BLOCK, block_last - b) - 1;
    for (int k = top; k >= 0; --k) {
      const int j = b + k;
      if (j >= wave_last) continue;              // wave-uniform
      float gr[GROW];
#pragma unroll
      for (int c = 0; c < GROW; ++c) gr[c] = 0.f;
      float t[9], mx, my, o;
      load_t(sh, k, t, mx, my, o);
      Pair e;
      const bool hit = j < last && eval_pair(t, mx, my, o, x, y, e);
      if (hit) {
        T = T / (1.0f - e.alpha);                  // transmittance in front of the pair
        const float w = e.alpha * T;
        const float4 cr = sh.r[3][k], nr = sh.r[4][k];
        const float m = map_m(e.depth);
        gr[R_C] = gC0 * w; gr[R_C + 1] = gC1 * w; gr[R_C + 2] = gC2 * w;
        gr[R_N] = gN0 * w; gr[R_N + 1] = gN1 * w; gr[R_N + 2] = gN2 * w;
        const float em = (M2 + A * m * m) - 2.0f * M1 * m;   // d dist / d w of this pair
        const float Gi = ((((gC0 * cr.x + gC1 * cr.y) + gC2 * cr.z) + gD * e.depth) +
                          ((gN0 * cr.w + gN1 * nr.x) + gN2 * nr.y)) + (gA + gDist * em);
        const float dL_dalpha = T * (Gi - S);
        S = e.alpha * Gi + (1.0f - e.alpha) * S;
        float dL_ddepth = w * gD + gDist * (2.0f * w * (m * A - M1)) * (MK * NEAR_Z / (e.depth * e.depth));
        if (j == med) dL_ddepth += gMed;
        float dL_drho = 0.f;
        if (!e.clamped) {
          gr[R_O] = e.G * dL_dalpha;
          dL_drho = -0.5f * e.alpha * dL_dalpha;
        }
        if (e.on_splat) {
          gr[R_T + 2] += dL_ddepth * e.su;
          gr[R_T + 5] += dL_ddepth * e.sv;
          gr[R_T + 8] += dL_ddepth;
          const float gsu = 2.0f * e.su * dL_drho + dL_ddepth * t[2];
          const float gsv = 2.0f * e.sv * dL_drho + dL_ddepth * t[5];
          const float gq0 = gsu * e.iqz, gq1 = gsv * e.iqz, gq2 = -(gsu * e.su + gsv * e.sv) * e.iqz;
          // q = k x l:  dL/dk = l x gq,  dL/dl = gq x k
          const float gk0 = e.l1 * gq2 - e.l2 * gq1, gk1 = e.l2 * gq0 - e.l0 * gq2, gk2 = e.l0 * gq1 - e.l1 * gq0;
          const float gl0 = gq1 * e.k2 - gq2 * e.k1, gl1 = gq2 * e.k0 - gq0 * e.k2, gl2 = gq0 * e.k1 - gq1 * e.k0;
          gr[R_T + 0] -= gk0; gr[R_T + 3] -= gk1; gr[R_T + 6] -= gk2;
          gr[R_T + 1] -= gl0; gr[R_T + 4] -= gl1; gr[R_T + 7] -= gl2;
          gr[R_T + 2] += x * gk0 + y * gl0;
          gr[R_T + 5] += x * gk1 + y * gl1;
          gr[R_T + 8] += x * gk2 + y * gl2;
        } else {
          gr[R_T + 8] += dL_ddepth;
          gr[R_MX] = 4.0f * e.dx * dL_drho;
          gr[R_MY] = 4.0f * e.dy * dL_drho;
        }
      }
      if (__builtin_amdgcn_ballot_w64(hit) != 0ull) {   // wave-uniform
        float* row = parts + ((size_t)sh.slot[k] * 4 + (size_t)wave) * GROW;
#pragma unroll
        for (int c = 0; c < GROW; ++c) {
          const float v = wave_reduce_sum_dpp(gr[c]);
          if (lane == 63) row[c] = v;
        }
      }
    }
  }
}

// ---------------------------------------------------------------- per-Gaussian sums and chain
__global__ __launch_bounds__(256) void fold2d_kernel(int64_t I, const float* __restrict__ parts,
                                                      float* __restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= I * GROW) return;
  const int64_t s = i / GROW, c = i - s * GROW;
  const float* p = parts + s * 4 * GROW + c;
  rows[i] = (p[0] + p[GROW]) + (p[2 * GROW] + p[3 * GROW]);
}

__global__ __launch_bounds__(256) void gaussian_sum2d_kernel(int P, const uint32_t* __restrict__ tiles,
                                                              const uint32_t* __restrict__ offsets,
                                                              const float* __restrict__ rows,
                                                              float* __restrict__ gsum) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)P * GROW) return;
  const int g = (int)(i / GROW), c = (int)(i - (int64_t)g * GROW);
  const uint32_t end = offsets[g], beg = end - tiles[g];
  float a0 = 0.f, a1 = 0.f;
  uint32_t s = beg;
  for (; s + 2 <= end; s += 2) {
    a0 += rows[(size_t)s * GROW + c];
    a1 += rows[(size_t)(s + 1) * GROW + c];
  }
  if (s < end) a0 += rows[(size_t)s * GROW + c];
  gsum[i] = a0 + a1;
}

__global__ __launch_bounds__(256) void gaussian2d_bwd_kernel(
    Params p, const float* __restrict__ scales, const float* __restrict__ rotations,
    const uint32_t* __restrict__ tiles, const float4* __restrict__ rec, const float* __restrict__ gsum,
    float* __restrict__ dL_dmeans3D, float* __restrict__ dL_dmeans2D, float* __restrict__ dL_dcolors,
    float* __restrict__ dL_dopac, float* __restrict__ dL_dscales, float* __restrict__ dL_drot) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= p.P) return;
  if (tiles[g] == 0u) {   // culled: no instance, every gradient is zero
#pragma unroll
    for (int c = 0; c < 3; ++c) { dL_dmeans3D[3 * g + c] = 0.f; dL_dmeans2D[3 * g + c] = 0.f; dL_dcolors[3 * g + c] = 0.f; }
    dL_dopac[g] = 0.f;
    dL_dscales[2 * g] = 0.f; dL_dscales[2 * g + 1] = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) dL_drot[4 * g + c] = 0.f;
    return;
  }
  const float* gs = gsum + (size_t)g * GROW;
  float gT[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) gT[c] = gs[R_T + c];
  const float gmx = gs[R_MX], gmy = gs[R_MY];
  const float4 a = rec[REC * g + 0], b = rec[REC * g + 1], c2 = rec[REC * g + 2], nr = rec[REC * g + 4];
  const float T[9] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c2.x};
  const float mx = c2.y, my = c2.z, sign = nr.z;
  dL_dmeans2D[3 * g] = gmx;
  dL_dmeans2D[3 * g + 1] = gmy;
  dL_dmeans2D[3 * g + 2] = 0.f;
  dL_dcolors[3 * g] = gs[R_C]; dL_dcolors[3 * g + 1] = gs[R_C + 1]; dL_dcolors[3 * g + 2] = gs[R_C + 2];
  dL_dopac[g] = gs[R_O];

  // mu = (sum t T_u T_w, sum t T_v T_w) / sum t T_w T_w
  const float d = (CUTOFF2 * (T[2] * T[2]) + CUTOFF2 * (T[5] * T[5])) + (-1.0f) * (T[8] * T[8]);
  const float tv[3] = {CUTOFF2, CUTOFF2, -1.0f};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float fi = tv[i] / d;
    gT[3 * i + 0] += gmx * fi * T[3 * i + 2];
    gT[3 * i + 1] += gmy * fi * T[3 * i + 2];
    gT[3 * i + 2] += fi * (gmx * (T[3 * i + 0] - 2.0f * mx * T[3 * i + 2]) + gmy * (T[3 * i + 1] - 2.0f * my * T[3 * i + 2]));
  }
  // rows of T = (a, a3) . projmatrix . N  ->  dL/da
  const float* Pm = p.proj;
  const float hw = 0.5f * (float)p.W, hw1 = 0.5f * ((float)p.W - 1.0f);
  const float hh = 0.5f * (float)p.H, hh1 = 0.5f * ((float)p.H - 1.0f);
  float ga[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float gc0 = hw * gT[3 * i], gc1 = hh * gT[3 * i + 1];
    const float gc3 = (hw1 * gT[3 * i] + hh1 * gT[3 * i + 1]) + gT[3 * i + 2];
#pragma unroll
    for (int j = 0; j < 3; ++j) ga[i][j] = (Pm[4 * j] * gc0 + Pm[4 * j + 1] * gc1) + Pm[4 * j + 3] * gc3;
  }
  dL_dmeans3D[3 * g] = ga[2][0];
  dL_dmeans3D[3 * g + 1] = ga[2][1];
  dL_dmeans3D[3 * g + 2] = ga[2][2];

  const float qr = rotations[4 * g], qx = rotations[4 * g + 1], qy = rotations[4 * g + 2], qz = rotations[4 * g + 3];
  const float R00 = 1.0f - 2.0f * (qy * qy + qz * qz), R01 = 2.0f * (qx * qy - qr * qz);
  const float R10 = 2.0f * (qx * qy + qr * qz), R11 = 1.0f - 2.0f * (qx * qx + qz * qz);
  const float R20 = 2.0f * (qx * qz - qr * qy), R21 = 2.0f * (qy * qz + qr * qx);
  const float s0 = p.scale_mod * scales[2 * g], s1 = p.scale_mod * scales[2 * g + 1];
  dL_dscales[2 * g] = p.scale_mod * ((R00 * ga[0][0] + R10 * ga[0][1]) + R20 * ga[0][2]);
  dL_dscales[2 * g + 1] = p.scale_mod * ((R01 * ga[1][0] + R11 * ga[1][1]) + R21 * ga[1][2]);
  // dL/dR: column 0 from t_u, column 1 from t_v, column 2 from the normal n_c = sign R_cw R[:, 2]
  const float* V = p.view;
  const float gn0 = gs[R_N], gn1 = gs[R_N + 1], gn2 = gs[R_N + 2];
  float G[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    G[r][0] = ga[0][r] * s0;
    G[r][1] = ga[1][r] * s1;
    G[r][2] = sign * ((V[4 * r] * gn0 + V[4 * r + 1] * gn1) + V[4 * r + 2] * gn2);
  }
  dL_drot[4 * g + 0] = 2.0f * (((-qz * G[0][1] + qy * G[0][2]) + (qz * G[1][0] - qx * G[1][2])) +
                               (-qy * G[2][0] + qx * G[2][1]));
  dL_drot[4 * g + 1] = 2.0f * (((qy * G[0][1] + qz * G[0][2]) + (qy * G[1][0] - 2.0f * qx * G[1][1] - qr * G[1][2])) +
                               (qz * G[2][0] + qr * G[2][1] - 2.0f * qx * G[2][2]));
  dL_drot[4 * g + 2] = 2.0f * (((-2.0f * qy * G[0][0] + qx * G[0][1] + qr * G[0][2]) + (qx * G[1][0] + qz * G[1][2])) +
                               (-qr * G[2][0] + qz * G[2][1] - 2.0f * qy * G[2][2]));
  dL_drot[4 * g + 3] = 2.0f * (((-2.0f * qz * G[0][0] - qr * G[0][1] + qx * G[0][2]) +
                                (qr * G[1][0] - 2.0f * qz * G[1][1] + qy * G[1][2])) +
                               (qx * G[2][0] + qy * G[2][1]));
}

__global__ void slots_to_ids2d_kernel(int64_t I, const uint32_t* __restrict__ list, const uint32_t* __restrict__ slot_g,
                                      uint32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < I) out[i] = slot_g[list[i]];
}

static int make_params(const pings_raster_settings* s, int P, Params& kp) {
  PINGS_ARG_CHECK(s != nullptr, "null settings");
  PINGS_ARG_CHECK(s->mode == PINGS_RASTER_2DGS, "settings mode is not PINGS_RASTER_2DGS");
  PINGS_ARG_CHECK(s->image_height > 0 && s->image_width > 0, "empty image");
  PINGS_ARG_CHECK(s->image_height < 65536 && s->image_width < 65536, "image too large");
  PINGS_ARG_CHECK(s->viewmatrix && s->projmatrix && s->bg, "null camera pointer");
  PINGS_ARG_CHECK(P >= 0, "negative Gaussian count");
  kp.P = P;
  kp.W = s->image_width;
  kp.H = s->image_height;
  kp.gx = ceil_div(kp.W, TILE);
  kp.gy = ceil_div(kp.H, TILE);
  kp.scale_mod = (float)s->scale_modifier;
  kp.view = s->viewmatrix;
  kp.proj = s->projmatrix;
  kp.bg = s->bg;
  kp.live = nullptr;
  kp.dyn_rows = 0;
  return PINGS_OK;
}

static int num_tiles(int H, int W) { return ceil_div(W, TILE) * ceil_div(H, TILE); }

}  // namespace raster2d
}  // namespace pings

using namespace pings::raster2d;
using pings::ceil_div;
namespace devprim = pings::devprim;

PINGS_API size_t pings_raster2d_geom_bytes(int P, int image_height, int image_width) {
  (void)image_height; (void)image_width;
  return carve_geom(nullptr, P).total;
}

PINGS_API size_t pings_raster2d_binning_bytes(int64_t num_instances, int image_height, int image_width) {
  return carve_bins(nullptr, num_instances, num_tiles(image_height, image_width)).total;
}

PINGS_API size_t pings_raster2d_image_bytes(int image_height, int image_width) {
  return carve_img(nullptr, image_width, image_height).total;
}

PINGS_API int pings_raster2d_preprocess(const pings_raster_settings* s, int P, const float* means3D,
                                        const float* colors, const float* opacities, const float* scales,
                                        const float* rotations, void* geom_blob, int32_t* radii,
                                        const int32_t* live_rows_dev, int dyn_rows, const int32_t* const* aux_dev,
                                        int aux_words, int32_t* aux_host, int64_t* num_instances, void* stream) {
  Params kp;
  const int st_ = make_params(s, P, kp);
  if (st_) return st_;
  PINGS_ARG_CHECK(num_instances != nullptr && geom_blob != nullptr, "null pointer");
  PINGS_ARG_CHECK(P == 0 || (means3D && colors && opacities && scales && rotations && radii), "null pointer");
  PINGS_ARG_CHECK(aux_words >= 0 && aux_words <= 6 && (aux_words == 0 || (aux_dev && aux_host)), "aux words");
  PINGS_ARG_CHECK(dyn_rows >= 0 && dyn_rows <= P, "dyn_rows outside [0, P]");
  kp.live = live_rows_dev;
  kp.dyn_rows = live_rows_dev ? dyn_rows : 0;
  hipStream_t st = pings::as_stream(stream);
  Geom gs = carve_geom(geom_blob, P);
  PINGS_HIP_CHECK(hipMemsetAsync(gs.count, 0, sizeof(unsigned long long), st));
  if (P > 0) {
    {
      pings::prof::Scope ps("preprocess2d", st);
      hipLaunchKernelGGL(preprocess2d_kernel, dim3(ceil_div(P, 256)), dim3(256), 0, st, kp, means3D, colors, opacities,
                         scales, rotations, gs.rec, gs.rect, gs.tiles, gs.key, radii);
      PINGS_LAUNCH_CHECK();
    }
    if (int e = devprim::inclusive_sum_u32(gs.temp, gs.temp_bytes, gs.tiles, gs.offsets, P, st)) return e;
    hipLaunchKernelGGL(total2d_kernel, dim3(ceil_div(P, 256)), dim3(256), 0, st, P, gs.tiles, gs.count);
    PINGS_LAUNCH_CHECK();
  }
  const uint32_t* lo = reinterpret_cast<const uint32_t*>(gs.count);
  const uint32_t* words[8] = {lo, lo + 1};    // little endian: low word, high word
  for (int i = 0; i < aux_words; ++i) words[2 + i] = reinterpret_cast<const uint32_t*>(aux_dev[i]);
  uint32_t out[8] = {0};
  const int rs = pings::host_read_words(words, 2 + aux_words, out, st);
  if (rs) return rs;
  for (int i = 0; i < aux_words; ++i) aux_host[i] = (int32_t)out[2 + i];
  const unsigned long long total = (unsigned long long)out[0] | ((unsigned long long)out[1] << 32);
  *num_instances = (int64_t)total;
  if (total >= 0x7FFFFFFFull) {
    pings::set_error("pings_raster2d_preprocess: %llu (Gaussian, tile) pairs exceed the sort's int range", total);
    return PINGS_ERR_CAPACITY;
  }
  return PINGS_OK;
}

PINGS_API int pings_raster2d_render(const pings_raster_settings* s, int P, int64_t I, void* geom_blob,
                                    void* binning_blob, void* image_blob, float* out_color, float* out_allmap,
                                    void* stream) {
  Params kp;
  const int st_ = make_params(s, P, kp);
  if (st_) return st_;
  PINGS_ARG_CHECK(geom_blob && binning_blob && image_blob && out_color && out_allmap, "null pointer");
  PINGS_ARG_CHECK(I >= 0 && I < 0x7FFFFFFF, "instance count");
  hipStream_t st = pings::as_stream(stream);
  const int nt = num_tiles(kp.H, kp.W);
  Geom gs = carve_geom(geom_blob, P);
  Bins bs = carve_bins(binning_blob, I, nt);
  Img im = carve_img(image_blob, kp.W, kp.H);
  PINGS_HIP_CHECK(hipMemsetAsync(bs.ranges, 0, sizeof(uint2) * (size_t)nt, st));
  if (I > 0) {
    pings::prof::Scope ps("binning2d", st);
    hipLaunchKernelGGL(duplicate2d_kernel, dim3(ceil_div(P, 256)), dim3(256), 0, st, P, kp.gx, gs.rect, gs.tiles,
                       gs.offsets, gs.key, bs.keys, bs.slots, bs.slot_g);
    PINGS_LAUNCH_CHECK();
    if (int e = devprim::sort_pairs_u64_u32(bs.temp, bs.temp_bytes, bs.keys, bs.keys_sorted, bs.slots, bs.point_list, I,
                                            0, 32 + tile_bits(nt), st))
      return e;
    hipLaunchKernelGGL(tile_ranges2d_kernel, dim3((unsigned)ceil_div<int64_t>(I, 256)), dim3(256), 0, st, I,
                       bs.keys_sorted, bs.ranges);
    PINGS_LAUNCH_CHECK();
  }
  {
    pings::prof::Scope ps("blend2d_fwd", st);
    hipLaunchKernelGGL(blend2d_fwd_kernel, dim3(nt), dim3(BLOCK), 0, st, kp.W, kp.H, kp.gx, kp.bg, bs.ranges,
                       bs.point_list, bs.slot_g, gs.rec, im, out_color, out_allmap);
    PINGS_LAUNCH_CHECK();
  }
  return PINGS_OK;
}

PINGS_API size_t pings_raster2d_backward_bytes(int P, int64_t I) {
  return carve_bwd(nullptr, P, I).total;
}

PINGS_API int pings_raster2d_backward(const pings_raster_settings* s, int P, int64_t I, const float* scales,
                                      const float* rotations, const void* geom_blob, const void* binning_blob,
                                      const void* image_blob, const float* dL_dcolor, const float* dL_dallmap,
                                      void* bwd_blob, float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dcolors,
                                      float* dL_dopacities, float* dL_dscales, float* dL_drotations, void* stream) {
  Params kp;
  const int st_ = make_params(s, P, kp);
  if (st_) return st_;
  PINGS_ARG_CHECK(geom_blob && binning_blob && image_blob && bwd_blob, "null pointer");
  PINGS_ARG_CHECK(P == 0 || (scales && rotations && dL_dmeans3D && dL_dmeans2D && dL_dcolors && dL_dopacities &&
                             dL_dscales && dL_drotations), "null pointer");
  PINGS_ARG_CHECK(I >= 0 && I < 0x7FFFFFFF, "instance count");
  if (P == 0) return PINGS_OK;
  hipStream_t st = pings::as_stream(stream);
  const int nt = num_tiles(kp.H, kp.W);
  Geom gs = carve_geom(const_cast<void*>(geom_blob), P);
  Bins bs = carve_bins(const_cast<void*>(binning_blob), I, nt);
  Img im = carve_img(const_cast<void*>(image_blob), kp.W, kp.H);
  const Bwd bw = carve_bwd(bwd_blob, P, I);
  float *parts = bw.parts, *rows = bw.rows, *gsum = bw.gsum;
  if (I > 0) {
    PINGS_HIP_CHECK(hipMemsetAsync(parts, 0, sizeof(float) * (size_t)I * 4 * GROW, st));
    {
      pings::prof::Scope ps("blend2d_bwd", st);
      hipLaunchKernelGGL(blend2d_bwd_kernel, dim3(nt), dim3(BLOCK), 0, st, kp.W, kp.H, kp.gx, kp.bg, bs.ranges,
                         bs.point_list, bs.slot_g, gs.rec, im, dL_dcolor, dL_dallmap, parts);
      PINGS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(fold2d_kernel, dim3((unsigned)ceil_div<int64_t>(I * GROW, 256)), dim3(256), 0, st, I, parts,
                       rows);
    PINGS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(gaussian_sum2d_kernel, dim3((unsigned)ceil_div<int64_t>((int64_t)P * GROW, 256)), dim3(256), 0,
                     st, P, gs.tiles, gs.offsets, rows, gsum);
  PINGS_LAUNCH_CHECK();
  hipLaunchKernelGGL(gaussian2d_bwd_kernel, dim3(ceil_div(P, 256)), dim3(256), 0, st, kp, scales, rotations, gs.tiles,
                     gs.rec, gsum, dL_dmeans3D, dL_dmeans2D, dL_dcolors, dL_dopacities, dL_dscales, dL_drotations);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API int pings_raster2d_debug_lists(const void* binning_blob, int64_t I, int image_height, int image_width,
                                         uint32_t* point_list, uint32_t* ranges_xy, void* stream) {
  PINGS_ARG_CHECK(binning_blob && ranges_xy && image_height > 0 && image_width > 0, "null pointer / empty image");
  const int nt = num_tiles(image_height, image_width);
  Bins bs = carve_bins(const_cast<void*>(binning_blob), I, nt);
  hipStream_t st = pings::as_stream(stream);
  if (I > 0 && point_list) {
    hipLaunchKernelGGL(slots_to_ids2d_kernel, dim3((unsigned)ceil_div<int64_t>(I, 256)), dim3(256), 0, st, I,
                       bs.point_list, bs.slot_g, point_list);
    PINGS_LAUNCH_CHECK();
  }
  PINGS_HIP_CHECK(hipMemcpyAsync(ranges_xy, bs.ranges, sizeof(uint2) * (size_t)nt, hipMemcpyDeviceToDevice, st));
  return PINGS_OK;
}

PINGS_API int pings_raster2d_debug_image(const void* image_blob, int image_height, int image_width, float* final_T,
                                         uint32_t* n_contrib, int32_t* median, void* stream) {
  PINGS_ARG_CHECK(image_blob && final_T && n_contrib && median && image_height > 0 && image_width > 0,
                  "null pointer / empty image");
  Img im = carve_img(const_cast<void*>(image_blob), image_width, image_height);
  hipStream_t st = pings::as_stream(stream);
  const size_t n = (size_t)image_height * image_width;
  PINGS_HIP_CHECK(hipMemcpyAsync(final_T, im.final_T, sizeof(float) * n, hipMemcpyDeviceToDevice, st));
  PINGS_HIP_CHECK(hipMemcpyAsync(n_contrib, im.n_contrib, sizeof(uint32_t) * n, hipMemcpyDeviceToDevice, st));
  PINGS_HIP_CHECK(hipMemcpyAsync(median, im.median, sizeof(int32_t) * n, hipMemcpyDeviceToDevice, st));
  return PINGS_OK;
}
