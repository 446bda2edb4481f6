// Depth-view fusion into a sparse truncated signed distance volume (pings_amd/tsdf_ops.py: TSDFVolume), the route the
// reference takes through Open3D's ScalableTSDFVolume (dataset/slam_dataset.py:1154-1193).  The rules are DESIGN §2.9
// and are restated in fp64 numpy by tests/tsdf_ref.py.
//
// The volume is a set of blocks of 8^3 voxels.  Block b = floor(g / 8) of grid point g has the key
// (bx + 2^20) << 42 | (by + 2^20) << 21 | (bz + 2^20), so ascending keys are ascending (bx, by, bz).  An open-addressing
// table of int64 keys (-1 = free) maps a key to the block's slot in the store; a slot is given once and never changes.
// Per block and field the store holds 512 consecutive floats, voxel (lx, ly, lz) at (lx*8 + ly)*8 + lz.
//   touch     one thread per strided pixel: its <= 8 candidate blocks, duplicates dropped inside the wave, found or
//             inserted with a 64-bit compare-and-swap; the first toucher of a block in this frame (an integer stamp per
//             table entry) files it in the frame's list, and in the list of new keys when it has no slot yet
//   assign    the frame's new keys sorted ascending, slots base + rank written into the table, the new blocks initialised
//   update    one workgroup per touched block, one thread per voxel for the whole launch: project, gather, average
//   densify   a box of grid points as dense arrays; vertices: marching-cubes keys -> positions from global integers
// Integer atomics only; every float of the store is the same from run to run.

#include "common.hpp"
#include "devprim.hpp"
#include "tsdf_table.hpp"

namespace {

using namespace pings::tsdf;       // key, table and block constants: tsdf_table.hpp

struct Camera {       // fp32, each value rounded once from the host's fp64
  float fx, fy, cx, cy;
  float m[12];        // rows of a 3x4: world -> camera for update, camera -> world for touch
  float ox, oy, oz, voxel, trunc, dmin, dmax;
  int H, W;
};

__device__ __forceinline__ bool valid_depth(const Camera& c, float d) {
  return isfinite(d) && d > c.dmin && d < c.dmax;
}

// counters: [0] touched blocks, [1] new blocks, [2] status bits
__global__ __launch_bounds__(kBlock) void tsdf_touch_kernel(Camera c, const float* __restrict__ depth, int stride, int ws,
                                                            int hs, int frame, i64* tkeys, const int32_t* tslots,
                                                            int32_t* tstamps, i64 tsize, i64 list_cap,
                                                            int32_t* __restrict__ touched, i64* __restrict__ new_keys,
                                                            int32_t* counters) {
  const i64 s = (i64)blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool pixel = s < (i64)ws * hs;
  i64 b0[3] = {0, 0, 0};
  int span[3] = {0, 0, 0};
  if (pixel) {
    const int u = (int)(s % ws) * stride, v = (int)(s / ws) * stride;
    const float d = depth[(i64)v * c.W + u];
    pixel = valid_depth(c, d);
    if (pixel) {
      const float x = ((float)u - c.cx) * d / c.fx, y = ((float)v - c.cy) * d / c.fy;
      const float q[3] = {c.m[0] * x + c.m[1] * y + c.m[2] * d + c.m[3], c.m[4] * x + c.m[5] * y + c.m[6] * d + c.m[7],
                          c.m[8] * x + c.m[9] * y + c.m[10] * d + c.m[11]};
      const float o[3] = {c.ox, c.oy, c.oz};
      const float edge = (float)kB * c.voxel;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float lo = floorf((q[a] - c.trunc - o[a]) / edge), hi = floorf((q[a] + c.trunc - o[a]) / edge);
        // the comparisons are false for NaN; hi - lo <= 1 by 2 trunc <= 8 voxel, held here against rounding
        if (!(lo >= (float)-kBias && hi < (float)kBias)) pixel = false;
        else {
          b0[a] = (i64)lo;
          span[a] = hi > lo ? 1 : 0;
        }
      }
      if (!pixel) atomicOr(&counters[2], PINGS_TSDF_EXTENT);
    }
  }
#pragma unroll 1
  for (int cand = 0; cand < 8; ++cand) {
    const int dx = cand & 1, dy = cand >> 1 & 1, dz = cand >> 2;
    bool pend = pixel && dx <= span[0] && dy <= span[1] && dz <= span[2];
    i64 key = 0;
    if (pend) {
      const i64 bx = b0[0] + dx, by = b0[1] + dy, bz = b0[2] + dz;
      pend = in_extent(bx) && in_extent(by) && in_extent(bz);
      if (pend) key = pack_key(bx, by, bz);
      else atomicOr(&counters[2], PINGS_TSDF_EXTENT);
    }
    // one lane per distinct key of the wave goes to memory: neighbouring pixels name the same blocks
    bool owner = false;
    for (;;) {
      const u64 m = __ballot(pend);
      if (!m) break;
      const int leader = __ffsll((long long)m) - 1;
      const i64 k = __shfl(key, leader, 64);
      if (pend && key == k) {
        pend = false;
        owner = lane == leader;
      }
    }
    if (!owner) continue;
    const i64 e = table_find_or_insert(tkeys, tsize, key);
    if (e < 0) {
      atomicOr(&counters[2], PINGS_TSDF_TABLE_FULL);
      continue;
    }
    if (atomicExch(&tstamps[e], frame) == frame) continue;     // another wave filed this block in this frame
    const i64 at = atomicAdd(&counters[0], 1);
    if (at < list_cap) touched[at] = (int32_t)e;
    if (tslots[e] < 0) {                                        // slots are written by the assign launch only
      const i64 an = atomicAdd(&counters[1], 1);
      if (an < list_cap) new_keys[an] = key;
    }
  }
}

__global__ __launch_bounds__(kBlock) void tsdf_assign_kernel(const i64* __restrict__ sorted, i64 n_new, i64 base,
                                                             const i64* __restrict__ tkeys, int32_t* tslots, i64 tsize,
                                                             i64* __restrict__ block_keys, float* __restrict__ tsdf,
                                                             float* __restrict__ weight, float* __restrict__ color) {
  const i64 r = blockIdx.x;
  if (r >= n_new) return;
  const i64 key = sorted[r], slot = base + r;
  if (threadIdx.x == 0) {
    block_keys[slot] = key;
    const i64 e = table_find(tkeys, tsize, key);
    if (e >= 0) tslots[e] = (int32_t)slot;
  }
  for (int l = threadIdx.x; l < kVox; l += kBlock) {
    tsdf[slot * kVox + l] = 1.f;
    weight[slot * kVox + l] = 0.f;
  }
  if (color)
    for (int l = threadIdx.x; l < 3 * kVox; l += kBlock) color[slot * 3 * kVox + l] = 0.f;
}

// rebuilds a table from the store's keys (after the table has grown): slot s of block_keys[s]
__global__ __launch_bounds__(kBlock) void tsdf_table_insert_kernel(const i64* __restrict__ block_keys, i64 nb, i64* tkeys,
                                                                   int32_t* tslots, i64 tsize, int32_t* status) {
  const i64 s = (i64)blockIdx.x * kBlock + threadIdx.x;
  if (s >= nb) return;
  const i64 e = table_find_or_insert(tkeys, tsize, block_keys[s]);
  if (e < 0) atomicOr(status, PINGS_TSDF_TABLE_FULL);
  else tslots[e] = (int32_t)s;
}

__global__ __launch_bounds__(kBlock) void tsdf_update_kernel(Camera c, const float* __restrict__ depth,
                                                             const float* __restrict__ image,
                                                             const int32_t* __restrict__ touched,
                                                             const i64* __restrict__ tkeys,
                                                             const int32_t* __restrict__ tslots, i64 tsize, i64 capacity,
                                                             float* __restrict__ tsdf, float* __restrict__ weight,
                                                             float* __restrict__ color) {
  const int32_t e = touched[blockIdx.x];
  if (e < 0 || e >= tsize) return;
  const i64 key = tkeys[e], slot = tslots[e];
  if (key < 0 || slot < 0 || slot >= capacity) return;
  const i64 bx = (key >> 42) - kBias, by = (key >> 21 & (2 * kBias - 1)) - kBias, bz = (key & (2 * kBias - 1)) - kBias;
  const i64 hw = (i64)c.H * c.W;
#pragma unroll
  for (int l = threadIdx.x; l < kVox; l += kBlock) {
    const float px = c.ox + c.voxel * (float)(bx * kB + (l >> 6));
    const float py = c.oy + c.voxel * (float)(by * kB + (l >> 3 & 7));
    const float pz = c.oz + c.voxel * (float)(bz * kB + (l & 7));
    const float x = c.m[0] * px + c.m[1] * py + c.m[2] * pz + c.m[3];
    const float y = c.m[4] * px + c.m[5] * py + c.m[6] * pz + c.m[7];
    const float z = c.m[8] * px + c.m[9] * py + c.m[10] * pz + c.m[11];
    if (!(z > 0.f)) continue;
    const float fu = floorf(c.fx * x / z + c.cx + 0.5f), fv = floorf(c.fy * y / z + c.cy + 0.5f);
    if (!(fu >= 0.f && fu < (float)c.W && fv >= 0.f && fv < (float)c.H)) continue;
    const i64 pix = (i64)fv * c.W + (i64)fu;
    const float d = depth[pix];
    if (!valid_depth(c, d)) continue;
    const float a = (fu - c.cx) / c.fx, b = (fv - c.cy) / c.fy;
    const float sdf = (d - z) * sqrtf(1.f + a * a + b * b);
    if (!(sdf > -c.trunc)) continue;
    const float t = fminf(1.f, sdf / c.trunc);
    const i64 o = slot * kVox + l;
    const float w = weight[o], w1 = w + 1.f;
    tsdf[o] = (tsdf[o] * w + t) / w1;
    if (color) {
      const i64 oc = slot * 3 * kVox + l;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) color[oc + ch * kVox] = (color[oc + ch * kVox] * w + image[ch * hw + pix]) / w1;
    }
    weight[o] = w1;
  }
}

struct Box {
  i64 lo[3];
  i64 nx, ny, nz;
};

__global__ __launch_bounds__(kBlock) void tsdf_densify_kernel(Box bx, const i64* __restrict__ tkeys,
                                                              const int32_t* __restrict__ tslots, i64 tsize, i64 capacity,
                                                              const float* __restrict__ tsdf,
                                                              const float* __restrict__ weight,
                                                              const float* __restrict__ color, float min_weight,
                                                              float* __restrict__ out_tsdf, float* __restrict__ out_weight,
                                                              float* __restrict__ out_color) {
  const i64 p = (i64)blockIdx.x * kBlock + threadIdx.x;
  if (p >= bx.nx * bx.ny * bx.nz) return;
  const i64 g[3] = {bx.lo[0] + p / (bx.ny * bx.nz), bx.lo[1] + (p / bx.nz) % bx.ny, bx.lo[2] + p % bx.nz};
  const i64 b[3] = {g[0] >> 3, g[1] >> 3, g[2] >> 3};      // arithmetic shift: floor division for negative points too
  float t = 1.f, w = 0.f, c[3] = {0.f, 0.f, 0.f};
  if (in_extent(b[0]) && in_extent(b[1]) && in_extent(b[2])) {
    const i64 e = table_find(tkeys, tsize, pack_key(b[0], b[1], b[2]));
    const i64 slot = e < 0 ? -1 : (i64)tslots[e];
    if (slot >= 0 && slot < capacity) {
      const int l = (int)((g[0] & 7) << 6 | (g[1] & 7) << 3 | (g[2] & 7));
      t = tsdf[slot * kVox + l];
      w = weight[slot * kVox + l];
      if (color && out_color) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch] = color[slot * 3 * kVox + ch * kVox + l];
      }
    }
  }
  if (w < min_weight) t = INFINITY;           // min_weight <= 0: the plain variant
  out_tsdf[p] = t;
  if (out_weight) out_weight[p] = w;
  if (out_color) {
    out_color[3 * p] = c[0];
    out_color[3 * p + 1] = c[1];
    out_color[3 * p + 2] = c[2];
  }
}

struct Origin {
  double o[3], voxel;
};

// Marching-cubes vertex key 4 p + slot of a chunk -> world position and colour from global quantities only, so two
// chunks that share an edge give the same bits (marching cubes itself returns fl32(i_local + t)).
__global__ __launch_bounds__(kBlock) void tsdf_vertices_kernel(Box bx, Origin og, const i64* __restrict__ keys, i64 nv,
                                                               const float* __restrict__ vol,
                                                               const float* __restrict__ col, float* __restrict__ verts,
                                                               float* __restrict__ colors) {
  const i64 r = (i64)blockIdx.x * kBlock + threadIdx.x;
  if (r >= nv) return;
  const i64 n = bx.nx * bx.ny * bx.nz, key = keys[r], p = key >> 2;
  const int slot = (int)(key & 3);
  const i64 strides[3] = {bx.ny * bx.nz, bx.nz, 1};
  const i64 p1 = slot ? p + strides[slot - 1] : p;
  if (key < 0 || p1 >= n) {                    // no key of pings_mc_emit on this box does this
    verts[3 * r] = verts[3 * r + 1] = verts[3 * r + 2] = NAN;
    if (colors) colors[3 * r] = colors[3 * r + 1] = colors[3 * r + 2] = 0.f;
    return;
  }
  const i64 g[3] = {bx.lo[0] + p / (bx.ny * bx.nz), bx.lo[1] + (p / bx.nz) % bx.ny, bx.lo[2] + p % bx.nz};
  double t = 0.0;
  if (slot) {
    const double v0 = vol[p], v1 = vol[p1];
    t = v0 / (v0 - v1);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) verts[3 * r + a] = (float)(og.o[a] + og.voxel * ((double)g[a] + (slot == a + 1 ? t : 0.0)));
  if (colors) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const double c0 = col[3 * p + ch], c1 = col[3 * p1 + ch];
      const double c = c0 + t * (c1 - c0);
      colors[3 * r + ch] = (float)fmin(1.0, fmax(0.0, c));
    }
  }
}

int make_camera(Camera* c, int H, int W, const double* intrinsic, const double* m, const double* origin,
                double voxel_length, double sdf_trunc, float depth_min, float depth_trunc) {
  PINGS_ARG_CHECK(intrinsic && m && origin, "null pointer");
  PINGS_ARG_CHECK(H > 0 && W > 0 && (i64)H * W < (i64)0x7FFFFFFF, "empty or too large image");
  PINGS_ARG_CHECK(voxel_length > 0.0 && sdf_trunc > 0.0, "voxel_length and sdf_trunc must be positive");
  PINGS_ARG_CHECK(2.0 * sdf_trunc <= kB * voxel_length, "2 sdf_trunc may not exceed the block edge");
  PINGS_ARG_CHECK(intrinsic[0] != 0.0 && intrinsic[1] != 0.0, "zero focal length");
  c->fx = (float)intrinsic[0];
  c->fy = (float)intrinsic[1];
  c->cx = (float)intrinsic[2];
  c->cy = (float)intrinsic[3];
  for (int i = 0; i < 12; ++i) c->m[i] = (float)m[i];
  c->ox = (float)origin[0];
  c->oy = (float)origin[1];
  c->oz = (float)origin[2];
  c->voxel = (float)voxel_length;
  c->trunc = (float)sdf_trunc;
  c->dmin = depth_min;
  c->dmax = depth_trunc;
  c->H = H;
  c->W = W;
  return PINGS_OK;
}

struct AssignScratch {
  i64* sorted;   // the new block keys in ascending order
  void* temp;
  size_t temp_bytes, total;
};
AssignScratch carve_assign(void* base, i64 n_new) {
  pings::Carver c(base);
  AssignScratch s;
  s.sorted = c.take<i64>((size_t)n_new);
  s.temp_bytes = pings::devprim::sort_keys_i64_temp_bytes(n_new);
  s.temp = c.take<char>(s.temp_bytes);
  s.total = c.total();
  return s;
}

constexpr i64 kMaxBoxPoints = (i64)1 << 40;

int check_box(const i64* lo, i64 nx, i64 ny, i64 nz) {
  PINGS_ARG_CHECK(lo, "null pointer");
  PINGS_ARG_CHECK(nx > 0 && ny > 0 && nz > 0, "empty or negative shape");
  PINGS_ARG_CHECK(nx <= kMaxBoxPoints / ny && nx * ny <= kMaxBoxPoints / nz, "box too large");
  PINGS_ARG_CHECK(pings::ceil_div<i64>(nx * ny * nz, kBlock) < (i64)0x7FFFFFFF, "box too large");
  const i64 lim = kBias * kB * 2;
  for (int a = 0; a < 3; ++a) PINGS_ARG_CHECK(lo[a] > -lim && lo[a] < lim, "box origin out of range");
  return PINGS_OK;
}

}  // namespace

PINGS_API int pings_tsdf_table_insert(const int64_t* block_keys, int64_t nb, int64_t* tkeys, int32_t* tslots,
                                      int64_t tsize, int32_t* status, void* stream) {
  PINGS_ARG_CHECK(table_ok(tkeys, tslots, tsize), "the table is null or its size is no power of two in [64, 2^31)");
  PINGS_ARG_CHECK(nb >= 0 && 2 * nb <= tsize, "the table must be at least twice the number of blocks");
  if (nb == 0) return PINGS_OK;
  PINGS_ARG_CHECK(block_keys && status, "null pointer");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("tsdf_table_insert", st);
  return pings::launch(tsdf_table_insert_kernel, dim3((unsigned)pings::ceil_div<i64>(nb, kBlock)), kBlock, 0, st,
                       block_keys, nb, tkeys, tslots, tsize, status);
}

PINGS_API int pings_tsdf_touch(const float* depth, int height, int width, const double* intrinsic,
                               const double* cam_to_world, const double* origin, double voxel_length, double sdf_trunc,
                               float depth_min, float depth_trunc, int stride, int frame, int64_t* tkeys,
                               const int32_t* tslots, int32_t* tstamps, int64_t tsize, int64_t list_cap,
                               int32_t* touched, int64_t* new_keys, int32_t* counters, int64_t* totals, void* stream) {
  Camera c;
  if (int e = make_camera(&c, height, width, intrinsic, cam_to_world, origin, voxel_length, sdf_trunc, depth_min,
                          depth_trunc))
    return e;
  PINGS_ARG_CHECK(depth && tstamps && touched && new_keys && counters && totals, "null pointer");
  PINGS_ARG_CHECK(table_ok(tkeys, tslots, tsize), "the table is null or its size is no power of two in [64, 2^31)");
  PINGS_ARG_CHECK(stride >= 1 && frame >= 1, "stride and frame start at 1");
  const int ws = (width + stride - 1) / stride, hs = (height + stride - 1) / stride;
  PINGS_ARG_CHECK(list_cap >= 8 * (i64)ws * hs, "the frame lists hold 8 entries per strided pixel");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("tsdf_touch", st);
  PINGS_HIP_CHECK(hipMemsetAsync(counters, 0, 4 * sizeof(int32_t), st));
  if (int e = pings::launch(tsdf_touch_kernel, dim3((unsigned)pings::ceil_div<i64>((i64)ws * hs, kBlock)), kBlock, 0, st,
                            c, depth, stride, ws, hs, frame, tkeys, tslots, tstamps, tsize, list_cap, touched, new_keys,
                            counters))
    return e;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(counters);
  const uint32_t* src[3] = {w, w + 1, w + 2};
  uint32_t got[3] = {0u, 0u, 0u};
  if (int e = pings::host_read_words(src, 3, got, st)) return e;
  for (int i = 0; i < 3; ++i) totals[i] = (int64_t)got[i];
  return PINGS_OK;
}

PINGS_API size_t pings_tsdf_assign_scratch_bytes(int64_t n_new) {
  if (n_new <= 0 || n_new >= (i64)0x7FFFFFFF) return 0;
  return carve_assign(nullptr, n_new).total;
}

PINGS_API int pings_tsdf_assign(const int64_t* new_keys, int64_t n_new, int64_t base_slot, int64_t capacity,
                                void* scratch, const int64_t* tkeys, int32_t* tslots, int64_t tsize,
                                int64_t* block_keys, float* tsdf, float* weight, float* color, void* stream) {
  PINGS_ARG_CHECK(n_new >= 0 && n_new < (i64)0x7FFFFFFF && base_slot >= 0, "negative count or slot");
  if (n_new == 0) return PINGS_OK;
  PINGS_ARG_CHECK(new_keys && scratch && block_keys && tsdf && weight, "null pointer");
  PINGS_ARG_CHECK(table_ok(tkeys, tslots, tsize), "the table is null or its size is no power of two in [64, 2^31)");
  PINGS_ARG_CHECK(base_slot + n_new <= capacity && capacity < (i64)0x7FFFFFFF, "the store is too small for the new blocks");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("tsdf_assign", st);
  const AssignScratch s = carve_assign(scratch, n_new);
  if (int e = pings::devprim::sort_keys_i64(s.temp, s.temp_bytes, new_keys, s.sorted, n_new, 0, 63, st)) return e;
  return pings::launch(tsdf_assign_kernel, dim3((unsigned)n_new), kBlock, 0, st, (const i64*)s.sorted, n_new, base_slot,
                       tkeys, tslots, tsize, block_keys, tsdf, weight, color);
}

PINGS_API int pings_tsdf_update(const float* depth, const float* image, int height, int width, const double* intrinsic,
                                const double* extrinsic, const double* origin, double voxel_length, double sdf_trunc,
                                float depth_min, float depth_trunc, const int32_t* touched, int64_t n_touched,
                                const int64_t* tkeys, const int32_t* tslots, int64_t tsize, int64_t capacity, float* tsdf,
                                float* weight, float* color, void* stream) {
  Camera c;
  if (int e = make_camera(&c, height, width, intrinsic, extrinsic, origin, voxel_length, sdf_trunc, depth_min,
                          depth_trunc))
    return e;
  PINGS_ARG_CHECK(n_touched >= 0 && n_touched < (i64)0x7FFFFFFF && capacity >= 0, "negative or too large count");
  if (n_touched == 0) return PINGS_OK;
  PINGS_ARG_CHECK(depth && touched && tsdf && weight, "null pointer");
  PINGS_ARG_CHECK((color != nullptr) == (image != nullptr), "a colour volume takes a colour image, and only it does");
  PINGS_ARG_CHECK(table_ok(tkeys, tslots, tsize), "the table is null or its size is no power of two in [64, 2^31)");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("tsdf_update", st);
  return pings::launch(tsdf_update_kernel, dim3((unsigned)n_touched), kBlock, 0, st, c, depth, image, touched, tkeys,
                       tslots, tsize, capacity, tsdf, weight, color);
}

PINGS_API int pings_tsdf_densify(const int64_t* tkeys, const int32_t* tslots, int64_t tsize, int64_t capacity,
                                 const float* tsdf, const float* weight, const float* color, const int64_t* lo,
                                 int64_t nx, int64_t ny, int64_t nz, float min_weight, float* out_tsdf,
                                 float* out_weight, float* out_color, void* stream) {
  if (int e = check_box(lo, nx, ny, nz)) return e;
  PINGS_ARG_CHECK(table_ok(tkeys, tslots, tsize), "the table is null or its size is no power of two in [64, 2^31)");
  PINGS_ARG_CHECK(capacity >= 0 && (capacity == 0 || (tsdf && weight)) && out_tsdf, "null pointer");
  PINGS_ARG_CHECK(!out_color || color || capacity == 0, "colour asked of a volume without colour");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("tsdf_densify", st);
  const Box bx{{lo[0], lo[1], lo[2]}, nx, ny, nz};
  return pings::launch(tsdf_densify_kernel, dim3((unsigned)pings::ceil_div<i64>(nx * ny * nz, kBlock)), kBlock, 0, st, bx,
                       tkeys, tslots, tsize, capacity, tsdf, weight, color, min_weight, out_tsdf, out_weight, out_color);
}

PINGS_API int pings_tsdf_vertices(const int64_t* keys, int64_t nv, const float* vol, const float* col, const int64_t* lo,
                                  int64_t nx, int64_t ny, int64_t nz, const double* origin, double voxel_length,
                                  float* verts, float* colors, void* stream) {
  if (int e = check_box(lo, nx, ny, nz)) return e;
  PINGS_ARG_CHECK(nv >= 0 && nv < (i64)0x7FFFFFFF * kBlock, "negative or too large count");
  if (nv == 0) return PINGS_OK;
  PINGS_ARG_CHECK(keys && vol && origin && verts, "null pointer");
  PINGS_ARG_CHECK((col != nullptr) == (colors != nullptr), "colours out need the dense colour field, and only they do");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("tsdf_vertices", st);
  const Box bx{{lo[0], lo[1], lo[2]}, nx, ny, nz};
  const Origin og{{origin[0], origin[1], origin[2]}, voxel_length};
  return pings::launch(tsdf_vertices_kernel, dim3((unsigned)pings::ceil_div<i64>(nv, kBlock)), kBlock, 0, st, bx, og, keys,
                       nv, vol, col, verts, colors);
}
