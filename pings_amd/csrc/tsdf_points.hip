// LiDAR scans fused into the sparse TSDF volume of tsdf.hip, with optional space carving (pings_amd/tsdf_ops.py:
// TSDFVolume.integrate_points).  The rules are DESIGN §2.9b and are restated in fp64 numpy by tests/tsdf_points_ref.py.
//
// Grid point g owns the half-open cube of edge `voxel` centred at origin + voxel g.  A ray o + s d, s in [s0, s1],
// samples every cube it crosses with a positive chord.  Both walks below step from cube to cube through the parameter
// at which the ray leaves the cube, computed from the cube's integer index, never by adding to a running value; the
// block walk uses the same expression on cubes of 8 voxels, so both see the same crossings.
//   touch       one thread per ray walks block by block; equal keys of a wave elect one owner, which files the block
//               through the table, stamps, lists and counters of tsdf.hip and notes its place in the list (tindex)
//   accumulate  one thread per ray walks voxel by voxel, probes the table once per block, and adds count and quantised
//               sample into the call's 64-bit accumulators with integer atomics
//   apply       one workgroup per touched block, one owner per voxel: the running average from the integer sums
// Sums are integers, so the store does not depend on the order of the rows and is the same bits from run to run.

#include "common.hpp"
#include "tsdf_table.hpp"

namespace {

using namespace pings::tsdf;

constexpr int kScaleBits = PINGS_TSDF_POINTS_SCALE_BITS;      // a sample is rint(t * 2^22)
constexpr int kCountShift = PINGS_TSDF_POINTS_COUNT_SHIFT;    // count above a 44-bit sum of q + 2^22 >= 0
constexpr float kScale = (float)(1 << kScaleBits);
constexpr i64 kOffset = (i64)1 << kScaleBits;
constexpr u64 kSumMask = ((u64)1 << kCountShift) - 1;
static_assert(kScaleBits + 1 + (64 - kCountShift) <= kCountShift, "2^20 samples of 2^23 must fit below the count");
// grid indices stay below 2^23 in magnitude so that (float)k + 0.5f is exact
constexpr float kGridLimit = (float)(kBias * kB - 64);

struct Scan {
  double org[3], voxel_d;       // the volume's origin and voxel edge as the host holds them
  float voxel, trunc, rmin, rmax;
  int carve, ray_mode, frame, max_steps;
  i64 n;
};

struct Ray {
  double od[3], pd[3];          // sensor and point relative to the volume's origin, exact differences of the inputs
  float o[3], d[3];             // the sensor rounded once, for the walk; unit direction
  float r, s0, s1;
};

// 0: the point is not valid, 1: a ray, 2: the ray leaves the volume's extent
__device__ __forceinline__ int make_ray(const Scan& sc, const float* __restrict__ points,
                                        const float* __restrict__ sensor, i64 i, Ray& ry) {
  float v[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float q = points[3 * i + a], so = sensor[a];
    v[a] = q - so;
    ry.od[a] = (double)so - sc.org[a];
    ry.pd[a] = (double)q - sc.org[a];
    ry.o[a] = (float)ry.od[a];
  }
  ry.r = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  if (!(isfinite(ry.r) && ry.r > sc.rmin && ry.r < sc.rmax)) return 0;       // false for NaN as well
  ry.s1 = ry.r + sc.trunc;
  ry.s0 = sc.carve ? 0.f : fmaxf(0.f, ry.r - sc.trunc);
  bool inside = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    ry.d[a] = v[a] / ry.r;
    const float e0 = (ry.o[a] + ry.s0 * ry.d[a]) / sc.voxel, e1 = (ry.o[a] + ry.s1 * ry.d[a]) / sc.voxel;
    inside = inside && fabsf(e0) < kGridLimit && fabsf(e1) < kGridLimit;
  }
  return inside ? 1 : 2;
}

// The cells of edge L voxels along a ray: cell K covers the grid points [L K, L K + L) per axis.
template <int L>
struct Walker {
  int k[3];
  float s_in;
  int budget;
  bool live;

  __device__ __forceinline__ void start(const Scan& sc, const Ray& ry) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int g = (int)floorf((ry.o[a] + ry.s0 * ry.d[a]) / sc.voxel + 0.5f);
      k[a] = L == 1 ? g : g >> 3;            // arithmetic shift: floor division
    }
    s_in = ry.s0;
    budget = sc.max_steps;
    live = true;
  }

  // Examines the current cell and moves to the next: true if the ray has a positive chord in the cell `cell`.
  __device__ __forceinline__ bool step(const Scan& sc, const Ray& ry, int cell[3]) {
    float ex[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float face = (float)(k[a] * L) + (ry.d[a] > 0.f ? (float)L - 0.5f : -0.5f);
      ex[a] = ry.d[a] == 0.f ? INFINITY : (face * sc.voxel - ry.o[a]) / ry.d[a];
      cell[a] = k[a];
    }
    const int ax = ex[0] <= ex[1] ? (ex[0] <= ex[2] ? 0 : 2) : (ex[1] <= ex[2] ? 1 : 2);
    const float s_out = ax == 0 ? ex[0] : ax == 1 ? ex[1] : ex[2];
    const bool hit = fminf(s_out, ry.s1) > s_in;
    if (!(s_out < ry.s1) || --budget <= 0) live = false;
    else {
#pragma unroll
      for (int a = 0; a < 3; ++a)
        if (a == ax) k[a] += ry.d[a] > 0.f ? 1 : -1;
      s_in = fmaxf(s_in, s_out);
    }
    return hit;
  }
};

// counters: [0] touched blocks, [1] new blocks, [2] status bits
__global__ __launch_bounds__(kBlock) void tsdf_points_touch_kernel(Scan sc, const float* __restrict__ points,
                                                                   const float* __restrict__ sensor, i64* tkeys,
                                                                   const int32_t* tslots, int32_t* tstamps,
                                                                   int32_t* tindex, i64 tsize, i64 list_cap,
                                                                   int32_t* __restrict__ touched,
                                                                   i64* __restrict__ new_keys, int32_t* counters) {
  const i64 i = (i64)blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  Ray ry;
  Walker<kB> w;
  w.live = false;
  if (i < sc.n) {
    const int kind = make_ray(sc, points, sensor, i, ry);
    if (kind == 2) atomicOr(&counters[2], PINGS_TSDF_EXTENT);
    if (kind == 1) w.start(sc, ry);
  }
  while (__ballot(w.live)) {               // the whole wave stays in the loop: the election below needs every lane
    bool pend = false;
    i64 key = 0;
    if (w.live) {
      int b[3];
      pend = w.step(sc, ry, b);
      if (pend) {
        pend = in_extent(b[0]) && in_extent(b[1]) && in_extent(b[2]);
        if (pend) key = pack_key(b[0], b[1], b[2]);
        else atomicOr(&counters[2], PINGS_TSDF_EXTENT);
      }
    }
    // one lane per distinct key of the wave goes to memory: neighbouring rays name the same blocks at the same step
    bool owner = false;
    for (;;) {
      const u64 m = __ballot(pend);
      if (!m) break;
      const int leader = __ffsll((long long)m) - 1;
      const i64 kl = __shfl(key, leader, 64);
      if (pend && key == kl) {
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
    if (atomicExch(&tstamps[e], sc.frame) == sc.frame) continue;     // filed earlier in this call
    const i64 at = atomicAdd(&counters[0], 1);
    if (at < list_cap) {
      touched[at] = (int32_t)e;
      tindex[e] = (int32_t)at;
    }
    if (tslots[e] < 0) {                                              // slots are written by the assign launch only
      const i64 an = atomicAdd(&counters[1], 1);
      if (an < list_cap) new_keys[an] = key;
    }
  }
}

// acc [n_touched, planes, 512]: plane 0 holds count << 44 | sum of (q + 2^22), planes 1..3 the colour sums
__global__ __launch_bounds__(kBlock) void tsdf_points_accumulate_kernel(Scan sc, const float* __restrict__ points,
                                                                        const float* __restrict__ colors,
                                                                        const float* __restrict__ sensor,
                                                                        const i64* __restrict__ tkeys,
                                                                        const int32_t* __restrict__ tstamps,
                                                                        const int32_t* __restrict__ tindex, i64 tsize,
                                                                        i64 n_touched, int planes, u64* acc) {
  const i64 i = (i64)blockIdx.x * kBlock + threadIdx.x;
  if (i >= sc.n) return;
  Ray ry;
  if (make_ray(sc, points, sensor, i, ry) != 1) return;
  u64 qc[3] = {0, 0, 0};
  if (planes > 1) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) qc[ch] = (u64)rintf(fminf(fmaxf(colors[3 * i + ch], 0.f), 1.f) * kScale);
  }
  Walker<1> w;
  w.start(sc, ry);
  i64 cur_key = -1, idx = -1;
  while (w.live) {
    int g[3];
    if (!w.step(sc, ry, g)) continue;
    // c - o and p - c in fp64: next to the sensor c - o is a small difference of large numbers, and the sign of
    // (c - o).(p - c) decides between +|p - c| and -|p - c|
    double co[3], pc[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double c = sc.voxel_d * (double)g[a];
      co[a] = c - ry.od[a];
      pc[a] = ry.pd[a] - c;
    }
    float sdf;
    if (sc.ray_mode) sdf = ry.r - (float)(co[0] * (double)ry.d[0] + co[1] * (double)ry.d[1] + co[2] * (double)ry.d[2]);
    else {
      const float dist = (float)sqrt(pc[0] * pc[0] + pc[1] * pc[1] + pc[2] * pc[2]);
      sdf = co[0] * pc[0] + co[1] * pc[1] + co[2] * pc[2] >= 0.0 ? dist : -dist;
    }
    if (!(sdf > -sc.trunc)) continue;
    const i64 key = pack_key(g[0] >> 3, g[1] >> 3, g[2] >> 3);
    if (key != cur_key) {                    // one probe per block of the walk
      cur_key = key;
      const i64 e = table_find(tkeys, tsize, key);
      idx = e >= 0 && tstamps[e] == sc.frame ? (i64)tindex[e] : -1;
      if (idx >= n_touched) idx = -1;
    }
    if (idx < 0) continue;                   // not filed by the block walk: a chord that fp32 cannot tell from zero
    const int l = (g[0] & 7) << 6 | (g[1] & 7) << 3 | (g[2] & 7);
    const i64 q = (i64)rintf(fminf(1.f, sdf / sc.trunc) * kScale);
    u64* row = acc + (idx * planes) * kVox + l;
    atomicAdd(row, ((u64)1 << kCountShift) + (u64)(q + kOffset));
    if (planes > 1) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) atomicAdd(row + (1 + ch) * kVox, qc[ch]);
    }
  }
}

__global__ __launch_bounds__(kBlock) void tsdf_points_apply_kernel(const int32_t* __restrict__ touched,
                                                                   const int32_t* __restrict__ tslots, i64 tsize,
                                                                   i64 capacity, int planes,
                                                                   const u64* __restrict__ acc, float max_weight,
                                                                   float* __restrict__ tsdf, float* __restrict__ weight,
                                                                   float* __restrict__ color) {
  const i64 b = blockIdx.x;
  const int32_t e = touched[b];
  if (e < 0 || e >= tsize) return;
  const i64 slot = tslots[e];
  if (slot < 0 || slot >= capacity) return;
  const double unit = 1.0 / (double)kScale;
#pragma unroll
  for (int l = threadIdx.x; l < kVox; l += kBlock) {
    const u64 a = acc[(b * planes) * kVox + l];
    const i64 n = (i64)(a >> kCountShift);
    if (n == 0) continue;                    // no updating sample: every field keeps its bits
    const i64 sum = (i64)(a & kSumMask) - n * kOffset;
    const i64 o = slot * kVox + l;
    const double w = weight[o], w1 = w + (double)n;
    tsdf[o] = (float)(((double)tsdf[o] * w + (double)sum * unit) / w1);
    if (planes > 1) {
      const i64 oc = slot * 3 * kVox + l;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const double cs = (double)acc[(b * planes + 1 + ch) * kVox + l] * unit;
        color[oc + ch * kVox] = (float)(((double)color[oc + ch * kVox] * w + cs) / w1);
      }
    }
    weight[o] = fminf((float)w1, max_weight);
  }
}

int make_scan(Scan* sc, int64_t n, const double* origin, double voxel_length, double sdf_trunc, float min_range,
              float max_range, int space_carving, int sdf_mode, int frame) {
  PINGS_ARG_CHECK(origin, "null pointer");
  PINGS_ARG_CHECK(n >= 0 && n <= PINGS_TSDF_POINTS_MAX, "a scan holds at most PINGS_TSDF_POINTS_MAX points");
  PINGS_ARG_CHECK(voxel_length > 0.0 && sdf_trunc > 0.0, "voxel_length and sdf_trunc must be positive");
  PINGS_ARG_CHECK(2.0 * sdf_trunc <= kB * voxel_length, "2 sdf_trunc may not exceed the block edge");
  PINGS_ARG_CHECK(min_range >= 0.f && max_range > min_range, "0 <= min_range < max_range");
  PINGS_ARG_CHECK(!space_carving || max_range < INFINITY, "space carving needs a finite max_range");
  PINGS_ARG_CHECK(sdf_mode == PINGS_TSDF_SDF_POINT || sdf_mode == PINGS_TSDF_SDF_RAY, "unknown sdf_mode");
  PINGS_ARG_CHECK(frame >= 1, "frame starts at 1");
  for (int a = 0; a < 3; ++a) sc->org[a] = origin[a];
  sc->voxel_d = voxel_length;
  sc->voxel = (float)voxel_length;
  sc->trunc = (float)sdf_trunc;
  sc->rmin = min_range;
  sc->rmax = max_range;
  sc->carve = space_carving ? 1 : 0;
  sc->ray_mode = sdf_mode == PINGS_TSDF_SDF_RAY;
  sc->frame = frame;
  sc->n = n;
  return PINGS_OK;
}

// More than the cells of edge `cell` a segment of length `len` can cross: one per axis and cell, and the ends.
int step_budget(double len, double cell) {
  const double steps = 3.0 * (floor(len / cell) + 2.0);
  return steps < 1e9 ? (int)steps : 1000000000;
}

}  // namespace

PINGS_API int pings_tsdf_points_touch(const float* points, int64_t n, const float* sensor, const double* origin,
                                      double voxel_length, double sdf_trunc, float min_range, float max_range,
                                      int space_carving, int frame, int64_t* tkeys, const int32_t* tslots,
                                      int32_t* tstamps, int32_t* tindex, int64_t tsize, int64_t list_cap,
                                      int32_t* touched, int64_t* new_keys, int32_t* counters, int64_t* totals,
                                      void* stream) {
  Scan sc;
  if (int e = make_scan(&sc, n, origin, voxel_length, sdf_trunc, min_range, max_range, space_carving,
                        PINGS_TSDF_SDF_POINT, frame))
    return e;
  PINGS_ARG_CHECK(counters && totals, "null pointer");
  PINGS_ARG_CHECK(n == 0 || (points && sensor && tstamps && tindex && touched && new_keys), "null pointer");
  PINGS_ARG_CHECK(table_ok(tkeys, tslots, tsize), "the table is null or its size is no power of two in [64, 2^31)");
  PINGS_ARG_CHECK(list_cap >= 0 && (space_carving || list_cap >= 8 * n), "the lists hold 8 entries per ray");
  const double len = space_carving ? (double)max_range + sdf_trunc : 2.0 * sdf_trunc;
  sc.max_steps = step_budget(len, kB * voxel_length);
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope scope("tsdf_points_touch", st);
  PINGS_HIP_CHECK(hipMemsetAsync(counters, 0, 4 * sizeof(int32_t), st));
  if (n > 0)
    if (int e = pings::launch(tsdf_points_touch_kernel, dim3((unsigned)pings::ceil_div<i64>(n, kBlock)), kBlock, 0, st,
                              sc, points, sensor, tkeys, tslots, tstamps, tindex, tsize, list_cap, touched, new_keys,
                              counters))
      return e;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(counters);
  const uint32_t* src[3] = {w, w + 1, w + 2};
  uint32_t got[3] = {0u, 0u, 0u};
  if (int e = pings::host_read_words(src, 3, got, st)) return e;
  for (int i = 0; i < 3; ++i) totals[i] = (int64_t)got[i];
  return PINGS_OK;
}

PINGS_API int pings_tsdf_points_accumulate(const float* points, const float* colors, int64_t n, const float* sensor,
                                           const double* origin, double voxel_length, double sdf_trunc,
                                           float min_range, float max_range, int space_carving, int sdf_mode,
                                           int frame, const int64_t* tkeys, const int32_t* tslots,
                                           const int32_t* tstamps, const int32_t* tindex, int64_t tsize,
                                           int64_t n_touched, uint64_t* acc, void* stream) {
  Scan sc;
  if (int e = make_scan(&sc, n, origin, voxel_length, sdf_trunc, min_range, max_range, space_carving, sdf_mode, frame))
    return e;
  PINGS_ARG_CHECK(n_touched >= 0 && n_touched < (i64)0x7FFFFFFF, "negative or too large count");
  if (n == 0 || n_touched == 0) return PINGS_OK;
  PINGS_ARG_CHECK(points && sensor && tstamps && tindex && acc, "null pointer");
  PINGS_ARG_CHECK(table_ok(tkeys, tslots, tsize), "the table is null or its size is no power of two in [64, 2^31)");
  const double len = space_carving ? (double)max_range + sdf_trunc : 2.0 * sdf_trunc;
  sc.max_steps = step_budget(len, voxel_length);
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope scope("tsdf_points_accumulate", st);
  return pings::launch(tsdf_points_accumulate_kernel, dim3((unsigned)pings::ceil_div<i64>(n, kBlock)), kBlock, 0, st, sc,
                       points, colors, sensor, tkeys, tstamps, tindex, tsize, n_touched, colors ? 4 : 1,
                       reinterpret_cast<u64*>(acc));
}

PINGS_API int pings_tsdf_points_apply(const int32_t* touched, int64_t n_touched, const int32_t* tslots, int64_t tsize,
                                      int64_t capacity, const uint64_t* acc, int with_color, float max_weight,
                                      float* tsdf, float* weight, float* color, void* stream) {
  PINGS_ARG_CHECK(n_touched >= 0 && n_touched < (i64)0x7FFFFFFF && capacity >= 0, "negative or too large count");
  if (n_touched == 0) return PINGS_OK;
  PINGS_ARG_CHECK(touched && tslots && acc && tsdf && weight, "null pointer");
  PINGS_ARG_CHECK(tsize >= 64, "the table is too small");
  PINGS_ARG_CHECK((color != nullptr) == (with_color != 0), "colour sums go into a colour volume, and only into one");
  PINGS_ARG_CHECK(max_weight >= 1.f, "max_weight is at least 1 (infinity: no cap)");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope scope("tsdf_points_apply", st);
  return pings::launch(tsdf_points_apply_kernel, dim3((unsigned)n_touched), kBlock, 0, st, touched, tslots, tsize,
                       capacity, with_color ? 4 : 1, reinterpret_cast<const u64*>(acc), max_weight, tsdf, weight, color);
}
