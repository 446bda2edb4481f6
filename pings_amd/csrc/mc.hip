// Marching cubes on the device (pings_amd/mesher_ops.py: marching_cubes), the step that follows `Mesher.query_points`
// in utils/mesher.py:363-389 (skimage there).  The geometry rules are DESIGN §2.7 and are restated in numpy by
// tests/mc_ref.py; both sides must produce the same bits in the same order.
//
// One thread per grid point p = (i*ny + j)*nz + k, 256 consecutive points per workgroup, so the volume is read along
// its contiguous last axis.  Thread p owns cell p (lowest corner p) and the four vertex keys 4p + slot (slot 0 = the
// point itself, 1..3 = its +x, +y, +z edge).  A key is emitted iff a kept face of one of the 8 cells around p uses it.
//   count   per-block vertex and face counts -> two inclusive scans -> totals, read once by the host
//   verts   recounts, scans the block, writes keys (sorted by construction) and positions at the block's offset
//   faces   retriangulates cell p and writes its faces, each key resolved by binary search in its owner block's slice
// No atomics, no per-cell state: the workspace is O(points / 256).

#include "common.hpp"
#include "devprim.hpp"

namespace {

using i64 = int64_t;
constexpr int kBlock = 256;

struct Grid {
  const float* vol;
  const uint8_t* mask;
  i64 nx, ny, nz;
  float level;
  int flags;
};

// DESIGN §2.7 "processed cells": skimage's mask read as gating the cell's lowest corner, plus all 8 corners finite.
// The one place this rule lives on the device (tests/mc_ref.py: processed).
__device__ __forceinline__ bool processed(const Grid& g, i64 base, const float (&v)[8]) {
  if (g.mask && !g.mask[base]) return false;
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) ok = ok && isfinite(v[c]);
  return ok;
}

// Edge e = 4a + o1 + 2*o2: axis a, (o1, o2) the corner bits of the two other axes in increasing axis order.
// Corner c = di + 2 dj + 4 dk.
__host__ __device__ constexpr int edge_axis(int e) { return e >> 2; }
__host__ __device__ constexpr int edge_lo(int e) {
  return edge_axis(e) == 0 ? ((e & 1) << 1) | ((e >> 1 & 1) << 2)
       : edge_axis(e) == 1 ? (e & 1) | ((e >> 1 & 1) << 2)
                           : (e & 1) | ((e >> 1 & 1) << 1);
}
__host__ __device__ constexpr int edge_of(int ca, int cb) {   // the edge between corners differing in one bit
  const int lo = ca & cb, a = (ca ^ cb) == 1 ? 0 : (ca ^ cb) == 2 ? 1 : 2;
  const int o1 = a == 0 ? (lo >> 1 & 1) : (lo & 1);
  const int o2 = a == 2 ? (lo >> 1 & 1) : (lo >> 2 & 1);
  return 4 * a + o1 + 2 * o2;
}
// Face (a, s): corners counter-clockwise about the outward normal, (u, w) = ((a+1)%3, (a+2)%3).
__host__ __device__ constexpr int face_corner(int a, int s, int m) {
  const int u = (a + 1) % 3, w = (a + 2) % 3;
  const int cu = s ? (m == 1 || m == 2) : (m == 2 || m == 3);
  const int cw = s ? (m == 2 || m == 3) : (m == 1 || m == 2);
  return (s << a) | (cu << u) | (cw << w);
}

// Key of the vertex on the crossing edge from point p0 (value v0, coordinate x0 along axis a) to p0 + stride.
__device__ __forceinline__ float edge_coord(float x0, float v0, float v1, float level) {
  const float t = (level - v0) / (v1 - v0);
  return x0 + t;
}
__device__ __forceinline__ i64 edge_key(i64 p0, i64 stride, int a, i64 ia, float v0, float v1, float level) {
  const float c = edge_coord((float)ia, v0, v1, level);
  if (c == (float)ia) return 4 * p0;
  if (c == (float)(ia + 1)) return 4 * (p0 + stride);
  return 4 * p0 + 1 + a;
}

// The 12 edge keys of a cell are read back by a run-time edge index: a column of LDS per thread, key e at
// [e * kBlock] (as a register array the compiler puts them in scratch).  One buffer for every caller.
__device__ __noinline__ i64* key_column() {
  __shared__ i64 s_key[12 * kBlock];
  return &s_key[threadIdx.x];
}

// Triangulates cell (i, j, k) and calls emit(k0, k1, k2) for every kept face in order; returns their number.
template <class F>
__device__ int cell_faces(const Grid& g, i64 i, i64 j, i64 k, F&& emit) {
  const i64 sx = g.ny * g.nz, sy = g.nz;
  const i64 base = (i * g.ny + j) * g.nz + k;
  float v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = g.vol[base + (c & 1) * sx + (c >> 1 & 1) * sy + (c >> 2 & 1)];
  unsigned below = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) below |= (v[c] < g.level ? 1u : 0u) << c;
  if (below == 0 || below == 255) return 0;
  if (!processed(g, base, v)) return 0;

  i64* key = key_column();
  unsigned cm = 0;
#pragma unroll
  for (int e = 0; e < 12; ++e) {
    const int a = edge_axis(e), lo = edge_lo(e), hi = lo | (1 << a);
    if (((below >> lo) ^ (below >> hi)) & 1) {
      cm |= 1u << e;
      const i64 p0 = base + (lo & 1) * sx + (lo >> 1 & 1) * sy + (lo >> 2 & 1);
      const i64 stride = a == 0 ? sx : a == 1 ? sy : 1;
      const i64 ia = (a == 0 ? i : a == 1 ? j : k) + (lo >> a & 1);
      key[e * kBlock] = edge_key(p0, stride, a, ia, v[lo], v[hi], g.level);
    }
  }
  // segments exit -> entry on every face: nxt holds the successor edge of each crossing edge
  uint64_t nxt = 0;
#pragma unroll
  for (int f = 0; f < 6; ++f) {
    const int a = f >> 1, s = f & 1;
    const int q0 = face_corner(a, s, 0), q1 = face_corner(a, s, 1), q2 = face_corner(a, s, 2), q3 = face_corner(a, s, 3);
    const int e0 = edge_of(q0, q1), e1 = edge_of(q1, q2), e2 = edge_of(q2, q3), e3 = edge_of(q3, q0);
    const unsigned b0 = below >> q0 & 1, b1 = below >> q1 & 1, b2 = below >> q2 & 1, b3 = below >> q3 & 1;
    const int ex[4] = {e0, e1, e2, e3};
    const unsigned bl[4] = {b0, b1, b2, b3};
    const bool amb = b0 == b2 && b1 == b3 && b0 != b1;
    bool conn = false;
    if (amb) {
      const float f0 = v[q0] - g.level, f1 = v[q1] - g.level, f2 = v[q2] - g.level, f3 = v[q3] - g.level;
      const float p02 = f0 * f2, p13 = f1 * f3;
      conn = b0 ? p02 > p13 : p13 > p02;
    }
    int entry = 0;
#pragma unroll
    for (int m = 0; m < 4; ++m)
      if (!bl[m] && bl[(m + 1) & 3]) entry = m;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      if (bl[m] && !bl[(m + 1) & 3]) {
        const int partner = amb ? (conn ? (m + 1) & 3 : (m + 3) & 3) : entry;
        int pe = ex[0];
#pragma unroll
        for (int q = 1; q < 4; ++q) pe = partner == q ? ex[q] : pe;
        nxt |= (uint64_t)pe << (4 * ex[m]);
      }
    }
  }
  const bool keep_degenerate = g.flags & PINGS_MC_ALLOW_DEGENERATE, ascent = g.flags & PINGS_MC_ASCENT;
  int nf = 0;
  unsigned todo = cm;
  while (todo) {
    const int s = __builtin_ctz(todo);
    uint64_t seq = 0;
    int n = 0, e = s, bm = 0;
    i64 best = 0;
    do {
      todo &= ~(1u << e);
      const i64 kk = key[e * kBlock];
      if (n == 0 || kk < best) { best = kk; bm = n; }
      seq |= (uint64_t)e << (4 * n);
      ++n;
      e = (int)(nxt >> (4 * e) & 15);
    } while (e != s && n < 12);
    for (int t = 1; t + 1 < n; ++t) {
      int ia = bm + t, ib = bm + t + 1;
      ia -= ia >= n ? n : 0;
      ib -= ib >= n ? n : 0;
      const i64 ka = key[(seq >> (4 * ia) & 15) * kBlock], kb = key[(seq >> (4 * ib) & 15) * kBlock];
      if (!keep_degenerate && (ka == best || kb == best || ka == kb)) continue;
      if (ascent) emit(best, kb, ka);
      else emit(best, ka, kb);
      ++nf;
    }
  }
  return nf;
}

struct PointIdx {
  i64 p, i, j, k;
  bool in;
};
__device__ __forceinline__ PointIdx point_of(const Grid& g) {
  PointIdx q;
  q.p = (i64)blockIdx.x * kBlock + threadIdx.x;
  q.in = q.p < g.nx * g.ny * g.nz;
  q.k = q.p % g.nz;
  q.j = (q.p / g.nz) % g.ny;
  q.i = q.p / (g.nz * g.ny);
  return q;
}
__device__ __forceinline__ bool has_cell(const Grid& g, i64 i, i64 j, i64 k) {
  return i >= 0 && j >= 0 && k >= 0 && i < g.nx - 1 && j < g.ny - 1 && k < g.nz - 1;
}

// Bit `slot` set iff key 4p + slot is used by a kept face of one of the 8 cells that have p as a corner.
__device__ unsigned vertex_slots(const Grid& g, const PointIdx& q) {
  if (!q.in) return 0;
  // a vertex owned by p lies on an edge at p, which crosses only if a neighbour's state differs from p's
  const i64 sx = g.ny * g.nz, sy = g.nz;
  const bool bp = g.vol[q.p] < g.level;
  bool mixed = false;
  if (q.i > 0) mixed |= (g.vol[q.p - sx] < g.level) != bp;
  if (q.i + 1 < g.nx) mixed |= (g.vol[q.p + sx] < g.level) != bp;
  if (q.j > 0) mixed |= (g.vol[q.p - sy] < g.level) != bp;
  if (q.j + 1 < g.ny) mixed |= (g.vol[q.p + sy] < g.level) != bp;
  if (q.k > 0) mixed |= (g.vol[q.p - 1] < g.level) != bp;
  if (q.k + 1 < g.nz) mixed |= (g.vol[q.p + 1] < g.level) != bp;
  if (!mixed) return 0;
  unsigned bits = 0;
  const i64 p = q.p;
  auto mark = [&](i64 a, i64 b, i64 c) {
    if ((a >> 2) == p) bits |= 1u << (a & 3);
    if ((b >> 2) == p) bits |= 1u << (b & 3);
    if ((c >> 2) == p) bits |= 1u << (c & 3);
  };
  for (int c = 0; c < 8; ++c) {
    const i64 ci = q.i - (c & 1), cj = q.j - (c >> 1 & 1), ck = q.k - (c >> 2 & 1);
    if (has_cell(g, ci, cj, ck)) cell_faces(g, ci, cj, ck, mark);
  }
  return bits;
}

__device__ __forceinline__ int cell_count(const Grid& g, const PointIdx& q) {
  if (!q.in || !has_cell(g, q.i, q.j, q.k)) return 0;
  return cell_faces(g, q.i, q.j, q.k, [](i64, i64, i64) {});
}

// Exclusive scan of one int per thread over the workgroup; *total = the workgroup's sum.
__device__ int block_exclusive_scan(int x, int* total) {
  __shared__ int wsum[kBlock / pings::kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = x;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(incl, off, 64);
    if (lane >= off) incl += y;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kBlock / pings::kWave; ++w) {
    before += w < wave ? wsum[w] : 0;
    all += wsum[w];
  }
  __syncthreads();
  *total = all;
  return before + incl - x;
}

__global__ __launch_bounds__(kBlock) void mc_count_kernel(Grid g, i64* __restrict__ vcnt, i64* __restrict__ fcnt) {
  const PointIdx q = point_of(g);
  const int nv = __builtin_popcount(vertex_slots(g, q));
  const int nf = cell_count(g, q);
  int tv, tf;
  block_exclusive_scan(nv, &tv);
  block_exclusive_scan(nf, &tf);
  if (threadIdx.x == 0) {
    vcnt[blockIdx.x] = tv;
    fcnt[blockIdx.x] = tf;
  }
}

__global__ void mc_totals_kernel(const i64* __restrict__ voff, const i64* __restrict__ foff, i64 nb, i64* __restrict__ tot) {
  if (threadIdx.x == 0) {
    tot[0] = voff[nb - 1];
    tot[1] = foff[nb - 1];
  }
}

__global__ __launch_bounds__(kBlock) void mc_verts_kernel(Grid g, const i64* __restrict__ voff, i64 nv,
                                                          i64* __restrict__ keys, float* __restrict__ verts) {
  const PointIdx q = point_of(g);
  const unsigned bits = vertex_slots(g, q);
  int tot;
  const int r0 = block_exclusive_scan(__builtin_popcount(bits), &tot);
  if (!bits) return;
  i64 o = (blockIdx.x ? voff[blockIdx.x - 1] : 0) + r0;
  const i64 sx = g.ny * g.nz, sy = g.nz;
  const float x[3] = {(float)q.i, (float)q.j, (float)q.k};
  for (int slot = 0; slot < 4; ++slot) {
    if (!(bits >> slot & 1) || o >= nv) continue;
    float c[3] = {x[0], x[1], x[2]};
    if (slot) {
      const int a = slot - 1;
      const i64 stride = a == 0 ? sx : a == 1 ? sy : 1;
      const float ca = edge_coord(x[a], g.vol[q.p], g.vol[q.p + stride], g.level);
      c[0] = a == 0 ? ca : c[0];
      c[1] = a == 1 ? ca : c[1];
      c[2] = a == 2 ? ca : c[2];
    }
    keys[o] = 4 * q.p + slot;
    verts[3 * o] = c[0];
    verts[3 * o + 1] = c[1];
    verts[3 * o + 2] = c[2];
    ++o;
  }
}

__device__ __forceinline__ i64 find_vertex(const i64* __restrict__ keys, const i64* __restrict__ voff, i64 key) {
  const i64 ob = (key >> 2) / kBlock;
  i64 lo = ob ? voff[ob - 1] : 0, hi = voff[ob];
  while (lo < hi) {
    const i64 mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;   // present by construction: a key used by a kept face is an emitted vertex of its owner
}

__global__ __launch_bounds__(kBlock) void mc_faces_kernel(Grid g, const i64* __restrict__ voff,
                                                          const i64* __restrict__ foff, const i64* __restrict__ keys,
                                                          i64 nf_total, i64* __restrict__ faces) {
  const PointIdx q = point_of(g);
  const int nf = cell_count(g, q);
  int tot;
  const int r0 = block_exclusive_scan(nf, &tot);
  if (!nf) return;
  i64 o = (blockIdx.x ? foff[blockIdx.x - 1] : 0) + r0;
  cell_faces(g, q.i, q.j, q.k, [&](i64 a, i64 b, i64 c) {
    if (o >= nf_total) return;
    faces[3 * o] = find_vertex(keys, voff, a);
    faces[3 * o + 1] = find_vertex(keys, voff, b);
    faces[3 * o + 2] = find_vertex(keys, voff, c);
    ++o;
  });
}

struct Scratch {
  i64 *vcnt, *fcnt, *voff, *foff, *tot;
  void* temp;
  size_t temp_bytes, total;
};

Scratch carve(i64 nb, void* base) {
  pings::Carver c(base);
  Scratch s{};
  s.vcnt = c.take<i64>((size_t)nb);
  s.fcnt = c.take<i64>((size_t)nb);
  s.voff = c.take<i64>((size_t)nb);
  s.foff = c.take<i64>((size_t)nb);
  s.tot = c.take<i64>(2);
  s.temp_bytes = pings::devprim::inclusive_sum_i64_temp_bytes(nb);
  s.temp = c.take<char>(s.temp_bytes);
  s.total = c.total();
  return s;
}

constexpr i64 kMaxPoints = (i64)1 << 40;   // keys are 4p + slot and the block count must fit an int

int check_args(const float* vol, i64 nx, i64 ny, i64 nz, int flags, const void* scratch) {
  PINGS_ARG_CHECK(vol && scratch, "null pointer");
  PINGS_ARG_CHECK(nx > 0 && ny > 0 && nz > 0, "empty or negative shape");
  PINGS_ARG_CHECK(nx <= kMaxPoints / ny && nx * ny <= kMaxPoints / nz, "grid too large");
  PINGS_ARG_CHECK(pings::ceil_div<i64>(nx * ny * nz, kBlock) < (i64)0x7FFFFFFF, "grid too large");
  PINGS_ARG_CHECK((flags & ~(PINGS_MC_ALLOW_DEGENERATE | PINGS_MC_ASCENT)) == 0, "unknown flags");
  return PINGS_OK;
}

}  // namespace

PINGS_API size_t pings_mc_scratch_bytes(int64_t nx, int64_t ny, int64_t nz) {
  if (nx <= 0 || ny <= 0 || nz <= 0 || nx > kMaxPoints / ny || nx * ny > kMaxPoints / nz) return 0;
  return carve(pings::ceil_div<i64>(nx * ny * nz, kBlock), nullptr).total;
}

PINGS_API int pings_mc_count(const float* vol, const uint8_t* mask, int64_t nx, int64_t ny, int64_t nz, float level,
                             int flags, void* scratch, int64_t* totals, void* stream) {
  if (int e = check_args(vol, nx, ny, nz, flags, scratch)) return e;
  PINGS_ARG_CHECK(totals, "null pointer");
  hipStream_t st = pings::as_stream(stream);
  const i64 nb = pings::ceil_div<i64>(nx * ny * nz, kBlock);
  Scratch s = carve(nb, scratch);
  const Grid g{vol, mask, nx, ny, nz, level, flags};
  pings::prof::Scope sc("mc_count", st);
  hipLaunchKernelGGL(mc_count_kernel, dim3((unsigned)nb), dim3(kBlock), 0, st, g, s.vcnt, s.fcnt);
  PINGS_LAUNCH_CHECK();
  if (int e = pings::devprim::inclusive_sum_i64(s.temp, s.temp_bytes, s.vcnt, s.voff, nb, st)) return e;
  if (int e = pings::devprim::inclusive_sum_i64(s.temp, s.temp_bytes, s.fcnt, s.foff, nb, st)) return e;
  hipLaunchKernelGGL(mc_totals_kernel, dim3(1), dim3(64), 0, st, s.voff, s.foff, nb, s.tot);
  PINGS_LAUNCH_CHECK();
  const uint32_t* w = reinterpret_cast<const uint32_t*>(s.tot);
  const uint32_t* src[4] = {w, w + 1, w + 2, w + 3};
  uint32_t got[4] = {0u, 0u, 0u, 0u};
  if (int e = pings::host_read_words(src, 4, got, st)) return e;
  totals[0] = (int64_t)((uint64_t)got[0] | (uint64_t)got[1] << 32);
  totals[1] = (int64_t)((uint64_t)got[2] | (uint64_t)got[3] << 32);
  return PINGS_OK;
}

PINGS_API int pings_mc_emit(const float* vol, const uint8_t* mask, int64_t nx, int64_t ny, int64_t nz, float level,
                            int flags, const void* scratch, int64_t nv, int64_t nf, int64_t* keys, float* verts,
                            int64_t* faces, void* stream) {
  if (int e = check_args(vol, nx, ny, nz, flags, scratch)) return e;
  PINGS_ARG_CHECK(nv >= 0 && nf >= 0, "negative count");
  PINGS_ARG_CHECK((nv == 0 || (keys && verts)) && (nf == 0 || faces), "null pointer");
  if (nv == 0) return PINGS_OK;
  hipStream_t st = pings::as_stream(stream);
  const i64 nb = pings::ceil_div<i64>(nx * ny * nz, kBlock);
  Scratch s = carve(nb, const_cast<void*>(scratch));
  const Grid g{vol, mask, nx, ny, nz, level, flags};
  pings::prof::Scope sc("mc_emit", st);
  // offsets come from the pings_mc_count call on the same inputs that gave nv / nf; writes stop at nv / nf regardless
  hipLaunchKernelGGL(mc_verts_kernel, dim3((unsigned)nb), dim3(kBlock), 0, st, g, s.voff, nv, keys, verts);
  PINGS_LAUNCH_CHECK();
  if (nf) {
    hipLaunchKernelGGL(mc_faces_kernel, dim3((unsigned)nb), dim3(kBlock), 0, st, g, s.voff, s.foff, keys, nf, faces);
    PINGS_LAUNCH_CHECK();
  }
  return PINGS_OK;
}
