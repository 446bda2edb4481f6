// Mesh finishing on the device (pings_amd/mesh_ops.py): what utils/mesher.py:500-530 does with Open3D after marching
// cubes: remove_duplicated_vertices, cluster_connected_triangles + remove_triangles_by_mask, compute_vertex_normals.
// The rules are DESIGN §2.7b and are restated in numpy by tests/mesh_ref.py; both sides give the same integers, and
// the same floats up to the fp32 evaluation of the normals.
//
//   weld      three stable 32-bit radix passes over an index array (z, y, x bit patterns, -0 as +0), run heads by
//             comparing neighbours, the head's position carried along each run by a max-scan, rep[v] = the run's first
//             (smallest, the sort being stable) index, keep = (rep[v] == v), exclusive scan, gather, face rewrite
//   clusters  3F (edge key, face) pairs sorted by key, a lock-free union-find over neighbouring equal keys that always
//             hooks the larger root under the smaller one, one flatten pass, integer counts, roots ranked by a scan
//   normals   (vertex, corner) pairs sorted by vertex, so that a vertex's corners lie in ascending face, then corner
//             order; one thread per vertex adds its corners' face normals in that order
//   compact   used flags, exclusive scan, gather, face rewrite
// The sorts and scans are the library's (devprim.hpp); there is no float atomic, no wait on another workgroup, no
// per-thread array.
#include <algorithm>
#include <utility>

#include "common.hpp"
#include "devprim.hpp"

namespace {

namespace devprim = pings::devprim;
using pings::Carver;
using i64 = int64_t;
using u32 = uint32_t;
using u64 = unsigned long long;
constexpr int kBlock = 256;
constexpr i64 kMaxIndex = (i64)0x7FFFFFFF;   // V and 3F stay below: indices are 32-bit inside the kernels

inline unsigned blocks(i64 n) { return (unsigned)pings::ceil_div<i64>(n > 0 ? n : 1, kBlock); }

// one size for the two scans of this file: the weld runs both through the same temp field
size_t scan_temp(i64 n) {
  return std::max(devprim::exclusive_sum_u32_temp_bytes(n), devprim::inclusive_max_u32_temp_bytes(n));
}

__device__ __forceinline__ i64 gid() { return (i64)blockIdx.x * kBlock + threadIdx.x; }

// ------------------------------------------------------------------------------------------------ weld
// The one place the weld's equality lives on the device (tests/mesh_ref.py: weld_key): the bit pattern with -0 as +0.
__device__ __forceinline__ u32 canon_bits(float x) {
  const u32 b = __float_as_uint(x);
  return b == 0x80000000u ? 0u : b;
}
__device__ __forceinline__ bool finite_bits(u32 b) { return (b & 0x7F800000u) != 0x7F800000u; }

__global__ __launch_bounds__(kBlock) void weld_key_kernel(const float* __restrict__ verts, const u32* __restrict__ idx,
                                                         i64 V, int axis, u32* __restrict__ key, u32* __restrict__ iota) {
  const i64 i = gid();
  if (i >= V) return;
  const u32 v = idx ? idx[i] : (u32)i;
  key[i] = canon_bits(verts[3 * (i64)v + axis]);
  if (iota) iota[i] = (u32)i;
}

// head[i] = i where sorted position i starts a run of equal vertices, else 0 (the max-scan then carries it along)
__global__ __launch_bounds__(kBlock) void weld_heads_kernel(const float* __restrict__ verts, const u32* __restrict__ idx,
                                                           i64 V, u32* __restrict__ head) {
  const i64 i = gid();
  if (i >= V) return;
  bool same = i > 0;
  if (same) {
    const i64 a = idx[i], b = idx[i - 1];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const u32 ka = canon_bits(verts[3 * a + c]), kb = canon_bits(verts[3 * b + c]);
      same = same && ka == kb && finite_bits(ka);
    }
  }
  head[i] = same ? 0u : (u32)i;
}

__global__ __launch_bounds__(kBlock) void weld_rep_kernel(const u32* __restrict__ idx, const u32* __restrict__ headpos,
                                                         i64 V, u32* __restrict__ rep, u32* __restrict__ keep) {
  const i64 i = gid();
  if (i >= V) return;
  const u32 h = headpos[i];            // <= i, a position of this run
  const u32 v = idx[i];
  rep[v] = idx[h];
  keep[v] = h == (u32)i ? 1u : 0u;
}

// rep == nullptr: the compaction form, where a dropped vertex maps to -1
__global__ __launch_bounds__(kBlock) void gather_kept_kernel(const float* __restrict__ verts, const u32* __restrict__ rep,
                                                            const u32* __restrict__ keep, const u32* __restrict__ pos,
                                                            i64 V, float* __restrict__ verts_out,
                                                            i64* __restrict__ remap, i64* __restrict__ kept,
                                                            u32* __restrict__ tot) {
  const i64 v = gid();
  if (v >= V) return;
  const bool k = keep[v] != 0;
  remap[v] = rep ? (i64)pos[rep[v]] : (k ? (i64)pos[v] : (i64)-1);
  if (k) {
    const i64 o = pos[v];              // < V: an exclusive count of flags over [0, v)
    verts_out[3 * o] = verts[3 * v];
    verts_out[3 * o + 1] = verts[3 * v + 1];
    verts_out[3 * o + 2] = verts[3 * v + 2];
    kept[o] = v;
  }
  if (v == V - 1) tot[0] = pos[v] + (k ? 1u : 0u);
}

// tot[1] = 1 if any corner lies outside [0, V); such a corner becomes -1 and indexes nothing
__global__ __launch_bounds__(kBlock) void remap_faces_kernel(const i64* __restrict__ faces, i64 n, i64 V,
                                                            const i64* __restrict__ remap, i64* __restrict__ out,
                                                            u32* __restrict__ tot) {
  const i64 e = gid();
  if (e >= n) return;
  const i64 a = faces[e];
  if (a < 0 || a >= V) {
    out[e] = -1;
    tot[1] = 1u;
    return;
  }
  out[e] = remap[a];
}

__global__ void clear_words_kernel(u32* __restrict__ w, int n) {
  if ((int)threadIdx.x < n) w[threadIdx.x] = 0u;
}

struct WeldScratch {
  u32 *key_a, *key_b, *idx_a, *idx_b, *rep, *keep, *pos, *tot;
  void* temp;
  size_t temp_bytes, total;
};
WeldScratch carve_weld(i64 V, void* base) {
  Carver c(base);
  WeldScratch s{};
  s.key_a = c.take<u32>(V);
  s.key_b = c.take<u32>(V);
  s.idx_a = c.take<u32>(V);
  s.idx_b = c.take<u32>(V);
  s.rep = c.take<u32>(V);
  s.keep = c.take<u32>(V);
  s.pos = c.take<u32>(V);
  s.tot = c.take<u32>(4);
  s.temp_bytes = std::max(devprim::sort_pairs_u32_u32_temp_bytes(V), scan_temp(V));
  s.temp = c.take<char>(s.temp_bytes);
  s.total = c.total();
  return s;
}

// ------------------------------------------------------------------------------------------------ clusters
__device__ __forceinline__ u32 load_parent(const u32* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void store_parent(u32* p, u32 v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// parent[x] <= x always, so every step of the walk goes to a strictly smaller index and the walk ends at a root.
// Path halving on the way: a stored grandparent is an ancestor too, and smaller than x.
__device__ __forceinline__ u32 find_root(u32* parent, u32 x) {
  u32 p = load_parent(parent + x);
  while (p != x) {
    const u32 g = load_parent(parent + p);
    if (g != p) store_parent(parent + x, g);
    x = p;
    p = g;
  }
  return x;
}

// Edge j of face f joins corners j and (j + 1) % 3.  key = min << 32 | max, value = f.  Also parent[f] = f, size[f] = 0.
__global__ __launch_bounds__(kBlock) void edge_keys_kernel(const i64* __restrict__ faces, i64 F, i64 V,
                                                          u64* __restrict__ key, u32* __restrict__ val,
                                                          u32* __restrict__ parent, u32* __restrict__ size,
                                                          u32* __restrict__ tot) {
  const i64 e = gid();
  if (e >= 3 * F) return;
  const i64 f = e / 3;
  const int j = (int)(e - 3 * f);
  i64 a = faces[e], b = faces[3 * f + (j == 2 ? 0 : j + 1)];
  if (a < 0 || a >= V) {
    tot[2] = 1u;      // reported after the host read; the key of a bad corner indexes nothing
    a = V;
  }
  if (b < 0 || b >= V) b = V;
  const i64 lo = a < b ? a : b, hi = a < b ? b : a;
  key[e] = (u64)lo << 32 | (u64)hi;
  val[e] = (u32)f;
  if (j == 0) {
    parent[f] = (u32)f;
    size[f] = 0u;
  }
}

__global__ __launch_bounds__(kBlock) void union_kernel(const u64* __restrict__ key, const u32* __restrict__ val, i64 n,
                                                      u32* __restrict__ parent) {
  const i64 i = gid();
  if (i < 1 || i >= n) return;
  if (key[i] != key[i - 1]) return;
  u32 a = val[i], b = val[i - 1];
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return;
    if (a < b) {
      const u32 t = a;
      a = b;
      b = t;
    }
    // a > b, a was a root when read: hook it under the smaller one.  A failed CAS means another thread hooked a in
    // the meantime (parent[a] < a now), and the next round walks on from there: no waiting, only this retry.
    const u32 old = atomicCAS(parent + a, a, b);
    if (old == a) return;
  }
}

// No union runs in this kernel, so the roots are fixed and every thread reaches its component's root, which is the
// component's smallest face index.  It goes to root[f], not into parent: a late halving store of another thread may
// still put a nearer ancestor there.
__global__ __launch_bounds__(kBlock) void flatten_kernel(u32* __restrict__ parent, i64 F, u32* __restrict__ root,
                                                        u32* __restrict__ size, u32* __restrict__ isroot) {
  const i64 f = gid();
  if (f >= F) return;
  const u32 r = find_root(parent, (u32)f);
  root[f] = r;
  isroot[f] = r == (u32)f ? 1u : 0u;
  // One atomic per distinct root in the wave, not per face: a mesh is mostly one big component, and a face per atomic
  // on that one counter took 5.7 ms at 1.15 M faces.  The first active lane's root is counted in every round.
  const int lane = threadIdx.x & (pings::kWave - 1);
  for (bool todo = true; todo;) {
    const u32 lead = (u32)__builtin_amdgcn_readfirstlane((int)r);
    const bool mine = r == lead;
    const unsigned long long m = __ballot(mine);
    if (mine) {
      if (__ffsll(m) - 1 == lane) atomicAdd(size + lead, (u32)__popcll(m));
      todo = false;
    }
  }
}

__global__ __launch_bounds__(kBlock) void labels_kernel(const u32* __restrict__ root, const u32* __restrict__ rank,
                                                       const u32* __restrict__ isroot, const u32* __restrict__ size,
                                                       i64 F, i64* __restrict__ labels, i64* __restrict__ counts,
                                                       u32* __restrict__ tot) {
  const i64 f = gid();
  if (f >= F) return;
  labels[f] = rank[root[f]];
  if (isroot[f]) counts[rank[f]] = size[f];     // rank[f] < number of roots <= F
  if (f == F - 1) tot[0] = rank[f] + isroot[f];
}

__global__ __launch_bounds__(kBlock) void keep_faces_kernel(const i64* __restrict__ labels, const i64* __restrict__ counts,
                                                           i64 F, i64 min_tri, u32* __restrict__ keep) {
  const i64 f = gid();
  if (f >= F) return;
  const i64 l = labels[f];
  keep[f] = (l >= 0 && l < F && counts[l] >= min_tri) ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void compact_faces_kernel(const i64* __restrict__ faces, const u32* __restrict__ keep,
                                                              const u32* __restrict__ pos, i64 F,
                                                              i64* __restrict__ out, u32* __restrict__ tot) {
  const i64 f = gid();
  if (f >= F) return;
  const bool k = keep[f] != 0;
  if (k) {
    const i64 o = pos[f];              // < F
    out[3 * o] = faces[3 * f];
    out[3 * o + 1] = faces[3 * f + 1];
    out[3 * o + 2] = faces[3 * f + 2];
  }
  if (f == F - 1) tot[1] = pos[f] + (k ? 1u : 0u);
}

struct ClusterScratch {
  u64 *key, *key_sorted;
  u32 *val, *val_sorted, *parent, *root, *size, *isroot, *rank, *tot;   // isroot / rank double as keep / pos of drop_small
  void* temp;
  size_t temp_bytes, total;
};
ClusterScratch carve_clusters(i64 F, void* base) {
  Carver c(base);
  ClusterScratch s{};
  s.tot = c.take<u32>(4);              // clusters, kept faces, bad corner
  s.key = c.take<u64>(3 * F);
  s.key_sorted = c.take<u64>(3 * F);
  s.val = c.take<u32>(3 * F);
  s.val_sorted = c.take<u32>(3 * F);
  s.parent = c.take<u32>(F);
  s.root = c.take<u32>(F);
  s.size = c.take<u32>(F);
  s.isroot = c.take<u32>(F);
  s.rank = c.take<u32>(F);
  s.temp_bytes = std::max(devprim::sort_pairs_u64_u32_temp_bytes(3 * F), scan_temp(F));
  s.temp = c.take<char>(s.temp_bytes);
  s.total = c.total();
  return s;
}

// ------------------------------------------------------------------------------------------------ normals
// key = the corner's vertex, or V for every corner of a face that names a vertex outside [0, V)
__global__ __launch_bounds__(kBlock) void corner_keys_kernel(const i64* __restrict__ faces, i64 F, i64 V,
                                                            u32* __restrict__ key, u32* __restrict__ val) {
  const i64 e = gid();
  if (e >= 3 * F) return;
  const i64 f = e / 3;
  const i64 a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  const bool ok = a >= 0 && a < V && b >= 0 && b < V && c >= 0 && c < V;
  key[e] = ok ? (u32)faces[e] : (u32)V;
  val[e] = (u32)e;
}

__global__ __launch_bounds__(kBlock) void normals_kernel(const float* __restrict__ verts, const i64* __restrict__ faces,
                                                        const u32* __restrict__ key, const u32* __restrict__ val,
                                                        i64 V, i64 n, float* __restrict__ normals) {
  const i64 v = gid();
  if (v >= V) return;
  i64 lo = 0, hi = n;
  while (lo < hi) {
    const i64 mid = lo + ((hi - lo) >> 1);
    if (key[mid] < (u32)v) lo = mid + 1;
    else hi = mid;
  }
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (i64 i = lo; i < n && key[i] == (u32)v; ++i) {
    const i64 f = val[i] / 3u;         // a sorted key < V: all three corners of f were checked
    const i64 a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    const float ax = verts[3 * a], ay = verts[3 * a + 1], az = verts[3 * a + 2];
    const float ux = verts[3 * b] - ax, uy = verts[3 * b + 1] - ay, uz = verts[3 * b + 2] - az;
    const float wx = verts[3 * c] - ax, wy = verts[3 * c + 1] - ay, wz = verts[3 * c + 2] - az;
    sx += uy * wz - uz * wy;
    sy += uz * wx - ux * wz;
    sz += ux * wy - uy * wx;
  }
  const float len = sqrtf(sx * sx + sy * sy + sz * sz);
  float nx = sx / len, ny = sy / len, nz = sz / len;
  if (!(len > 0.f) || !isfinite(nx) || !isfinite(ny) || !isfinite(nz)) {
    nx = 0.f;
    ny = 0.f;
    nz = 1.f;
  }
  normals[3 * v] = nx;
  normals[3 * v + 1] = ny;
  normals[3 * v + 2] = nz;
}

struct NormalScratch {
  u32 *key, *key_sorted, *val, *val_sorted;
  void* temp;
  size_t temp_bytes, total;
};
NormalScratch carve_normals(i64 F, void* base) {
  Carver c(base);
  NormalScratch s{};
  const size_t n = F > 0 ? 3 * (size_t)F : 1;   // a mesh without faces still gets a blob
  s.key = c.take<u32>(n);
  s.key_sorted = c.take<u32>(n);
  s.val = c.take<u32>(n);
  s.val_sorted = c.take<u32>(n);
  s.temp_bytes = devprim::sort_pairs_u32_u32_temp_bytes(3 * F);
  s.temp = c.take<char>(s.temp_bytes);
  s.total = c.total();
  return s;
}

// ------------------------------------------------------------------------------------------------ compact
__global__ __launch_bounds__(kBlock) void clear_kernel(u32* __restrict__ w, i64 n, u32* __restrict__ tot) {
  const i64 i = gid();
  if (i < n) w[i] = 0u;
  if (i < 4) tot[i] = 0u;
}

__global__ __launch_bounds__(kBlock) void mark_used_kernel(const i64* __restrict__ faces, i64 n, i64 V,
                                                          u32* __restrict__ used, u32* __restrict__ tot) {
  const i64 e = gid();
  if (e >= n) return;
  const i64 a = faces[e];
  if (a < 0 || a >= V) tot[1] = 1u;
  else used[a] = 1u;                   // every writer stores the same word
}

struct CompactScratch {
  u32 *used, *pos, *tot;
  void* temp;
  size_t temp_bytes, total;
};
CompactScratch carve_compact(i64 V, void* base) {
  Carver c(base);
  CompactScratch s{};
  s.used = c.take<u32>(V);
  s.pos = c.take<u32>(V);
  s.tot = c.take<u32>(4);
  s.temp_bytes = scan_temp(V);
  s.temp = c.take<char>(s.temp_bytes);
  s.total = c.total();
  return s;
}

bool sizes_ok(i64 V, i64 F) { return V > 0 && V < kMaxIndex && F >= 0 && F < kMaxIndex / 3; }

int bits_for(i64 max_value) {
  int b = 1;
  while (b < 32 && ((i64)1 << b) <= max_value) ++b;
  return b;
}

}  // namespace

PINGS_API size_t pings_mesh_weld_scratch_bytes(int64_t V, int64_t F) {
  return sizes_ok(V, F) ? carve_weld(V, nullptr).total : 0;
}

PINGS_API int pings_mesh_weld(const float* verts, int64_t V, const int64_t* faces, int64_t F, void* scratch,
                              float* verts_out, int64_t* faces_out, int64_t* remap, int64_t* kept, int64_t* n_out,
                              void* stream) {
  PINGS_ARG_CHECK(verts && scratch && verts_out && remap && kept && n_out, "null pointer");
  PINGS_ARG_CHECK(V > 0 && F >= 0, "empty or negative shape");
  PINGS_ARG_CHECK(sizes_ok(V, F), "mesh too large for 32-bit indices");
  PINGS_ARG_CHECK(F == 0 || (faces && faces_out), "null pointer");
  hipStream_t st = pings::as_stream(stream);
  WeldScratch s = carve_weld(V, scratch);
  pings::prof::Scope sc("mesh_weld", st);
  const unsigned nb = blocks(V);
  // z, then y, then x: after the three stable passes equal vertices are neighbours, each run in ascending index
  u32 *idx_cur = s.idx_a, *idx_next = s.idx_b;
  for (int axis = 2; axis >= 0; --axis) {
    const bool first = axis == 2;      // the first pass reads the vertices in order and writes the identity into idx_cur
    hipLaunchKernelGGL(weld_key_kernel, dim3(nb), dim3(kBlock), 0, st, verts, first ? (const u32*)nullptr : idx_cur, V,
                       axis, s.key_a, first ? idx_cur : (u32*)nullptr);
    PINGS_LAUNCH_CHECK();
    if (int e = devprim::sort_pairs_u32_u32(s.temp, s.temp_bytes, s.key_a, s.key_b, idx_cur, idx_next, V, 0, 32, st))
      return e;
    std::swap(idx_cur, idx_next);
  }
  const u32* idx = idx_cur;
  u32 *head = s.key_a, *headpos = s.key_b;
  hipLaunchKernelGGL(weld_heads_kernel, dim3(nb), dim3(kBlock), 0, st, verts, idx, V, head);
  PINGS_LAUNCH_CHECK();
  if (int e = devprim::inclusive_max_u32(s.temp, s.temp_bytes, head, headpos, V, st)) return e;
  hipLaunchKernelGGL(weld_rep_kernel, dim3(nb), dim3(kBlock), 0, st, idx, (const u32*)headpos, V, s.rep, s.keep);
  PINGS_LAUNCH_CHECK();
  if (int e = devprim::exclusive_sum_u32(s.temp, s.temp_bytes, s.keep, s.pos, V, st)) return e;
  hipLaunchKernelGGL(clear_words_kernel, dim3(1), dim3(64), 0, st, s.tot, 4);
  PINGS_LAUNCH_CHECK();
  hipLaunchKernelGGL(gather_kept_kernel, dim3(nb), dim3(kBlock), 0, st, verts, (const u32*)s.rep, (const u32*)s.keep,
                     (const u32*)s.pos, V, verts_out, remap, kept, s.tot);
  PINGS_LAUNCH_CHECK();
  if (F) {
    hipLaunchKernelGGL(remap_faces_kernel, dim3(blocks(3 * F)), dim3(kBlock), 0, st, faces, 3 * F, V,
                       (const i64*)remap, faces_out, s.tot);
    PINGS_LAUNCH_CHECK();
  }
  const u32* src[2] = {s.tot, s.tot + 1};
  u32 got[2] = {0u, 0u};
  if (int e = pings::host_read_words(src, 2, got, st)) return e;
  *n_out = (int64_t)got[0];
  PINGS_ARG_CHECK(got[1] == 0u, "a face names a vertex outside [0, V)");
  return PINGS_OK;
}

PINGS_API size_t pings_mesh_clusters_scratch_bytes(int64_t F) {
  return sizes_ok(1, F) && F > 0 ? carve_clusters(F, nullptr).total : 0;
}
PINGS_API size_t pings_mesh_drop_small_scratch_bytes(int64_t F) { return pings_mesh_clusters_scratch_bytes(F); }

PINGS_API int pings_mesh_clusters(const int64_t* faces, int64_t F, int64_t V, void* scratch, int64_t* labels,
                                  int64_t* counts, int64_t* n_clusters, void* stream) {
  PINGS_ARG_CHECK(faces && scratch && labels && counts, "null pointer");
  PINGS_ARG_CHECK(V > 0 && F > 0, "empty or negative shape");
  PINGS_ARG_CHECK(sizes_ok(V, F), "mesh too large for 32-bit indices");
  hipStream_t st = pings::as_stream(stream);
  ClusterScratch s = carve_clusters(F, scratch);
  pings::prof::Scope sc("mesh_clusters", st);
  const i64 n = 3 * F;
  hipLaunchKernelGGL(clear_words_kernel, dim3(1), dim3(64), 0, st, s.tot, 4);
  PINGS_LAUNCH_CHECK();
  hipLaunchKernelGGL(edge_keys_kernel, dim3(blocks(n)), dim3(kBlock), 0, st, faces, F, V, s.key, s.val, s.parent, s.size,
                     s.tot);
  PINGS_LAUNCH_CHECK();
  const int vb = bits_for(V);          // both halves of a key are <= V
  if (int e = devprim::sort_pairs_u64_u32(s.temp, s.temp_bytes, s.key, s.key_sorted, s.val, s.val_sorted, n, 0, 32 + vb,
                                          st))
    return e;
  hipLaunchKernelGGL(union_kernel, dim3(blocks(n)), dim3(kBlock), 0, st, (const u64*)s.key_sorted,
                     (const u32*)s.val_sorted, n, s.parent);
  PINGS_LAUNCH_CHECK();
  hipLaunchKernelGGL(flatten_kernel, dim3(blocks(F)), dim3(kBlock), 0, st, s.parent, F, s.root, s.size, s.isroot);
  PINGS_LAUNCH_CHECK();
  if (int e = devprim::exclusive_sum_u32(s.temp, s.temp_bytes, s.isroot, s.rank, F, st)) return e;
  hipLaunchKernelGGL(labels_kernel, dim3(blocks(F)), dim3(kBlock), 0, st, (const u32*)s.root, (const u32*)s.rank,
                     (const u32*)s.isroot, (const u32*)s.size, F, labels, counts, s.tot);
  PINGS_LAUNCH_CHECK();
  if (!n_clusters) return PINGS_OK;
  const u32* src[2] = {s.tot, s.tot + 2};
  u32 got[2] = {0u, 0u};
  if (int e = pings::host_read_words(src, 2, got, st)) return e;
  *n_clusters = (int64_t)got[0];
  PINGS_ARG_CHECK(got[1] == 0u, "a face names a vertex outside [0, V)");
  return PINGS_OK;
}

PINGS_API int pings_mesh_drop_small(const int64_t* faces, int64_t F, const int64_t* labels, const int64_t* counts,
                                    int64_t min_tri, void* scratch, int64_t* faces_out, int64_t* totals, void* stream) {
  PINGS_ARG_CHECK(faces && labels && counts && scratch && faces_out && totals, "null pointer");
  PINGS_ARG_CHECK(F > 0, "empty or negative shape");
  PINGS_ARG_CHECK(sizes_ok(1, F), "mesh too large for 32-bit indices");
  hipStream_t st = pings::as_stream(stream);
  ClusterScratch s = carve_clusters(F, scratch);
  pings::prof::Scope sc("mesh_drop_small", st);
  u32 *keep = s.isroot, *pos = s.rank;
  hipLaunchKernelGGL(keep_faces_kernel, dim3(blocks(F)), dim3(kBlock), 0, st, labels, counts, F, min_tri, keep);
  PINGS_LAUNCH_CHECK();
  if (int e = devprim::exclusive_sum_u32(s.temp, s.temp_bytes, keep, pos, F, st)) return e;
  hipLaunchKernelGGL(compact_faces_kernel, dim3(blocks(F)), dim3(kBlock), 0, st, faces, (const u32*)keep,
                     (const u32*)pos, F, faces_out, s.tot);
  PINGS_LAUNCH_CHECK();
  const u32* src[3] = {s.tot, s.tot + 1, s.tot + 2};
  u32 got[3] = {0u, 0u, 0u};
  if (int e = pings::host_read_words(src, 3, got, st)) return e;
  totals[0] = (int64_t)got[0];
  totals[1] = (int64_t)got[1];
  PINGS_ARG_CHECK(got[2] == 0u, "a face names a vertex outside [0, V)");
  return PINGS_OK;
}

PINGS_API size_t pings_mesh_vertex_normals_scratch_bytes(int64_t V, int64_t F) {
  return sizes_ok(V, F) ? carve_normals(F, nullptr).total : 0;
}

PINGS_API int pings_mesh_vertex_normals(const float* verts, int64_t V, const int64_t* faces, int64_t F, void* scratch,
                                        float* normals, void* stream) {
  PINGS_ARG_CHECK(verts && scratch && normals, "null pointer");
  PINGS_ARG_CHECK(V > 0 && F >= 0, "empty or negative shape");
  PINGS_ARG_CHECK(sizes_ok(V, F), "mesh too large for 32-bit indices");
  PINGS_ARG_CHECK(F == 0 || faces, "null pointer");
  hipStream_t st = pings::as_stream(stream);
  NormalScratch s = carve_normals(F, scratch);
  pings::prof::Scope sc("mesh_vertex_normals", st);
  const i64 n = 3 * F;
  if (n) {
    hipLaunchKernelGGL(corner_keys_kernel, dim3(blocks(n)), dim3(kBlock), 0, st, faces, F, V, s.key, s.val);
    PINGS_LAUNCH_CHECK();
    if (int e = devprim::sort_pairs_u32_u32(s.temp, s.temp_bytes, s.key, s.key_sorted, s.val, s.val_sorted, n, 0,
                                            bits_for(V), st))
      return e;
  }
  hipLaunchKernelGGL(normals_kernel, dim3(blocks(V)), dim3(kBlock), 0, st, verts, faces, (const u32*)s.key_sorted,
                     (const u32*)s.val_sorted, V, n, normals);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API size_t pings_mesh_compact_vertices_scratch_bytes(int64_t V, int64_t F) {
  return sizes_ok(V, F) ? carve_compact(V, nullptr).total : 0;
}

PINGS_API int pings_mesh_compact_vertices(const float* verts, int64_t V, const int64_t* faces, int64_t F,
                                          void* scratch, float* verts_out, int64_t* faces_out, int64_t* remap,
                                          int64_t* kept, int64_t* n_out, void* stream) {
  PINGS_ARG_CHECK(verts && scratch && verts_out && remap && kept && n_out, "null pointer");
  PINGS_ARG_CHECK(V > 0 && F >= 0, "empty or negative shape");
  PINGS_ARG_CHECK(sizes_ok(V, F), "mesh too large for 32-bit indices");
  PINGS_ARG_CHECK(F == 0 || (faces && faces_out), "null pointer");
  hipStream_t st = pings::as_stream(stream);
  CompactScratch s = carve_compact(V, scratch);
  pings::prof::Scope sc("mesh_compact_vertices", st);
  hipLaunchKernelGGL(clear_kernel, dim3(blocks(V)), dim3(kBlock), 0, st, s.used, V, s.tot);
  PINGS_LAUNCH_CHECK();
  if (F) {
    hipLaunchKernelGGL(mark_used_kernel, dim3(blocks(3 * F)), dim3(kBlock), 0, st, faces, 3 * F, V, s.used, s.tot);
    PINGS_LAUNCH_CHECK();
  }
  if (int e = devprim::exclusive_sum_u32(s.temp, s.temp_bytes, s.used, s.pos, V, st)) return e;
  hipLaunchKernelGGL(gather_kept_kernel, dim3(blocks(V)), dim3(kBlock), 0, st, verts, (const u32*)nullptr,
                     (const u32*)s.used, (const u32*)s.pos, V, verts_out, remap, kept, s.tot);
  PINGS_LAUNCH_CHECK();
  if (F) {
    // tot[1] already holds the bounds flag; the rewrite sets it again for the same corners
    hipLaunchKernelGGL(remap_faces_kernel, dim3(blocks(3 * F)), dim3(kBlock), 0, st, faces, 3 * F, V,
                       (const i64*)remap, faces_out, s.tot);
    PINGS_LAUNCH_CHECK();
  }
  const u32* src[2] = {s.tot, s.tot + 1};
  u32 got[2] = {0u, 0u};
  if (int e = pings::host_read_words(src, 2, got, st)) return e;
  *n_out = (int64_t)got[0];
  PINGS_ARG_CHECK(got[1] == 0u, "a face names a vertex outside [0, V)");
  return PINGS_OK;
}
