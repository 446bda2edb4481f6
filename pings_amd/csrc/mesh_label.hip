// Labelled meshes on the device (pings_amd/mesh_ops.py): what Mesher.estimate_vertices_sem (utils/mesher.py:393-412)
// does with a colour dict and Open3D's remove_vertices_by_mask.  Rules: DESIGN §2.7c, restated in numpy by
// tests/sem_ref.py.
//
//   label_colors     one thread per vertex: colour = table[label] / 255, drop = label <= 0; a label outside the table,
//                    or one whose `valid` is 0, gets colour 0 and is counted in a device word (an integer atomic), never
//                    indexed
//   remove_vertices  keep flags, exclusive scan, gather (kept vertices keep their order), a face is kept iff its three
//                    corners are, second scan, faces rewritten in order; one host read carries both counts, the bounds
//                    flag and the caller's count of bad labels
// The scans are the library's (devprim.hpp); no float atomic, no per-thread array.
#include <algorithm>

#include "common.hpp"
#include "devprim.hpp"

namespace {

namespace devprim = pings::devprim;
using pings::Carver;
using i64 = int64_t;
using u32 = uint32_t;
constexpr int kBlock = 256;
constexpr i64 kMaxIndex = (i64)0x7FFFFFFF;   // V and 3F stay below: indices are 32-bit inside the kernels

inline unsigned blocks(i64 n) { return (unsigned)pings::ceil_div<i64>(n > 0 ? n : 1, kBlock); }
bool sizes_ok(i64 V, i64 F) { return V > 0 && V < kMaxIndex && F >= 0 && F < kMaxIndex / 3; }

__device__ __forceinline__ i64 gid() { return (i64)blockIdx.x * kBlock + threadIdx.x; }

__global__ __launch_bounds__(kBlock) void label_colors_kernel(const i64* __restrict__ labels, i64 V,
                                                             const uint8_t* __restrict__ table,
                                                             const uint8_t* __restrict__ valid, i64 T,
                                                             float* __restrict__ colors, uint8_t* __restrict__ drop,
                                                             int32_t* __restrict__ bad) {
  const i64 v = gid();
  if (v >= V) return;
  const i64 l = labels[v];
  const bool ok = l >= 0 && l < T && valid[l] != 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) colors[3 * v + c] = ok ? (float)table[3 * l + c] / 255.f : 0.f;
  drop[v] = l <= 0 ? 1 : 0;
  if (!ok) atomicAdd(bad, 1);
}

__global__ __launch_bounds__(kBlock) void keep_vertices_kernel(const uint8_t* __restrict__ drop, i64 V,
                                                              u32* __restrict__ keep, u32* __restrict__ tot) {
  const i64 v = gid();
  if (v < V) keep[v] = drop[v] ? 0u : 1u;
  if (v < 4) tot[v] = 0u;
}

__global__ __launch_bounds__(kBlock) void gather_vertices_kernel(const float* __restrict__ verts,
                                                                const u32* __restrict__ keep,
                                                                const u32* __restrict__ pos, i64 V,
                                                                float* __restrict__ verts_out, i64* __restrict__ remap,
                                                                i64* __restrict__ kept, u32* __restrict__ tot) {
  const i64 v = gid();
  if (v >= V) return;
  const bool k = keep[v] != 0;
  remap[v] = k ? (i64)pos[v] : (i64)-1;
  if (k) {
    const i64 o = pos[v];              // < V: an exclusive count of flags over [0, v)
    verts_out[3 * o] = verts[3 * v];
    verts_out[3 * o + 1] = verts[3 * v + 1];
    verts_out[3 * o + 2] = verts[3 * v + 2];
    kept[o] = v;
  }
  if (v == V - 1) tot[0] = pos[v] + (k ? 1u : 0u);
}

// tot[2] = 1 if any corner lies outside [0, V); such a face is dropped and indexes nothing
__global__ __launch_bounds__(kBlock) void keep_faces_kernel(const i64* __restrict__ faces, i64 F, i64 V,
                                                           const i64* __restrict__ remap, u32* __restrict__ fkeep,
                                                           u32* __restrict__ tot) {
  const i64 f = gid();
  if (f >= F) return;
  bool k = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const i64 a = faces[3 * f + c];
    if (a < 0 || a >= V) {
      tot[2] = 1u;
      k = false;
    } else {
      k = k && remap[a] >= 0;
    }
  }
  fkeep[f] = k ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void gather_faces_kernel(const i64* __restrict__ faces, i64 F,
                                                             const i64* __restrict__ remap,
                                                             const u32* __restrict__ fkeep,
                                                             const u32* __restrict__ fpos, i64* __restrict__ faces_out,
                                                             u32* __restrict__ tot) {
  const i64 f = gid();
  if (f >= F) return;
  const bool k = fkeep[f] != 0;
  if (k) {                             // a kept face has its three corners inside [0, V) and kept
    const i64 o = fpos[f];             // < F
#pragma unroll
    for (int c = 0; c < 3; ++c) faces_out[3 * o + c] = remap[faces[3 * f + c]];
  }
  if (f == F - 1) tot[1] = fpos[f] + (k ? 1u : 0u);
}

struct RemoveScratch {
  u32 *keep, *pos, *fkeep, *fpos, *tot;
  void* temp;
  size_t temp_bytes, total;
};
RemoveScratch carve_remove(i64 V, i64 F, void* base) {
  Carver c(base);
  RemoveScratch s{};
  s.keep = c.take<u32>(V);
  s.pos = c.take<u32>(V);
  s.fkeep = c.take<u32>(F > 0 ? F : 1);
  s.fpos = c.take<u32>(F > 0 ? F : 1);
  s.tot = c.take<u32>(4);
  s.temp_bytes = std::max(devprim::exclusive_sum_u32_temp_bytes(V), devprim::exclusive_sum_u32_temp_bytes(F));
  s.temp = c.take<char>(s.temp_bytes);
  s.total = c.total();
  return s;
}

}  // namespace

PINGS_API int pings_mesh_label_colors(const int64_t* labels, int64_t V, const uint8_t* table, const uint8_t* valid,
                                      int64_t T, float* colors, uint8_t* drop, int32_t* bad, void* stream) {
  PINGS_ARG_CHECK(labels && table && valid && colors && drop && bad, "null pointer");
  PINGS_ARG_CHECK(V > 0 && V < kMaxIndex && T > 0 && T < kMaxIndex, "empty or oversize shape");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("mesh_label_colors", st);
  return pings::launch(label_colors_kernel, dim3(blocks(V)), kBlock, 0, st, labels, V, table, valid, T, colors, drop,
                       bad);
}

PINGS_API size_t pings_mesh_remove_vertices_scratch_bytes(int64_t V, int64_t F) {
  return sizes_ok(V, F) ? carve_remove(V, F, nullptr).total : 0;
}

PINGS_API int pings_mesh_remove_vertices(const float* verts, int64_t V, const int64_t* faces, int64_t F,
                                         const uint8_t* drop, const int32_t* bad, void* scratch, float* verts_out,
                                         int64_t* faces_out, int64_t* remap, int64_t* kept, int64_t* totals,
                                         void* stream) {
  PINGS_ARG_CHECK(verts && drop && scratch && verts_out && remap && kept && totals, "null pointer");
  PINGS_ARG_CHECK(V > 0 && F >= 0, "empty or negative shape");
  PINGS_ARG_CHECK(sizes_ok(V, F), "mesh too large for 32-bit indices");
  PINGS_ARG_CHECK(F == 0 || (faces && faces_out), "null pointer");
  hipStream_t st = pings::as_stream(stream);
  RemoveScratch s = carve_remove(V, F, scratch);
  pings::prof::Scope sc("mesh_remove_vertices", st);
  if (int e = pings::launch(keep_vertices_kernel, dim3(blocks(V)), kBlock, 0, st, drop, V, s.keep, s.tot)) return e;
  if (int e = devprim::exclusive_sum_u32(s.temp, s.temp_bytes, s.keep, s.pos, V, st)) return e;
  if (int e = pings::launch(gather_vertices_kernel, dim3(blocks(V)), kBlock, 0, st, verts, (const u32*)s.keep,
                            (const u32*)s.pos, V, verts_out, remap, kept, s.tot))
    return e;
  if (F) {
    if (int e = pings::launch(keep_faces_kernel, dim3(blocks(F)), kBlock, 0, st, faces, F, V, (const i64*)remap, s.fkeep,
                              s.tot))
      return e;
    if (int e = devprim::exclusive_sum_u32(s.temp, s.temp_bytes, s.fkeep, s.fpos, F, st)) return e;
    if (int e = pings::launch(gather_faces_kernel, dim3(blocks(F)), kBlock, 0, st, faces, F, (const i64*)remap,
                              (const u32*)s.fkeep, (const u32*)s.fpos, faces_out, s.tot))
      return e;
  }
  // one record: kept vertices, kept faces, the bounds flag, the caller's count of bad labels
  const u32* src[4] = {s.tot, s.tot + 1, s.tot + 2, bad ? reinterpret_cast<const u32*>(bad) : s.tot + 3};
  u32 got[4] = {0u, 0u, 0u, 0u};
  if (int e = pings::host_read_words(src, 4, got, st)) return e;
  totals[0] = (int64_t)got[0];
  totals[1] = (int64_t)got[1];
  totals[2] = (int64_t)got[3];
  PINGS_ARG_CHECK(got[2] == 0u, "a face names a vertex outside [0, V)");
  return PINGS_OK;
}
