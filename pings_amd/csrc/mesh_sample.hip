// Surface sampling of a triangle mesh on the device, for gfx950: the cloud that the reference's
// `eval_mesh` (eval/eval_mesh_utils.py:8-60) scores, with its bounding-box crop fused in.  The contract is restated in
// numpy by tests/mesh_sample_ref.py; the output is bit-equal to it and bitwise the same from run to run.
//   areas      one thread per triangle: 0.5 |(v1 - v0) x (v2 - v0)| in fp64, 0 for a triangle with a vertex outside the
//              inclusive box (Open3D's `crop`: no compaction, a dropped triangle owns no samples), with a corner index
//              outside [0, V) or with a non-finite vertex; quantised once to q = llrint(A * 2^32), an int64 count.
//   scan       Q = inclusive sum of q (devprim).  Integer sums: the allocation does not depend on the scan's order.
//   sampling   one thread per point i: the first triangle t with llrint(Q_t * N / Q) > i by a binary search over Q,
//              barycentrics from splitmix64 keyed on (seed, i), the point in fp64, rounded to fp32 once.
// Neighbouring lanes own neighbouring points, so a wave's searches read the same few cache lines of Q at every level;
// the kernel stores 12 B (16 B with `tri`) per point.  One search per thread is the form kept: bracketing the lanes'
// searches by two wave-uniform ones was measured and is slower.  No float atomics; the only atomic is the OR into *status.
// No entry point here allocates, copies or waits.
#include <cmath>

#include "common.hpp"
#include "devprim.hpp"

namespace {

namespace devprim = pings::devprim;
using i64 = long long;
using u64 = unsigned long long;

constexpr int kBlock = 256;
constexpr i64 kMaxCount = ((i64)1 << 31) - 1;                              // F, V and N each fit an int
constexpr double kUnit = (double)((i64)1 << PINGS_MESH_SAMPLE_UNIT_BITS);  // quanta per square metre
constexpr double kInvU32 = 1.0 / 4294967296.0;

inline unsigned blocks_for(i64 n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// the largest q one triangle may hold: F * cap <= 2^PINGS_MESH_SAMPLE_SUM_BITS, so Q never overflows an int64
inline i64 area_cap(i64 F) { return ((i64)1 << PINGS_MESH_SAMPLE_SUM_BITS) / F; }

__device__ __forceinline__ bool finite3(const float* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

__device__ __forceinline__ bool in_box(const float* v, const double* box) {
  return (double)v[0] >= box[0] && (double)v[0] <= box[3] && (double)v[1] >= box[1] && (double)v[1] <= box[4] &&
         (double)v[2] >= box[2] && (double)v[2] <= box[5];
}

__global__ __launch_bounds__(kBlock) void area_kernel(const float* __restrict__ verts, i64 V,
                                                      const int64_t* __restrict__ faces, i64 F,
                                                      const double* __restrict__ box, i64 cap, int64_t* __restrict__ q,
                                                      int32_t* __restrict__ status) {
  const i64 t = (i64)blockIdx.x * kBlock + threadIdx.x;
  if (t >= F) return;
  const i64 a = (i64)faces[3 * t], b = (i64)faces[3 * t + 1], c = (i64)faces[3 * t + 2];
  i64 out = 0;
  int bits = 0;
  if (a < 0 || a >= V || b < 0 || b >= V || c < 0 || c >= V) {
    bits = PINGS_MESH_SAMPLE_INDEX;
  } else {
    const float v0[3] = {verts[3 * a], verts[3 * a + 1], verts[3 * a + 2]};
    const float v1[3] = {verts[3 * b], verts[3 * b + 1], verts[3 * b + 2]};
    const float v2[3] = {verts[3 * c], verts[3 * c + 1], verts[3 * c + 2]};
    if (!(finite3(v0) && finite3(v1) && finite3(v2))) {
      bits = PINGS_MESH_SAMPLE_NONFINITE;
    } else {
      bool keep = true;
      if (box) {
        const double bx[6] = {box[0], box[1], box[2], box[3], box[4], box[5]};
        keep = in_box(v0, bx) && in_box(v1, bx) && in_box(v2, bx);
      }
      if (keep) {
        const double e1x = (double)v1[0] - (double)v0[0], e1y = (double)v1[1] - (double)v0[1],
                     e1z = (double)v1[2] - (double)v0[2];
        const double e2x = (double)v2[0] - (double)v0[0], e2y = (double)v2[1] - (double)v0[1],
                     e2z = (double)v2[2] - (double)v0[2];
        const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
        const double scaled = 0.5 * __dsqrt_rn((cx * cx + cy * cy) + cz * cz) * kUnit;
        if (scaled <= (double)cap) out = llrint(scaled);      // cap <= 2^62: the conversion is in range
        else bits = PINGS_MESH_SAMPLE_AREA_CAP;                // also an area that overflowed to +inf
      }
    }
  }
  q[t] = (int64_t)out;
  if (bits) atomicOr(status, bits);
}

// the number of points owned by triangles 0..t
__device__ __forceinline__ i64 bound_of(i64 Qt, double n, double total) { return llrint((double)Qt * n / total); }

// the first t in [lo, hi] with bound_of(Q[t]) > i, given that hi qualifies
__device__ __forceinline__ i64 owner_of(const int64_t* __restrict__ Q, i64 lo, i64 hi, i64 i, double n, double total) {
  while (lo < hi) {
    const i64 mid = lo + ((hi - lo) >> 1);
    if (bound_of((i64)Q[mid], n, total) > i) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(kBlock) void sample_kernel(const float* __restrict__ verts,
                                                        const int64_t* __restrict__ faces, i64 F,
                                                        const int64_t* __restrict__ Q, i64 N, u64 seed,
                                                        float* __restrict__ points, int32_t* __restrict__ tri,
                                                        int64_t* __restrict__ count) {
  const i64 i = (i64)blockIdx.x * kBlock + threadIdx.x;
  const i64 Qall = (i64)Q[F - 1];
  if (i == 0) *count = Qall > 0 ? (int64_t)N : 0;
  if (i >= N || Qall <= 0) return;
  const double n = (double)N, total = (double)Qall;
  // first t with bound_of(Q[t]) > i; bound_of(Q[F - 1]) = N > i, so hi = F - 1 always qualifies
  const i64 lo = owner_of(Q, 0, F - 1, i, n, total);
  // bound_of(Q[lo]) > bound_of(Q[lo - 1]) means q[lo] > 0: the area kernel found its three corners inside [0, V)
  const i64 a = (i64)faces[3 * lo], b = (i64)faces[3 * lo + 1], c = (i64)faces[3 * lo + 2];
  u64 z = seed + (u64)(i + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const double u1 = (double)(uint32_t)(z >> 32) * kInvU32, u2 = (double)(uint32_t)(z & 0xffffffffull) * kInvU32;
  const double s = __dsqrt_rn(u1);
  const double wa = 1.0 - s, wb = s * (1.0 - u2), wc = s * u2;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double p = (wa * (double)verts[3 * a + k] + wb * (double)verts[3 * b + k]) + wc * (double)verts[3 * c + k];
    points[3 * i + k] = (float)p;
  }
  if (tri) tri[i] = (int32_t)lo;
}

struct SampleScratch {
  int64_t *q, *Q;
  void* temp;
  size_t temp_bytes, total;
};

SampleScratch carve_sample(void* base, i64 F) {
  pings::Carver c(base);
  SampleScratch s{};
  s.q = c.take<int64_t>((size_t)F);
  s.Q = c.take<int64_t>((size_t)F);
  s.temp_bytes = pings::align_up(devprim::inclusive_sum_i64_temp_bytes(F));
  s.temp = c.take<char>(s.temp_bytes);
  s.total = c.total();
  return s;
}

bool count_ok(int64_t n) { return n > 0 && n <= kMaxCount; }

}  // namespace

PINGS_API size_t pings_mesh_sample_scratch_bytes(int64_t F) { return count_ok(F) ? carve_sample(nullptr, F).total : 0; }

PINGS_API int pings_mesh_sample(const float* verts, int64_t V, const int64_t* faces, int64_t F, const double* box,
                                int64_t N, int64_t seed, void* scratch, float* points, int32_t* tri, int64_t* count,
                                int32_t* status, void* stream) {
  PINGS_ARG_CHECK(verts && faces && scratch && points && count && status, "null pointer");
  PINGS_ARG_CHECK(count_ok(V) && count_ok(F), "empty or oversized mesh");
  PINGS_ARG_CHECK(count_ok(N), "empty or oversized sample");
  hipStream_t st = pings::as_stream(stream);
  const SampleScratch s = carve_sample(scratch, F);
  pings::prof::Scope sc("mesh_sample", st);
  area_kernel<<<blocks_for(F), kBlock, 0, st>>>(verts, V, faces, F, box, area_cap(F), s.q, status);
  PINGS_LAUNCH_CHECK();
  if (int e = devprim::inclusive_sum_i64(s.temp, s.temp_bytes, s.q, s.Q, F, st)) return e;
  sample_kernel<<<blocks_for(N), kBlock, 0, st>>>(verts, faces, F, s.Q, N, (u64)seed, points, tri, count);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}
