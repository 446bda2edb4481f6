// Fused AdamW: one optimiser step of every tensor of every parameter group in one launch.
//
// The job table travels by value in the kernel arguments (no H2D copy, no allocation).  Work items are
// (tensor, chunk of PINGS_ADAMW_CHUNK elements); a workgroup finds the tensor of an item by a binary search over the
// inclusive prefix of chunk counts, which depends on blockIdx only and therefore runs on the scalar unit.  The grid is
// capped and strides over the items, so a 160 M-element feature table and a 1-element exposure scalar share a launch.
// 28 bytes move per element: p, g, m, v read, p, m, v written.
#include "common.hpp"

namespace {
using i64 = long long;

constexpr int kMaxJobs = PINGS_ADAMW_MAX_JOBS;
constexpr int kChunk = PINGS_ADAMW_CHUNK;
constexpr int kThreads = 256;
constexpr int kMaxGrid = 2048;      // 256 CUs x 8 workgroups: enough to saturate HBM, the rest is strided
static_assert(kChunk % (kThreads * 4) == 0, "a chunk is a whole number of 16-byte passes of the workgroup");

struct AdamwJobs {
  pings_adamw_job job[kMaxJobs];
  i64 end[kMaxJobs];                // inclusive prefix of chunk counts: items [end[t-1], end[t]) belong to tensor t
  int njobs;
};
// The 4 KB limit is HIP's on the EXPLICIT arguments; the compiler appends 256 bytes of hidden arguments behind them
// (the kernarg segment of this kernel is 4,104 bytes), which do not count against it.
static_assert(sizeof(AdamwJobs) <= 4096, "the job table must fit the 4 KB limit on explicit kernel arguments");

// torch's `_single_tensor_adam` with decoupled weight decay, operation by operation (-ffp-contract=off keeps the
// products and sums apart; `/` and sqrtf are the IEEE ones)
__device__ __forceinline__ void adamw_element(float& p, float g, float& m, float& v, const pings_adamw_job& j) {
  p = p * j.decay;
  m = m + (g - m) * j.one_minus_beta1;
  v = v * j.beta2 + (j.one_minus_beta2 * g) * g;
  const float denom = sqrtf(v) / j.bc2_sqrt + j.eps;
  p = p - (j.step_size * m) / denom;
}

__global__ __launch_bounds__(kThreads) void adamw_kernel(const AdamwJobs J) {
  const i64 items = J.end[J.njobs - 1];
  for (i64 item = blockIdx.x; item < items; item += gridDim.x) {
    int lo = 0, hi = J.njobs - 1;   // first tensor whose end exceeds the item
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (J.end[mid] > item) hi = mid; else lo = mid + 1;
    }
    const pings_adamw_job& j = J.job[lo];
    const i64 base = (item - (lo ? J.end[lo - 1] : 0)) * kChunk;
    const i64 left = j.n - base;
    const int len = left < kChunk ? (int)left : kChunk;
    float* __restrict__ p = j.p + base;
    const float* __restrict__ g = j.g + base;
    float* __restrict__ m = j.m + base;
    float* __restrict__ v = j.v + base;
    // chunk bases are multiples of 16 bytes, so the tensor's alignment is the chunk's
    const bool vec = ((reinterpret_cast<uintptr_t>(j.p) | reinterpret_cast<uintptr_t>(j.g) |
                       reinterpret_cast<uintptr_t>(j.m) | reinterpret_cast<uintptr_t>(j.v)) & 15) == 0;
    int done = 0;
    if (vec) {
      const int nvec = len >> 2;
#pragma unroll 2
      for (int q = threadIdx.x; q < nvec; q += kThreads) {
        float4 P = reinterpret_cast<float4*>(p)[q];
        const float4 G = reinterpret_cast<const float4*>(g)[q];
        float4 M = reinterpret_cast<float4*>(m)[q];
        float4 V = reinterpret_cast<float4*>(v)[q];
        adamw_element(P.x, G.x, M.x, V.x, j);
        adamw_element(P.y, G.y, M.y, V.y, j);
        adamw_element(P.z, G.z, M.z, V.z, j);
        adamw_element(P.w, G.w, M.w, V.w, j);
        reinterpret_cast<float4*>(p)[q] = P;
        reinterpret_cast<float4*>(m)[q] = M;
        reinterpret_cast<float4*>(v)[q] = V;
      }
      done = nvec << 2;
    }
    for (int e = done + threadIdx.x; e < len; e += kThreads) {   // a misaligned tensor, or the tail of the last chunk
      float P = p[e], M = m[e], V = v[e];
      adamw_element(P, g[e], M, V, j);
      p[e] = P;
      m[e] = M;
      v[e] = V;
    }
  }
}
}  // namespace

PINGS_API int pings_adamw_step(const pings_adamw_job* jobs, int njobs, int* launches_out, void* stream) {
  if (launches_out) *launches_out = 0;
  PINGS_ARG_CHECK(njobs >= 0, "negative job count");
  PINGS_ARG_CHECK(njobs == 0 || jobs, "null job table");
  for (int t = 0; t < njobs; ++t) {
    PINGS_ARG_CHECK(jobs[t].n >= 0, "negative size in job");
    PINGS_ARG_CHECK(jobs[t].n == 0 || (jobs[t].p && jobs[t].g && jobs[t].m && jobs[t].v), "null pointer in job");
    PINGS_ARG_CHECK(((reinterpret_cast<uintptr_t>(jobs[t].p) | reinterpret_cast<uintptr_t>(jobs[t].g) |
                      reinterpret_cast<uintptr_t>(jobs[t].m) | reinterpret_cast<uintptr_t>(jobs[t].v)) & 3) == 0,
                    "fp32 tensors are 4-byte aligned");
  }
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope scope("adamw_step", st);
  int launches = 0;
  for (int first = 0; first < njobs; first += kMaxJobs) {
    AdamwJobs J{};
    J.njobs = njobs - first < kMaxJobs ? njobs - first : kMaxJobs;
    i64 items = 0;
    for (int t = 0; t < J.njobs; ++t) {
      J.job[t] = jobs[first + t];
      items += pings::ceil_div<i64>(J.job[t].n, kChunk);
      J.end[t] = items;
    }
    if (items == 0) continue;
    const unsigned grid = (unsigned)(items < kMaxGrid ? items : kMaxGrid);
    if (int e = pings::launch(adamw_kernel, dim3(grid), kThreads, 0, st, J)) return e;
    ++launches;
  }
  if (launches_out) *launches_out = launches;
  return PINGS_OK;
}
