// Semantic loss block of the mapper (utils/mapper.py:863-866, 929-946) without host waits: log-softmax of the semantic
// decoder's output per (row, neighbour), the IDW sum over the neighbours, and NLLLoss(mean) over every d-th labelled
// row.  The reference selects the labelled rows with two boolean-index selections (a nonzero each, so a host wait
// each); here the selection stays on the device and every launch size depends on B, k, S and d only.
//
//   sem_select_kernel    (d > 1 only) one workgroup: label mask, stable rank of each masked row (wave ballots, then the
//                        wave counts in order), selected[b] = masked and rank % d == 0
//   sem_reduce_kernel    multi-block, a group of G = pow2 >= S lanes per (row, neighbour) vector, lanes on consecutive
//                        floats of raw: max and sum by cross-lane reduction, w * log_softmax[y] into fp64 per-block sums
//                        in a fixed tree order; with d == 1 it takes the mask itself and writes selected[]
//   sem_final_kernel     one workgroup: the per-block sums in block order, nll = -sum / n (0/0 = NaN for an empty
//                        selection, as torch's NLLLoss(mean)), the counts, n kept in the scratch for the backward
//   sem_backward_kernel  the same lane mapping: d raw = g / n * w * (softmax - onehot) on selected rows, 0.0 elsewhere
// A label >= S never indexes memory: the row is unlabelled and counted.  No float atomics: bitwise reproducible.
#include <cmath>
#include "common.hpp"

namespace {

constexpr int SEL_THREADS = 1024, RED_THREADS = 256, MAX_BLOCKS = 256, MAX_K = 16, MAX_S = 32;
constexpr int F_WF = 1, F_FREESPACE = 2, F_LABEL_I64 = 4;
constexpr int PART = 3;                      // doubles per block: sum of w * logp[y], selected rows, labels >= S

__host__ __device__ inline int group_lanes(int S) {
  int g = 1;
  while (g < S) g <<= 1;
  return g;
}

__host__ __device__ inline long long n_vectors(const pings_sem_loss_args& a) {
  return (a.flags & F_WF) ? a.B : a.B * (long long)a.k;
}

inline int n_blocks(const pings_sem_loss_args& a) {
  const long long per_block = RED_THREADS / group_lanes(a.S);
  const long long nb = (n_vectors(a) + per_block - 1) / per_block;
  return (int)(nb < 1 ? 1 : (nb > MAX_BLOCKS ? MAX_BLOCKS : nb));
}

__device__ inline long long label_of(const pings_sem_loss_args& a, long long b) {
  return (a.flags & F_LABEL_I64) ? static_cast<const int64_t*>(a.label)[b]
                                 : (long long)static_cast<const int32_t*>(a.label)[b];
}

// labelled, by the reference's mask; a label >= S counts as unlabelled (the reference's NLLLoss asserts there)
__device__ inline bool labelled(const pings_sem_loss_args& a, long long y) {
  return ((a.flags & F_FREESPACE) ? y >= 0 : y > 0) && y < a.S;
}

__device__ inline double* scratch_part(const pings_sem_loss_args& a) { return static_cast<double*>(a.scratch); }
__device__ inline double* scratch_n(const pings_sem_loss_args& a) {
  return static_cast<double*>(a.scratch) + PART * MAX_BLOCKS;
}

__global__ __launch_bounds__(SEL_THREADS) void sem_select_kernel(pings_sem_loss_args a) {
  __shared__ uint32_t wcount[SEL_THREADS / 64];
  __shared__ long long sBase;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long long B = a.B, d = a.d;
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  if (t == 0) sBase = 0;
  __syncthreads();
  for (long long c0 = 0; c0 < B; c0 += SEL_THREADS) {
    const long long i = c0 + t;
    const bool m = i < B && labelled(a, label_of(a, i));
    const unsigned long long bal = __ballot(m);
    if (lane == 0) wcount[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    long long r = sBase;
    for (int w = 0; w < wave; ++w) r += wcount[w];
    r += __popcll(bal & below);
    if (i < B) a.selected[i] = (m && r % d == 0) ? 1 : 0;
    __syncthreads();
    if (t == 0) {
      long long s = 0;
      for (int w = 0; w < SEL_THREADS / 64; ++w) s += wcount[w];
      sBase += s;
    }
    __syncthreads();
  }
}

// What every lane of a vector's group holds: the logit of its class (idle lanes of the group: -inf), the row, and
// whether the row is selected.  A vector that is not selected, or lies past the end, reads nothing and holds zeros.
struct Vec {
  long long b, y;
  int j, c;          // neighbour, class of this lane (c >= S: idle)
  bool live, sel;    // inside the batch; row selected
  float x, w;
};

template <bool D1>
__device__ inline Vec load_vec(const pings_sem_loss_args& a, long long v, int c) {
  Vec r;
  const int K = (a.flags & F_WF) ? 1 : a.k;
  r.live = v < n_vectors(a);
  r.b = r.live ? v / K : 0;
  r.j = (int)(v - r.b * K);
  r.c = c;
  r.y = r.live ? label_of(a, r.b) : -1;
  r.sel = r.live && (D1 ? labelled(a, r.y) : a.selected[r.b] != 0);
  r.x = c < a.S ? 0.f : -INFINITY;
  r.w = 1.f;
  if (r.sel) {
    if (c < a.S) r.x = a.raw[v * a.S + c];
    if (!(a.flags & F_WF)) r.w = a.w[v];
  }
  return r;
}

// max and sum of exp(x - max) over the G lanes of the group (G a power of two <= 32: the xor partners stay inside it)
__device__ inline void group_softmax(float x, int G, float& mx, float& e, float& sum) {
  mx = x;
  for (int off = G >> 1; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  e = expf(x - mx);            // idle lanes: exp(-inf) = 0
  sum = e;
  for (int off = G >> 1; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
}

template <int N>
__device__ inline void block_sum(double (&v)[N], double* sh) {   // sh: [N][blockDim.x]; result in v of thread 0
  const int t = threadIdx.x, n = blockDim.x;
#pragma unroll
  for (int k = 0; k < N; ++k) sh[k * n + t] = v[k];
  __syncthreads();
  for (int s = n / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int k = 0; k < N; ++k) sh[k * n + t] += sh[k * n + t + s];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = sh[k * n];
  __syncthreads();
}

template <bool D1>
__global__ __launch_bounds__(RED_THREADS) void sem_reduce_kernel(pings_sem_loss_args a) {
  __shared__ double sh[PART * RED_THREADS];
  const int G = group_lanes(a.S), per_block = RED_THREADS / G;
  const int c = threadIdx.x & (G - 1), slot = threadIdx.x / G;
  const long long NV = n_vectors(a);
  const long long chunk = ((NV + gridDim.x - 1) / gridDim.x + per_block - 1) / per_block * per_block;
  const long long v0 = blockIdx.x * chunk, v1 = v0 + chunk < NV ? v0 + chunk : NV;
  double acc[PART] = {0.0, 0.0, 0.0};
  for (long long base = v0; base < v1; base += per_block) {     // block-uniform trip count: every lane shuffles
    const Vec r = load_vec<D1>(a, base + slot, c);
    float mx, e, sum;
    group_softmax(r.x, G, mx, e, sum);
    // the logit of class y sits in lane y of the group; an unselected vector reads its own lane
    const int src = (threadIdx.x & 63 & ~(G - 1)) + (r.sel ? (int)r.y : 0);
    const float xy = __shfl(r.x, src, 64);
    if (c == 0 && r.live) {
      if (r.sel) acc[0] += (double)(r.w * (xy - mx - logf(sum)));
      if (r.j == 0) {
        if (D1) a.selected[r.b] = r.sel ? 1 : 0;
        acc[1] += r.sel ? 1.0 : 0.0;
        acc[2] += r.y >= a.S ? 1.0 : 0.0;
      }
    }
  }
  block_sum<PART>(acc, sh);
  if (threadIdx.x == 0)
    for (int q = 0; q < PART; ++q) scratch_part(a)[PART * blockIdx.x + q] = acc[q];
}

__global__ __launch_bounds__(64) void sem_final_kernel(pings_sem_loss_args a, int NB) {
  if (threadIdx.x != 0) return;
  double s[PART] = {0.0, 0.0, 0.0};
  for (int b = 0; b < NB; ++b)
    for (int q = 0; q < PART; ++q) s[q] += scratch_part(a)[PART * b + q];
  a.loss[0] = (float)(-s[0] / s[1]);         // 0/0: NaN, as torch's NLLLoss(mean) of an empty input
  a.counts[0] = s[1];
  a.counts[1] = s[2];
  scratch_n(a)[0] = s[1];
}

__global__ __launch_bounds__(RED_THREADS) void sem_backward_kernel(pings_sem_loss_args a) {
  const int G = group_lanes(a.S), per_block = RED_THREADS / G;
  const int c = threadIdx.x & (G - 1), slot = threadIdx.x / G;
  const long long NV = n_vectors(a);
  const float scale = a.gl[0] / (float)scratch_n(a)[0];        // no row is selected when n = 0: never used there
  for (long long base = (long long)blockIdx.x * per_block; base < NV; base += (long long)gridDim.x * per_block) {
    const Vec r = load_vec<false>(a, base + slot, c);
    float mx, e, sum;
    group_softmax(r.x, G, mx, e, sum);
    if (r.live && c < a.S) {
      float g = 0.f;
      if (r.sel) g = scale * r.w * (e / sum - (c == r.y ? 1.f : 0.f));
      a.d_raw[(base + slot) * a.S + c] = g;
    }
  }
}

int check_args(const pings_sem_loss_args* a) {
  PINGS_ARG_CHECK(a != nullptr, "null args");
  PINGS_ARG_CHECK(a->B > 0 && a->B < (1ll << 31), "B must be in 1..2^31-1");
  PINGS_ARG_CHECK(a->k >= 1 && a->k <= MAX_K, "k must be in 1..16");
  PINGS_ARG_CHECK(a->S >= 1 && a->S <= MAX_S, "S must be in 1..32");
  PINGS_ARG_CHECK(a->d >= 1, "d must be >= 1");
  PINGS_ARG_CHECK(!(a->flags & F_WF) || a->k == 1, "weighted_first has k = 1");
  PINGS_ARG_CHECK(a->raw && a->label && a->selected && a->scratch, "null raw / label / selected / scratch");
  PINGS_ARG_CHECK((a->flags & F_WF) || a->w, "null weights");
  return PINGS_OK;
}

}  // namespace

PINGS_API size_t pings_sem_loss_scratch_bytes(int64_t B) {
  return B > 0 && B < (1ll << 31) ? sizeof(double) * (PART * MAX_BLOCKS + 1) : 0;
}

PINGS_API int pings_sem_loss_forward(const pings_sem_loss_args* a, void* stream) {
  if (int e = check_args(a)) return e;
  PINGS_ARG_CHECK(a->loss && a->counts, "null loss / counts");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("sem_loss_forward", st);
  const int NB = n_blocks(*a);
  if (a->d > 1) {
    if (int e = pings::launch(sem_select_kernel, dim3(1), SEL_THREADS, 0, st, *a)) return e;
    if (int e = pings::launch(sem_reduce_kernel<false>, dim3(NB), RED_THREADS, 0, st, *a)) return e;
  } else {
    if (int e = pings::launch(sem_reduce_kernel<true>, dim3(NB), RED_THREADS, 0, st, *a)) return e;
  }
  return pings::launch(sem_final_kernel, dim3(1), 64, 0, st, *a, NB);
}

PINGS_API int pings_sem_loss_backward(const pings_sem_loss_args* a, void* stream) {
  if (int e = check_args(a)) return e;
  PINGS_ARG_CHECK(a->gl && a->d_raw, "null backward buffers");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("sem_loss_backward", st);
  const long long per_block = RED_THREADS / group_lanes(a->S);
  const long long nb = (n_vectors(*a) + per_block - 1) / per_block;
  return pings::launch(sem_backward_kernel, dim3((unsigned)(nb > 2048 ? 2048 : nb)), RED_THREADS, 0, st, *a);
}
