// SDF-sample loss block of the mapper (utils/mapper.py:836-930, 1493-1544) without host waits: BCE over the batch,
// the Eikonal term over every d-th sample of the free-space band, the colour L1 over the near-surface rows with a
// colour label.  The reference selects both subsets with boolean indexing (a nonzero each, so a host wait each); here
// the subset sizes stay on the device and every launch size depends on B and d only.
//
//   sl_select_kernel    one workgroup: Eikonal mask, stable rank of each masked row (wave ballots, then the wave
//                       counts in order), rows of rank % d == 0 compacted into idx / xsel in row order; rows
//                       ceil(M/d)..cap are padding (idx -1, the query coord[0]) so that the central differences
//                       behind it run at the fixed capacity cap = ceil(B/d)
//   (the caller runs the fused central-difference gradient on the cap rows)
//   sl_reduce_kernel    multi-block: IDW sums, sdf_pred, BCE with logits, colour sigmoid + IDW + L1 on the masked
//                       rows, (|g|-1)^2 on the live Eikonal rows; fp64 per-block sums in a fixed tree order
//   sl_final_kernel     one workgroup: the per-block sums in block order, the means (0/0 = NaN for an empty subset,
//                       as torch's mean of an empty tensor), the counts
//   sl_backward_kernel  one thread per row: d sdf per neighbour, d colour decoder output, d g (zero on padding)
// No float atomics: bitwise reproducible.
#include <algorithm>
#include <cmath>
#include "common.hpp"

namespace {

constexpr int SEL_THREADS = 1024, RED_THREADS = 256, MAX_BLOCKS = 256, MAX_K = 16, MAX_C = 8;
constexpr int F_EIK = 1, F_COL = 2, F_COL_W = 4, F_BCE_W = 8, F_WF = 16;

__device__ inline float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

__host__ __device__ inline int n_blocks(long long B, long long cap) {
  const long long rows = B > cap ? B : cap;
  long long nb = (rows + RED_THREADS - 1) / RED_THREADS;
  return (int)(nb < 1 ? 1 : (nb > MAX_BLOCKS ? MAX_BLOCKS : nb));
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

__global__ __launch_bounds__(SEL_THREADS) void sl_select_kernel(pings_sdf_loss_args a) {
  __shared__ uint32_t wcount[SEL_THREADS / 64];
  __shared__ long long sBase;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long long B = a.B, cap = a.cap, d = a.d;
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  if (t == 0) sBase = 0;
  __syncthreads();
  for (long long c0 = 0; c0 < B; c0 += SEL_THREADS) {
    const long long i = c0 + t;
    const bool m = i < B && fabsf(a.label[i]) < a.eik_band;
    const unsigned long long bal = __ballot(m);
    if (lane == 0) wcount[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    long long r = sBase;
    for (int w = 0; w < wave; ++w) r += wcount[w];
    r += __popcll(bal & below);
    if (m && r % d == 0) {
      const long long j = r / d;      // j < ceil(B/d) = cap
      a.idx[j] = (int32_t)i;
      a.xsel[3 * j + 0] = a.coord[3 * i + 0];
      a.xsel[3 * j + 1] = a.coord[3 * i + 1];
      a.xsel[3 * j + 2] = a.coord[3 * i + 2];
    }
    __syncthreads();
    if (t == 0) {
      long long s = 0;
      for (int w = 0; w < SEL_THREADS / 64; ++w) s += wcount[w];
      sBase += s;
    }
    __syncthreads();
  }
  const long long M = sBase, live = (M + d - 1) / d;
  const float x0 = a.coord[0], y0 = a.coord[1], z0 = a.coord[2];
  for (long long j = live + t; j < cap; j += SEL_THREADS) {
    a.idx[j] = -1;
    a.xsel[3 * j + 0] = x0;
    a.xsel[3 * j + 1] = y0;
    a.xsel[3 * j + 2] = z0;
  }
  if (t == 0) a.meta[0] = (int32_t)live;
}

__device__ inline bool color_row(const pings_sdf_loss_args& a, long long b) {
  return fabsf(a.label[b]) < a.col_band && a.color_label[(long long)a.C * b] >= 0.f;
}

// colour prediction of row b, channel c: sum_k w sigmoid(c) (or sigmoid(c) for weighted_first)
__device__ inline float color_pred(const pings_sdf_loss_args& a, long long b, int c) {
  const int K = a.k, C = a.C;
  if (a.flags & F_WF) return sigmoidf_(a.c[(long long)C * b + c]);
  float p = 0.f;
  for (int j = 0; j < K; ++j) p += sigmoidf_(a.c[((long long)K * b + j) * C + c]) * a.w[(long long)K * b + j];
  return p;
}

__device__ inline float row_pred(const pings_sdf_loss_args& a, long long b) {
  if (a.flags & F_WF) return a.s[b];
  const int K = a.k;
  float p = 0.f;
  for (int j = 0; j < K; ++j) p += a.s[(long long)K * b + j] * a.w[(long long)K * b + j];
  return p;
}

__global__ __launch_bounds__(RED_THREADS) void sl_reduce_kernel(pings_sdf_loss_args a) {
  __shared__ double sh[4 * RED_THREADS];
  const long long B = a.B, cap = a.cap;
  const int NB = gridDim.x;
  const long long cb = (B + NB - 1) / NB, ce = (cap + NB - 1) / NB;
  double v[4] = {0.0, 0.0, 0.0, 0.0};   // BCE sum, Eikonal sum, colour sum, colour rows
  const long long b0 = blockIdx.x * cb, b1 = b0 + cb < B ? b0 + cb : B;
  const float inv_sigma = 1.f / a.sigma;
  for (long long b = b0 + threadIdx.x; b < b1; b += RED_THREADS) {
    const float pred = row_pred(a, b);
    a.sdf_pred[b] = pred;
    // BCEWithLogits(pred / sigma, sigmoid(label / sigma)) in torch's stable form
    const float x = pred * inv_sigma, y = sigmoidf_(a.label[b] * inv_sigma);
    const float mx = fmaxf(-x, 0.f);
    float l = (1.f - y) * x + mx + logf(expf(-mx) + expf(-x - mx));
    if (a.flags & F_BCE_W) l *= fabsf(a.weight[b]);
    v[0] += (double)l;
    if ((a.flags & F_COL) && color_row(a, b)) {
      const float wt = (a.flags & F_COL_W) ? fabsf(a.weight[b]) : 1.f;
      for (int c = 0; c < a.C; ++c)
        v[2] += (double)(wt * fabsf(color_pred(a, b, c) - a.color_label[(long long)a.C * b + c]));
      v[3] += 1.0;
    }
  }
  if (a.flags & F_EIK) {
    const long long live = a.meta[0];
    const long long e0 = blockIdx.x * ce, e1 = e0 + ce < live ? e0 + ce : live;
    for (long long j = e0 + threadIdx.x; j < e1; j += RED_THREADS) {
      const float gx = a.g[3 * j], gy = a.g[3 * j + 1], gz = a.g[3 * j + 2];
      const float r = sqrtf(gx * gx + gy * gy + gz * gz) - 1.f;
      v[1] += (double)(r * r);
    }
  }
  block_sum<4>(v, sh);
  if (threadIdx.x == 0)
    for (int q = 0; q < 4; ++q) a.part[4 * blockIdx.x + q] = v[q];
}

__global__ __launch_bounds__(64) void sl_final_kernel(pings_sdf_loss_args a, int NB) {
  if (threadIdx.x != 0) return;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = 0; b < NB; ++b)
    for (int q = 0; q < 4; ++q) s[q] += a.part[4 * b + q];
  const long long live = (a.flags & F_EIK) ? a.meta[0] : 0;
  const long long ncol = (long long)s[3];
  a.losses[0] = (float)(s[0] / (double)a.B);
  a.losses[1] = (a.flags & F_EIK) ? (float)(s[1] / (double)live) : 0.f;                 // 0/0: NaN, as torch
  a.losses[2] = (a.flags & F_COL) ? (float)(s[2] / (double)(ncol * a.C)) : 0.f;
  a.counts[0] = (double)live;
  a.counts[1] = (double)ncol;
  a.meta[1] = (int32_t)ncol;
}

__global__ __launch_bounds__(RED_THREADS) void sl_backward_kernel(pings_sdf_loss_args a) {
  const long long r = (long long)blockIdx.x * RED_THREADS + threadIdx.x;
  const int K = a.k, C = a.C;
  const bool wf = (a.flags & F_WF) != 0;
  if (r < a.B) {
    const long long b = r;
    const float inv_sigma = 1.f / a.sigma;
    const float x = row_pred(a, b) * inv_sigma, y = sigmoidf_(a.label[b] * inv_sigma);
    float wt = (a.flags & F_BCE_W) ? fabsf(a.weight[b]) : 1.f;
    float dp = a.gl[0] * wt * (sigmoidf_(x) - y) / (float)a.B * inv_sigma;
    if (a.g_pred) dp += a.g_pred[b];
    if (wf) a.d_s[b] = dp;
    else
      for (int j = 0; j < K; ++j) a.d_s[(long long)K * b + j] = dp * a.w[(long long)K * b + j];
    if (a.flags & F_COL) {
      const int rows = wf ? 1 : K;
      float* dc = a.d_c + (long long)rows * C * b;
      if (color_row(a, b)) {
        const float wc = (a.flags & F_COL_W) ? fabsf(a.weight[b]) : 1.f;
        const float scale = a.gl[2] * wc / (float)((long long)a.meta[1] * C);
        for (int c = 0; c < C; ++c) {
          const float diff = color_pred(a, b, c) - a.color_label[(long long)C * b + c];
          const float dpc = scale * (float)((diff > 0.f) - (diff < 0.f));
          if (wf) {
            const float sg = sigmoidf_(a.c[(long long)C * b + c]);
            dc[c] = dpc * (1.f - sg) * sg;
          } else {
            for (int j = 0; j < K; ++j) {
              const float sg = sigmoidf_(a.c[((long long)K * b + j) * C + c]);
              dc[j * C + c] = dpc * a.w[(long long)K * b + j] * (1.f - sg) * sg;
            }
          }
        }
      } else {
        for (int q = 0; q < rows * C; ++q) dc[q] = 0.f;
      }
    }
  }
  if ((a.flags & F_EIK) && r < a.cap) {
    const long long j = r, live = a.meta[0];
    float gx = 0.f, gy = 0.f, gz = 0.f;
    if (j < live) {
      gx = a.g[3 * j]; gy = a.g[3 * j + 1]; gz = a.g[3 * j + 2];
      const float n = sqrtf(gx * gx + gy * gy + gz * gz);
      // d mean((|g|-1)^2) / dg = 2 (|g|-1) g / |g| / live; torch's norm backward is 0 at |g| = 0
      const float coef = n > 0.f ? a.gl[1] * 2.f * (n - 1.f) / (float)live / n : 0.f;
      gx *= coef; gy *= coef; gz *= coef;
    }
    a.d_g[3 * j] = gx; a.d_g[3 * j + 1] = gy; a.d_g[3 * j + 2] = gz;
  }
}

int check_args(const pings_sdf_loss_args* a) {
  PINGS_ARG_CHECK(a != nullptr, "null args");
  PINGS_ARG_CHECK(a->B > 0 && a->B < (1ll << 31), "B must be in 1..2^31-1");
  PINGS_ARG_CHECK(a->d >= 1 && a->cap == (a->B + a->d - 1) / a->d, "cap must be ceil(B/d)");
  PINGS_ARG_CHECK(a->k >= 1 && a->k <= MAX_K, "k must be in 1..16");
  PINGS_ARG_CHECK(!(a->flags & F_COL) || (a->C >= 1 && a->C <= MAX_C && a->color_label), "colour inputs");
  PINGS_ARG_CHECK(!(a->flags & (F_COL_W | F_BCE_W)) || a->weight, "null weight");
  PINGS_ARG_CHECK(a->label && a->meta && a->sigma > 0.f, "null label / meta or sigma <= 0");
  return PINGS_OK;
}

}  // namespace

PINGS_API int pings_sdf_loss_partials(int64_t B, int64_t cap) { return n_blocks(B, cap); }

PINGS_API int pings_sdf_loss_select(const pings_sdf_loss_args* a, void* stream) {
  if (int e = check_args(a)) return e;
  PINGS_ARG_CHECK(a->coord && a->idx && a->xsel, "null select buffers");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("sdf_loss_select", st);
  hipLaunchKernelGGL(sl_select_kernel, dim3(1), dim3(SEL_THREADS), 0, st, *a);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API int pings_sdf_loss_reduce(const pings_sdf_loss_args* a, void* stream) {
  if (int e = check_args(a)) return e;
  PINGS_ARG_CHECK(a->s && (a->flags & F_WF || a->w) && a->part && a->sdf_pred && a->losses && a->counts,
                  "null reduce buffers");
  PINGS_ARG_CHECK(!(a->flags & F_COL) || a->c, "null colour decoder output");
  PINGS_ARG_CHECK(!(a->flags & F_EIK) || a->g, "null Eikonal gradient");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("sdf_loss_reduce", st);
  const int NB = n_blocks(a->B, a->cap);
  hipLaunchKernelGGL(sl_reduce_kernel, dim3(NB), dim3(RED_THREADS), 0, st, *a);
  PINGS_LAUNCH_CHECK();
  hipLaunchKernelGGL(sl_final_kernel, dim3(1), dim3(64), 0, st, *a, NB);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API int pings_sdf_loss_backward(const pings_sdf_loss_args* a, void* stream) {
  if (int e = check_args(a)) return e;
  PINGS_ARG_CHECK(a->gl && a->s && a->d_s && (a->flags & F_WF || a->w), "null backward buffers");
  PINGS_ARG_CHECK(!(a->flags & F_COL) || (a->c && a->d_c), "null colour buffers");
  PINGS_ARG_CHECK(!(a->flags & F_EIK) || (a->g && a->d_g), "null Eikonal gradient");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("sdf_loss_backward", st);
  const long long rows = std::max<long long>(a->B, (a->flags & F_EIK) ? a->cap : 0);
  hipLaunchKernelGGL(sl_backward_kernel, dim3((unsigned)((rows + RED_THREADS - 1) / RED_THREADS)), dim3(RED_THREADS),
                     0, st, *a);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}
