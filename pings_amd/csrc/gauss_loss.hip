// Gaussian-space loss block of the joint mapping iteration (utils/mapper.py:1331-1483) without host waits:
//   opacity / opacity entropy over alpha_all, the constraint mask, a uniform sample of at most `cap` constrained
//   Gaussians, isotropy and area of the sampled scales, and the SDF / SDF-normal consistency and invalid-opacity terms
//   on the (1+R)*cap query rows.  Every count the reference reads back with .item() stays on the device.
//
//   gl_mask_kernel      multi-block: random 31-bit key of every constrained Gaussian (0xFFFFFFFF otherwise), the
//                       per-block constraint count and opacity / entropy partial sums (fp64, fixed tree order)
//   gl_select_kernel    one workgroup: fixed-order sum of the partials, S = min(count, cap) (0 when count <= 10),
//                       radix select of the S-th smallest key, then an ordered compaction: the S Gaussians with the
//                       smallest keys (ties broken by index), in ascending index order.  A uniform subset without
//                       replacement; the keys are a hash of (device seed, index), so a seed gives the same draw
//   gl_prepare_kernel   per sample row: normal = normalised third column of R(q), query rows (unshifted block first,
//                       then block k = xyz + n * shift), labels
//   pings_sdf_forward   (sdf_fwd) on the (1+R)*cap rows, dS/dx and the neighbour lists kept
//   gl_reduce_kernel    one workgroup: valid mask, the masked means, isotropy, area, invalid opacity, counts
//   backward:  gl_rows_bwd_kernel (d s, d dS/dx, d n per row) -> pings_sdf_backward + pings_sdf_double_backward (table,
//   decoder) and sdf_hvp_kernel (d x = dS/dx * d s + H_S(x) v per row) -> gl_scatter_bwd_kernel (the 1+R copies of a
//   sample summed in block order, normal -> quaternion, dense gradients; sampled rows are distinct, no atomics) and
//   gl_alpha_all_bwd_kernel.
// No float atomics; fixed summation orders: bitwise reproducible for a fixed seed.
#include <algorithm>
#include <cmath>
#include "common.hpp"
#include "knn_common.hpp"

namespace {
using namespace pings_knn;

constexpr int MASK_BLOCKS = 256, MASK_THREADS = 256, SEL_THREADS = 1024;
constexpr uint32_t NO_KEY = 0xFFFFFFFFu;
constexpr float IDW_EPS = 1e-15f;   // as sdf_bwd.hip / the forward weights

__device__ inline uint32_t key_of(unsigned long long seed, long long i) {
  // splitmix64 finaliser of (seed, index): 31 bits, so that NO_KEY sorts after every constrained Gaussian
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (uint32_t)(z >> 33);
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

__global__ __launch_bounds__(MASK_THREADS) void gl_mask_kernel(pings_gauss_loss_args a) {
  __shared__ double sh[4 * MASK_THREADS];
  const long long P = a.P, Na = a.Na;
  const long long cp = (P + MASK_BLOCKS - 1) / MASK_BLOCKS, ca = (Na + MASK_BLOCKS - 1) / MASK_BLOCKS;
  const unsigned long long seed = a.seed ? (unsigned long long)a.seed[0] : 0ull;
  double v[4] = {0.0, 0.0, 0.0, 0.0};   // constraint count, sum alpha (< min), count (< min), entropy sum
  const long long p0 = blockIdx.x * cp, p1 = p0 + cp < P ? p0 + cp : P;
  for (long long i = p0 + threadIdx.x; i < p1; i += MASK_THREADS) {
    bool c = a.visible[i] != 0 && a.alpha[i] > a.min_alpha;
    if (a.contrib) c = c && a.contrib[i] > a.contrib_thr;
    if (a.free_mask) c = c && a.free_mask[i] == 0;
    a.keys[i] = c ? key_of(seed, i) : NO_KEY;
    v[0] += c ? 1.0 : 0.0;
  }
  const long long q0 = blockIdx.x * ca, q1 = q0 + ca < Na ? q0 + ca : Na;
  for (long long i = q0 + threadIdx.x; i < q1; i += MASK_THREADS) {
    const float x = a.alpha_all[i];
    if (x < a.min_alpha) { v[1] += (double)x; v[2] += 1.0; }
    const float o = fminf(fmaxf(fabsf(x), 1e-6f), 1.f - 1e-6f);   // opacity_entropy_loss(|alpha|), loss_utils.py:166
    v[3] += (double)(-o * logf(o) - (1.f - o) * logf(1.f - o));
  }
  block_sum<4>(v, sh);
  if (threadIdx.x == 0)
    for (int k = 0; k < 4; ++k) a.part[blockIdx.x * 4 + k] = v[k];
}

__global__ __launch_bounds__(SEL_THREADS) void gl_select_kernel(pings_gauss_loss_args a) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t sPrefix, sWant;
  __shared__ uint32_t sW[2][SEL_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t == 0) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < MASK_BLOCKS; ++b)
      for (int k = 0; k < 4; ++k) s[k] += a.part[b * 4 + k];
    const long long count = (long long)s[0], nlt = (long long)s[2];
    long long S = a.n_inject >= 0 ? a.n_inject : (count < a.cap ? count : a.cap);
    if (count <= 10) S = 0;                                   // mapper.py:1379 gate
    a.meta[0] = (int32_t)count; a.meta[1] = (int32_t)S; a.meta[2] = (int32_t)nlt;
    a.losses[0] = (a.flags & 1) && nlt > 0 ? -(float)(s[1] / (double)nlt) : 0.f;
    a.losses[1] = (a.flags & 2) ? (float)(s[3] / (double)a.Na) : 0.f;   // NaN for an empty alpha_all, as torch
    a.counts[0] = (double)nlt; a.counts[1] = (double)count; a.counts[2] = (double)S;
    sWant = (uint32_t)S;
    sPrefix = 0u;
  }
  __syncthreads();
  const long long S = sWant;
  if (S == 0) return;
  if (a.n_inject >= 0) {
    for (long long r = t; r < S; r += SEL_THREADS) a.idx[r] = (int32_t)a.inject_idx[r];
    return;
  }
  // radix select, 8 bits per pass: prefix / want become the S-th smallest key and its rank among equal keys
  uint32_t himask = 0u;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (t < 256) hist[t] = 0u;
    __syncthreads();
    const uint32_t prefix = sPrefix;
    for (long long i = t; i < a.P; i += SEL_THREADS) {
      const uint32_t k = a.keys[i];
      if ((k & himask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);   // integer LDS counts
    }
    __syncthreads();
    if (t == 0) {
      uint32_t want = sWant, b = 0;
      for (; b < 255u && hist[b] < want; ++b) want -= hist[b];
      sWant = want;
      sPrefix = prefix | (b << shift);
    }
    himask |= 255u << shift;
    __syncthreads();
  }
  const uint32_t T = sPrefix, take_eq = sWant;
  // ordered compaction: every key < T, and the first take_eq keys == T in index order
  long long base_lt = 0, base_eq = 0;
  const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  for (long long c0 = 0; c0 < a.P; c0 += SEL_THREADS) {
    const long long i = c0 + t;
    const uint32_t k = i < a.P ? a.keys[i] : NO_KEY;
    const bool lt = k < T, eq = k == T;
    const unsigned long long blt = __ballot(lt), beq = __ballot(eq);
    if (lane == 0) { sW[0][wave] = (uint32_t)__popcll(blt); sW[1][wave] = (uint32_t)__popcll(beq); }
    __syncthreads();
    long long olt = base_lt + __popcll(blt & below), oeq = base_eq + __popcll(beq & below);
    long long tlt = 0, teq = 0;
    for (int w = 0; w < SEL_THREADS / 64; ++w) {
      if (w < wave) { olt += sW[0][w]; oeq += sW[1][w]; }
      tlt += sW[0][w]; teq += sW[1][w];
    }
    const long long pos = olt + (oeq < (long long)take_eq ? oeq : (long long)take_eq);
    if (lt || (eq && oeq < (long long)take_eq)) a.idx[pos] = (int32_t)i;
    base_lt += tlt; base_eq += teq;
    __syncthreads();
  }
}

// normal = normalize(R(q)[:, 2]) (general_utils.py:199-212, F.normalize eps 1e-12); also returns the raw column
__device__ inline void quat_normal(const float* q, float& nx, float& ny, float& nz, float& cx, float& cy, float& cz,
                                   float& len) {
  const float r = q[0], x = q[1], y = q[2], z = q[3];
  cx = 2.f * (x * z + r * y); cy = 2.f * (y * z - r * x); cz = 1.f - 2.f * (x * x + y * y);
  len = sqrtf(cx * cx + cy * cy + cz * cz);
  const float d = fmaxf(len, 1e-12f);
  nx = cx / d; ny = cy / d; nz = cz / d;
}

__global__ __launch_bounds__(256) void gl_prepare_kernel(pings_gauss_loss_args a) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.cap) return;
  const long long S = a.meta[1], cap = a.cap;
  float px = 0.f, py = 0.f, pz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
  if (r < S) {
    const long long i = a.idx[r];
    px = a.xyz[3 * i]; py = a.xyz[3 * i + 1]; pz = a.xyz[3 * i + 2];
    float cx, cy, cz, len;
    quat_normal(a.rot + 4 * i, nx, ny, nz, cx, cy, cz, len);
  }
  a.normal[3 * r] = nx; a.normal[3 * r + 1] = ny; a.normal[3 * r + 2] = nz;
  a.queries[3 * r] = px; a.queries[3 * r + 1] = py; a.queries[3 * r + 2] = pz;
  a.label[r] = 0.f;
  for (int k = 1; k <= a.R; ++k) {
    const long long j = k * cap + r;
    // (randn - 0.5) * 2 * range: the reference's shift, not centred on zero (mapper.py:1432)
    const float sh = r < S ? (a.randn[(k - 1) * cap + r] - 0.5f) * 2.0f * a.shift_range : 0.f;
    a.queries[3 * j] = px + nx * sh; a.queries[3 * j + 1] = py + ny * sh; a.queries[3 * j + 2] = pz + nz * sh;
    a.label[j] = sh;
  }
}

__global__ __launch_bounds__(SEL_THREADS) void gl_reduce_kernel(pings_gauss_loss_args a) {
  __shared__ double sh[6 * SEL_THREADS];
  const int t = threadIdx.x;
  const long long S = a.meta[1], cap = a.cap, rows = (1 + a.R) * cap;
  const int nc = a.ncols;
  const bool sdf_on = (a.flags & 16) != 0;
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // |s - label|, normal error, n valid, invalid alpha, n invalid, iso
  double ar = 0.0;
  if (sdf_on) {
    for (long long j = t; j < rows; j += SEL_THREADS) {
      const long long r = j % cap;
      const bool live = r < S;
      const float gx = a.grad[3 * j], gy = a.grad[3 * j + 1], gz = a.grad[3 * j + 2];
      const float gn = sqrtf(gx * gx + gy * gy + gz * gz);
      const bool valid = live && gn < a.grad_max && gn > a.grad_min && a.nn[j] >= 3;
      a.valid[j] = valid ? 1 : 0;
      if (valid) {
        v[0] += (double)fabsf(a.sdf[j] - a.label[j]);
        const float d = gn + 1e-7f;
        const float e = 1.f - ((gx / d) * a.normal[3 * r] + (gy / d) * a.normal[3 * r + 1] + (gz / d) * a.normal[3 * r + 2]);
        v[1] += (double)e;
        v[2] += 1.0;
      } else if (live && j < cap) {
        v[3] += (double)a.alpha[a.idx[r]];
        v[4] += 1.0;
      }
    }
  }
  for (long long r = t; r < S; r += SEL_THREADS) {
    const float* s = a.scale + (long long)a.idx[r] * a.scale_cols;
    const float m = nc == 3 ? (s[0] + s[1] + s[2]) / 3.f : (s[0] + s[1]) / 2.f;
    float iso = fabsf(s[0] - m) + fabsf(s[1] - m);
    if (nc == 3) iso += fabsf(s[2] - m);
    v[5] += (double)iso;
    ar += (double)(nc == 3 ? s[0] * s[1] * s[2] : s[0] * s[1]);
  }
  block_sum<6>(v, sh);
  double w[1] = {ar};
  block_sum<1>(w, sh);
  if (t == 0) {
    const float qnan = __builtin_nanf("");
    const bool on = S > 0;
    a.losses[2] = (a.flags & 4) && on ? (float)(v[5] / (double)(S * nc)) : 0.f;
    a.losses[3] = (a.flags & 8) && on ? (float)(w[0] / (double)S) * a.inv_voxel_pow : 0.f;
    a.losses[4] = sdf_on && on ? (v[2] > 0 ? (float)(v[0] / v[2]) : qnan) : 0.f;
    a.losses[5] = sdf_on && on ? (v[2] > 0 ? (float)(v[1] / v[2]) : qnan) : 0.f;
    a.losses[6] = sdf_on && on ? (v[4] > 0 ? (float)(v[3] / v[4]) : qnan) : 0.f;
    a.meta[3] = (int32_t)v[2]; a.meta[4] = (int32_t)v[4];
    a.counts[3] = sdf_on && on ? v[2] : 0.0;
    a.counts[4] = sdf_on && on ? v[4] : 0.0;
  }
}

// ---------------------------------------------------------------- backward
__global__ __launch_bounds__(256) void gl_rows_bwd_kernel(pings_gauss_loss_args a) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long cap = a.cap, rows = (1 + a.R) * cap;
  if (j >= rows) return;
  float ds = 0.f, v0 = 0.f, v1 = 0.f, v2 = 0.f, n0 = 0.f, n1 = 0.f, n2 = 0.f;
  const int nv = a.meta[3];
  if (a.valid[j] && nv > 0) {
    const float c4 = a.g[4] / (float)nv, c5 = a.g[5] / (float)nv;
    const float d = a.sdf[j] - a.label[j];
    ds = d > 0.f ? c4 : (d < 0.f ? -c4 : 0.f);
    const long long r = j % cap;
    const float gx = a.grad[3 * j], gy = a.grad[3 * j + 1], gz = a.grad[3 * j + 2];
    const float gn = sqrtf(gx * gx + gy * gy + gz * gz), inv = 1.f / (gn + 1e-7f);
    const float nx = a.normal[3 * r], ny = a.normal[3 * r + 1], nz = a.normal[3 * r + 2];
    const float dot = gx * nx + gy * ny + gz * nz;
    // e = 1 - <g, n> / (|g| + eps):  de/dg = -n inv + <g, n> inv^2 g / |g|
    const float k = gn > 0.f ? dot * inv * inv / gn : 0.f;   // torch's norm backward is 0 at the origin
    v0 = c5 * (k * gx - nx * inv); v1 = c5 * (k * gy - ny * inv); v2 = c5 * (k * gz - nz * inv);
    n0 = -c5 * gx * inv; n1 = -c5 * gy * inv; n2 = -c5 * gz * inv;
  }
  a.ds[j] = ds;
  a.v[3 * j] = v0; a.v[3 * j + 1] = v1; a.v[3 * j + 2] = v2;
  a.dn[3 * j] = n0; a.dn[3 * j + 1] = n1; a.dn[3 * j + 2] = n2;
}

// d x_b = dS/dx_b * ds_b + H_S(x_b) v_b for the per-neighbour decoder (weighted_first = 0):
//   S = sum_m w_m s_m,  s_m = scale MLP([f_m, R_m^T (x - p_m)]),  w_m = u_m / U,  u_m = 1 / (|x - g_m|^2 + eps)
//   H v = sum_m (Hw_m v) s_m + dw_m (t_m . v) + t_m (dw_m . v),   t_m = R_m d s_m / d n   (relu'' = 0)
//   Hw_m v = (Hu_m v - dw_m (dU . v) - dU (dw_m . v) - w_m HU v) / U,   Hu_m v = 8 u^3 e (e . v) - 2 u^2 v
// One wave per query, lane h = hidden unit (its W1 row in registers) for the decoder, lane m = neighbour after.
template <int IN_PAD>
__global__ __launch_bounds__(256) void sdf_hvp_kernel(pings_sdf_hvp_args a) {
  __shared__ __attribute__((aligned(16))) float sIn[4][MAX_NNK][IN_PAD > 64 ? IN_PAD : 64];
  __shared__ float sS[4][MAX_NNK][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int F = a.F, IN = F + 3, H = a.H, nnk = a.nnk;
  float w1[IN_PAD], w1n0, w1n1, w1n2;
  load_w1_rows<IN_PAD>(a.W1, IN, H, &sIn[0][0][0], w1, w1n0, w1n1, w1n2);
  const float b1 = lane < H ? a.b1[lane] : 0.f, w2 = lane < H ? a.W2[lane] : 0.f, b2 = a.b2[0];
  const long long nwaves = (long long)gridDim.x * 4;
  for (long long q = (long long)blockIdx.x * 4 + wave; q < a.B; q += nwaves) {
    const float ds = a.ds ? a.ds[q] : 0.f;
    const float vx = a.v[3 * q], vy = a.v[3 * q + 1], vz = a.v[3 * q + 2];
    float ox = 0.f, oy = 0.f, oz = 0.f;
    if (vx != 0.f || vy != 0.f || vz != 0.f) {   // wave-uniform: dead and invalid rows skip the decoder
      const float qx = a.queries[3 * q], qy = a.queries[3 * q + 1], qz = a.queries[3 * q + 2];
      long long id = -1;
      float u = 0.f, ex = 0.f, ey = 0.f, ez = 0.f;
      if (lane < nnk) {
        id = a.idx[q * nnk + lane];
        float nx = 0.f, ny = 0.f, nz = 0.f;
        if (id >= 0) {
          const float px = qx - a.points[3 * id], py = qy - a.points[3 * id + 1], pz = qz - a.points[3 * id + 2];
          nx = px; ny = py; nz = pz;
          if (a.after_pgo) rot_passive(a.orientations + 4 * id, px, py, pz, nx, ny, nz);
          const long long gi = a.gidx[q * nnk + lane];
          ex = qx - a.gpoints[3 * gi]; ey = qy - a.gpoints[3 * gi + 1]; ez = qz - a.gpoints[3 * gi + 2];
          u = 1.0f / (((ex * ex + ey * ey) + ez * ez) + IDW_EPS);
        }
        sIn[wave][lane][F] = nx; sIn[wave][lane][F + 1] = ny; sIn[wave][lane][F + 2] = nz;
        for (int i = IN; i < IN_PAD; ++i) sIn[wave][lane][i] = 0.f;
      }
      for (int e = lane; e < nnk * F; e += 64) {
        const int mm = e / F, f = e - mm * F;
        const long long idm = a.idx[q * nnk + mm];
        sIn[wave][mm][f] = idm >= 0 ? a.features[idm * F + f] : 0.f;
      }
      __builtin_amdgcn_wave_barrier();
      for (int mm = 0; mm < nnk; ++mm) {
        float pre = b1;
#pragma unroll
        for (int i = 0; i < IN_PAD; ++i) pre = fmaf(w1[i], sIn[wave][mm][i], pre);
        const bool on = lane < H && pre > 0.f;
        const float s = wave_sum_all(on ? w2 * pre : 0.f);
        const float g0 = wave_sum_all(on ? w2 * w1n0 : 0.f), g1 = wave_sum_all(on ? w2 * w1n1 : 0.f),
                    g2 = wave_sum_all(on ? w2 * w1n2 : 0.f);
        if (lane == 0) {
          sS[wave][mm][0] = a.scale * (s + b2);
          sS[wave][mm][1] = a.scale * g0; sS[wave][mm][2] = a.scale * g1; sS[wave][mm][3] = a.scale * g2;
        }
      }
      __builtin_amdgcn_wave_barrier();
      const float U = wave_sum_all(u);
      float sm = 0.f, tx = 0.f, ty = 0.f, tz = 0.f;
      if (lane < nnk && id >= 0) {
        sm = sS[wave][lane][0];
        const float gx = sS[wave][lane][1], gy = sS[wave][lane][2], gz = sS[wave][lane][3];
        tx = gx; ty = gy; tz = gz;
        if (a.after_pgo) rot_active(a.orientations + 4 * id, gx, gy, gz, tx, ty, tz);
      }
      const float u2 = u * u, ev = (ex * vx + ey * vy) + ez * vz;
      const float gux = -2.f * u2 * ex, guy = -2.f * u2 * ey, guz = -2.f * u2 * ez;
      const float hx = 8.f * u2 * u * ex * ev - 2.f * u2 * vx, hy = 8.f * u2 * u * ey * ev - 2.f * u2 * vy,
                  hz = 8.f * u2 * u * ez * ev - 2.f * u2 * vz;
      const float GUx = wave_sum_all(gux), GUy = wave_sum_all(guy), GUz = wave_sum_all(guz);
      const float HUx = wave_sum_all(hx), HUy = wave_sum_all(hy), HUz = wave_sum_all(hz);
      float cx = 0.f, cy = 0.f, cz = 0.f;
      if (U > 0.f && lane < nnk && id >= 0) {
        const float iU = 1.f / U, w = u * iU;
        const float dwx = (gux - w * GUx) * iU, dwy = (guy - w * GUy) * iU, dwz = (guz - w * GUz) * iU;
        const float GUv = GUx * vx + GUy * vy + GUz * vz, dwv = dwx * vx + dwy * vy + dwz * vz;
        const float tv = tx * vx + ty * vy + tz * vz;
        const float Hx = (hx - dwx * GUv - GUx * dwv - w * HUx) * iU, Hy = (hy - dwy * GUv - GUy * dwv - w * HUy) * iU,
                    Hz = (hz - dwz * GUv - GUz * dwv - w * HUz) * iU;
        cx = Hx * sm + dwx * tv + tx * dwv; cy = Hy * sm + dwy * tv + ty * dwv; cz = Hz * sm + dwz * tv + tz * dwv;
      }
      ox = wave_sum_all(cx); oy = wave_sum_all(cy); oz = wave_sum_all(cz);
      __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) {
      const float* g = a.grad_x;
      a.out[3 * q] = (g ? g[3 * q] * ds : 0.f) + ox;
      a.out[3 * q + 1] = (g ? g[3 * q + 1] * ds : 0.f) + oy;
      a.out[3 * q + 2] = (g ? g[3 * q + 2] * ds : 0.f) + oz;
    }
  }
}

__global__ __launch_bounds__(256) void gl_scatter_bwd_kernel(pings_gauss_loss_args a) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long S = a.meta[1], cap = a.cap;
  if (r >= S) return;
  const long long i = a.idx[r];
  const float* g = a.g;
  const int nc = a.ncols;
  // isotropy and area: d scale (mean over S * nc elements, resp. S rows)
  const float* s = a.scale + i * a.scale_cols;
  float* dsc = a.d_scale + i * a.scale_cols;
  if (a.flags & 4) {
    const float m = nc == 3 ? (s[0] + s[1] + s[2]) / 3.f : (s[0] + s[1]) / 2.f;
    const float c = g[2] / (float)(S * nc);
    float sg[3] = {0.f, 0.f, 0.f}, sum = 0.f;
    for (int k = 0; k < nc; ++k) { const float d = s[k] - m; sg[k] = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); sum += sg[k]; }
    for (int k = 0; k < nc; ++k) dsc[k] += c * (sg[k] - sum / (float)nc);
  }
  if (a.flags & 8) {
    const float c = g[3] / (float)S * a.inv_voxel_pow;
    if (nc == 3) { dsc[0] += c * s[1] * s[2]; dsc[1] += c * s[0] * s[2]; dsc[2] += c * s[0] * s[1]; }
    else { dsc[0] += c * s[1]; dsc[1] += c * s[0]; }
  }
  if (!(a.flags & 16)) return;
  const int ninv = a.meta[4];
  if (!a.valid[r] && ninv > 0) a.d_alpha[i] = g[6] / (float)ninv;
  // the 1 + R copies of the sample, in block order
  float dx = a.dq[3 * r], dy = a.dq[3 * r + 1], dz = a.dq[3 * r + 2];
  float dnx = a.dn[3 * r], dny = a.dn[3 * r + 1], dnz = a.dn[3 * r + 2];
  for (int k = 1; k <= a.R; ++k) {
    const long long j = k * cap + r;
    const float qx = a.dq[3 * j], qy = a.dq[3 * j + 1], qz = a.dq[3 * j + 2], sh = a.label[j];
    dx += qx; dy += qy; dz += qz;
    dnx += a.dn[3 * j] + sh * qx; dny += a.dn[3 * j + 1] + sh * qy; dnz += a.dn[3 * j + 2] + sh * qz;
  }
  a.d_xyz[3 * i] = dx; a.d_xyz[3 * i + 1] = dy; a.d_xyz[3 * i + 2] = dz;
  // normalise: dN = (dn - n <n, dn>) / |N|  (F.normalize below its eps: dN = dn / eps)
  const float* q = a.rot + 4 * i;
  float nx, ny, nz, cx, cy, cz, len;
  quat_normal(q, nx, ny, nz, cx, cy, cz, len);
  float d0, d1, d2;
  if (len > 1e-12f) {
    const float p = nx * dnx + ny * dny + nz * dnz;
    d0 = (dnx - nx * p) / len; d1 = (dny - ny * p) / len; d2 = (dnz - nz * p) / len;
  } else {
    d0 = dnx / 1e-12f; d1 = dny / 1e-12f; d2 = dnz / 1e-12f;
  }
  const float rr = q[0], x = q[1], y = q[2], z = q[3];
  a.d_rot[4 * i] = 2.f * y * d0 - 2.f * x * d1;
  a.d_rot[4 * i + 1] = 2.f * z * d0 - 2.f * rr * d1 - 4.f * x * d2;
  a.d_rot[4 * i + 2] = 2.f * rr * d0 + 2.f * z * d1 - 4.f * y * d2;
  a.d_rot[4 * i + 3] = 2.f * x * d0 + 2.f * y * d1;
}

__global__ __launch_bounds__(256) void gl_alpha_all_bwd_kernel(pings_gauss_loss_args a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.Na) return;
  const float x = a.alpha_all[i];
  float d = 0.f;
  const int nlt = a.meta[2];
  if ((a.flags & 1) && nlt > 0 && x < a.min_alpha) d -= a.g[0] / (float)nlt;
  if (a.flags & 2) {
    const float ax = fabsf(x);
    if (ax >= 1e-6f && ax <= 1.f - 1e-6f && x != 0.f) {   // clamp passes the gradient inside [min, max]; |x|' = sign
      const float de = logf((1.f - ax) / ax);
      d += a.g[1] / (float)a.Na * de * (x > 0.f ? 1.f : -1.f);
    }
  }
  a.d_alpha_all[i] = d;
}

int check_args(const pings_gauss_loss_args* a) {
  PINGS_ARG_CHECK(a != nullptr, "null args");
  PINGS_ARG_CHECK(a->P >= 0 && a->P < 0x7FFFFFF0LL && a->Na >= 0 && a->Na < (1LL << 40), "sizes out of range");
  PINGS_ARG_CHECK(a->cap > 0 && a->cap < (1LL << 28), "cap out of range");
  PINGS_ARG_CHECK(a->R >= 0 && a->R <= 64, "shift count out of range");
  PINGS_ARG_CHECK(a->ncols == 2 || a->ncols == 3, "ncols must be 2 or 3");
  PINGS_ARG_CHECK(a->scale_cols >= a->ncols, "scale rows narrower than ncols");
  PINGS_ARG_CHECK(a->n_inject <= a->cap, "more injected samples than cap");
  PINGS_ARG_CHECK(a->meta && a->losses && a->counts, "null outputs");
  return PINGS_OK;
}

}  // namespace

PINGS_API int pings_gauss_loss_select(const pings_gauss_loss_args* a, void* stream) {
  if (int e = check_args(a)) return e;
  PINGS_ARG_CHECK(a->keys && a->part && a->idx, "null workspace");
  PINGS_ARG_CHECK(a->P == 0 || (a->visible && a->alpha), "null Gaussian inputs");
  PINGS_ARG_CHECK(a->Na == 0 || a->alpha_all, "null alpha_all");
  PINGS_ARG_CHECK(a->n_inject >= 0 ? a->inject_idx != nullptr : a->seed != nullptr, "need a seed or injected indices");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("gauss_loss_select", st);
  hipLaunchKernelGGL(gl_mask_kernel, dim3(MASK_BLOCKS), dim3(MASK_THREADS), 0, st, *a);
  PINGS_LAUNCH_CHECK();
  hipLaunchKernelGGL(gl_select_kernel, dim3(1), dim3(SEL_THREADS), 0, st, *a);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API int pings_gauss_loss_prepare(const pings_gauss_loss_args* a, void* stream) {
  if (int e = check_args(a)) return e;
  PINGS_ARG_CHECK(a->idx && a->normal && a->queries && a->label, "null workspace");
  PINGS_ARG_CHECK(a->R == 0 || a->randn, "null shift draws");
  PINGS_ARG_CHECK(a->P == 0 || (a->xyz && a->rot), "null Gaussian inputs");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("gauss_loss_prepare", st);
  hipLaunchKernelGGL(gl_prepare_kernel, dim3((unsigned)((a->cap + 255) / 256)), dim3(256), 0, st, *a);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API int pings_gauss_loss_reduce(const pings_gauss_loss_args* a, void* stream) {
  if (int e = check_args(a)) return e;
  PINGS_ARG_CHECK(a->idx && (a->P == 0 || a->scale), "null inputs");
  PINGS_ARG_CHECK(!(a->flags & 16) || (a->grad && a->sdf && a->nn && a->valid && a->normal && a->label),
                  "null SDF rows");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("gauss_loss_reduce", st);
  hipLaunchKernelGGL(gl_reduce_kernel, dim3(1), dim3(SEL_THREADS), 0, st, *a);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API int pings_gauss_loss_backward_rows(const pings_gauss_loss_args* a, void* stream) {
  if (int e = check_args(a)) return e;
  PINGS_ARG_CHECK(a->g && a->ds && a->v && a->dn && a->valid && a->grad && a->sdf, "null backward buffers");
  hipStream_t st = pings::as_stream(stream);
  const long long rows = (1 + a->R) * a->cap;
  pings::prof::Scope ps("gauss_loss_bwd_rows", st);
  hipLaunchKernelGGL(gl_rows_bwd_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, *a);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API int pings_gauss_loss_backward_scatter(const pings_gauss_loss_args* a, void* stream) {
  if (int e = check_args(a)) return e;
  PINGS_ARG_CHECK(a->g, "null upstream gradient");
  PINGS_ARG_CHECK(a->P == 0 || (a->d_xyz && a->d_rot && a->d_scale && a->d_alpha), "null Gaussian gradients");
  PINGS_ARG_CHECK(!(a->flags & 16) || (a->dq && a->dn && a->valid), "null SDF row gradients");
  PINGS_ARG_CHECK(a->Na == 0 || a->d_alpha_all, "null alpha_all gradient");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("gauss_loss_bwd_scatter", st);
  // the dense outputs arrive zeroed (one memset of the caller's single allocation)
  hipLaunchKernelGGL(gl_scatter_bwd_kernel, dim3((unsigned)((a->cap + 255) / 256)), dim3(256), 0, st, *a);
  PINGS_LAUNCH_CHECK();
  if (a->Na > 0) {
    hipLaunchKernelGGL(gl_alpha_all_bwd_kernel, dim3((unsigned)((a->Na + 255) / 256)), dim3(256), 0, st, *a);
    PINGS_LAUNCH_CHECK();
  }
  return PINGS_OK;
}

PINGS_API int pings_sdf_hvp_x(const pings_sdf_hvp_args* a, void* stream) {
  PINGS_ARG_CHECK(a != nullptr, "null args");
  PINGS_ARG_CHECK(a->H > 0 && a->H <= 64 && a->F > 0 && a->F <= 61, "decoder shape outside the fused kernels");
  PINGS_ARG_CHECK(a->nnk > 0 && a->nnk <= MAX_NNK, "nn_k must be in 1..16");
  PINGS_ARG_CHECK(!a->after_pgo || a->orientations, "after_pgo needs orientations");
  PINGS_ARG_CHECK(a->B == 0 || (a->W1 && a->b1 && a->W2 && a->b2 && a->features && a->points && a->gpoints &&
                                a->queries && a->idx && a->gidx && a->v && a->out), "null pointer");
  if (a->B == 0) return PINGS_OK;
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("sdf_hvp_x", st);
  const int IN = a->F + 3;
  const unsigned nb = (unsigned)std::min<long long>((a->B + 3) / 4, 2048);
  if (IN <= 12) hipLaunchKernelGGL(sdf_hvp_kernel<12>, dim3(nb), dim3(256), 0, st, *a);
  else if (IN <= 20) hipLaunchKernelGGL(sdf_hvp_kernel<20>, dim3(nb), dim3(256), 0, st, *a);
  else if (IN <= 36) hipLaunchKernelGGL(sdf_hvp_kernel<36>, dim3(nb), dim3(256), 0, st, *a);
  else hipLaunchKernelGGL(sdf_hvp_kernel<64>, dim3(nb), dim3(256), 0, st, *a);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}
