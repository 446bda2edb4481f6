// Tracker registration step: normal equations of one point-to-implicit-model Gauss-Newton /
// Levenberg-Marquardt iteration, utils/tracker.py:608-689 (`implicit_reg`, adapted there from LocNDF).
//
// With J_i = [p_i x g_i, g_i] (rotation first, then translation) the reference forms  N = J^T (w J)  and
// g = -(J w)^T r  with two GEMMs over the n x 6 Jacobian after materialising the cross products, the concatenation
// and the weighted copy (five n-sized temporaries).  Here one pass reads the 8 floats of a point and accumulates the
// 21 distinct entries of N and the 6 of g in fp64 registers; wave shuffle + LDS reduce per workgroup, per-workgroup
// partials in global memory, and a second tiny kernel sums them in fixed order: bitwise reproducible.  HBM bound:
// 32 B per point.
//
// The odometry loop (`pings_reg_transform` / `_assemble` / `_step`, pings_amd/tracker_ops.py: tracking) runs a whole
// iteration of Tracker.tracking around the fused query with the pose in device memory: the validity filter and the
// weights are folded into the same one-pass accumulation (invalid points weighted out, nothing compacted), and one
// single-workgroup kernel sums the partials, solves, composes the pose and writes the small record the host reads.
#include <cmath>
#include "common.hpp"

namespace {

constexpr int kTerms = 27;    // 21 upper-triangle entries of N, 6 of g
constexpr int kBlocks = 512;

__global__ __launch_bounds__(256) void reg_accumulate_kernel(const float* __restrict__ pts, const float* __restrict__ grad,
                                                             const float* __restrict__ res, const float* __restrict__ wgt,
                                                             long long n, double* __restrict__ partial) {
  __shared__ double red[4][kTerms];
  double acc[kTerms];
#pragma unroll
  for (int k = 0; k < kTerms; ++k) acc[k] = 0.0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
    const float gx = grad[3 * i], gy = grad[3 * i + 1], gz = grad[3 * i + 2];
    float J[6];
    J[0] = py * gz - pz * gy;   // torch.linalg.cross(points, sdf_grad) in fp32, as the reference
    J[1] = pz * gx - px * gz;
    J[2] = px * gy - py * gx;
    J[3] = gx; J[4] = gy; J[5] = gz;
    const double w = (double)wgt[i], r = (double)res[i];
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const double wa = w * (double)J[a];
#pragma unroll
      for (int b = a; b < 6; ++b) acc[k++] += wa * (double)J[b];
      acc[21 + a] -= wa * r;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kTerms; ++k) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < kTerms)
    partial[(size_t)blockIdx.x * kTerms + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

__global__ void reg_finish_kernel(const double* __restrict__ partial, int nblocks, float* __restrict__ out) {
  __shared__ double tot[kTerms];
  const int k = threadIdx.x;
  if (k < kTerms) {
    double v = 0.0;
    for (int b = 0; b < nblocks; ++b) v += partial[(size_t)b * kTerms + k];
    tot[k] = v;
  }
  __syncthreads();
  if (k == 0) {
    int t = 0;
    for (int a = 0; a < 6; ++a)
      for (int b = a; b < 6; ++b) {
        out[a * 6 + b] = (float)tot[t];
        out[b * 6 + a] = (float)tot[t];
        ++t;
      }
    for (int a = 0; a < 6; ++a) out[36 + a] = (float)tot[21 + a];
  }
}

// LM damping, the fp64 6x6 solve and the exponential map of one registration step (utils/tracker.py:649-689, :774-783)
// in one single-thread kernel: the reference spends ~30 tiny torch launches and a host sync (linalg.inv checks its
// info word) on it, 50-100 times per frame.  N is damped in fp32 like the reference's `N_mat += lambda diag(N_mat)`,
// then everything is fp64: t = N^-1 g by Gaussian elimination with partial pivoting, R = I + S sin(a) + S^2 (1 - cos a).
// status (optional device word): PINGS_REG_SINGULAR = a pivot is exactly zero or not finite — the case in which the
// reference's torch.linalg.inv raises (utils/tracker.py:668; LAPACK getrf info > 0); PINGS_REG_ILL_CONDITIONED = the
// smallest pivot is below 1e-7 (one fp32 ulp: N arrives rounded to fp32) of the largest entry of the damped matrix,
// i.e. the step is decided by rounding noise; PINGS_REG_NONFINITE = t or the pose came out Inf / NaN.
// The solve of one step from the 42 floats [N | g]: returns the status bits (PINGS_REG_*), writes T[16] and t[6].
__device__ int reg_solve_dev(const float* __restrict__ ng, float lm_lambda, double* __restrict__ T_out,
                             double* __restrict__ t_out) {
  double A[6][7];
  double scale = 0.0, min_piv = 1e300;
  int flags = 0;
  for (int r = 0; r < 6; ++r) {
    for (int c = 0; c < 6; ++c) {
      float v = ng[r * 6 + c];
      if (r == c) v += lm_lambda * v;
      A[r][c] = (double)v;
      scale = fmax(scale, fabs((double)v));
    }
    A[r][6] = (double)ng[36 + r];
  }
  for (int k = 0; k < 6; ++k) {
    int piv = k;
    for (int r = k + 1; r < 6; ++r)
      if (fabs(A[r][k]) > fabs(A[piv][k])) piv = r;
    if (piv != k)
      for (int c = 0; c < 7; ++c) { const double t = A[k][c]; A[k][c] = A[piv][c]; A[piv][c] = t; }
    if (A[k][k] == 0.0 || !isfinite(A[k][k])) flags |= PINGS_REG_SINGULAR;
    min_piv = fmin(min_piv, fabs(A[k][k]));
    const double inv = 1.0 / A[k][k];
    for (int r = k + 1; r < 6; ++r) {
      const double f = A[r][k] * inv;
      for (int c = k; c < 7; ++c) A[r][c] -= f * A[k][c];
    }
  }
  double t[6];
  for (int r = 5; r >= 0; --r) {
    double v = A[r][6];
    for (int c = r + 1; c < 6; ++c) v -= A[r][c] * t[c];
    t[r] = v / A[r][r];
  }
  const double angle = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
  const double ax = t[0] / angle, ay = t[1] / angle, az = t[2] / angle;   // angle = 0 -> NaN, as the reference
  const double S[3][3] = {{0.0, -az, ay}, {az, 0.0, -ax}, {-ay, ax, 0.0}};
  const double sn = sin(angle), cs = 1.0 - cos(angle);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double s2 = 0.0;
      for (int k = 0; k < 3; ++k) s2 += S[r][k] * S[k][c];
      T_out[r * 4 + c] = (r == c ? 1.0 : 0.0) + S[r][c] * sn + s2 * cs;
    }
  for (int r = 0; r < 3; ++r) T_out[r * 4 + 3] = t[3 + r];
  T_out[12] = 0.0; T_out[13] = 0.0; T_out[14] = 0.0; T_out[15] = 1.0;
  if (t_out)
    for (int r = 0; r < 6; ++r) t_out[r] = t[r];
  if (!(min_piv >= 1e-7 * scale)) flags |= PINGS_REG_ILL_CONDITIONED;   // also when scale is NaN
  bool fin = true;
  for (int r = 0; r < 6; ++r) fin = fin && isfinite(t[r]);
  // (t = 0 exactly makes the axis 0 / 0, as in the reference's expmap: reported as non-finite, not as singular)
  for (int r = 0; r < 12; ++r) fin = fin && isfinite(T_out[r]);
  if (!fin) flags |= PINGS_REG_NONFINITE;
  return flags;
}

__global__ void reg_solve_kernel(const float* __restrict__ ng, float lm_lambda, double* __restrict__ T_out,
                                 double* __restrict__ t_out, int32_t* __restrict__ status) {
  const int flags = reg_solve_dev(ng, lm_lambda, T_out, t_out);
  if (status) *status = flags;
}

// ---------------------------------------------------------------- device-resident odometry loop
// One iteration of Tracker.tracking (utils/tracker.py:43-210) around the fused query: transform, assemble, step.  The
// pose stays in device memory; the host reads the 8-word record of the step and nothing else.

constexpr int kLoopTerms = 32;   // 27 normal-equation entries, valid count, sum w, sum |r|, sum w r^2, (pad)
constexpr int kLoopBlocks = 256;
constexpr int kTraceRow = 24;

__host__ __device__ inline int loop_blocks(long long n) {
  long long nb = (n + 255) / 256;
  return (int)(nb < 1 ? 1 : (nb > kLoopBlocks ? kLoopBlocks : nb));
}

// transform_torch (utils/tools.py:888-900): [p, 1] @ T.to(fp32).T, in fp32
__global__ __launch_bounds__(256) void reg_transform_kernel(const float* __restrict__ src, const double* __restrict__ T,
                                                            long long n, float* __restrict__ out) {
  float M[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) M[k] = (float)T[k];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) out[3 * i + r] = ((M[4 * r] * x + M[4 * r + 1] * y) + M[4 * r + 2] * z) + M[4 * r + 3];
  }
}

// registration_step (utils/tracker.py:353-605) up to implicit_reg's GEMMs, with the invalid points weighted out
__global__ __launch_bounds__(256) void reg_assemble_kernel(pings_reg_loop_args a) {
  __shared__ double red[4][kLoopTerms];
  double acc[kLoopTerms];
#pragma unroll
  for (int k = 0; k < kLoopTerms; ++k) acc[k] = 0.0;
  const bool normals = (a.flags & PINGS_REG_F_NORMALS) && a.normals, div = a.flags & PINGS_REG_F_DIV_GRAD;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (long long)gridDim.x * blockDim.x) {
    const float gx = a.grad[3 * i], gy = a.grad[3 * i + 1], gz = a.grad[3 * i + 2];
    const float gn = sqrtf((gx * gx + gy * gy) + gz * gz);
    const bool ok = a.mask[i] && gn < a.max_grad && gn > a.min_grad && a.std[i] < a.max_std;
    if (a.valid) a.valid[i] = ok;
    if (!ok) continue;
    float sdf = a.sdf[i];
    if (div) sdf = sdf / gn;
    const float r = sdf - a.label[i];
    float w = 1.f;
    if (a.gm_dist > 0.f) { const float q = a.gm_dist / (a.gm_dist + r * r); w = q * q; }          // w_res
    if (a.gm_grad > 0.f) {                                                                        // * w_grad
      const float an = gn - 1.f, q = a.gm_grad / (a.gm_grad + an * an);
      w = w * (q * q);
    }
    if (normals) {                                                                                // * w_normal
      const float den = gn + 1e-7f;
      const float ux = gx / den, uy = gy / den, uz = gz / den;
      const float d = (a.normals[3 * i] * ux + a.normals[3 * i + 1] * uy) + a.normals[3 * i + 2] * uz;
      w = w * (0.5f + fabsf(d));
    }
    const float px = a.cur[3 * i], py = a.cur[3 * i + 1], pz = a.cur[3 * i + 2];
    float J[6];
    J[0] = py * gz - pz * gy;
    J[1] = pz * gx - px * gz;
    J[2] = px * gy - py * gx;
    J[3] = gx; J[4] = gy; J[5] = gz;
    const double wd = (double)w, rd = (double)r;
    int k = 0;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
      const double wa = wd * (double)J[p];
#pragma unroll
      for (int q = p; q < 6; ++q) acc[k++] += wa * (double)J[q];
      acc[21 + p] -= wa * rd;
    }
    acc[27] += 1.0;
    acc[28] += wd;
    acc[29] += fabs(rd);
    acc[30] += wd * rd * rd;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kLoopTerms; ++k) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < kLoopTerms)
    a.part[(size_t)blockIdx.x * kLoopTerms + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// reg_assemble_kernel with the colour terms of registration_step (utils/tracker.py:485-535) and implicit_color_reg
// (:692-737).  The reference sums the geometric and the photometric system before damping (N = N_geo + lambda N_col, g
// likewise), so both go into the same 27 sums and reg_step_kernel runs behind this kernel as it stands.  PHOTO: residual
// r_c = I_pred - I_src and J_c = [p x grad I, grad I] of the intensity (the one channel, or 0.144 c0 + 0.299 c1 +
// 0.587 c2 of three: utils/tools.py:723, applied to colours and Jacobian rows alike).  CONSIST: the weight is multiplied
// by exp(-|I_src - I_pred|), no Jacobian is read.  Validity is the SDF's alone; an invalid point's colours are not read.
__device__ inline float reg_intensity(const float* __restrict__ c, int channels) {
  return channels == 3 ? (0.144f * c[0] + 0.299f * c[1]) + 0.587f * c[2] : c[0];
}

__global__ __launch_bounds__(256) void reg_assemble_color_kernel(pings_reg_loop_args a, pings_reg_color_args ca) {
  __shared__ double red[4][kLoopTerms];
  double acc[kLoopTerms];
#pragma unroll
  for (int k = 0; k < kLoopTerms; ++k) acc[k] = 0.0;
  const bool normals = (a.flags & PINGS_REG_F_NORMALS) && a.normals, div = a.flags & PINGS_REG_F_DIV_GRAD;
  const bool photo = ca.mode == PINGS_REG_COLOR_PHOTO;
  const int C = ca.channels;
  const double lam = (double)ca.photo_weight;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (long long)gridDim.x * blockDim.x) {
    const float gx = a.grad[3 * i], gy = a.grad[3 * i + 1], gz = a.grad[3 * i + 2];
    const float gn = sqrtf((gx * gx + gy * gy) + gz * gz);
    const bool ok = a.mask[i] && gn < a.max_grad && gn > a.min_grad && a.std[i] < a.max_std;
    if (a.valid) a.valid[i] = ok;
    if (!ok) continue;
    float sdf = a.sdf[i];
    if (div) sdf = sdf / gn;
    const float r = sdf - a.label[i];
    float w = 1.f;
    if (a.gm_dist > 0.f) { const float q = a.gm_dist / (a.gm_dist + r * r); w = q * q; }          // w_res
    if (a.gm_grad > 0.f) {                                                                        // * w_grad
      const float an = gn - 1.f, q = a.gm_grad / (a.gm_grad + an * an);
      w = w * (q * q);
    }
    if (normals) {                                                                                // * w_normal
      const float den = gn + 1e-7f;
      const float ux = gx / den, uy = gy / den, uz = gz / den;
      const float d = (a.normals[3 * i] * ux + a.normals[3 * i + 1] * uy) + a.normals[3 * i + 2] * uz;
      w = w * (0.5f + fabsf(d));
    }
    const float i_src = reg_intensity(ca.src_color + (size_t)i * C, C);
    const float i_pred = reg_intensity(ca.color_pred + (size_t)i * C, C);
    const float rc = i_pred - i_src;
    if (!photo) w = w * expf(-fabsf(i_src - i_pred));                                             // * w_color
    const float px = a.cur[3 * i], py = a.cur[3 * i + 1], pz = a.cur[3 * i + 2];
    float J[6], Jc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    J[0] = py * gz - pz * gy;
    J[1] = pz * gx - px * gz;
    J[2] = px * gy - py * gx;
    J[3] = gx; J[4] = gy; J[5] = gz;
    if (photo) {
      const float* jc = ca.color_jac + (size_t)i * C * 3;
      float cx, cy, cz;
      if (C == 3) {
        cx = (0.144f * jc[0] + 0.299f * jc[3]) + 0.587f * jc[6];
        cy = (0.144f * jc[1] + 0.299f * jc[4]) + 0.587f * jc[7];
        cz = (0.144f * jc[2] + 0.299f * jc[5]) + 0.587f * jc[8];
      } else {
        cx = jc[0]; cy = jc[1]; cz = jc[2];
      }
      Jc[0] = py * cz - pz * cy;
      Jc[1] = pz * cx - px * cz;
      Jc[2] = px * cy - py * cx;
      Jc[3] = cx; Jc[4] = cy; Jc[5] = cz;
    }
    const double wd = (double)w, rd = (double)r, wl = wd * lam, rcd = (double)rc;
    int k = 0;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
      const double wa = wd * (double)J[p], wc = wl * (double)Jc[p];
#pragma unroll
      for (int q = p; q < 6; ++q) acc[k++] += wa * (double)J[q] + wc * (double)Jc[q];
      acc[21 + p] -= wa * rd + wc * rcd;
    }
    acc[27] += 1.0;
    acc[28] += wd;
    acc[29] += fabs(rd);
    acc[30] += wd * rd * rd;
    acc[31] += fabs(rcd);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kLoopTerms; ++k) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < kLoopTerms) {
    const double v = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    // slot 31 of `part` stays the pad it is today (0); sum |r_c| has a buffer of its own
    if (threadIdx.x < kLoopTerms - 1) a.part[(size_t)blockIdx.x * kLoopTerms + threadIdx.x] = v;
    else {
      a.part[(size_t)blockIdx.x * kLoopTerms + threadIdx.x] = 0.0;
      ca.photo_part[blockIdx.x] = v;
    }
  }
}

// The update of one iteration (utils/tracker.py:407-413, :494-497, :608-689, :121-168) in one workgroup of 64
__global__ __launch_bounds__(64) void reg_step_kernel(pings_reg_loop_args a, int nblocks) {
  __shared__ double tot[kLoopTerms];
  const int k = threadIdx.x;
  if (k < kLoopTerms) {
    double v = 0.0;
    for (int b = 0; b < nblocks; ++b) v += a.part[(size_t)b * kLoopTerms + k];
    tot[k] = v;
  }
  __syncthreads();
  if (k != 0) return;
  const double cnt = tot[27];
  double D[16];
  double res_cm = 0.0;
  int flags = 0;
  if (cnt < 10.0) {   // registration_step's early return: identity step, residual 0.0
    for (int e = 0; e < 16; ++e) D[e] = (e % 5 == 0) ? 1.0 : 0.0;
  } else {
    // w /= 2 mean(w) scales N and g by one factor: the step is unchanged, the damped N is not re-rounded differently
    const double c = (a.flags & PINGS_REG_F_WEIGHTED) ? cnt / (2.0 * tot[28]) : 1.0;
    float ng[42];
    int t = 0;
    for (int p = 0; p < 6; ++p)
      for (int q = p; q < 6; ++q) {
        const float v = (float)(c * tot[t++]);
        ng[p * 6 + q] = v;
        ng[q * 6 + p] = v;
      }
    for (int p = 0; p < 6; ++p) ng[36 + p] = (float)(c * tot[21 + p]);
    flags = reg_solve_dev(ng, a.lm_lambda, D, nullptr);
    res_cm = (double)(float)(tot[29] / cnt) * 100.0;   // torch.mean(|r|).item() of an fp32 tensor, times 100
  }
  double Tn[16];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      double v = 0.0;
      for (int m = 0; m < 4; ++m) v += D[r * 4 + m] * a.T[m * 4 + c];
      Tn[r * 4 + c] = v;
    }
  for (int e = 0; e < 16; ++e) {
    a.T[e] = Tn[e];
    a.delta[e] = D[e];
  }
  const double rot_deg = acos(((D[0] + D[5]) + D[10] - 1.0) / 2.0) * 180.0 / M_PI;   // NaN when (tr - 1) / 2 > 1
  const double tran_m = sqrt((D[3] * D[3] + D[7] * D[7]) + D[11] * D[11]);
  a.record[0] = (int32_t)cnt;
  a.record[1] = flags;
  const double vals[3] = {res_cm, rot_deg, tran_m};
  for (int e = 0; e < 3; ++e) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(vals[e]);
    a.record[2 + 2 * e] = (int32_t)(uint32_t)(u & 0xffffffffull);
    a.record[3 + 2 * e] = (int32_t)(uint32_t)(u >> 32);
  }
  if (a.trace && a.iter >= 0 && a.iter < a.trace_cap) {
    double* row = a.trace + (size_t)a.iter * kTraceRow;
    row[0] = cnt; row[1] = res_cm; row[2] = rot_deg; row[3] = tran_m; row[4] = (double)flags;
    row[5] = tot[28]; row[6] = tot[30]; row[7] = 0.0;
    for (int e = 0; e < 16; ++e) row[8 + e] = D[e];
  }
}

}  // namespace

PINGS_API int pings_reg_solve_checked(const float* normal_eq, float lm_lambda, double* T_out, double* t_out,
                                      int32_t* status_dev, int32_t* status_host, void* stream) {
  PINGS_ARG_CHECK(normal_eq && T_out, "null pointer");
  PINGS_ARG_CHECK(status_dev || !status_host, "status_host needs status_dev");
  hipStream_t st = pings::as_stream(stream);
  {
    pings::prof::Scope sc("reg_solve", st);
    reg_solve_kernel<<<1, 1, 0, st>>>(normal_eq, lm_lambda, T_out, t_out, status_dev);
    PINGS_LAUNCH_CHECK();
  }
  if (status_host) {   // the reference synchronises here as well (linalg.inv reads its info word)
    const uint32_t* w[1] = {reinterpret_cast<const uint32_t*>(status_dev)};
    uint32_t v = 0;
    const int rc = pings::host_read_words(w, 1, &v, st);
    if (rc != PINGS_OK) return rc;
    *status_host = (int32_t)v;
  }
  return PINGS_OK;
}

PINGS_API int pings_reg_solve(const float* normal_eq, float lm_lambda, double* T_out, double* t_out, void* stream) {
  return pings_reg_solve_checked(normal_eq, lm_lambda, T_out, t_out, nullptr, nullptr, stream);
}

PINGS_API size_t pings_reg_normal_equations_scratch_bytes(void) { return sizeof(double) * kBlocks * kTerms; }

PINGS_API int pings_reg_normal_equations(const float* points, const float* sdf_grad, const float* sdf_residual,
                                         const float* weight, int64_t n, void* scratch, float* out, void* stream) {
  PINGS_ARG_CHECK(n >= 0 && out && scratch, "bad argument");
  PINGS_ARG_CHECK(n == 0 || (points && sdf_grad && sdf_residual && weight), "null input");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("reg_normal_equations", st);
  int nb = (int)((n + 255) / 256);
  nb = nb < 1 ? 1 : (nb > kBlocks ? kBlocks : nb);
  reg_accumulate_kernel<<<nb, 256, 0, st>>>(points, sdf_grad, sdf_residual, weight, (long long)n,
                                            reinterpret_cast<double*>(scratch));
  PINGS_LAUNCH_CHECK();
  reg_finish_kernel<<<1, 64, 0, st>>>(reinterpret_cast<const double*>(scratch), nb, out);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API int pings_reg_partials(int64_t n) { return loop_blocks(n); }

PINGS_API int pings_reg_transform(const pings_reg_loop_args* a, void* stream) {
  PINGS_ARG_CHECK(a && a->n >= 0 && a->T && a->cur, "bad argument");
  PINGS_ARG_CHECK(a->n == 0 || a->src, "null source points");
  if (a->n == 0) return PINGS_OK;
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("reg_transform", st);
  long long nb = (a->n + 255) / 256;
  nb = nb > 2048 ? 2048 : nb;
  reg_transform_kernel<<<(int)nb, 256, 0, st>>>(a->src, a->T, (long long)a->n, a->cur);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API int pings_reg_assemble(const pings_reg_loop_args* a, void* stream) {
  PINGS_ARG_CHECK(a && a->n >= 0 && a->part, "bad argument");
  PINGS_ARG_CHECK(a->n == 0 || (a->cur && a->sdf && a->grad && a->std && a->mask && a->label), "null input");
  PINGS_ARG_CHECK(!(a->flags & PINGS_REG_F_NORMALS) || a->normals, "PINGS_REG_F_NORMALS without normals");
  PINGS_ARG_CHECK((a->flags & ~7) == 0, "unknown flag");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("reg_assemble", st);
  reg_assemble_kernel<<<loop_blocks(a->n), 256, 0, st>>>(*a);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API int pings_reg_assemble_color(const pings_reg_loop_args* a, const pings_reg_color_args* c, void* stream) {
  PINGS_ARG_CHECK(a && a->n >= 0 && a->part, "bad argument");
  PINGS_ARG_CHECK(a->n == 0 || (a->cur && a->sdf && a->grad && a->std && a->mask && a->label), "null input");
  PINGS_ARG_CHECK(!(a->flags & PINGS_REG_F_NORMALS) || a->normals, "PINGS_REG_F_NORMALS without normals");
  PINGS_ARG_CHECK((a->flags & ~7) == 0, "unknown flag");
  PINGS_ARG_CHECK(c && c->photo_part, "null colour arguments");
  PINGS_ARG_CHECK(c->channels == 1 || c->channels == 3, "channels must be 1 or 3");
  PINGS_ARG_CHECK(c->mode == PINGS_REG_COLOR_PHOTO || c->mode == PINGS_REG_COLOR_CONSIST, "unknown colour mode");
  PINGS_ARG_CHECK(a->n == 0 || (c->src_color && c->color_pred), "null colours");
  PINGS_ARG_CHECK(a->n == 0 || c->mode != PINGS_REG_COLOR_PHOTO || c->color_jac, "the photometric term needs color_jac");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("reg_assemble_color", st);
  reg_assemble_color_kernel<<<loop_blocks(a->n), 256, 0, st>>>(*a, *c);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API int pings_reg_step(const pings_reg_loop_args* a, void* stream) {
  PINGS_ARG_CHECK(a && a->n >= 0 && a->part && a->T && a->delta && a->record, "bad argument");
  PINGS_ARG_CHECK(!a->trace || a->trace_cap > 0, "trace without rows");
  PINGS_ARG_CHECK((a->flags & ~7) == 0, "unknown flag");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("reg_step", st);
  reg_step_kernel<<<1, 64, 0, st>>>(*a, loop_blocks(a->n));
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API int pings_reg_read_record(const int32_t* record_dev, int32_t* record_host, void* stream) {
  PINGS_ARG_CHECK(record_dev && record_host, "null pointer");
  const uint32_t* w[8];
  for (int i = 0; i < 8; ++i) w[i] = reinterpret_cast<const uint32_t*>(record_dev) + i;
  return pings::host_read_words(w, 8, reinterpret_cast<uint32_t*>(record_host), pings::as_stream(stream));
}
