// Pose-graph optimisation on the device (the reference's utils/pgo.py is a wrapper over GTSAM).
//
// The graph PINGS builds is a chain: priors, one odometry factor per consecutive pair of frames, and a few loop
// factors.  Its normal matrix is block tridiagonal (6x6 blocks) plus U U^T with six columns per loop, so one damped
// Levenberg-Marquardt step is solved directly:
//     T = tridiagonal part + lambda diag(H)  = L L^T            one sequential block Cholesky sweep
//     [x0 Y] = T^-1 [b U]                                        one column per lane, chunks of columns
//     (I + U^T Y) y = U^T x0                                     dense Cholesky, one workgroup
//     delta = T^-1 (b - U y)                                     one more sweep
// All arithmetic is fp64 in plain C++ (the weights span 625 .. 1e18).  Every sum has a fixed order and the only atomic
// is the integer OR into the status word, so two runs agree bit for bit.  The trial is accepted or rejected by the
// device (pgo_decide_kernel); the host reads one record per trial.
#include <cmath>

#include "common.hpp"

namespace {

constexpr double kSeriesAngle = 1e-2;   // below it the trigonometric coefficients are three-term Taylor series
constexpr double kNearPi = 0.1;         // residual rotations within this of pi are out of contract
constexpr double kLambdaMax = 1e5;
#ifndef PINGS_PGO_BLOCK
#define PINGS_PGO_BLOCK 256             // threads of the reductions; 1 in a host build that runs threads one by one
#endif
constexpr int kReduce = PINGS_PGO_BLOCK;
constexpr int kDense = PINGS_PGO_BLOCK == 1 ? 1 : 1024;       // threads of the dense capacitance solve
constexpr int kDenseLanes = kDense < 64 ? kDense : 64;
constexpr int kDenseWaves = kDense / kDenseLanes;

struct Pose {
  double R[9], t[3];
};

__device__ inline Pose load_pose(const double* p) {
  Pose a;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) a.R[3 * r + c] = p[4 * r + c];
    a.t[r] = p[4 * r + 3];
  }
  return a;
}

__device__ inline void store_pose(const Pose& a, double* p) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) p[4 * r + c] = a.R[3 * r + c];
    p[4 * r + 3] = a.t[r];
  }
  p[12] = 0.0; p[13] = 0.0; p[14] = 0.0; p[15] = 1.0;
}

__device__ inline Pose inverse(const Pose& a) {
  Pose o;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) o.R[3 * r + c] = a.R[3 * c + r];
    o.t[r] = -((a.R[r] * a.t[0] + a.R[3 + r] * a.t[1]) + a.R[6 + r] * a.t[2]);
  }
  return o;
}

__device__ inline Pose mul(const Pose& a, const Pose& b) {
  Pose o;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      o.R[3 * r + c] = (a.R[3 * r] * b.R[c] + a.R[3 * r + 1] * b.R[3 + c]) + a.R[3 * r + 2] * b.R[6 + c];
    o.t[r] = ((a.R[3 * r] * b.t[0] + a.R[3 * r + 1] * b.t[1]) + a.R[3 * r + 2] * b.t[2]) + a.t[r];
  }
  return o;
}

__device__ inline void mat3_mul(const double* a, const double* b, double* o) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) o[3 * r + c] = (a[3 * r] * b[c] + a[3 * r + 1] * b[3 + c]) + a[3 * r + 2] * b[6 + c];
}

__device__ inline void skew(const double* w, double* S) {
  S[0] = 0.0;   S[1] = -w[2]; S[2] = w[1];
  S[3] = w[2];  S[4] = 0.0;   S[5] = -w[0];
  S[6] = -w[1]; S[7] = w[0];  S[8] = 0.0;
}

// k[0..5] = sin t / t, (1 - cos t) / t^2, (t - sin t) / t^3, (t^2 + 2 cos t - 2) / (2 t^4),
//           (2 t - 3 sin t + t cos t) / (2 t^5), 1 / t^2 - (1 + cos t) / (2 t sin t)
__device__ inline void coeffs(double th, double* k) {
  const double t2 = th * th;
  if (th < kSeriesAngle) {
    const double t4 = t2 * t2;
    k[0] = 1.0 - t2 / 6.0 + t4 / 120.0;
    k[1] = 0.5 - t2 / 24.0 + t4 / 720.0;
    k[2] = 1.0 / 6.0 - t2 / 120.0 + t4 / 5040.0;
    k[3] = 1.0 / 24.0 - t2 / 720.0 + t4 / 40320.0;
    k[4] = 1.0 / 120.0 - t2 / 2520.0 + t4 / 120960.0;
    k[5] = 1.0 / 12.0 + t2 / 720.0 + t4 / 30240.0;
    return;
  }
  const double s = sin(th), c = cos(th);
  k[0] = s / th;
  k[1] = (1.0 - c) / t2;
  k[2] = (th - s) / (t2 * th);
  k[3] = (t2 + 2.0 * c - 2.0) / (2.0 * t2 * t2);
  k[4] = (2.0 * th - 3.0 * s + th * c) / (2.0 * t2 * t2 * th);
  k[5] = 1.0 / t2 - (1.0 + c) / (2.0 * th * s);
}

// xi = (omega, V^-1 t); returns the rotation angle
__device__ inline double log_se3(const Pose& a, double* xi) {
  const double s[3] = {0.5 * (a.R[7] - a.R[5]), 0.5 * (a.R[2] - a.R[6]), 0.5 * (a.R[3] - a.R[1])};
  const double sn = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
  const double th = atan2(sn, 0.5 * (((a.R[0] + a.R[4]) + a.R[8]) - 1.0));
  const double t2 = th * th;
  const double kk = th < kSeriesAngle ? 1.0 + t2 / 6.0 + 7.0 * (t2 * t2) / 360.0 : th / sn;
#pragma unroll
  for (int i = 0; i < 3; ++i) xi[i] = s[i] * kk;
  double k[6], W[9], W2[9];
  coeffs(th, k);
  skew(xi, W);
  mat3_mul(W, W, W2);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    double v = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) v += (((r == c ? 1.0 : 0.0) - 0.5 * W[3 * r + c]) + k[5] * W2[3 * r + c]) * a.t[c];
    xi[3 + r] = v;
  }
  return th;
}

__device__ inline Pose exp_se3(const double* xi) {
  const double th = sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]);
  double k[6], W[9], W2[9];
  coeffs(th, k);
  skew(xi, W);
  mat3_mul(W, W, W2);
  Pose o;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    double v = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double eye = r == c ? 1.0 : 0.0;
      o.R[3 * r + c] = (eye + k[0] * W[3 * r + c]) + k[1] * W2[3 * r + c];
      v += ((eye + k[1] * W[3 * r + c]) + k[2] * W2[3 * r + c]) * xi[3 + c];
    }
    o.t[r] = v;
  }
  return o;
}

// d Log(T Exp(d)) / d d at T = Exp(xi): [[A, 0], [-A Q A, A]], the left Jacobian's blocks at -xi.  A and B = -A Q A.
__device__ inline void dlog_blocks(const double* xi, double* A, double* B) {
  const double th = sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]);
  double k[6];
  coeffs(th, k);
  const double nw[3] = {-xi[0], -xi[1], -xi[2]}, nv[3] = {-xi[3], -xi[4], -xi[5]};
  double W[9], V[9], W2[9], WV[9], VW[9], WVW[9], WWV[9], VWW[9], WVWW[9], WWVW[9], Q[9], QA[9];
  skew(nw, W);
  skew(nv, V);
  mat3_mul(W, W, W2);
  mat3_mul(W, V, WV);
  mat3_mul(V, W, VW);
  mat3_mul(WV, W, WVW);
  mat3_mul(W, WV, WWV);
  mat3_mul(VW, W, VWW);
  mat3_mul(WVW, W, WVWW);
  mat3_mul(W, WVW, WWVW);
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    const double eye = (e == 0 || e == 4 || e == 8) ? 1.0 : 0.0;
    A[e] = (eye - 0.5 * W[e]) + k[5] * W2[e];
    Q[e] = ((0.5 * V[e] + k[2] * ((WV[e] + VW[e]) + WVW[e])) + k[3] * ((WWV[e] + VWW[e]) - 3.0 * WVW[e])) +
           k[4] * (WVWW[e] + WWVW[e]);
  }
  mat3_mul(Q, A, QA);
  mat3_mul(A, QA, B);
#pragma unroll
  for (int e = 0; e < 9; ++e) B[e] = -B[e];
}

// ---------------------------------------------------------------- linearise: one factor per thread
template <bool kJac>
__global__ __launch_bounds__(64) void pgo_linearise_kernel(const double* __restrict__ X, const int32_t* __restrict__ fi,
                                                           const int32_t* __restrict__ fj, const double* __restrict__ Z,
                                                           const double* __restrict__ Wm, long long F,
                                                           double* __restrict__ res, double* __restrict__ jac,
                                                           double* __restrict__ costf, int32_t* status) {
  const long long f = (long long)blockIdx.x * 64 + threadIdx.x;
  if (f >= F) return;
  const int i = fi[f], j = fj[f];
  Pose h = load_pose(X + 16 * (long long)i);
  if (j >= 0) h = mul(inverse(h), load_pose(X + 16 * (long long)j));
  const Pose e = mul(inverse(load_pose(Z + 16 * f)), h);
  double xi[6];
  const double th = log_se3(e, xi);
  const double* W = Wm + 36 * f;
  double r[6], cost = 0.0;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    double v = 0.0;
#pragma unroll
    for (int b = 0; b < 6; ++b) v += W[6 * a + b] * xi[b];
    r[a] = v;
    cost += v * v;
  }
  cost *= 0.5;
  costf[f] = cost;
  int bits = 0;
  if (th > M_PI - kNearPi) bits |= PINGS_PGO_ST_NEAR_PI;
  if (!(fabs(cost) <= 1.7e308)) bits |= PINGS_PGO_ST_NONFINITE;
  if (bits) atomicOr(status, bits);
  if (!kJac) return;
#pragma unroll
  for (int a = 0; a < 6; ++a) res[6 * f + a] = r[a];
  double A[9], B[9];
  dlog_blocks(xi, A, B);
  double Jj[36];                                       // W [[A, 0], [B, A]]
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double lo = 0.0, hi = 0.0;
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        lo += W[6 * a + b] * A[3 * b + c];
        hi += W[6 * a + 3 + b] * A[3 * b + c];
      }
#pragma unroll
      for (int b = 0; b < 3; ++b) lo += W[6 * a + 3 + b] * B[3 * b + c];
      Jj[6 * a + c] = lo;
      Jj[6 * a + 3 + c] = hi;
    }
  double* out = jac + 72 * f;
  if (j < 0) {                                         // a prior: its one Jacobian sits in slot 0
#pragma unroll
    for (int e2 = 0; e2 < 36; ++e2) {
      out[e2] = Jj[e2];
      out[36 + e2] = 0.0;
    }
    return;
  }
  // J_i = -J_j Ad(h^-1),  Ad(T) = [[R, 0], [[t]x R, R]]
  const Pose hi = inverse(h);
  double S[9], SR[9];
  skew(hi.t, S);
  mat3_mul(S, hi.R, SR);
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double lo = 0.0, up = 0.0;
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        lo += Jj[6 * a + b] * hi.R[3 * b + c];
        up += Jj[6 * a + 3 + b] * hi.R[3 * b + c];
      }
#pragma unroll
      for (int b = 0; b < 3; ++b) lo += Jj[6 * a + 3 + b] * SR[3 * b + c];
      out[6 * a + c] = -lo;
      out[6 * a + 3 + c] = -up;
    }
#pragma unroll
  for (int e2 = 0; e2 < 36; ++e2) out[36 + e2] = Jj[e2];
}

// sum of v[0..n) by one workgroup in a fixed order: strided partial sums, then a tree through LDS
__device__ inline double block_sum(const double* __restrict__ v, long long n) {
  __shared__ double part[kReduce];
  double s = 0.0;
  for (long long i = threadIdx.x; i < n; i += kReduce) s += v[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int w = kReduce / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  return part[0];
}

__global__ __launch_bounds__(kReduce) void pgo_cost_kernel(const double* __restrict__ costf, long long F, double* out) {
  const double s = block_sum(costf, F);
  if (threadIdx.x == 0) *out = s;
}

// ---------------------------------------------------------------- assemble: one (node, row) per thread
struct Lists {
  const int32_t *fi, *fj, *kind, *lcol, *node_off, *node_ent;
};

__global__ __launch_bounds__(64) void pgo_assemble_kernel(Lists g, long long N, const double* __restrict__ res,
                                                          const double* __restrict__ jac, double* __restrict__ D,
                                                          double* __restrict__ E, double* __restrict__ grad,
                                                          double* __restrict__ hdiag) {
  const long long tid = (long long)blockIdx.x * 64 + threadIdx.x;
  if (tid >= N * 6) return;
  const long long n = tid / 6;
  const int r = (int)(tid - n * 6);
  double d[6] = {0, 0, 0, 0, 0, 0}, sub[6] = {0, 0, 0, 0, 0, 0}, gr = 0.0, hd = 0.0;
  for (int e = g.node_off[n]; e < g.node_off[n + 1]; ++e) {
    const int ent = g.node_ent[e];
    const long long f = ent >> 1;
    const int slot = ent & 1;
    const double* J = jac + 72 * f + 36 * slot;
    const double* rr = res + 6 * f;
    double jr[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) jr[k] = J[6 * k + r];
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      a += jr[k] * rr[k];
      b += jr[k] * jr[k];
    }
    gr += a;
    hd += b;
    const int kind = g.kind[f];
    if (kind == PINGS_PGO_LOOP) continue;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) v += jr[k] * J[6 * k + c];
      d[c] += v;
    }
    if (kind != PINGS_PGO_CHAIN) continue;
    const long long other = slot ? g.fi[f] : g.fj[f];
    if (other != n + 1) continue;
    const double* Jo = jac + 72 * f + 36 * (1 - slot);  // E_n = H[n+1][n] = sum J_{n+1}^T J_n
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) v += Jo[6 * k + r] * J[6 * k + c];
      sub[c] += v;
    }
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    D[36 * n + 6 * r + c] = d[c];
    E[36 * n + 6 * r + c] = sub[c];
  }
  grad[tid] = gr;
  hdiag[tid] = hd;
}

// ---------------------------------------------------------------- block-tridiagonal Cholesky: a sequential sweep
// T_nn = D_n + lambda diag(hdiag_n), T_{n+1,n} = E_n.  Lf[n]: the lower triangle of L_nn with 1 / L_cc on the diagonal;
// M[n] = E_n L_nn^-T.  One lane walks the chain: every block depends on the one before it.  A lone wave issues one
// fp64 instruction at a time, so the sweep's time is its instruction count: the inner products are fused (fma).
__global__ __launch_bounds__(64) void pgo_factor_kernel(long long N, const double* __restrict__ D,
                                                        const double* __restrict__ E, const double* __restrict__ hdiag,
                                                        const double* __restrict__ state, double* __restrict__ Lf,
                                                        double* __restrict__ M, int32_t* status) {
  if (threadIdx.x != 0) return;
  const double lam = state[0];
  double Mp[36];
  bool bad = false;
  for (long long n = 0; n < N; ++n) {
    double A[36], inv[6];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c <= r; ++c) {
        double v = D[36 * n + 6 * r + c];
        if (r == c) v += lam * hdiag[6 * n + r];
        if (n > 0) {
          double s = 0.0;
#pragma unroll
          for (int k = 0; k < 6; ++k) s = fma(Mp[6 * r + k], Mp[6 * c + k], s);
          v -= s;
        }
        A[6 * r + c] = v;
      }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double s = A[6 * c + c];
#pragma unroll
      for (int k = 0; k < c; ++k) s = fma(-A[6 * c + k], A[6 * c + k], s);
      if (!(s > 0.0) || !(s <= 1.7e308)) {
        bad = true;
        s = 1.0;
      }
      const double dd = sqrt(s);
      inv[c] = 1.0 / dd;
      A[6 * c + c] = dd;
#pragma unroll
      for (int r = c + 1; r < 6; ++r) {
        double v = A[6 * r + c];
#pragma unroll
        for (int k = 0; k < c; ++k) v = fma(-A[6 * r + k], A[6 * c + k], v);
        A[6 * r + c] = v * inv[c];
      }
    }
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) Lf[36 * n + 6 * r + c] = c < r ? A[6 * r + c] : (c == r ? inv[r] : 0.0);
    if (n + 1 < N) {
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          double v = E[36 * n + 6 * i + c];
#pragma unroll
          for (int k = 0; k < c; ++k) v = fma(-Mp[6 * i + k], A[6 * c + k], v);
          Mp[6 * i + c] = v * inv[c];
        }
#pragma unroll
      for (int e = 0; e < 36; ++e) M[36 * n + e] = Mp[e];
    }
  }
  if (bad) atomicOr(status, PINGS_PGO_ST_NOT_POSDEF);
}

// ---------------------------------------------------------------- right-hand sides [N][6][cw]
// column c0 + col of the system: 0 is b = -grad, 1 + 6 l + k is column k of loop l's block of U
__global__ __launch_bounds__(256) void pgo_rhs_fill_kernel(long long N, int cw, int c0, const double* __restrict__ grad,
                                                           double* __restrict__ rhs) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= N * 6 * cw) return;
  const long long row = idx / cw;
  const int col = (int)(idx - row * cw);
  rhs[idx] = (c0 + col == 0) ? -grad[row] : 0.0;
}

__global__ __launch_bounds__(64) void pgo_rhs_loops_kernel(Lists g, const int32_t* __restrict__ loop_f, long long L,
                                                           int cw, int c0, int nc, const double* __restrict__ jac,
                                                           double* __restrict__ rhs) {
  const long long tid = (long long)blockIdx.x * 64 + threadIdx.x;
  if (tid >= L * 72) return;
  const long long l = tid / 72;
  const int q = (int)(tid - l * 72), slot = q / 36, k = (q % 36) / 6, rr = q % 6;
  const long long col = 1 + 6 * l + k - c0;
  if (col < 0 || col >= nc) return;
  const long long f = loop_f[l];
  const long long node = slot ? g.fj[f] : g.fi[f];
  rhs[(node * 6 + rr) * cw + col] = jac[72 * f + 36 * slot + 6 * k + rr];
}

// ---------------------------------------------------------------- sweeps: one column per lane, in place
// The factor blocks are read at addresses the whole wave shares; a step is about 80 fused multiply-adds per lane.
__global__ __launch_bounds__(64) void pgo_sweep_kernel(long long N, const double* __restrict__ Lf,
                                                       const double* __restrict__ M, double* __restrict__ rhs, int cw,
                                                       int nc) {
  const int col = blockIdx.x * 64 + threadIdx.x;
  if (col >= nc) return;
  double p[6] = {0, 0, 0, 0, 0, 0};
  for (long long n = 0; n < N; ++n) {                  // L y = b
    const double* Ln = Lf + 36 * n;
    double b[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) b[k] = rhs[(n * 6 + k) * cw + col];
    if (n > 0) {
      const double* Mn = M + 36 * (n - 1);
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) s = fma(Mn[6 * r + c], p[c], s);
        b[r] -= s;
      }
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      double v = b[r];
#pragma unroll
      for (int c = 0; c < r; ++c) v = fma(-Ln[6 * r + c], p[c], v);
      p[r] = v * Ln[6 * r + r];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) rhs[(n * 6 + k) * cw + col] = p[k];
  }
  for (long long n = N - 1; n >= 0; --n) {             // L^T x = y
    const double* Ln = Lf + 36 * n;
    double b[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) b[k] = rhs[(n * 6 + k) * cw + col];
    if (n + 1 < N) {
      const double* Mn = M + 36 * n;
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) s = fma(Mn[6 * r + c], p[r], s);
        b[c] -= s;
      }
    }
#pragma unroll
    for (int r = 5; r >= 0; --r) {
      double v = b[r];
#pragma unroll
      for (int c = r + 1; c < 6; ++c) v = fma(-Ln[6 * c + r], b[c], v);
      b[r] = v * Ln[6 * r + r];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      p[k] = b[k];
      rhs[(n * 6 + k) * cw + col] = b[k];
    }
  }
}

// ---------------------------------------------------------------- capacitance: cap [6L][1 + 6L] = [U^T x0 | I + U^T Y]
__global__ __launch_bounds__(64) void pgo_capacitance_kernel(Lists g, const int32_t* __restrict__ loop_f, long long L,
                                                             int cw, int c0, int nc, const double* __restrict__ jac,
                                                             const double* __restrict__ rhs, double* __restrict__ cap) {
  const int col = blockIdx.x * 64 + threadIdx.x;
  const long long p = blockIdx.y;                      // row of U^T: 6 l + k
  if (col >= nc) return;
  const long long l = p / 6;
  const int k = (int)(p - l * 6);
  const long long f = loop_f[l];
  const long long ni = g.fi[f], nj = g.fj[f];
  const double* Ji = jac + 72 * f + 6 * k;
  const double* Jj = Ji + 36;
  double s = 0.0;
#pragma unroll
  for (int rr = 0; rr < 6; ++rr) s += Ji[rr] * rhs[(ni * 6 + rr) * cw + col];
#pragma unroll
  for (int rr = 0; rr < 6; ++rr) s += Jj[rr] * rhs[(nj * 6 + rr) * cw + col];
  const long long gcol = (long long)c0 + col;
  if (gcol == p + 1) s += 1.0;
  cap[p * (6 * L + 1) + gcol] = s;
}

// dense Cholesky of the lower triangle of C (cap's columns 1 ..) and the solve C y = cap's column 0, one workgroup.
// Right-looking: column k is scaled and copied to y (contiguous), then every wave updates whole rows of the trailing
// triangle from it.  y is the answer at the end.
__global__ __launch_bounds__(kDense) void pgo_dense_solve_kernel(int m, double* __restrict__ cap, double* __restrict__ y,
                                                               int32_t* status) {
  const int ld = m + 1, tid = threadIdx.x, lane = tid % kDenseLanes, wave = tid / kDenseLanes;
  double* C = cap + 1;
  bool bad = false;
  for (int k = 0; k < m; ++k) {
    __syncthreads();
    double d = C[(long long)k * ld + k];
    if (!(d > 0.0) || !(d <= 1.7e308)) {
      bad = true;
      d = 1.0;
    }
    const double sd = sqrt(d);
    __syncthreads();
    if (tid == 0) C[(long long)k * ld + k] = sd;
    for (int r = k + 1 + tid; r < m; r += kDense) {
      const double v = C[(long long)r * ld + k] / sd;
      C[(long long)r * ld + k] = v;
      y[r] = v;
    }
    __syncthreads();
    for (int r = k + 1 + wave; r < m; r += kDenseWaves) {
      const double lrk = y[r];
      for (int c = k + 1 + lane; c <= r; c += kDenseLanes) C[(long long)r * ld + c] -= lrk * y[c];
    }
  }
  for (int k = 0; k < m; ++k) {                        // L z = q
    __syncthreads();
    const double zk = cap[(long long)k * ld] / C[(long long)k * ld + k];
    __syncthreads();
    if (tid == 0) cap[(long long)k * ld] = zk;
    for (int r = k + 1 + tid; r < m; r += kDense) cap[(long long)r * ld] -= C[(long long)r * ld + k] * zk;
  }
  for (int k = m - 1; k >= 0; --k) {                   // L^T y = z
    __syncthreads();
    const double yk = cap[(long long)k * ld] / C[(long long)k * ld + k];
    __syncthreads();
    if (tid == 0) cap[(long long)k * ld] = yk;
    for (int r = tid; r < k; r += kDense) cap[(long long)r * ld] -= C[(long long)k * ld + r] * yk;
  }
  __syncthreads();
  for (int r = tid; r < m; r += kDense) y[r] = cap[(long long)r * ld];
  if (bad && tid == 0) atomicOr(status, PINGS_PGO_ST_NOT_POSDEF);
}

// the last right-hand side b - U y, [N][6][1]
__global__ __launch_bounds__(64) void pgo_rhs_final_kernel(Lists g, long long N, const double* __restrict__ grad,
                                                           const double* __restrict__ jac, const double* __restrict__ y,
                                                           double* __restrict__ rhs) {
  const long long tid = (long long)blockIdx.x * 64 + threadIdx.x;
  if (tid >= N * 6) return;
  const long long n = tid / 6;
  const int r = (int)(tid - n * 6);
  double v = -grad[tid];
  for (int e = g.node_off[n]; e < g.node_off[n + 1]; ++e) {
    const int ent = g.node_ent[e];
    const long long f = ent >> 1;
    if (g.kind[f] != PINGS_PGO_LOOP) continue;
    const double* J = jac + 72 * f + 36 * (ent & 1);
    const double* yl = y + 6 * (long long)g.lcol[f];
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) s += J[6 * k + r] * yl[k];
    v -= s;
  }
  rhs[tid] = v;
}

// ---------------------------------------------------------------- step
__global__ __launch_bounds__(64) void pgo_retract_kernel(long long N, const double* __restrict__ X,
                                                         const double* __restrict__ delta, double* __restrict__ cand,
                                                         int32_t* status) {
  const long long n = (long long)blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  double xi[6], a = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    xi[k] = delta[6 * n + k];
    a += fabs(xi[k]);
  }
  if (!(a <= 1.7e308)) atomicOr(status, PINGS_PGO_ST_NONFINITE);
  store_pose(mul(load_pose(X + 16 * n), exp_se3(xi)), cand + 16 * n);
}

// state: 0 lambda, 1 cost before, 2 cost after, 3 accepted
__global__ __launch_bounds__(kReduce) void pgo_decide_kernel(const double* __restrict__ costf, long long F,
                                                             double* state, double* record, int32_t* status,
                                                             int iteration, double rel_tol) {
  const double after = block_sum(costf, F);
  if (threadIdx.x != 0) return;
  const double before = state[1], lam = state[0];
  const bool accepted = after <= before;               // false for a NaN
  int st = *status;
  if (!(fabs(after) <= 1.7e308)) st |= PINGS_PGO_ST_NONFINITE;
  double next = lam;
  if (accepted) {
    next = lam / 10.0;
    if (before - after <= rel_tol * before) st |= PINGS_PGO_ST_CONVERGED;
  } else {
    next = lam * 10.0;
    if (next > kLambdaMax) st |= PINGS_PGO_ST_LAMBDA_MAX;
  }
  *status = st;
  state[0] = next;
  state[2] = after;
  state[3] = accepted ? 1.0 : 0.0;
  record[0] = before;
  record[1] = after;
  record[2] = lam;
  record[3] = accepted ? 1.0 : 0.0;
  record[4] = (double)st;
  record[5] = (double)iteration;
  record[6] = 0.0;
  record[7] = 0.0;
}

__global__ __launch_bounds__(256) void pgo_commit_kernel(long long count, const double* __restrict__ state,
                                                         const double* __restrict__ cand, double* __restrict__ X) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < count && state[3] != 0.0) X[i] = cand[i];
}

__global__ __launch_bounds__(64) void pgo_pose_diff_kernel(long long N, const double* __restrict__ after,
                                                           const double* __restrict__ before, double* out64,
                                                           float* out32) {
  const long long n = (long long)blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  double m[16];
  store_pose(mul(load_pose(after + 16 * n), inverse(load_pose(before + 16 * n))), m);
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    if (out64) out64[16 * n + e] = m[e];
    if (out32) out32[16 * n + e] = (float)m[e];
  }
}

// ---------------------------------------------------------------- host
struct Scratch {
  double *cand, *res, *jac, *costf, *D, *E, *grad, *hdiag, *Lf, *M, *rhs, *cap, *y;
  size_t total;
};

Scratch carve(void* base, int64_t N, int64_t F, int64_t L, int32_t chunk) {
  pings::Carver c(base);
  const size_t n = (size_t)N, f = F > 0 ? (size_t)F : 1, m = (size_t)(6 * L);
  const size_t cols = 1 + m, cw = cols < (size_t)chunk ? cols : (size_t)chunk;
  Scratch s;
  s.cand = c.take<double>(n * 16);
  s.res = c.take<double>(f * 6);
  s.jac = c.take<double>(f * 72);
  s.costf = c.take<double>(f);
  s.D = c.take<double>(n * 36);
  s.E = c.take<double>(n * 36);
  s.grad = c.take<double>(n * 6);
  s.hdiag = c.take<double>(n * 6);
  s.Lf = c.take<double>(n * 36);
  s.M = c.take<double>(n * 36);
  s.rhs = c.take<double>(n * 6 * (L > 0 ? cw : 1));
  s.cap = c.take<double>(m > 0 ? m * (m + 1) : 1);
  s.y = c.take<double>(m > 0 ? m : 1);
  s.total = c.total();
  return s;
}

int check_args(const pings_pgo_args* a) {
  PINGS_ARG_CHECK(a != nullptr, "null pointer");
  PINGS_ARG_CHECK(a->n_nodes >= 1 && a->n_nodes < (1ll << 26), "1 <= n_nodes < 2^26");
  PINGS_ARG_CHECK(a->n_factors >= 1 && a->n_factors < (1ll << 26), "1 <= n_factors < 2^26");
  PINGS_ARG_CHECK(a->n_loops >= 0 && a->n_loops <= a->n_factors && a->n_loops < 5000, "0 <= n_loops < 5000");
  PINGS_ARG_CHECK(a->chunk >= 64 && a->chunk % 64 == 0 && a->chunk <= 4096, "chunk: a multiple of 64 up to 4096");
  PINGS_ARG_CHECK(a->fi && a->fj && a->Z && a->W && a->scratch && a->status, "null pointer");
  return PINGS_OK;
}

int blocks(long long n, int per) { return (int)((n + per - 1) / per); }

template <bool kJac>
int linearise(const pings_pgo_args* a, const Scratch& s, const double* X, hipStream_t st) {
  return pings::launch(pgo_linearise_kernel<kJac>, dim3(blocks(a->n_factors, 64)), 64, 0, st, X, a->fi, a->fj, a->Z,
                       a->W, (long long)a->n_factors, s.res, s.jac, s.costf, a->status);
}

}  // namespace

PINGS_API size_t pings_pgo_scratch_bytes(int64_t n_nodes, int64_t n_factors, int64_t n_loops, int32_t chunk) {
  if (n_nodes < 1 || n_factors < 0 || n_loops < 0 || chunk < 64) return 0;
  return carve(nullptr, n_nodes, n_factors, n_loops, chunk).total;
}

PINGS_API int pings_pgo_cost(const pings_pgo_args* a, const double* poses, double* out_cost, void* stream) {
  if (int e = check_args(a)) return e;
  PINGS_ARG_CHECK(poses && out_cost, "null pointer");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("pgo_cost", st);
  const Scratch s = carve(a->scratch, a->n_nodes, a->n_factors, a->n_loops, a->chunk);
  if (int e = linearise<false>(a, s, poses, st)) return e;
  return pings::launch(pgo_cost_kernel, dim3(1), kReduce, 0, st, (const double*)s.costf, (long long)a->n_factors,
                       out_cost);
}

PINGS_API int pings_pgo_iteration(const pings_pgo_args* a, void* stream) {
  if (int e = check_args(a)) return e;
  PINGS_ARG_CHECK(a->X && a->state && a->record && a->kind && a->lcol && a->node_off && a->node_ent, "null pointer");
  PINGS_ARG_CHECK(a->n_loops == 0 || a->loop_f, "loops without loop_f");
  hipStream_t st = pings::as_stream(stream);
  const long long N = a->n_nodes, F = a->n_factors, L = a->n_loops;
  const Scratch s = carve(a->scratch, N, F, L, a->chunk);
  const Lists g{a->fi, a->fj, a->kind, a->lcol, a->node_off, a->node_ent};
  const int cols = (int)(1 + 6 * L), cw = cols < a->chunk ? cols : a->chunk;
  {
    pings::prof::Scope ps("pgo_linearise", st);
    if (int e = linearise<true>(a, s, a->X, st)) return e;
    if (int e = pings::launch(pgo_cost_kernel, dim3(1), kReduce, 0, st, (const double*)s.costf, F, a->state + 1))
      return e;
    if (int e = pings::launch(pgo_assemble_kernel, dim3(blocks(N * 6, 64)), 64, 0, st, g, N, (const double*)s.res,
                              (const double*)s.jac, s.D, s.E, s.grad, s.hdiag))
      return e;
  }
  {
    pings::prof::Scope ps("pgo_factor", st);
    if (int e = pings::launch(pgo_factor_kernel, dim3(1), 64, 0, st, N, (const double*)s.D, (const double*)s.E,
                              (const double*)s.hdiag, (const double*)a->state, s.Lf, s.M, a->status))
      return e;
  }
  if (L > 0) {
    for (int c0 = 0; c0 < cols; c0 += cw) {
      const int nc = cols - c0 < cw ? cols - c0 : cw;
      {
        pings::prof::Scope ps("pgo_sweeps", st);
        if (int e = pings::launch(pgo_rhs_fill_kernel, dim3(blocks(N * 6 * cw, 256)), 256, 0, st, N, cw, c0,
                                  (const double*)s.grad, s.rhs))
          return e;
        if (int e = pings::launch(pgo_rhs_loops_kernel, dim3(blocks(L * 72, 64)), 64, 0, st, g, a->loop_f, L, cw, c0,
                                  nc, (const double*)s.jac, s.rhs))
          return e;
        if (int e = pings::launch(pgo_sweep_kernel, dim3(blocks(nc, 64)), 64, 0, st, N, (const double*)s.Lf,
                                  (const double*)s.M, s.rhs, cw, nc))
          return e;
      }
      pings::prof::Scope ps("pgo_capacitance", st);
      if (int e = pings::launch(pgo_capacitance_kernel, dim3(blocks(nc, 64), (unsigned)(6 * L)), 64, 0, st, g,
                                a->loop_f, L, cw, c0, nc, (const double*)s.jac, (const double*)s.rhs, s.cap))
        return e;
    }
    pings::prof::Scope ps("pgo_capacitance", st);
    if (int e = pings::launch(pgo_dense_solve_kernel, dim3(1), kDense, 0, st, (int)(6 * L), s.cap, s.y, a->status))
      return e;
  }
  {
    pings::prof::Scope ps("pgo_sweeps", st);
    if (int e = pings::launch(pgo_rhs_final_kernel, dim3(blocks(N * 6, 64)), 64, 0, st, g, N, (const double*)s.grad,
                              (const double*)s.jac, (const double*)s.y, s.rhs))
      return e;
    if (int e = pings::launch(pgo_sweep_kernel, dim3(1), 64, 0, st, N, (const double*)s.Lf, (const double*)s.M, s.rhs,
                              1, 1))
      return e;
  }
  pings::prof::Scope ps("pgo_step", st);
  if (int e = pings::launch(pgo_retract_kernel, dim3(blocks(N, 64)), 64, 0, st, N, (const double*)a->X,
                            (const double*)s.rhs, s.cand, a->status))
    return e;
  if (int e = linearise<false>(a, s, s.cand, st)) return e;
  if (int e = pings::launch(pgo_decide_kernel, dim3(1), kReduce, 0, st, (const double*)s.costf, F, a->state, a->record,
                            a->status, (int)a->iteration, a->rel_tol))
    return e;
  return pings::launch(pgo_commit_kernel, dim3(blocks(N * 16, 256)), 256, 0, st, N * 16, (const double*)a->state,
                       (const double*)s.cand, a->X);
}

PINGS_API int pings_pgo_read_record(const double* record_dev, double* record_host, void* stream) {
  PINGS_ARG_CHECK(record_dev && record_host, "null pointer");
  const uint32_t* src = reinterpret_cast<const uint32_t*>(record_dev);
  uint32_t* dst = reinterpret_cast<uint32_t*>(record_host);
  for (int half = 0; half < 2; ++half) {               // 8 doubles = two polled reads of 8 words, one wait for the data
    const uint32_t* w[8];
    for (int i = 0; i < 8; ++i) w[i] = src + 8 * half + i;
    if (int e = pings::host_read_words(w, 8, dst + 8 * half, pings::as_stream(stream))) return e;
  }
  return PINGS_OK;
}

PINGS_API int pings_pgo_pose_diff(const double* after, const double* before, int64_t n, double* out64, float* out32,
                                  void* stream) {
  PINGS_ARG_CHECK(n >= 0 && (out64 || out32), "bad argument");
  if (n == 0) return PINGS_OK;
  PINGS_ARG_CHECK(after && before, "null pointer");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("pgo_pose_diff", st);
  return pings::launch(pgo_pose_diff_kernel, dim3(blocks(n, 64)), 64, 0, st, (long long)n, after, before, out64, out32);
}
