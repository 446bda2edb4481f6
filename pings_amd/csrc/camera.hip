// Camera pose on the device (utils/campose_utils.py:28-98, gaussian_splatting/utils/cameras.py:207-219).
//
// The reference's `update_pose` is three dozen flops spread over dozens of launches on 3x3 / 4x4 tensors and six host
// waits (two `angle < 1e-5` branches, `tau_norm == 0`, three `linalg.inv` status reads); `set_pose` makes two of the
// inversions.  Here each is ONE launch of one 64-lane workgroup: every lane evaluates the same fp64 arithmetic from
// the fp32 inputs (read through element strides, so the transposed views a `CamImage` holds need no copy launch) and
// lane i stores the i-th word of the output block.  Each output is rounded to fp32 once.  Plain stores, no LDS, no
// atomics.
//
// Output block (fp32 words):  [0,16) world_view_transform = T_cw^T   [16,32) full_proj_transform = wvt(fp32) . P
//                             [32,35) camera_center   35 unused   36 |tau|   37 converged (uint32 0 / 1)
#include "common.hpp"

namespace {

constexpr int CAM_WVT = 0, CAM_FPT = 16, CAM_CENTER = 32, CAM_NORM = 36, CAM_FLAG = 37;

struct View2 {
  const float* p;
  long long s0, s1;
  __device__ double at(int r, int c) const { return (double)p[r * s0 + c * s1]; }
  __device__ float raw(int r, int c) const { return p[r * s0 + c * s1]; }
};

// lane `lane` stores word `lane` of the first 35 words: wvt and center given in fp64, fpt from the ROUNDED wvt
__device__ inline void store_block(const double (&Tcw)[4][4], const double (&center)[3], const View2& P, float* out,
                                   int lane) {
  float w[4][4];                                       // world_view_transform = T_cw^T, rounded once
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) w[r][c] = (float)Tcw[c][r];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) acc += (double)w[r][k] * P.at(k, c);
      if (lane == CAM_WVT + 4 * r + c) out[lane] = w[r][c];
      if (lane == CAM_FPT + 4 * r + c) out[lane] = (float)acc;
    }
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (lane == CAM_CENTER + k) out[lane] = (float)center[k];
  if (lane == CAM_CENTER + 3) out[lane] = 0.f;
}

struct UpdateArgs {
  View2 R, P, wvt, fpt;
  const float *T, *center;
  long long T_s, center_s;
  float *trans_delta, *rot_delta, *out;
  double threshold;
};

__global__ __launch_bounds__(64) void camera_update_pose_kernel(UpdateArgs a) {
  const int lane = threadIdx.x;
  double rho[3], th[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    rho[k] = (double)a.trans_delta[k];
    th[k] = (double)a.rot_delta[k];
  }
  const double angle2 = th[0] * th[0] + th[1] * th[1] + th[2] * th[2];
  const double norm = sqrt(rho[0] * rho[0] + rho[1] * rho[1] + rho[2] * rho[2] + angle2);
  float* out = a.out;
  if (norm == 0.0) {                                   // pose optimisation off: the reference touches nothing
    if (lane < 16) out[CAM_WVT + lane] = a.wvt.raw(lane >> 2, lane & 3);
    else if (lane < 32) out[lane] = a.fpt.raw((lane - 16) >> 2, lane & 3);
    else if (lane < 35) out[lane] = a.center[(lane - 32) * a.center_s];
    else if (lane == 35) out[lane] = 0.f;
    else if (lane == CAM_NORM) out[lane] = 0.f;
    else if (lane == CAM_FLAG) reinterpret_cast<uint32_t*>(out)[lane] = 1u;
    return;
  }
  const double angle = sqrt(angle2);
  // W = skew(theta), W2 = W W
  const double W[3][3] = {{0.0, -th[2], th[1]}, {th[2], 0.0, -th[0]}, {-th[1], th[0], 0.0}};
  double W2[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) W2[r][c] = W[r][0] * W[0][c] + W[r][1] * W[1][c] + W[r][2] * W[2][c];
  double ra, rb, va, vb;                               // R = I + ra W + rb W2,  V = I + va W + vb W2
  if (angle < 1e-5) {
    ra = 1.0; rb = 0.5; va = 0.5; vb = 1.0 / 6.0;
  } else {
    const double s = sin(angle), c = cos(angle);
    ra = s / angle;
    rb = (1.0 - c) / angle2;
    va = rb;
    vb = (angle - s) / (angle2 * angle);
  }
  double E[3][4];                                      // SE3_exp(tau), rows 0..2
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    double t = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double eye = r == c ? 1.0 : 0.0;
      E[r][c] = eye + ra * W[r][c] + rb * W2[r][c];
      t += (eye + va * W[r][c] + vb * W2[r][c]) * rho[c];
    }
    E[r][3] = t;
  }
  double Tcw[4][4];                                    // SE3_exp(tau) . [R T; 0 1]
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      Tcw[r][c] = E[r][0] * a.R.at(0, c) + E[r][1] * a.R.at(1, c) + E[r][2] * a.R.at(2, c);
    Tcw[r][3] = E[r][0] * (double)a.T[0] + E[r][1] * (double)a.T[a.T_s] + E[r][2] * (double)a.T[2 * a.T_s] + E[r][3];
  }
  Tcw[3][0] = Tcw[3][1] = Tcw[3][2] = 0.0;
  Tcw[3][3] = 1.0;
  double center[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) center[k] = -(Tcw[0][k] * Tcw[0][3] + Tcw[1][k] * Tcw[1][3] + Tcw[2][k] * Tcw[2][3]);
  store_block(Tcw, center, a.P, out, lane);
  if (lane == 35) out[lane] = 0.f;
  if (lane == CAM_NORM) out[lane] = (float)norm;
  if (lane == CAM_FLAG) reinterpret_cast<uint32_t*>(out)[lane] = norm < a.threshold ? 1u : 0u;
  if (lane >= 40 && lane < 43) a.trans_delta[lane - 40] = 0.f;
  if (lane >= 43 && lane < 46) a.rot_delta[lane - 43] = 0.f;
}

template <typename S>
__global__ __launch_bounds__(64) void camera_set_pose_kernel(const S* __restrict__ Twc, long long s0, long long s1,
                                                             View2 P, float* __restrict__ out) {
  const int lane = threadIdx.x;
  double m[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) m[r][c] = (double)Twc[r * s0 + c * s1];
  // general inverse: 2x2 minors of the upper and the lower row pair, cofactors, determinant
  const double s_0 = m[0][0] * m[1][1] - m[1][0] * m[0][1], s_1 = m[0][0] * m[1][2] - m[1][0] * m[0][2];
  const double s_2 = m[0][0] * m[1][3] - m[1][0] * m[0][3], s_3 = m[0][1] * m[1][2] - m[1][1] * m[0][2];
  const double s_4 = m[0][1] * m[1][3] - m[1][1] * m[0][3], s_5 = m[0][2] * m[1][3] - m[1][2] * m[0][3];
  const double c_5 = m[2][2] * m[3][3] - m[3][2] * m[2][3], c_4 = m[2][1] * m[3][3] - m[3][1] * m[2][3];
  const double c_3 = m[2][1] * m[3][2] - m[3][1] * m[2][2], c_2 = m[2][0] * m[3][3] - m[3][0] * m[2][3];
  const double c_1 = m[2][0] * m[3][2] - m[3][0] * m[2][2], c_0 = m[2][0] * m[3][1] - m[3][0] * m[2][1];
  const double det = s_0 * c_5 - s_1 * c_4 + s_2 * c_3 + s_3 * c_2 - s_4 * c_1 + s_5 * c_0;
  const double inv = 1.0 / det;                        // singular input: non-finite outputs, no exception
  double Tcw[4][4];
  Tcw[0][0] = (m[1][1] * c_5 - m[1][2] * c_4 + m[1][3] * c_3) * inv;
  Tcw[0][1] = (-m[0][1] * c_5 + m[0][2] * c_4 - m[0][3] * c_3) * inv;
  Tcw[0][2] = (m[3][1] * s_5 - m[3][2] * s_4 + m[3][3] * s_3) * inv;
  Tcw[0][3] = (-m[2][1] * s_5 + m[2][2] * s_4 - m[2][3] * s_3) * inv;
  Tcw[1][0] = (-m[1][0] * c_5 + m[1][2] * c_2 - m[1][3] * c_1) * inv;
  Tcw[1][1] = (m[0][0] * c_5 - m[0][2] * c_2 + m[0][3] * c_1) * inv;
  Tcw[1][2] = (-m[3][0] * s_5 + m[3][2] * s_2 - m[3][3] * s_1) * inv;
  Tcw[1][3] = (m[2][0] * s_5 - m[2][2] * s_2 + m[2][3] * s_1) * inv;
  Tcw[2][0] = (m[1][0] * c_4 - m[1][1] * c_2 + m[1][3] * c_0) * inv;
  Tcw[2][1] = (-m[0][0] * c_4 + m[0][1] * c_2 - m[0][3] * c_0) * inv;
  Tcw[2][2] = (m[3][0] * s_4 - m[3][1] * s_2 + m[3][3] * s_0) * inv;
  Tcw[2][3] = (-m[2][0] * s_4 + m[2][1] * s_2 - m[2][3] * s_0) * inv;
  Tcw[3][0] = (-m[1][0] * c_3 + m[1][1] * c_1 - m[1][2] * c_0) * inv;
  Tcw[3][1] = (m[0][0] * c_3 - m[0][1] * c_1 + m[0][2] * c_0) * inv;
  Tcw[3][2] = (-m[3][0] * s_3 + m[3][1] * s_1 - m[3][2] * s_0) * inv;
  Tcw[3][3] = (m[2][0] * s_3 - m[2][1] * s_1 + m[2][2] * s_0) * inv;
  const double center[3] = {m[0][3], m[1][3], m[2][3]};
  store_block(Tcw, center, P, out, lane);
  if (lane >= 35 && lane < 38) out[lane] = 0.f;       // the record is unused here
}

}  // namespace

PINGS_API int pings_camera_update_pose(const pings_camera_pose_args* args, void* stream) {
  PINGS_ARG_CHECK(args != nullptr, "null pointer");
  PINGS_ARG_CHECK(args->R && args->T && args->projection_matrix && args->world_view_transform &&
                      args->full_proj_transform && args->camera_center && args->cam_trans_delta &&
                      args->cam_rot_delta && args->out,
                  "null pointer");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("camera_update_pose", st);
  UpdateArgs a;
  a.R = {args->R, args->R_s0, args->R_s1};
  a.P = {args->projection_matrix, args->proj_s0, args->proj_s1};
  a.wvt = {args->world_view_transform, args->wvt_s0, args->wvt_s1};
  a.fpt = {args->full_proj_transform, args->fpt_s0, args->fpt_s1};
  a.T = args->T;
  a.T_s = args->T_s;
  a.center = args->camera_center;
  a.center_s = args->center_s;
  a.trans_delta = args->cam_trans_delta;
  a.rot_delta = args->cam_rot_delta;
  a.out = args->out;
  a.threshold = (double)args->converged_threshold;
  return pings::launch(camera_update_pose_kernel, dim3(1), 64, 0, st, a);
}

PINGS_API int pings_camera_set_pose(const void* T_wc, int is_f64, int64_t s0, int64_t s1,
                                    const float* projection_matrix, int64_t proj_s0, int64_t proj_s1, float* out,
                                    void* stream) {
  PINGS_ARG_CHECK(T_wc && projection_matrix && out, "null pointer");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("camera_set_pose", st);
  const View2 P{projection_matrix, proj_s0, proj_s1};
  if (is_f64)
    return pings::launch(camera_set_pose_kernel<double>, dim3(1), 64, 0, st, static_cast<const double*>(T_wc),
                         (long long)s0, (long long)s1, P, out);
  return pings::launch(camera_set_pose_kernel<float>, dim3(1), 64, 0, st, static_cast<const float*>(T_wc),
                       (long long)s0, (long long)s1, P, out);
}
