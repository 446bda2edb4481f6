// LiDAR frame front-end on the device, for gfx950.
//
// The block of the reference's per-frame loop that turns a raw scan and the frame's camera images into what the mapper
// trains on (dataset/slam_dataset.py:584-621, :776-784, :803-856; utils/tools.py:1088-1177, :1242-1351;
// gaussian_splatting/utils/cameras.py:233-243):
//   lidar_crop            the four strict comparisons of `crop_frame` as one byte mask
//   lidar_deskew          `deskewing`: the min / max of the time stamps as per-workgroup partials, then one apply launch
//                         whose first wave reduces the partials and forms axis and angle of every LiDAR's pose in fp64;
//                         a point is rotated with Rodrigues' formula in fp32.  No [N,3,3] tensor, no `nonzero`.
//   lidar_slerp_pose      `slerp_pose` (optionally inverted and left-multiplied) in fp64, one 64-lane launch
//   lidar_project         all points into all cameras in one launch: colours of the last camera that sees a point, the
//                         per-pixel minimum depth as an integer atomic on the complemented bit pattern of the positive
//                         float (zero = no hit, so one clear serves every camera of the frame)
//   lidar_depth_pyramid   level 0 decoded and levels 1-3 of `set_depth_img` written straight from it, all cameras in one
//                         launch ('nearest-exact' at scale 0.5 reads source index 2 i + 1)
// Plain stores apart from the one integer atomic, whose result does not depend on the order: every output is bitwise
// reproducible.  Matrices of the LiDAR rig are host values and travel in the kernel arguments.
#include "common.hpp"

namespace {

using i64 = long long;

constexpr int kMaxCams = PINGS_LIDAR_MAX_CAMS;
constexpr int kMaxLidars = PINGS_LIDAR_MAX_LIDARS;
constexpr int kMaxParts = 256;                                 // workgroups of the time-stamp range launch

inline unsigned blocks_for(i64 n) { return (unsigned)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1); }

__device__ inline double load_real(const void* p, int is_f64, int i) {
  return is_f64 ? static_cast<const double*>(p)[i] : (double)static_cast<const float*>(p)[i];
}

// ------------------------------------------------------------------ crop
__global__ __launch_bounds__(256) void crop_kernel(const float* __restrict__ pts, i64 n, i64 stride, float min_z,
                                                   float max_z, float min_r, float max_r, int on_xy,
                                                   uint8_t* __restrict__ mask) {
  const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* p = pts + i * stride;
  const float x = p[0], y = p[1], z = p[2];
  float d2 = x * x + y * y;
  if (!on_xy) d2 += z * z;
  const float dist = sqrtf(d2);
  mask[i] = (dist > min_r && dist < max_r && z > min_z && z < max_z) ? 1 : 0;   // a NaN row fails a comparison
}

// ------------------------------------------------------------------ rotation helpers (fp64)
// Axis and angle in [0, pi] of a rotation matrix through its quaternion (largest-pivot branch, so the result is well
// conditioned up to pi).  The identity gives angle 0 exactly, with the axis (1,0,0).
__device__ inline void axis_angle(const double (&R)[3][3], double (&a)[3], double& theta) {
  const double tr = R[0][0] + R[1][1] + R[2][2];
  double w, x, y, z;
  if (tr > 0.0) {
    const double s = sqrt(tr + 1.0) * 2.0;
    w = 0.25 * s; x = (R[2][1] - R[1][2]) / s; y = (R[0][2] - R[2][0]) / s; z = (R[1][0] - R[0][1]) / s;
  } else if (R[0][0] > R[1][1] && R[0][0] > R[2][2]) {
    const double s = sqrt(1.0 + R[0][0] - R[1][1] - R[2][2]) * 2.0;
    w = (R[2][1] - R[1][2]) / s; x = 0.25 * s; y = (R[0][1] + R[1][0]) / s; z = (R[0][2] + R[2][0]) / s;
  } else if (R[1][1] > R[2][2]) {
    const double s = sqrt(1.0 + R[1][1] - R[0][0] - R[2][2]) * 2.0;
    w = (R[0][2] - R[2][0]) / s; x = (R[0][1] + R[1][0]) / s; y = 0.25 * s; z = (R[1][2] + R[2][1]) / s;
  } else {
    const double s = sqrt(1.0 + R[2][2] - R[0][0] - R[1][1]) * 2.0;
    w = (R[1][0] - R[0][1]) / s; x = (R[0][2] + R[2][0]) / s; y = (R[1][2] + R[2][1]) / s; z = 0.25 * s;
  }
  if (w < 0.0) { w = -w; x = -x; y = -y; z = -z; }
  const double nv = sqrt(x * x + y * y + z * z);
  if (nv == 0.0) {
    a[0] = 1.0; a[1] = 0.0; a[2] = 0.0;
    theta = 0.0;
    return;
  }
  theta = 2.0 * atan2(nv, w);
  a[0] = x / nv; a[1] = y / nv; a[2] = z / nv;
}

// inverse of the affine map [A t] (rows 0..2 of a 4x4 whose last row is 0 0 0 1): cofactors and determinant
__device__ inline void affine_inverse(const double (&M)[12], double (&I)[12]) {
  const double a = M[0], b = M[1], c = M[2], d = M[4], e = M[5], f = M[6], g = M[8], h = M[9], k = M[10];
  const double c00 = e * k - f * h, c01 = f * g - d * k, c02 = d * h - e * g;
  const double inv = 1.0 / (a * c00 + b * c01 + c * c02);
  I[0] = c00 * inv; I[1] = (c * h - b * k) * inv; I[2] = (b * f - c * e) * inv;
  I[4] = c01 * inv; I[5] = (a * k - c * g) * inv; I[6] = (c * d - a * f) * inv;
  I[8] = c02 * inv; I[9] = (b * g - a * h) * inv; I[10] = (a * e - b * d) * inv;
#pragma unroll
  for (int r = 0; r < 3; ++r) I[4 * r + 3] = -(I[4 * r] * M[3] + I[4 * r + 1] * M[7] + I[4 * r + 2] * M[11]);
}

// ------------------------------------------------------------------ deskew
template <typename S>
__global__ __launch_bounds__(256) void ts_range_kernel(const S* __restrict__ ts, i64 n, double* __restrict__ part) {
  __shared__ double s_lo[4], s_hi[4];
  double lo = INFINITY, hi = -INFINITY;
  int nan = 0;
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
    const double v = (double)ts[i];
    nan |= v != v;
    lo = fmin(lo, v);
    hi = fmax(hi, v);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fmin(lo, __shfl_xor(lo, off, 64));
    hi = fmax(hi, __shfl_xor(hi, off, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    s_lo[threadIdx.x >> 6] = lo;
    s_hi[threadIdx.x >> 6] = hi;
  }
  const int any_nan = __syncthreads_or(nan);                   // torch.min / torch.max hand a NaN on
  if (threadIdx.x == 0) {
    lo = fmin(fmin(s_lo[0], s_lo[1]), fmin(s_lo[2], s_lo[3]));
    hi = fmax(fmax(s_hi[0], s_hi[1]), fmax(s_hi[2], s_hi[3]));
    part[2 * blockIdx.x] = any_nan ? (double)NAN : lo;
    part[2 * blockIdx.x + 1] = any_nan ? (double)NAN : hi;
  }
}

struct Slot {                  // one LiDAR of the rig, as the per-point arithmetic reads it (fp32, rounded once)
  float a[3], theta, t[3];
  float T[12], Ti[12];         // main -> this LiDAR and back; unused for slot 0
};

struct DeskewK {
  float* pts;
  i64 n, stride;
  const void* ts;
  const void* pose;            // DEVICE [4,4] row-major, T_last<-cur
  const void* lidar;           // [n] int32 / int64, or null: every row is the main LiDAR's
  const double* part;
  double ref;
  int ts_f64, pose_f64, lidar_i64, K, nparts;
  double T[kMaxLidars][12];
  double diff[kMaxLidars];
};

__global__ __launch_bounds__(256) void deskew_kernel(DeskewK k) {
  __shared__ Slot s_slot[kMaxLidars + 1];
  __shared__ double s_range[2];
  if (threadIdx.x < 64) {                                      // one-wave prelude, fp64
    const int lane = threadIdx.x;
    double lo = INFINITY, hi = -INFINITY;
    int nan = 0;
    for (int j = lane; j < k.nparts; j += 64) {
      const double a = k.part[2 * j], b = k.part[2 * j + 1];
      nan |= (a != a) || (b != b);
      lo = fmin(lo, a);
      hi = fmax(hi, b);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      lo = fmin(lo, __shfl_xor(lo, off, 64));
      hi = fmax(hi, __shfl_xor(hi, off, 64));
    }
    if (__any(nan)) lo = hi = (double)NAN;
    if (lane == 0) {
      s_range[0] = lo;
      s_range[1] = hi;
    }
    if (lane <= k.K) {                                         // lane j: pose_j = T_j . pose . T_j^-1 (j = 0: the pose)
      double P[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) P[i] = load_real(k.pose, k.pose_f64, i);
      Slot& s = s_slot[lane];
      if (lane > 0) {
        double T[12], Ti[12], Q[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) T[i] = k.T[lane - 1][i];
        affine_inverse(T, Ti);
#pragma unroll
        for (int r = 0; r < 3; ++r) {                          // Q = T . P
#pragma unroll
          for (int c = 0; c < 4; ++c)
            Q[4 * r + c] = T[4 * r] * P[c] + T[4 * r + 1] * P[4 + c] + T[4 * r + 2] * P[8 + c] + (c == 3 ? T[4 * r + 3] : 0.0);
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {                          // P = Q . Ti
#pragma unroll
          for (int c = 0; c < 4; ++c)
            P[4 * r + c] = Q[4 * r] * Ti[c] + Q[4 * r + 1] * Ti[4 + c] + Q[4 * r + 2] * Ti[8 + c] + (c == 3 ? Q[4 * r + 3] : 0.0);
        }
#pragma unroll
        for (int i = 0; i < 12; ++i) {
          s.T[i] = (float)T[i];
          s.Ti[i] = (float)Ti[i];
        }
      }
      const double R[3][3] = {{P[0], P[1], P[2]}, {P[4], P[5], P[6]}, {P[8], P[9], P[10]}};
      double a[3], theta;
      axis_angle(R, a, theta);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        s.a[i] = (float)a[i];
        s.t[i] = (float)P[4 * i + 3];
      }
      s.theta = (float)theta;
    }
  }
  __syncthreads();
  const double lo = s_range[0], span = s_range[1] - s_range[0];
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < k.n; i += (i64)gridDim.x * 256) {
    int slot = 0;
    if (k.lidar) {
      const i64 id = k.lidar_i64 ? static_cast<const i64*>(k.lidar)[i] : (i64) static_cast<const int*>(k.lidar)[i];
      if (id < 0 || id > k.K) continue;                        // a LiDAR the list does not name stays as it is
      slot = (int)id;
    }
    const double t = k.ts_f64 ? static_cast<const double*>(k.ts)[i] : (double)static_cast<const float*>(k.ts)[i];
    double sd = (t - lo) / span - k.ref;                       // max == min: 0 / 0, NaN as in the reference
    if (slot > 0) sd += k.diff[slot - 1];
    const float s = (float)sd;
    const Slot& L = s_slot[slot];
    float* p = k.pts + i * k.stride;
    float x = p[0], y = p[1], z = p[2];
    if (slot > 0) {
      const float X = ((L.T[0] * x + L.T[1] * y) + L.T[2] * z) + L.T[3];
      const float Y = ((L.T[4] * x + L.T[5] * y) + L.T[6] * z) + L.T[7];
      const float Z = ((L.T[8] * x + L.T[9] * y) + L.T[10] * z) + L.T[11];
      x = X; y = Y; z = Z;
    }
    float sn, cs;
    sincosf(s * L.theta, &sn, &cs);
    const float ax = L.a[0], ay = L.a[1], az = L.a[2];
    const float dot = (ax * x + ay * y + az * z) * (1.f - cs);
    float rx = x * cs + (ay * z - az * y) * sn + ax * dot + s * L.t[0];
    float ry = y * cs + (az * x - ax * z) * sn + ay * dot + s * L.t[1];
    float rz = z * cs + (ax * y - ay * x) * sn + az * dot + s * L.t[2];
    if (slot > 0) {
      const float X = ((L.Ti[0] * rx + L.Ti[1] * ry) + L.Ti[2] * rz) + L.Ti[3];
      const float Y = ((L.Ti[4] * rx + L.Ti[5] * ry) + L.Ti[6] * rz) + L.Ti[7];
      const float Z = ((L.Ti[8] * rx + L.Ti[9] * ry) + L.Ti[10] * rz) + L.Ti[11];
      rx = X; ry = Y; rz = Z;
    }
    p[0] = rx; p[1] = ry; p[2] = rz;
  }
}

// ------------------------------------------------------------------ slerp_pose
struct SlerpK {
  const void *pose, *left;
  void* out;
  double s;
  int pose_f64, left_f64, out_f64, invert;
};

__global__ __launch_bounds__(64) void slerp_pose_kernel(SlerpK k) {
  const int lane = threadIdx.x;
  double P[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) P[i] = load_real(k.pose, k.pose_f64, i);
  const double R[3][3] = {{P[0], P[1], P[2]}, {P[4], P[5], P[6]}, {P[8], P[9], P[10]}};
  double a[3], theta;
  axis_angle(R, a, theta);
  const double ang = k.s * theta, sn = sin(ang), cs = cos(ang), vs = 1.0 - cs;
  double M[4][4];                                              // [R(s), s t; 0 1]
  M[0][0] = cs + vs * a[0] * a[0];        M[0][1] = vs * a[0] * a[1] - sn * a[2]; M[0][2] = vs * a[0] * a[2] + sn * a[1];
  M[1][0] = vs * a[1] * a[0] + sn * a[2]; M[1][1] = cs + vs * a[1] * a[1];        M[1][2] = vs * a[1] * a[2] - sn * a[0];
  M[2][0] = vs * a[2] * a[0] - sn * a[1]; M[2][1] = vs * a[2] * a[1] + sn * a[0]; M[2][2] = cs + vs * a[2] * a[2];
#pragma unroll
  for (int r = 0; r < 3; ++r) M[r][3] = k.s * P[4 * r + 3];
  M[3][0] = M[3][1] = M[3][2] = 0.0;
  M[3][3] = 1.0;
  if (k.invert) {                                              // rigid: [R^T, -R^T t]
    double N[4][4];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) N[r][c] = M[c][r];
      N[r][3] = -(M[0][r] * M[0][3] + M[1][r] * M[1][3] + M[2][r] * M[2][3]);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) M[r][c] = N[r][c];
  }
  double v = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double e = M[r][c];
      if (k.left) {
        e = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) e += load_real(k.left, k.left_f64, 4 * r + j) * M[j][c];
      }
      if (lane == 4 * r + c) v = e;
    }
  if (lane < 16) {
    if (k.out_f64) static_cast<double*>(k.out)[lane] = v;
    else static_cast<float*>(k.out)[lane] = (float)v;
  }
}

// ------------------------------------------------------------------ projection
struct CamK {
  const float *image, *K, *T;
  uint32_t* keys;
  int H, W;
};

struct ProjectK {
  const float* pts;
  i64 n, stride;
  float* rgb;
  float* ind;
  uint8_t* vis;
  i64 rgb_stride, ind_stride;
  float min_d, max_d;
  int ncam, init;
  CamK cam[kMaxCams];
};

__global__ __launch_bounds__(256) void project_kernel(ProjectK k) {
  __shared__ float s_m[kMaxCams][21];                          // K (9) and rows 0..2 of T_c_l (12) of every camera
  for (int j = threadIdx.x; j < k.ncam * 21; j += 256) {
    const int c = j / 21, e = j % 21;
    s_m[c][e] = e < 9 ? k.cam[c].K[e] : k.cam[c].T[e - 9];
  }
  __syncthreads();
  const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
  if (i >= k.n) return;
  const float* p = k.pts + i * k.stride;
  const float x = p[0], y = p[1], z = p[2];
  int last = -1;
  i64 at = 0;
  for (int c = 0; c < k.ncam; ++c) {
    const float* Km = s_m[c];
    const float* T = s_m[c] + 9;
    const float X = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    const float Y = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    const float Z = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
    const float qx = (Km[0] * X + Km[1] * Y) + Km[2] * Z;
    const float qy = (Km[3] * X + Km[4] * Y) + Km[5] * Z;
    float d = (Km[6] * X + Km[7] * Y) + Km[8] * Z;
    if (d == 0.f) d = -1e-6f;
    const float ad = fabsf(d);
    const float u = rintf(qx / ad), v = rintf(qy / ad);        // half to even; -0 counts as pixel 0
    const int W = k.cam[c].W, H = k.cam[c].H;
    const bool seen = u >= 0.f && u < (float)W && v >= 0.f && v < (float)H && d > k.min_d && d < k.max_d;
    if (seen) {                                                // d > min_d >= 0: integer order is float order
      const i64 pix = (i64)(int)v * W + (int)u;
      atomicMax(k.cam[c].keys + pix, ~__float_as_uint(d));
      last = c;
      at = pix;
    }
  }
  if (last >= 0) {                                             // a later camera overwrites an earlier one's colour
    const float* img = k.cam[last].image;
    const i64 plane = (i64)k.cam[last].H * k.cam[last].W;
    float* o = k.rgb + i * k.rgb_stride;
    o[0] = img[at]; o[1] = img[plane + at]; o[2] = img[2 * plane + at];
    if (k.ind) k.ind[i * k.ind_stride] = 0.f;
  } else if (k.init) {
    float* o = k.rgb + i * k.rgb_stride;
    o[0] = o[1] = o[2] = -1.f;
    if (k.ind) k.ind[i * k.ind_stride] = -1.f;
  }
  if (k.vis) k.vis[i] = last >= 0 ? 1 : 0;
}

struct PyrCam {
  const uint32_t* keys;
  const float* src;
  float* level[4];
  int H, W;
};
struct PyramidK {
  PyrCam cam[kMaxCams];
};

__global__ __launch_bounds__(256) void depth_pyramid_kernel(PyramidK k) {
  const PyrCam& c = k.cam[blockIdx.y];
  const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
  if (i >= (i64)c.H * c.W) return;
  const int y = (int)(i / c.W), x = (int)(i % c.W);
  float d;
  if (c.keys) {
    const uint32_t key = c.keys[i];
    d = key ? __uint_as_float(~key) : 0.f;
  } else {
    d = c.src[i];
  }
  if (c.level[0]) c.level[0][i] = d;
#pragma unroll
  for (int l = 1; l < 4; ++l) {                                // level l reads level-0 index 2^l j + 2^l - 1
    const int m = (1 << l) - 1;
    if (c.level[l] && ((x + 1) & m) == 0 && ((y + 1) & m) == 0)
      c.level[l][(i64)(((y + 1) >> l) - 1) * (c.W >> l) + (((x + 1) >> l) - 1)] = d;
  }
}

}  // namespace

PINGS_API int pings_lidar_crop(const float* points, int64_t n, int64_t stride, double min_z, double max_z,
                               double min_range, double max_range, int32_t on_xy_plane, uint8_t* mask, void* stream) {
  PINGS_ARG_CHECK(n >= 0 && stride >= 3, "bad size");
  if (n == 0) return PINGS_OK;
  PINGS_ARG_CHECK(points && mask, "null pointer");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("lidar_crop", st);
  return pings::launch(crop_kernel, dim3(blocks_for(n)), 256, 0, st, points, (i64)n, (i64)stride, (float)min_z,
                       (float)max_z, (float)min_range, (float)max_range, (int)on_xy_plane, mask);
}

PINGS_API size_t pings_lidar_deskew_scratch_bytes(void) { return sizeof(double) * 2 * kMaxParts; }

PINGS_API int pings_lidar_deskew(float* points, int64_t n, int64_t stride, const void* ts, int32_t ts_is_f64,
                                 const void* pose, int32_t pose_is_f64, double ts_ref_pose, const void* lidar_idx,
                                 int32_t lidar_idx_is_i64, int32_t num_other, const double* T_l_lm,
                                 const double* ts_diff, void* scratch, void* stream) {
  PINGS_ARG_CHECK(n > 0 && stride >= 3, "bad size (the time stamps of an empty scan have no minimum)");
  PINGS_ARG_CHECK(points && ts && pose && scratch, "null pointer");
  PINGS_ARG_CHECK(num_other >= 0 && num_other <= kMaxLidars, "0..8 other LiDARs");
  PINGS_ARG_CHECK(num_other == 0 || (T_l_lm && lidar_idx), "null pointer (multi-LiDAR)");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("lidar_deskew", st);
  DeskewK k;
  k.pts = points;
  k.n = n;
  k.stride = stride;
  k.ts = ts;
  k.pose = pose;
  k.lidar = num_other > 0 ? lidar_idx : nullptr;
  k.part = static_cast<const double*>(scratch);
  k.ref = ts_ref_pose;
  k.ts_f64 = ts_is_f64;
  k.pose_f64 = pose_is_f64;
  k.lidar_i64 = lidar_idx_is_i64;
  k.K = num_other;
  for (int j = 0; j < kMaxLidars; ++j) {
    for (int e = 0; e < 12; ++e) k.T[j][e] = j < num_other ? T_l_lm[16 * j + e] : 0.0;
    k.diff[j] = (j < num_other && ts_diff) ? ts_diff[j] : 0.0;
  }
  const unsigned nb = blocks_for(n) < (unsigned)kMaxParts ? blocks_for(n) : (unsigned)kMaxParts;
  k.nparts = (int)nb;
  double* part = static_cast<double*>(scratch);
  if (ts_is_f64) {
    if (int e = pings::launch(ts_range_kernel<double>, dim3(nb), 256, 0, st, static_cast<const double*>(ts), (i64)n, part))
      return e;
  } else {
    if (int e = pings::launch(ts_range_kernel<float>, dim3(nb), 256, 0, st, static_cast<const float*>(ts), (i64)n, part))
      return e;
  }
  const unsigned na = blocks_for(n) < 1024u ? blocks_for(n) : 1024u;
  return pings::launch(deskew_kernel, dim3(na), 256, 0, st, k);
}

PINGS_API int pings_lidar_slerp_pose(const void* pose, int32_t pose_is_f64, double s, const void* left,
                                     int32_t left_is_f64, int32_t invert, void* out, int32_t out_is_f64, void* stream) {
  PINGS_ARG_CHECK(pose && out, "null pointer");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("lidar_slerp_pose", st);
  SlerpK k;
  k.pose = pose;
  k.left = left;
  k.out = out;
  k.s = s;
  k.pose_f64 = pose_is_f64;
  k.left_f64 = left_is_f64;
  k.out_f64 = out_is_f64;
  k.invert = invert;
  return pings::launch(slerp_pose_kernel, dim3(1), 64, 0, st, k);
}

PINGS_API int pings_lidar_project(const float* points, int64_t n, int64_t stride, const pings_lidar_cam* cams,
                                  int32_t ncam, double min_depth, double max_depth, float* rgb, int64_t rgb_stride,
                                  float* indicator, int64_t indicator_stride, uint8_t* visible, int32_t init,
                                  void* stream) {
  PINGS_ARG_CHECK(n >= 0 && stride >= 3 && rgb_stride >= 3 && indicator_stride >= 1, "bad size");
  PINGS_ARG_CHECK(ncam >= 0 && ncam <= kMaxCams, "0..8 cameras");
  PINGS_ARG_CHECK(min_depth >= 0.0, "min_depth must not be negative (the depth minimum orders bit patterns)");
  PINGS_ARG_CHECK(ncam == 0 || cams, "null pointer");
  ProjectK k;
  for (int c = 0; c < ncam; ++c) {
    PINGS_ARG_CHECK(cams[c].image && cams[c].K && cams[c].T && cams[c].keys, "null pointer in camera");
    PINGS_ARG_CHECK(cams[c].H > 0 && cams[c].W > 0 && (int64_t)cams[c].H * cams[c].W < (int64_t)0x7FFFFFF0,
                    "bad image size");
    k.cam[c] = {cams[c].image, cams[c].K, cams[c].T, cams[c].keys, cams[c].H, cams[c].W};
  }
  for (int c = ncam; c < kMaxCams; ++c) k.cam[c] = {nullptr, nullptr, nullptr, nullptr, 0, 0};
  if (n == 0) return PINGS_OK;
  PINGS_ARG_CHECK(points && rgb, "null pointer");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("lidar_project", st);
  k.pts = points;
  k.n = n;
  k.stride = stride;
  k.rgb = rgb;
  k.ind = indicator;
  k.vis = visible;
  k.rgb_stride = rgb_stride;
  k.ind_stride = indicator_stride;
  k.min_d = (float)min_depth;
  k.max_d = (float)max_depth;
  k.ncam = ncam;
  k.init = init;
  return pings::launch(project_kernel, dim3(blocks_for(n)), 256, 0, st, k);
}

PINGS_API int pings_lidar_depth_pyramid(const pings_lidar_cam* cams, int32_t ncam, void* stream) {
  PINGS_ARG_CHECK(cams && ncam > 0 && ncam <= kMaxCams, "1..8 cameras");
  PyramidK k;
  int64_t most = 0;
  for (int c = 0; c < kMaxCams; ++c) {
    if (c >= ncam) {
      k.cam[c] = {nullptr, nullptr, {nullptr, nullptr, nullptr, nullptr}, 0, 0};
      continue;
    }
    PINGS_ARG_CHECK((cams[c].keys != nullptr) != (cams[c].src != nullptr), "one of keys and src in camera");
    PINGS_ARG_CHECK(cams[c].H > 0 && cams[c].W > 0 && (int64_t)cams[c].H * cams[c].W < (int64_t)0x7FFFFFF0,
                    "bad image size");
    k.cam[c] = {cams[c].keys, cams[c].src, {cams[c].l0, cams[c].l1, cams[c].l2, cams[c].l3}, cams[c].H, cams[c].W};
    const int64_t px = (int64_t)cams[c].H * cams[c].W;
    if (px > most) most = px;
  }
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("lidar_depth_pyramid", st);
  return pings::launch(depth_pyramid_kernel, dim3(blocks_for(most), (unsigned)ncam), 256, 0, st, k);
}
