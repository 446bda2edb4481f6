// Which kernel a fused SDF query runs (host only): knn_sdf.hip, sdf_fwd_mfma.hip and sdf_bwd.hip launch what sdf_plan
// says and decide nothing themselves; pings_sdf_plan (knn_sdf.hip) answers the same question without a device.
#pragma once
#include <cstdlib>
#include <cstring>

#include "knn_host.hpp"

namespace pings_knn {

enum SdfOrder { SDF_FORWARD = 0, SDF_BACKWARD = 1, SDF_DOUBLE_BACKWARD = 2 };
enum SdfFamily { SDF_VECTOR = 0, SDF_MATRIX_CORE = 1 };   // lane = hidden unit | four queries per wave step on the MFMA
struct SdfPlan {
  SdfFamily family;
  int in_pad;   // the kernel's <IN_PAD>: padded decoder input width
};

// A pure function of the shape, the order, whether every 16-byte access is aligned (`misaligned`: the feature table;
// for the backward also its row scratch) and PINGS_SDF_FWD / PINGS_SDF_BWD = vector, read per call: the tests switch
// them in-process.
inline SdfPlan sdf_plan(int nn_k, int F, int hidden, bool weighted_first, SdfOrder order, bool misaligned) {
  const int F4 = F >> 2;
  const char* env = getenv(order == SDF_FORWARD ? "PINGS_SDF_FWD" : "PINGS_SDF_BWD");
  bool matrix = !(env && strcmp(env, "vector") == 0) && !weighted_first && nn_k <= 8 && hidden <= 64 && !misaligned &&
                (F & 3) == 0 && F4 > 0 && (F4 & (F4 - 1)) == 0;   // rows gathered 16 bytes a lane, 2^k lanes a row
  if (order == SDF_FORWARD) matrix = matrix && F + 4 <= 36;       // inputs + bias column fit the widest class built
  else matrix = matrix && F <= 32;                                // the backward stages at most 32 features
  if (order == SDF_DOUBLE_BACKWARD) matrix = false;               // the second order has no matrix-core kernel
  const int need = matrix ? F + 4 : F + 3;                        // matrix core: one more column for the bias
  SdfPlan p;
  p.family = matrix ? SDF_MATRIX_CORE : SDF_VECTOR;
  if (matrix) p.in_pad = need <= 12 ? 12 : need <= 20 ? 20 : 36;
  else if (order == SDF_FORWARD) p.in_pad = need <= 12 ? 12 : need <= 36 ? 36 : 64;
  else p.in_pad = need <= 12 ? 12 : need <= 20 ? 20 : need <= 36 ? 36 : 64;
  return p;
}

inline bool misaligned16(const void* a, const void* b = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15u) != 0;
}

// sdf_fwd_mfma.hip: the SDF_MATRIX_CORE forward of class `in_pad`
int sdf_forward_mfma_launch(int in_pad, const pings_knn_map* m, const pings_sdf_decoder* dec, const float* features,
                            const float* points, const float* orientations, const float* certainties,
                            int32_t after_pgo, const float* queries, int64_t B, float* sdf, float* grad_x,
                            int64_t* nn_counts, float* certainty, int64_t* idx_out, float* w_out, float* sdf_std,
                            int64_t* gidx_out, hipStream_t st);

}  // namespace pings_knn
