// Loop-closure context (utils/loop_detector.py of the reference) on the device: descriptors of M poses from one pass
// over the cloud, the ring-key search and the sector-shift search with no host step between them.
//
//   bin_kernel        a thread per (pose, point): transform, ring / sector, max z by an INTEGER atomicMax on an
//                     order-preserving key of the fp32 bits (order of arrival cannot matter); destination row for the
//                     feature sums
//   pings_rows        the project's deterministic scatter-add (row_scatter.hpp): feature sums in ascending point index
//   finalize_kernel   a workgroup per pose: decode the maxima (an untouched bin is 0.0), sums -> means, ring keys as the
//                     mean over the sectors in ascending sector
//   ringkey_kernel    one workgroup: every (query, candidate) ring-key distance, winner = lexicographic minimum of
//                     (distance, query, position in cand) -- the reference's first-wins rules -- into the record
//   shift_kernel      one workgroup: reads the winner from the record, S shifted column-wise cosine means, first maximum
//
// No float atomics, no fixed point; every sum has a fixed order, so two runs agree bit for bit.
#include <cfloat>
#include <climits>

#include "common.hpp"
#include "row_scatter.hpp"

namespace {

constexpr int kMaxR = PINGS_LOOP_MAX_R, kMaxS = PINGS_LOOP_MAX_S, kMaxD = PINGS_LOOP_MAX_D, kMaxQ = PINGS_LOOP_MAX_Q;
constexpr int kMaxC = PINGS_LOOP_MAX_C;
constexpr int kSearchThreads = 1024;
constexpr float kCosEps = 1e-8f;     // F.cosine_similarity's eps

// fp32 -> uint32 whose unsigned order is the order of the floats; 0 is taken by no finite value (= an empty bin)
__device__ __forceinline__ uint32_t order_key(float z) {
  const uint32_t b = __float_as_uint(z);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float order_value(uint32_t k) {
  if (k == 0u) return 0.0f;
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

__global__ __launch_bounds__(256) void bin_kernel(const float* __restrict__ pts, long long N,
                                                  const float* __restrict__ T, int R, int S, float max_len,
                                                  float gap_ring, float gap_sector, uint32_t rows,
                                                  uint32_t* __restrict__ zkey, uint32_t* __restrict__ keys,
                                                  uint32_t* __restrict__ src_row) {
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int m = blockIdx.y;
  const float* t = T + 12 * m;
  const float x = pts[3 * n], y = pts[3 * n + 1], z = pts[3 * n + 2];
  const float px = t[0] * x + t[1] * y + t[2] * z + t[3];
  const float py = t[4] * x + t[5] * y + t[6] * z + t[7];
  const float pz = t[8] * x + t[9] * y + t[10] * z + t[11];
  const float r = sqrtf(px * px + py * py + pz * pz);
  const bool kept = r < max_len;                    // false for NaN and inf rows
  uint32_t row = rows;
  if (kept) {
    const float deg = atan2f(py, px) * 180.0f / 3.14159265358979323846f + 180.0f;
    int ring = (int)floorf(r / gap_ring), sector = (int)floorf(deg / gap_sector);
    ring = min(max(ring, 0), R - 1);
    sector = min(max(sector, 0), S - 1);
    row = (uint32_t)m * (uint32_t)(R * S) + (uint32_t)(ring * S + sector);
    const uint32_t k = order_key(pz);
    if (zkey[row] < k) atomicMax(&zkey[row], k);    // the word only grows: a stale read costs an atomic, never a value
  }
  if (keys) {
    const long long p = (long long)m * N + n;
    keys[p] = row;
    src_row[p] = (uint32_t)n;
  }
}

__global__ __launch_bounds__(256) void finalize_kernel(const uint32_t* __restrict__ zkey,
                                                       const uint32_t* __restrict__ offset, int R, int S, int D,
                                                       float* __restrict__ sc, float* __restrict__ rk,
                                                       float* __restrict__ scf, float* __restrict__ rkf,
                                                       const int32_t* __restrict__ use_stored,
                                                       const float* __restrict__ st_sc, const float* __restrict__ st_rk,
                                                       const float* __restrict__ st_scf,
                                                       const float* __restrict__ st_rkf) {
  const int m = blockIdx.x, RS = R * S;
  const bool stored = use_stored && use_stored[m] != 0;
  if (stored) {   // this pose takes the node's stored descriptor (utils/loop_detector.py:135-139)
    for (int b = threadIdx.x; b < RS; b += 256) sc[(size_t)m * RS + b] = st_sc[b];
    for (int b = threadIdx.x; b < R; b += 256) rk[(size_t)m * R + b] = st_rk[b];
    if (D > 0) {
      for (int b = threadIdx.x; b < RS * D; b += 256) scf[(size_t)m * RS * D + b] = st_scf[b];
      for (int b = threadIdx.x; b < R * D; b += 256) rkf[(size_t)m * R * D + b] = st_rkf[b];
    }
    return;
  }
  for (int b = threadIdx.x; b < RS; b += 256) {
    const size_t row = (size_t)m * RS + b;
    sc[row] = order_value(zkey[row]);
    if (D > 0) {
      const uint32_t cnt = offset[row + 1] - offset[row];
      if (cnt > 0u) {
        const float c = (float)cnt;
        for (int d = 0; d < D; ++d) scf[row * D + d] = scf[row * D + d] / c;
      }
    }
  }
  __syncthreads();
  for (int r = threadIdx.x; r < R; r += 256) {
    float a = 0.f;
    for (int s = 0; s < S; ++s) a += sc[(size_t)m * RS + r * S + s];
    rk[(size_t)m * R + r] = a / (float)S;
  }
  for (int i = threadIdx.x; i < R * D; i += 256) {
    const int r = i / D, d = i % D;
    float a = 0.f;
    for (int s = 0; s < S; ++s) a += scf[((size_t)m * RS + r * S + s) * D + d];
    rkf[(size_t)m * R * D + i] = a / (float)S;
  }
}

__global__ __launch_bounds__(256) void ring_key_kernel(const float* __restrict__ sc, int R, int S, int Dd,
                                                       float* __restrict__ rk) {
  for (int i = threadIdx.x; i < R * Dd; i += 256) {
    const int r = i / Dd, d = i % Dd;
    float a = 0.f;
    for (int s = 0; s < S; ++s) a += sc[((size_t)r * S + s) * Dd + d];
    rk[i] = a / (float)S;
  }
}

// One thread per virtual pose k: utils/loop_detector.py:84-133 with the reference's precisions (direction and offsets in
// fp32, poses in fp64).  inv(frame_pose @ inv(T_k)) in closed form for a pose whose last row is (0, 0, 0, 1).
__global__ __launch_bounds__(64) void poses_kernel(const double* __restrict__ F, const double* __restrict__ L, int side,
                                                   float step, float* __restrict__ transforms,
                                                   double* __restrict__ tran_from_frame, float* __restrict__ lat_tran,
                                                   int32_t* __restrict__ use_stored) {
  const int k = threadIdx.x, M = 2 * side + 1;
  if (k >= M) return;
  float lx = 0.f, ly = 1.f, lz = 0.f;
  if (L) {
    const double dx = F[3] - L[3], dy = F[7] - L[7], dz = F[11] - L[11];
    const double nrm = sqrt(dx * dx + dy * dy + dz * dz);
    const float ux = (float)(dx / nrm), uy = (float)(dy / nrm), uz = (float)(dz / nrm);   // 0 / 0 = NaN, as there
    lx = 0.f * ux + -1.f * uy + 0.f * uz;
    ly = 1.f * ux + 0.f * uy + 0.f * uz;
    lz = 0.f * ux + 0.f * uy + 1.f * uz;
  }
  const float d = (float)(k - side) * step;
  const float tx = d * lx, ty = d * ly, tz = d * lz;
  lat_tran[3 * k] = tx, lat_tran[3 * k + 1] = ty, lat_tran[3 * k + 2] = tz;
  use_stored[k] = sqrtf(tx * tx + ty * ty + tz * tz) == 0.f ? 1 : 0;   // `torch.norm(cur_lat_tran) == 0`
  double* E = tran_from_frame + 16 * k;
  for (int i = 0; i < 16; ++i) E[i] = (i % 5 == 0) ? 1.0 : 0.0;
  E[3] = (double)tx, E[7] = (double)ty, E[11] = (double)tz;
  // V = F @ inv(T_k): rotation A of F, translation t - A lat
  const double a00 = F[0], a01 = F[1], a02 = F[2], a10 = F[4], a11 = F[5], a12 = F[6], a20 = F[8], a21 = F[9],
               a22 = F[10];
  const double vx = F[3] - (a00 * tx + a01 * ty + a02 * tz), vy = F[7] - (a10 * tx + a11 * ty + a12 * tz),
               vz = F[11] - (a20 * tx + a21 * ty + a22 * tz);
  const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
  const double det = a00 * c00 + a01 * c01 + a02 * c02;
  const double i00 = c00 / det, i01 = (a02 * a21 - a01 * a22) / det, i02 = (a01 * a12 - a02 * a11) / det;
  const double i10 = c01 / det, i11 = (a00 * a22 - a02 * a20) / det, i12 = (a02 * a10 - a00 * a12) / det;
  const double i20 = c02 / det, i21 = (a01 * a20 - a00 * a21) / det, i22 = (a00 * a11 - a01 * a10) / det;
  float* o = transforms + 12 * k;
  o[0] = (float)i00, o[1] = (float)i01, o[2] = (float)i02, o[3] = (float)-(i00 * vx + i01 * vy + i02 * vz);
  o[4] = (float)i10, o[5] = (float)i11, o[6] = (float)i12, o[7] = (float)-(i10 * vx + i11 * vy + i12 * vz);
  o[8] = (float)i20, o[9] = (float)i21, o[10] = (float)i22, o[11] = (float)-(i20 * vx + i21 * vy + i22 * vz);
}

__device__ __forceinline__ bool better(float d, int q, int c, float bd, int bq, int bc) {
  return d < bd || (d == bd && (q < bq || (q == bq && c < bc)));
}

// LDS: Q * len query keys, then 3 * kSearchThreads words of the reduction.
__global__ __launch_bounds__(kSearchThreads) void ringkey_kernel(const float* __restrict__ bank_key, int len,
                                                                 long long capacity, const int32_t* __restrict__ cand,
                                                                 int C, const float* __restrict__ qkey, int Q,
                                                                 int use_feature, double thre,
                                                                 int32_t* __restrict__ record) {
  extern __shared__ float lds[];
  float* qk = lds;
  float* red_d = lds + Q * len;
  int* red_q = reinterpret_cast<int*>(red_d + kSearchThreads);
  int* red_c = red_q + kSearchThreads;
  const int tid = threadIdx.x;
  for (int i = tid; i < Q * len; i += kSearchThreads) qk[i] = qkey[i];
  __syncthreads();
  float best_d = FLT_MAX;
  int best_q = INT_MAX, best_c = INT_MAX;
  for (int c = tid; c < C; c += kSearchThreads) {
    const long long slot = cand[c];
    if (slot < 0 || slot >= capacity) continue;     // never read outside the bank
    const float* key = bank_key + (size_t)slot * len;
    float acc[kMaxQ], qn[kMaxQ];
#pragma unroll
    for (int q = 0; q < kMaxQ; ++q) acc[q] = 0.f, qn[q] = 0.f;
    float cn = 0.f;
    for (int i = 0; i < len; ++i) {
      const float v = key[i];
      cn = fmaf(v, v, cn);
#pragma unroll
      for (int q = 0; q < kMaxQ; ++q)
        if (q < Q) {
          const float u = qk[q * len + i];
          if (use_feature) {
            acc[q] = fmaf(u, v, acc[q]);
            qn[q] = fmaf(u, u, qn[q]);
          } else {
            acc[q] += fabsf(u - v);
          }
        }
    }
#pragma unroll
    for (int q = 0; q < kMaxQ; ++q)
      if (q < Q) {
        float d = acc[q];
        if (use_feature) d = 1.0f - acc[q] / (fmaxf(sqrtf(qn[q]), kCosEps) * fmaxf(sqrtf(cn), kCosEps));
        if (better(d, q, c, best_d, best_q, best_c)) best_d = d, best_q = q, best_c = c;
      }
  }
  red_d[tid] = best_d, red_q[tid] = best_q, red_c[tid] = best_c;
  __syncthreads();
  for (int w = kSearchThreads / 2; w > 0; w >>= 1) {
    if (tid < w && better(red_d[tid + w], red_q[tid + w], red_c[tid + w], red_d[tid], red_q[tid], red_c[tid]))
      red_d[tid] = red_d[tid + w], red_q[tid] = red_q[tid + w], red_c[tid] = red_c[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    const bool found = red_c[0] != INT_MAX && red_d[0] < 1e5f;     // `min_dist_ringkey = 1e5` (:237)
    record[0] = found ? red_c[0] : -1;
    record[1] = found ? red_q[0] : 0;
    record[2] = __float_as_int(found ? red_d[0] : 1e5f);
    record[5] = (found && !((double)red_d[0] > thre)) ? 1 : 0;
  }
}

// LDS: column norms of both descriptors (2 * S * Dd) and the S means.  direct: A = bank, B = qctx as given.
__global__ __launch_bounds__(kSearchThreads) void shift_kernel(const float* __restrict__ bank, int R, int S, int Dd,
                                                               const int32_t* __restrict__ cand,
                                                               const float* __restrict__ qctx, int direct,
                                                               const float* __restrict__ query_tran,
                                                               int32_t* __restrict__ record,
                                                               float* __restrict__ win_tran) {
  extern __shared__ float lds[];
  const int ncol = S * Dd, tid = threadIdx.x;
  const float *A = bank, *B = qctx;
  if (!direct) {
    if (record[5] == 0) return;     // the ring-key gate is closed: fields 3 and 4 stay as they are
    const size_t len = (size_t)R * ncol;
    A = bank + (size_t)cand[record[0]] * len;
    B = qctx + (size_t)record[1] * len;
    if (tid < 3 && query_tran && win_tran) win_tran[tid] = query_tran[3 * record[1] + tid];
  }
  float* na = lds;
  float* nb = lds + ncol;
  float* sim = nb + ncol;
  for (int col = tid; col < ncol; col += kSearchThreads) {
    float sa = 0.f, sb = 0.f;
    for (int r = 0; r < R; ++r) {
      const float a = A[(size_t)r * ncol + col], b = B[(size_t)r * ncol + col];
      sa = fmaf(a, a, sa);
      sb = fmaf(b, b, sb);
    }
    na[col] = fmaxf(sqrtf(sa), kCosEps);
    nb[col] = fmaxf(sqrtf(sb), kCosEps);
  }
  __syncthreads();
  const int wave = tid / pings::kWave, lane = tid % pings::kWave, nwaves = kSearchThreads / pings::kWave;
  for (int i = wave + 1; i <= S; i += nwaves) {     // shift i: column (s, d) of the rolled A is column (s - i, d) of A
    float acc = 0.f;
    for (int col = lane; col < ncol; col += pings::kWave) {
      const int s = col / Dd, d = col - s * Dd;
      const int cola = ((s + S - i) % S) * Dd + d;
      float dot = 0.f;
      for (int r = 0; r < R; ++r) dot = fmaf(A[(size_t)r * ncol + cola], B[(size_t)r * ncol + col], dot);
      acc += dot / (na[cola] * nb[col]);
    }
    for (int o = pings::kWave / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) sim[i - 1] = acc / (float)ncol;
  }
  __syncthreads();
  if (tid == 0) {
    float best = sim[0];
    int arg = 0;
    for (int i = 1; i < S; ++i)
      if (sim[i] > best) best = sim[i], arg = i;     // first maximum: the smallest shift wins a tie
    record[3] = __float_as_int(1.0f - best);
    record[4] = arg + 1;
  }
}

bool shape_ok(int R, int S, int D) { return R >= 1 && R <= kMaxR && S >= 1 && S <= kMaxS && D >= 0 && D <= kMaxD; }

struct ContextScratch {
  uint32_t* zkey;              // [rows] largest height key per bin
  uint32_t *keys, *src_row;    // [pairs] bin and point of every (point, pose) pair; with features only
  pings_rows::Plan plan;       // the feature sums by bin; with features only
  size_t total;
};
ContextScratch carve_context(void* base, int64_t rows, int64_t pairs, bool features) {
  pings::Carver c(base);
  ContextScratch s{};
  s.zkey = c.take<uint32_t>((size_t)rows);
  if (features) {
    const size_t n = (size_t)(pairs > 0 ? pairs : 1);
    s.keys = c.take<uint32_t>(n);
    s.src_row = c.take<uint32_t>(n);
    char* plan = c.take<char>(pings_rows::carve(nullptr, pairs, rows).total);
    s.plan = pings_rows::carve(plan, pairs, rows);
  }
  s.total = c.total();
  return s;
}

}  // namespace

PINGS_API size_t pings_loop_context_scratch_bytes(int64_t n_points, int32_t M, int32_t R, int32_t S, int32_t D) {
  if (n_points < 0 || M < 1 || M > kMaxQ || !shape_ok(R, S, D) || n_points * M >= 0x7FFFFFF0LL) return 0;
  return carve_context(nullptr, (int64_t)M * R * S, n_points * M, D > 0).total;
}

PINGS_API int pings_loop_context_build(const float* points, int64_t n_points, const float* features, int32_t D,
                                       const float* transforms, int32_t M, int32_t R, int32_t S, double max_length,
                                       const int32_t* use_stored, const float* stored_sc, const float* stored_ringkey,
                                       const float* stored_sc_feat, const float* stored_ringkey_feat, void* scratch,
                                       float* sc, float* ringkey, float* sc_feat, float* ringkey_feat, void* stream) {
  PINGS_ARG_CHECK(M >= 1 && M <= kMaxQ && shape_ok(R, S, D), "shape outside the limits (PINGS_LOOP_MAX_*)");
  PINGS_ARG_CHECK(n_points >= 0 && n_points * M < 0x7FFFFFF0LL && max_length > 0.0, "bad point count or max_length");
  PINGS_ARG_CHECK(transforms && scratch && sc && ringkey && (n_points == 0 || points), "null pointer");
  PINGS_ARG_CHECK(D == 0 || (sc_feat && ringkey_feat && (n_points == 0 || features)), "null pointer (features)");
  PINGS_ARG_CHECK(!use_stored || (stored_sc && stored_ringkey && (D == 0 || (stored_sc_feat && stored_ringkey_feat))),
                  "null pointer (stored descriptor)");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("loop_context_build", st);
  const int64_t rows = (int64_t)M * R * S, pairs = n_points * M;
  const ContextScratch s = carve_context(scratch, rows, pairs, D > 0);
  uint32_t *zkey = s.zkey, *keys = s.keys, *src_row = s.src_row;
  const pings_rows::Plan& plan = s.plan;
  PINGS_HIP_CHECK(hipMemsetAsync(zkey, 0, (size_t)rows * 4, st));
  if (n_points > 0) {
    const dim3 grid((unsigned)((n_points + 255) / 256), (unsigned)M);
    if (int e = pings::launch(bin_kernel, grid, 256, 0, st, points, (long long)n_points, transforms, (int)R, (int)S,
                              (float)max_length, (float)(max_length / R), (float)(360.0 / S), (uint32_t)rows, zkey,
                              keys, src_row))
      return e;
  }
  if (D > 0) {
    if (int e = pings_rows::build(plan, keys, pairs, rows, st)) return e;
    if (int e = pings_rows::gather_sum(plan, rows, D, features, D, src_row, nullptr, sc_feat, st)) return e;
  }
  return pings::launch(finalize_kernel, dim3((unsigned)M), 256, 0, st, (const uint32_t*)zkey,
                       (const uint32_t*)plan.offset, (int)R, (int)S, (int)D, sc, ringkey, sc_feat, ringkey_feat,
                       use_stored, stored_sc, stored_ringkey, stored_sc_feat, stored_ringkey_feat);
}

PINGS_API int pings_loop_ring_key(const float* sc, int32_t R, int32_t S, int32_t D, float* ringkey, void* stream) {
  PINGS_ARG_CHECK(shape_ok(R, S, D), "shape outside the limits (PINGS_LOOP_MAX_*)");
  PINGS_ARG_CHECK(sc && ringkey, "null pointer");
  return pings::launch(ring_key_kernel, dim3(1), 256, 0, pings::as_stream(stream), sc, (int)R, (int)S,
                       (int)(D > 0 ? D : 1), ringkey);
}

PINGS_API int pings_loop_virtual_poses(const double* frame_pose, const double* last_frame_pose, int32_t side_count,
                                       double step_m, float* transforms, double* tran_from_frame, float* lat_tran,
                                       int32_t* use_stored, void* stream) {
  PINGS_ARG_CHECK(side_count >= 0 && 2 * side_count + 1 <= kMaxQ, "side count outside the limits (PINGS_LOOP_MAX_Q)");
  PINGS_ARG_CHECK(frame_pose && transforms && tran_from_frame && lat_tran && use_stored, "null pointer");
  return pings::launch(poses_kernel, dim3(1), 64, 0, pings::as_stream(stream), frame_pose, last_frame_pose,
                       (int)side_count, (float)step_m, transforms, tran_from_frame, lat_tran, use_stored);
}

PINGS_API int pings_loop_search(const float* bank_context, const float* bank_ringkey, int64_t capacity,
                                const int32_t* cand, int32_t C, const float* query_context, const float* query_ringkey,
                                int32_t Q, int32_t R, int32_t S, int32_t D, int32_t use_feature, double ringkey_thre,
                                const float* query_tran, int32_t* record, float* win_tran, void* stream) {
  PINGS_ARG_CHECK(shape_ok(R, S, D) && Q >= 1 && Q <= kMaxQ && C >= 1 && C <= kMaxC && capacity >= 1,
                  "shape outside the limits (PINGS_LOOP_MAX_*)");
  PINGS_ARG_CHECK(!use_feature || D >= 1, "use_feature needs D >= 1");
  PINGS_ARG_CHECK(bank_context && bank_ringkey && cand && query_context && query_ringkey && record, "null pointer");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("loop_search", st);
  const int Dd = use_feature ? D : 1, len = R * Dd;
  const size_t lds1 = ((size_t)Q * len + 3 * kSearchThreads) * 4, lds2 = ((size_t)2 * S * Dd + S) * 4;
  if (int e = pings::launch(ringkey_kernel, dim3(1), kSearchThreads, lds1, st, bank_ringkey, len, (long long)capacity,
                            cand, (int)C, query_ringkey, (int)Q, (int)use_feature, ringkey_thre, record))
    return e;
  return pings::launch(shift_kernel, dim3(1), kSearchThreads, lds2, st, bank_context, (int)R, (int)S, Dd, cand,
                       query_context, 0, query_tran, record, win_tran);
}

PINGS_API int pings_loop_context_distance(const float* sc1, const float* sc2, int32_t R, int32_t S, int32_t D,
                                          int32_t* record, void* stream) {
  PINGS_ARG_CHECK(shape_ok(R, S, D), "shape outside the limits (PINGS_LOOP_MAX_*)");
  PINGS_ARG_CHECK(sc1 && sc2 && record, "null pointer");
  const int Dd = D > 0 ? D : 1;
  return pings::launch(shift_kernel, dim3(1), kSearchThreads, ((size_t)2 * S * Dd + S) * 4, pings::as_stream(stream),
                       sc1, (int)R, (int)S, Dd, (const int32_t*)nullptr, sc2, 1, (const float*)nullptr, record,
                       (float*)nullptr);
}

PINGS_API int pings_loop_read_record(const int32_t* record_dev, const float* win_tran_dev, int32_t* record_host,
                                     void* stream) {
  PINGS_ARG_CHECK(record_dev && record_host, "null pointer");
  const uint32_t* w[8];
  for (int i = 0; i < 8; ++i) w[i] = reinterpret_cast<const uint32_t*>(record_dev) + i;
  if (win_tran_dev)
    for (int i = 0; i < 3; ++i) w[5 + i] = reinterpret_cast<const uint32_t*>(win_tran_dev) + i;
  return pings::host_read_words(w, 8, reinterpret_cast<uint32_t*>(record_host), pings::as_stream(stream));
}
