// Decoder MLP  y = relu(x W1^T + b1) W2^T + b2  on the gfx950 matrix cores, forward and backward.
//
// fp32 in / fp32 accumulate (v_mfma_f32_32x32x2_f32): bitwise an fp32 fma chain, so the 1e-4 parity
// bound of the reference's fp32 decoders (model/decoder.py:62-82) holds without mixed precision.
//
// Work decomposition: a workgroup has NW = HID/32 waves and walks 32-row tiles of x; wave w owns
// hidden units 32w .. 32w+31 for ALL products, so every matrix it needs from the previous product is
// already in its accumulators:
//   GEMM1 (transposed)  H^T[hid, row]  = W1[hid, :] . x[row, :]^T        A = W1 (LDS), B = x tile (LDS)
//   GEMM2               Y^T[o, row]   += W2[o, hid] . H^T[hid, row]      B = the GEMM1 accumulator itself
//                       (accumulator-as-operand: the 32x32 C tile has its column on the lane and its rows
//                        in the 16 registers, which IS the B-operand layout when k runs over the tile's
//                        rows in the order (s&3) + 8(s>>2) + 4(lane>>5); the A operand is read from LDS
//                        in that same k order)
//   backward            gH^T = (W2^T gY^T) * relu'(H^T) ;  gX^T += W1^T gH^T (B = the gH^T accumulator);
//                       gW2^T[hid,o] += H^T gY and gW1[hid,i] += gH^T x sum over ROWS, i.e. over the
//                       accumulators' lane index, so H^T and gH^T take one trip through LDS (transposed
//                       read) — the only transposes in the kernel.
// Partial Y^T / gX^T tiles of the NW waves are summed through LDS in fixed order; weight gradients are
// kept in registers across all row tiles of the workgroup, written as per-workgroup partials and summed
// by a second kernel in fixed order (bitwise reproducible, no atomics).
#include "mlp_common.hpp"

using namespace pings::mlp;

namespace {

__global__ void mlp_reduce_kernel(const float* __restrict__ partials, int nblocks, size_t per_block, int IN,
                                  int HID, int OUT, float* __restrict__ gW1, float* __restrict__ gb1,
                                  float* __restrict__ gW2, float* __restrict__ gb2) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= per_block) return;
  // eight independent accumulation chains (fixed assignment -> still deterministic) keep loads in flight
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int b = 0;
  for (; b + 8 <= nblocks; b += 8) {
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] += partials[(size_t)(b + u) * per_block + e];
  }
  for (; b < nblocks; ++b) a[0] += partials[(size_t)b * per_block + e];
  const float s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  const size_t nW1 = (size_t)HID * IN, nW2 = (size_t)OUT * HID;
  if (e < nW1) gW1[e] = s;
  else if (e < nW1 + nW2) gW2[e - nW1] = s;
  else if (e < nW1 + nW2 + HID) gb1[e - nW1 - nW2] = s;
  else gb2[e - nW1 - nW2 - HID] = s;
}

__global__ void mlp_reduce_grouped_kernel(MlpJobs j, int HID) {
  const int g = blockIdx.y;
  const int nblocks = j.wg0[g + 1] - j.wg0[g];
  const size_t per_block = j.per_block[g];
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= per_block) return;
  const float* partials = j.partials[g];
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int b = 0;
  for (; b + 8 <= nblocks; b += 8) {
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] += partials[(size_t)(b + u) * per_block + e];
  }
  for (; b < nblocks; ++b) a[0] += partials[(size_t)b * per_block + e];
  const float s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  const size_t nW1 = (size_t)HID * j.IN[g], nW2 = (size_t)j.OUT[g] * HID;
  if (e < nW1) j.gW1[g][e] = s;
  else if (e < nW1 + nW2) j.gW2[g][e - nW1] = s;
  else if (e < nW1 + nW2 + HID) j.gb1[g][e - nW1 - nW2] = s;
  else j.gb2[g][e - nW1 - nW2 - HID] = s;
}

int check_dims(int64_t N, int IN, int HID, int OUT) {
  PINGS_ARG_CHECK(N >= 0, "negative N");
  PINGS_ARG_CHECK(IN > 0 && IN <= MAX_INP, "IN must be in 1..64");
  PINGS_ARG_CHECK(HID > 0 && HID <= 128 && HID % 32 == 0, "HID must be 32, 64, 96 or 128");
  PINGS_ARG_CHECK(OUT > 0 && OUT <= OUTP, "OUT must be in 1..32");
  return PINGS_OK;
}

// Sums a launch's per-workgroup partials in fixed order into the four weight gradients.
int launch_reduce(hipStream_t st, const float* partials, int nblocks, size_t per_block, int IN, int HID, int OUT,
                  float* gW1, float* gb1, float* gW2, float* gb2) {
  return pings::launch(mlp_reduce_kernel, dim3((unsigned)pings::ceil_div<size_t>(per_block, 256)), 256, 0, st, partials,
                nblocks, per_block, IN, HID, OUT, gW1, gb1, gW2, gb2);
}

int fill_jobs(const pings_mlp_job* jobs, int njobs, MlpJobs& J) {
  PINGS_ARG_CHECK(jobs && njobs > 0 && njobs <= MAX_JOBS, "1..8 jobs");
  for (int g = 0; g < njobs; ++g) {
    const pings_mlp_job& q = jobs[g];
    PINGS_ARG_CHECK(q.IN > 0 && q.IN <= 32 && q.OUT > 0 && q.OUT <= OUTP, "grouped MLP: IN <= 32, OUT <= 32");
    PINGS_ARG_CHECK(q.x && q.W1 && q.b1 && q.W2 && q.b2, "null pointer in job");
    J.x[g] = q.x; J.W1[g] = q.W1; J.b1[g] = q.b1; J.W2[g] = q.W2; J.b2[g] = q.b2; J.y[g] = q.y;
    J.gy[g] = q.dL_dy; J.gx[g] = q.dL_dx; J.gW1[g] = q.dL_dW1; J.gb1[g] = q.dL_db1; J.gW2[g] = q.dL_dW2;
    J.gb2[g] = q.dL_db2; J.IN[g] = q.IN; J.OUT[g] = q.OUT;
    J.per_block[g] = partial_floats(q.IN, 128, q.OUT);
    J.partials[g] = nullptr;
  }
  return PINGS_OK;
}

}  // namespace

PINGS_API size_t pings_mlp_backward_scratch_bytes(int IN, int HID, int OUT) {
  if (IN <= 0 || HID <= 0 || OUT <= 0) return 0;
  return sizeof(float) * partial_floats(IN, HID, OUT) * MAX_BWD_BLOCKS;
}

PINGS_API int pings_mlp_forward(const float* x, int64_t N, int IN, int HID, int OUT, const float* W1,
                                const float* b1, const float* W2, const float* b2, float* y,
                                void* stream) {
  if (int e = check_dims(N, IN, HID, OUT)) return e;
  if (N == 0) return PINGS_OK;
  PINGS_ARG_CHECK(x && W1 && b1 && W2 && b2 && y, "null pointer");
  hipStream_t st = pings::as_stream(stream);
  const Dims d = make_dims(N, IN, HID, OUT);
  const long long ntiles = tiles_of(N);
  const Plan p = mlp_plan(IN, HID, OUT);
  pings::prof::Scope ps("mlp_fwd", st);
  switch (p.fwd) {
    case FAM_WAVE128: return launch_fwd_wave(wave_grid(ntiles, 512), st, N, IN, OUT, x, W1, b1, W2, b2, y);
    case FAM_H64O1: return launch_fwd_h64o1(p, wave_grid(ntiles, 512), st, N, IN, x, W1, b1, W2, b2, y);
    default: return launch_fwd_wg(p, wg_grid(ntiles), st, d, x, W1, b1, W2, b2, y);
  }
}

PINGS_API int pings_mlp_backward(const float* x, const float* dL_dy, int64_t N, int IN, int HID,
                                 int OUT, const float* W1, const float* b1, const float* W2,
                                 void* scratch, float* dL_dx, float* dL_dW1, float* dL_db1,
                                 float* dL_dW2, float* dL_db2, void* stream) {
  if (int e = check_dims(N, IN, HID, OUT)) return e;
  PINGS_ARG_CHECK(W1 && b1 && W2 && scratch && dL_dW1 && dL_db1 && dL_dW2 && dL_db2, "null pointer");
  hipStream_t st = pings::as_stream(stream);
  const size_t per_block = partial_floats(IN, HID, OUT);
  if (N == 0) {
    PINGS_HIP_CHECK(hipMemsetAsync(dL_dW1, 0, sizeof(float) * HID * IN, st));
    PINGS_HIP_CHECK(hipMemsetAsync(dL_dW2, 0, sizeof(float) * OUT * HID, st));
    PINGS_HIP_CHECK(hipMemsetAsync(dL_db1, 0, sizeof(float) * HID, st));
    PINGS_HIP_CHECK(hipMemsetAsync(dL_db2, 0, sizeof(float) * OUT, st));
    return PINGS_OK;
  }
  PINGS_ARG_CHECK(x && dL_dy, "null pointer");
  const Dims d = make_dims(N, IN, HID, OUT);
  const long long ntiles = tiles_of(N);
  const Plan p = mlp_plan(IN, HID, OUT);
  const int grid = p.bwd == FAM_WG ? wg_grid(ntiles) : wave_grid(ntiles, 256);
  float* part = reinterpret_cast<float*>(scratch);
  pings::prof::Scope ps("mlp_bwd", st);
  int e;
  switch (p.bwd) {
    case FAM_WAVE128: e = launch_bwd_wave(grid, st, N, IN, OUT, x, dL_dy, W1, b1, W2, dL_dx, part, per_block); break;
    case FAM_H64O1: e = launch_bwd_h64o1(p, grid, st, N, IN, x, dL_dy, W1, b1, W2, dL_dx, part, per_block); break;
    default: e = launch_bwd_wg(p, grid, st, d, x, dL_dy, W1, b1, W2, dL_dx, part); break;
  }
  if (e) return e;
  return launch_reduce(st, part, grid, per_block, IN, HID, OUT, dL_dW1, dL_db1, dL_dW2, dL_db2);
}

PINGS_API int pings_mlp_double_backward_supported(int IN, int HID, int OUT) {
  return (HID == 64 && OUT == 1 && IN > 0 && IN <= 64) ? 1 : 0;
}

PINGS_API int pings_mlp_double_backward(const float* x, const float* ddx, const float* dL_dy, int64_t N, int IN,
                                        int HID, int OUT, const float* W1, const float* b1, const float* W2,
                                        void* scratch, float* d_dy, float* d_W1, float* d_W2, void* stream) {
  if (int e = check_dims(N, IN, HID, OUT)) return e;
  PINGS_ARG_CHECK(pings_mlp_double_backward_supported(IN, HID, OUT), "double backward: hidden 64, one output only");
  PINGS_ARG_CHECK(W1 && b1 && W2 && d_W1 && d_W2 && scratch, "null pointer");
  hipStream_t st = pings::as_stream(stream);
  if (N == 0) {
    PINGS_HIP_CHECK(hipMemsetAsync(d_W1, 0, sizeof(float) * HID * IN, st));
    PINGS_HIP_CHECK(hipMemsetAsync(d_W2, 0, sizeof(float) * OUT * HID, st));
    return PINGS_OK;
  }
  PINGS_ARG_CHECK(x && ddx && dL_dy && d_dy, "null pointer");
  const size_t per_block = partial_floats(IN, HID, OUT);
  const int grid = wave_grid(tiles_of(N), 256);
  // scratch: MAX_BWD_BLOCKS partials (pings_mlp_backward_scratch_bytes), then 65 floats that take the reduce kernel's
  // (all-zero) gb1 / gb2 columns
  float* part = reinterpret_cast<float*>(scratch);
  float* dummy = part + (size_t)MAX_BWD_BLOCKS * per_block - 72;   // the launch uses at most 256 of the 1024 partials
  pings::prof::Scope ps("mlp_dbl", st);
  const Plan p = mlp_plan(IN, HID, OUT);
  if (int e = launch_dbl_h64o1(p, grid, st, N, IN, x, ddx, dL_dy, W1, b1, W2, d_dy, part, per_block)) return e;
  return launch_reduce(st, part, grid, per_block, IN, HID, OUT, d_W1, dummy, d_W2, dummy + 64);
}

// ---------------------------------------------------------------- grouped launches (several decoders, same rows)
PINGS_API int pings_mlp_forward_grouped(const pings_mlp_job* jobs, int njobs, int64_t N, void* stream) {
  return pings_mlp_forward_grouped_dyn(jobs, njobs, N, nullptr, stream);
}

PINGS_API int pings_mlp_forward_grouped_dyn(const pings_mlp_job* jobs, int njobs, int64_t N, const int32_t* n_rows_dev,
                                            void* stream) {
  MlpJobs J;
  if (int e = fill_jobs(jobs, njobs, J)) return e;
  PINGS_ARG_CHECK(N >= 0, "negative N");
  if (N == 0) return PINGS_OK;
  for (int g = 0; g < njobs; ++g) PINGS_ARG_CHECK(J.y[g] != nullptr, "null output");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("mlp_fwd", st);
  // two resident workgroups per CU over ALL jobs together: every workgroup stages its weights once and then walks
  // njobs times more tiles than in a per-decoder launch of 512 workgroups
  return launch_fwd_wave_grouped(wave_grid(tiles_of(N), 512 / njobs), njobs, st, N, J, n_rows_dev);
}

PINGS_API size_t pings_mlp_backward_grouped_scratch_bytes(const pings_mlp_job* jobs, int njobs) {
  size_t total = 0;
  if (!jobs) return 0;
  for (int g = 0; g < njobs; ++g) total += sizeof(float) * partial_floats(jobs[g].IN, 128, jobs[g].OUT) * 256;
  return total;
}

PINGS_API int pings_mlp_backward_grouped(const pings_mlp_job* jobs, int njobs, int64_t N, void* scratch,
                                         void* stream) {
  MlpJobs J;
  if (int e = fill_jobs(jobs, njobs, J)) return e;
  PINGS_ARG_CHECK(N > 0 && scratch, "grouped backward needs rows and scratch");
  float* p = reinterpret_cast<float*>(scratch);
  size_t max_pb = 0;
  for (int g = 0; g < njobs; ++g) {
    PINGS_ARG_CHECK(J.gy[g] && J.gW1[g] && J.gb1[g] && J.gW2[g] && J.gb2[g], "null gradient pointer in job");
    J.partials[g] = p;
    p += J.per_block[g] * 256;
    if (J.per_block[g] > max_pb) max_pb = J.per_block[g];
  }
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("mlp_bwd", st);
  // one resident workgroup per CU over all jobs together (see the forward), split between the jobs in proportion to
  // their MFMAs per tile: 4 x (17 + OH + 16 + 32), OH = k-steps of product B (mlp_bwd_wave_dispatch)
  const long long ntiles = tiles_of(N);
  const int want = wave_grid(ntiles, 256);   // workgroups that give every wave one tile, at most all of them
  int cost[MAX_JOBS];
  for (int g = 0; g < njobs; ++g) {
    const bool vecg = (J.OUT[g] % 4 == 0) && ((reinterpret_cast<uintptr_t>(J.gy[g]) & 15) == 0);
    const int oh = !vecg ? 16 : (J.OUT[g] == 24 ? 12 : (J.OUT[g] == 8 ? 4 : 16));
    cost[g] = 17 + oh + 16 + 32;
  }
  // 256 workgroups (one per CU) over the jobs so that the LAST wave finishes as early as possible: a job with w
  // workgroups needs ceil(ntiles / 4w) rounds of cost[g] MFMAs.  Greedy on the maximum (one more workgroup to the job
  // that finishes last) is optimal for a minimum over non-increasing step functions.  Shares merely proportional to
  // the costs left 5.9 % on the table at 125k points: 3907 tiles over 54 x 4 waves are 18.09 -> 19 rounds.
  int share[MAX_JOBS];
  for (int g = 0; g < njobs; ++g) share[g] = 1;
  for (int left = 256 - njobs; left > 0; --left) {
    int worst = -1;
    long long worst_t = -1;
    for (int g = 0; g < njobs; ++g) {
      const long long t_g = ((ntiles + 4LL * share[g] - 1) / (4LL * share[g])) * cost[g];
      if (t_g > worst_t) { worst_t = t_g; worst = g; }
    }
    if (share[worst] >= want) break;      // one tile per wave already: more workgroups would idle
    ++share[worst];
  }
  J.wg0[0] = 0;
  for (int g = 0; g < njobs; ++g) J.wg0[g + 1] = J.wg0[g] + share[g];
  if (int e = launch_bwd_wave_grouped(J.wg0[njobs], njobs, st, N, J)) return e;
  return pings::launch(mlp_reduce_grouped_kernel, dim3((unsigned)pings::ceil_div<size_t>(max_pb, 256), njobs), 256, 0, st, J,
                128);
}
