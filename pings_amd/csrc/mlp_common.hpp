// Shared definitions of the decoder MLP kernels (mlp.hip: what is computed and how it is laid out on the matrix cores).
//
// Which kernels a call runs is decided HERE, by mlp_plan, as a pure function of the shape.  mlp.hip (the C entry points)
// branches on the plan and on nothing else; each kernel family sits with its launch functions in its own file:
//   mlp_wave128.hip   one independent wave per 32-row tile, HID = 128, IN <= 32 (every Gaussian decoder), also grouped
//   mlp_h64o1.hip     the SDF decoder shape, HID = 64, OUT = 1: forward, backward, backward of the backward
//   mlp_wg.hip        a workgroup of HID / 32 waves per tile, weights in LDS: every other shape check_dims admits
#pragma once
#include "common.hpp"

namespace pings {
namespace mlp {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int TR = 32;        // rows per tile
constexpr int MAX_INP = 64;   // padded input width limit
constexpr int OUTP = 32;      // padded output width
constexpr int BW_LD = 33;     // leading dimension of the backward wave kernels' private transpose tiles and W1 image

__device__ inline int rowmap(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

__device__ inline f32x16 mfma(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

struct Dims {
  long long N;
  int IN, INP, HID, OUT;  // INP = IN rounded up to even
  int ldw1, ldw2, ldx, ldg;  // LDS leading dimensions (odd -> conflict-free column walks)
};

__host__ __device__ inline Dims make_dims(long long N, int IN, int HID, int OUT) {
  Dims d;
  d.N = N; d.IN = IN; d.HID = HID; d.OUT = OUT;
  d.INP = (IN + 1) & ~1;
  d.ldw1 = d.INP + 1;
  d.ldw2 = HID + 1;
  d.ldx = d.INP + 1;
  d.ldg = OUTP + 1;
  return d;
}

// Several decoders over the same rows in ONE launch (blockIdx.y = decoder): the five spawn decoders of a view
// (gaussian_renderer/__init__.py:605-716) share their row count and, four of them, their input; one grid of
// 5 x 512 workgroups keeps every CU busy through the weight prologues and costs one launch instead of five.
constexpr int MAX_JOBS = 8;
struct MlpJobs {
  const float *x[MAX_JOBS], *W1[MAX_JOBS], *b1[MAX_JOBS], *W2[MAX_JOBS], *b2[MAX_JOBS];
  float* y[MAX_JOBS];
  const float* gy[MAX_JOBS];
  float* gx[MAX_JOBS];
  float* partials[MAX_JOBS];
  size_t per_block[MAX_JOBS];
  float *gW1[MAX_JOBS], *gb1[MAX_JOBS], *gW2[MAX_JOBS], *gb2[MAX_JOBS];
  int IN[MAX_JOBS], OUT[MAX_JOBS];
  int wg0[MAX_JOBS + 1];   // backward: job g owns workgroups [wg0[g], wg0[g + 1]) of a 1-D grid (cost-proportional shares)
};

// backward scratch layout per workgroup: [HID*IN] gW1, [OUT*HID] gW2, [HID] gb1, [OUT] gb2
__host__ __device__ inline size_t partial_floats(int IN, int HID, int OUT) {
  return (size_t)HID * IN + (size_t)OUT * HID + HID + OUT;
}
constexpr int MAX_BWD_BLOCKS = 1024;  // partials the scratch of a single (not grouped) backward is sized for

// ---------------------------------------------------------------- the plan
enum Family {
  FAM_WAVE128,  // HID = 128, IN <= 32
  FAM_H64O1,    // HID = 64, OUT = 1
  FAM_WG,       // everything else
};

struct Plan {
  Family fwd, bwd;        // the double backward exists for FAM_H64O1 only (pings_mlp_double_backward_supported)
  int fwd_ks;             // FAM_H64O1 forward <KS>: k-steps per lane half, 2 KS >= IN + 1 (the bias column)
  int h64_ns, h64_ib;     // FAM_H64O1 backward <NS, IB, 0> and double backward <NS, IB>: k-steps, 32-wide input blocks
  int fwd_pfx;            // FAM_WG forward <PF_X>: prefetch registers per thread for a tile of x
  int bwd_pfx, bwd_pfg;   // FAM_WG backward <PF_X, PF_G>: the same, and for the tile of gY
};

inline Plan mlp_plan(int IN, int HID, int OUT) {
  Plan p = {};
  const bool wave128 = HID == 128 && IN <= 32, h64o1 = HID == 64 && OUT == 1;
  p.bwd = wave128 ? FAM_WAVE128 : h64o1 ? FAM_H64O1 : FAM_WG;
  // The SDF forward holds a row's inputs and the bias column in 2 KS <= 36 registers, hence IN <= 35 (every shipped
  // feature width: F + 3 = 35 or 11); wider inputs take the workgroup kernel.  Its backward and double backward read
  // their operands from an LDS image in up to 32 k-steps of two inputs and so take every IN check_dims admits.
  p.fwd = (h64o1 && IN > 35) ? FAM_WG : p.bwd;
  p.fwd_ks = IN + 1 <= 12 ? 6 : IN + 1 <= 20 ? 10 : 18;
  // two inputs per k-step; a second 32-wide input block beyond IN = 32.  <18, 1, 3> (the three position inputs of
  // IN = 35 on the vector ALU instead of a second block) measured no faster: DESIGN 2.4
  p.h64_ns = IN <= 12 ? 6 : IN <= 32 ? 16 : IN <= 36 ? 18 : 32;
  p.h64_ib = IN <= 32 ? 1 : 2;
  // workgroup kernels: ceil(32 * INP / threads) registers of x per thread, rounded up to a size class (the backward's
  // classes per thread count); the tile of gY is 32 x 32 floats whatever OUT is: 4, 6 (5.3), 8, 16 for 4 .. 1 waves
  const int nthr = 64 * (HID / 32), need = (TR * ((IN + 1) & ~1) + nthr - 1) / nthr;
  p.fwd_pfx = need <= 5 ? 5 : need <= 10 ? 10 : need <= 18 ? 18 : 32;
  // (HID = 128 comes here with IN > 32 only: need = ceil(INP / 8) is 5 .. 8)
  p.bwd_pfx = HID == 128 ? (need <= 5 ? 5 : 9) : HID == 96 ? (need <= 6 ? 6 : 11)
            : HID == 64 ? (need <= 9 ? 9 : 16) : (need <= 18 ? 18 : 32);
  p.bwd_pfg = HID == 128 ? 4 : HID == 96 ? 6 : HID == 64 ? 8 : 16;
  return p;
}

// ---------------------------------------------------------------- grids
inline long long tiles_of(long long N) { return (N + TR - 1) / TR; }
// wave kernels: a workgroup is four independent waves with one tile each per trip; cap = the workgroups resident at once
// (forward 512 = two per CU, weights in registers; backward 256 = one per CU, as its registers and LDS dictate)
inline int wave_grid(long long ntiles, long long cap) {
  const long long want = (ntiles + 3) / 4;
  return (int)(want < cap ? want : cap);
}
// workgroup kernels: a workgroup per tile, two resident per CU so that the weights are staged once each
inline int wg_grid(long long ntiles) { return (int)(ntiles < 512 ? ntiles : 512); }

// ---------------------------------------------------------------- launch functions (each in the file of its kernels)
// All return a PINGS status; `grid` comes from the rules above.  mlp_wave128.hip:
int launch_fwd_wave(int grid, hipStream_t st, long long N, int IN, int OUT, const float* x, const float* W1,
                    const float* b1, const float* W2, const float* b2, float* y);
int launch_fwd_wave_grouped(int grid, int njobs, hipStream_t st, long long N, const MlpJobs& J, const int* n_dev);
int launch_bwd_wave(int grid, hipStream_t st, long long N, int IN, int OUT, const float* x, const float* gy,
                    const float* W1, const float* b1, const float* W2, float* gx, float* partials, size_t per_block);
int launch_bwd_wave_grouped(int grid, int njobs, hipStream_t st, long long N, const MlpJobs& J);
// mlp_h64o1.hip
int launch_fwd_h64o1(const Plan& p, int grid, hipStream_t st, long long N, int IN, const float* x, const float* W1,
                     const float* b1, const float* W2, const float* b2, float* y);
int launch_bwd_h64o1(const Plan& p, int grid, hipStream_t st, long long N, int IN, const float* x, const float* gy,
                     const float* W1, const float* b1, const float* W2, float* gx, float* partials, size_t per_block);
int launch_dbl_h64o1(const Plan& p, int grid, hipStream_t st, long long N, int IN, const float* x, const float* a,
                     const float* gy, const float* W1, const float* b1, const float* W2, float* ggy, float* partials,
                     size_t per_block);
// mlp_wg.hip
int launch_fwd_wg(const Plan& p, int grid, hipStream_t st, const Dims& d, const float* x, const float* W1,
                  const float* b1, const float* W2, const float* b2, float* y);
int launch_bwd_wg(const Plan& p, int grid, hipStream_t st, const Dims& d, const float* x, const float* gy,
                  const float* W1, const float* b1, const float* W2, float* gx, float* partials);

}  // namespace mlp
}  // namespace pings
