// Decoder MLP, wave kernels for HID = 128, IN <= 32 (every Gaussian decoder): one independent wave per 32-row tile,
// forward and backward, single and grouped (several decoders in one launch).  Layouts and the accumulator-as-operand
// chaining are described in mlp.hip.
#include "mlp_common.hpp"

namespace pings {
namespace mlp {
namespace {

// ---------------------------------------------------------------- forward, one independent wave per 32-row tile
// For the GS decoders (HID = 128, IN <= 32, OUT <= 32: every shipped config).  A wave takes a 32-row tile from x to y
// with no workgroup barrier, no LDS and no weight traffic after its prologue: both weight matrices live in its
// registers as MFMA A-operand fragments (W1: 4 hidden blocks x 17 k-steps, W2: 4 x 16), the x tile is loaded straight
// into the B-operand layout (the k order of the first product is free: lane half h takes inputs 16 h .. 16 h + 15,
// sixteen contiguous floats of its row), the bias b1 rides along as one more k-step against a constant 1, and each
// 32-unit block of the hidden layer goes accumulator -> ReLU -> B operand of the second product (accumulator-as-
// operand chaining), which accumulates Y^T over the four blocks in ONE accumulator initialised with b2: no
// cross-wave sum.  132 MFMAs per tile and wave; the next tile's x is in flight meanwhile.  Results are bitwise those
// of the workgroup kernel's fma order up to the order of the hidden-block sum, i.e. within 1e-6.
__device__ __forceinline__ void mlp_fwd_wave_body(long long N, int IN, int OUT, const float* __restrict__ x,
                                                  const float* __restrict__ W1, const float* __restrict__ b1,
                                                  const float* __restrict__ W2, const float* __restrict__ b2,
                                                  float* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 31, h = lane >> 5;
  // ---- weight fragments
  float w1f[4][17], w2f[4][16], b2f[16];
  const bool vecw = (IN % 4 == 0) && ((reinterpret_cast<uintptr_t>(W1) & 15) == 0) &&
                    ((reinterpret_cast<uintptr_t>(W2) & 15) == 0);
#pragma unroll
  for (int hb = 0; hb < 4; ++hb) {
    const int hid = hb * 32 + r;
    if (vecw) {  // 16-byte loads: a lane's 16 inputs of a hidden unit, and its four runs of four hidden units of W2
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int k = 16 * h + 4 * q4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < IN) v = *reinterpret_cast<const float4*>(W1 + (size_t)hid * IN + k);
        w1f[hb][4 * q4] = v.x; w1f[hb][4 * q4 + 1] = v.y; w1f[hb][4 * q4 + 2] = v.z; w1f[hb][4 * q4 + 3] = v.w;
        float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < OUT) u = *reinterpret_cast<const float4*>(W2 + (size_t)r * 128 + hb * 32 + 8 * q4 + 4 * h);
        w2f[hb][4 * q4] = u.x; w2f[hb][4 * q4 + 1] = u.y; w2f[hb][4 * q4 + 2] = u.z; w2f[hb][4 * q4 + 3] = u.w;
      }
    } else {
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int k = 16 * h + s;
        w1f[hb][s] = k < IN ? W1[(size_t)hid * IN + k] : 0.f;
      }
#pragma unroll
      for (int t = 0; t < 16; ++t) w2f[hb][t] = r < OUT ? W2[(size_t)r * 128 + hb * 32 + rowmap(t, h)] : 0.f;
    }
    w1f[hb][16] = h == 0 ? b1[hid] : 0.f;            // k-step 16: (constant 1, zero) against (b1, 0)
  }
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int o = rowmap(t, h);
    b2f[t] = o < OUT ? b2[o] : 0.f;
  }
  const bool vec = (IN % 4 == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0);
  const long long ntiles = (N + 31) / 32;
  const long long nwaves = (long long)gridDim.x * (blockDim.x >> 6);
  const long long wave0 = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);

  float xf[16], xn[16];
  auto fetch = [&](long long t, float (&dst)[16]) {
    const long long row = t * 32 + r;
    const bool ok = row < N;
    if (vec) {
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int k = 16 * h + 4 * q4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok && k < IN) v = *reinterpret_cast<const float4*>(x + (size_t)row * IN + k);
        dst[4 * q4 + 0] = v.x; dst[4 * q4 + 1] = v.y; dst[4 * q4 + 2] = v.z; dst[4 * q4 + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int s2 = 0; s2 < 16; ++s2) {
        const int k = 16 * h + s2;
        dst[s2] = (ok && k < IN) ? x[(size_t)row * IN + k] : 0.f;
      }
    }
  };
  if (wave0 < ntiles) fetch(wave0, xn);
  for (long long t = wave0; t < ntiles; t += nwaves) {
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2) xf[s2] = xn[s2];
    if (t + nwaves < ntiles) fetch(t + nwaves, xn);
    const float one = h == 0 ? 1.f : 0.f;
    f32x16 yacc;
#pragma unroll
    for (int q = 0; q < 16; ++q) yacc[q] = b2f[q];
#pragma unroll
    for (int hb = 0; hb < 4; ++hb) {
      f32x16 acc = {0};
#pragma unroll
      for (int s2 = 0; s2 < 16; ++s2) acc = mfma(w1f[hb][s2], xf[s2], acc);
      acc = mfma(w1f[hb][16], one, acc);
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[q] = fmaxf(acc[q], 0.f);
#pragma unroll
      for (int q = 0; q < 16; ++q) yacc = mfma(w2f[hb][q], acc[q], yacc);
    }
    // Y^T[o = rowmap(q, h)][row = r]: four runs of four consecutive outputs per lane
    const long long row = t * 32 + r;
    if (row < N) {
      float* dst = y + (size_t)row * OUT;
      if (OUT % 4 == 0 && ((reinterpret_cast<uintptr_t>(y) & 15) == 0)) {
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const int o = 8 * gq + 4 * h;
          if (o < OUT)
            *reinterpret_cast<float4*>(dst + o) = make_float4(yacc[4 * gq], yacc[4 * gq + 1], yacc[4 * gq + 2], yacc[4 * gq + 3]);
        }
      } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int o = rowmap(q, h);
          if (o < OUT) dst[o] = yacc[q];
        }
      }
    }
  }
}

__global__ __launch_bounds__(256, 2) void mlp_fwd_wave_kernel(long long N, int IN, int OUT, const float* __restrict__ x,
                                                              const float* __restrict__ W1, const float* __restrict__ b1,
                                                              const float* __restrict__ W2, const float* __restrict__ b2,
                                                              float* __restrict__ y) {
  mlp_fwd_wave_body(N, IN, OUT, x, W1, b1, W2, b2, y);
}

__global__ __launch_bounds__(256, 2) void mlp_fwd_wave_grouped_kernel(long long N, MlpJobs j,
                                                                      const int* __restrict__ n_dev) {
  const int g = blockIdx.y;
  if (n_dev) N = min(N, (long long)*n_dev);   // N sized the grid and the buffers; the rows to decode are counted on the device
  mlp_fwd_wave_body(N, j.IN[g], j.OUT[g], j.x[g], j.W1[g], j.b1[g], j.W2[g], j.b2[g], j.y[g]);
}

// ---------------------------------------------------------------- backward, one independent wave per 32-row tile
// Same idea as mlp_fwd_wave_kernel, for HID = 128, IN <= 32: a wave takes a 32-row tile through all five products for
// all four hidden blocks; nothing but the read-only weight images in LDS is shared, so the only barrier is the one
// after staging them.  Per hidden block hb (k orders are free, lane half h takes k = 16 h .. 16 h + 15):
//   A  pre^T  = W1_hb x^T (+ b1 as a 17th k-step)          A = register fragments of W1, B = x rows
//   B  gH^T   = W2_hb^T gY^T, masked by pre > 0             A = W2 image in LDS,          B = gY rows
//   C  gX^T  += W1_hb^T gH^T                                A = W1 image in LDS,          B = the gH^T accumulator
//   D  gW2^T_hb += H^T gY,  gW1_hb += gH^T x  (sums over rows = lanes of the accumulators): H^T and gH^T make one
//      trip through the wave's private LDS to become A operands, B = x / gY read column-wise from global memory;
//      gb1 falls out of the transposed gH^T fragments, gb2 of the gY columns.
// 324 MFMAs per tile.  Weight-gradient accumulators stay in registers across the wave's tiles (8 x 16 + 5 VGPRs),
// are added across the four waves in LDS (wave order) and written as one partial per workgroup, summed by
// mlp_reduce_kernel in fixed order: bitwise reproducible.
constexpr int BW_LDS_FLOATS = 128 * BW_LD + 32 * 129 + 4 * 2 * 32 * BW_LD + 4 * 4 * 32 * BW_LD;   // mlp_bwd_wave_dispatch
constexpr int BW_REGION = 128 * 32 + 32 * 129 + 160;   // one wave's weight-gradient region in the epilogue
static_assert(4 * BW_REGION <= BW_LDS_FLOATS, "the four epilogue regions must fit the kernel's LDS");
#ifdef PINGS_MLP_STATS
__device__ unsigned long long g_mlp_stats[8];
__device__ unsigned long long g_mlp_clock[2];   // shader-clock cycles and 100 MHz real-time ticks of one workgroup's life
#endif
// Findings, so that nobody rebuilds the experiments (profiles/r04/mlp_sched_barrier_ab.txt,
// profiles/r04/mlp_bwd_ceiling.txt): hard scheduling barriers between the products of mlp_bwd_wave_body (pinning the
// operand reads of the next product above the MFMAs of the current one) measured 0.300-0.310 ms against 0.281 without,
// and sched_group_barrier chains for the stretch between two transposes changed the ISA as intended and gained nothing.
// The source order — the reads of the next product written ahead of the current product's MFMAs — is what the
// compiler's scheduler needs.
// The wave barriers around the wave-private LDS round trips (tile views; before / after the transpose writes) are NOT
// optional: builds without the two around the transposes were no faster (0.285-0.288 ms) and failed tests/test_mlp.py —
// the compiler does move the transposed reads across the writes without the fence.
// (wave barrier = scheduling fence; the empty asm with a memory clobber states the memory ordering explicitly)
#define MLP_WB_T do { __builtin_amdgcn_wave_barrier(); __asm__ volatile("" ::: "memory"); } while (0)

// The five products, issued so that the matrix pipe does not wait for operands:
//  * the A operands of a product are read from LDS into registers ONE PRODUCT AHEAD, while the previous product's MFMAs
//    execute: fetched just in time (ds_read -> s_waitcnt -> two MFMAs) each pair of MFMAs (128 cycles) exposes an LDS
//    round trip (57 % pipe busy);
//  * every global load is unconditional on a clamped address with a mask afterwards: bounds-checked loads compile to
//    one basic block each (~100 per tile) that nothing can be scheduled across.
//  * OH = k-steps of product B (gH^T = W2^T gY^T) per lane half: OUT / 2 when the decoder's output count is one of the
//    shipped classes (8, 24, 32: alpha; xyz / scale / colour; rotation — gaussian_renderer/__init__.py:609-708), so
//    that product does not multiply the zero padding of a 32-wide output tile; 16 with zero padding otherwise.
template <int OH, bool VECX, bool VECG>
__device__ __forceinline__ void mlp_bwd_wave_body(long long N, int IN, int OUT, const float* __restrict__ x,
                                                  const float* __restrict__ gy, const float* __restrict__ W1,
                                                  const float* __restrict__ b1, const float* __restrict__ W2,
                                                  float* __restrict__ gx, float* __restrict__ sW1, float* __restrict__ sW2, float* __restrict__ sT,
                                                  float* __restrict__ sXG, const int blk, const int nblk,
                                                  f32x16 (&aW2T)[4], f32x16 (&aW1)[4], float (&aB1)[4], float& aB2) {
  // LDS (declared once in mlp_bwd_wave_dispatch): sW1 = W1[hid][i] as [128][BW_LD], zero beyond IN; sW2 = W2[o][hid] as
  // [32][129], zero beyond OUT; sT = per wave H^T and gH^T as [4][2][32 * BW_LD] ([hid_local][row]); sXG = per wave the
  // double-buffered x and gY tiles [4][x0, x1, g0, g1][32 * BW_LD]
  const int tid = threadIdx.x, lane = tid & 63;
  // the wave index as a scalar: the tile index, the tile's base addresses and the wave's LDS windows stay in SGPRs
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;

#pragma unroll
  for (int hb = 0; hb < 4; ++hb) {
    aB1[hb] = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) { aW2T[hb][q] = 0.f; aW1[hb][q] = 0.f; }
  }
  aB2 = 0.f;

  float b1f[4];  // bias k-step of product A: (b1, 0) against (1, 0); loaded with the weight images below
  float* myH = sT + (wave * 2 + 0) * 32 * BW_LD;
  float* myG = sT + (wave * 2 + 1) * 32 * BW_LD;
  // the wave's private, double-buffered images of its tile of x and gY, [row][column] with leading dimension BW_LD
  // (conflict-free by rows and by columns): the row view (B operands of products A / B) and the column view (B operands
  // of the weight-gradient products) are both read from here, so a tile's rows are fetched from HBM ONCE, coalesced
  float* myX = sXG + (wave * 4 + 0) * 32 * BW_LD;   // + buf * 32 * BW_LD
  float* myGY = sXG + (wave * 4 + 2) * 32 * BW_LD;
  // lane half h of product B takes outputs o0 .. o0 + OH - 1
  const int o0 = h * OH;
  // every LDS access below is ONE per-lane base plus a compile-time offset (the instruction's immediate field): written
  // as (r, h)-dependent index expressions the compiler hoisted ~100 loop-invariant addresses out of the tile loop
  // and spilled them
  const float* const baseA = sW1 + r * BW_LD + 16 * h;        // + hb * 32 * BW_LD + s          (A operands of product A)
  const float* const baseB = sW2 + o0 * 129 + r;              // + s * 129 + hb * 32            (A operands of product B)
  const float* const baseC = sW1 + 4 * h * BW_LD + r;         // + (hb * 32 + rm(q)) * BW_LD    (A operands of product C)
  float* const wrH = myH + 4 * h * BW_LD + r;                 // + rm(q) * BW_LD                (transpose: write)
  float* const wrG = myG + 4 * h * BW_LD + r;
  const float* const rdH = myH + r * BW_LD + 16 * h;          // + s                            (transpose: read)
  const float* const rdG = myG + r * BW_LD + 16 * h;
  const long long ntiles = (N + 31) / 32;
  const long long nwaves = (long long)nblk * 4;       // this decoder's share of the grid (mlp_bwd_wave_grouped_kernel)
  const long long wave0 = (long long)blk * 4 + wave;

  // Row r of tile t: columns 16 h .. 16 h + 15 of x and of gY (zero beyond IN / OUT and beyond row N).  Every load is
  // issued whatever the row / column — the address is clamped into the array and the value masked afterwards with
  // integer ops — so a tile's fetch is ONE basic block with all loads in flight together.
  // fetch_rows only LOADS (raw values stay in flight in xd / gd for the whole tile); stage_rows masks them (integer and:
  // no select the compiler could turn back into a branch) and writes the LDS image.
  auto fetch_rows = [&](long long t, float (&xd)[16], float (&gd)[16]) {
    // address = wave-uniform tile base (SGPR pair) + a 32-bit per-lane element offset.  (As 64-bit per-lane pointers
    // the compiler kept ~25 loop-invariant address pairs, spilled them and re-read them from scratch at the top of
    // every tile: 28 scratch loads in front of the fetch.)  The lane half goes through an opaque move so that the
    // clamped column offsets are a handful of integer ops per tile instead of hoisted registers.
    long long tb = t * 32;
    if (tb > N - 1) tb = N - 1;                      // beyond the last tile: row N - 1 again, never used
    const long long below = N - 1 - tb;              // rows of the array after the tile's first one
    const int rl = below < 31 ? (r < (int)below ? r : (int)below) : r;
    int hh = h;
    __asm__ volatile("" : "+v"(hh));
    const float* xb = x + (size_t)tb * IN;
    const float* gb = gy + (size_t)tb * OUT;
    const uint32_t xro = (uint32_t)(rl * IN), gro = (uint32_t)(rl * OUT);   // unsigned: the saddr + 32-bit voffset form
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const int k = 16 * hh + 4 * q4;
      if (VECX) {    // IN a multiple of four, 16-byte aligned rows
        const float4 v = *reinterpret_cast<const float4*>(xb + (xro + (uint32_t)(k < IN ? k : 0)));
        xd[4 * q4] = v.x; xd[4 * q4 + 1] = v.y; xd[4 * q4 + 2] = v.z; xd[4 * q4 + 3] = v.w;
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) xd[4 * q4 + u] = xb[xro + (uint32_t)(k + u < IN ? k + u : 0)];
      }
      if (VECG) {
        const float4 u4 = *reinterpret_cast<const float4*>(gb + (gro + (uint32_t)(k < OUT ? k : 0)));
        gd[4 * q4] = u4.x; gd[4 * q4 + 1] = u4.y; gd[4 * q4 + 2] = u4.z; gd[4 * q4 + 3] = u4.w;
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) gd[4 * q4 + u] = gb[gro + (uint32_t)(k + u < OUT ? k + u : 0)];
      }
    }
  };
  auto stage_rows = [&](int buf, long long t, const float (&xd)[16], const float (&gd)[16]) {
    const uint32_t live = (t * 32 + r) < N ? 0xFFFFFFFFu : 0u;
    float* dx = myX + buf * 32 * BW_LD + r * BW_LD + 16 * h;
    float* dg = myGY + buf * 32 * BW_LD + r * BW_LD + 16 * h;
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2) {
      const int c = 16 * h + s2;
      dx[s2] = __uint_as_float(__float_as_uint(xd[s2]) & (c < IN ? live : 0u));
      dg[s2] = __uint_as_float(__float_as_uint(gd[s2]) & (c < OUT ? live : 0u));
    }
  };
  // A operands of products A (+ bias step) and B of hidden block hb, from the LDS weight images
  float opA[17], opB[OH];
  auto load_AB = [&](int hb) {
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2) opA[s2] = baseA[hb * 32 * BW_LD + s2];
    opA[16] = b1f[hb];
#pragma unroll
    for (int s2 = 0; s2 < OH; ++s2) opB[s2] = baseB[s2 * 129 + hb * 32];
  };

#ifdef PINGS_MLP_STATS   // diagnostic build only (tools/build_stats_lib.sh): shader-clock ticks per phase of the tile loop
  unsigned long long st_t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define MLP_TICK(k_) do { const unsigned long long now_ = __builtin_readcyclecounter(); st_t[k_] += now_ - st_last; st_last = now_; } while (0)
  unsigned long long st_last = __builtin_readcyclecounter();
#else
#define MLP_TICK(k_) do { } while (0)
#endif
  // row views (B operands of products A / B) of the tile about to be processed: read from the staged image at the END
  // of the previous tile, under its last weight-gradient products, so that a tile starts with its MFMAs
  float xf[16], gyf[OH];
  auto read_rows = [&](int b) {
    const float* bxr = myX + b * 32 * BW_LD + r * BW_LD + 16 * h;
    const float* bgr = myGY + b * 32 * BW_LD + r * BW_LD + o0;
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2) xf[s2] = bxr[s2];
#pragma unroll
    for (int s2 = 0; s2 < OH; ++s2) gyf[s2] = bgr[s2];
  };
  float xn[16], gn[16];
  int buf = 0;
  fetch_rows(wave0 < ntiles ? wave0 : 0, xn, gn);
  // the weight images are staged under the first tile's fetch
  for (int e = tid; e < 128 * 32; e += 256) {
    const int j = e >> 5, i = e & 31;
    sW1[j * BW_LD + i] = i < IN ? W1[(size_t)j * IN + i] : 0.f;
  }
  for (int e = tid; e < 32 * 128; e += 256) {
    const int o = e >> 7, j = e & 127;
    sW2[o * 129 + j] = o < OUT ? W2[(size_t)o * 128 + j] : 0.f;
  }
#pragma unroll
  for (int hb = 0; hb < 4; ++hb) b1f[hb] = h == 0 ? b1[hb * 32 + r] : 0.f;
  __syncthreads();
  stage_rows(0, wave0 < ntiles ? wave0 : 0, xn, gn);
  MLP_WB_T;
  read_rows(0);
  load_AB(0);
  const float one = h == 0 ? 1.f : 0.f;
  MLP_TICK(0);   // prologue
  for (long long t = wave0; t < ntiles; t += nwaves) {
    // the next tile's rows: in flight for the whole of this tile, staged into the other LDS buffer at its end
    // (beyond the last tile the clamped addresses re-read row N - 1 and the values are never used)
    fetch_rows(t + nwaves, xn, gn);
    float xcol[16], gycol[16];     // column views (B operands of the weight-gradient products): first used in product D
    {
      const float* bxc = myX + buf * 32 * BW_LD + 16 * h * BW_LD + r;
      const float* bgc = myGY + buf * 32 * BW_LD + 16 * h * BW_LD + r;
#pragma unroll
      for (int s2 = 0; s2 < 16; ++s2) {
        xcol[s2] = bxc[s2 * BW_LD];
        gycol[s2] = bgc[s2 * BW_LD];
      }
    }
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2) aB2 += gycol[s2];
    f32x16 gxacc = {0};
    MLP_TICK(1);   // tile start: operand views from LDS
#pragma unroll
    for (int hb = 0; hb < 4; ++hb) {
      // ---- products A and B on the operands read one product ago; meanwhile the A operands of product C
      float opC[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) opC[q] = baseC[(hb * 32 + (q & 3) + 8 * (q >> 2)) * BW_LD];
      f32x16 pre = {0}, gH = {0};
#pragma unroll
      for (int s2 = 0; s2 < 17; ++s2) {
        pre = mfma(opA[s2], s2 < 16 ? xf[s2] : one, pre);
        if (s2 < OH) gH = mfma(opB[s2], gyf[s2], gH);
      }
      MLP_TICK(2);   // products A / B issued
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        gH[q] = pre[q] > 0.f ? gH[q] : 0.f;
        pre[q] = fmaxf(pre[q], 0.f);
      }
      MLP_TICK(3);   // mask (waits for the products)
      // ---- product C; meanwhile H^T and gH^T take their trip through the wave's private LDS ([hid_local][row])
      MLP_WB_T;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        wrH[((q & 3) + 8 * (q >> 2)) * BW_LD] = pre[q];
        wrG[((q & 3) + 8 * (q >> 2)) * BW_LD] = gH[q];
      }
      // last hidden block: the next tile's rows (in flight since the top of this tile) go into the other image
      if (hb == 3) stage_rows(buf ^ 1, t + nwaves, xn, gn);
      MLP_WB_T;
      float aH[16], aG[16];
#pragma unroll
      for (int s2 = 0; s2 < 16; ++s2) {
        aH[s2] = rdH[s2];
        aG[s2] = rdG[s2];
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) gxacc = mfma(opC[q], gH[q], gxacc);   // (computed even when gx is null: no branch)
      MLP_TICK(4);   // transposes + product C issued
      // ---- the weight-gradient products; meanwhile the operands of the next hidden block's A and B
      load_AB((hb + 1) & 3);
      if (hb == 3) read_rows(buf ^ 1);
#pragma unroll
      for (int s2 = 0; s2 < 16; ++s2) {
        aB1[hb] += aG[s2];
        aW2T[hb] = mfma(aH[s2], gycol[s2], aW2T[hb]);
        aW1[hb] = mfma(aG[s2], xcol[s2], aW1[hb]);
      }
      MLP_TICK(5);   // products D issued
    }
    buf ^= 1;
    MLP_TICK(6);
    if (gx) {
      const long long row = t * 32 + r;
      if (row < N) {
        float* dst = gx + (size_t)row * IN;
        if (IN % 4 == 0 && ((reinterpret_cast<uintptr_t>(gx) & 15) == 0)) {
#pragma unroll
          for (int gq = 0; gq < 4; ++gq) {
            const int i = 8 * gq + 4 * h;
            if (i < IN)
              *reinterpret_cast<float4*>(dst + i) =
                  make_float4(gxacc[4 * gq], gxacc[4 * gq + 1], gxacc[4 * gq + 2], gxacc[4 * gq + 3]);
          }
        } else {
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int i = rowmap(q, h);
            if (i < IN) dst[i] = gxacc[q];
          }
        }
      }
    }
  }

  MLP_TICK(7);   // gX store of the last tile
#ifdef PINGS_MLP_STATS
  if (lane == 0)
    for (int k_ = 0; k_ < 8; ++k_) atomicAdd(&g_mlp_stats[k_], st_t[k_]);
#endif
}

// The workgroup's partial weight gradients (after mlp_bwd_wave_body; its own function so that the body's LDS pointers,
// which promise not to alias each other, are out of scope when the whole array is re-carved).  Every wave writes its
// accumulators into its OWN region of the (now dead) LDS at once, then all 256 threads add the four regions in wave
// order and write the partial in the global layout (the waves taking turns to add into one image cost four serial
// rounds and five barriers, ~5 us of the launch's ~35 us of fixed cost).  Region: gW1 as [hid][32] (lane = i), gW2 as
// [o][129] (lane = o), gb1, gb2.
__device__ __forceinline__ void mlp_bwd_wave_epilogue(int IN, int OUT, float* __restrict__ partials, size_t per_block,
                                                      float* __restrict__ sAll, const int blk, const f32x16 (&aW2T)[4],
                                                      const f32x16 (&aW1)[4], const float (&aB1)[4], const float aB2) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  __syncthreads();
  {
    float* R = sAll + wave * BW_REGION;
    float* rW1 = R, *rW2 = R + 128 * 32, *rB = R + 128 * 32 + 32 * 129;
#pragma unroll
    for (int hb = 0; hb < 4; ++hb) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int hid = hb * 32 + rowmap(q, h);
        rW2[r * 129 + hid] = aW2T[hb][q];
        rW1[hid * 32 + r] = aW1[hb][q];
      }
      const float v = aB1[hb] + __shfl_xor(aB1[hb], 32, 64);  // the two row halves of hidden unit hb*32 + r
      if (h == 0) rB[hb * 32 + r] = v;
    }
    const float v2 = aB2 + __shfl_xor(aB2, 32, 64);
    if (h == 0) rB[128 + r] = v2;
  }
  __syncthreads();
  float* P = partials + (size_t)blk * per_block;
  const int nW1 = 128 * IN, nW2 = OUT * 128;
  auto sum4 = [&](int off) {
    return ((sAll[off] + sAll[BW_REGION + off]) + sAll[2 * BW_REGION + off]) + sAll[3 * BW_REGION + off];
  };
  {
    const int i = tid & 31;
    if (i < IN)
      for (int j = tid >> 5; j < 128; j += 8) P[j * IN + i] = sum4(j * 32 + i);
  }
  for (int e = tid; e < nW2; e += 256) P[nW1 + e] = sum4(128 * 32 + (e >> 7) * 129 + (e & 127));
  if (tid < 128) P[nW1 + nW2 + tid] = sum4(128 * 32 + 32 * 129 + tid);
  if (tid < OUT) P[nW1 + nW2 + 128 + tid] = sum4(128 * 32 + 32 * 129 + 128 + tid);
}

// one instantiation per output class (the B product's k-steps are compile-time); the choice is uniform per workgroup.
// One wave per SIMD (~430 of its 512 registers).  A second body that fitted a wave into 231 registers, so that eight
// waves shared a CU, measured equal at every size (0.255 vs 0.247 ms at 125k points, slope 1.70 vs 1.71 us per 1000
// points: DESIGN 2.4 (f), profiles/r04/mlp_bwd_ceiling.txt) and was removed; last present in 14a8a4e.
__device__ __forceinline__ void mlp_bwd_wave_dispatch(long long N, int IN, int OUT, const float* __restrict__ x,
                                                      const float* __restrict__ gy, const float* __restrict__ W1,
                                                      const float* __restrict__ b1, const float* __restrict__ W2,
                                                      float* __restrict__ gx, float* __restrict__ partials,
                                                      size_t per_block, const int blk, const int nblk) {
  // one array (the epilogue re-carves it into four per-wave regions): W1 image, W2 image, transposes, x / gY tiles.
  // 135 KB in all: one workgroup per CU, as the registers dictate anyway
  __shared__ float sAll[BW_LDS_FLOATS];
  float* const sW1 = sAll;
  float* const sW2 = sW1 + 128 * BW_LD;
  float* const sT = sW2 + 32 * 129;
  float* const sXG = sT + 4 * 2 * 32 * BW_LD;
  // 16-byte row loads where the row length and the base allow (the colour decoder's 19 inputs: scalar loads of x)
  const bool vecx = (IN % 4 == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0);
  const bool vecg = (OUT % 4 == 0) && ((reinterpret_cast<uintptr_t>(gy) & 15) == 0);
  // (macros, not generic lambdas: written as lambdas both kernels compile to other code, with other SGPR spill counts)
#define PINGS_BWD_BODY(OH_, VX_, VG_) \
  mlp_bwd_wave_body<OH_, VX_, VG_>(N, IN, OUT, x, gy, W1, b1, W2, gx, sW1, sW2, sT, sXG, blk, nblk, aW2T, aW1, aB1, aB2)
#define PINGS_BWD_CLASS(VX_)                          \
  do {                                                \
    if (!vecg) PINGS_BWD_BODY(16, VX_, false);        \
    else if (OUT == 24) PINGS_BWD_BODY(12, VX_, true); \
    else if (OUT == 8) PINGS_BWD_BODY(4, VX_, true);  \
    else PINGS_BWD_BODY(16, VX_, true);               \
  } while (0)
  f32x16 aW2T[4], aW1[4];   // the wave's weight-gradient accumulators: 128 registers for the whole launch
  float aB1[4], aB2;
  if (vecx) PINGS_BWD_CLASS(true);
  else PINGS_BWD_CLASS(false);
#undef PINGS_BWD_CLASS
#undef PINGS_BWD_BODY
  mlp_bwd_wave_epilogue(IN, OUT, partials, per_block, sAll, blk, aW2T, aW1, aB1, aB2);
}

__global__ __launch_bounds__(256, 1) void mlp_bwd_wave_kernel(long long N, int IN, int OUT, const float* __restrict__ x,
                                                              const float* __restrict__ gy, const float* __restrict__ W1,
                                                              const float* __restrict__ b1, const float* __restrict__ W2,
                                                              float* __restrict__ gx, float* __restrict__ partials,
                                                              size_t per_block) {
  mlp_bwd_wave_dispatch(N, IN, OUT, x, gy, W1, b1, W2, gx, partials, per_block, (int)blockIdx.x, (int)gridDim.x);
}

// 1-D grid; decoder g owns workgroups [wg0[g], wg0[g + 1]): shares proportional to the decoders' MFMAs per tile (the
// 32-wide rotation decoder issues 324 per tile, the 8-wide alpha decoder 276), so that they finish together — with
// equal shares the launch lasted as long as its most expensive decoder (6 % more)
__global__ __launch_bounds__(256, 1) void mlp_bwd_wave_grouped_kernel(long long N, MlpJobs j, int njobs) {
#ifdef PINGS_MLP_STATS
  const unsigned long long c0_ = __builtin_readcyclecounter(), w0_ = wall_clock64();
#endif
  int g = 0;
  while (g + 1 < njobs && (int)blockIdx.x >= j.wg0[g + 1]) ++g;
  mlp_bwd_wave_dispatch(N, j.IN[g], j.OUT[g], j.x[g], j.gy[g], j.W1[g], j.b1[g], j.W2[g], j.gx[g], j.partials[g],
                        j.per_block[g], (int)blockIdx.x - j.wg0[g], j.wg0[g + 1] - j.wg0[g]);
#ifdef PINGS_MLP_STATS
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    g_mlp_clock[0] = __builtin_readcyclecounter() - c0_;
    g_mlp_clock[1] = wall_clock64() - w0_;
  }
#endif
}

}  // namespace

int launch_fwd_wave(int grid, hipStream_t st, long long N, int IN, int OUT, const float* x, const float* W1,
                    const float* b1, const float* W2, const float* b2, float* y) {
  return launch(mlp_fwd_wave_kernel, dim3(grid), 256, 0, st, N, IN, OUT, x, W1, b1, W2, b2, y);
}

int launch_fwd_wave_grouped(int grid, int njobs, hipStream_t st, long long N, const MlpJobs& J, const int* n_dev) {
  return launch(mlp_fwd_wave_grouped_kernel, dim3(grid, njobs), 256, 0, st, N, J, n_dev);
}

int launch_bwd_wave(int grid, hipStream_t st, long long N, int IN, int OUT, const float* x, const float* gy,
                    const float* W1, const float* b1, const float* W2, float* gx, float* partials, size_t per_block) {
  return launch(mlp_bwd_wave_kernel, dim3(grid), 256, 0, st, N, IN, OUT, x, gy, W1, b1, W2, gx, partials, per_block);
}

int launch_bwd_wave_grouped(int grid, int njobs, hipStream_t st, long long N, const MlpJobs& J) {
  return launch(mlp_bwd_wave_grouped_kernel, dim3(grid), 256, 0, st, N, J, njobs);
}

}  // namespace mlp
}  // namespace pings

#ifdef PINGS_MLP_STATS   // here because these two device symbols are: the library has no relocatable device code
using pings::mlp::g_mlp_stats;
using pings::mlp::g_mlp_clock;
PINGS_API int pings_debug_mlp_stats(unsigned long long* out8, int reset) {
  PINGS_HIP_CHECK(hipDeviceSynchronize());
  PINGS_HIP_CHECK(hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_mlp_stats), 64));
  if (reset) {
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    PINGS_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_mlp_stats), z, 64));
  }
  return PINGS_OK;
}
// out2 = {shader-clock cycles, 100 MHz real-time ticks} of workgroup 0 of the last grouped backward launch: the clock
// the kernel really ran at = 100 MHz x out2[0] / out2[1]
PINGS_API int pings_debug_mlp_clock(unsigned long long* out2) {
  PINGS_HIP_CHECK(hipDeviceSynchronize());
  PINGS_HIP_CHECK(hipMemcpyFromSymbol(out2, HIP_SYMBOL(g_mlp_clock), 16));
  return PINGS_OK;
}
#endif
