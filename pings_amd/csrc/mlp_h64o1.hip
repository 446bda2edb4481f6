// Decoder MLP, the SDF decoder shape (HID = 64, OUT = 1): forward, backward and backward of the backward, each one
// independent wave per 32-row tile.  Layouts and the accumulator-as-operand chaining are described in mlp.hip.
#include "mlp_common.hpp"

namespace pings {
namespace mlp {
namespace {

// ---------------------------------------------------------------- forward, SDF decoder shape (HID 64, OUT 1)
// `Decoder.sdf` (model/decoder.py:100-104) on [N, F + 3] rows: the general kernels above pad OUT = 1 to a 32-wide
// second product (96 % of its MFMAs multiply zeros) and stage the tile through LDS with three barriers.  Here a wave
// owns a 32-row tile outright, no LDS, no barrier:
//   H^T[64 x 32] = [W1 | b1] [x | 1]^T   two 32x32 accumulators (hidden blocks), KS k-steps of v_mfma_f32_32x32x2_f32;
//                                        the k order is free, so lane half h takes input columns KS*h .. KS*h + KS - 1:
//                                        KS consecutive floats of the lane's own row (loaded straight into the B
//                                        operand, the next tile's row in flight meanwhile), W1 columns in the same
//                                        order as register-resident A fragments; column IN is the bias (x = 1);
//   y[row] = b2 + sum_h W2[h] relu(H^T[h][row])   on the accumulator layout (column = row of the tile on the lane,
//                                        16 hidden units per register set and lane half): 32 fma + one half swap.
// 2 * KS MFMAs per 32 rows (36 for F = 32) against 18 + 16 + 16 * 2 of the padded product.
template <int KS>
__global__ __launch_bounds__(256, 2) void mlp_fwd_h64o1_kernel(long long N, int IN, const float* __restrict__ x,
                                                               const float* __restrict__ W1, const float* __restrict__ b1,
                                                               const float* __restrict__ W2, const float* __restrict__ b2,
                                                               float* __restrict__ y) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  float w1f[2][KS], w2f[2][16];
#pragma unroll
  for (int hb = 0; hb < 2; ++hb) {
    const int hid = hb * 32 + r;                     // A operand: row m = r, k = half
#pragma unroll
    for (int s2 = 0; s2 < KS; ++s2) {
      const int c = KS * h + s2;
      w1f[hb][s2] = c < IN ? W1[(size_t)hid * IN + c] : (c == IN ? b1[hid] : 0.f);
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) w2f[hb][q] = W2[hb * 32 + rowmap(q, h)];
  }
  const float bias2 = b2[0];
  const long long ntiles = (N + 31) / 32;
  const long long nwaves = (long long)gridDim.x * (blockDim.x >> 6);
  const long long wave0 = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  float xf[KS], xn[KS];
  auto fetch = [&](long long t, float (&dst)[KS]) {
    const long long row = t * 32 + r;
    const bool ok = row < N;
    const float* src = x + (size_t)(ok ? row : 0) * IN;
#pragma unroll
    for (int s2 = 0; s2 < KS; ++s2) {
      const int c = KS * h + s2;
      dst[s2] = c < IN ? (ok ? src[c] : 0.f) : (c == IN ? 1.f : 0.f);
    }
  };
  if (wave0 < ntiles) fetch(wave0, xn);
  for (long long t = wave0; t < ntiles; t += nwaves) {
#pragma unroll
    for (int s2 = 0; s2 < KS; ++s2) xf[s2] = xn[s2];
    if (t + nwaves < ntiles) fetch(t + nwaves, xn);
    f32x16 a0 = {0}, a1 = {0};
#pragma unroll
    for (int s2 = 0; s2 < KS; ++s2) {               // two independent accumulator chains, interleaved
      a0 = mfma(w1f[0][s2], xf[s2], a0);
      a1 = mfma(w1f[1][s2], xf[s2], a1);
    }
    float p = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) p = fmaf(w2f[0][q], fmaxf(a0[q], 0.f), p);
#pragma unroll
    for (int q = 0; q < 16; ++q) p = fmaf(w2f[1][q], fmaxf(a1[q], 0.f), p);
    p += __shfl_xor(p, 32, 64);                     // the other 32 hidden units of this row
    const long long row = t * 32 + r;
    if (h == 0 && row < N) y[row] = p + bias2;
  }
}

// ---------------------------------------------------------------- backward of the SDF decoder shape: HID = 64, OUT = 1
// (`Decoder.sdf`, decoder.py:102-104: [B k, F + 3] -> 64 -> 1; F + 3 = 35 or 11).  Same wave-per-tile scheme as
// mlp_bwd_wave_kernel, specialised for the single output: gH^T = relu'(pre) * W2[hid] * gy[row] is elementwise in the
// accumulator layout, gW2 / gb1 / gb2 accumulate per lane over all of the wave's tiles (one cross-lane reduction at
// the very end), and only gH^T makes the LDS trip for gW1 += gH^T x.  Inputs are consumed two per MFMA step
// (k = 2 s + h), so IN = 35 costs 18 steps of product A instead of a padded 32.  NS = k-steps, IB = 32-wide input
// blocks.  Per tile and hidden block: NS + 1 (A) + 16 IB (C) + 16 IB (D) MFMAs.
template <int NS, int IB, int NT>
__global__ __launch_bounds__(256, 1) void mlp_bwd_wave_h64o1_kernel(long long N, int IN, const float* __restrict__ x,
                                                                    const float* __restrict__ gy,
                                                                    const float* __restrict__ W1,
                                                                    const float* __restrict__ b1,
                                                                    const float* __restrict__ W2, float* __restrict__ gx,
                                                                    float* __restrict__ partials, size_t per_block) {
  constexpr int WI = 32 * IB + NT;          // input columns held in the W1 image
  constexpr int LD1 = WI | 1;               // odd leading dimension: conflict-free in both orientations
  static_assert(NT == 0 || IB == 1, "tail inputs follow a single 32-wide block");
  __shared__ float sW1[64 * LD1];          // W1[hid][i], zero beyond IN; reused for the workgroup's gW1
  __shared__ float sG[4][32 * BW_LD];      // per wave: gH^T as [hid_local][row]
  __shared__ float sB[64 + 64 + 1];        // workgroup sums of gW2, gb1, gb2
  __shared__ float sW2[64];                // W2[0][hid]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  for (int e = tid; e < 64 * WI; e += 256) {
    const int j = e / WI, i = e - j * WI;
    sW1[j * LD1 + i] = i < IN ? W1[(size_t)j * IN + i] : 0.f;
  }
  if (tid < 64) sW2[tid] = W2[tid];
  float b1f[2];
#pragma unroll
  for (int hb = 0; hb < 2; ++hb) b1f[hb] = h == 0 ? b1[hb * 32 + r] : 0.f;
  __syncthreads();

  f32x16 aW1[2][IB];
  float aW2[2][16], aB1[2][16], aB2 = 0.f;
  float aT[NT > 0 ? NT : 1][2][16];  // gW1 of the NT tail inputs: per-lane sums over rows, like aW2 / aB1
#pragma unroll
  for (int hb = 0; hb < 2; ++hb) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      aW2[hb][q] = 0.f;
      aB1[hb][q] = 0.f;
#pragma unroll
      for (int j = 0; j < NT; ++j) aT[j][hb][q] = 0.f;
#pragma unroll
      for (int ib = 0; ib < IB; ++ib) aW1[hb][ib][q] = 0.f;
    }
  }
  float* myG = &sG[wave][0];
  const long long ntiles = (N + 31) / 32;
  const long long nwaves = (long long)gridDim.x * 4;
  const float one = h == 0 ? 1.f : 0.f;
  for (long long t = (long long)blockIdx.x * 4 + wave; t < ntiles; t += nwaves) {
    // (a register prefetch of the next tile's operands, as in mlp_bwd_wave_kernel, measured 12 % SLOWER here)
    asm volatile("" ::: "memory");  // keep the loop-invariant LDS operands in LDS (hoisting them costs ~100 VGPRs)
    const long long row = t * 32 + r;
    const bool ok = row < N;
    float xf[NS];
#pragma unroll
    for (int s2 = 0; s2 < NS; ++s2) xf[s2] = (ok && 2 * s2 + h < IN) ? x[(size_t)row * IN + 2 * s2 + h] : 0.f;
    const float gyr = ok ? gy[row] : 0.f;
    float xcol[IB][16];  // x[row = 16 h + s][column = 32 ib + r]
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2) {
      const long long rc = t * 32 + 16 * h + s2;
#pragma unroll
      for (int ib = 0; ib < IB; ++ib)
        xcol[ib][s2] = (rc < N && 32 * ib + r < IN) ? x[(size_t)rc * IN + 32 * ib + r] : 0.f;
    }
    aB2 += h == 0 ? gyr : 0.f;
    // tail inputs 32 .. 32 + NT - 1 of this lane's row (xf holds the inputs of parity h: fetch the others from the
    // lane of the other half, same row) and their gX, both on the vector ALU: a second 32-wide MFMA block for three
    // position inputs would double products C and D
    float xt[NT > 0 ? NT : 1], gxt[NT > 0 ? NT : 1];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const float own = xf[16 + j / 2], other = __shfl_xor(own, 32, 64);
      xt[j] = (j & 1) == h ? own : other;
      gxt[j] = 0.f;
    }
    f32x16 gxacc[IB];
#pragma unroll
    for (int ib = 0; ib < IB; ++ib) gxacc[ib] = f32x16{0};
#pragma unroll
    for (int hb = 0; hb < 2; ++hb) {
      f32x16 pre = {0};
#pragma unroll
      for (int s2 = 0; s2 < NS; ++s2) pre = mfma(sW1[(hb * 32 + r) * LD1 + 2 * s2 + h], xf[s2], pre);
      pre = mfma(b1f[hb], one, pre);
      float gH[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        gH[q] = pre[q] > 0.f ? sW2[hb * 32 + rowmap(q, h)] * gyr : 0.f;
        aW2[hb][q] = fmaf(fmaxf(pre[q], 0.f), gyr, aW2[hb][q]);
        aB1[hb][q] += gH[q];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          aT[j][hb][q] = fmaf(gH[q], xt[j], aT[j][hb][q]);
          gxt[j] = fmaf(sW1[(hb * 32 + rowmap(q, h)) * LD1 + 32 + j], gH[q], gxt[j]);
        }
      }
      if (gx) {
#pragma unroll
        for (int ib = 0; ib < IB; ++ib)
#pragma unroll
          for (int q = 0; q < 16; ++q)
            gxacc[ib] = mfma(sW1[(hb * 32 + rowmap(q, h)) * LD1 + 32 * ib + r], gH[q], gxacc[ib]);
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int q = 0; q < 16; ++q) myG[rowmap(q, h) * BW_LD + r] = gH[q];
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int s2 = 0; s2 < 16; ++s2) {
        const float aG = myG[r * BW_LD + 16 * h + s2];
#pragma unroll
        for (int ib = 0; ib < IB; ++ib) aW1[hb][ib] = mfma(aG, xcol[ib][s2], aW1[hb][ib]);
      }
    }
    if (gx && ok) {
      float* dst = gx + (size_t)row * IN;
#pragma unroll
      for (int ib = 0; ib < IB; ++ib)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int i = 32 * ib + rowmap(q, h);
          if (i < IN) dst[i] = gxacc[ib][q];
        }
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const float v = gxt[j] + __shfl_xor(gxt[j], 32, 64);  // the two halves hold disjoint hidden units
      if (gx && ok && h == 0 && 32 + j < IN) gx[(size_t)row * IN + 32 + j] = v;
    }
  }

  // per-lane sums over rows -> sums over the 32 lanes that share h (hidden unit hb*32 + rowmap(q, h))
#pragma unroll
  for (int hb = 0; hb < 2; ++hb)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) {
        aW2[hb][q] += __shfl_xor(aW2[hb][q], off, 64);
        aB1[hb][q] += __shfl_xor(aB1[hb][q], off, 64);
#pragma unroll
        for (int j = 0; j < NT; ++j) aT[j][hb][q] += __shfl_xor(aT[j][hb][q], off, 64);
      }
    }
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) aB2 += __shfl_xor(aB2, off, 64);

  // the four waves add theirs in wave order: gW1 into the (now dead) W1 image, the vectors into sB
  for (int w = 0; w < 4; ++w) {
    __syncthreads();
    if (wave == w) {
#pragma unroll
      for (int hb = 0; hb < 2; ++hb)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int hid = hb * 32 + rowmap(q, h);
#pragma unroll
          for (int ib = 0; ib < IB; ++ib) {
            float* d1 = &sW1[hid * LD1 + 32 * ib + r];
            if (w == 0) *d1 = aW1[hb][ib][q]; else *d1 += aW1[hb][ib][q];
          }
          if (r == 0) {
            if (w == 0) { sB[hid] = aW2[hb][q]; sB[64 + hid] = aB1[hb][q]; }
            else { sB[hid] += aW2[hb][q]; sB[64 + hid] += aB1[hb][q]; }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
              if (w == 0) sW1[hid * LD1 + 32 + j] = aT[j][hb][q]; else sW1[hid * LD1 + 32 + j] += aT[j][hb][q];
            }
          }
        }
      if (lane == 0) { if (w == 0) sB[128] = aB2; else sB[128] += aB2; }
    }
  }
  __syncthreads();
  float* P = partials + (size_t)blockIdx.x * per_block;  // [64 IN | 64 | 64 | 1]
  const int nW1 = 64 * IN;
  for (int e = tid; e < nW1; e += 256) P[e] = sW1[(e / IN) * LD1 + (e % IN)];
  if (tid < 64) { P[nW1 + tid] = sB[tid]; P[nW1 + 64 + tid] = sB[64 + tid]; }
  if (tid == 0) P[nW1 + 128] = sB[128];
}

// ---------------------------------------------------------------- backward of the backward, SDF decoder shape
// The mapper's Eikonal / consistency terms differentiate dS/dx once more (utils/tools.py:409-419 `get_gradient` with
// create_graph=True, used at utils/mapper.py:1445-1448): the first-order backward
//     gx[n, :] = gy[n] * sum_j m[n, j] W2[j] W1[j, :]          (m = [W1 x + b1 > 0])
// is itself a graph node, and a loss on gx sends a cotangent a = dL/dgx [N, IN] back through it:
//     ggy[n]    = sum_j m[n, j] W2[j] u[n, j]                  u = a W1^T
//     gW2[j]    = sum_n gy[n] m[n, j] u[n, j]
//     gW1[j, :] = sum_n gy[n] m[n, j] W2[j] a[n, :]
// (nothing reaches x or b1: the mask is piecewise constant, as in torch's own relu).  Same wave-per-tile scheme and
// accumulator layouts as mlp_bwd_wave_h64o1_kernel: product A twice (x for the mask, a for u, sharing the W1
// fragments), the elementwise part in the accumulator layout, gH2^T = (m W2 gy)^T through the wave's private LDS
// tile for gW1 += gH2^T a.  Partials in the layout of the first-order kernel ([64 IN | gW2 64 | 64 zeros | 0]) so
// that mlp_reduce_kernel sums them.
template <int NS, int IB>
__global__ __launch_bounds__(256, 1) void mlp_dbl_wave_h64o1_kernel(long long N, int IN, const float* __restrict__ x,
                                                                    const float* __restrict__ a,
                                                                    const float* __restrict__ gy,
                                                                    const float* __restrict__ W1,
                                                                    const float* __restrict__ b1,
                                                                    const float* __restrict__ W2,
                                                                    float* __restrict__ ggy,
                                                                    float* __restrict__ partials, size_t per_block) {
  constexpr int WI = 32 * IB;
  constexpr int LD1 = WI | 1;
  __shared__ float sW1[64 * LD1];          // W1[hid][i], zero beyond IN; reused for the workgroup's gW1
  __shared__ float sG[4][32 * BW_LD];      // per wave: gH2^T as [hid_local][row]
  __shared__ float sB[64];                 // workgroup sum of gW2
  __shared__ float sW2[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  for (int e = tid; e < 64 * WI; e += 256) {
    const int j = e / WI, i = e - j * WI;
    sW1[j * LD1 + i] = i < IN ? W1[(size_t)j * IN + i] : 0.f;
  }
  if (tid < 64) sW2[tid] = W2[tid];
  float b1f[2];
#pragma unroll
  for (int hb = 0; hb < 2; ++hb) b1f[hb] = h == 0 ? b1[hb * 32 + r] : 0.f;
  __syncthreads();

  f32x16 aW1[2][IB];
  float aW2[2][16];
#pragma unroll
  for (int hb = 0; hb < 2; ++hb)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      aW2[hb][q] = 0.f;
#pragma unroll
      for (int ib = 0; ib < IB; ++ib) aW1[hb][ib][q] = 0.f;
    }
  float* myG = &sG[wave][0];
  const long long ntiles = (N + 31) / 32;
  const long long nwaves = (long long)gridDim.x * 4;
  const float one = h == 0 ? 1.f : 0.f;
  for (long long t = (long long)blockIdx.x * 4 + wave; t < ntiles; t += nwaves) {
    asm volatile("" ::: "memory");  // keep the loop-invariant LDS operands in LDS (as in the first-order kernel)
    const long long row = t * 32 + r;
    const bool ok = row < N;
    float xf[NS], af[NS];
#pragma unroll
    for (int s2 = 0; s2 < NS; ++s2) {
      const bool in = ok && 2 * s2 + h < IN;
      xf[s2] = in ? x[(size_t)row * IN + 2 * s2 + h] : 0.f;
      af[s2] = in ? a[(size_t)row * IN + 2 * s2 + h] : 0.f;
    }
    const float gyr = ok ? gy[row] : 0.f;
    float acol[IB][16];  // a[row = 16 h + s][column = 32 ib + r]
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2) {
      const long long rc = t * 32 + 16 * h + s2;
#pragma unroll
      for (int ib = 0; ib < IB; ++ib)
        acol[ib][s2] = (rc < N && 32 * ib + r < IN) ? a[(size_t)rc * IN + 32 * ib + r] : 0.f;
    }
    float ggy_part = 0.f;
#pragma unroll
    for (int hb = 0; hb < 2; ++hb) {
      f32x16 pre = {0}, u = {0};
#pragma unroll
      for (int s2 = 0; s2 < NS; ++s2) {
        const float w = sW1[(hb * 32 + r) * LD1 + 2 * s2 + h];
        pre = mfma(w, xf[s2], pre);
        u = mfma(w, af[s2], u);
      }
      pre = mfma(b1f[hb], one, pre);
      float gH[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const bool on = pre[q] > 0.f;
        const float w2 = sW2[hb * 32 + rowmap(q, h)];
        gH[q] = on ? w2 * gyr : 0.f;
        aW2[hb][q] = fmaf(on ? u[q] : 0.f, gyr, aW2[hb][q]);
        ggy_part = fmaf(on ? w2 : 0.f, u[q], ggy_part);
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int q = 0; q < 16; ++q) myG[rowmap(q, h) * BW_LD + r] = gH[q];
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int s2 = 0; s2 < 16; ++s2) {
        const float aG = myG[r * BW_LD + 16 * h + s2];
#pragma unroll
        for (int ib = 0; ib < IB; ++ib) aW1[hb][ib] = mfma(aG, acol[ib][s2], aW1[hb][ib]);
      }
    }
    ggy_part += __shfl_xor(ggy_part, 32, 64);   // the two lane halves hold disjoint hidden units of the same row
    if (ok && h == 0) ggy[row] = ggy_part;
  }

  // per-lane sums over rows -> sums over the 32 lanes that share h (hidden unit hb*32 + rowmap(q, h))
#pragma unroll
  for (int hb = 0; hb < 2; ++hb)
#pragma unroll
    for (int q = 0; q < 16; ++q)
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) aW2[hb][q] += __shfl_xor(aW2[hb][q], off, 64);
  // the four waves add theirs in wave order: gW1 into the (now dead) W1 image, gW2 into sB
  for (int w = 0; w < 4; ++w) {
    __syncthreads();
    if (wave == w) {
#pragma unroll
      for (int hb = 0; hb < 2; ++hb)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int hid = hb * 32 + rowmap(q, h);
#pragma unroll
          for (int ib = 0; ib < IB; ++ib) {
            float* d1 = &sW1[hid * LD1 + 32 * ib + r];
            if (w == 0) *d1 = aW1[hb][ib][q]; else *d1 += aW1[hb][ib][q];
          }
          if (r == 0) { if (w == 0) sB[hid] = aW2[hb][q]; else sB[hid] += aW2[hb][q]; }
        }
    }
  }
  __syncthreads();
  float* P = partials + (size_t)blockIdx.x * per_block;  // [64 IN | gW2 64 | 64 zeros | 0]
  const int nW1 = 64 * IN;
  for (int e = tid; e < nW1; e += 256) P[e] = sW1[(e / IN) * LD1 + (e % IN)];
  if (tid < 64) { P[nW1 + tid] = sB[tid]; P[nW1 + 64 + tid] = 0.f; }
  if (tid == 0) P[nW1 + 128] = 0.f;
}

// f(NS, IB) as integral constants for the <NS, IB> classes that exist (mlp_plan)
template <typename F>
int with_h64o1_class(const Plan& p, F&& f) {
  using std::integral_constant;
  if (p.h64_ib == 1) return with_class<6, 16>(p.h64_ns, "decoder MLP", [&](auto ns) { return f(ns, integral_constant<int, 1>{}); });
  return with_class<18, 32>(p.h64_ns, "decoder MLP", [&](auto ns) { return f(ns, integral_constant<int, 2>{}); });
}

}  // namespace

int launch_fwd_h64o1(const Plan& p, int grid, hipStream_t st, long long N, int IN, const float* x, const float* W1,
                     const float* b1, const float* W2, const float* b2, float* y) {
  return with_class<6, 10, 18>(p.fwd_ks, "decoder MLP", [&](auto ks) {
    return launch(mlp_fwd_h64o1_kernel<ks()>, dim3(grid), 256, 0, st, N, IN, x, W1, b1, W2, b2, y);
  });
}

int launch_bwd_h64o1(const Plan& p, int grid, hipStream_t st, long long N, int IN, const float* x, const float* gy,
                     const float* W1, const float* b1, const float* W2, float* gx, float* partials, size_t per_block) {
  return with_h64o1_class(p, [&](auto ns, auto ib) {
    return launch(mlp_bwd_wave_h64o1_kernel<ns(), ib(), 0>, dim3(grid), 256, 0, st, N, IN, x, gy, W1, b1, W2, gx,
                  partials, per_block);
  });
}

int launch_dbl_h64o1(const Plan& p, int grid, hipStream_t st, long long N, int IN, const float* x, const float* a,
                     const float* gy, const float* W1, const float* b1, const float* W2, float* ggy, float* partials,
                     size_t per_block) {
  return with_h64o1_class(p, [&](auto ns, auto ib) {
    return launch(mlp_dbl_wave_h64o1_kernel<ns(), ib()>, dim3(grid), 256, 0, st, N, IN, x, a, gy, W1, b1, W2, ggy,
                  partials, per_block);
  });
}

}  // namespace mlp
}  // namespace pings
