// Decoder MLP, workgroup kernels: a workgroup of NW = HID / 32 waves walks 32-row tiles, weights staged in LDS, wave w
// owns hidden units 32w .. 32w+31 (the decomposition mlp.hip describes).  They run every shape the wave kernels do not
// take (mlp_plan); on HID = 128, IN <= 32 the wave kernels measured 28 / 45 / 55 / 60 TFLOP/s against 22 / 31 / 34 / 35
// here.
#include "mlp_common.hpp"

namespace pings {
namespace mlp {
namespace {

// ---------------------------------------------------------------- forward
template <int PF_X>
__global__ __launch_bounds__(256) void mlp_fwd_kernel(Dims d, const float* __restrict__ x, const float* __restrict__ W1,
                               const float* __restrict__ b1, const float* __restrict__ W2,
                               const float* __restrict__ b2, float* __restrict__ y) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int NW = d.HID / 32, nthreads = NW * 64;
  float* sW1 = lds;                                  // [HID][ldw1]
  float* sW2 = sW1 + d.HID * d.ldw1;                 // [OUTP][ldw2]
  float* sX = sW2 + OUTP * d.ldw2;                   // [TR][ldx]
  float* sY = sX + TR * d.ldx;                       // [NW][OUTP][TR+1]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;

  for (int e = tid; e < d.HID * d.INP; e += nthreads) {
    const int j = e / d.INP, i = e - j * d.INP;
    sW1[j * d.ldw1 + i] = i < d.IN ? W1[(size_t)j * d.IN + i] : 0.f;
  }
  for (int e = tid; e < OUTP * d.HID; e += nthreads) {
    const int o = e / d.HID, j = e - o * d.HID;
    sW2[o * d.ldw2 + j] = o < d.OUT ? W2[(size_t)o * d.HID + j] : 0.f;
  }
  float bias1[16];
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) bias1[reg] = b1[wave * 32 + rowmap(reg, h)];

  const long long ntiles = (d.N + TR - 1) / TR;
  // The next tile of x is fetched into registers while the current one is multiplied (one wave per SIMD:
  // without this the matrix pipe idles for the whole HBM round trip of every tile).
  float px[PF_X];
  auto fetch = [&](long long t) {
#pragma unroll
    for (int u = 0; u < PF_X; ++u) {
      const int e = tid + u * nthreads;
      const int rr = e / d.INP, i = e - rr * d.INP;
      const long long gr = t * TR + rr;
      px[u] = (e < TR * d.INP && gr < d.N && i < d.IN) ? x[(size_t)gr * d.IN + i] : 0.f;
    }
  };
  if ((long long)blockIdx.x < ntiles) fetch(blockIdx.x);
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long row0 = t * TR;
    __syncthreads();  // previous tile's sX / sY consumed (also orders the weight staging on the first trip)
#pragma unroll
    for (int u = 0; u < PF_X; ++u) {
      const int e = tid + u * nthreads;
      if (e < TR * d.INP) {
        const int rr = e / d.INP, i = e - rr * d.INP;
        sX[rr * d.ldx + i] = px[u];
      }
    }
    __syncthreads();
    if (t + gridDim.x < ntiles) fetch(t + gridDim.x);
    f32x16 acc = {0};
    {
      // the trip count is a kernel argument, which keeps hipcc from unrolling an MFMA loop: groups of four with a
      // static inner loop let it issue the eight LDS operand reads of a group together, ahead of the four MFMAs
      const float* pa = sW1 + (wave * 32 + r) * d.ldw1 + h;
      const float* pb = sX + r * d.ldx + h;
      const int half = d.INP / 2;
      int s = 0;
      for (; s + 4 <= half; s += 4) {
        float a4[4], b4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { a4[u] = pa[2 * (s + u)]; b4[u] = pb[2 * (s + u)]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = mfma(a4[u], b4[u], acc);
      }
      for (; s < half; ++s) acc = mfma(pa[2 * s], pb[2 * s], acc);
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) acc[reg] = fmaxf(acc[reg] + bias1[reg], 0.f);
    f32x16 acc2 = {0};
#pragma unroll
    for (int s = 0; s < 16; ++s)
      acc2 = mfma(sW2[r * d.ldw2 + wave * 32 + rowmap(s, h)], acc[s], acc2);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) sY[(wave * OUTP + rowmap(reg, h)) * (TR + 1) + r] = acc2[reg];
    __syncthreads();
    for (int e = tid; e < TR * d.OUT; e += nthreads) {
      const int rr = e / d.OUT, o = e - rr * d.OUT;
      const long long gr = row0 + rr;
      if (gr < d.N) {
        float v = b2[o];
        for (int w = 0; w < NW; ++w) v += sY[(w * OUTP + o) * (TR + 1) + rr];
        y[(size_t)gr * d.OUT + o] = v;
      }
    }
  }
}

// ---------------------------------------------------------------- backward
template <int PF_X, int PF_G>
__global__ __launch_bounds__(256) void mlp_bwd_kernel(Dims d, const float* __restrict__ x, const float* __restrict__ gy,
                               const float* __restrict__ W1, const float* __restrict__ b1,
                               const float* __restrict__ W2, float* __restrict__ gx,
                               float* __restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int NW = d.HID / 32, nthreads = NW * 64;
  const int NIB = (d.INP + 31) / 32;                 // 32-wide blocks of the input dimension (1 or 2)
  float* sW1 = lds;                                  // [HID][ldw1]
  float* sW2 = sW1 + d.HID * d.ldw1;                 // [OUTP][ldw2]
  float* sX = sW2 + OUTP * d.ldw2;                   // [TR][ldx]
  float* sGY = sX + TR * d.ldx;                      // [TR][ldg]
  float* sHT = sGY + TR * d.ldg;                     // [NW][32 hid][TR+1]
  float* sGH = sHT + NW * 32 * (TR + 1);             // [NW][32 hid][TR+1]
  float* sGX = sGH + NW * 32 * (TR + 1);             // [NW][NIB*32][TR+1]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;

  for (int e = tid; e < d.HID * d.INP; e += nthreads) {
    const int j = e / d.INP, i = e - j * d.INP;
    sW1[j * d.ldw1 + i] = i < d.IN ? W1[(size_t)j * d.IN + i] : 0.f;
  }
  for (int e = tid; e < OUTP * d.HID; e += nthreads) {
    const int o = e / d.HID, j = e - o * d.HID;
    sW2[o * d.ldw2 + j] = o < d.OUT ? W2[(size_t)o * d.HID + j] : 0.f;
  }
  float bias1[16];
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) bias1[reg] = b1[wave * 32 + rowmap(reg, h)];

  // persistent accumulators of this wave's 32 hidden units
  f32x16 aW2T = {0};          // gW2^T tile: [hid (rows, reg map)] x [o (lane)]
  f32x16 aW1a = {0}, aW1b = {0};  // gW1 tiles: [hid] x [i 0..31], [hid] x [i 32..63]
  f32x16 aB1 = {0};           // per-lane (row) partial of gb1 for hid = rowmap(reg, h)
  float aB2 = 0.f;            // thread o < OUT of wave 0: column sum of gY

  float* myHT = sHT + wave * 32 * (TR + 1);
  float* myGH = sGH + wave * 32 * (TR + 1);
  float* myGX = sGX + wave * NIB * 32 * (TR + 1);

  const long long ntiles = (d.N + TR - 1) / TR;
  // next tile of x / gY prefetched into registers during the current tile's products
  float px[PF_X], pg[PF_G];
  auto fetch = [&](long long t) {
#pragma unroll
    for (int u = 0; u < PF_X; ++u) {
      const int e = tid + u * nthreads;
      const int rr = e / d.INP, i = e - rr * d.INP;
      const long long gr = t * TR + rr;
      px[u] = (e < TR * d.INP && gr < d.N && i < d.IN) ? x[(size_t)gr * d.IN + i] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < PF_G; ++u) {
      const int e = tid + u * nthreads;
      const int rr = e / OUTP, o = e - rr * OUTP;
      const long long gr = t * TR + rr;
      pg[u] = (e < TR * OUTP && gr < d.N && o < d.OUT) ? gy[(size_t)gr * d.OUT + o] : 0.f;
    }
  };
  if ((long long)blockIdx.x < ntiles) fetch(blockIdx.x);
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long row0 = t * TR;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PF_X; ++u) {
      const int e = tid + u * nthreads;
      if (e < TR * d.INP) {
        const int rr = e / d.INP, i = e - rr * d.INP;
        sX[rr * d.ldx + i] = px[u];
      }
    }
#pragma unroll
    for (int u = 0; u < PF_G; ++u) {
      const int e = tid + u * nthreads;
      if (e < TR * OUTP) {
        const int rr = e / OUTP, o = e - rr * OUTP;
        sGY[rr * d.ldg + o] = pg[u];
      }
    }
    __syncthreads();
    if (t + gridDim.x < ntiles) fetch(t + gridDim.x);
    if (wave == 0 && lane < d.OUT) {
      float s = 0.f;
      for (int rr = 0; rr < TR; ++rr) s += sGY[rr * d.ldg + lane];
      aB2 += s;
    }
    // H^T (hidden units of this wave) for the tile's rows
    f32x16 hT = {0};
    {
      const float* pa = sW1 + (wave * 32 + r) * d.ldw1 + h;
      const float* pb = sX + r * d.ldx + h;
      const int half = d.INP / 2;
      int s = 0;
      for (; s + 4 <= half; s += 4) {
        float a4[4], b4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { a4[u] = pa[2 * (s + u)]; b4[u] = pb[2 * (s + u)]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) hT = mfma(a4[u], b4[u], hT);
      }
      for (; s < half; ++s) hT = mfma(pa[2 * s], pb[2 * s], hT);
    }
    // gH^T = W2^T gY^T  (A = W2^T: row = hid on the lane, k = o)
    f32x16 gT = {0};
#pragma unroll
    for (int s = 0; s < OUTP / 2; ++s)
      gT = mfma(sW2[(2 * s + h) * d.ldw2 + wave * 32 + r], sGY[r * d.ldg + 2 * s + h], gT);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const float pre = hT[reg] + bias1[reg];
      hT[reg] = fmaxf(pre, 0.f);
      gT[reg] = pre > 0.f ? gT[reg] : 0.f;
      aB1[reg] += gT[reg];
    }
    // gX^T partial of this wave: [i, row] = sum_{hid in wave} W1[hid][i] gH^T[hid][row]
    //   A = W1^T: row = i on the lane, k = hid in accumulator order; B = the gH^T accumulator
    if (gx) {
      for (int ib = 0; ib < NIB; ++ib) {
        f32x16 ax = {0};
        const int i = ib * 32 + r;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
          const float a = i < d.INP ? sW1[(wave * 32 + rowmap(s, h)) * d.ldw1 + i] : 0.f;
          ax = mfma(a, gT[s], ax);
        }
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) myGX[(ib * 32 + rowmap(reg, h)) * (TR + 1) + r] = ax[reg];
      }
    }
    // transpose H^T / gH^T through LDS: element [hid (reg map)][row (lane)]
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      myHT[rowmap(reg, h) * (TR + 1) + r] = hT[reg];
      myGH[rowmap(reg, h) * (TR + 1) + r] = gT[reg];
    }
    __builtin_amdgcn_wave_barrier();
    // gW2^T[hid][o] += sum_row H^T[hid][row] gY[row][o]   (A: row = hid on the lane, k = data row)
    // gW1[hid][i]   += sum_row gH^T[hid][row] x[row][i]
#pragma unroll
    for (int s = 0; s < TR / 2; ++s) {
      const int k = 2 * s + h;
      const float aH = myHT[r * (TR + 1) + k];
      const float aG = myGH[r * (TR + 1) + k];
      aW2T = mfma(aH, sGY[k * d.ldg + r], aW2T);
      aW1a = mfma(aG, r < d.INP ? sX[k * d.ldx + r] : 0.f, aW1a);
      if (NIB > 1) aW1b = mfma(aG, (32 + r) < d.INP ? sX[k * d.ldx + 32 + r] : 0.f, aW1b);
    }
    __syncthreads();
    if (gx) {
      for (int e = tid; e < TR * d.IN; e += nthreads) {
        const int rr = e / d.IN, i = e - rr * d.IN;
        const long long gr = row0 + rr;
        if (gr < d.N) {
          float v = 0.f;
          for (int w = 0; w < NW; ++w) v += sGX[(w * NIB * 32 + i) * (TR + 1) + rr];
          gx[(size_t)gr * d.IN + i] = v;
        }
      }
    }
  }

  // ---- write this workgroup's partial weight gradients
  float* P = partials + (size_t)blockIdx.x * partial_floats(d.IN, d.HID, d.OUT);
  float* pW1 = P;
  float* pW2 = pW1 + (size_t)d.HID * d.IN;
  float* pB1 = pW2 + (size_t)d.OUT * d.HID;
  float* pB2 = pB1 + d.HID;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int hid = wave * 32 + rowmap(reg, h);
    if (r < d.OUT) pW2[(size_t)r * d.HID + hid] = aW2T[reg];           // lane = o
    if (r < d.IN) pW1[(size_t)hid * d.IN + r] = aW1a[reg];             // lane = i
    if (NIB > 1 && 32 + r < d.IN) pW1[(size_t)hid * d.IN + 32 + r] = aW1b[reg];
  }
  // gb1: sum the per-row partials over the 32 lanes that share h
  __syncthreads();
  float* sRed = sHT;  // reuse: [NW][64 lanes][16]
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) sRed[(wave * 64 + lane) * 17 + reg] = aB1[reg];
  __syncthreads();
  for (int e = tid; e < d.HID; e += nthreads) {
    const int w = e >> 5, m = e & 31;          // hidden unit m of wave w: find (reg, hh) with rowmap = m
    const int hh = (m >> 2) & 1, reg = (m & 3) + 4 * (m >> 3);
    float s = 0.f;
    for (int l = 0; l < 32; ++l) s += sRed[(w * 64 + hh * 32 + l) * 17 + reg];
    pB1[e] = s;
  }
  if (wave == 0 && lane < d.OUT) pB2[lane] = aB2;
}

size_t fwd_lds_bytes(const Dims& d) {
  const int NW = d.HID / 32;
  return sizeof(float) * ((size_t)d.HID * d.ldw1 + (size_t)OUTP * d.ldw2 + (size_t)TR * d.ldx +
                          (size_t)NW * OUTP * (TR + 1));
}

size_t bwd_lds_bytes(const Dims& d) {
  const int NW = d.HID / 32, NIB = (d.INP + 31) / 32;
  size_t tail = (size_t)2 * NW * 32 * (TR + 1) + (size_t)NW * NIB * 32 * (TR + 1);
  const size_t red = (size_t)NW * 64 * 17;  // gb1 reduction reuses the sHT/sGH region
  if (tail < red) tail = red;
  return sizeof(float) * ((size_t)d.HID * d.ldw1 + (size_t)OUTP * d.ldw2 + (size_t)TR * d.ldx +
                          (size_t)TR * d.ldg + tail);
}

// The kernels' LDS exceeds the 64 KB a kernel may ask for without saying so.
template <typename... KA, typename... A>
int launch_wg(void (*kernel)(KA...), int grid, size_t lds, hipStream_t st, const Dims& d, A... args) {
  PINGS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds));
  return launch(kernel, dim3(grid), 64 * (d.HID / 32), lds, st, d, args...);
}

}  // namespace

int launch_fwd_wg(const Plan& p, int grid, hipStream_t st, const Dims& d, const float* x, const float* W1,
                  const float* b1, const float* W2, const float* b2, float* y) {
  return with_class<5, 10, 18, 32>(p.fwd_pfx, "decoder MLP", [&](auto px) {
    return launch_wg(mlp_fwd_kernel<px()>, grid, fwd_lds_bytes(d), st, d, x, W1, b1, W2, b2, y);
  });
}

int launch_bwd_wg(const Plan& p, int grid, hipStream_t st, const Dims& d, const float* x, const float* gy,
                  const float* W1, const float* b1, const float* W2, float* gx, float* partials) {
  auto launch = [&](auto px, auto pg) {
    return launch_wg(mlp_bwd_kernel<px(), pg()>, grid, bwd_lds_bytes(d), st, d, x, gy, W1, b1, W2, gx, partials);
  };
  using std::integral_constant;   // the <PF_X, PF_G> classes that exist: PF_G follows the thread count (mlp_plan)
  switch (p.bwd_pfg) {
    case 4: return with_class<5, 9>(p.bwd_pfx, "decoder MLP", [&](auto px) { return launch(px, integral_constant<int, 4>{}); });
    case 6: return with_class<6, 11>(p.bwd_pfx, "decoder MLP", [&](auto px) { return launch(px, integral_constant<int, 6>{}); });
    case 8: return with_class<9, 16>(p.bwd_pfx, "decoder MLP", [&](auto px) { return launch(px, integral_constant<int, 8>{}); });
    default: return with_class<18, 32>(p.bwd_pfx, "decoder MLP", [&](auto px) { return launch(px, integral_constant<int, 16>{}); });
  }
}

}  // namespace mlp
}  // namespace pings
