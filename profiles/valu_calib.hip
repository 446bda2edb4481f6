// Vector-ALU issue rate of gfx950, measured: how many wave64 fp32 instructions per second the chip sustains when every
// SIMD holds many waves that do nothing else.  Calibrates the "valu" roofline of bench.py (the blend kernels are bound
// by it), the way pmc_calib.hip calibrates the HBM counters.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Ipings_amd/csrc -o profiles/_build/valu_calib profiles/valu_calib.hip \
//     && profiles/_build/valu_calib
// Kernels: 16 independent accumulators per lane, ITER rounds of one instruction per accumulator.
//   fma      v_fma_f32            (plain fp32)
//   pk_fma   v_pk_fma_f32         (two fp32 per lane and instruction)
//   mix      12 v_fma_f32 + 2 v_exp_f32 + 2 v_rcp_f32 per round (roughly the blend loop's transcendental share)
//   pk_mix   12 v_pk_fma_f32 + 2 v_exp_f32 + 2 v_rcp_f32 per round (the mix with its fmas packed: 24 fp32 fmas)
//   mix24    24 v_fma_f32 + 2 v_exp_f32 + 2 v_rcp_f32 per round (the same fp32 work as pk_mix, unpacked)
// pk_mix against mix24 answers whether packing pays inside a loop that also issues transcendentals: both do the same
// 24 fmas and 4 transcendentals per round, so their rate in rounds is the figure (G wave-rounds/s, whole chip).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "raster_common.hpp"   // wave_reduce16, wave_reduce16_swap (device inlines only; nothing of the library is linked)

using f2 = __attribute__((ext_vector_type(2))) float;
constexpr int ITER = 4096;

__global__ __launch_bounds__(256) void k_fma(float* out, float x, float y) {
  float a[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) a[i] = (float)(threadIdx.x + i);
  for (int it = 0; it < ITER; ++it) {
#pragma unroll
    for (int i = 0; i < 16; ++i) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(x), "v"(y));   // (the compiler packs plain C)
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += a[i];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_pk_fma(float* out, float x, float y) {
  f2 a[16];
  const f2 xx = {x, x}, yy = {y, y};
#pragma unroll
  for (int i = 0; i < 16; ++i) a[i] = (f2){(float)(threadIdx.x + i), (float)i};
  for (int it = 0; it < ITER; ++it) {
#pragma unroll
    for (int i = 0; i < 16; ++i) asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(xx), "v"(yy));
  }
  f2 s = {0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 16; ++i) s += a[i];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s.x + s.y;
}

__global__ __launch_bounds__(256) void k_mix(float* out, float x, float y) {
  float a[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) a[i] = 0.001f * (float)(threadIdx.x + i);
  for (int it = 0; it < ITER; ++it) {
#pragma unroll
    for (int i = 0; i < 12; ++i) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(x), "v"(y));
    asm volatile("v_exp_f32 %0, %0" : "+v"(a[12]));
    asm volatile("v_exp_f32 %0, %0" : "+v"(a[13]));
    asm volatile("v_rcp_f32 %0, %0" : "+v"(a[14]));
    asm volatile("v_rcp_f32 %0, %0" : "+v"(a[15]));
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += a[i];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_pk_mix(float* out, float x, float y) {
  f2 a[12];
  float e[4];
  const f2 xx = {x, x}, yy = {y, y};
#pragma unroll
  for (int i = 0; i < 12; ++i) a[i] = (f2){0.001f * (float)(threadIdx.x + i), 0.002f * (float)i};
#pragma unroll
  for (int i = 0; i < 4; ++i) e[i] = 0.001f * (float)(threadIdx.x + 12 + i);
  for (int it = 0; it < ITER; ++it) {
#pragma unroll
    for (int i = 0; i < 12; ++i) asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(xx), "v"(yy));
    asm volatile("v_exp_f32 %0, %0" : "+v"(e[0]));
    asm volatile("v_exp_f32 %0, %0" : "+v"(e[1]));
    asm volatile("v_rcp_f32 %0, %0" : "+v"(e[2]));
    asm volatile("v_rcp_f32 %0, %0" : "+v"(e[3]));
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 12; ++i) s += a[i].x + a[i].y;
#pragma unroll
  for (int i = 0; i < 4; ++i) s += e[i];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_mix24(float* out, float x, float y) {
  float a[24], e[4];
#pragma unroll
  for (int i = 0; i < 24; ++i) a[i] = 0.001f * (float)(threadIdx.x + i);
#pragma unroll
  for (int i = 0; i < 4; ++i) e[i] = 0.001f * (float)(threadIdx.x + 24 + i);
  for (int it = 0; it < ITER; ++it) {
#pragma unroll
    for (int i = 0; i < 24; ++i) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(x), "v"(y));
    asm volatile("v_exp_f32 %0, %0" : "+v"(e[0]));
    asm volatile("v_exp_f32 %0, %0" : "+v"(e[1]));
    asm volatile("v_rcp_f32 %0, %0" : "+v"(e[2]));
    asm volatile("v_rcp_f32 %0, %0" : "+v"(e[3]));
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 24; ++i) s += a[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) s += e[i];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

// The lane swaps of gfx950 and the two 16 x 64 reduce-scatters built on them (raster_common.hpp).
//   swap32 / swap16   8 independent v_permlane32_swap / v_permlane16_swap per round behind one s_nop 1 (the two wait
//                     states a swap needs after a VALU write of its operands), 16 registers
//   red_none          16 v_pk_mul_f32 that renew the 16 packed accumulators, nothing else: the rounds' common part
//   red_dpp           + 16 folds + wave_reduce16      (the class-2 backward before r12, the forward kernels)
//   red_swap          + wave_reduce16_swap<false>     (surfel)
//   red_swap_zero6    + wave_reduce16_swap<true>      (3DGS: six slots zero)
// The reductions of successive rounds do not depend on each other (the totals go to a separate sum).
template <int ROWS>
__global__ __launch_bounds__(256) void k_swap(float* out, float x, float y) {
  float a[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) a[i] = x * (float)(threadIdx.x + i) + y;
  for (int it = 0; it < ITER; ++it) {
    if (ROWS == 32)
      PINGS_SWAP8("v_permlane32_swap_b32", a[0], a[8], a[1], a[9], a[2], a[10], a[3], a[11], a[4], a[12], a[5], a[13],
                  a[6], a[14], a[7], a[15]);
    else
      PINGS_SWAP8("v_permlane16_swap_b32", a[0], a[8], a[1], a[9], a[2], a[10], a[3], a[11], a[4], a[12], a[5], a[13],
                  a[6], a[14], a[7], a[15]);
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += a[i];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <int VARIANT>   // 0 none, 1 fold + wave_reduce16, 2 wave_reduce16_swap<false>, 3 wave_reduce16_swap<true>
__global__ __launch_bounds__(256) void k_red(float* out, float x, float y) {
  using namespace pings::raster;
  const int lane = threadIdx.x & 63;
  f2 v2[16];
  const f2 xx = {x, x};
#pragma unroll
  for (int i = 0; i < 16; ++i) v2[i] = (f2){y * (float)(threadIdx.x + i), y * (float)(i + 1)};
  float s = 0.f;
  for (int it = 0; it < ITER; ++it) {
#pragma unroll
    for (int i = 0; i < 16; ++i) asm volatile("v_pk_mul_f32 %0, %0, %1" : "+v"(v2[i]) : "v"(xx));
    if (VARIANT == 1) {
      float v[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) v[q] = v2[q].x + v2[q].y;
      s += wave_reduce16(v, lane);
    } else if (VARIANT == 2) {
      s += wave_reduce16_swap<false>(v2, lane);
    } else if (VARIANT == 3) {
      s += wave_reduce16_swap<true>(v2, lane);
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) s += v2[i].x + v2[i].y;
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <typename K>
double run(K kernel, int blocks, float* out) {
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, 0, out, 0.999f, 0.001f);
  (void)hipDeviceSynchronize();
  (void)hipEventRecord(e0, 0);
  for (int r = 0; r < 5; ++r) hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, 0, out, 0.999f, 0.001f);
  (void)hipEventRecord(e1, 0);
  (void)hipEventSynchronize(e1);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  return ms / 5.0 * 1e-3;
}

int main() {
  hipDeviceProp_t p;
  (void)hipGetDeviceProperties(&p, 0);
  const int cus = p.multiProcessorCount;
  float* out;
  (void)hipMalloc(&out, sizeof(float) * 256 * cus * 8 * 4);
  printf("{\"device\": \"%s\", \"cus\": %d, \"clock_mhz\": %d, \"results\": [", p.gcnArchName, cus, p.clockRate / 1000);
  bool first = true;
  for (int wps : {1, 2, 3, 4, 8}) {                         // waves per SIMD
    const int blocks = cus * wps;                        // 256 threads = 4 waves = one per SIMD of a CU
    const double waves = (double)blocks * 4;
    const double insts = waves * ITER * 16;              // wave-instructions of the measured kind per launch
    const double t_f = run(k_fma, blocks, out), t_p = run(k_pk_fma, blocks, out), t_m = run(k_mix, blocks, out);
    const double t_pm = run(k_pk_mix, blocks, out), t_m24 = run(k_mix24, blocks, out);
    const double rounds = waves * ITER;                  // wave-rounds of 24 fp32 fmas + 4 transcendentals
    printf("%s{\"waves_per_simd\": %d, \"fma_Ginst_s\": %.1f, \"pk_fma_Ginst_s\": %.1f, \"mix_Ginst_s\": %.1f, "
           "\"pk_mix_Ginst_s\": %.1f, \"pk_mix_Grounds_s\": %.2f, \"mix24_Grounds_s\": %.2f, ", first ? "" : ", ",
           wps, insts / t_f / 1e9, insts / t_p / 1e9, insts / t_m / 1e9, insts / t_pm / 1e9, rounds / t_pm / 1e9,
           rounds / t_m24 / 1e9);
    // swaps: 8 per round; cycles per wave instruction and SIMD = nominal clock x SIMDs / rate (the clock under load is
    // lower than the nominal one, so the RATIO to the fma figure is what carries over)
    const double t_s32 = run(k_swap<32>, blocks, out), t_s16 = run(k_swap<16>, blocks, out);
    const double swaps = waves * ITER * 8;
    const double t_r0 = run(k_red<0>, blocks, out), t_r1 = run(k_red<1>, blocks, out), t_r2 = run(k_red<2>, blocks, out);
    const double t_r3 = run(k_red<3>, blocks, out);
    // ns per wave-round on one SIMD: time x SIMDs / rounds
    const double simds = (double)cus * 4, ns = 1e9 * simds / rounds, cyc = (double)p.clockRate * 1e3 * simds;
    printf("\"swap32_Ginst_s\": %.1f, \"swap16_Ginst_s\": %.1f, \"fma_cycles\": %.2f, \"pk_fma_cycles\": %.2f, "
           "\"swap32_cycles\": %.2f, \"swap16_cycles\": %.2f, "
           "\"red_none_ns\": %.2f, \"red_dpp_ns\": %.2f, \"red_swap_ns\": %.2f, \"red_swap_zero6_ns\": %.2f}",
           swaps / t_s32 / 1e9, swaps / t_s16 / 1e9, cyc * t_f / insts, cyc * t_p / insts, cyc * t_s32 / swaps,
           cyc * t_s16 / swaps, t_r0 * ns, t_r1 * ns, t_r2 * ns, t_r3 * ns);
    first = false;
  }
  printf("]}\n");
  (void)hipFree(out);
  return 0;
}
