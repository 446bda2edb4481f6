// Shared helpers for the libpings_hip translation units (device + host).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "pings_hip.h"

namespace pings {

void set_error(const char* fmt, ...);  // abi.hip

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

template <typename T>
__host__ __device__ constexpr T ceil_div(T a, T b) { return (a + b - 1) / b; }

constexpr int kWave = 64;  // gfx950 wavefront

inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// Bump allocator over a caller-owned scratch blob: every field starts on a 256-byte boundary.  With base == nullptr it
// only measures, so one carve function gives both the exported size (carve(nullptr, ...).total) and the placement.
// take reserves what it is asked for: a field that must not be empty is asked for with `n > 0 ? n : 1`.
struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* p) : base(static_cast<char*>(p)) {}
  template <class T>
  T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += align_up(count * sizeof(T));
    return p;
  }
  size_t total() const { return off; }
};

#if defined(__HIPCC__)
// Exclusive scan of one int per thread over a workgroup of Block threads (whole waves); *total = the workgroup's sum.
// Every thread of the workgroup calls it.
template <int Block>
__device__ inline int block_exclusive_scan(int x, int* total) {
  constexpr int kWaves = Block / kWave;
  __shared__ int wsum[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = x;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(incl, off, 64);
    if (lane >= off) incl += y;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    before += w < wave ? wsum[w] : 0;
    all += wsum[w];
  }
  __syncthreads();
  *total = all;
  return before + incl - x;
}
#endif

// Stream-ordered read of up to 8 device words (32 bit each) into host memory WITHOUT a blocking wait inside the HIP
// runtime: one wave copies the words into pinned, device-mapped host memory behind everything already queued on `st` and
// the host polls a sequence number (abi.hip).  A blocking hipStreamSynchronize wakes through an interrupt, which on one
// box of the pool arrived only with a 60 Hz tick (16 ms per wait); polling does not depend on it and costs a few
// microseconds on every box.  Returns a PINGS status.
int host_read_words(const uint32_t* const* dev_words, int n, uint32_t* out, hipStream_t st);

// Optional per-stage HIP-event timing (off by default; bench.py turns it on to get the
// per-kernel durations its roofline figures are computed from).
namespace prof {
bool enabled(const char* name);
void begin(const char* name, hipStream_t st);
void end(hipStream_t st);
struct Scope {
  hipStream_t st;
  bool on;
  Scope(const char* name, hipStream_t s) : st(s), on(enabled(name)) { if (on) begin(name, st); }
  ~Scope() { if (on) end(st); }
};
}  // namespace prof

}  // namespace pings

// Every C-ABI entry point returns 0 on success; HIP failures are turned into
// PINGS_ERR_HIP with a message retrievable through pings_last_error().
#define PINGS_HIP_CHECK(expr)                                                        \
  do {                                                                               \
    hipError_t _e = (expr);                                                          \
    if (_e != hipSuccess) {                                                          \
      pings::set_error("%s:%d %s -> %s", __FILE__, __LINE__, #expr,                  \
                       hipGetErrorString(_e));                                       \
      return PINGS_ERR_HIP;                                                          \
    }                                                                                \
  } while (0)

#define PINGS_LAUNCH_CHECK() PINGS_HIP_CHECK(hipGetLastError())

#define PINGS_ARG_CHECK(cond, msg)                                                   \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      pings::set_error("%s:%d invalid argument: %s (%s)", __FILE__, __LINE__, msg,   \
                       #cond);                                                       \
      return PINGS_ERR_ARG;                                                          \
    }                                                                                \
  } while (0)

namespace pings {

// Returns f(std::integral_constant<int, V>{}), a PINGS status, for the V among Vs that equals v: where a planned class
// becomes a kernel template argument (`[&](auto ks) { ... kernel<ks()> ... }`).  Only the listed classes are
// instantiated; a class with no kernel is an error, never another kernel.  `what` names the path in the error text.
template <int... Vs, typename F>
int with_class(int v, const char* what, F&& f) {
  int e = PINGS_ERR_ARG;
  if (!((v == Vs ? (e = f(std::integral_constant<int, Vs>{}), true) : false) || ...))
    set_error("%s: no kernel is built for class %d", what, v);
  return e;
}

// the same for a flag that is a kernel template argument: f(std::true_type{}) or f(std::false_type{})
template <typename F>
int with_flag(bool v, F&& f) { return v ? f(std::true_type{}) : f(std::false_type{}); }

// hipLaunchKernelGGL and the launch check, as a PINGS status
template <typename... KA, typename... A>
int launch(void (*kernel)(KA...), dim3 grid, int nthreads, size_t lds, hipStream_t st, A... args) {
  hipLaunchKernelGGL(kernel, grid, dim3(nthreads), lds, st, args...);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

}  // namespace pings
