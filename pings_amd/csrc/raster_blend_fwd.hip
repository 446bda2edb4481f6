// Gaussian(-surfel) rasteriser, forward blend kernels, for gfx950.
//
//   blend_fwd_wave_kernel   one independent wave per 8x8 quadrant (the default); long tile lists in parallel segments
//   blend_fwd_tile_kernel   one wave per 16x16 tile, four pixels per lane
//   per-Gaussian sums       `contributions` / `n_touched` are reduced per (tile, Gaussian) instance on chip (DPP wave
//                           sum + LDS), stored once per instance, then summed per Gaussian: no global atomics
//
// blend_plan (raster_layout.hip) decides which of them a view runs; launch_blend_fwd at the end of this file launches them.
#include "raster_common.hpp"

namespace pings {
namespace raster {

// ---------------------------------------------------------------- forward, one independent wave per 8x8 quadrant
// Footprint class 1 (footprints of a few tiles).  A 16x16 tile is four 8x8 quadrants; wave q of a workgroup owns
// quadrant q (qx = q & 1, qy = q >> 1) of the workgroup's tile, lane l the pixel (l & 7, l >> 3) of it.  Sub-tile
// culling: a record whose footprint ellipse (alpha >= 1/255) cannot reach the wave's quadrant would contribute
// exactly zero to its pixels, so skipping it leaves the outputs unchanged bit for bit; a wave visits only ~37 % of
// a tile's records on a street-like scene.  As the four culled lists of a tile differ that much in length, the waves
// share nothing that would make them wait for each other (a kernel whose four waves staged the list together in
// rounds idled at the round barriers and could not stop before the slowest one).  Every wave
// walks the tile list by itself: 64 entries at a time it fetches slot -> Gaussian -> record (the next window is in
// flight while the current one is blended), tests the footprint against ITS quadrant, compacts the survivors into
// its own LDS slots and blends them front to back; it stops as soon as its 64 pixels are done.  No barriers.
// Per-instance sums are written per quadrant (inst_wq / inst_cntq) and folded by combine_quadrants_kernel into
// inst_w / inst_cnt / inst_qmask, which is all that the kernels downstream read.
// Workgroups of four waves, wave = quadrant of ONE tile: the four walk the same list, so what one fetched (list entries,
// ids, records) the others find in the CU's L1; as one-wave workgroups the four quadrants of a tile were dealt to four
// XCDs (round-robin dispatch) and each fetched the list through its own L2.
template <int MODE>
__device__ __forceinline__ void blend_fwd_wave_body(
    const KParams& p, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
    const float4* __restrict__ rec, const uint32_t* __restrict__ gval, float* __restrict__ out_color,
    float* __restrict__ out_normal, float* __restrict__ out_depth, float* __restrict__ out_alpha,
    float* __restrict__ final_T, uint32_t* __restrict__ n_contrib, float* __restrict__ inst_wq,
    uint32_t* __restrict__ inst_cntq, const uint32_t* __restrict__ tile_order,
    const uint32_t* __restrict__ seg_tile_unit0, const unsigned block) {
  __shared__ float4 sA_[4][64], sB_[4][64], sC_[4][64], sD_[4][64];
  __shared__ uint32_t sSlot_[4][64];
  __shared__ int sE_[4][64];
  __shared__ float sW_[4][64];
  __shared__ uint32_t sCnt_[4][64];

  const int lane = threadIdx.x & 63, q = (int)(threadIdx.x >> 6);
  float4 *sA = sA_[q], *sB = sB_[q], *sC = sC_[q], *sD = sD_[q];
  uint32_t *sSlot = sSlot_[q], *sCnt = sCnt_[q];
  int* sE = sE_[q];
  float* sW = sW_[q];
  const int tile = (int)tile_order[block];
  if (seg_tile_unit0 && seg_tile_unit0[tile] != 0xFFFFFFFFu) return;   // a long list: blended in parallel segments
  const int tx = tile % p.gx, ty = tile / p.gx;
  const int pix_x = tx * TILE + 8 * (q & 1) + (lane & 7);
  const int pix_y = ty * TILE + 8 * (q >> 1) + (lane >> 3);
  const float pixf_x = (float)pix_x, pixf_y = (float)pix_y;
  const float qx0 = (float)(tx * TILE + 8 * (q & 1)), qy0 = (float)(ty * TILE + 8 * (q >> 1));
  const size_t HW = (size_t)p.W * p.H;
  float rx = 0.f, ry = 0.f;
  if (MODE == MODE_SURFEL) {
    const float cxp = (p.prcp ? p.prcp[0] : 0.5f) * (float)p.W - 0.5f;
    const float cyp = (p.prcp ? p.prcp[1] : 0.5f) * (float)p.H - 0.5f;
    rx = (pixf_x - cxp) / p.fx;
    ry = (pixf_y - cyp) / p.fy;
  }
  const uint2 range = ranges[tile];
  const int todo = (int)(range.y - range.x);
  const bool inside = pix_x < p.W && pix_y < p.H;
  float T = 1.0f, C0 = 0.f, C1 = 0.f, C2 = 0.f, N0 = 0.f, N1 = 0.f, N2 = 0.f, D = 0.f;
  uint32_t last = 0;
  bool done = !inside;

  // window being fetched: slot, Gaussian id, first two record quads of list entry base + lane
  // two-stage fetch pipeline (list entry -> Gaussian id | id -> whole record), see blend_fwd_seg_kernel
  uint32_t f_slot = 0, f_g = 0, n_slot = 0, n_g = 0;
  float4 f_a = make_float4(0.f, 0.f, 0.f, 0.f), f_b = f_a, f_c = f_a, f_d = f_a;
  bool f_ok = false, n_ok = false;
  auto fetch_ids = [&](int base) {
    const int e = base + lane;
    n_ok = e < todo;
    if (n_ok) {
      n_slot = point_list[range.x + e];
      n_g = gval[n_slot];
    }
  };
  auto fetch_records = [&]() {
    f_slot = n_slot; f_g = n_g; f_ok = n_ok;
    if (f_ok) {
      f_a = rec[4 * (size_t)f_g + 0];
      f_b = rec[4 * (size_t)f_g + 1];
      f_c = rec[4 * (size_t)f_g + 2];
      if (MODE == MODE_SURFEL) f_d = rec[4 * (size_t)f_g + 3];
    }
  };
  if (todo > 0 && !__all(done)) {
    fetch_ids(0);
    fetch_records();
    if (64 < todo) fetch_ids(64); else n_ok = false;
  }

  for (int base = 0; base < todo; base += 64) {
    if (__all(done)) break;
    const uint32_t slot = f_slot;
    const float4 ra = f_a, rb = f_b, rc = f_c, rd = f_d;
    const bool ok = f_ok;
    if (base + 64 < todo) {                                // in flight while this window is blended
      fetch_records();
      if (base + 128 < todo) fetch_ids(base + 128); else n_ok = false;
    }
    bool rel = false;
    if (ok) {
      const float thr = 2.f * __logf(255.f * ra.z) + 2e-3f;
      rel = !footprint_misses_rect(ra.x, ra.y, rb.x, rb.y, rb.z, thr, qx0, qx0 + 7.f, qy0, qy0 + 7.f);
    }
    const unsigned long long bal = __ballot(rel);
    const int n = __popcll(bal);
    if (rel) {
      const int at = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
      sA[at] = ra;
      sB[at] = rb;
      sC[at] = rc;
      if (MODE == MODE_SURFEL) sD[at] = rd;
      sSlot[at] = slot;
      sE[at] = base + lane;
    }
    sW[lane] = 0.f;
    if (MODE == MODE_3DGS) sCnt[lane] = 0u;
    __builtin_amdgcn_wave_barrier();

    // records in groups of 16, their weight sums reduced together (see blend_fwd_tile_kernel)
    bool stop_all = false;
    for (int j0 = 0; j0 < n && !stop_all; j0 += 16) {
      float ws[16], wc[16];
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) { ws[jj] = 0.f; wc[jj] = 0.f; }
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) {
        const int j = j0 + jj;
        if (j >= n || stop_all) continue;   // wave-uniform
        const float4 a = sA[j], b = sB[j], c = sC[j];
        float4 nn = make_float4(0.f, 0.f, 0.f, 0.f);
        if (MODE == MODE_SURFEL) nn = sD[j];
        const float dx = a.x - pixf_x;
        const float p0 = -0.5f * (b.x * dx * dx);
        const float pxy = b.y * dx;
        const float dy = a.y - pixf_y;
        const float power = (p0 - 0.5f * (b.z * dy * dy)) - pxy * dy;
        const float alpha = fminf(ALPHA_MAX, a.z * __expf(power));
        const bool valid = !done && (power <= 0.0f) && (alpha >= ALPHA_MIN);
        const float test_T = T * (1.0f - alpha);
        const bool stop = valid && (test_T < T_EPS);
        const bool contrib = valid && !stop;
        done = done || stop;
        if (__any(contrib)) {
          const float w = contrib ? alpha * T : 0.f;
          C0 = fmaf(c.x, w, C0);
          C1 = fmaf(c.y, w, C1);
          C2 = fmaf(c.z, w, C2);
          if (MODE == MODE_SURFEL) {
            const float den = (nn.x * rx + nn.y * ry) + nn.z;
            float d = den < -DEN_EPS ? c.w * __builtin_amdgcn_rcpf(den) : a.w;
            d = fminf(fmaxf(d, a.w - b.w), a.w + b.w);
            N0 = fmaf(nn.x, w, N0);
            N1 = fmaf(nn.y, w, N1);
            N2 = fmaf(nn.z, w, N2);
            D = fmaf(d, w, D);
          } else {
            D = fmaf(a.w, w, D);
            wc[jj] = (contrib && test_T > 0.5f) ? 1.f : 0.f;
          }
          T = contrib ? test_T : T;
          last = contrib ? (uint32_t)(sE[j] + 1) : last;
          ws[jj] = w;
        }
        stop_all = __all(done);
      }
      const int slot16 = 8 * (lane & 1) + 4 * ((lane >> 1) & 1) + ((lane >> 2) & 3);
      const float tw = wave_reduce16(ws, lane);
      if (lane < 16 && j0 + slot16 < n) sW[j0 + slot16] = tw;
      if (MODE == MODE_3DGS) {
        const float tc = wave_reduce16(wc, lane);
        if (lane < 16 && j0 + slot16 < n) sCnt[j0 + slot16] = (uint32_t)tc;
      }
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < n) {
      const float w = sW[lane];
      if (w != 0.f) {  // untouched entries stay at their memset zero
        inst_wq[4 * (size_t)sSlot[lane] + q] = w;
        if (MODE == MODE_3DGS) inst_cntq[4 * (size_t)sSlot[lane] + q] = sCnt[lane];
      }
    }
    __builtin_amdgcn_wave_barrier();
  }

  if (inside) {
    const size_t pix_id = (size_t)pix_y * p.W + pix_x;
    const float A = 1.0f - T;
    final_T[pix_id] = T;
    n_contrib[pix_id] = last;
    out_color[pix_id] = C0 + T * p.bg[0];
    out_color[HW + pix_id] = C1 + T * p.bg[1];
    out_color[2 * HW + pix_id] = C2 + T * p.bg[2];
    out_alpha[pix_id] = A;
    if (MODE == MODE_SURFEL) {
      out_normal[pix_id] = N0;
      out_normal[HW + pix_id] = N1;
      out_normal[2 * HW + pix_id] = N2;
      out_depth[pix_id] = D / fmaxf(A, DEPTH_ALPHA_EPS);
    } else {
      out_depth[pix_id] = D;
    }
  }
}

// ---------------------------------------------------------------- forward of LONG tile lists, in parallel segments
// A wave blends ~8 list entries per microsecond, one after the other: a tile whose list holds 14,000 records (the
// horizon of a street scene: thousands of edge-on surfels behind one another, none of them opaque) keeps ONE wave per
// quadrant busy for 1.7 ms while the rest of the chip has long finished.  Front-to-back compositing is associative:
//     (C, T) of a list = (C_a + T_a C_b, T_a T_b)  for the list split into a | b,
// so lists longer than SEG_THR entries are cut into segments of SEG entries, each blended by its own wave:
//   pass T  every (tile, segment, quadrant) wave walks its segment and multiplies up (1 - alpha) per pixel — alpha
//           evaluation only, the cheap half of the blend, and no termination test (that needs the transmittance in
//           front, which is what this pass is producing);
//   pass B  the wave multiplies the products of the segments in front of it — which is the transmittance its pixels
//           start with, and also tells it whether a pixel has stopped before (the running value is monotone, so it
//           stopped in segment s iff T_in(s) P(s) < T_EPS) — and then blends its segment EXACTLY like the serial
//           kernel does: same alpha arithmetic, same stop rule, same per-instance weight sums, `n_contrib` in global
//           list positions; colour / normal / depth partial sums, T and the last contributor go to a per-segment slab;
//   pass C  one wave per (tile, quadrant) adds the slabs in list order and writes the pixel outputs.
// What differs from the serial kernel is floating-point association only: T_in is a product of per-segment products
// instead of one running product, the colour sum a sum of per-segment sums (relative 1e-6); the stop decision can
// flip for a pixel whose transmittance sits within that rounding of 1e-4.  Lists up to SEG_THR entries never come
// here, so every list-parity test against the oracle is untouched; `PINGS_BLEND_SEG=<entries>` forces a small
// segment size (tests), 0 turns the path off.
constexpr int SEG_SLAB = 10;           // floats per pixel in a segment slab: C0 C1 C2 N0 N1 N2 D T last(bits) touched

// One workgroup: tiles with more than `thr` entries get ceil(L / seg) units; units of a tile are contiguous.
// head[0] = number of units, head[1] = number of long tiles.  unit_tile[u], unit_seg[u]; tile_unit0[tile] (or ~0u).
__global__ __launch_bounds__(1024) void seg_plan_kernel(const uint2* __restrict__ ranges, int num_tiles, uint32_t thr,
                                                        uint32_t seg, uint32_t max_units, uint32_t* __restrict__ head,
                                                        uint32_t* __restrict__ unit_tile, uint32_t* __restrict__ unit_seg,
                                                        uint32_t* __restrict__ tile_unit0) {
  __shared__ uint32_t sScan[1024];
  __shared__ uint32_t sBase;
  const int tid = threadIdx.x;
  if (tid == 0) sBase = 0u;
  __syncthreads();
  for (int t0 = 0; t0 < num_tiles; t0 += 1024) {
    const int t = t0 + tid;
    uint32_t n = 0;
    if (t < num_tiles) {
      const uint32_t L = ranges[t].y - ranges[t].x;
      if (L > thr) n = (L + seg - 1) / seg;
    }
    sScan[tid] = n;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const uint32_t add = tid >= off ? sScan[tid - off] : 0u;
      __syncthreads();
      sScan[tid] += add;
      __syncthreads();
    }
    const uint32_t base = sBase + sScan[tid] - n;
    if (t < num_tiles) {
      const bool fits = n > 0 && base + n <= max_units;   // a tile that does not fit stays with the serial kernel
      tile_unit0[t] = fits ? base : 0xFFFFFFFFu;
      if (fits) {
        for (uint32_t k = 0; k < n; ++k) { unit_tile[base + k] = (uint32_t)t; unit_seg[base + k] = k; }
      } else {
        for (uint32_t k = 0; k < n && base + k < max_units; ++k) { unit_tile[base + k] = 0xFFFFFFFFu; unit_seg[base + k] = 1u; }
      }
    }
    __syncthreads();
    if (tid == 1023) sBase += sScan[1023];
    __syncthreads();
  }
  if (tid == 0) head[0] = sBase < max_units ? sBase : max_units;
}

// PASS: 0 = transmittance products, 1 = blend.  Pass T leaves, per (unit, quadrant), the offsets of the entries that
// passed its footprint test (seg_rel / seg_nrel); with REUSE pass B walks that list in dense 64-entry windows — no
// fetch of the 63 % of the entries that cannot reach the quadrant, no second footprint test, no second compaction,
// 2.7x fewer windows.  The same entries in the same order: bit-identical to the re-testing form (REUSE = false, kept
// for segment sizes beyond 16-bit offsets).
template <int MODE, int PASS, bool REUSE = false>
__device__ __forceinline__ void blend_fwd_seg_body(
    const KParams& p, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
    const float4* __restrict__ rec, const uint32_t* __restrict__ gval, uint32_t seg, const uint32_t* __restrict__ head,
    const uint32_t* __restrict__ unit_tile, const uint32_t* __restrict__ unit_seg, float* __restrict__ segP,
    float* __restrict__ slab, float* __restrict__ inst_wq, uint32_t* __restrict__ inst_cntq, const unsigned block,
    uint16_t* __restrict__ seg_rel = nullptr, uint32_t* __restrict__ seg_nrel = nullptr) {
  __shared__ float4 sA_[4][64], sB_[4][64], sC_[PASS == 1 ? 4 : 1][64], sD_[PASS == 1 ? 4 : 1][64];
  __shared__ uint32_t sSlot_[PASS == 1 ? 4 : 1][64];
  __shared__ int sE_[PASS == 1 ? 4 : 1][64];
  __shared__ float sW_[PASS == 1 ? 4 : 1][64];
  __shared__ uint32_t sCnt_[PASS == 1 ? 4 : 1][64];

  const int lane = threadIdx.x & 63, q = (int)(threadIdx.x >> 6);   // wave = quadrant (see blend_fwd_wave_kernel)
  constexpr int QB = PASS == 1 ? 1 : 0;
  float4 *sA = sA_[q], *sB = sB_[q], *sC = sC_[QB * q], *sD = sD_[QB * q];
  uint32_t *sSlot = sSlot_[QB * q], *sCnt = sCnt_[QB * q];
  int* sE = sE_[QB * q];
  float* sW = sW_[QB * q];
  const uint32_t unit = block;
  if (unit >= head[0] || unit_tile[unit] == 0xFFFFFFFFu) return;
  const int tile = (int)unit_tile[unit];
  const uint32_t sg = unit_seg[unit];
  const int tx = tile % p.gx, ty = tile / p.gx;
  const int pix_x = tx * TILE + 8 * (q & 1) + (lane & 7);
  const int pix_y = ty * TILE + 8 * (q >> 1) + (lane >> 3);
  const float pixf_x = (float)pix_x, pixf_y = (float)pix_y;
  const float qx0 = (float)(tx * TILE + 8 * (q & 1)), qy0 = (float)(ty * TILE + 8 * (q >> 1));
  float rx = 0.f, ry = 0.f;
  if (MODE == MODE_SURFEL && PASS == 1) {
    const float cxp = (p.prcp ? p.prcp[0] : 0.5f) * (float)p.W - 0.5f;
    const float cyp = (p.prcp ? p.prcp[1] : 0.5f) * (float)p.H - 0.5f;
    rx = (pixf_x - cxp) / p.fx;
    ry = (pixf_y - cyp) / p.fy;
  }
  const uint2 range = ranges[tile];
  const int L = (int)(range.y - range.x);
  const int e_lo = (int)(sg * seg);
  int e_hi = min(L, (int)((sg + 1) * seg));
  const bool inside = pix_x < p.W && pix_y < p.H;
  const size_t my = ((size_t)unit * 4 + q) * 64 + lane;
  // REUSE: the window loop below runs over positions [0, nrel) of pass T's list instead of entries [e_lo, e_hi)
  uint16_t* rel_list = seg_rel ? seg_rel + ((size_t)unit * 4 + q) * seg : nullptr;
  int w_lo = e_lo;
  if (REUSE) { w_lo = 0; e_hi = (int)seg_nrel[(size_t)unit * 4 + q]; }
  int nrel_out = 0;

  float T = 1.0f;
  bool done = !inside;
  if (PASS == 1) {
    // transmittance in front of this segment; stopped before it?
    const size_t first = ((size_t)(unit - sg) * 4 + q) * 64 + lane;
    for (uint32_t s2 = 0; s2 < sg; ++s2) {
      T *= segP[first + (size_t)s2 * 256];
      if (T < T_EPS) { done = true; break; }
    }
  }
  float C0 = 0.f, C1 = 0.f, C2 = 0.f, N0 = 0.f, N1 = 0.f, N2 = 0.f, D = 0.f;
  uint32_t last = 0;

  // The fetch of a window is a chain of three dependent loads (list entry -> Gaussian id -> record).  It runs as a
  // two-stage pipeline: the ids of window k + 2 and the records of window k + 1 are in flight while window k is
  // blended, so no stage has to cover more than two dependent latencies with one window's work (with the whole chain
  // one window ahead, the short windows of pass T waited for it).
  uint32_t f_slot = 0, f_g = 0, n_slot = 0, n_g = 0;
  int f_e = 0, n_e = 0;                  // list position (entry index in the tile's list) of the fetched record
  float4 f_a = make_float4(0.f, 0.f, 0.f, 0.f), f_b = f_a, f_c = f_a, f_d = f_a;
  bool f_ok = false, n_ok = false;
  auto fetch_ids = [&](int base) {       // stage 1: list entry -> Gaussian id
    const int e = base + lane;
    n_ok = e < e_hi;
    if (n_ok) {
      n_e = REUSE ? e_lo + (int)rel_list[e] : e;
      n_slot = point_list[range.x + n_e];
      n_g = gval[n_slot];
    }
  };
  auto fetch_records = [&]() {           // stage 2: the ids that stage 1 brought -> first two record quads
    f_slot = n_slot; f_g = n_g; f_ok = n_ok; f_e = n_e;
    if (f_ok) {
      f_a = rec[4 * (size_t)f_g + 0];
      f_b = rec[4 * (size_t)f_g + 1];
      if (PASS == 1) {                   // the other half of the 64-byte record: same cache line, and the blend loop
        f_c = rec[4 * (size_t)f_g + 2];  // no longer starts with a load of its own
        if (MODE == MODE_SURFEL) f_d = rec[4 * (size_t)f_g + 3];
      }
    }
  };
  if (w_lo < e_hi && !__all(done)) {
    fetch_ids(w_lo);
    fetch_records();
    if (w_lo + 64 < e_hi) fetch_ids(w_lo + 64); else n_ok = false;
  }

  for (int base = w_lo; base < e_hi; base += 64) {
    if (__all(done)) break;
    const uint32_t slot = f_slot;
    const float4 ra = f_a, rb = f_b, rc = f_c, rd = f_d;
    const bool ok = f_ok;
    const int ent = f_e;
    if (base + 64 < e_hi) {
      fetch_records();
      if (base + 128 < e_hi) fetch_ids(base + 128); else n_ok = false;
    }
    bool rel = ok;                        // REUSE: pass T tested these entries already
    if (!REUSE && ok) {
      const float thr = 2.f * __logf(255.f * ra.z) + 2e-3f;
      rel = !footprint_misses_rect(ra.x, ra.y, rb.x, rb.y, rb.z, thr, qx0, qx0 + 7.f, qy0, qy0 + 7.f);
    }
    const unsigned long long bal = __ballot(rel);
    const int n = __popcll(bal);
    if (rel) {
      const int at = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
      sA[at] = ra;
      sB[at] = rb;
      if (PASS == 1) {
        sC[at] = rc;
        if (MODE == MODE_SURFEL) sD[at] = rd;
        sSlot[at] = slot;
        sE[at] = ent;
      } else if (rel_list) {
        rel_list[nrel_out + at] = (uint16_t)(ent - e_lo);
      }
    }
    nrel_out += n;
    if (PASS == 1) {
      sW[lane] = 0.f;
      if (MODE == MODE_3DGS) sCnt[lane] = 0u;
    }
    __builtin_amdgcn_wave_barrier();

    if (PASS == 0) {
      for (int j = 0; j < n; ++j) {
        const float4 a = sA[j], b = sB[j];
        const float dx = a.x - pixf_x;
        const float p0 = -0.5f * (b.x * dx * dx);
        const float pxy = b.y * dx;
        const float dy = a.y - pixf_y;
        const float power = (p0 - 0.5f * (b.z * dy * dy)) - pxy * dy;
        const float alpha = fminf(ALPHA_MAX, a.z * __expf(power));
        const bool valid = inside && (power <= 0.0f) && (alpha >= ALPHA_MIN);
        T = valid ? T * (1.0f - alpha) : T;
      }
    } else {
      // records in groups of 16, their weight sums reduced together (see blend_fwd_tile_kernel)
      bool stop_all = false;
      for (int j0 = 0; j0 < n && !stop_all; j0 += 16) {
        float ws[16], wc[16];
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) { ws[jj] = 0.f; wc[jj] = 0.f; }
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) {
          const int j = j0 + jj;
          if (j >= n || stop_all) continue;   // wave-uniform
          const float4 a = sA[j], b = sB[j];
          const float dx = a.x - pixf_x;
          const float p0 = -0.5f * (b.x * dx * dx);
          const float pxy = b.y * dx;
          const float dy = a.y - pixf_y;
          const float power = (p0 - 0.5f * (b.z * dy * dy)) - pxy * dy;
          const float alpha = fminf(ALPHA_MAX, a.z * __expf(power));
          const float4 c = sC[j];
          float4 nn = make_float4(0.f, 0.f, 0.f, 0.f);
          if (MODE == MODE_SURFEL) nn = sD[j];
          const bool valid = !done && (power <= 0.0f) && (alpha >= ALPHA_MIN);
          const float test_T = T * (1.0f - alpha);
          const bool stop = valid && (test_T < T_EPS);
          const bool contrib = valid && !stop;
          done = done || stop;
          if (__any(contrib)) {
            const float w = contrib ? alpha * T : 0.f;
            C0 = fmaf(c.x, w, C0);
            C1 = fmaf(c.y, w, C1);
            C2 = fmaf(c.z, w, C2);
            if (MODE == MODE_SURFEL) {
              const float den = (nn.x * rx + nn.y * ry) + nn.z;
              float d = den < -DEN_EPS ? c.w * __builtin_amdgcn_rcpf(den) : a.w;
              d = fminf(fmaxf(d, a.w - b.w), a.w + b.w);
              N0 = fmaf(nn.x, w, N0);
              N1 = fmaf(nn.y, w, N1);
              N2 = fmaf(nn.z, w, N2);
              D = fmaf(d, w, D);
            } else {
              D = fmaf(a.w, w, D);
              wc[jj] = (contrib && test_T > 0.5f) ? 1.f : 0.f;
            }
            T = contrib ? test_T : T;
            last = contrib ? (uint32_t)(sE[j] + 1) : last;
            ws[jj] = w;
          }
          stop_all = __all(done);
        }
        const int slot16 = 8 * (lane & 1) + 4 * ((lane >> 1) & 1) + ((lane >> 2) & 3);
        const float tw = wave_reduce16(ws, lane);
        if (lane < 16 && j0 + slot16 < n) sW[j0 + slot16] = tw;
        if (MODE == MODE_3DGS) {
          const float tc = wave_reduce16(wc, lane);
          if (lane < 16 && j0 + slot16 < n) sCnt[j0 + slot16] = (uint32_t)tc;
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
    if (PASS == 1 && lane < n) {
      const float w = sW[lane];
      if (w != 0.f) {
        inst_wq[4 * (size_t)sSlot[lane] + q] = w;
        if (MODE == MODE_3DGS) inst_cntq[4 * (size_t)sSlot[lane] + q] = sCnt[lane];
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (PASS == 0) {
    segP[my] = T;
    if (seg_nrel && lane == 0) seg_nrel[(size_t)unit * 4 + q] = (uint32_t)nrel_out;
  } else {
    float* o = slab + ((size_t)unit * 4 + q) * 64 * SEG_SLAB + lane;
    o[0] = C0; o[64] = C1; o[128] = C2; o[192] = N0; o[256] = N1; o[320] = N2; o[384] = D;
    o[448] = T;                                     // transmittance behind this segment (its pixels' running value)
    o[512] = __uint_as_float(last);
    o[576] = done ? 1.f : 0.f;
  }
}

template <int MODE, int PASS, bool REUSE>
__global__ __launch_bounds__(256) void blend_fwd_seg_kernel(
    KParams p, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
    const float4* __restrict__ rec, const uint32_t* __restrict__ gval, uint32_t seg, const uint32_t* __restrict__ head,
    const uint32_t* __restrict__ unit_tile, const uint32_t* __restrict__ unit_seg, float* __restrict__ segP,
    float* __restrict__ slab, float* __restrict__ inst_wq, uint32_t* __restrict__ inst_cntq,
    uint16_t* __restrict__ seg_rel, uint32_t* __restrict__ seg_nrel) {
  blend_fwd_seg_body<MODE, PASS, REUSE>(p, ranges, point_list, rec, gval, seg, head, unit_tile, unit_seg, segP, slab,
                                        inst_wq, inst_cntq, blockIdx.x, seg_rel, seg_nrel);
}

template <int MODE>
__global__ __launch_bounds__(256) void blend_fwd_wave_kernel(
    KParams p, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
    const float4* __restrict__ rec, const uint32_t* __restrict__ gval, float* __restrict__ out_color,
    float* __restrict__ out_normal, float* __restrict__ out_depth, float* __restrict__ out_alpha,
    float* __restrict__ final_T, uint32_t* __restrict__ n_contrib, float* __restrict__ inst_wq,
    uint32_t* __restrict__ inst_cntq, const uint32_t* __restrict__ tile_order,
    const uint32_t* __restrict__ seg_tile_unit0) {
  blend_fwd_wave_body<MODE>(p, ranges, point_list, rec, gval, out_color, out_normal, out_depth, out_alpha, final_T,
                            n_contrib, inst_wq, inst_cntq, tile_order, seg_tile_unit0, blockIdx.x);
}

// The short-list tiles and pass T of the segmented tiles in ONE launch (workgroups [0, num_tiles) are tiles, the rest
// segment units): the two touch disjoint tiles and both spend a third of their time in s_waitcnt, so together they
// fill what each leaves idle.  (A side stream does the same with two launches — 0.775 -> 0.719 ms on C3 — but its
// cross-queue event wait once took 11 ms per frame on one box of the pool; one launch needs no such wait.)
template <int MODE>
__global__ __launch_bounds__(256) void blend_fwd_wave_segT_kernel(
    KParams p, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
    const float4* __restrict__ rec, const uint32_t* __restrict__ gval, float* __restrict__ out_color,
    float* __restrict__ out_normal, float* __restrict__ out_depth, float* __restrict__ out_alpha,
    float* __restrict__ final_T, uint32_t* __restrict__ n_contrib, float* __restrict__ inst_wq,
    uint32_t* __restrict__ inst_cntq, const uint32_t* __restrict__ tile_order,
    const uint32_t* __restrict__ seg_tile_unit0, unsigned num_tiles, uint32_t seg, const uint32_t* __restrict__ head,
    const uint32_t* __restrict__ unit_tile, const uint32_t* __restrict__ unit_seg, float* __restrict__ segP,
    uint16_t* __restrict__ seg_rel, uint32_t* __restrict__ seg_nrel) {
  if (blockIdx.x < num_tiles)
    blend_fwd_wave_body<MODE>(p, ranges, point_list, rec, gval, out_color, out_normal, out_depth, out_alpha, final_T,
                              n_contrib, inst_wq, inst_cntq, tile_order, seg_tile_unit0, blockIdx.x);
  else
    blend_fwd_seg_body<MODE, 0>(p, ranges, point_list, rec, gval, seg, head, unit_tile, unit_seg, segP, nullptr, inst_wq,
                                inst_cntq, blockIdx.x - num_tiles, seg_rel, seg_nrel);
}

// PASS C: first-segment waves add their tile's slabs in list order and write the pixel outputs.
template <int MODE>
__global__ __launch_bounds__(256) void blend_fwd_seg_combine_kernel(
    KParams p, const uint2* __restrict__ ranges, uint32_t seg, const uint32_t* __restrict__ head,
    const uint32_t* __restrict__ unit_tile, const uint32_t* __restrict__ unit_seg, const float* __restrict__ slab,
    float* __restrict__ out_color, float* __restrict__ out_normal, float* __restrict__ out_depth,
    float* __restrict__ out_alpha, float* __restrict__ final_T, uint32_t* __restrict__ n_contrib) {
  const int lane = threadIdx.x & 63;
  const uint32_t unit = blockIdx.x;
  const int q = (int)(threadIdx.x >> 6);
  if (unit >= head[0] || unit_seg[unit] != 0u || unit_tile[unit] == 0xFFFFFFFFu) return;
  const int tile = (int)unit_tile[unit];
  const int tx = tile % p.gx, ty = tile / p.gx;
  const int pix_x = tx * TILE + 8 * (q & 1) + (lane & 7);
  const int pix_y = ty * TILE + 8 * (q >> 1) + (lane >> 3);
  if (pix_x >= p.W || pix_y >= p.H) return;
  const uint32_t L = ranges[tile].y - ranges[tile].x;
  const uint32_t nseg = (L + seg - 1) / seg;
  float C0 = 0.f, C1 = 0.f, C2 = 0.f, N0 = 0.f, N1 = 0.f, N2 = 0.f, D = 0.f, T = 1.0f;
  uint32_t last = 0;
  for (uint32_t s2 = 0; s2 < nseg; ++s2) {
    const float* o = slab + ((size_t)(unit + s2) * 4 + q) * 64 * SEG_SLAB + lane;
    C0 += o[0]; C1 += o[64]; C2 += o[128]; N0 += o[192]; N1 += o[256]; N2 += o[320]; D += o[384];
    const uint32_t l2 = __float_as_uint(o[512]);
    if (l2 != 0u) { last = l2; T = o[448]; }          // the last segment that blended something holds T and n_contrib
    if (o[576] != 0.f) break;                        // the pixel stopped inside (or before) this segment
  }
  const size_t HW = (size_t)p.W * p.H;
  const size_t pix_id = (size_t)pix_y * p.W + pix_x;
  const float A = 1.0f - T;
  final_T[pix_id] = T;
  n_contrib[pix_id] = last;
  out_color[pix_id] = C0 + T * p.bg[0];
  out_color[HW + pix_id] = C1 + T * p.bg[1];
  out_color[2 * HW + pix_id] = C2 + T * p.bg[2];
  out_alpha[pix_id] = A;
  if (MODE == MODE_SURFEL) {
    out_normal[pix_id] = N0;
    out_normal[HW + pix_id] = N1;
    out_normal[2 * HW + pix_id] = N2;
    out_depth[pix_id] = D / fmaxf(A, DEPTH_ALPHA_EPS);
  } else {
    out_depth[pix_id] = D;
  }
}

// ---------------------------------------------------------------- forward, one independent wave per 16x16 tile
// Footprint class 2 (footprints of many tiles: almost every record of a tile's list reaches all four quadrants, so
// sub-tile culling buys nothing).  Same window pipeline as the quadrant kernel, but the wave owns the whole tile with
// FOUR pixels per lane (k & 1 -> x half, k >> 1 -> y half): the record fetch from LDS, the footprint test and the
// wave reduction of the blend weights are paid once per 256 pixels instead of once per 64, and the per-instance sum
// is final — no per-quadrant partials, no 16-byte-per-instance memset, no combine pass.  Pixel arithmetic is the
// quadrant kernel's, op for op (images bit-identical); the per-instance weight sum adds the same terms in another
// order.  inst_qmask is NOT produced: only the pixel-per-lane backward (which this class uses) may follow.
// tile_maxc[tile] = the largest n_contrib of the tile's pixels inside the image, which the wave holds when it stores
// them: the work estimate of the backward dispatch order (tile_max_contrib_kernel computes it for the other forwards).
template <int MODE>
__global__ __launch_bounds__(64) void blend_fwd_tile_kernel(
    KParams p, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
    const float4* __restrict__ rec, const uint32_t* __restrict__ gval, float* __restrict__ out_color,
    float* __restrict__ out_normal, float* __restrict__ out_depth, float* __restrict__ out_alpha,
    float* __restrict__ final_T, uint32_t* __restrict__ n_contrib, float* __restrict__ inst_w,
    uint32_t* __restrict__ inst_cnt, const uint32_t* __restrict__ tile_order, uint32_t* __restrict__ tile_maxc) {
  constexpr int PPL = 4;
  __shared__ float4 sA[64], sB[64], sC[64], sD[64];
  __shared__ uint32_t sSlot[64];
  __shared__ float sW[64];
  __shared__ uint32_t sCnt[64];

  const int lane = threadIdx.x;
  const int tile = (int)tile_order[blockIdx.x];
  const int tx = tile % p.gx, ty = tile / p.gx;
  const float qx0 = (float)(tx * TILE), qy0 = (float)(ty * TILE);
  const size_t HW = (size_t)p.W * p.H;
  int pix_x[2], pix_y[2];
  float pixf_x[2], pixf_y[2], rx[2] = {0.f, 0.f}, ry[2] = {0.f, 0.f};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    pix_x[h] = tx * TILE + 8 * h + (lane & 7);
    pix_y[h] = ty * TILE + 8 * h + (lane >> 3);
    pixf_x[h] = (float)pix_x[h];
    pixf_y[h] = (float)pix_y[h];
  }
  if (MODE == MODE_SURFEL) {
    const float cxp = (p.prcp ? p.prcp[0] : 0.5f) * (float)p.W - 0.5f;
    const float cyp = (p.prcp ? p.prcp[1] : 0.5f) * (float)p.H - 0.5f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      rx[h] = (pixf_x[h] - cxp) / p.fx;
      ry[h] = (pixf_y[h] - cyp) / p.fy;
    }
  }
  const uint2 range = ranges[tile];
  const int todo = (int)(range.y - range.x);
  // pixel state per row r = k >> 1 as packed pairs (f2 component h = k & 1): the two pixels of a row share the
  // record's dy terms, and every per-pixel multiply / add / fma below is one v_pk_* instruction for both, rounded per
  // component as the scalar instruction would be — images, final_T and n_contrib stay bit-identical to the
  // pixel-per-lane kernel.
  const f2 pixf_x2 = {pixf_x[0], pixf_x[1]}, rx2 = {rx[0], rx[1]};
  f2 T[2], C0[2], C1[2], C2[2], N0[2], N1[2], N2[2], D[2];
  uint32_t last[PPL];
  bool inside[PPL];
  // A pixel that has stopped (or lies outside the image) is "done".  Instead of a boolean that the compiler keeps as a
  // 0/1 VGPR and turns back into a lane mask every record (v_and + v_cmp per pixel), the state lives in the alpha
  // threshold of the validity test: ALPHA_MIN while blending, DONE_AMIN (> ALPHA_MAX) once done, so `alpha >= amin`
  // is exactly `!done && alpha >= ALPHA_MIN`.  The wave's count of pixels not yet done is kept in a scalar register
  // (a pixel stops at most once), which replaces the per-record all-done vote.
  constexpr float DONE_AMIN = 2.0f;
  const float done_amin = DONE_AMIN;
  float amin[PPL];
  int live_px = 0;   // wave-uniform
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    T[r] = f2{1.0f, 1.0f};
    C0[r] = C1[r] = C2[r] = N0[r] = N1[r] = N2[r] = D[r] = f2{0.f, 0.f};
  }
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    last[k] = 0;
    inside[k] = pix_x[k & 1] < p.W && pix_y[k >> 1] < p.H;
    amin[k] = inside[k] ? ALPHA_MIN : DONE_AMIN;
    live_px += __popcll(__ballot(inside[k]));
  }

  // two-stage fetch pipeline (list entry -> Gaussian id | id -> whole record), see blend_fwd_seg_kernel
  uint32_t f_slot = 0, f_g = 0, n_slot = 0, n_g = 0;
  float4 f_a = make_float4(0.f, 0.f, 0.f, 0.f), f_b = f_a, f_c = f_a, f_d = f_a;
  bool f_ok = false, n_ok = false;
  auto fetch_ids = [&](int base) {
    const int e = base + lane;
    n_ok = e < todo;
    if (n_ok) {
      n_slot = point_list[range.x + e];
      n_g = gval[n_slot];
    }
  };
  auto fetch_records = [&]() {
    f_slot = n_slot; f_g = n_g; f_ok = n_ok;
    if (f_ok) {
      f_a = rec[4 * (size_t)f_g + 0];
      f_b = rec[4 * (size_t)f_g + 1];
      f_c = rec[4 * (size_t)f_g + 2];
      if (MODE == MODE_SURFEL) f_d = rec[4 * (size_t)f_g + 3];
    }
  };
  if (todo > 0 && live_px > 0) {
    fetch_ids(0);
    fetch_records();
    if (64 < todo) fetch_ids(64); else n_ok = false;
  }

  for (int base = 0; base < todo; base += 64) {
    if (live_px == 0) break;
    const uint32_t slot = f_slot;
    const float4 ra = f_a, rb = f_b, rc = f_c, rd = f_d;
    const bool ok = f_ok;
    if (base + 64 < todo) {                                // in flight while this window is blended
      fetch_records();
      if (base + 128 < todo) fetch_ids(base + 128); else n_ok = false;
    }
    bool rel = false;
    if (ok) {
      const float thr = 2.f * __logf(255.f * ra.z) + 2e-3f;
      rel = !footprint_misses_rect(ra.x, ra.y, rb.x, rb.y, rb.z, thr, qx0, qx0 + 15.f, qy0, qy0 + 15.f);
    }
    const unsigned long long bal = __ballot(rel);
    const int n = __popcll(bal);
    if (rel) {
      const int at = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
      sA[at] = ra;
      sB[at] = rb;
      // the record's list position + 1 (what n_contrib takes) travels in the record's unused fourth word: the normal's
      // (surfels) or the colour's (3DGS, which has no q), so the blend reads it with the record, not from an array of its own
      const float e1f = __uint_as_float((uint32_t)(base + lane + 1));
      sC[at] = MODE == MODE_SURFEL ? rc : make_float4(rc.x, rc.y, rc.z, e1f);
      if (MODE == MODE_SURFEL) sD[at] = make_float4(rd.x, rd.y, rd.z, e1f);
      sSlot[at] = slot;
    }
    sW[lane] = 0.f;
    if (MODE == MODE_3DGS) sCnt[lane] = 0u;
    __builtin_amdgcn_wave_barrier();

    // Records in groups of 16: every record's weight sum over the tile's pixels (and, 3DGS, its count of pixels it is
    // the dominant contributor of) stays in a register until the group is done, then ONE transposed reduce-scatter
    // (raster_common.hpp: wave_reduce16, ~55 vector ops for 16 sums) replaces sixteen 7-step DPP reductions and their
    // dependent chains.  The unrolled group keeps the register indices static.
    // Each record's sums are assigned once, after its branches: a conditional store into ws[] made the compiler carry
    // the whole zero-initialised array through every record's control flow (~12 v_mov per record).
    for (int j0 = 0; j0 < n && live_px > 0; j0 += 16) {
      float ws[16], wc[16];
      // the group's first record index in a VECTOR register: a record's LDS reads are then this one base plus the record's
      // position in the instruction's immediate offset, instead of a scalar address moved to a VGPR for every record
      int jv = j0;
      asm("" : "+v"(jv));
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) {
        const int j = j0 + jj;
        float wsum = 0.f;
        uint32_t touched = 0;
        if (j < n && live_px > 0) {   // wave-uniform
          float4 a = sA[jv + jj], b = sB[jv + jj];
          const float4 c = sC[jv + jj];
          float4 nn = make_float4(0.f, 0.f, 0.f, 0.f);
          if (MODE == MODE_SURFEL) nn = sD[jv + jj];
          // whole 16-byte reads of a and b: pz and rz come with the words the alpha test needs instead of by reads of
          // their own in the branch, and opacity sits in an aligned register pair (no move to build the packed operand)
          asm("" : "+v"(a.w), "+v"(b.w));
          const f2 dx = f2s(a.x) - pixf_x2;
          const f2 p0 = f2s(-0.5f) * ((f2s(b.x) * dx) * dx);
          const f2 pxy = f2s(b.y) * dx;
          f2 alpha[2], test_T[2];
          // the per-pixel decisions as lane masks (raster_common.hpp): each compare is issued once and lands in an
          // SGPR pair, stop / contrib are scalar logic on them, and every select below reads its mask directly
          lmask contrib[PPL];
          int n_stop = 0;
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            const float dy = a.y - pixf_y[r];
            const f2 power = (p0 - f2s(0.5f * (b.z * dy * dy))) - pxy * f2s(dy);
            const f2 ag = f2s(a.z) * f2{__expf(power.x), __expf(power.y)};
            alpha[r] = f2{fminf(ALPHA_MAX, ag.x), fminf(ALPHA_MAX, ag.y)};
            test_T[r] = T[r] * (f2s(1.0f) - alpha[r]);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const int k = 2 * r + h;
              const lmask valid = mask_le(power[h], 0.0f) & mask_ge(alpha[r][h], amin[k]);   // amin folds in !done
              const cmask lt = mask_lt(test_T[r][h], T_EPS);
              const lmask stop = valid & lt;
              contrib[k] = valid & ~lt;
              amin[k] = mask_sel(stop, done_amin, amin[k]);
              n_stop += mask_count(stop);
            }
          }
          live_px -= n_stop;
          if ((contrib[0] | contrib[1] | contrib[2] | contrib[3]) != 0ull) {
            const uint32_t e1 = __float_as_uint(MODE == MODE_SURFEL ? nn.w : c.w);
            // depth clamp as one v_med3: fminf(fmaxf(d, lo), hi) == med3(d, min(lo, hi), hi) for every non-NaN d
            // (lo > hi clamps to hi either way), and d is never NaN here
            const float zhi = a.w + b.w, zlo = fminf(a.w - b.w, zhi);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
              const lmask c0 = contrib[2 * r], c1 = contrib[2 * r + 1];
              const f2 w = mask_sel2_0(c0, c1, alpha[r] * T[r]);
              C0[r] = fma2(f2s(c.x), w, C0[r]);
              C1[r] = fma2(f2s(c.y), w, C1[r]);
              C2[r] = fma2(f2s(c.z), w, C2[r]);
              if (MODE == MODE_SURFEL) {
                const f2 den = (f2s(nn.x) * rx2 + f2s(nn.y * ry[r])) + f2s(nn.z);
                const f2 dq = f2s(c.w) * f2{__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)};
                // compared and selected on directly: the compiler's select, which it keeps two wait states behind the compare
                const f2 d0 = sel2(den.x < -DEN_EPS, den.y < -DEN_EPS, dq, f2s(a.w));
                const f2 d = {__builtin_amdgcn_fmed3f(d0.x, zlo, zhi), __builtin_amdgcn_fmed3f(d0.y, zlo, zhi)};
                N0[r] = fma2(f2s(nn.x), w, N0[r]);
                N1[r] = fma2(f2s(nn.y), w, N1[r]);
                N2[r] = fma2(f2s(nn.z), w, N2[r]);
                D[r] = fma2(d, w, D[r]);
              } else {
                D[r] = fma2(f2s(a.w), w, D[r]);
                touched += mask_one(c0 & mask_gt(test_T[r].x, 0.5f));
                touched += mask_one(c1 & mask_gt(test_T[r].y, 0.5f));
              }
              T[r] = mask_sel2(c0, c1, test_T[r], T[r]);
              last[2 * r] = mask_sel(c0, e1, last[2 * r]);
              last[2 * r + 1] = mask_sel(c1, e1, last[2 * r + 1]);
              wsum = r == 0 ? w.x + w.y : (wsum + w.x) + w.y;   // pixel order k = 0..3, as the scalar sum
            }
          }
        }
        ws[jj] = wsum;
        wc[jj] = (float)touched;   // 3DGS: <= 4 per lane, <= 256 per record: exact in fp32
      }
      // lane l of every 16-lane row ends with the total of slot 8*(l&1) + 4*((l>>1)&1) + ((l>>2)&3)
      const int slot16 = 8 * (lane & 1) + 4 * ((lane >> 1) & 1) + ((lane >> 2) & 3);
      const float tw = wave_reduce16(ws, lane);
      if (lane < 16 && j0 + slot16 < n) sW[j0 + slot16] = tw;
      if (MODE == MODE_3DGS) {
        const float tc = wave_reduce16(wc, lane);
        if (lane < 16 && j0 + slot16 < n) sCnt[j0 + slot16] = (uint32_t)tc;
      }
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < n) {
      const float w = sW[lane];
      if (w != 0.f) {  // untouched entries stay at their memset zero
        inst_w[sSlot[lane]] = w;
        if (MODE == MODE_3DGS) inst_cnt[sSlot[lane]] = sCnt[lane];
      }
    }
    __builtin_amdgcn_wave_barrier();
  }

#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    if (!inside[k]) continue;
    const int r = k >> 1, h = k & 1;
    const float Tk = T[r][h];
    const size_t pix_id = (size_t)pix_y[r] * p.W + pix_x[h];
    const float A = 1.0f - Tk;
    final_T[pix_id] = Tk;
    n_contrib[pix_id] = last[k];
    out_color[pix_id] = C0[r][h] + Tk * p.bg[0];
    out_color[HW + pix_id] = C1[r][h] + Tk * p.bg[1];
    out_color[2 * HW + pix_id] = C2[r][h] + Tk * p.bg[2];
    out_alpha[pix_id] = A;
    if (MODE == MODE_SURFEL) {
      out_normal[pix_id] = N0[r][h];
      out_normal[HW + pix_id] = N1[r][h];
      out_normal[2 * HW + pix_id] = N2[r][h];
      out_depth[pix_id] = D[r][h] / fmaxf(A, DEPTH_ALPHA_EPS);
    } else {
      out_depth[pix_id] = D[r][h];
    }
  }
  uint32_t mc = 0u;
#pragma unroll
  for (int k = 0; k < PPL; ++k) mc = max(mc, inside[k] ? last[k] : 0u);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mc = max(mc, (uint32_t)__shfl_xor((int)mc, off, 64));
  if (lane == 0) tile_maxc[tile] = mc;
}

// inst_w[slot] = sum over the quadrants in fixed order, inst_cnt likewise, inst_qmask = quadrants that blended
template <int MODE>
__global__ __launch_bounds__(256) void combine_quadrants_kernel(int64_t I, const float4* __restrict__ wq,
                                                                const uint4* __restrict__ cq, float* __restrict__ inst_w,
                                                                uint32_t* __restrict__ inst_cnt,
                                                                uint8_t* __restrict__ inst_qmask) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) { inst_w[I] = 0.f; inst_qmask[I] = 0; }  // sentinel entry of the live-instance scans
  if (i >= I) return;
  const float4 w = wq[i];
  inst_w[i] = ((w.x + w.y) + w.z) + w.w;
  inst_qmask[i] = (uint8_t)((w.x != 0.f ? 1u : 0u) | (w.y != 0.f ? 2u : 0u) | (w.z != 0.f ? 4u : 0u) | (w.w != 0.f ? 8u : 0u));
  if (MODE == MODE_3DGS) {
    const uint4 c = cq[i];
    inst_cnt[i] = c.x + c.y + c.z + c.w;
  }
}

__device__ inline uint32_t wave_reduce_sum_u32(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
  return v;
}

// Per-Gaussian sum of its per-instance values (contiguous run of `tiles` slots).  One lane per
// depth rank; runs longer than SMALL_RUN are summed by the whole wave.  Fixed summation order -> bitwise reproducible.
constexpr int SMALL_RUN = 16;
template <typename T>
__global__ __launch_bounds__(256) void per_gaussian_sum_kernel(
    int P, const uint32_t* __restrict__ gidx_sorted, const uint32_t* __restrict__ nvalid,
    const uint32_t* __restrict__ offsets_sorted, const uint32_t* __restrict__ tiles_sorted,
    const T* __restrict__ inst, T* __restrict__ out) {
  // one lane per DEPTH RANK: neither the rectangle nor the rank of a Gaussian is looked up.  `out` is all zeros when
  // this launch starts (duplicate_kernel of the same render call streams them out in Gaussian order), and only a rank
  // that kept a tile — on the headline one survivor in a hundred — reads its offset and its Gaussian's index and
  // stores a sum: no scattered store per Gaussian.  The run of such a rank is found with two coalesced words; the long
  // runs sit at neighbouring ranks and are dealt to different waves (strided_rank).
  const int r = strided_rank(P);
  const int lane = threadIdx.x & 63;
  uint32_t n = 0, base = 0;
  if (r >= 0 && (uint32_t)r < *nvalid) {
    n = tiles_sorted[r];
    if (n != 0u) base = offsets_sorted[r] - n;
  }
  T sum = (T)0;
  if (n <= (uint32_t)SMALL_RUN)
    for (uint32_t k = 0; k < n; ++k) sum += inst[base + k];
  unsigned long long m = __ballot(n > (uint32_t)SMALL_RUN);
  while (m) {
    const int src = __ffsll((long long)m) - 1;
    m &= m - 1;
    const uint32_t nb = lane_value(n, src);
    const uint32_t bb = lane_value(base, src);
    T acc = (T)0, acc1 = (T)0, acc2 = (T)0, acc3 = (T)0;
    uint32_t k = lane;
    for (; k + 192 < nb; k += 256) {  // four independent loads in flight
      acc += inst[bb + k];
      acc1 += inst[bb + k + 64];
      acc2 += inst[bb + k + 128];
      acc3 += inst[bb + k + 192];
    }
    for (; k < nb; k += 64) acc += inst[bb + k];
    acc = (acc + acc1) + (acc2 + acc3);
    if constexpr (sizeof(T) == 4 && !std::is_integral<T>::value) {
      acc = wave_sum_to_all(acc);
    } else {
      acc = (T)wave_reduce_sum_u32((uint32_t)acc);
    }
    if (lane == src) sum = acc;
  }
  if (n != 0u) out[gidx_sorted[r]] = sum;
}

// ---------------------------------------------------------------- host: the forward kernels of a BlendPlan
struct FwdOut {   // the image outputs every forward blend kernel writes
  float *color, *normal, *depth, *alpha;
};

// wave per 8x8 quadrant; tile lists of more than two segments in parallel segments (passes T, B, C)
template <int MODE>
static int launch_blend_fwd_wave(const KParams& kp, const BlendPlan& plan, int64_t I, int num_tiles, const GeomState& gs,
                          const BinState& bs, const ImageState& im, const FwdOut& o, hipStream_t st) {
  const uint32_t seg = plan.seg;
  if (I > 0) PINGS_HIP_CHECK(hipMemsetAsync(bs.inst_wq, 0, 16 * (size_t)I, st));
  if (I > 0 && MODE == MODE_3DGS) PINGS_HIP_CHECK(hipMemsetAsync(bs.inst_cntq, 0, 16 * (size_t)I, st));
  if (!plan.seg_on) {
    hipLaunchKernelGGL((blend_fwd_wave_kernel<MODE>), dim3(num_tiles), dim3(256), 0, st, kp, bs.ranges,
                       bs.point_list, gs.rec, bs.gval, o.color, o.normal, o.depth, o.alpha,
                       im.final_T, im.n_contrib, bs.inst_wq, bs.inst_cntq, bs.tile_order,
                       (const uint32_t*)nullptr);
  } else {
    hipLaunchKernelGGL(seg_plan_kernel, dim3(1), dim3(1024), 0, st, bs.ranges, num_tiles, 2u * seg, seg,
                       bs.seg_max_units, bs.seg_head, bs.seg_unit_tile, bs.seg_unit_seg, bs.seg_tile_unit0);
    PINGS_LAUNCH_CHECK();
    // short-list tiles + pass T of the segments in one launch, then pass B and pass C
    const dim3 gseg(bs.seg_max_units);
    uint16_t* const rel = plan.seg_reuse ? bs.seg_rel : nullptr;
    uint32_t* const nrel = plan.seg_reuse ? bs.seg_nrel : nullptr;
    hipLaunchKernelGGL((blend_fwd_wave_segT_kernel<MODE>), dim3((unsigned)num_tiles + bs.seg_max_units), dim3(256), 0,
                       st, kp, bs.ranges, bs.point_list, gs.rec, bs.gval, o.color, o.normal, o.depth,
                       o.alpha, im.final_T, im.n_contrib, bs.inst_wq, bs.inst_cntq, bs.tile_order,
                       bs.seg_tile_unit0, (unsigned)num_tiles, seg, bs.seg_head, bs.seg_unit_tile,
                       bs.seg_unit_seg, bs.seg_P, rel, nrel);
    if (plan.seg_reuse)
      hipLaunchKernelGGL((blend_fwd_seg_kernel<MODE, 1, true>), gseg, dim3(256), 0, st, kp, bs.ranges, bs.point_list,
                         gs.rec, bs.gval, seg, bs.seg_head, bs.seg_unit_tile, bs.seg_unit_seg, bs.seg_P, bs.seg_slab,
                         bs.inst_wq, bs.inst_cntq, rel, nrel);
    else
      hipLaunchKernelGGL((blend_fwd_seg_kernel<MODE, 1, false>), gseg, dim3(256), 0, st, kp, bs.ranges, bs.point_list,
                         gs.rec, bs.gval, seg, bs.seg_head, bs.seg_unit_tile, bs.seg_unit_seg, bs.seg_P, bs.seg_slab,
                         bs.inst_wq, bs.inst_cntq, rel, nrel);
    hipLaunchKernelGGL((blend_fwd_seg_combine_kernel<MODE>), gseg, dim3(256), 0, st, kp, bs.ranges, seg, bs.seg_head,
                       bs.seg_unit_tile, bs.seg_unit_seg, bs.seg_slab, o.color, o.normal, o.depth,
                       o.alpha, im.final_T, im.n_contrib);
    PINGS_LAUNCH_CHECK();
  }
  if (I > 0)
    hipLaunchKernelGGL((combine_quadrants_kernel<MODE>), dim3((unsigned)pings::ceil_div<int64_t>(I, 256)),
                       dim3(256), 0, st, I, reinterpret_cast<const float4*>(bs.inst_wq),
                       reinterpret_cast<const uint4*>(bs.inst_cntq), bs.inst_w, bs.inst_cnt, bs.inst_qmask);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

// With I > 0 `per_gaussian` must be all zeros on `st` before this call: per_gaussian_sum_kernel stores only the sums of
// the Gaussians that kept a tile.  pings_raster_render's duplicate_kernel launch, which runs whenever I > 0, writes them.
int launch_blend_fwd(int mode, const KParams& kp, const BlendPlan& plan, int P, int64_t I, const GeomState& gs,
                     const BinState& bs, const ImageState& im, float* out_color, float* out_normal, float* out_depth,
                     float* out_alpha, void* per_gaussian, hipStream_t st) {
  const int num_tiles = kp.gx * kp.gy;
  const FwdOut o{out_color, out_normal, out_depth, out_alpha};
  {
    pings::prof::Scope ps_blend("blend_fwd", st);
    const int e = with_mode(mode, [&](auto m) -> int {
      constexpr int M = m();
      switch (plan.fwd) {
        case BlendPlan::FWD_TILE:   // (the per-instance sums it stores into were cleared with `ranges`)
          hipLaunchKernelGGL((blend_fwd_tile_kernel<M>), dim3(num_tiles), dim3(64), 0, st, kp, bs.ranges,
                             bs.point_list, gs.rec, bs.gval, o.color, o.normal, o.depth, o.alpha,
                             im.final_T, im.n_contrib, bs.inst_w, bs.inst_cnt, bs.tile_order, bs.tile_maxc);
          break;
        case BlendPlan::FWD_WAVE:
          if (int e = launch_blend_fwd_wave<M>(kp, plan, I, num_tiles, gs, bs, im, o, st)) return e;
      }
      PINGS_LAUNCH_CHECK();
      return PINGS_OK;
    });
    if (e) return e;
  }
  if (P > 0) {
    pings::prof::Scope ps("per_gaussian_sum", st);
    const dim3 grid(pings::ceil_div(P, 256)), block(256);
    if (I == 0) {
      PINGS_HIP_CHECK(hipMemsetAsync(per_gaussian, 0, 4 * (size_t)P, st));
    } else if (mode == PINGS_RASTER_SURFEL) {
      hipLaunchKernelGGL(per_gaussian_sum_kernel<float>, grid, block, 0, st, P, gs.gidx_sorted, gs.nvalid,
                         gs.offsets_sorted, gs.tiles_sorted, (const float*)bs.inst_w,
                         reinterpret_cast<float*>(per_gaussian));
    } else {
      hipLaunchKernelGGL(per_gaussian_sum_kernel<uint32_t>, grid, block, 0, st, P, gs.gidx_sorted, gs.nvalid,
                         gs.offsets_sorted, gs.tiles_sorted, (const uint32_t*)bs.inst_cnt,
                         reinterpret_cast<uint32_t*>(per_gaussian));
    }
    PINGS_LAUNCH_CHECK();
  }
  return PINGS_OK;
}

}  // namespace raster
}  // namespace pings
