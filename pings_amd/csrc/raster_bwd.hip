// Gaussian(-surfel) rasteriser, backward pass, for gfx950.  No floating-point atomics anywhere.
//
//   live scan             cidx = exclusive scan of (inst_w > 0) over the instance slots: only
//                         instances that blended something in the forward pass get a gradient row.
//   blend_bwd_tile_kernel footprint class 2, pixels on the lanes: one wave per 16x16 tile, four pixels per lane,
//                         walks the tile's sorted list back to front in batches of 64 records staged in LDS;
//                         dead instances and records whose footprint misses the tile are skipped.  Each pixel
//                         re-derives alpha / transmittance and forms the 16 per-(pixel, Gaussian) gradient terms
//                         of the blend record; the wave reduces them with a transposed reduce-scatter that starts
//                         with the lane swaps (raster_common.hpp: wave_reduce16_swap; 16 values x 64 lanes -> one
//                         64-B row).  The row is stored ONCE per live instance; the rows of one Gaussian are
//                         contiguous (slot order = depth rank order).
//   blend_bwd_scan_kernel footprint class 1, records on the lanes: one wave per 8x8 quadrant, two wave scans per
//                         pixel instead of a reduction per record; one row per (live instance, quadrant).
//   row_chunk_sum_kernel  balanced first level of the per-Gaussian sum: one 16-lane group per
//                         (Gaussian, chunk of <= 64 rows) pair, lane = column, streaming 64-B rows.
//   gaussian_bwd_*_kernel per Gaussian: adds its chunk partials, then chains through conic / EWA projection /
//                         quaternion / scale / camera transform to the input gradients and the pose-tangent terms
//                         (block-reduced, fixed order).  _rank_: over the depth ranks that own a pair, behind the zero
//                         fill of the blend launch's trailing workgroups (few Gaussians own a row); _index_: in index
//                         order, rows located through the depth rank (most do).
//   tau_reduce_kernel     final fixed-order reduction of the pose-tangent partials.  (Run by the last workgroup of
//                         the chain kernel instead, behind a device-scope fence and a ticket, it saved the launch
//                         and cost 640 us: the release writes back the L2 of the workgroup's XCD, once per workgroup,
//                         while the gradient stores of the others keep it dirty.)
//
// Gradient definitions are those torch autograd derives from oracle/raster_cpu.py (clamps have
// zero gradient where active, min(0.99, .) included).
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <type_traits>

#include "raster_common.hpp"

namespace pings {
namespace raster {

constexpr int BATCH = 64;
// cap on the tiles per frame that blend_bwd_scan_kernel splits over four waves per quadrant (BlendPlan::long_thr)
constexpr uint32_t LONG_TILES_MAX = 2048;
constexpr uint32_t DEAD_ROW = 0xFFFFFFFFu;

// ---------------------------------------------------------------- blend backward, pixel-per-lane, wave per 16x16 tile
// Footprint class 2: ONE wave owns the 16x16 tile, four pixels per lane (lane -> pixel map of blend_fwd_tile_kernel:
// pixel (h, r) of lane l is (8h + (l & 7), 8r + (l >> 3)) in the tile).  The 16 gradient terms of a lane's four pixels
// are summed in registers before the wave reduction, which is the expensive part: the per-record overhead (LDS record
// fetch, 16-value wave reduction) is paid once per 256 pixels.  A lane's two pixels of a row (h = 0, 1) are computed as
// one packed pair (f2: .x = left half, .y = right half): they share the row's dy / ry terms, their x terms are one
// packed value, and nearly every per-pixel operation becomes one v_pk_* instruction for two pixels.  Only exp and the
// reciprocals stay scalar.  The alpha / validity decisions are the forward pass's operations, component for component
// (packed multiplies and adds round each component as the scalar ones do; no contraction there).
template <int MODE>
__device__ __forceinline__ void blend_bwd_tile_body(
    BParams p, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
    const float4* __restrict__ rec, const uint32_t* __restrict__ gval, const float* __restrict__ final_T,
    const uint32_t* __restrict__ n_contrib, const float* __restrict__ out_depth, const float* __restrict__ dL_dcolor,
    const float* __restrict__ dL_dnormal, const float* __restrict__ dL_ddepth, const float* __restrict__ dL_dalpha,
    const float* __restrict__ inst_w, const uint32_t* __restrict__ cidx, float* __restrict__ rows,
    const uint32_t* __restrict__ tile_order, int interior_on) {
  __shared__ float4 sA[BATCH], sB[BATCH], sC[BATCH], sD[BATCH];
  __shared__ uint32_t sRow[BATCH];  // compact gradient-row index, DEAD_ROW for dead instances
  __shared__ float4 sG[BATCH][4];
  __shared__ uint8_t sList[BATCH];  // live records of the batch that may reach the tile (ascending)
  __shared__ uint8_t sInt[BATCH];   // 1: the record is interior to the tile (raster_common.hpp: blend_interior)

  const int lane = threadIdx.x;
  const int tile = (int)tile_order[blockIdx.x];   // longest-processing-time-first dispatch (raster_fwd.hip)
  const int tx = tile % p.gx, ty = tile / p.gx;
  const int pix_x = tx * TILE + (lane & 7), pix_y0 = ty * TILE + (lane >> 3);
  const f2 pixf_x = {(float)pix_x, (float)(pix_x + 8)};
  const float pixf_y[2] = {(float)pix_y0, (float)(pix_y0 + 8)};
  const float tileX0 = (float)(tx * TILE), tileY0 = (float)(ty * TILE);
  const size_t HW = (size_t)p.W * p.H;

  f2 rx = {0.f, 0.f};
  float ry[2] = {0.f, 0.f};
  TileRays rays = {0.f, 0.f, 0.f, 0.f};
  if (MODE == MODE_SURFEL) {
    const float cxp = (p.prcp ? p.prcp[0] : 0.5f) * (float)p.W - 0.5f;
    const float cyp = (p.prcp ? p.prcp[1] : 0.5f) * (float)p.H - 0.5f;
    rx = f2{(pixf_x.x - cxp) / p.fx, (pixf_x.y - cxp) / p.fx};
#pragma unroll
    for (int r = 0; r < 2; ++r) ry[r] = (pixf_y[r] - cyp) / p.fy;
    rays = tile_rays_uniform(tile_rays(tileX0, tileY0, cxp, cyp, p.fx, p.fy));
  }

  const uint2 range = ranges[tile];
  // per row r, component h: the pixel (h, r)
  uint32_t last[2][2];
  f2 T[2], gC0[2], gC1[2], gC2[2], gN0[2], gN1[2], gN2[2], gD[2];
  // Bs: blend of s = (upstream gradient) . (record features) over the records behind, normalised, MINUS
  // coefT / T with coefT = (dL/dalpha_out - bg . dL/dcolor) T_final.  The offset is what makes
  //   dL/dalpha_rec = (s - Bs_true) Tn + coefT / (1 - alpha) = (s - Bs) Tn
  // hold with T the transmittance behind the record and Tn = T / (1 - alpha) in front of it, and Bs keeps the same
  // recurrence Bs <- Bs + alpha (s - Bs): the offset -coefT / T turns into -coefT / Tn exactly when alpha is blended
  // in.  It starts at -coefT / T_final = bg . dL/dcolor - dL/dalpha_out, and no per-pixel coefT is carried.
  f2 Bs[2];
  uint32_t lmax = 0;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    T[r] = f2{1.f, 1.f};
    gC0[r] = gC1[r] = gC2[r] = gN0[r] = gN1[r] = gN2[r] = gD[r] = Bs[r] = f2{0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      last[r][h] = 0;
      const int pix_y = pix_y0 + 8 * r, pix_xh = pix_x + 8 * h;
      if (pix_xh < p.W && pix_y < p.H) {
        const size_t pix_id = (size_t)pix_y * p.W + pix_xh;
        last[r][h] = n_contrib[pix_id];
        const float T_final = final_T[pix_id];
        T[r][h] = T_final;
        float c0 = 0.f, c1 = 0.f, c2 = 0.f;
        if (dL_dcolor) {
          c0 = dL_dcolor[pix_id];
          c1 = dL_dcolor[HW + pix_id];
          c2 = dL_dcolor[2 * HW + pix_id];
        }
        gC0[r][h] = c0;
        gC1[r][h] = c1;
        gC2[r][h] = c2;
        float gA = dL_dalpha ? dL_dalpha[pix_id] : 0.f;
        const float gDo = dL_ddepth ? dL_ddepth[pix_id] : 0.f;
        if (MODE == MODE_SURFEL) {
          if (dL_dnormal) {
            gN0[r][h] = dL_dnormal[pix_id];
            gN1[r][h] = dL_dnormal[HW + pix_id];
            gN2[r][h] = dL_dnormal[2 * HW + pix_id];
          }
          const float A = 1.0f - T_final;
          if (A > DEPTH_ALPHA_EPS) {
            gD[r][h] = gDo / A;
            gA -= gDo * out_depth[pix_id] / A;
          }
        } else {
          gD[r][h] = gDo;
        }
        Bs[r][h] = ((p.bg[0] * c0 + p.bg[1] * c1) + p.bg[2] * c2) - gA;
      }
      lmax = max(lmax, last[r][h]);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) lmax = max(lmax, (uint32_t)__shfl_xor((int)lmax, off, 64));
  const int max_last = __builtin_amdgcn_readfirstlane((int)lmax);
  // the 0.5 of the cov2D xx / yy gradient terms, applied to the reduced sums (wave_reduce16_swap: the first four lanes
  // of each 16-lane row hold the record's row, lane l slot red_slot)
  const int red_slot = red16_lane_slot(lane);
  const bool red_store = (lane & 12) == 0;
  const float red_scale = (red_slot == G_CONX || red_slot == G_CONZ) ? 0.5f : 1.0f;

  const int nbatch = ceil_div(max_last, BATCH);
  for (int b = nbatch - 1; b >= 0; --b) {
    const int start = b * BATCH;
    const int n = min(BATCH, max_last - start);
    __syncthreads();  // previous batch's LDS fully consumed
    bool hit = false;
    if (lane < n) {
      const uint32_t slot = point_list[range.x + start + lane];
      const uint32_t g = gval[slot];
      const float4 ra = rec[4 * (size_t)g + 0];
      const float4 rb = rec[4 * (size_t)g + 1];
      sA[lane] = ra;
      sB[lane] = rb;
      const float4 rc = rec[4 * (size_t)g + 2];
      sC[lane] = rc;
      float4 rd = make_float4(0.f, 0.f, 0.f, 0.f);
      if (MODE == MODE_SURFEL) sD[lane] = rd = rec[4 * (size_t)g + 3];
      const bool live = inst_w[slot] > 0.f;  // blended something in the forward pass
      sRow[lane] = live ? cidx[slot] : DEAD_ROW;
      if (live) hit = quadrant_mask(ra.x, ra.y, ra.z, rb.x, rb.y, rb.z, tileX0, tileY0) != 0u;
      // records interior to the tile take the lean trip below; the flags become one scalar mask over the list
      if (MODE == MODE_SURFEL)
        sInt[lane] = hit && interior_on && blend_interior(ra.x, ra.y, ra.z, ra.w, rb.x, rb.y, rb.z, rb.w, rc.w, rd.x, rd.y,
                                                          rd.z, tileX0, tileY0, rays) ? 1 : 0;
    }
    const unsigned long long bal = __ballot(hit);
    if (hit) sList[__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u))] = (uint8_t)lane;
    const int cnt = __popcll(bal);
    {
      float4* z = &sG[0][0];
      const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int e = lane; e < BATCH * 4; e += 64) z[e] = zero;
    }
    __syncthreads();
    unsigned long long int_bits = 0ull;   // bit jj: list entry jj is interior (wave-uniform)
    if (MODE == MODE_SURFEL) int_bits = __ballot(lane < cnt && sInt[sList[lane < cnt ? lane : 0] & (BATCH - 1)] != 0);

    // Two-deep software pipeline over the list: the INDEX of record jj-2 and the RECORD jj-1 are fetched from LDS
    // while record jj is processed, so neither LDS latency sits in an iteration's dependency chain.
    // The loop is unrolled by two over two register sets: a trip reads its record from one set while the next record
    // goes straight into the other, so nothing is copied from "next" to "current" (8 v_mov_b64 + 9 v_mov_b32 a trip).
    int i0 = cnt > 0 ? (int)sList[cnt - 1] : 0;
    int i1 = cnt > 1 ? (int)sList[cnt - 2] : 0;
    float4 a0 = sA[i0], b0 = sB[i0], c0 = sC[i0], n0 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 a1, b1, c1, n1 = n0;
    if (MODE == MODE_SURFEL) n0 = sD[i0];
    // INT: the trip of a record interior to the tile (blend_interior: every pixel passes the alpha tests unclamped and
    // takes the unclamped ray hit).  It leaves out the decisions and the three rows that are exactly zero for such a
    // record (G_ZLO, G_ZHI, G_PZ); everything it keeps is the general trip's, operation for operation, so both give the
    // same bits wherever the classifier holds.
    auto trip = [&](auto interior_c, const float4& ca, const float4& cb, const float4& cc, const float4& cn, const int j)
                    __attribute__((always_inline)) {
      constexpr bool INT = MODE == MODE_SURFEL && decltype(interior_c)::value;
      const uint32_t idx = (uint32_t)(start + j);
      // the forward pass's alpha and validity, operation for operation (blend_fwd_tile_kernel)
      const f2 dx = f2s(ca.x) - pixf_x;
      const f2 p0 = f2s(-0.5f) * ((f2s(cb.x) * dx) * dx);
      const f2 pxy = f2s(cb.y) * dx;
      f2 Gs[2], raw[2], alpha[2];
      float dyv[2];
      bool valid[2][2];
      bool any_v = false;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const float dy = ca.y - pixf_y[r];
        dyv[r] = dy;
        const f2 power = (p0 - f2s(0.5f * (cb.z * dy * dy))) - pxy * f2s(dy);
        Gs[r] = f2{__expf(power.x), __expf(power.y)};
        raw[r] = f2s(ca.z) * Gs[r];
        alpha[r] = INT ? raw[r] : f2{fminf(ALPHA_MAX, raw[r].x), fminf(ALPHA_MAX, raw[r].y)};
        valid[r][0] = idx < last[r][0] && (INT || ((power.x <= 0.0f) && (alpha[r].x >= ALPHA_MIN)));
        valid[r][1] = idx < last[r][1] && (INT || ((power.y <= 0.0f) && (alpha[r].y >= ALPHA_MIN)));
        any_v = any_v || valid[r][0] || valid[r][1];
      }
      if (!__any(any_v)) return;

      // gradient accumulation only: multiply-adds may fuse here (fewer instructions, one rounding less per term).
      // The first row assigns the 16 packed accumulators, the second adds to them; they are folded once per record.
      {
#pragma clang fp contract(fast)
      f2 v2[16];
      if (MODE != MODE_SURFEL) v2[G_NX] = v2[G_NY] = v2[G_NZ] = v2[G_Q] = v2[G_ZLO] = v2[G_ZHI] = f2{0.f, 0.f};
      if (INT) v2[G_ZLO] = v2[G_ZHI] = v2[G_PZ] = f2{0.f, 0.f};
      const float zlo = ca.w - cb.w, zhi = ca.w + cb.w;
      const float zlo_m = fminf(zlo, zhi);   // med3(d, min(lo, hi), hi) == fminf(fmaxf(d, lo), hi) for non-NaN d
      const f2 cxdx = f2s(cb.x) * dx;        // q = conic . (dx, dy) as two adds per pixel
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const bool first = r == 0;
        auto acc = [&](int q, f2 x) { v2[q] = first ? x : v2[q] + x; };
        // Validity folded into alpha: an invalid pixel blends av = 0, so 1 - av = 1, rcp(1) = 1 exactly and Tn == T
        // bit for bit; w = av * Tn and T = Tn need no select.
        const f2 av = sel2(valid[r][0], valid[r][1], alpha[r], f2{0.f, 0.f});
        const f2 one_m = f2s(1.0f) - av;
        const f2 inv_one_m = {__builtin_amdgcn_rcpf(one_m.x), __builtin_amdgcn_rcpf(one_m.y)};  // alpha <= 0.99
        const f2 Tn = T[r] * inv_one_m;
        const f2 w = av * Tn;
        // dL/dalpha needs sum_ch (feature_ch - B_ch) g_ch with B the normalised blend of the records behind.  Both
        // the blend recurrence and the dot product are linear, so ONE scalar per pixel is tracked instead of the
        // eight channels:  s = g . feature,  dLda = s - Bs,  Bs <- Bs + alpha (s - Bs).
        f2 sdot = (f2s(cc.x) * gC0[r] + f2s(cc.y) * gC1[r]) + f2s(cc.z) * gC2[r];
        acc(G_R, gC0[r] * w);
        acc(G_G, gC1[r] * w);
        acc(G_B, gC2[r] * w);
        if (MODE == MODE_SURFEL) {
          sdot += (f2s(cn.x) * gN0[r] + f2s(cn.y) * gN1[r]) + f2s(cn.z) * gN2[r];
          // per-pixel depth of this surfel
          const f2 den = fma2(f2s(cn.x), rx, f2s(fmaf(cn.y, ry[r], cn.z)));
          const f2 inv_den = {__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)};
          f2 d0 = f2s(cc.w) * inv_den, gq;
          if (INT) {
            sdot = fma2(d0, gD[r], sdot);
            // rounded on its own as in the general trip, where a select stands between the product and the sum
            gq = mul_rounded(gD[r] * w, inv_den);
          } else {
            const bool hit0 = den.x < -DEN_EPS, hit1 = den.y < -DEN_EPS;
            d0 = sel2(hit0, hit1, d0, f2s(ca.w));
            const f2 d = {__builtin_amdgcn_fmed3f(d0.x, zlo_m, zhi), __builtin_amdgcn_fmed3f(d0.y, zlo_m, zhi)};
            sdot = fma2(d, gD[r], sdot);
            const f2 gd = gD[r] * w;
            const bool lo0 = d0.x < zlo, lo1 = d0.y < zlo, hi0 = d0.x > zhi, hi1 = d0.y > zhi;
            const bool mid0 = !lo0 && !hi0, mid1 = !lo1 && !hi1;
            const f2 zero = {0.f, 0.f};
            acc(G_ZLO, sel2(lo0, lo1, gd, zero));
            acc(G_ZHI, sel2(hi0, hi1, gd, zero));
            gq = sel2(mid0 && hit0, mid1 && hit1, gd * inv_den, zero);
            acc(G_PZ, sel2(mid0 && !hit0, mid1 && !hit1, gd, zero));
          }
          acc(G_Q, gq);
          const f2 gden = -gq * d0;  // = -gd * d0 / den on the unclamped ray hit, else 0
          v2[G_NX] = fma2(gden, rx, first ? gN0[r] * w : fma2(gN0[r], w, v2[G_NX]));
          v2[G_NY] = fma2(gden, f2s(ry[r]), first ? gN1[r] * w : fma2(gN1[r], w, v2[G_NY]));
          v2[G_NZ] = fma2(gN2[r], w, first ? gden : v2[G_NZ] + gden);
        } else {
          sdot = fma2(f2s(ca.w), gD[r], sdot);
          acc(G_PZ, gD[r] * w);
        }
        f2 dLda = sdot - Bs[r];
        Bs[r] = fma2(av, dLda, Bs[r]);
        dLda = dLda * Tn;
        // alpha = min(0.99, opacity * G): no gradient through the clamp when it is active
        dLda = sel2(valid[r][0] && (INT || raw[r].x <= ALPHA_MAX), valid[r][1] && (INT || raw[r].y <= ALPHA_MAX), dLda,
                    f2{0.f, 0.f});
        acc(G_OPAC, Gs[r] * dLda);
        const f2 dLp = raw[r] * dLda;  // dL/dpower = G * (opacity * dL/dalpha)
        // q = conic . d.  d power / d mean = -q, and d power / d cov2D = 0.5 q q^T: accumulating the
        // gradient w.r.t. the 2-D COVARIANCE here (instead of w.r.t. the conic, to be pushed through
        // -conic G conic afterwards) keeps every per-pixel term O(1); the conic form sums d d^T terms
        // of order 1e6 that must cancel to O(1) for large anisotropic footprints, which fp32 cannot do.
        // The 0.5 of the xx / yy terms is applied once to the reduced sums (exact: a power of two).
        const f2 qx = cxdx + f2s(cb.y * dyv[r]), qy = pxy + f2s(cb.z * dyv[r]);
        const f2 ux = dLp * qx, uy = dLp * qy;
        acc(G_MX, -ux);
        acc(G_MY, -uy);
        acc(G_CONX, ux * qx);
        acc(G_CONY, ux * qy);
        acc(G_CONZ, uy * qy);
        T[r] = Tn;
      }
      const float tot = wave_reduce16_swap<MODE != MODE_SURFEL ? RED_ZERO6 : INT ? RED_ZERO3 : RED_FULL>(v2, lane) * red_scale;
      if (red_store) reinterpret_cast<float*>(&sG[j][0])[red_slot] = tot;
      }
    };
    for (int jj = cnt - 1; jj >= 0; jj -= 2) {
      {  // record i0 from set 0; set 1 takes record i1, i0 the index two trips ahead
        const int j = i0;
        a1 = sA[i1]; b1 = sB[i1]; c1 = sC[i1];
        if (MODE == MODE_SURFEL) n1 = sD[i1];
        i0 = (int)sList[jj > 1 ? jj - 2 : 0];
        if ((int_bits >> jj) & 1ull) trip(std::true_type{}, a0, b0, c0, n0, j);
        else trip(std::false_type{}, a0, b0, c0, n0, j);
      }
      if (jj == 0) break;
      {  // record i1 from set 1; set 0 takes record i0
        const int j = i1;
        a0 = sA[i0]; b0 = sB[i0]; c0 = sC[i0];
        if (MODE == MODE_SURFEL) n0 = sD[i0];
        i1 = (int)sList[jj > 2 ? jj - 3 : 0];
        if ((int_bits >> (jj - 1)) & 1ull) trip(std::true_type{}, a1, b1, c1, n1, j);
        else trip(std::false_type{}, a1, b1, c1, n1, j);
      }
    }
    __syncthreads();
    for (int e = lane; e < n * 4; e += 64) {
      const int j = e >> 2, part = e & 3;
      if (sRow[j] != DEAD_ROW) reinterpret_cast<float4*>(rows)[(size_t)sRow[j] * 4 + part] = sG[j][part];
    }
  }
}

// Zeros for the six per-Gaussian gradient arrays (why they start at zero: the per-Gaussian chain, below).  One workgroup
// writes slice `part` of `nparts`: 16-byte stores, no reads; an array's unaligned head and its tail go out as single
// floats.  The stores are nontemporal: nobody reads the zeros soon, and as ordinary stores at the end of the blend
// launch the 68 P bytes pushed the gradient rows out of the cache in front of row_chunk_sum_kernel, which reads them
// next (headline: 9.8 -> 12.5 - 14.3 us; nontemporal 9.8 - 10.2 us, profiles/r16).
struct GradFill {
  float* ptr[6];
  size_t count[6];   // floats
};
typedef float v4f __attribute__((ext_vector_type(4)));
__device__ inline void grad_fill_part(const GradFill& f, uint32_t part, uint32_t nparts) {
  const size_t tid = (size_t)part * blockDim.x + threadIdx.x, nthreads = (size_t)nparts * blockDim.x;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    float* const p = f.ptr[a];
    const size_t n = f.count[a];
    const size_t head = min(n, (size_t)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2);
    const size_t nvec = (n - head) >> 2;
    v4f* const body = reinterpret_cast<v4f*>(p + head);
    for (size_t i = tid; i < nvec; i += nthreads) __builtin_nontemporal_store(v4f{0.f, 0.f, 0.f, 0.f}, body + i);
    const size_t tail = head + 4 * nvec;   // fewer than four floats each: the first threads take them
    if (tid < head) p[tid] = 0.f;
    if (tid < n - tail) p[tail + tid] = 0.f;
  }
}

// The kernel is its body inlined (as blend_fwd_wave_kernel is blend_fwd_wave_body).  With the body written straight
// into the __global__ function the compiler handles `p` differently (kernel argument, not a by-value copy), and the
// record loop came out with other operand orders and a slightly different schedule: 0.306 -> 0.311 ms on the Metric-1
// cloud in one A/B, at the edge of the run-to-run spread.  This form compiles to the same instructions as before.
//
// The workgroups behind the last tile (blockIdx.x >= num_tiles; none when the grid is num_tiles) write the zeros of
// the six per-Gaussian gradient arrays and leave: workgroups are dispatched in order, so they start when the last
// tile waves have started and the longest-first schedule begins to free wave slots, and their stores go out beside
// the tail of the tile waves instead of in a launch of their own.  No tile wave runs an instruction more.
template <int MODE>
__global__ __launch_bounds__(64, 3) void blend_bwd_tile_kernel(
    BParams p, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
    const float4* __restrict__ rec, const uint32_t* __restrict__ gval, const float* __restrict__ final_T,
    const uint32_t* __restrict__ n_contrib, const float* __restrict__ out_depth, const float* __restrict__ dL_dcolor,
    const float* __restrict__ dL_dnormal, const float* __restrict__ dL_ddepth, const float* __restrict__ dL_dalpha,
    const float* __restrict__ inst_w, const uint32_t* __restrict__ cidx, float* __restrict__ rows,
    const uint32_t* __restrict__ tile_order, uint32_t num_tiles, GradFill fill, int interior_on) {
  if (blockIdx.x >= num_tiles) {
    grad_fill_part(fill, blockIdx.x - num_tiles, gridDim.x - num_tiles);
    return;
  }
  blend_bwd_tile_body<MODE>(p, ranges, point_list, rec, gval, final_T, n_contrib, out_depth, dL_dcolor, dL_dnormal,
                            dL_ddepth, dL_dalpha, inst_w, cidx, rows, tile_order, interior_on);
}

// ---------------------------------------------------------------- blend backward, Gaussian-per-lane ("wave64 scan")
// The kernel above puts PIXELS on the lanes: the 16 gradient terms of a record then have to be summed over the wave
// for every record (a 16 x 64 reduce-scatter, ~60 of the ~250 instructions of an iteration), and eight blend
// channels are walked per pixel.  Here RECORDS are on the lanes.  One wave owns one 8x8 quadrant of a tile and walks
// the tile list back to front; the records that blended something in this quadrant (the forward pass left a 4-bit
// quadrant mask per instance) are compacted, 64 at a time, onto the lanes — lane 0 the rearmost.  For each of the
// quadrant's 64 pixels (uniform across the wave) every lane evaluates its record's alpha; the transmittance in
// front of each record is the pixel's running transmittance divided by an inclusive PREFIX PRODUCT of (1 - alpha)
// over the lanes, and the colour / normal / depth blended behind it collapses, after the dot product with the
// pixel's upstream gradient, into an exclusive PREFIX SUM of one scalar (w s): two DPP wave scans per pixel replace
// the per-record reduction, and the 16 gradient terms simply accumulate in the lane's registers over the 64
// pixels.  Each lane stores its 64-byte row once per (instance, quadrant); rows of one Gaussian stay contiguous and
// are summed by the same per-Gaussian kernels.  Waves never synchronise with each other; pixels that finished
// before the chunk are skipped for the whole wave.  Bitwise reproducible (fixed pixel order per lane).
// work estimate of a tile for the dispatch order: the largest n_contrib of its 256 pixels (one wave per tile)
__global__ __launch_bounds__(64) void tile_max_contrib_kernel(int W, int H, int gx, const uint32_t* __restrict__ n_contrib,
                                                              uint32_t* __restrict__ work) {
  const int tile = blockIdx.x, lane = threadIdx.x;
  const int tx = tile % gx, ty = tile / gx;
  uint32_t m = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int x = tx * TILE + (lane & 15), y = ty * TILE + 4 * r + (lane >> 4);
    if (x < W && y < H) m = max(m, n_contrib[(size_t)y * W + x]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
  if (lane == 0) work[tile] = m;
}

template <int CTRL, int ROW_MASK>
__device__ inline float dpp_f(float old, float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v),
                                                                CTRL, ROW_MASK, 0xf, false));
}

__device__ inline float wave_incl_scan_mul(float x) {
  x *= dpp_f<0x111, 0xf>(1.f, x);  // row_shr:1
  x *= dpp_f<0x112, 0xf>(1.f, x);  // row_shr:2
  x *= dpp_f<0x114, 0xf>(1.f, x);  // row_shr:4
  x *= dpp_f<0x118, 0xf>(1.f, x);  // row_shr:8
  x *= dpp_f<0x142, 0xa>(1.f, x);  // row_bcast:15 -> rows 1, 3
  x *= dpp_f<0x143, 0xc>(1.f, x);  // row_bcast:31 -> rows 2, 3
  return x;
}

__device__ inline float wave_incl_scan_add(float x) {
  x += dpp_f<0x111, 0xf>(0.f, x);
  x += dpp_f<0x112, 0xf>(0.f, x);
  x += dpp_f<0x114, 0xf>(0.f, x);
  x += dpp_f<0x118, 0xf>(0.f, x);
  x += dpp_f<0x142, 0xa>(0.f, x);
  x += dpp_f<0x143, 0xc>(0.f, x);
  return x;
}

// value of lane - 1 (lane 0 gets `first`)
__device__ inline float wave_shr1(float x, float first) { return dpp_f<0x138, 0xf>(first, x); }

// The same scans inside lane GROUPS of G = 16 / 32 / 64 lanes (a 16-lane DPP row, a half wave, the wave): a chunk with
// at most G records puts 64 / G pixels on the wave at once, each on its own group (grp_* below).
template <int G>
__device__ inline float grp_incl_scan_mul(float x) {
  x *= dpp_f<0x111, 0xf>(1.f, x);
  x *= dpp_f<0x112, 0xf>(1.f, x);
  x *= dpp_f<0x114, 0xf>(1.f, x);
  x *= dpp_f<0x118, 0xf>(1.f, x);
  if (G >= 32) x *= dpp_f<0x142, 0xa>(1.f, x);
  if (G >= 64) x *= dpp_f<0x143, 0xc>(1.f, x);
  return x;
}
template <int G>
__device__ inline float grp_incl_scan_add(float x) {
  x += dpp_f<0x111, 0xf>(0.f, x);
  x += dpp_f<0x112, 0xf>(0.f, x);
  x += dpp_f<0x114, 0xf>(0.f, x);
  x += dpp_f<0x118, 0xf>(0.f, x);
  if (G >= 32) x += dpp_f<0x142, 0xa>(0.f, x);
  if (G >= 64) x += dpp_f<0x143, 0xc>(0.f, x);
  return x;
}
// value of the previous lane of the group (the group's first lane gets `first`)
template <int G>
__device__ inline float grp_shr1(float x, float first, int lane) {
  if (G == 16) return dpp_f<0x111, 0xf>(first, x);          // row_shr:1, lanes without a source keep `first`
  const float y = dpp_f<0x138, 0xf>(first, x);               // wave_shr:1
  return (G == 32 && lane == 32) ? first : y;
}

#ifdef PINGS_BWD_STATS
#define STATS_PARAMS , unsigned long long& st_dead, unsigned long long& st_any, unsigned long long& st_exec, unsigned long long& st_valid
#define STATS_ARGS , st_dead, st_any, st_exec, st_valid
#else
#define STATS_PARAMS
#define STATS_ARGS
#endif

// The pixel loop of blend_bwd_scan_kernel for one chunk of `take` <= G records: 64 / G pixels per step, lane l = record
// l % G of pixel pp0 + l / G (records are replicated over the groups by the caller).  Per pixel the arithmetic is the
// one-pixel form's, op for op; a lane's 16 sums run over its group's pixels and the groups are added at the end
// (fixed order: deterministic).
// Pixels [pix0, pix0 + NPIX) of the quadrant: all 64 for a wave that owns the quadrant, 16 (two pixel rows) for each of
// the four waves that share a long-list quadrant.
template <int MODE, int G, int NPIX>
__device__ inline void scan_pixels(float4 (*sPix)[4], int lane, int pix0, int e, int min_e, const float4& a,
                                   const float4& b, const float4& c, const float4& nn, float (&v)[16] STATS_PARAMS) {
  constexpr int NG = 64 / G;
  const int grp = lane / G;
  const float zlo = a.w - b.w, zhi = a.w + b.w;
  for (int pp0 = 0; pp0 < NPIX; pp0 += NG) {
    const int pp = pix0 + pp0 + grp;
    const float4 s0 = sPix[pp][0];
    const int last_p = (int)__float_as_uint(s0.z);
    if (!__any(last_p > min_e)) {                      // these pixels had stopped before the chunk's first record
#ifdef PINGS_BWD_STATS
      st_dead += NG;
#endif
      continue;
    }
    const float4 s1 = sPix[pp][1], s2 = sPix[pp][2], s3 = sPix[pp][3];
    const float T_p = s0.x, R_p = s0.y, coefT = s0.w;
    const float dx = a.x - s2.w;
    const float dy = a.y - s3.x;
    const float p0 = -0.5f * (b.x * dx * dx);
    const float pxy = b.y * dx;
    const float power = (p0 - 0.5f * (b.z * dy * dy)) - pxy * dy;   // the forward pass' op order
    const float Gs = __expf(power);
    const float raw = a.z * Gs;
    const float alpha = fminf(ALPHA_MAX, raw);
    const bool valid = (e < last_p) && (power <= 0.0f) && (alpha >= ALPHA_MIN);
#ifdef PINGS_BWD_STATS
    if (!__any(valid)) st_any += NG; else { st_exec += NG; st_valid += (unsigned)__popcll(__ballot(valid)); }
#endif
    if (!__any(valid)) continue;                          // no record reaches any of these pixels: their state
                                                          // (T / 1, R + 0) and every gradient sum stay as they are
    const float av = valid ? alpha : 0.f;
    const float P_in = grp_incl_scan_mul<G>(1.0f - av);   // product of (1 - alpha) over this and the records behind
    const float P_ex = grp_shr1<G>(P_in, 1.0f, lane);
    const float inv_P = __builtin_amdgcn_rcpf(P_in);
    const float Tn = T_p * inv_P;                        // transmittance in front of this record
    const float inv_one_m = P_ex * inv_P;                // 1 / (1 - alpha)
    const float w = av * Tn;
    float S_in;
    {
    // gradient accumulation only (alpha / validity were decided above in the forward pass' op order): multiply-adds
    // may fuse here
#pragma clang fp contract(fast)
    // s = (upstream gradient) . (features of this record at this pixel)
    float sdot = (c.x * s1.x + c.y * s1.y) + c.z * s1.z;
    v[G_R] = fmaf(s1.x, w, v[G_R]);
    v[G_G] = fmaf(s1.y, w, v[G_G]);
    v[G_B] = fmaf(s1.z, w, v[G_B]);
    if (MODE == MODE_SURFEL) {
      sdot += (nn.x * s2.x + nn.y * s2.y) + nn.z * s2.z;
      const float den = (nn.x * s3.y + nn.y * s3.z) + nn.z;
      const bool hit = den < -DEN_EPS;
      const float inv_den = __builtin_amdgcn_rcpf(den);
      const float d0 = hit ? c.w * inv_den : a.w;
      const float d = fminf(fmaxf(d0, zlo), zhi);
      sdot = fmaf(d, s1.w, sdot);
      const float gd = s1.w * w;
      const bool lo = d0 < zlo, hi = d0 > zhi;
      const bool mid = !lo && !hi;
      v[G_ZLO] += lo ? gd : 0.f;
      v[G_ZHI] += hi ? gd : 0.f;
      const float gq = (mid && hit) ? gd * inv_den : 0.f;
      v[G_Q] += gq;
      v[G_PZ] += (mid && !hit) ? gd : 0.f;
      const float gden = -gq * d0;
      v[G_NX] += fmaf(gden, s3.y, s2.x * w);
      v[G_NY] += fmaf(gden, s3.z, s2.y * w);
      v[G_NZ] += s2.z * w + gden;
    } else {
      sdot = fmaf(a.w, s1.w, sdot);
      v[G_PZ] = fmaf(s1.w, w, v[G_PZ]);
    }
    const float ws = w * sdot;
    S_in = grp_incl_scan_add<G>(ws);                     // w s over this and the records behind (in the chunk)
    const float R_l = R_p + grp_shr1<G>(S_in, 0.f, lane); // blended behind this record, dotted with the gradient
    // dL/dalpha = T s - (R - coefT) / (1 - alpha)
    float dLda = fmaf(Tn, sdot, (coefT - R_l) * inv_one_m);
    dLda = (valid && raw <= ALPHA_MAX) ? dLda : 0.f;     // no gradient through the active 0.99 clamp
    v[G_OPAC] = fmaf(Gs, dLda, v[G_OPAC]);
    const float dLp = raw * dLda;
    const float qx = b.x * dx + b.y * dy, qy = b.y * dx + b.z * dy;
    v[G_MX] -= dLp * qx;
    v[G_MY] -= dLp * qy;
    v[G_CONX] += 0.5f * qx * qx * dLp;
    v[G_CONY] += qx * qy * dLp;
    v[G_CONZ] += 0.5f * qy * qy * dLp;
    }
    if ((lane & (G - 1)) == G - 1) {                     // the group's last lane: pixel state after the whole chunk
      sPix[pp][0].x = Tn;
      sPix[pp][0].y = R_p + S_in;
    }
  }
  if (G < 64) {                                          // the groups hold partial sums of the SAME records: add them
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (G == 16) v[k] += __shfl_xor(v[k], 16, 64);
      v[k] += __shfl_xor(v[k], 32, 64);
    }
  }
}

#ifdef PINGS_BWD_STATS  // diagnostic build only: loop-efficiency counters of blend_bwd_scan_kernel
__device__ unsigned long long g_bwd_stats[8];
#endif

// Workgroups of four waves.  A tile of ordinary length takes one workgroup, wave w = quadrant w.  A LONG tile (largest
// per-pixel contributor count >= the long-list threshold: the first *n_long entries of the descending tile order)
// takes four workgroups, one per quadrant, whose four waves share the quadrant — 16 pixels each, all walking the same
// chunks; a record's four partial rows are added in LDS (wave order: deterministic).  With one wave per quadrant
// throughout, the launch waited for the few waves with the longest lists (C3 street: longest wave 59 chunks, about
// 0.6 of the kernel's 0.70 ms; mean 4.8).  Long tiles come first in the grid; a second launch for them would run
// alone on the chip (measured: slower than no split at all).
template <int MODE>
__global__ __launch_bounds__(256) void blend_bwd_scan_kernel(
    BParams p, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
    const float4* __restrict__ rec, const uint32_t* __restrict__ gval, const float* __restrict__ final_T,
    const uint32_t* __restrict__ n_contrib, const float* __restrict__ out_depth, const float* __restrict__ dL_dcolor,
    const float* __restrict__ dL_dnormal, const float* __restrict__ dL_ddepth, const float* __restrict__ dL_dalpha,
    const uint8_t* __restrict__ qmask, const uint32_t* __restrict__ cidx, float* __restrict__ rows,
    const uint32_t* __restrict__ tile_order, const uint32_t* __restrict__ n_long) {
  // pixel state, per quadrant: {T, R, last, coefT} {gC0, gC1, gC2, gD} {gN0, gN1, gN2, px} {py, rx, ry, -}
  // ordinary tile: four quadrants x 64 pixels x 4; long tile: the first quarter + the waves' partial rows of a chunk
  __shared__ float4 sBuf[256 + 1024];
  __shared__ int sQeAll[4][128];        // per wave: queue of relevant list entries, back to front
  __shared__ uint32_t sQsAll[4][128];   // their instance slots

  const int lane = threadIdx.x & 63, wv = (int)(threadIdx.x >> 6);
  int* sQe = sQeAll[wv];
  uint32_t* sQs = sQsAll[wv];
  const uint32_t nl = *n_long;
  const bool lng = blockIdx.x < 4u * nl;
  int tile, q;
  if (lng) {
    tile = (int)tile_order[blockIdx.x >> 2];
    q = (int)(blockIdx.x & 3);
  } else {
    const uint32_t ti = nl + (blockIdx.x - 4u * nl);
    if (ti >= (uint32_t)(p.gx * p.gy)) return;
    tile = (int)tile_order[ti];
    q = wv;
  }
  float4 (*sPix)[4] = reinterpret_cast<float4 (*)[4]>(sBuf + (lng ? 0 : 256 * wv));
  float (*sV)[16][64] = reinterpret_cast<float (*)[16][64]>(sBuf + 256);   // [wave][term][record]: 16 KB
  const int tx = tile % p.gx, ty = tile / p.gx;
  const int pix_x = tx * TILE + 8 * (q & 1) + (lane & 7);
  const int pix_y = ty * TILE + 8 * (q >> 1) + (lane >> 3);
  const size_t HW = (size_t)p.W * p.H;

  uint32_t last = 0;
  {
    float T = 1.f, gC0 = 0.f, gC1 = 0.f, gC2 = 0.f, gN0 = 0.f, gN1 = 0.f, gN2 = 0.f, gD = 0.f, coefT = 0.f;
    float rx = 0.f, ry = 0.f;
    if (MODE == MODE_SURFEL) {
      const float cxp = (p.prcp ? p.prcp[0] : 0.5f) * (float)p.W - 0.5f;
      const float cyp = (p.prcp ? p.prcp[1] : 0.5f) * (float)p.H - 0.5f;
      rx = ((float)pix_x - cxp) / p.fx;
      ry = ((float)pix_y - cyp) / p.fy;
    }
    if (pix_x < p.W && pix_y < p.H) {
      const size_t pix_id = (size_t)pix_y * p.W + pix_x;
      last = n_contrib[pix_id];
      const float T_final = final_T[pix_id];
      T = T_final;
      if (dL_dcolor) {
        gC0 = dL_dcolor[pix_id];
        gC1 = dL_dcolor[HW + pix_id];
        gC2 = dL_dcolor[2 * HW + pix_id];
      }
      float gA = dL_dalpha ? dL_dalpha[pix_id] : 0.f;
      const float gDo = dL_ddepth ? dL_ddepth[pix_id] : 0.f;
      if (MODE == MODE_SURFEL) {
        if (dL_dnormal) {
          gN0 = dL_dnormal[pix_id];
          gN1 = dL_dnormal[HW + pix_id];
          gN2 = dL_dnormal[2 * HW + pix_id];
        }
        const float A = 1.0f - T_final;
        if (A > DEPTH_ALPHA_EPS) {
          gD = gDo / A;
          gA -= gDo * out_depth[pix_id] / A;
        }
      } else {
        gD = gDo;
      }
      const float bgdot = (p.bg[0] * gC0 + p.bg[1] * gC1) + p.bg[2] * gC2;
      coefT = (gA - bgdot) * T_final;
    }
    sPix[lane][0] = make_float4(T, 0.f, __uint_as_float(last), coefT);
    sPix[lane][1] = make_float4(gC0, gC1, gC2, gD);
    sPix[lane][2] = make_float4(gN0, gN1, gN2, (float)pix_x);
    sPix[lane][3] = make_float4((float)pix_y, rx, ry, 0.f);
  }
  uint32_t m = last;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
  if (lng) __syncthreads();   // every wave wrote the whole quadrant's state (identical values) before any updates it
  int pos = (int)m;  // list entries [0, pos) can matter to this quadrant
  if (pos == 0) return;
  const uint2 range = ranges[tile];
  const uint32_t below = (1u << q) - 1u;
  int nq = 0;
#ifdef PINGS_BWD_STATS
  unsigned long long st_chunks = 0, st_dead = 0, st_any = 0, st_exec = 0, st_valid = 0, st_take = 0;
#endif

  while (true) {
    // ---- queue the next relevant entries (entries behind `pos` are done)
    while (nq < 64 && pos > 0) {
      const int e = pos - 1 - lane;
      uint32_t slot = 0;
      bool rel = false;
      if (e >= 0) {
        slot = point_list[range.x + e];
        rel = ((qmask[slot] >> q) & 1u) != 0u;
      }
      const unsigned long long bal = __ballot(rel);
      if (rel) {
        const int at = nq + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        sQe[at] = e;
        sQs[at] = slot;
      }
      nq += __popcll(bal);
      pos -= 64;
    }
    if (nq == 0) break;
    const int take = nq < 64 ? nq : 64;
    // records replicated over the lane groups of scan_pixels: group size 16 / 32 / 64 by the chunk's record count
    const int gl = take <= 16 ? (lane & 15) : (take <= 32 ? (lane & 31) : lane);
    const bool act = gl < take;
    const int e = act ? sQe[gl] : 0x7FFFFFFF;        // an idle lane is never `valid`
    const uint32_t slot = act ? sQs[gl] : 0u;
    const int rest = nq - take;                        // < 64: shift the remainder to the queue's front
    const int me = lane < rest ? sQe[take + lane] : 0;
    const uint32_t ms = lane < rest ? sQs[take + lane] : 0u;
    if (lane < rest) { sQe[lane] = me; sQs[lane] = ms; }
    nq = rest;
    const int min_e = __shfl(e, take - 1, 64);         // frontmost record of the chunk

    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a, c = a, nn = a;
    uint32_t row = 0;
    if (act) {
      const uint32_t g = gval[slot];
      a = rec[4 * (size_t)g + 0];
      b = rec[4 * (size_t)g + 1];
      c = rec[4 * (size_t)g + 2];
      if (MODE == MODE_SURFEL) nn = rec[4 * (size_t)g + 3];
      row = cidx[slot] + (uint32_t)__builtin_popcount((unsigned)qmask[slot] & below);
    }
    float v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = 0.f;

#ifdef PINGS_BWD_STATS
    ++st_chunks; st_take += (unsigned)take;
#endif
    // Chunks that hold at most 16 / 32 records (short lists: a quadrant of a mapping view sees ~20 relevant records)
    // put four / two pixels on the wave at once: lane l works on record l % G for pixel pp0 + l / G.  Measured before
    // this split on the bench's mapping view: 21 records per chunk, 6.9 valid lanes of 64 per pixel iteration.
    if (lng) {
      if (take <= 16) scan_pixels<MODE, 16, 16>(sPix, lane, 16 * wv, e, min_e, a, b, c, nn, v STATS_ARGS);
      else if (take <= 32) scan_pixels<MODE, 32, 16>(sPix, lane, 16 * wv, e, min_e, a, b, c, nn, v STATS_ARGS);
      else scan_pixels<MODE, 64, 16>(sPix, lane, 16 * wv, e, min_e, a, b, c, nn, v STATS_ARGS);
    } else {
      if (take <= 16) scan_pixels<MODE, 16, 64>(sPix, lane, 0, e, min_e, a, b, c, nn, v STATS_ARGS);
      else if (take <= 32) scan_pixels<MODE, 32, 64>(sPix, lane, 0, e, min_e, a, b, c, nn, v STATS_ARGS);
      else scan_pixels<MODE, 64, 64>(sPix, lane, 0, e, min_e, a, b, c, nn, v STATS_ARGS);
    }
    float4* dst = reinterpret_cast<float4*>(rows) + (size_t)row * 4;
    if (!lng) {
      if (act && gl == lane) {                         // every group holds the same sums: the first one stores
        dst[0] = make_float4(v[0], v[1], v[2], v[3]);
        dst[1] = make_float4(v[4], v[5], v[6], v[7]);
        dst[2] = make_float4(v[8], v[9], v[10], v[11]);
        dst[3] = make_float4(v[12], v[13], v[14], v[15]);
      }
    } else {
      // the four waves' sums over their 16 pixels each meet in LDS; wave w adds and stores quarter w of the row
      if (gl == lane) {
#pragma unroll
        for (int k = 0; k < 16; ++k) sV[wv][k][lane] = v[k];
      }
      __syncthreads();
      if (act && gl == lane) {
        float o4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = 4 * wv + u;
          o4[u] = ((sV[0][k][lane] + sV[1][k][lane]) + sV[2][k][lane]) + sV[3][k][lane];
        }
        dst[wv] = make_float4(o4[0], o4[1], o4[2], o4[3]);
      }
      __syncthreads();                                 // the next chunk overwrites sV
    }
  }
#ifdef PINGS_BWD_STATS
  if (lane == 0) {
    atomicAdd(&g_bwd_stats[0], st_chunks); atomicAdd(&g_bwd_stats[1], st_dead); atomicAdd(&g_bwd_stats[2], st_any);
    atomicAdd(&g_bwd_stats[3], st_exec); atomicAdd(&g_bwd_stats[4], st_valid); atomicAdd(&g_bwd_stats[5], st_take);
  }
#endif
}

// ---------------------------------------------------------------- balanced per-Gaussian row sums
// LiveOp, RowRanges: raster_common.hpp; pair_off and pair_owner: raster_scan_chunks

// one 16-lane group per (Gaussian, chunk) pair; lane = column of the 16-float row.  The number of pairs lives on the
// device (pair_off[P]): a bounded grid (PINGS_ROWSUM_WGS workgroups) strides over them, instead of a grid for the
// host's upper bound np_max whose workgroups mostly read the count and leave.
__global__ __launch_bounds__(256) void row_chunk_sum_kernel(RowRanges rr, const uint32_t* __restrict__ pair_off,
                                                             const uint32_t* __restrict__ pair_owner,
                                                             const float* __restrict__ rows,
                                                             float* __restrict__ partials) {
  const int c = threadIdx.x & 15;
  const uint32_t npairs = pair_off[rr.P];
  const uint32_t stride = gridDim.x * (256u / 16u);
  for (uint32_t q = blockIdx.x * (256u / 16u) + (threadIdx.x >> 4); q < npairs; q += stride) {
    const uint32_t r = pair_owner[q];
    const uint32_t j = q - pair_off[r];
    const uint32_t row_end = rr.row_end(r);
    uint32_t row = rr.row_begin(r) + j * (uint32_t)CH;
    const uint32_t stop = min(row + (uint32_t)CH, row_end);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (; row + 4 <= stop; row += 4) {
      a0 += rows[(size_t)row * 16 + c];
      a1 += rows[(size_t)(row + 1) * 16 + c];
      a2 += rows[(size_t)(row + 2) * 16 + c];
      a3 += rows[(size_t)(row + 3) * 16 + c];
    }
    for (; row < stop; ++row) a0 += rows[(size_t)row * 16 + c];
    partials[(size_t)q * 16 + c] = (a0 + a1) + (a2 + a3);
  }
}

// ---------------------------------------------------------------- per-Gaussian chain
// The six gradient arrays start at zero: all but a few per cent of the Gaussians own no live row (culled, or no tile
// kept behind the occlusion bound, or never blended), and gaussian_bwd_rank_kernel only visits the depth ranks that do.
// The zeros ride in the blend-backward launch when there is one (grad_fill_part, in front of blend_bwd_tile_kernel);
// a frame without instances has no blend launch and runs this kernel (as does PINGS_GRAD_FILL=l).
__global__ __launch_bounds__(256) void grad_zero_kernel(GradFill f) { grad_fill_part(f, blockIdx.x, gridDim.x); }

// G += the chunk partials [qa, qb) of one Gaussian, in ascending order; AHEAD rows are loaded before their adds (the
// adds keep their order, so the sums keep their bits)
template <int AHEAD>
__device__ inline void sum_partials(const float* __restrict__ partials, uint32_t qa, uint32_t qb, float (&G)[16]) {
  const float4* prow = reinterpret_cast<const float4*>(partials);
  uint32_t k = qa;
  if (AHEAD > 1) {
    for (; k + AHEAD <= qb; k += AHEAD) {
      float4 ld[AHEAD][4];
#pragma unroll
      for (int u = 0; u < AHEAD; ++u)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) ld[u][q4] = prow[(size_t)(k + u) * 4 + q4];
#pragma unroll
      for (int u = 0; u < AHEAD; ++u)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          G[q4 * 4 + 0] += ld[u][q4].x;
          G[q4 * 4 + 1] += ld[u][q4].y;
          G[q4 * 4 + 2] += ld[u][q4].z;
          G[q4 * 4 + 3] += ld[u][q4].w;
        }
    }
  }
  for (; k < qb; ++k) {
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const float4 r = prow[(size_t)k * 4 + q4];
      G[q4 * 4 + 0] += r.x;
      G[q4 * 4 + 1] += r.y;
      G[q4 * 4 + 2] += r.z;
      G[q4 * 4 + 3] += r.w;
    }
  }
}

// The gradient row of Gaussian g from its summed blend gradients G: the chain through projection, covariance and
// quaternion when the Gaussian has a live row (`live`), zeros otherwise; tau = its pose-tangent terms.
template <int MODE>
__device__ inline void gaussian_row(const BParams& p, int g, bool live, const float (&G)[16],
                                    const float* __restrict__ means3D, const float* __restrict__ scales,
                                    const float* __restrict__ rotations, float* __restrict__ dL_dmeans3D,
                                    float* __restrict__ dL_dmeans2D, float* __restrict__ dL_dcolors,
                                    float* __restrict__ dL_dopacities, float* __restrict__ dL_dscales,
                                    float* __restrict__ dL_drotations, float (&tau)[6]) {
  float gm[3] = {0.f, 0.f, 0.f}, gs[3] = {0.f, 0.f, 0.f}, gq4[4] = {0.f, 0.f, 0.f, 0.f};
  float g2d[2] = {0.f, 0.f};
  if (live) {
    const float* V = p.view;
    const float* Pm = p.proj_raw;
    const float x = means3D[3 * g], y = means3D[3 * g + 1], z = means3D[3 * g + 2];
    const float px = ((V[0] * x + V[4] * y) + V[8] * z) + V[12];
    const float py = ((V[1] * x + V[5] * y) + V[9] * z) + V[13];
    const float pz = ((V[2] * x + V[6] * y) + V[10] * z) + V[14];
    float gp[3] = {0.f, 0.f, 0.f};
    // ---- 2-D mean
    {
      const float hx = ((Pm[0] * px + Pm[4] * py) + Pm[8] * pz) + Pm[12];
      const float hy = ((Pm[1] * px + Pm[5] * py) + Pm[9] * pz) + Pm[13];
      const float hw = ((Pm[3] * px + Pm[7] * py) + Pm[11] * pz) + Pm[15];
      const float pw = 1.0f / (hw + 1e-7f);
      const float gndx = 0.5f * (float)p.W * G[G_MX];
      const float gndy = 0.5f * (float)p.H * G[G_MY];
      g2d[0] = gndx;
      g2d[1] = gndy;
      const float kx = hx * pw * pw, ky = hy * pw * pw;
#pragma unroll
      for (int i = 0; i < 3; ++i)
        gp[i] = gndx * (Pm[4 * i + 0] * pw - kx * Pm[4 * i + 3]) +
                gndy * (Pm[4 * i + 1] * pw - ky * Pm[4 * i + 3]);
    }
    // ---- covariance
    const float qr = rotations[4 * g], qx = rotations[4 * g + 1], qy = rotations[4 * g + 2],
                qz = rotations[4 * g + 3];
    float R[3][3];
    R[0][0] = 1.0f - 2.0f * (qy * qy + qz * qz); R[0][1] = 2.0f * (qx * qy - qr * qz); R[0][2] = 2.0f * (qx * qz + qr * qy);
    R[1][0] = 2.0f * (qx * qy + qr * qz); R[1][1] = 1.0f - 2.0f * (qx * qx + qz * qz); R[1][2] = 2.0f * (qy * qz - qr * qx);
    R[2][0] = 2.0f * (qx * qz - qr * qy); R[2][1] = 2.0f * (qy * qz + qr * qx); R[2][2] = 1.0f - 2.0f * (qx * qx + qy * qy);
    const float S[3] = {p.scale_mod * scales[3 * g], p.scale_mod * scales[3 * g + 1],
                        p.scale_mod * scales[3 * g + 2]};
    float RS[3][3], Mc[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) RS[i][k] = R[i][k] * S[k];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int k = 0; k < 3; ++k)
        Mc[a][k] = (V[a] * RS[0][k] + V[4 + a] * RS[1][k]) + V[8 + a] * RS[2][k];
    const float txz = px / pz, tyz = py / pz;
    const bool clx = (txz < -p.limx) || (txz > p.limx), cly = (tyz < -p.limy) || (tyz > p.limy);
    const float tx = fminf(p.limx, fmaxf(-p.limx, txz)) * pz;
    const float ty = fminf(p.limy, fmaxf(-p.limy, tyz)) * pz;
    const float iz = 1.0f / pz, iz2 = iz * iz;
    const float J00 = p.fx * iz, J02 = -(p.fx * tx) * iz2, J11 = p.fy * iz, J12 = -(p.fy * ty) * iz2;
    float T0[3], T1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      T0[k] = J00 * Mc[0][k] + J02 * Mc[2][k];
      T1[k] = J11 * Mc[1][k] + J12 * Mc[2][k];
    }
    const float ca = ((T0[0] * T0[0] + T0[1] * T0[1]) + T0[2] * T0[2]) + LOWPASS;
    const float cb = (T0[0] * T1[0] + T0[1] * T1[1]) + T0[2] * T1[2];
    const float cc = ((T1[0] * T1[0] + T1[1] * T1[1]) + T1[2] * T1[2]) + LOWPASS;
    // the blend pass accumulated dL/d(cov2D) directly: a = cov_xx, b = cov_xy (the single
    // off-diagonal parameter), c = cov_yy
    (void)ca; (void)cb; (void)cc;
    const float ga = G[G_CONX], gb = G[G_CONY], gc = G[G_CONZ];
    float gT0[3], gT1[3], gMc[3][3];
    float gJ00 = 0.f, gJ02 = 0.f, gJ11 = 0.f, gJ12 = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      gT0[k] = 2.0f * ga * T0[k] + gb * T1[k];
      gT1[k] = 2.0f * gc * T1[k] + gb * T0[k];
      gJ00 += gT0[k] * Mc[0][k];
      gJ02 += gT0[k] * Mc[2][k];
      gJ11 += gT1[k] * Mc[1][k];
      gJ12 += gT1[k] * Mc[2][k];
      gMc[0][k] = J00 * gT0[k];
      gMc[1][k] = J11 * gT1[k];
      gMc[2][k] = J02 * gT0[k] + J12 * gT1[k];
    }
    // J -> camera point
    gp[2] += -p.fx * iz2 * gJ00 - p.fy * iz2 * gJ11;
    gp[2] += 2.0f * p.fx * tx * iz2 * iz * gJ02 + 2.0f * p.fy * ty * iz2 * iz * gJ12;
    const float gtx = -p.fx * iz2 * gJ02, gty = -p.fy * iz2 * gJ12;
    if (clx) gp[2] += gtx * tx * iz; else gp[0] += gtx;
    if (cly) gp[2] += gty * ty * iz; else gp[1] += gty;
    // Mc = Wc RS
    float gRS[3][3], gWc[3][3];
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int k = 0; k < 3; ++k)
        gRS[b][k] = (V[4 * b + 0] * gMc[0][k] + V[4 * b + 1] * gMc[1][k]) + V[4 * b + 2] * gMc[2][k];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b)
        gWc[a][b] = (gMc[a][0] * RS[b][0] + gMc[a][1] * RS[b][1]) + gMc[a][2] * RS[b][2];
    float gR[3][3];
    float gS[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        gS[k] += gRS[i][k] * R[i][k];
        gR[i][k] = gRS[i][k] * S[k];
      }
    float gpz_direct = G[G_PZ];
    if (MODE == MODE_SURFEL) {
      // normal n = sgn * Wc R[:,2], q = n . p
      float nx = (V[0] * R[0][2] + V[4] * R[1][2]) + V[8] * R[2][2];
      float ny = (V[1] * R[0][2] + V[5] * R[1][2]) + V[9] * R[2][2];
      float nz = (V[2] * R[0][2] + V[6] * R[1][2]) + V[10] * R[2][2];
      const float q = (nx * px + ny * py) + nz * pz;
      float sgn = 1.0f;
      if (!p.front_only && q > 0.0f) sgn = -1.0f;
      nx *= sgn; ny *= sgn; nz *= sgn;
      const float gq = G[G_Q];
      const float gn[3] = {G[G_NX] + gq * px, G[G_NY] + gq * py, G[G_NZ] + gq * pz};
      gp[0] += gq * nx;
      gp[1] += gq * ny;
      gp[2] += gq * nz;
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        gR[b][2] += sgn * ((V[4 * b + 0] * gn[0] + V[4 * b + 1] * gn[1]) + V[4 * b + 2] * gn[2]);
#pragma unroll
        for (int a = 0; a < 3; ++a) gWc[a][b] += sgn * gn[a] * R[b][2];
      }
      // depth clamp window zlo = pz - rz, zhi = pz + rz, rz = 3 max(S0, S1)
      gpz_direct += G[G_ZLO] + G[G_ZHI];
      const float grz = 3.0f * (G[G_ZHI] - G[G_ZLO]);
      if (S[0] > S[1]) gS[0] += grz;
      else if (S[1] > S[0]) gS[1] += grz;
      else { gS[0] += 0.5f * grz; gS[1] += 0.5f * grz; }
    }
    gp[2] += gpz_direct;
    // quaternion
    gq4[0] = 2.0f * (-qz * gR[0][1] + qy * gR[0][2] + qz * gR[1][0] - qx * gR[1][2] - qy * gR[2][0] + qx * gR[2][1]);
    gq4[1] = 2.0f * (qy * gR[0][1] + qz * gR[0][2] + qy * gR[1][0] - 2.0f * qx * gR[1][1] - qr * gR[1][2] + qz * gR[2][0] + qr * gR[2][1] - 2.0f * qx * gR[2][2]);
    gq4[2] = 2.0f * (-2.0f * qy * gR[0][0] + qx * gR[0][1] + qr * gR[0][2] + qx * gR[1][0] + qz * gR[1][2] - qr * gR[2][0] + qz * gR[2][1] - 2.0f * qy * gR[2][2]);
    gq4[3] = 2.0f * (-2.0f * qz * gR[0][0] - qr * gR[0][1] + qx * gR[0][2] + qr * gR[1][0] - 2.0f * qz * gR[1][1] + qy * gR[1][2] + qx * gR[2][0] + qy * gR[2][1]);
#pragma unroll
    for (int k = 0; k < 3; ++k) gs[k] = p.scale_mod * gS[k];
    // world mean: p = Wc m + t
#pragma unroll
    for (int b = 0; b < 3; ++b)
      gm[b] = (V[4 * b + 0] * gp[0] + V[4 * b + 1] * gp[1]) + V[4 * b + 2] * gp[2];
    // pose tangent at tau = 0: d rho = gp ; d theta = p x gp + sum_b Wc[:,b] x gWc[:,b]
    tau[0] = gp[0]; tau[1] = gp[1]; tau[2] = gp[2];
    float th0 = py * gp[2] - pz * gp[1];
    float th1 = pz * gp[0] - px * gp[2];
    float th2 = px * gp[1] - py * gp[0];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const float w0 = V[4 * b + 0], w1 = V[4 * b + 1], w2 = V[4 * b + 2];
      th0 += w1 * gWc[2][b] - w2 * gWc[1][b];
      th1 += w2 * gWc[0][b] - w0 * gWc[2][b];
      th2 += w0 * gWc[1][b] - w1 * gWc[0][b];
    }
    tau[3] = th0; tau[4] = th1; tau[5] = th2;
  }
  dL_dmeans3D[3 * g] = gm[0]; dL_dmeans3D[3 * g + 1] = gm[1]; dL_dmeans3D[3 * g + 2] = gm[2];
  dL_dmeans2D[3 * g] = g2d[0]; dL_dmeans2D[3 * g + 1] = g2d[1]; dL_dmeans2D[3 * g + 2] = 0.f;
  dL_dcolors[3 * g] = G[G_R]; dL_dcolors[3 * g + 1] = G[G_G]; dL_dcolors[3 * g + 2] = G[G_B];
  dL_dopacities[g] = G[G_OPAC];
  dL_dscales[3 * g] = gs[0]; dL_dscales[3 * g + 1] = gs[1]; dL_dscales[3 * g + 2] = gs[2];
  dL_drotations[4 * g] = gq4[0]; dL_drotations[4 * g + 1] = gq4[1];
  dL_drotations[4 * g + 2] = gq4[2]; dL_drotations[4 * g + 3] = gq4[3];
}

// block reduction of the pose-tangent terms (fixed order -> deterministic)
__device__ inline void store_tau_partial(const float (&tau)[6], float* __restrict__ tau_partials) {
  __shared__ float sTau[256 / 64][6];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const float s = wave_reduce_sum_dpp(tau[k]);
    if (lane == 63) sTau[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int k = threadIdx.x;
    tau_partials[(size_t)blockIdx.x * 6 + k] = ((sTau[0][k] + sTau[1][k]) + sTau[2][k]) + sTau[3][k];
  }
}

// The per-Gaussian chain, two launch plans (pings_raster_backward picks by the blend plan):
//
// BY OWNER OF A CHUNK PAIR, behind the zero fill (grad_fill_part) — for frames in which few Gaussians own a gradient row
// (footprint class 2: the occlusion bound leaves most survivors without a tile; headline: 951 of 332,253 survivors own one, in
// 8,925 (Gaussian, chunk) pairs).  One thread per pair q of the chunk scan; the thread of a Gaussian's FIRST pair
// (pair_off[owner] == q) runs its chain, the others leave.  pair_owner and pair_off are indexed by pair and by depth
// rank and read coalesced; neither the rectangle nor the rank of a Gaussian is looked up, and a depth rank without a
// live row costs nothing.  A Gaussian with a loop over n chunk partials is followed by n - 1 idle threads, so the long
// loops of the nearest Gaussians (up to num_tiles * 4 / CH partials each, neighbours in depth rank) spread over the
// waves by themselves: a wave never sums more than 64 + the longest loop's partials.  The grid is sized for the host's
// bound np_max; the number of pairs is a device word and the workgroups behind it leave after one scalar load.  Rows
// are stored for the Gaussians with a live row only, as scattered single floats.
// The pose-tangent partial of a workgroup sums the owners among ITS 256 pairs: the grouping depends on the live rows
// alone, not on how many Gaussians survived culling or what rank they got, so frames that blend the same instances
// (the tile-rectangle rules, the two depth sorts) sum the pose gradient in the same order.
//
// G, the sum of an owner's chunk partials [pair_off[r], pair_off[r + 1]), is formed BY 16-LANE GROUPS (GROUP_SUM): the
// owners among the workgroup's 256 pairs are dealt round-robin to its sixteen groups, lane c of a group adds component
// c of the partials in ascending order, GROUP_AHEAD rows in flight, each row one coalesced 64-byte request; the sums
// go to LDS at the owner's slot and the owner thread takes them from there.  A lane alone (sum_partials, the other
// instance: PINGS_CHAIN_SUM=l) fetches a row as four 16-byte loads of its own and keeps PART_AHEAD rows in flight: the
// 123 partials of the headline's nearest Gaussians were sixteen dependent round trips of one lane while its wave and
// most of the GPU waited.  Either way a component is 0 + p[qa] + p[qa + 1] + ... in this order: the same bits.  A loop
// that runs past the workgroup's last pair is summed whole by its group; nothing is taken from another workgroup.
constexpr int PART_AHEAD = 8;
constexpr int GROUP_AHEAD = 16;
constexpr int G_PITCH = 17;   // floats per owner slot of sG: the owners' 16 reads fall into different banks
// q: the thread's pair; owner: it is the first pair of a Gaussian, whose partials end at qb
__device__ inline void sum_partials_by_group(const float* __restrict__ partials, uint32_t q, bool owner, uint32_t qb,
                                             float (&G)[16]) {
  __shared__ float sG[256 * G_PITCH];
  __shared__ uint32_t sSlot[256], sEnd[256];   // the workgroup's owners, compacted: thread, end of its partials
  __shared__ uint32_t sCount[256 / 64];
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  const unsigned long long owners = __ballot(owner);
  if (lane == 0) sCount[wave] = (uint32_t)__popcll(owners);
  __syncthreads();
  uint32_t at = (uint32_t)__popcll(owners & ((1ull << lane) - 1ull)), n_owners = 0;
#pragma unroll
  for (uint32_t w = 0; w < 256 / 64; ++w) {
    if (w < wave) at += sCount[w];
    n_owners += sCount[w];
  }
  if (owner) {
    sSlot[at] = t;
    sEnd[at] = qb;
  }
  __syncthreads();
  const uint32_t c = t & 15u, q0 = q - t;
  for (uint32_t o = t >> 4; o < n_owners; o += 256 / 16) {
    const uint32_t slot = sSlot[o], end = sEnd[o];
    float acc = 0.f;
    for (uint32_t k = q0 + slot; k < end; k += GROUP_AHEAD) {
      float ld[GROUP_AHEAD];
#pragma unroll
      for (int u = 0; u < GROUP_AHEAD; ++u)
        if (k + u < end) ld[u] = partials[(size_t)(k + u) * 16 + c];
#pragma unroll
      for (int u = 0; u < GROUP_AHEAD; ++u)
        if (k + u < end) acc += ld[u];
    }
    sG[slot * G_PITCH + c] = acc;
  }
  __syncthreads();
  if (owner) {
#pragma unroll
    for (int k = 0; k < 16; ++k) G[k] = sG[t * G_PITCH + k];
  }
}

template <int MODE, bool GROUP_SUM>
__global__ __launch_bounds__(256, 2) void gaussian_bwd_rank_kernel(
    BParams p, const float* __restrict__ means3D, const float* __restrict__ scales,
    const float* __restrict__ rotations, const uint32_t* __restrict__ gidx_sorted,
    const uint32_t* __restrict__ pair_off, const uint32_t* __restrict__ pair_owner,
    const float* __restrict__ partials, float* __restrict__ dL_dmeans3D, float* __restrict__ dL_dmeans2D, float* __restrict__ dL_dcolors,
    float* __restrict__ dL_dopacities, float* __restrict__ dL_dscales,
    float* __restrict__ dL_drotations, float* __restrict__ tau_partials) {
  const uint32_t npairs = pair_off[p.P];
  if (blockIdx.x * 256u >= npairs) return;   // tau_reduce_kernel sums the workgroups in front of this one
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  float tau[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const uint32_t r = q < npairs ? pair_owner[q] : 0u;
  const bool owner = q < npairs && pair_off[r] == q;
  float G[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) G[k] = 0.f;
  const uint32_t qb = owner ? pair_off[r + 1] : 0u;
  if (GROUP_SUM) sum_partials_by_group(partials, q, owner, qb, G);
  if (owner) {
    if (!GROUP_SUM) sum_partials<PART_AHEAD>(partials, q, qb, G);
    gaussian_row<MODE>(p, (int)gidx_sorted[r], true, G, means3D, scales, rotations, dL_dmeans3D, dL_dmeans2D,
                       dL_dcolors, dL_dopacities, dL_dscales, dL_drotations, tau);
  }
  store_tau_partial(tau, tau_partials);
}

// BY GAUSSIAN INDEX — for frames in which most survivors own a row (small footprints, nothing saturates: C3 has
// 814,949 survivors of 1M).  Parameters are read and all gradient rows written coalesced, zeros included; only the
// words that locate the Gaussian's chunk partials go through its depth rank.  (By rank such a frame scatters seventeen
// floats per Gaussian over six arrays: C3's chain 0.070 -> 0.165 ms, profiles/r15.)
template <int MODE>
__global__ __launch_bounds__(256, 4) void gaussian_bwd_index_kernel(
    BParams p, const float* __restrict__ means3D, const float* __restrict__ scales,
    const float* __restrict__ rotations, const uint4* __restrict__ rect, const uint32_t* __restrict__ rank_of,
    const uint32_t* __restrict__ tiles_sorted, const uint32_t* __restrict__ pair_off,
    const float* __restrict__ partials, float* __restrict__ dL_dmeans3D, float* __restrict__ dL_dmeans2D, float* __restrict__ dL_dcolors,
    float* __restrict__ dL_dopacities, float* __restrict__ dL_dscales,
    float* __restrict__ dL_drotations, float* __restrict__ tau_partials) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  float tau[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (g < p.P) {
    uint32_t n_tiles = 0u, qa = 0u, qb = 0u;
    if (rect[g].w != 0u) {  // survived culling: has a depth rank
      const uint32_t rank = rank_of[g];
      n_tiles = tiles_sorted[rank];
      qa = pair_off[rank];
      qb = pair_off[rank + 1];
    }
    float G[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) G[k] = 0.f;
    sum_partials<1>(partials, qa, qb, G);
    gaussian_row<MODE>(p, g, n_tiles > 0 && qb > qa, G, means3D, scales, rotations, dL_dmeans3D, dL_dmeans2D,
                       dL_dcolors, dL_dopacities, dL_dscales, dL_drotations, tau);
  }
  store_tau_partial(tau, tau_partials);
}

// sums the per-workgroup partials in fp64: of the workgroups that hold a pair (gaussian_bwd_rank_kernel; npairs != nullptr)
// or of all `nblocks_all` (gaussian_bwd_index_kernel)
__global__ __launch_bounds__(256) void tau_reduce_kernel(const float* __restrict__ partials,
                                                          const uint32_t* __restrict__ npairs, int nblocks_all,
                                                          float* __restrict__ dL_dtau) {
  const int nblocks = npairs ? (int)((*npairs + 255u) / 256u) : nblocks_all;
  __shared__ double sRed[4][6];
  double s[6] = {0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < nblocks; i += 256) {
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] += (double)partials[(size_t)i * 6 + k];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_down(s[k], off, 64);
    if ((threadIdx.x & 63) == 0) sRed[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < 6)
    dL_dtau[threadIdx.x] = (float)(((sRed[0][threadIdx.x] + sRed[1][threadIdx.x]) + sRed[2][threadIdx.x]) + sRed[3][threadIdx.x]);
}

}  // namespace raster
}  // namespace pings

using namespace pings::raster;

PINGS_API int pings_raster_backward(const pings_raster_settings* s, int P, int64_t I,
                                    const float* means3D, const float* colors,
                                    const float* opacities, const float* scales,
                                    const float* rotations, const void* geom_blob,
                                    const void* binning_blob, const void* image_blob,
                                    const float* out_color, const float* out_normal,
                                    const float* out_depth, const float* out_alpha,
                                    const float* dL_dcolor, const float* dL_dnormal,
                                    const float* dL_ddepth, const float* dL_dalpha,
                                    void* bwd_blob, float* dL_dmeans3D, float* dL_dmeans2D,
                                    float* dL_dcolors, float* dL_dopacities, float* dL_dscales,
                                    float* dL_drotations, float* dL_dtau, int footprint_class,
                                    void* stream) {
  BParams bp;
  if (int e = fill_camera(s, P, bp)) return e;
  PINGS_ARG_CHECK(dL_dtau != nullptr, "null dL_dtau");
  hipStream_t st = pings::as_stream(stream);
  if (P == 0) {   // otherwise tau_reduce_kernel writes all six
    PINGS_HIP_CHECK(hipMemsetAsync(dL_dtau, 0, 6 * sizeof(float), st));
    return PINGS_OK;
  }
  PINGS_ARG_CHECK(P > 0 && means3D && colors && opacities && scales && rotations && geom_blob &&
                      binning_blob && image_blob && out_depth && bwd_blob && dL_dmeans3D &&
                      dL_dmeans2D && dL_dcolors && dL_dopacities && dL_dscales && dL_drotations,
                  "null pointer");
  PINGS_ARG_CHECK(I >= 0 && I < (int64_t)0x7FFFFFF0, "instance count out of range");
  (void)out_color; (void)out_normal; (void)out_alpha;
  const RasterKnobs knobs = read_knobs();
  const int num_tiles = bp.gx * bp.gy;
  const BlendPlan plan = blend_plan(knobs, footprint_class, I, num_tiles);
  GeomState gs = carve_geom(const_cast<void*>(geom_blob), P, num_tiles);
  BinState bs = carve_binning(const_cast<void*>(binning_blob), I, num_tiles, knobs.blend_seg);
  ImageState im = carve_image(const_cast<void*>(image_blob), bp.W, bp.H);
  BwdState bw = carve_bwd(bwd_blob, P, I);
  const dim3 block(256);
  const RowRanges rr{P, gs.offsets_sorted, gs.tiles_sorted, bw.cidx};

  // The prelude of the blend backward: the tile order (tiles by descending largest per-pixel contributor count, the
  // records a tile walks), the live rows' scan and the chunk scan with its owners.  The tile order shares nothing with
  // the scans and is one workgroup: it rides in the reduce launch of the live scan.  (On a side stream next to the row
  // scans — two chains of small launches — the step came out 0.008 - 0.025 ms SLOWER on Metric-1 / C2: the fork and
  // join cost more than the 16 us they could hide.)
  TileOrderJob order_job;
  if (I > 0) {
    pings::prof::Scope ps("tile_order", st);
    const bool fwd_left_it = plan.fwd == BlendPlan::FWD_TILE;   // blend_fwd_tile_kernel's epilogue: the same numbers
    if (!fwd_left_it) {
      hipLaunchKernelGGL(tile_max_contrib_kernel, dim3(num_tiles), dim3(64), 0, st, bp.W, bp.H, bp.gx, im.n_contrib,
                         bs.tile_work);
      PINGS_LAUNCH_CHECK();
    }
    order_job.work = fwd_left_it ? bs.tile_maxc : bs.tile_work;
    order_job.num_tiles = num_tiles;
    order_job.order = bs.tile_order + num_tiles;
    order_job.n_long = bs.tile_order + 2 * (size_t)num_tiles;
    order_job.long_thr = plan.long_thr;
    order_job.long_max = LONG_TILES_MAX;
  }
  {
    pings::prof::Scope ps("live_scan", st);
    if (I > 0 && plan.bwd_scan) {
      // one row per (instance, quadrant it blended in): inst_qmask has I+1 entries, the last one zero
      if (int e = raster_scan_pop(bs.inst_qmask, I + 1, bw.cidx, bw.temp, bw.temp_bytes, knobs.library_scan, order_job, st))
        return e;
    } else if (I > 0) {
      // inst_w has I+1 entries, the last one zero: cidx[I] = number of live instances
      if (int e = raster_scan_live(bs.inst_w, I + 1, bw.cidx, bw.temp, bw.temp_bytes, knobs.library_scan, order_job, st))
        return e;
    } else {
      PINGS_HIP_CHECK(hipMemsetAsync(bw.cidx, 0, 2 * sizeof(uint32_t), st));
    }
    if (int e = raster_scan_chunks(rr, bw.pair_off, bw.pair_owner, bw.temp, bw.temp_bytes, knobs.library_scan, st))
      return e;
  }
  // The pixel-per-lane backward is followed by the chain over the owners of the chunk pairs, which stores the rows of
  // the Gaussians with a live row only: the rest is zeros (68 P bytes), written by trailing workgroups of the blend
  // launch or, without a blend launch, by grad_zero_kernel.
  const bool by_rank = !plan.bwd_scan;
  GradFill fill;
  {
    float* const grads[6] = {dL_dmeans3D, dL_dmeans2D, dL_dcolors, dL_dopacities, dL_dscales, dL_drotations};
    const size_t per[6] = {3, 3, 3, 1, 3, 4};
    for (int a = 0; a < 6; ++a) { fill.ptr[a] = grads[a]; fill.count[a] = per[a] * (size_t)P; }
  }
  const bool fill_in_blend = by_rank && I > 0 && knobs.grad_fill_wgs > 0;
  if (I > 0) {
    pings::prof::Scope ps("blend_bwd", st);
    const uint32_t* order = bs.tile_order + num_tiles;
    with_mode(s->mode, [&](auto m) {
      constexpr int M = m();
      if (plan.bwd_scan) {
        // one workgroup per ordinary tile, four per long tile (their number lives on the device: the grid is sized
        // for the cap, workgroups past the last tile leave at once)
        const uint32_t* n_long = bs.tile_order + 2 * (size_t)num_tiles;
        const unsigned grid_s = (unsigned)(num_tiles + 3 * std::min<long long>(num_tiles, LONG_TILES_MAX));
        hipLaunchKernelGGL((blend_bwd_scan_kernel<M>), dim3(grid_s), dim3(256), 0, st, bp, bs.ranges,
                           bs.point_list, gs.rec, bs.gval, im.final_T, im.n_contrib, out_depth, dL_dcolor, dL_dnormal,
                           dL_ddepth, dL_dalpha, bs.inst_qmask, bw.cidx, bw.rows, order, n_long);
      } else {
        const unsigned fill_wgs = fill_in_blend ? knobs.grad_fill_wgs : 0u;
        hipLaunchKernelGGL((blend_bwd_tile_kernel<M>), dim3((unsigned)num_tiles + fill_wgs), dim3(64), 0, st, bp,
                           bs.ranges, bs.point_list, gs.rec, bs.gval, im.final_T, im.n_contrib, out_depth, dL_dcolor,
                           dL_dnormal, dL_ddepth, dL_dalpha, bs.inst_w, bw.cidx, bw.rows, order, (uint32_t)num_tiles,
                           fill, (int)plan.interior_bwd);
      }
    });
    PINGS_LAUNCH_CHECK();
  }
  {
    pings::prof::Scope ps("row_chunk_sum", st);
    hipLaunchKernelGGL(row_chunk_sum_kernel, dim3(knobs.rowsum_wgs), block, 0, st, rr, bw.pair_off, bw.pair_owner,
                       bw.rows, bw.partials);
    PINGS_LAUNCH_CHECK();
  }
  const int nblocks = pings::ceil_div(P, 256);
  {
    pings::prof::Scope ps_g("gaussian_bwd", st);
    // The chain's launch plan follows the blend plan.  The pixel-per-lane backward is the plan of footprint class 2:
    // large footprints, so the occlusion bound leaves few Gaussians a tile and fewer a live row — zeros are streamed
    // and the chain runs over the owners of the chunk pairs.  The scan backward is the plan of small footprints, where most
    // survivors own a row: the chain runs in index order and writes every row itself.
    if (by_rank && !fill_in_blend) {
      // 17 P floats as 16-byte stores, eight or so to a thread
      const unsigned fill_grid = (unsigned)std::min<size_t>(2048, pings::ceil_div<size_t>((size_t)P * 17, 4 * 256));
      hipLaunchKernelGGL(grad_zero_kernel, dim3(fill_grid), block, 0, st, fill);
      PINGS_LAUNCH_CHECK();
    }
    with_mode(s->mode, [&](auto m) {
      if (by_rank) {
        const auto chain = knobs.chain_sum_lanes ? gaussian_bwd_rank_kernel<m(), false> : gaussian_bwd_rank_kernel<m(), true>;
        hipLaunchKernelGGL(chain, dim3((unsigned)pings::ceil_div<size_t>(bw.np_max, 256)), block,
                           0, st, bp, means3D, scales, rotations, gs.gidx_sorted, bw.pair_off, bw.pair_owner,
                           bw.partials, dL_dmeans3D, dL_dmeans2D, dL_dcolors, dL_dopacities, dL_dscales, dL_drotations,
                           bw.tau_partials);
      } else
        hipLaunchKernelGGL(gaussian_bwd_index_kernel<m()>, dim3(nblocks), block, 0, st, bp, means3D, scales, rotations,
                           gs.rect, gs.rank_of, gs.tiles_sorted, bw.pair_off, bw.partials, dL_dmeans3D, dL_dmeans2D,
                           dL_dcolors, dL_dopacities, dL_dscales, dL_drotations, bw.tau_partials);
    });
    PINGS_LAUNCH_CHECK();
    hipLaunchKernelGGL(tau_reduce_kernel, dim3(1), block, 0, st, bw.tau_partials,
                       by_rank ? (const uint32_t*)(bw.pair_off + P) : (const uint32_t*)nullptr, nblocks, dL_dtau);
    PINGS_LAUNCH_CHECK();
  }
  return PINGS_OK;
}

#ifdef PINGS_BWD_STATS
PINGS_API int pings_debug_bwd_stats(unsigned long long* out8, int reset) {
  PINGS_HIP_CHECK(hipDeviceSynchronize());
  PINGS_HIP_CHECK(hipMemcpyFromSymbol(out8, HIP_SYMBOL(pings::raster::g_bwd_stats), 64));
  if (reset) {
    unsigned long long z[8] = {0};
    PINGS_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(pings::raster::g_bwd_stats), z, 64));
  }
  return PINGS_OK;
}
#endif
