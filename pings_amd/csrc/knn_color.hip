// Fused colour query with its Jacobian for gfx950: the colour head of Tracker.query_source_points
// (utils/tracker.py:328-336) on neighbour lists that a search has already produced.
//
// The tracker's photometric term asks for colour[B,C] = IDW of sigmoid(colour decoder) and for d colour_c / d query,
// which the reference gets from one autograd pass per channel through query_feature (model/neural_gaussians.py:593-710)
// and Decoder.regress_color (model/decoder.py:133).  Here one wave64 handles a query, shaped like sdf_forward_kernel
// (knn_sdf.hip): lane h owns hidden unit h of the one-hidden-level decoder, its W1 row and its C entries of W2 stay in
// registers across the queries of the wave, the k colour-feature rows are gathered into LDS sixteen bytes a lane, and
// every wave-wide sum of a neighbour (C outputs, and with the Jacobian 3 C direction-input gradients) goes through the
// transposed eight-value reduction of knn_common.hpp.  The neighbour rows `idx` are those pings_sdf_forward(idx_out) or
// pings_knn_search emit for the same queries, so the search is not repeated; -1 (and any row outside the tables) is
// "no neighbour": zero features, zero vector, zero weight.
//
// Jacobian, per-neighbour mode (both parts, as autograd gives them; SURVEY a13 for the SDF):
//   sum_j w_j s'(raw_jc) R_j (sum_h W2[c,h] [pre_jh > 0] W1[h, Fc..Fc+2])  +  (1/U) sum_j (col_jc - colour_c) du_j/dx
// with u_j = 1 / (|x - p_j|^2 + 1e-15), U = sum u, du_j/dx = -2 u_j^2 (x - p_j); n_j = R_j^T (x - p_j) after a pose
// graph optimisation, so the gradient w.r.t. x of a gradient g_n w.r.t. n_j is R_j g_n (rot_active).
// weighted_first: one decoder evaluation of in = sum_j w_j [f_j, n_j]; the chain rule through `in` gives the same two
// parts with g_in = s'(raw_c) W1^T (W2[c] . [pre > 0]).
// A query without a neighbour: colour 0 (per-neighbour) or sigmoid(mlp(0)) (weighted_first), Jacobian 0 (:650-662).
#include "knn_host.hpp"

namespace {
using namespace pings_knn;

constexpr int MAX_CH = 3;

__device__ inline float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

template <int IN_PAD, bool JAC>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, 2) void color_forward_kernel(
    pings_color_decoder dec, const float* __restrict__ features, long long rows, const float* __restrict__ points,
    const float* __restrict__ orientations, int after_pgo, const float* __restrict__ queries, long long B,
    const long long* __restrict__ idx, int nnk, float* __restrict__ color_out, float* __restrict__ jac_out) {
  __shared__ long long sIdx[WAVES_PER_BLOCK][MAX_NNK];
  __shared__ float sW[WAVES_PER_BLOCK][MAX_NNK];
  __shared__ float sDu[WAVES_PER_BLOCK][MAX_NNK];                    // -2 u_j^2 / U: d w / dx is sDu (x - p_j) terms
  __shared__ __attribute__((aligned(16))) float sIn[WAVES_PER_BLOCK][MAX_NNK][IN_PAD];
  __shared__ __attribute__((aligned(16))) float sAvg[WAVES_PER_BLOCK][IN_PAD];   // weighted_first: sum_j w_j in_j
  __shared__ float sVec[WAVES_PER_BLOCK][MAX_NNK][4];                // x - p_j
  __shared__ float sR[WAVES_PER_BLOCK][MAX_NNK + 1][MAX_CH][4];      // per (neighbour, channel): raw | t, g_n[3]
  __shared__ float sS[WAVES_PER_BLOCK][MAX_NNK][4];                  // per (neighbour, channel): sigmoid(raw)

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int F = dec.feat_dim, IN = F + 3, Hd = dec.hidden, C = dec.channels;
  float w1[IN_PAD];
  float b1 = 0.f, w2[MAX_CH] = {0.f, 0.f, 0.f}, b2[MAX_CH] = {0.f, 0.f, 0.f};
  float w1n0, w1n1, w1n2;
  load_w1_rows<IN_PAD>(dec.W1, IN, Hd, &sIn[0][0][0], w1, w1n0, w1n1, w1n2);
  if (lane < Hd) b1 = dec.b1[lane];
#pragma unroll
  for (int c = 0; c < MAX_CH; ++c)
    if (c < C) {
      if (lane < Hd) w2[c] = dec.W2[c * Hd + lane];
      b2[c] = dec.b2[c];
    }

  const bool f_vec = (F & 3) == 0 && ((reinterpret_cast<uintptr_t>(features) & 15u) == 0);
  const int F4 = F >> 2;
  const int slot = reduce8_slot(lane);
  const long long nwaves = (long long)gridDim.x * WAVES_PER_BLOCK;
  for (long long q = (long long)blockIdx.x * WAVES_PER_BLOCK + wave; q < B; q += nwaves) {
    const float qx = queries[3 * q], qy = queries[3 * q + 1], qz = queries[3 * q + 2];
    // ---- neighbours (lane i < nn_k owns neighbour i): vector, squared distance, inverse-distance weight
    long long my_idx = -1;
    if (lane < nnk) {
      my_idx = idx[q * nnk + lane];
      if (my_idx >= rows) my_idx = -1;
      sIdx[wave][lane] = my_idx;
    }
    float vx = 0.f, vy = 0.f, vz = 0.f, u = 0.f;
    if (my_idx >= 0) {
      vx = qx - points[3 * my_idx];
      vy = qy - points[3 * my_idx + 1];
      vz = qz - points[3 * my_idx + 2];
      u = 1.0f / (((vx * vx + vy * vy) + vz * vz) + 1e-15f);
    }
    const int count = __popcll(__ballot(my_idx >= 0));
    const float U = wave_sum_all(u);
    const float wgt = (my_idx >= 0) ? u / U : 0.f;
    if (lane < nnk) {
      sW[wave][lane] = wgt;
      sDu[wave][lane] = (my_idx >= 0) ? (-2.f * u * u) / U : 0.f;
      sVec[wave][lane][0] = vx; sVec[wave][lane][1] = vy; sVec[wave][lane][2] = vz;
      float nx = vx, ny = vy, nz = vz;
      if (after_pgo && my_idx >= 0) rot_passive(orientations + 4 * my_idx, vx, vy, vz, nx, ny, nz);
      sIn[wave][lane][F] = nx; sIn[wave][lane][F + 1] = ny; sIn[wave][lane][F + 2] = nz;
      for (int i = IN; i < IN_PAD; ++i) sIn[wave][lane][i] = 0.f;
    }
    __builtin_amdgcn_wave_barrier();
    // ---- feature rows -> LDS (zeros for missing neighbours)
    if (f_vec) {
      for (int e = lane; e < nnk * F4; e += 64) {
        const int mm = e / F4, c4 = e - mm * F4;
        const long long id = sIdx[wave][mm];
        const float4 v = id >= 0 ? reinterpret_cast<const float4*>(features + id * F)[c4]
                                 : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(&sIn[wave][mm][4 * c4]) = v;
      }
    } else {
      for (int e = lane; e < nnk * F; e += 64) {
        const int mm = e / F, f = e - mm * F;
        const long long id = sIdx[wave][mm];
        sIn[wave][mm][f] = id >= 0 ? features[id * F + f] : 0.f;
      }
    }
    __builtin_amdgcn_wave_barrier();

    float col[MAX_CH] = {0.f, 0.f, 0.f};
    float jac[MAX_CH][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    if (dec.weighted_first) {
      // in = sum_m w_m [f_m, n_m] (neural_gaussians.py:701-705), one decoder evaluation
      if (lane < IN_PAD) {
        float a = 0.f;
        for (int mm = 0; mm < nnk; ++mm) a = fmaf(sW[wave][mm], sIn[wave][mm][lane], a);
        sAvg[wave][lane] = a;
      }
      __builtin_amdgcn_wave_barrier();
      float pre = b1;
#pragma unroll
      for (int i = 0; i < IN_PAD; i += 4) {
        const float4 t4 = *reinterpret_cast<const float4*>(&sAvg[wave][i]);
        pre = fmaf(w1[i], t4.x, pre);
        pre = fmaf(w1[i + 1], t4.y, pre);
        pre = fmaf(w1[i + 2], t4.z, pre);
        pre = fmaf(w1[i + 3], t4.w, pre);
      }
      const bool on = lane < Hd;
      const float hid = on ? fmaxf(pre, 0.f) : 0.f;
      const bool act = on && pre > 0.f;
      {
        float v[8];
#pragma unroll
        for (int c = 0; c < MAX_CH; ++c) v[c] = w2[c] * hid;
        const float g0 = act ? w2[0] : 0.f;
        v[3] = w1n0 * g0; v[4] = w1n1 * g0; v[5] = w1n2 * g0; v[6] = 0.f; v[7] = 0.f;
        const float tot = wave_reduce8(v, lane);
        if (lane < 8) {
          if (slot < 3) sR[wave][MAX_NNK][slot][0] = tot;
          else if (slot < 6) sR[wave][MAX_NNK][0][1 + slot - 3] = tot;
        }
      }
      if (JAC && count > 0) {
        if (C > 1) {
          float v[8];
          const float g1 = act ? w2[1] : 0.f, g2 = act ? w2[2] : 0.f;
          v[0] = w1n0 * g1; v[1] = w1n1 * g1; v[2] = w1n2 * g1;
          v[3] = w1n0 * g2; v[4] = w1n1 * g2; v[5] = w1n2 * g2; v[6] = 0.f; v[7] = 0.f;
          const float tot = wave_reduce8(v, lane);
          if (lane < 8 && slot < 6) sR[wave][MAX_NNK][1 + slot / 3][1 + slot % 3] = tot;
        }
        // t_mc = (W1^T (W2[c] . [pre > 0])) . in_m for every neighbour
        for (int mm = 0; mm < nnk; ++mm) {
          float acc = 0.f;
#pragma unroll
          for (int i = 0; i < IN_PAD; i += 4) {
            const float4 t4 = *reinterpret_cast<const float4*>(&sIn[wave][mm][i]);
            acc = fmaf(w1[i], t4.x, acc);
            acc = fmaf(w1[i + 1], t4.y, acc);
            acc = fmaf(w1[i + 2], t4.z, acc);
            acc = fmaf(w1[i + 3], t4.w, acc);
          }
          float v[8];
#pragma unroll
          for (int c = 0; c < MAX_CH; ++c) v[c] = act ? acc * w2[c] : 0.f;
          v[3] = 0.f; v[4] = 0.f; v[5] = 0.f; v[6] = 0.f; v[7] = 0.f;
          const float tot = wave_reduce8(v, lane);
          if (lane < 8 && slot < 3) sR[wave][mm][slot][0] = tot;
        }
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int c = 0; c < MAX_CH; ++c) {
        if (c >= C) continue;
        col[c] = sigmoidf(b2[c] + sR[wave][MAX_NNK][c][0]);
        if (JAC && count > 0) {
          const float ds = col[c] * (1.0f - col[c]);
          const float gn0 = sR[wave][MAX_NNK][c][1], gn1 = sR[wave][MAX_NNK][c][2], gn2 = sR[wave][MAX_NNK][c][3];
          float gx = 0.f, gy = 0.f, gz = 0.f, tbar = 0.f;
          for (int mm = 0; mm < nnk; ++mm) {
            const long long id = sIdx[wave][mm];
            if (id < 0) continue;
            float a0 = gn0, a1 = gn1, a2 = gn2;
            if (after_pgo) rot_active(orientations + 4 * id, gn0, gn1, gn2, a0, a1, a2);
            const float wm = sW[wave][mm];
            gx = fmaf(wm, a0, gx); gy = fmaf(wm, a1, gy); gz = fmaf(wm, a2, gz);
            tbar = fmaf(wm, sR[wave][mm][c][0], tbar);
          }
          for (int mm = 0; mm < nnk; ++mm) {
            if (sIdx[wave][mm] < 0) continue;
            const float k = (sR[wave][mm][c][0] - tbar) * sDu[wave][mm];
            gx = fmaf(k, sVec[wave][mm][0], gx);
            gy = fmaf(k, sVec[wave][mm][1], gy);
            gz = fmaf(k, sVec[wave][mm][2], gz);
          }
          jac[c][0] = ds * gx; jac[c][1] = ds * gy; jac[c][2] = ds * gz;
        }
      }
    } else {
      // per-neighbour decoder, sigmoid, then the IDW sum of the colours (utils/tracker.py:329-331)
      for (int mm = 0; mm < nnk; ++mm) {
        if (sIdx[wave][mm] < 0) continue;     // weight 0: the neighbour's colour does not reach the sum
        float pre = b1;
#pragma unroll
        for (int i = 0; i < IN_PAD; i += 4) {   // the row is broadcast from LDS sixteen bytes at a time
          const float4 t4 = *reinterpret_cast<const float4*>(&sIn[wave][mm][i]);
          pre = fmaf(w1[i], t4.x, pre);
          pre = fmaf(w1[i + 1], t4.y, pre);
          pre = fmaf(w1[i + 2], t4.z, pre);
          pre = fmaf(w1[i + 3], t4.w, pre);
        }
        const bool on = lane < Hd;
        const float hid = on ? fmaxf(pre, 0.f) : 0.f;
        if (!JAC) {
          float v[8];
#pragma unroll
          for (int c = 0; c < MAX_CH; ++c) v[c] = w2[c] * hid;
          v[3] = 0.f; v[4] = 0.f; v[5] = 0.f; v[6] = 0.f; v[7] = 0.f;
          const float tot = wave_reduce8(v, lane);
          if (lane < 8 && slot < 3) sR[wave][mm][slot][0] = tot;
        } else {
          const bool act = on && pre > 0.f;
          float v[8];
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const float gh = act ? w2[j] : 0.f;
            v[4 * j] = w2[j] * hid;
            v[4 * j + 1] = w1n0 * gh; v[4 * j + 2] = w1n1 * gh; v[4 * j + 3] = w1n2 * gh;
          }
          float tot = wave_reduce8(v, lane);
          if (lane < 8) sR[wave][mm][slot >> 2][slot & 3] = tot;
          if (C > 2) {
            const float gh = act ? w2[2] : 0.f;
            v[0] = w2[2] * hid;
            v[1] = w1n0 * gh; v[2] = w1n1 * gh; v[3] = w1n2 * gh;
            v[4] = 0.f; v[5] = 0.f; v[6] = 0.f; v[7] = 0.f;
            tot = wave_reduce8(v, lane);
            if (lane < 8 && slot < 4) sR[wave][mm][2][slot] = tot;
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
      // the k C sigmoids once, one (neighbour, channel) pair per lane, instead of on every lane of the finishing pass
      if (lane < nnk * C) {
        const int mm = lane / C, c = lane - mm * C;
        const float bb = c == 0 ? b2[0] : (c == 1 ? b2[1] : b2[2]);
        sS[wave][mm][c] = sIdx[wave][mm] >= 0 ? sigmoidf(bb + sR[wave][mm][c][0]) : 0.f;
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int c = 0; c < MAX_CH; ++c) {
        if (c >= C) continue;
        float gx = 0.f, gy = 0.f, gz = 0.f, acc = 0.f;
        for (int mm = 0; mm < nnk; ++mm) {
          const long long id = sIdx[wave][mm];
          if (id < 0) continue;
          const float s = sS[wave][mm][c];
          const float wm = sW[wave][mm];
          acc = fmaf(wm, s, acc);
          if (JAC) {
            float gn0 = sR[wave][mm][c][1], gn1 = sR[wave][mm][c][2], gn2 = sR[wave][mm][c][3];
            if (after_pgo) rot_active(orientations + 4 * id, gn0, gn1, gn2, gn0, gn1, gn2);
            const float k = wm * (s * (1.0f - s));
            gx = fmaf(k, gn0, gx); gy = fmaf(k, gn1, gy); gz = fmaf(k, gn2, gz);
          }
        }
        col[c] = acc;
        if (JAC && count > 0) {
          for (int mm = 0; mm < nnk; ++mm) {
            if (sIdx[wave][mm] < 0) continue;
            const float s = sS[wave][mm][c];
            const float k = (s - acc) * sDu[wave][mm];
            gx = fmaf(k, sVec[wave][mm][0], gx);
            gy = fmaf(k, sVec[wave][mm][1], gy);
            gz = fmaf(k, sVec[wave][mm][2], gz);
          }
          jac[c][0] = gx; jac[c][1] = gy; jac[c][2] = gz;
        }
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < MAX_CH; ++c)
        if (c < C) {
          color_out[q * C + c] = col[c];
          if (JAC) {
            jac_out[(q * C + c) * 3] = jac[c][0];
            jac_out[(q * C + c) * 3 + 1] = jac[c][1];
            jac_out[(q * C + c) * 3 + 2] = jac[c][2];
          }
        }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace

PINGS_API int pings_color_forward(const pings_color_decoder* dec, const float* features, int64_t rows,
                                  const float* points, const float* orientations, int32_t after_pgo,
                                  const float* queries, int64_t B, const int64_t* idx, int32_t nn_k, float* color,
                                  float* jac, void* stream) {
  PINGS_ARG_CHECK(dec && dec->W1 && dec->b1 && dec->W2 && dec->b2, "null decoder");
  PINGS_ARG_CHECK(dec->hidden > 0 && dec->hidden <= 64, "hidden must be in 1..64");
  PINGS_ARG_CHECK(dec->feat_dim > 0 && dec->feat_dim + 3 <= MAX_IN, "feature dim must be <= 61");
  PINGS_ARG_CHECK(dec->channels >= 1 && dec->channels <= MAX_CH, "channels must be in 1..3");
  PINGS_ARG_CHECK(nn_k > 0 && nn_k <= MAX_NNK, "nn_k must be in 1..16");
  PINGS_ARG_CHECK(!after_pgo || orientations, "after_pgo needs orientations");
  PINGS_ARG_CHECK(B >= 0 && rows >= 0, "negative size");
  if (B == 0) return PINGS_OK;
  PINGS_ARG_CHECK(rows > 0 && features && points && queries && idx && color, "null pointer");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope ps("color_forward", st);
  const int need = dec->feat_dim + 3;
  const int pad = need <= 12 ? 12 : need <= 36 ? 36 : 64;
  return pings::with_class<12, 36, 64>(pad, "colour forward", [&](auto p) {
    return pings::with_flag(jac != nullptr, [&](auto j) {
      const auto kernel = color_forward_kernel<decltype(p)::value, decltype(j)::value>;
      // (Measured and dropped: one resident round of workgroups, resident_grid, as the SDF vector kernel uses — colour
      // device loop 9.76 against 9.91 ms per 50-iteration call at 20,000 points, 38.5 against 36.3 ms at 131,072.)
      return pings::launch(kernel, dim3(capped_grid(B)), 64 * WAVES_PER_BLOCK, 0, st, *dec, features, (long long)rows,
                           points, orientations, (int)after_pgo, queries, (long long)B, (const long long*)idx,
                           (int)nn_k, color, jac);
    });
  });
}
