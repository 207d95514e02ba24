// sg_generic.hip — generic Siamese fwd(+bwd) kernel: one wavefront owns one
// graph pair; the pair record, every activation and every gradient tensor of
// the pair live in the wave's LDS slice; lanes sweep each op element-wise.
// Covers every layer stack sg_build_plan accepts (GCN/Dense/Padding/Average/
// Attention → NTN/Dot), all activations, both NTN modes and both loss modes.
// The default AIDS stack has a fused register/MFMA kernel (sg_fast.hip); this
// one is its general fallback and its on-GPU cross-check.
//
// Reference math: layers.py:91-118 (GCN), 136-140 (Average), 154-160
// (Attention), 192-205 (Dense), 223-227 (Padding), 249-252 (Dot), 282-310
// (NTN), 332-338 (sparse dropout); models.py:39-88; model_mse.py:117-151.
#include "sg_gen_nodes.h"   // gen_forward_nodes, gen_backward_nodes, rows_of (shared)
#include "sg_paths.h"

namespace {

struct GenArgs {
  const uint8_t *recs;
  const int32_t *order;   // processing order (sg_pair_order) or null
  int64_t n_pairs;
  int64_t pair_offset;
  float inv_batch;      // 1/B for the aligned loss
  const float *params;
  uint32_t key;
  const float *y_stats; // {ybar, ½Σ(y-ȳ)²}
  float *s_out;
  float *slab;          // [gridDim.x][n_params + 1]
};

template <bool BWD>
__global__ void __launch_bounds__(256) sg_generic_kernel(SgGenPlan P, GenArgs A) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int gfl = BWD ? ((P.n_params + 1 + 3) & ~3) : 0;
  float *G = smem;
  float *S = smem + gfl + wave * P.wave_floats;
  const float *__restrict__ prm = A.params;
  if (BWD) {
    for (int i = threadIdx.x; i < gfl; i += blockDim.x) G[i] = 0.f;
  }
  __syncthreads();
  const int nmax = P.n_max;
  const float ybar = (BWD && P.loss_mode == SG_LOSS_BROADCAST) ? A.y_stats[0] : 0.f;
  float loss_acc = 0.f;
  for (int64_t q = (int64_t)blockIdx.x * nw + wave; q < A.n_pairs; q += (int64_t)gridDim.x * nw) {
    int64_t p = q;   // record = batch pair index
    if (A.order) {
      const int v = A.order[q];
      p = v < 0 ? 0 : (v >= A.n_pairs ? A.n_pairs - 1 : v);   // never out of bounds
    }
    const uint32_t *rec = (const uint32_t *)(A.recs + (size_t)p * (size_t)P.hbm_words * 4u);
    uint32_t *R = (uint32_t *)(S + P.l_rec);
    if (P.adj_dtype == SG_DTYPE_BF16) {   // widen Â to the f32 LDS layout
      const int aw = P.hbm_adj_words;
      for (int i = lane; i < P.hbm_words; i += SG_WAVE) {
        const uint32_t v = rec[i];
        if (i < aw) {
          R[2 * i] = v << 16;
          R[2 * i + 1] = v & 0xFFFF0000u;
        } else if (i - aw < P.rec_words - 2 * aw) {
          R[i + aw] = v;
        }
      }
    } else {
      for (int i = lane; i < P.rec_words; i += SG_WAVE) R[i] = rec[i];
    }
    sg_wsync();
    const float *adj = S + P.l_rec;
    const int *types = (const int *)(S + P.l_rec + P.rec_types);
    const int n0 = ((const int *)(S + P.l_rec))[P.rec_nnodes];
    const int n1 = ((const int *)(S + P.l_rec))[P.rec_nnodes + 1];
    const float label = S[P.l_rec + P.rec_label];
    const uint32_t pk = sg_pair_key(A.key, (uint32_t)(A.pair_offset + p));
    gen_forward_nodes(P, S, prm, adj, types, n0, n1, pk, lane);

    // ---- pair head ----
    const SgGenLayer &last = P.L[P.nl - 1];
    const float *e0 = S + last.l_out;
    const float *e1 = e0 + last.Rout * last.dout;
    const int D = P.D, K = P.K;
    float s = 0.f, rsum = 0.f, usum = 0.f;
    float *x12 = S + P.l_x12, *u = S + P.l_u, *m = S + P.l_m;
    if (P.head_kind == SG_NTN) {
      for (int e = lane; e < 2 * D; e += SG_WAVE) {
        const int sd = e / D, q = e - sd * D;
        const float v = (sd ? e1 : e0)[q];
        x12[e] = sg_keep(pk, P.head_li, sd, q, P.head_thr) ? v * P.head_inv_keep : 0.f;
      }
      sg_wsync();
      for (int e = lane; e < D * K; e += SG_WAVE) {  // u[a][k] = Σ_b W[a][b][k] x2[b]
        const int a = e / K, k = e - a * K;
        float acc = 0.f;
        for (int b = 0; b < D; ++b) acc = fmaf(prm[P.offW + (a * D + b) * K + k], x12[D + b], acc);
        u[e] = acc;
      }
      sg_wsync();
      for (int k = lane; k < K; k += SG_WAVE) {
        float acc = 0.f;
        for (int i = 0; i < 2 * D; ++i) acc = fmaf(prm[P.offV + k * 2 * D + i], x12[i], acc);
        for (int a = 0; a < D; ++a) acc = fmaf(x12[a], u[a * K + k], acc);
        if (P.head_bias) acc += prm[P.offB + k];
        m[k] = acc;
      }
      sg_wsync();
      for (int k = 0; k < K; ++k) {
        const float r = sg_act(P.head_act, m[k]);
        const float U = prm[P.offU + k];
        rsum += r;
        usum += U;
        if (P.ntn_mode == SG_NTN_INTENDED) s = fmaf(U, r, s);
      }
      if (P.ntn_mode == SG_NTN_REFERENCE) s = usum * rsum;
    } else {  // Dot
      float part = 0.f;
      for (int q = lane; q < D; q += SG_WAVE) part = fmaf(e0[q], e1[q], part);
      s = sg_wave_sum(part);
    }

    if (!BWD) {
      if (lane == 0) A.s_out[p] = s;
      continue;
    }
    if (A.s_out && lane == 0) A.s_out[p] = s;
    // ---- loss (model_mse.py:145-151) ----
    const float yhat = sg_final(P.final_act, P.yeta, s);
    float gy;
    if (P.loss_mode == SG_LOSS_BROADCAST) {
      gy = yhat - ybar;                     // ∂/∂ŷ_j of l2_loss((B,1)-(B,))/B
      loss_acc += 0.5f * gy * gy;
    } else {
      const float dlt = yhat - label;
      gy = dlt * A.inv_batch;
      loss_acc += 0.5f * dlt * dlt * A.inv_batch;
    }
    const float gs = gy * sg_final_grad(P.final_act, P.yeta, s, yhat);

    // ---- head backward ----
    float *gcur = S + P.l_g0, *gnext = S + P.l_g1;
    const int Rh = last.Rout * last.dout;
    if (P.head_kind == SG_NTN) {
      float *gm = S + P.l_gm;
      for (int k = lane; k < K; k += SG_WAVE) {
        const float r = sg_act(P.head_act, m[k]);
        const float gr = (P.ntn_mode == SG_NTN_REFERENCE) ? gs * usum : gs * prm[P.offU + k];
        const float g = sg_act_grad(P.head_act, m[k], r, gr);
        gm[k] = g;
        if (P.head_bias) atomicAdd(&G[P.offB + k], g);
        atomicAdd(&G[P.offU + k], (P.ntn_mode == SG_NTN_REFERENCE) ? gs * rsum : gs * r);
      }
      sg_wsync();
      for (int e = lane; e < K * 2 * D; e += SG_WAVE) {
        const int k = e / (2 * D), i = e - k * 2 * D;
        atomicAdd(&G[P.offV + e], gm[k] * x12[i]);
      }
      for (int e = lane; e < D * D * K; e += SG_WAVE) {
        const int a = e / (D * K), rem = e - a * D * K, b = rem / K, k = rem - b * K;
        atomicAdd(&G[P.offW + e], gm[k] * x12[a] * x12[D + b]);
      }
      for (int e = lane; e < 2 * D; e += SG_WAVE) {
        const int sd = e / D, q = e - sd * D;
        float acc = 0.f;
        for (int k = 0; k < K; ++k) acc = fmaf(prm[P.offV + k * 2 * D + e], gm[k], acc);
        if (sd == 0) {
          for (int k = 0; k < K; ++k) acc = fmaf(u[q * K + k], gm[k], acc);
        } else {
          for (int k = 0; k < K; ++k) {
            float w = 0.f;
            for (int a = 0; a < D; ++a) w = fmaf(x12[a], prm[P.offW + (a * D + q) * K + k], w);
            acc = fmaf(gm[k], w, acc);
          }
        }
        const float g = sg_keep(pk, P.head_li, sd, q, P.head_thr) ? acc * P.head_inv_keep : 0.f;
        gcur[sd * Rh + q] = g;
      }
    } else {
      for (int e = lane; e < 2 * D; e += SG_WAVE) {
        const int sd = e / D, q = e - sd * D;
        gcur[e] = gs * (sd ? e0[q] : e1[q]);
      }
    }
    sg_wsync();
    gen_backward_nodes(P, S, G, prm, adj, types, n0, n1, pk, lane, gcur, gnext);
  }
  if (BWD) {
    if (lane == 0) atomicAdd(&G[P.n_params], loss_acc);
    __syncthreads();
    float *dst = A.slab + (size_t)blockIdx.x * (size_t)(P.n_params + 1);
    for (int i = threadIdx.x; i <= P.n_params; i += blockDim.x) dst[i] = G[i];
  }
}

}  // namespace

// Launch shape of the generic kernel (sg_paths.h); the backward's accumulator is the
// gradient and the loss.  sg_workspace_bytes sizes the slab through sg_generic_slab_floats.
static SgGenLaunch sg_generic_launch(const SgGenPlan &P, int64_t n_pairs, bool bwd) {
  return sg_gen_launch_shape(P, bwd ? P.n_params + 1 : 0, n_pairs);
}

int sg_generic_lds_ok(const SgGenPlan &P, bool bwd) { return sg_generic_launch(P, 1, bwd).fits(); }

int64_t sg_generic_slab_floats(const SgGenPlan &P, int64_t n_pairs) {
  return (int64_t)sg_generic_launch(P, n_pairs, true).blocks * (P.n_params + 1);
}

int sg_generic_run(const SgGenPlan &P, const SgPairRun &r, int *blocks_out) {
  const bool bwd = r.bwd;
  const hipStream_t stream = r.stream;
  const SgGenLaunch L = sg_generic_launch(P, r.n_pairs, bwd);
  if (!L.fits()) return SG_ERR_UNSUPPORTED;
  GenArgs A;
  A.recs = (const uint8_t *)r.recs;
  A.order = r.order;
  A.n_pairs = r.n_pairs;
  A.pair_offset = r.pair_offset;
  A.inv_batch = r.batch_total > 0 ? 1.f / (float)r.batch_total : 0.f;
  A.params = r.params;
  A.key = sg_seed_key(r.seed);
  A.y_stats = r.y_stats;
  A.s_out = r.s_out;
  A.slab = r.slab;
  sg_allow_lds(bwd ? (const void *)sg_generic_kernel<true> : (const void *)sg_generic_kernel<false>,
               L.lds_bytes);
  if (bwd)
    hipLaunchKernelGGL(sg_generic_kernel<true>, dim3(L.blocks), dim3(64 * L.waves_per_block),
                       L.lds_bytes, stream, P, A);
  else
    hipLaunchKernelGGL(sg_generic_kernel<false>, dim3(L.blocks), dim3(64 * L.waves_per_block),
                       L.lds_bytes, stream, P, A);
  if (blocks_out) *blocks_out = L.blocks;
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}
