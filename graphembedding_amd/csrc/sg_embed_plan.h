// sg_embed_plan.h — what the embed-once translation units share (sg_embed.hip: retrieval,
// include/siamese_embed.h; sg_embed_train.hip: training, include/siamese_embed_train.h):
// the dropout-off plan of a model, the limits of the NTN score grid, and the per-query
// table kernel.  Internal linkage throughout: each unit compiles its own copy.
#pragma once
#include "sg_gen_nodes.h"
#include "sg_paths.h"

namespace {

constexpr int kGridMaxD = 31;     // D + 1 <= 32: at most 8 MFMA k-steps
constexpr int kGridMaxK = 16;     // one 16-column tile
constexpr int64_t kMaxRows = (int64_t)1 << 29;   // launch sizes stay below 2^31 workgroups

// The plan of the model with dropout off and the f32 store (inference mode)
int embed_plan(const sg_model_t *model, SgGenPlan *P) {
  if (!model) return SG_ERR_ARG;
  int64_t wn = 0;
  if (sg_web_plan_params(model, &wn) == SG_OK && sg_web_lds_ok(model)) return SG_ERR_UNSUPPORTED;
  sg_model_t m = *model;
  m.keep_prob = 1.f;   // every threshold 65536: sg_keep is always true
  m.adj_dtype = SG_DTYPE_F32;
  return sg_build_plan(&m, P);
}

int plan_embed_dim(const SgGenPlan &P) {
  const SgGenLayer &last = P.L[P.nl - 1];
  return last.Rout * last.dout;
}

// largest node count the stack takes: the record capacity and the rows of a Padding layer
// that pads the graph's own rows (A9).  A Padding layer after pooling or after another
// Padding (rin_fixed >= 0) pads a fixed row count and does not bound the graph.
int plan_max_nodes(const SgGenPlan &P) {
  int mx = P.n_max;
  for (int l = 0; l < P.nl; ++l)
    if (P.L[l].kind == SG_PADDING && P.L[l].rin_fixed < 0 && P.L[l].Rout < mx) mx = P.L[l].Rout;
  return mx;
}

// ---------------------------------------------------------------------------
// Query tables Q [m][Dp][16], Dp = D + 1 rounded up to the MFMA k-step of 4; rows above D
// and columns k >= K are zero.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) sg_grid_q_kernel(const float *__restrict__ eq, int64_t m,
                                                        int D, int K, int Dp,
                                                        const float *__restrict__ prm, int offW,
                                                        int offV, int offB,
                                                        float *__restrict__ Q) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= m * Dp * 16) return;
  const int k = (int)(t & 15);
  const int64_t ib = t >> 4;
  const int b = (int)(ib % Dp);
  const float *e = eq + (ib / Dp) * D;
  float acc = 0.f;
  if (k < K && b < D) {
    for (int a = 0; a < D; ++a) acc = fmaf(e[a], prm[offW + (a * D + b) * K + k], acc);
    acc += prm[offV + k * 2 * D + D + b];
  } else if (k < K && b == D) {
    for (int a = 0; a < D; ++a) acc = fmaf(prm[offV + k * 2 * D + a], e[a], acc);
    if (offB >= 0) acc += prm[offB + k];
  }
  Q[t] = acc;
}

// the NTN head the grid serves, or an SG_ERR_* code
int grid_plan(const sg_model_t *model, SgGenPlan *P) {
  const int rc = embed_plan(model, P);
  if (rc != SG_OK) return rc;
  if (P->head_kind != SG_NTN || P->D > kGridMaxD || P->K > kGridMaxK) return SG_ERR_UNSUPPORTED;
  return SG_OK;
}

int grid_dp(const SgGenPlan &P) { return (P.D + 1 + 3) & ~3; }

}  // namespace
