// sg_embed_plan.h — what the embed-once translation units share (sg_embed_nodes.hip: the
// node stack on single graphs, forward and backward, for include/siamese_embed.h,
// siamese_embed_train.h and siamese_embed_drop.h; sg_embed.hip: the score grid and top-k of
// retrieval; sg_embed_train.hip: the grid of training; sg_search.hip: search,
// include/siamese_search.h):
// the plans of a model (dropout read as off, dropout refused, dropout kept); the store side
// of the embedding kernel (which
// graphs a wavefront takes, what it reports, Â and the types staged in its LDS slice);
// the NTN score grid's limits, query-chunk split, common kernel arguments, per-query table
// kernel and MFMA operand helpers; and the key of the top-k selections' total order.
// Internal linkage throughout: each unit compiles its own copy.
#pragma once
#include <type_traits>

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

// The plan of the model with its own dropout (keep_prob and the per-layer dropout flags, as
// the pair paths build it) and the f32 store: graph-keyed masks (sg_embed_nodes.hip, MASK)
int embed_drop_plan(const sg_model_t *model, SgGenPlan *P) {
  if (!model) return SG_ERR_ARG;
  if (!(model->keep_prob > 0.f && model->keep_prob <= 1.f)) return SG_ERR_ARG;
  int64_t wn = 0;
  if (sg_web_plan_params(model, &wn) == SG_OK && sg_web_lds_ok(model)) return SG_ERR_UNSUPPORTED;
  sg_model_t m = *model;
  m.adj_dtype = SG_DTYPE_F32;
  return sg_build_plan(&m, P);
}

// embed_plan with the NTN head the score grid serves, or an SG_ERR_* code
int grid_plan(const sg_model_t *model, SgGenPlan *P) {
  const int rc = embed_plan(model, P);
  if (rc != SG_OK) return rc;
  if (P->head_kind != SG_NTN || P->D > kGridMaxD || P->K > kGridMaxK) return SG_ERR_UNSUPPORTED;
  return SG_OK;
}

// SG_OK for a model without any effective dropout (what embed-once training without masks
// serves: train_plan, and dot_train_plan of sg_dot_grid.hip), or an SG_ERR_* code
int plan_no_dropout(const sg_model_t *model) {
  if (!(model->keep_prob > 0.f && model->keep_prob <= 1.f)) return SG_ERR_ARG;
  if (sg_keep_threshold(model->keep_prob) != 65536u)
    for (int li = 0; li < model->num_layers; ++li)
      if (model->layers[li].dropout) return SG_ERR_UNSUPPORTED;
  return SG_OK;
}

// grid_plan / embed_plan of a model without any effective dropout, or an SG_ERR_* code
// (embed-once training, include/siamese_embed_train.h)
int train_plan(const sg_model_t *model, SgGenPlan *P, bool grid) {
  if (!model) return SG_ERR_ARG;
  const int rc = grid ? grid_plan(model, P) : embed_plan(model, P);
  return rc != SG_OK ? rc : plan_no_dropout(model);
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
// The store side of the embedding kernel (sg_embed_nodes_kernel, sg_embed_nodes.hip): one
// wavefront runs the node stack on two graphs, the two "sides" of the generic kernel's LDS
// slice; unit q of a call takes entries 2 q and 2 q + 1 of graph_idx.
// ---------------------------------------------------------------------------
struct StoreArgs {
  const float *sadj;
  const int32_t *stypes, *sn;
  int n_graphs, max_nodes;
  const int32_t *gidx;   // store ids of the entries, or null: entry c is graph c
  int64_t count;
  int32_t *status;
};

void fill_store_args(StoreArgs &A, const SgGenPlan &P, const float *store_adj,
                     const int32_t *store_types, const int32_t *store_n, int n_graphs,
                     const int32_t *graph_idx, int64_t count, int32_t *status_out) {
  A.sadj = store_adj;
  A.stypes = store_types;
  A.sn = store_n;
  A.n_graphs = n_graphs;
  A.max_nodes = plan_max_nodes(P);
  A.gidx = graph_idx;
  A.count = count;
  A.status = status_out;
}

// Resolves unit q of the wavefront whose LDS slice is S.  Per side: have, the entry exists
// (the second of an odd tail does not); ok, it can be embedded; g and n, the graph the side
// computes and its node count.  An entry that cannot be embedded (id outside the store:
// SG_ERR_ARG; node count outside [1, max_nodes]: SG_ERR_SHAPE, both raised in the device
// status) or that does not exist is replaced by the other side's graph for the computation
// (never n = 0: Average divides by the row count); its ok stays false and the caller writes
// nothing for it, or zeros.  Returns false, with nothing staged, when neither side can be
// embedded; else Â [2][n_max][n_max] and the types [2][n_max] of both sides are staged at
// adj and types in the pair-record layout and the wavefront is synchronised.
// (Plain arrays of the caller, not a struct: the compiler keeps them in registers.)
__device__ __forceinline__ bool stage_graph_pair(const SgGenPlan &P, const StoreArgs &A, float *S,
                                                 int64_t q, int lane, int (&g)[2], int (&n)[2],
                                                 bool (&ok)[2], bool (&have)[2], float *&adj,
                                                 int *&types) {
  for (int s = 0; s < 2; ++s) {
    const int64_t c = 2 * q + s;
    have[s] = c < A.count;
    g[s] = 0;
    n[s] = 0;
    ok[s] = false;
    if (!have[s]) continue;
    const int64_t id = A.gidx ? (int64_t)A.gidx[c] : c;
    const bool in_store = id >= 0 && id < A.n_graphs;
    if (in_store) {
      g[s] = (int)id;
      n[s] = A.sn[id];
    }
    ok[s] = in_store && n[s] >= 1 && n[s] <= A.max_nodes;
    if (!ok[s] && lane == 0 && A.status)
      atomicExch(A.status, (int32_t)(in_store ? SG_ERR_SHAPE : SG_ERR_ARG));
  }
  if (!ok[0] && !ok[1]) return false;
  if (!ok[0]) { g[0] = g[1]; n[0] = n[1]; }
  if (!ok[1]) { g[1] = g[0]; n[1] = n[0]; }
  const int nmax = P.n_max, nn = nmax * nmax;
  adj = S + P.l_rec;
  types = (int *)(S + P.l_rec + P.rec_types);
  for (int w = lane; w < 2 * nn; w += SG_WAVE) {
    const int s = w / nn, o = w - s * nn;
    adj[w] = A.sadj[(size_t)g[s] * nn + o];
  }
  for (int w = lane; w < 2 * nmax; w += SG_WAVE) {
    const int s = w / nmax, o = w - s * nmax;
    types[w] = A.stypes[(size_t)g[s] * nmax + o];
  }
  sg_wsync();
  return true;
}

// ---------------------------------------------------------------------------
// NTN score grid: the head the grid serves, its query tables, and what the forward kernel
// (sg_grid_kernel) and the forward + adjoint kernel (sg_grid_bwd_kernel) set up alike.
// ---------------------------------------------------------------------------
int grid_dp(const SgGenPlan &P) { return (P.D + 1 + 3) & ~3; }

// Workgroups of a grid kernel: ncb column blocks of 64 database rows times nqc chunks of qb
// queries (a multiple of the workgroup's 4 wavefronts): enough chunks to reach `target`
// workgroups, else as many queries as possible per load of the database tiles.  The guards
// (ncb of an empty grid, nqc >= 1, qb >= 4) only act for m = 0 or n = 0, which the
// workspace query of the training call accepts; they are no-ops for every grid that runs.
struct GridSplit {
  int64_t ncb, nqc, qb, blocks;
};

GridSplit grid_split(int64_t m, int64_t n, int64_t target) {
  GridSplit s;
  s.ncb = (n + 63) / 64;
  int64_t nqc = (target + s.ncb - 1) / (s.ncb > 0 ? s.ncb : 1);
  const int64_t max_qc = (m + 3) / 4;
  nqc = nqc > max_qc ? max_qc : nqc;
  nqc = nqc < 1 ? 1 : nqc;
  s.qb = (((m + nqc - 1) / nqc) + 3) & ~(int64_t)3;
  s.qb = s.qb < 4 ? 4 : s.qb;
  s.nqc = (m + s.qb - 1) / s.qb;
  s.blocks = s.ncb * s.nqc;
  return s;
}

// Query tables Q [m][Dp][16], Dp = D + 1 rounded up to the MFMA k-step of 4; rows above D
// and columns k >= K are zero.
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

void launch_grid_q(const SgGenPlan &P, const float *emb_q, int64_t m, const float *params,
                   float *Q, hipStream_t st) {
  const int Dp = grid_dp(P);
  const int64_t qelems = m * Dp * 16;
  hipLaunchKernelGGL(sg_grid_q_kernel, dim3((unsigned)((qelems + 255) / 256)), dim3(256), 0, st,
                     emb_q, m, P.D, P.K, Dp, params, P.offW, P.offV, P.offB, Q);
}

// The arguments both grid kernels take; each kernel's struct derives from this one.
struct GridCommon {
  const float *Q, *edb, *U;
  int64_t m, n, ncb;
  int D, K, qb;
  int act, ntn_mode, final_act;
  float yeta;
};

void fill_grid_common(GridCommon &A, const SgGenPlan &P, const float *Q, const float *emb_db,
                      const float *params, int64_t m, int64_t n, const GridSplit &s) {
  A.Q = Q;
  A.edb = emb_db;
  A.U = params + P.offU;
  A.m = m;
  A.n = n;
  A.ncb = s.ncb;
  A.D = P.D;
  A.K = P.K;
  A.qb = (int)s.qb;
  A.act = P.head_act;
  A.ntn_mode = P.ntn_mode;
  A.final_act = P.final_act;
  A.yeta = P.yeta;
}

// f(std::integral_constant<int, NS>) for NS = ns, the MFMA k-steps Dp / 4 in 1 .. 8
template <class F>
void grid_dispatch_ns(int ns, F &&f) {
  switch (ns) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 7: f(std::integral_constant<int, 7>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
  }
}

// component b of the augmented database row [e_j, 1, 0…]; rows j >= n are zero
__device__ __forceinline__ float grid_aug(const GridCommon &A, int64_t j, int b) {
  if (j >= A.n || b > A.D) return 0.f;
  return b < A.D ? A.edb[j * A.D + b] : 1.f;
}

// The scale of the sum over k: ΣU in parameter order (reference, quirk A1: every r_k counts
// once and the sum is scaled by ΣU) or 1 (intended: the weights are per column).
__device__ __forceinline__ float grid_usum(const GridCommon &A) {
  float usum = 1.f;
  if (A.ntn_mode != SG_NTN_INTENDED) {
    usum = 0.f;
    for (int k = 0; k < A.K; ++k) usum += A.U[k];
  }
  return usum;
}

// Column k of the 16-column tile.  mask: k < K (act(0) of a padded column is not 0 for
// sigmoid); w: the weight of r_k in the sum over k (intended U_k, reference 1); uw: ∂s/∂r_k
// (intended U_k, reference ΣU).  w and uw are 0 for a padded column.
struct GridCol {
  bool mask;
  float w, uw;
};

__device__ __forceinline__ GridCol grid_col(const GridCommon &A, int k, float usum) {
  const bool intended = A.ntn_mode == SG_NTN_INTENDED;
  GridCol c;
  c.mask = k < A.K;
  c.w = c.mask ? (intended ? A.U[k] : 1.f) : 0.f;
  c.uw = c.mask ? (intended ? A.U[k] : usum) : 0.f;
  return c;
}

// The MFMA operand of query i's table: b[s] = Q_i[4 s + (lane >> 4)][lane & 15], one
// coalesced 256-B load per k-step (L2-resident).  Returns Q_i.
template <int NS>
__device__ __forceinline__ const float *grid_load_q(const GridCommon &A, int64_t i, int lane,
                                                    float (&b)[NS]) {
  const float *__restrict__ Qi = A.Q + i * (NS * 64);
#pragma unroll
  for (int s = 0; s < NS; ++s) b[s] = Qi[s * 64 + lane];
  return Qi;
}

// ---------------------------------------------------------------------------
// The total order of the top-k selections (sg_topk_rows, sg_search_topk): a 64-bit key
// (rank of the value, column) whose unsigned order is by value (descending when largest),
// ties to the smaller column, NaN after every number and by column.  Keys of distinct
// columns differ, and every key is below ~0 (columns are < 2^31).
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t topk_key(float x, uint32_t col, int largest) {
  uint32_t rk = 0xFFFFFFFFu;   // NaN: after every number
  if (x == x) {
    const uint32_t u = x == 0.f ? 0u : __float_as_uint(x);   // -0 ranks with +0
    const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    rk = largest ? ~asc : asc;   // both within [0x007FFFFF, 0xFF800000]
  }
  return ((uint64_t)rk << 32) | col;
}

}  // namespace
