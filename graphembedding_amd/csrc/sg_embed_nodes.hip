// sg_embed_nodes.hip — the generic node stack on single graphs: every embed-once call that
// embeds graphs or takes an embedding's gradient back through the node layers.
//   sg_embed, sg_embed_dim                    include/siamese_embed.h        (inference plan)
//   sg_embed_bwd (+ workspace query)          include/siamese_embed_train.h  (dropout-0 plan)
//   sg_embed_drop, sg_embed_drop_bwd (+ ws)   include/siamese_embed_drop.h   (the model's dropout)
// One kernel template and one host launcher serve all of them: a call is (plan, BWD, MASK).
//
// MASK is graph-keyed dropout.  The reference draws its masks per pair (layers.py:334-336,
// tf.nn.dropout; quirk A4); here entry c' = entry_offset + c of a call is side c' & 1 of unit
// c' >> 1 and draws the masks the generic pair kernel (sg_generic.hip) draws for that pair
// and side: the node layers' through gen_forward_nodes / gen_backward_nodes under the unit's
// key, and the mask the NTN head puts on its input vector (sg_generic.hip: x12 in the
// forward, the gradient of e0 / e1 in the backward), which is a per-side operation on the
// embedding and so folds into the forward's output row and the backward's seed.  The grid
// kernels then run unchanged on the masked embeddings, with keep_prob 1.
// The plain calls are the masked calls with MASK off: key 0 under a plan whose thresholds
// all keep, no head mask, entry_offset 0; their instantiations hold no hash or mask code.
#include "../../include/siamese_embed.h"
#include "../../include/siamese_embed_drop.h"
#include "../../include/siamese_embed_train.h"
#include "sg_embed_bwd.h"

namespace {

// A mode ignores the fields it does not use.
struct EmbedNodesArgs : StoreArgs {
  const float *params;
  float *out;        // forward: [count][E]
  const float *g_emb;
  float *slab;       // BWD: [gridDim.x][hoff]
  int64_t unit0;     // MASK: entry_offset / 2, the global number of the call's unit 0
  uint32_t key;      // MASK: sg_seed_key(seed)
  int hoff;          // BWD: floats of the accumulator and of a slab row
};

// MASK: element e of side s through the head-input mask (sg_generic.hip, x12): thr 65536
// keeps all.  Else the value.
template <bool MASK>
__device__ __forceinline__ float head_masked(const SgGenPlan &P, uint32_t pk, int s, int e,
                                             float v) {
  if constexpr (MASK)
    return sg_keep(pk, P.head_li, s, e, P.head_thr) ? v * P.head_inv_keep : 0.f;
  else
    return v;
}

// ---------------------------------------------------------------------------
// One wavefront runs gen_forward_nodes on the two graphs stage_graph_pair resolves and stages
// (sg_embed_plan.h), under the key of unit unit0 + q (MASK) or key 0.
// Forward: each side's row goes out (through the head mask); the row of an entry that cannot
// be embedded is zeroed, the missing partner of an odd tail has no row.
// Backward: the output gradients of the two sides are seeded from g_emb (through the head
// mask: g_emb is the gradient of the masked embedding), gen_backward_nodes adds into the
// workgroup's zeroed accumulator G[0 .. hoff), and G goes to the workgroup's slab row.  A
// side that cannot be embedded runs the other side's graph under its own side index with a
// zero seed: the backward is linear in the seed, so it adds exact zeros.
// ---------------------------------------------------------------------------
template <bool BWD, bool MASK>
__global__ void __launch_bounds__(256) sg_embed_nodes_kernel(SgGenPlan P, EmbedNodesArgs A) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int gfl = BWD ? (A.hoff + 3) & ~3 : 0;
  float *G = smem;
  float *S = smem + gfl + wave * P.wave_floats;
  if constexpr (BWD) {
    for (int i = threadIdx.x; i < gfl; i += blockDim.x) G[i] = 0.f;
    __syncthreads();
  }
  const SgGenLayer &last = P.L[P.nl - 1];
  const int E = last.Rout * last.dout;
  const int64_t npair = (A.count + 1) >> 1;
  for (int64_t q = (int64_t)blockIdx.x * nw + wave; q < npair; q += (int64_t)gridDim.x * nw) {
    int g[2], n[2];
    bool ok[2], have[2];
    float *adj;
    int *types;
    const bool run = stage_graph_pair(P, A, S, q, lane, g, n, ok, have, adj, types);
    if (!run) {
      if constexpr (!BWD) {
        float *o0 = A.out + (size_t)(2 * q) * E, *o1 = o0 + E;
        for (int e = lane; e < E; e += SG_WAVE) {
          o0[e] = 0.f;
          if (have[1]) o1[e] = 0.f;
        }
      }
      continue;
    }
    uint32_t pk = 0u;
    if constexpr (MASK) pk = sg_pair_key(A.key, (uint32_t)(A.unit0 + q));
    gen_forward_nodes(P, S, A.params, adj, types, n[0], n[1], pk, lane);
    if constexpr (!BWD) {
      const float *e0 = S + last.l_out;
      float *o0 = A.out + (size_t)(2 * q) * E, *o1 = o0 + E;
      for (int e = lane; e < E; e += SG_WAVE) {
        o0[e] = ok[0] ? head_masked<MASK>(P, pk, 0, e, e0[e]) : 0.f;
        if (have[1]) o1[e] = ok[1] ? head_masked<MASK>(P, pk, 1, e, e0[E + e]) : 0.f;
      }
    } else {
      float *gcur = S + P.l_g0, *gnext = S + P.l_g1;
      const float *ge = A.g_emb + (size_t)(2 * q) * E;
      // both sides written out, as in the forward: with one loop over e < 2 E and a run-time
      // side the masked kernel gets a 36-byte private segment (the plain one does not)
      for (int e = lane; e < E; e += SG_WAVE) {
        gcur[e] = ok[0] ? head_masked<MASK>(P, pk, 0, e, ge[e]) : 0.f;
        gcur[E + e] = ok[1] ? head_masked<MASK>(P, pk, 1, e, ge[E + e]) : 0.f;
      }
      sg_wsync();
      gen_backward_nodes(P, S, G, A.params, adj, types, n[0], n[1], pk, lane, gcur, gnext);
    }
    sg_wsync();   // the next graphs overwrite the slice
  }
  if constexpr (BWD) {
    __syncthreads();
    float *dst = A.slab + (size_t)blockIdx.x * (size_t)A.hoff;
    for (int i = threadIdx.x; i < A.hoff; i += blockDim.x) dst[i] = G[i];
  }
}

// ---------------------------------------------------------------------------
// Host: the plan a call runs under, and the one launcher
// ---------------------------------------------------------------------------
enum NodesPlan {
  kInference,   // embed_plan: keep_prob read as 1
  kTrain,       // train_plan: a model with effective dropout is refused
  kDropout      // embed_drop_plan: the model's dropout, graph-keyed masks (MASK)
};

int nodes_plan(NodesPlan kind, const sg_model_t *model, SgGenPlan *P) {
  switch (kind) {
    case kInference: return embed_plan(model, P);
    case kTrain: return train_plan(model, P, false);
    default: return embed_drop_plan(model, P);
  }
}

// flat offset of the head's first variable: the node layers' range is [0, head_offset)
int head_offset(const SgGenPlan &P) { return P.head_kind == SG_NTN ? P.offW : P.n_params; }

// The generic kernel's shape with one unit per two entries; the backward has the node layers'
// gradient as the accumulator, and its workspace is one slab row per workgroup of this shape.
SgGenLaunch nodes_launch(const SgGenPlan &P, bool bwd, int64_t count) {
  return sg_gen_launch_shape(P, bwd ? head_offset(P) : 0, (count + 1) / 2);
}

int64_t nodes_bwd_workspace_bytes(NodesPlan kind, const sg_model_t *model, int64_t count) {
  SgGenPlan P;
  if (count < 0 || nodes_plan(kind, model, &P) != SG_OK) return -1;
  const SgGenLaunch L = nodes_launch(P, true, count);
  if (!L.fits()) return -1;
  return (int64_t)L.blocks * head_offset(P) * 4 + 256;
}

// The arguments of a call, in the order of the widest one (sg_embed_drop_bwd).  The plain
// calls have entry_offset 0 and seed 0; a forward has emb_out, a backward g_emb, grad_out
// and workspace.
struct NodesCall {
  const sg_model_t *model;
  const float *store_adj;
  const int32_t *store_types, *store_n;
  int32_t n_graphs, n_max;
  const int32_t *graph_idx;
  int64_t count, entry_offset;
  const float *params;
  uint64_t seed;
  float *emb_out;
  const float *g_emb;
  float *grad_out;
  int32_t *status_out;
  void *workspace;
  sg_stream_t stream;
};

// Checks in the order the headers document, then the launch (and, backward, the fixed-order
// sum of the slab rows into the node layers' range of grad_out).
int embed_nodes(NodesPlan kind, bool bwd, const NodesCall &c) {
  if (!c.model || c.count < 0 || c.entry_offset < 0) return SG_ERR_ARG;
  if (c.entry_offset & 1) return SG_ERR_ARG;   // a call starts at side 0 of a unit
  if (c.n_graphs <= 0 || c.n_max <= 0) return SG_ERR_ARG;
  SgGenPlan P;
  const int rc = nodes_plan(kind, c.model, &P);
  if (rc != SG_OK) return rc;
  if (c.n_max != P.n_max) return SG_ERR_ARG;   // the store's slots are the model's capacity
  if (bwd && !c.grad_out) return SG_ERR_ARG;
  const int hoff = head_offset(P);
  hipStream_t st = (hipStream_t)c.stream;
  if (c.count == 0) {
    if (!bwd) return SG_OK;
    return hipMemsetAsync(c.grad_out, 0, (size_t)hoff * 4u, st) == hipSuccess ? SG_OK : SG_ERR_HIP;
  }
  if (!c.store_adj || !c.store_types || !c.store_n || !c.params) return SG_ERR_ARG;
  if (bwd ? (!c.g_emb || !c.workspace) : !c.emb_out) return SG_ERR_ARG;
  const SgGenLaunch L = nodes_launch(P, bwd, c.count);
  if (!L.fits()) return SG_ERR_UNSUPPORTED;
  EmbedNodesArgs A;
  fill_store_args(A, P, c.store_adj, c.store_types, c.store_n, c.n_graphs, c.graph_idx, c.count,
                  c.status_out);
  A.key = sg_seed_key(c.seed);
  A.unit0 = c.entry_offset >> 1;
  A.hoff = hoff;
  A.params = c.params;
  A.out = c.emb_out;
  A.g_emb = c.g_emb;
  A.slab = (float *)c.workspace;
  const bool mask = kind == kDropout;
  void (*kernel)(SgGenPlan, EmbedNodesArgs) =
      bwd ? (mask ? sg_embed_nodes_kernel<true, true> : sg_embed_nodes_kernel<true, false>)
          : (mask ? sg_embed_nodes_kernel<false, true> : sg_embed_nodes_kernel<false, false>);
  sg_allow_lds((const void *)kernel, L.lds_bytes);
  hipLaunchKernelGGL(kernel, dim3(L.blocks), dim3(64 * L.waves_per_block), L.lds_bytes, st, P, A);
  if (bwd)
    hipLaunchKernelGGL(sg_sum_rows, dim3((unsigned)((hoff + 255) / 256)), dim3(256), 0, st,
                       (const float *)A.slab, (int64_t)L.blocks, (int64_t)hoff, c.grad_out);
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

}  // namespace

extern "C" {

int32_t sg_embed_dim(const sg_model_t *model) {
  SgGenPlan P;
  if (embed_plan(model, &P) != SG_OK) return -1;
  return plan_embed_dim(P);
}

int32_t sg_embed(const sg_model_t *model, const float *store_adj, const int32_t *store_types,
                 const int32_t *store_n, int32_t n_graphs, int32_t n_max,
                 const int32_t *graph_idx, int64_t count, const float *params,
                 float *emb_out, int32_t *status_out, sg_stream_t stream) {
  return embed_nodes(kInference, false,
                     {model, store_adj, store_types, store_n, n_graphs, n_max, graph_idx, count,
                      0, params, 0, emb_out, nullptr, nullptr, status_out, nullptr, stream});
}

int64_t sg_embed_bwd_workspace_bytes(const sg_model_t *model, int64_t count) {
  return nodes_bwd_workspace_bytes(kTrain, model, count);
}

int32_t sg_embed_bwd(const sg_model_t *model, const float *store_adj,
                     const int32_t *store_types, const int32_t *store_n, int32_t n_graphs,
                     int32_t n_max, const int32_t *graph_idx, int64_t count,
                     const float *params, const float *g_emb, float *grad_out,
                     int32_t *status_out, void *workspace, sg_stream_t stream) {
  return embed_nodes(kTrain, true,
                     {model, store_adj, store_types, store_n, n_graphs, n_max, graph_idx, count,
                      0, params, 0, nullptr, g_emb, grad_out, status_out, workspace, stream});
}

int32_t sg_embed_drop(const sg_model_t *model, const float *store_adj,
                      const int32_t *store_types, const int32_t *store_n, int32_t n_graphs,
                      int32_t n_max, const int32_t *graph_idx, int64_t count,
                      int64_t entry_offset, const float *params, uint64_t seed, float *emb_out,
                      int32_t *status_out, sg_stream_t stream) {
  return embed_nodes(kDropout, false,
                     {model, store_adj, store_types, store_n, n_graphs, n_max, graph_idx, count,
                      entry_offset, params, seed, emb_out, nullptr, nullptr, status_out, nullptr,
                      stream});
}

int64_t sg_embed_drop_bwd_workspace_bytes(const sg_model_t *model, int64_t count) {
  return nodes_bwd_workspace_bytes(kDropout, model, count);
}

int32_t sg_embed_drop_bwd(const sg_model_t *model, const float *store_adj,
                          const int32_t *store_types, const int32_t *store_n, int32_t n_graphs,
                          int32_t n_max, const int32_t *graph_idx, int64_t count,
                          int64_t entry_offset, const float *params, uint64_t seed,
                          const float *g_emb, float *grad_out, int32_t *status_out,
                          void *workspace, sg_stream_t stream) {
  return embed_nodes(kDropout, true,
                     {model, store_adj, store_types, store_n, n_graphs, n_max, graph_idx, count,
                      entry_offset, params, seed, nullptr, g_emb, grad_out, status_out, workspace,
                      stream});
}

}  // extern "C"
