// sg_embed_drop.hip — embed-once training with dropout (include/siamese_embed_drop.h): the
// node stack of single graphs, forward and backward, under graph-keyed dropout masks.
//
// The reference draws its masks per pair (layers.py:334-336, tf.nn.dropout; quirk A4); here
// entry c' = entry_offset + c of a call is side c' & 1 of unit c' >> 1 and draws the masks
// the generic pair kernel (sg_generic.hip) draws for that pair and side: the node layers'
// through gen_forward_nodes / gen_backward_nodes under the unit's key, and the mask the NTN
// head puts on its input vector (sg_generic.hip: x12 in the forward, the gradient of e0 / e1
// in the backward), which is a per-side operation on the embedding and so folds into the
// forward's output row and the backward's seed.  The grid kernels then run unchanged on the
// masked embeddings, with keep_prob 1.
// The kernels are sg_embed_kernel (sg_embed.hip) and sg_embed_bwd_kernel (sg_embed_train.hip)
// with a key and the head mask; they are kept apart so that those two compile as before.
#include "../../include/siamese_embed_drop.h"
#include "sg_embed_bwd.h"

namespace {

struct EmbedDropArgs : StoreArgs {
  uint32_t key;      // sg_seed_key(seed)
  int64_t unit0;     // entry_offset / 2: the global number of the call's unit 0
  const float *params;
  float *out;
};

// the head-input mask of element e of side s (sg_generic.hip, x12): thr 65536 keeps all
__device__ __forceinline__ float head_masked(const SgGenPlan &P, uint32_t pk, int s, int e,
                                             float v) {
  return sg_keep(pk, P.head_li, s, e, P.head_thr) ? v * P.head_inv_keep : 0.f;
}

// ---------------------------------------------------------------------------
// Forward: sg_embed_kernel's staging; the masks of unit unit0 + q; each side's row goes out
// through the head mask.  A side that cannot be embedded runs the other side's graph under
// its own side index; nothing of it is written but zeros.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) sg_embed_drop_kernel(SgGenPlan P, EmbedDropArgs A) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  float *S = smem + wave * P.wave_floats;
  const SgGenLayer &last = P.L[P.nl - 1];
  const int E = last.Rout * last.dout;
  const int64_t npair = (A.count + 1) >> 1;
  for (int64_t q = (int64_t)blockIdx.x * nw + wave; q < npair; q += (int64_t)gridDim.x * nw) {
    int g[2], n[2];
    bool ok[2], have[2];
    float *adj;
    int *types;
    const bool run = stage_graph_pair(P, A, S, q, lane, g, n, ok, have, adj, types);
    float *o0 = A.out + (size_t)(2 * q) * E, *o1 = o0 + E;
    if (!run) {
      for (int e = lane; e < E; e += SG_WAVE) {
        o0[e] = 0.f;
        if (have[1]) o1[e] = 0.f;
      }
      continue;
    }
    const uint32_t pk = sg_pair_key(A.key, (uint32_t)(A.unit0 + q));
    gen_forward_nodes(P, S, A.params, adj, types, n[0], n[1], pk, lane);
    const float *e0 = S + last.l_out;
    for (int e = lane; e < E; e += SG_WAVE) {
      o0[e] = ok[0] ? head_masked(P, pk, 0, e, e0[e]) : 0.f;
      if (have[1]) o1[e] = ok[1] ? head_masked(P, pk, 1, e, e0[E + e]) : 0.f;
    }
    sg_wsync();   // the next graphs overwrite the slice
  }
}

// ---------------------------------------------------------------------------
// Backward: sg_embed_bwd_kernel's slab per workgroup; the same masked forward, the seed is
// g_emb through the head mask (g_emb is the gradient of the masked embedding), then
// gen_backward_nodes under the unit's key.  A substituted side has a zero seed.
// ---------------------------------------------------------------------------
struct EmbedDropBwdArgs : StoreArgs {
  uint32_t key;
  int64_t unit0;
  int hoff;
  const float *params, *g_emb;
  float *slab;   // [gridDim.x][hoff]
};

__global__ void __launch_bounds__(256) sg_embed_drop_bwd_kernel(SgGenPlan P, EmbedDropBwdArgs A) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int gfl = (A.hoff + 3) & ~3;
  float *G = smem;
  float *S = smem + gfl + wave * P.wave_floats;
  for (int i = threadIdx.x; i < gfl; i += blockDim.x) G[i] = 0.f;
  __syncthreads();
  const SgGenLayer &last = P.L[P.nl - 1];
  const int E = last.Rout * last.dout;
  const int64_t npair = (A.count + 1) >> 1;
  for (int64_t q = (int64_t)blockIdx.x * nw + wave; q < npair; q += (int64_t)gridDim.x * nw) {
    int g[2], n[2];
    bool ok[2], have[2];
    float *adj;
    int *types;
    if (!stage_graph_pair(P, A, S, q, lane, g, n, ok, have, adj, types)) continue;
    const uint32_t pk = sg_pair_key(A.key, (uint32_t)(A.unit0 + q));
    gen_forward_nodes(P, S, A.params, adj, types, n[0], n[1], pk, lane);
    float *gcur = S + P.l_g0, *gnext = S + P.l_g1;
    const float *ge = A.g_emb + (size_t)(2 * q) * E;
    for (int e = lane; e < E; e += SG_WAVE) {
      gcur[e] = ok[0] ? head_masked(P, pk, 0, e, ge[e]) : 0.f;
      gcur[E + e] = ok[1] ? head_masked(P, pk, 1, e, ge[E + e]) : 0.f;
    }
    sg_wsync();
    gen_backward_nodes(P, S, G, A.params, adj, types, n[0], n[1], pk, lane, gcur, gnext);
    sg_wsync();   // the next graphs overwrite the slice
  }
  __syncthreads();
  float *dst = A.slab + (size_t)blockIdx.x * (size_t)A.hoff;
  for (int i = threadIdx.x; i < A.hoff; i += blockDim.x) dst[i] = G[i];
}

// what both calls check alike, in the order the header documents
int drop_args(const sg_model_t *model, int64_t count, int64_t entry_offset, int32_t n_graphs,
              int32_t n_max, SgGenPlan *P) {
  if (!model || count < 0 || entry_offset < 0) return SG_ERR_ARG;
  if (entry_offset & 1) return SG_ERR_ARG;   // a call starts at side 0 of a unit
  if (n_graphs <= 0 || n_max <= 0) return SG_ERR_ARG;
  const int rc = embed_drop_plan(model, P);
  if (rc != SG_OK) return rc;
  if (n_max != P->n_max) return SG_ERR_ARG;   // the store's slots are the model's capacity
  return SG_OK;
}

}  // namespace

extern "C" {

int32_t sg_embed_drop(const sg_model_t *model, const float *store_adj,
                      const int32_t *store_types, const int32_t *store_n, int32_t n_graphs,
                      int32_t n_max, const int32_t *graph_idx, int64_t count,
                      int64_t entry_offset, const float *params, uint64_t seed, float *emb_out,
                      int32_t *status_out, sg_stream_t stream) {
  SgGenPlan P;
  const int rc = drop_args(model, count, entry_offset, n_graphs, n_max, &P);
  if (rc != SG_OK) return rc;
  if (count == 0) return SG_OK;
  if (!store_adj || !store_types || !store_n || !params || !emb_out) return SG_ERR_ARG;
  // sg_embed's shape: no accumulator, one unit per two entries
  const SgGenLaunch L = sg_gen_launch_shape(P, 0, (count + 1) / 2);
  if (!L.fits()) return SG_ERR_UNSUPPORTED;
  EmbedDropArgs A;
  fill_store_args(A, P, store_adj, store_types, store_n, n_graphs, graph_idx, count, status_out);
  A.key = sg_seed_key(seed);
  A.unit0 = entry_offset >> 1;
  A.params = params;
  A.out = emb_out;
  sg_allow_lds((const void *)sg_embed_drop_kernel, L.lds_bytes);
  hipLaunchKernelGGL(sg_embed_drop_kernel, dim3(L.blocks), dim3(64 * L.waves_per_block),
                     L.lds_bytes, (hipStream_t)stream, P, A);
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

int64_t sg_embed_drop_bwd_workspace_bytes(const sg_model_t *model, int64_t count) {
  SgGenPlan P;
  if (count < 0 || embed_drop_plan(model, &P) != SG_OK) return -1;
  const SgGenLaunch L = embed_bwd_launch(P, count);
  if (!L.fits()) return -1;
  return (int64_t)L.blocks * head_offset(P) * 4 + 256;
}

int32_t sg_embed_drop_bwd(const sg_model_t *model, const float *store_adj,
                          const int32_t *store_types, const int32_t *store_n, int32_t n_graphs,
                          int32_t n_max, const int32_t *graph_idx, int64_t count,
                          int64_t entry_offset, const float *params, uint64_t seed,
                          const float *g_emb, float *grad_out, int32_t *status_out,
                          void *workspace, sg_stream_t stream) {
  SgGenPlan P;
  const int rc = drop_args(model, count, entry_offset, n_graphs, n_max, &P);
  if (rc != SG_OK) return rc;
  if (!grad_out) return SG_ERR_ARG;
  const int hoff = head_offset(P);
  hipStream_t st = (hipStream_t)stream;
  if (count == 0)
    return hipMemsetAsync(grad_out, 0, (size_t)hoff * 4u, st) == hipSuccess ? SG_OK : SG_ERR_HIP;
  if (!store_adj || !store_types || !store_n || !params || !g_emb || !workspace)
    return SG_ERR_ARG;
  const SgGenLaunch L = embed_bwd_launch(P, count);
  if (!L.fits()) return SG_ERR_UNSUPPORTED;
  EmbedDropBwdArgs A;
  fill_store_args(A, P, store_adj, store_types, store_n, n_graphs, graph_idx, count, status_out);
  A.key = sg_seed_key(seed);
  A.unit0 = entry_offset >> 1;
  A.hoff = hoff;
  A.params = params;
  A.g_emb = g_emb;
  A.slab = (float *)workspace;
  sg_allow_lds((const void *)sg_embed_drop_bwd_kernel, L.lds_bytes);
  hipLaunchKernelGGL(sg_embed_drop_bwd_kernel, dim3(L.blocks), dim3(64 * L.waves_per_block),
                     L.lds_bytes, st, P, A);
  hipLaunchKernelGGL(sg_sum_rows, dim3((unsigned)((hoff + 255) / 256)), dim3(256), 0, st,
                     (const float *)A.slab, (int64_t)L.blocks, (int64_t)hoff, grad_out);
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

}  // extern "C"
