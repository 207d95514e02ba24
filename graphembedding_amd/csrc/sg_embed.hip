// sg_embed.hip — embed-once retrieval (include/siamese_embed.h): graph-level embeddings
// from the generic node stack, the NTN score grid as a batched small-k GEMM on
// v_mfma_f32_16x16x4_f32, and per-row top-k selection.
//
// The NTN head (layers.py:282-310) of (query i as graph 1, database j as graph 2) is
//   m_k = e_i^T W[:,:,k] e_j + V[k] · [e_i, e_j] + bias[k]  =  [e_j, 1] · Q_i[:, k]
// with the per-query table  Q_i[b][k] = Σ_a e_i[a] W[a][b][k] + V[k][D + b]  (b < D) and
// Q_i[D][k] = Σ_a V[k][a] e_i[a] + bias[k]: 2 (D + 1) K FLOP per pair after O(m + n) work.
// Inference mode: no dropout anywhere (the header states the deviation, quirk A4).
#include "../../include/siamese_embed.h"
#include "sg_gen_nodes.h"
#include "sg_mfma.h"
#include "sg_paths.h"

namespace {

using sgk::f4;

constexpr int kTopkMax = 64;

// ---------------------------------------------------------------------------
// Embeddings: one wavefront runs gen_forward_nodes on two graphs (the two "sides" of the
// generic kernel's LDS slice).  A graph that cannot be embedded (bad id, bad node count)
// or the missing partner of an odd tail is replaced by the other side's graph for the
// computation (never n = 0: Average divides by the row count) and is not written / zeroed.
// ---------------------------------------------------------------------------
struct EmbedArgs {
  const float *sadj;
  const int32_t *stypes, *sn;
  int n_graphs, max_nodes;
  const int32_t *gidx;
  int64_t count;
  const float *params;
  float *out;
  int32_t *status;
};

__global__ void __launch_bounds__(256) sg_embed_kernel(SgGenPlan P, EmbedArgs A) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  float *S = smem + wave * P.wave_floats;
  const int nmax = P.n_max, nn = nmax * nmax;
  const SgGenLayer &last = P.L[P.nl - 1];
  const int E = last.Rout * last.dout;
  const int64_t npair = (A.count + 1) >> 1;
  for (int64_t q = (int64_t)blockIdx.x * nw + wave; q < npair; q += (int64_t)gridDim.x * nw) {
    int g[2], n[2];
    bool ok[2], have[2];
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
    float *o0 = A.out + (size_t)(2 * q) * E, *o1 = o0 + E;
    if (!ok[0] && !ok[1]) {
      for (int e = lane; e < E; e += SG_WAVE) {
        o0[e] = 0.f;
        if (have[1]) o1[e] = 0.f;
      }
      continue;
    }
    if (!ok[0]) { g[0] = g[1]; n[0] = n[1]; }
    if (!ok[1]) { g[1] = g[0]; n[1] = n[0]; }
    // stage Â and the node types of the two graphs in the pair-record layout
    float *adj = S + P.l_rec;
    int *types = (int *)(S + P.l_rec + P.rec_types);
    for (int w = lane; w < 2 * nn; w += SG_WAVE) {
      const int s = w / nn, o = w - s * nn;
      adj[w] = A.sadj[(size_t)g[s] * nn + o];
    }
    for (int w = lane; w < 2 * nmax; w += SG_WAVE) {
      const int s = w / nmax, o = w - s * nmax;
      types[w] = A.stypes[(size_t)g[s] * nmax + o];
    }
    sg_wsync();
    gen_forward_nodes(P, S, A.params, adj, types, n[0], n[1], 0u, lane);
    const float *e0 = S + last.l_out;
    for (int e = lane; e < E; e += SG_WAVE) {
      o0[e] = ok[0] ? e0[e] : 0.f;
      if (have[1]) o1[e] = ok[1] ? e0[E + e] : 0.f;
    }
    sg_wsync();   // the next graphs overwrite the slice
  }
}

}  // namespace

// embed_plan, grid_plan, grid_dp and the query tables' sg_grid_q_kernel, shared with
// sg_embed_train.hip.  Included here, between the embedding kernel and the grid kernel,
// where the table kernel was defined: the unit's code object keeps its function order.
#include "sg_embed_plan.h"

namespace {

// ---------------------------------------------------------------------------
// Score grid over the tables Q [m][Dp][16].  A workgroup owns 64 database rows (four
// 16-row tiles) and a range of
// queries; each of its four wavefronts keeps the augmented rows [e_j, 1, 0…] of the four
// tiles as MFMA A operands in NS = Dp / 4 registers per tile (lane l: row l & 15, k-slot
// l >> 4) and walks every fourth query of the range.  Per query the B operand is Q_i
// (lane l: Q_i[4 s + (l >> 4)][l & 15], one coalesced 256-B load per k-step, L2-resident),
// C[16 j x 16 k] = A·B takes NS MFMAs per tile on four independent accumulators, and the
// head's sum over k is a DPP row sum (C: lane l register r = row 4 (l >> 4) + r, column
// l & 15).  Afterwards every lane of a 16-lane row holds the 16 scores of its four rows
// in the four tiles; lane (g, c) keeps tile c >> 2, register c & 3, so the wavefront
// stores the 64 scores of one row of `out` as one 256-B segment.
// ---------------------------------------------------------------------------
struct GridArgs {
  const float *Q, *edb, *U;
  int64_t m, n, ld, ncb;
  int D, K, qb;
  int act, ntn_mode, final_act, apply_final;
  float yeta;
  float *out;
};

template <int NS>
__global__ void __launch_bounds__(256) sg_grid_kernel(GridArgs A) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int64_t cb = (int64_t)blockIdx.x % A.ncb, qc = (int64_t)blockIdx.x / A.ncb;
  const int64_t j0 = cb * 64;
  const int D = A.D, K = A.K;
  float a[4][NS];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int64_t j = j0 + 16 * t + c;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int b = 4 * s + g;
      float v = 0.f;
      if (j < A.n) v = b < D ? A.edb[j * D + b] : (b == D ? 1.f : 0.f);
      a[t][s] = v;
    }
  }
  // column k = c of C: its weight (intended: U[k]; reference, quirk A1: 1, the sum is
  // scaled by ΣU) and its mask (act(0) of a padded column is not 0 for sigmoid)
  const bool kmask = c < K;
  float wk = 0.f, usum = 1.f;
  if (A.ntn_mode == SG_NTN_INTENDED) {
    if (kmask) wk = A.U[c];
  } else {
    wk = 1.f;
    usum = 0.f;
    for (int k = 0; k < K; ++k) usum += A.U[k];
  }
  const int64_t q1 = (qc + 1) * A.qb < A.m ? (qc + 1) * A.qb : A.m;
  const int64_t jst = j0 + 16 * (c >> 2) + 4 * g + (c & 3);   // the column this lane stores
  for (int64_t i = qc * A.qb + wave; i < q1; i += 4) {
    const float *__restrict__ Qi = A.Q + i * (NS * 64);
    float b[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) b[s] = Qi[s * 64 + lane];
    f4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = sgk::mfma4(a[t][s], b[s], acc[t]);
    float v[16];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[4 * t + r] = kmask ? sg_act(A.act, acc[t][r]) * wk : 0.f;
    sgk::row_sum16_n<16>(v);
    float s = v[0];
#pragma unroll
    for (int x = 1; x < 16; ++x) s = c == x ? v[x] : s;
    s *= usum;
    if (A.apply_final) s = sg_final(A.final_act, A.yeta, s);
    if (jst < A.n) A.out[i * A.ld + jst] = s;
  }
}

template <int NS>
void launch_grid(const GridArgs &A, int64_t blocks, hipStream_t st) {
  hipLaunchKernelGGL(sg_grid_kernel<NS>, dim3((unsigned)blocks), dim3(256), 0, st, A);
}

// ---------------------------------------------------------------------------
// Top-k of each row: one wavefront per row, k selection rounds.  Every element maps to a
// 64-bit key (rank of the value, column) whose unsigned order is the documented total
// order; a round scans the row for the smallest key strictly above the previous round's,
// then reduces over the wavefront.  The input is only read.
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

__global__ void __launch_bounds__(256) sg_topk_kernel(const float *__restrict__ vals, int64_t m,
                                                      int64_t n, int64_t ld, int k, int largest,
                                                      int32_t *__restrict__ idx,
                                                      float *__restrict__ vout) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= m) return;
  const float *__restrict__ v = vals + row * ld;
  uint64_t prev = 0;   // below every key
  for (int r = 0; r < k; ++r) {
    uint64_t best = ~0ull;   // above every key (columns are < 2^31)
    for (int64_t col = lane; col < n; col += SG_WAVE) {
      const uint64_t key = topk_key(v[col], (uint32_t)col, largest);
      if (key > prev && key < best) best = key;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint64_t other = __shfl_xor(best, o, 64);
      best = other < best ? other : best;
    }
    prev = best;
    if (lane == 0) {
      const uint32_t col = (uint32_t)best;   // k <= n: a candidate always exists
      idx[row * k + r] = (int32_t)col;
      if (vout) vout[row * k + r] = v[col];
    }
  }
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
  if (!model || count < 0 || n_graphs <= 0 || n_max <= 0) return SG_ERR_ARG;
  SgGenPlan P;
  const int rc = embed_plan(model, &P);
  if (rc != SG_OK) return rc;
  if (n_max != P.n_max) return SG_ERR_ARG;   // the store's slots are the model's capacity
  if (count == 0) return SG_OK;
  if (!store_adj || !store_types || !store_n || !params || !emb_out) return SG_ERR_ARG;
  // launch shape of the generic kernel's forward: up to 4 waves per workgroup within 80 KB
  const size_t wbytes = (size_t)P.wave_floats * 4u;
  int nw = 4;
  while (nw > 1 && nw * wbytes > 81920u) --nw;
  const size_t lds = nw * wbytes;
  if (lds > 163840u) return SG_ERR_UNSUPPORTED;
  EmbedArgs A;
  A.sadj = store_adj;
  A.stypes = store_types;
  A.sn = store_n;
  A.n_graphs = n_graphs;
  A.max_nodes = plan_max_nodes(P);
  A.gidx = graph_idx;
  A.count = count;
  A.params = params;
  A.out = emb_out;
  A.status = status_out;
  int per_cu = (int)(163840u / lds);
  per_cu = per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu);
  const int64_t want = ((count + 1) / 2 + nw - 1) / nw;
  const int64_t cap = (int64_t)sg_num_cus() * per_cu;
  const int blocks = (int)(want < cap ? want : cap);
  if (lds > 65536u)
    (void)hipFuncSetAttribute((const void *)sg_embed_kernel,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(sg_embed_kernel, dim3(blocks), dim3(64 * nw), lds, (hipStream_t)stream, P, A);
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

int64_t sg_score_grid_workspace_bytes(const sg_model_t *model, int64_t m) {
  SgGenPlan P;
  if (m < 0 || m > kMaxRows || grid_plan(model, &P) != SG_OK) return -1;
  return m * grid_dp(P) * 16 * 4 + 256;
}

int32_t sg_score_grid(const sg_model_t *model, const float *emb_q, const float *emb_db,
                      int64_t m, int64_t n, const float *params, int32_t apply_final,
                      float *out, int64_t ld_out, void *workspace, sg_stream_t stream) {
  if (!model || m < 0 || n < 0) return SG_ERR_ARG;
  SgGenPlan P;
  const int rc = grid_plan(model, &P);
  if (rc != SG_OK) return rc;
  if (m > kMaxRows || n > kMaxRows) return SG_ERR_UNSUPPORTED;
  if (m == 0 || n == 0) return SG_OK;
  if (!emb_q || !emb_db || !params || !out || !workspace || ld_out < n) return SG_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int Dp = grid_dp(P);
  float *Q = (float *)workspace;
  const int64_t qelems = m * Dp * 16;
  hipLaunchKernelGGL(sg_grid_q_kernel, dim3((unsigned)((qelems + 255) / 256)), dim3(256), 0, st,
                     emb_q, m, P.D, P.K, Dp, params, P.offW, P.offV, P.offB, Q);
  GridArgs A;
  A.Q = Q;
  A.edb = emb_db;
  A.U = params + P.offU;
  A.m = m;
  A.n = n;
  A.ld = ld_out;
  A.ncb = (n + 63) / 64;
  A.D = P.D;
  A.K = P.K;
  A.act = P.head_act;
  A.ntn_mode = P.ntn_mode;
  A.final_act = P.final_act;
  A.apply_final = apply_final ? 1 : 0;
  A.yeta = P.yeta;
  A.out = out;
  // queries per workgroup (a multiple of its 4 wavefronts): enough workgroups to fill the
  // device, else as many queries as possible per load of the database tiles
  const int64_t target = (int64_t)sg_num_cus() * 8;
  int64_t nqc = (target + A.ncb - 1) / A.ncb;
  const int64_t max_qc = (m + 3) / 4;
  nqc = nqc > max_qc ? max_qc : nqc;
  const int64_t qb = (((m + nqc - 1) / nqc) + 3) & ~(int64_t)3;
  nqc = (m + qb - 1) / qb;
  A.qb = (int)qb;
  const int64_t blocks = A.ncb * nqc;
  if (blocks > 0x7FFFFFFF) return SG_ERR_UNSUPPORTED;
  switch (Dp / 4) {
    case 1: launch_grid<1>(A, blocks, st); break;
    case 2: launch_grid<2>(A, blocks, st); break;
    case 3: launch_grid<3>(A, blocks, st); break;
    case 4: launch_grid<4>(A, blocks, st); break;
    case 5: launch_grid<5>(A, blocks, st); break;
    case 6: launch_grid<6>(A, blocks, st); break;
    case 7: launch_grid<7>(A, blocks, st); break;
    default: launch_grid<8>(A, blocks, st); break;
  }
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

int32_t sg_topk_rows(const float *vals, int64_t m, int64_t n, int64_t ld, int32_t k,
                     int32_t largest, int32_t *idx_out, float *val_out, sg_stream_t stream) {
  if (m < 0 || n < 0 || k < 1) return SG_ERR_ARG;
  if (k > kTopkMax) return SG_ERR_UNSUPPORTED;
  if (k > n || ld < n || n > 0x7FFFFFFF || m > 0x7FFFFFFF) return SG_ERR_ARG;
  if (m == 0) return SG_OK;
  if (!vals || !idx_out) return SG_ERR_ARG;
  hipLaunchKernelGGL(sg_topk_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0,
                     (hipStream_t)stream, vals, m, n, ld, k, largest ? 1 : 0, idx_out, val_out);
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

}  // extern "C"
