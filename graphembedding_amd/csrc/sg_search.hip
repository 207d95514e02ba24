// sg_search.hip — embed-once search (include/siamese_search.h): the NTN score grid of
// sg_embed.hip fused with a per-query running top-k, so the m x n scores never reach
// memory.  The arithmetic of one score is sg_grid_kernel's, operation for operation (the
// contract is bitwise equality with sg_score_grid + sg_topk_rows); what differs is what
// happens to a score: it becomes a topk_key and meets the query's current k-th best.
#include "../../include/siamese_search.h"
#include "sg_embed_plan.h"
#include "sg_mfma.h"
#include "sg_search_lists.h"

namespace {

using sgk::f4;

// ---------------------------------------------------------------------------
// How a call is cut (search_split, sg_search_split.h) and its workspace
// [Q tables | candidate keys | candidate values].
// ---------------------------------------------------------------------------
struct SearchPlan : SearchSplit {
  int64_t q_bytes, ws_bytes;
  size_t lds;
};

// Every host check that needs no pointer; the SG_ERR_* order is sg_score_grid's, then
// search_split's.
int search_plan(const sg_model_t *model, int64_t m, int64_t n, int32_t k, int64_t seg_cols,
                SgGenPlan *P, SearchPlan *S) {
  if (!model || m < 0 || n < 0) return SG_ERR_ARG;
  int rc = grid_plan(model, P);
  if (rc != SG_OK) return rc;
  // 8 workgroups per CU fill the device; 32768 B of LDS for the lists of a workgroup's queries
  rc = search_split(SearchUnit{(int64_t)sg_num_cus() * 8, 4, 32768}, m, n, k, seg_cols, S);
  if (rc != SG_OK) return rc;
  S->lds = (size_t)S->qb * k * kListBytes;
  S->q_bytes = (m * grid_dp(*P) * 16 * 4 + 255) & ~(int64_t)255;
  S->ws_bytes = S->q_bytes + S->cand_bytes;
  return SG_OK;
}

// The running top-k list of a query, its write-out and the merge of the segments' candidate
// lists are shared with sg_web_search.hip and sg_dot_grid.hip: sg_search_lists.h.

// ---------------------------------------------------------------------------
// A workgroup owns one segment of the database and one chunk of qb queries.  As in
// sg_grid_kernel each of its four wavefronts keeps the augmented rows of a 64-column block
// as MFMA A operands and walks every fourth query of the chunk, so per (query, block) the
// operand traffic is the grid's: NS coalesced 256-B loads of Q_i.  (Keeping Q_i and
// streaming the blocks instead would gather 4 NS A-operand dwords per lane per (query,
// block) through the texture path, four times the loads for the same MFMAs.)  The lists of
// a wavefront's queries are its own LDS: no workgroup barrier anywhere.
// Lane (g, c) ends a block with the score of column j0 + 16 (c >> 2) + 4 g + (c & 3).
// ---------------------------------------------------------------------------
struct SearchArgs : GridCommon {   // ncb counts segments here
  int64_t seg;
  int apply_final, k, largest;
  ListOut out;
};

template <int NS>
__global__ void __launch_bounds__(256) sg_search_kernel(SearchArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, c = lane & 15, k = A.k;
  const int64_t sgm = (int64_t)blockIdx.x % A.ncb, qc = (int64_t)blockIdx.x / A.ncb;
  const int64_t q0 = qc * A.qb;
  const int64_t q1 = q0 + A.qb < A.m ? q0 + A.qb : A.m;
  const int64_t c0 = sgm * A.seg;
  const int64_t c1 = c0 + A.seg < A.n ? c0 + A.seg : A.n;
  uint64_t *lkeys = (uint64_t *)smem;                 // [qb][k]
  float *lvals = (float *)(lkeys + (size_t)A.qb * k);   // [qb][k]
  for (int64_t i = q0 + wave; i < q1; i += 4) list_reset(lkeys + (i - q0) * k, k, lane);
  sg_wsync();
  const float usum = grid_usum(A);
  const GridCol col = grid_col(A, c, usum);   // column k = c of C
  const bool kmask = col.mask;
  const float wk = col.w;
  const int jl = 16 * (c >> 2) + 4 * g + (c & 3);
  for (int64_t j0 = c0; j0 < c1; j0 += 64) {
    float a[4][NS];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int s = 0; s < NS; ++s) a[t][s] = grid_aug(A, j0 + 16 * t + c, 4 * s + g);
    const int64_t jst = j0 + jl;   // the column whose score this lane ends up with
    for (int64_t i = q0 + wave; i < q1; i += 4) {
      float b[NS];
      grid_load_q<NS>(A, i, lane, b);
      uint64_t *lk = lkeys + (i - q0) * k;
      const uint64_t thr = lk[k - 1];
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
      const uint64_t key = jst < A.n ? topk_key(s, (uint32_t)jst, A.largest) : ~0ull;
      list_offer(lk, lvals + (i - q0) * k, k, lane, key, s, thr);
    }
  }
  for (int64_t i = q0 + wave; i < q1; i += 4) {
    if (lane >= k) continue;
    const uint64_t key = lkeys[(i - q0) * k + lane];
    const float val = lvals[(i - q0) * k + lane];
    if (A.ncb == 1) {   // k <= n: every entry is a column
      A.out.idx[i * k + lane] = (int32_t)(uint32_t)key;
      if (A.out.val) A.out.val[i * k + lane] = val;
    } else {   // a short last segment leaves sentinels; their values are never read
      const int64_t o = (sgm * A.m + i) * k + lane;
      A.out.ckey[o] = key;
      A.out.cval[o] = val;
    }
  }
}

}  // namespace

extern "C" {

int64_t sg_search_topk_workspace_bytes(const sg_model_t *model, int64_t m, int64_t n,
                                       int32_t k, int64_t seg_cols) {
  SgGenPlan P;
  SearchPlan S;
  if (search_plan(model, m, n, k, seg_cols, &P, &S) != SG_OK) return -1;
  return S.ws_bytes;
}

int32_t sg_search_topk(const sg_model_t *model, const float *emb_q, const float *emb_db,
                       int64_t m, int64_t n, const float *params, int32_t apply_final,
                       int32_t k, int32_t largest, int64_t seg_cols, int32_t *idx_out,
                       float *val_out, void *workspace, sg_stream_t stream) {
  SgGenPlan P;
  SearchPlan S;
  const int rc = search_plan(model, m, n, k, seg_cols, &P, &S);
  if (rc != SG_OK) return rc;
  if (m == 0) return SG_OK;
  if (!emb_q || !emb_db || !params || !idx_out || !workspace) return SG_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  float *Q = (float *)workspace;
  launch_grid_q(P, emb_q, m, params, Q, st);
  GridSplit split;
  split.ncb = S.nseg;
  split.nqc = S.nqc;
  split.qb = S.qb;
  split.blocks = S.blocks;
  SearchArgs A;
  fill_grid_common(A, P, Q, emb_db, params, m, n, split);
  A.seg = S.seg;
  A.apply_final = apply_final ? 1 : 0;
  A.k = k;
  A.largest = largest ? 1 : 0;
  A.out = list_out((char *)workspace + S.q_bytes, S, idx_out, val_out);
  grid_dispatch_ns(grid_dp(P) / 4, [&](auto ns) {
    hipLaunchKernelGGL(sg_search_kernel<decltype(ns)::value>, dim3((unsigned)S.blocks),
                       dim3(256), S.lds, st, A);
  });
  launch_search_merge(A.out, S, m, k, st);
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

}  // extern "C"
