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

constexpr int64_t kSegMin = 1024;       // the library's own segment choice lies in
constexpr int64_t kSegMax = 65536;      // [kSegMin, kSegMax] columns
constexpr int kListLds = 32768;         // LDS for the lists of a workgroup's queries

// ---------------------------------------------------------------------------
// How a call is cut: S segments of seg database columns times nqc chunks of qb queries, one
// workgroup each, and the workspace [Q tables | candidate keys | candidate values].
// ---------------------------------------------------------------------------
struct SearchPlan {
  int64_t seg, nseg, nqc, qb, blocks;
  int64_t q_bytes, cand, ws_bytes;   // cand: candidate entries, nseg · m · k
  size_t lds;
};

// Every host check that needs no pointer; the SG_ERR_* order is sg_score_grid's, then
// sg_topk_rows', then seg_cols.
int search_plan(const sg_model_t *model, int64_t m, int64_t n, int32_t k, int64_t seg_cols,
                SgGenPlan *P, SearchPlan *S) {
  if (!model || m < 0 || n < 0) return SG_ERR_ARG;
  const int rc = grid_plan(model, P);
  if (rc != SG_OK) return rc;
  if (k < 1) return SG_ERR_ARG;
  if (k > kTopkMax) return SG_ERR_UNSUPPORTED;
  if (k > n) return SG_ERR_ARG;
  if (seg_cols < 0 || (seg_cols & 63) != 0) return SG_ERR_ARG;
  if (m > kMaxRows || n > kMaxRows) return SG_ERR_UNSUPPORTED;   // n < 2^31 with it
  const int64_t target = (int64_t)sg_num_cus() * 8;   // workgroups that fill the device
  const int64_t max_qc = m > 4 ? (m + 3) / 4 : 1;
  int64_t seg = seg_cols;
  if (seg == 0) {
    // a list costs about k (1 + ln(seg / k)) insertions per segment and k rounds over
    // its k candidates in the merge: segments of 1024 columns per list entry (at least
    // 4096) amortise both, shorter ones only where the queries alone cannot fill the device
    seg = 4096;
    while (seg < 1024 * (int64_t)k) seg <<= 1;   // k <= 64: at most kSegMax
    while (seg > kSegMin && ((n + seg - 1) / seg) * max_qc < target) seg >>= 1;
  }
  if (seg > n) seg = (n + 63) & ~(int64_t)63;   // one segment (k <= n: n >= 1)
  S->seg = seg;
  S->nseg = (n + seg - 1) / seg;
  // query chunks as grid_split cuts them: enough to reach the target, else as many
  // queries as possible per load of the database tiles, within the LDS of the lists
  int64_t nqc = (target + S->nseg - 1) / S->nseg;
  nqc = nqc > max_qc ? max_qc : nqc;
  int64_t qb = (((m + nqc - 1) / nqc) + 3) & ~(int64_t)3;
  const int64_t qb_cap = (kListLds / (kListBytes * k)) & ~3;   // >= 40
  qb = qb > qb_cap ? qb_cap : qb;
  qb = qb < 4 ? 4 : qb;
  S->qb = qb;
  S->nqc = m > 0 ? (m + qb - 1) / qb : 1;
  S->blocks = S->nseg * S->nqc;
  if (S->blocks > 0x7FFFFFFF) return SG_ERR_UNSUPPORTED;
  S->lds = (size_t)qb * k * kListBytes;
  S->q_bytes = (m * grid_dp(*P) * 16 * 4 + 255) & ~(int64_t)255;
  S->cand = S->nseg * m * k;
  // the library's own choice depends on m and on the device: its workspace is sized for
  // the shortest segments it may pick, so the size is monotone and the same everywhere
  const int64_t ws_seg = seg_cols == 0 ? (n + kSegMin - 1) / kSegMin : S->nseg;
  S->ws_bytes = S->q_bytes + ws_seg * m * k * kListBytes + 256;
  return SG_OK;
}

// The running top-k list of a query (list_insert) and the merge of the segments' candidate
// lists (sg_search_merge_kernel) are shared with sg_web_search.hip: sg_search_lists.h.

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
  uint64_t *ckey;   // candidates [nseg][m][k], or
  float *cval;
  int32_t *idx;     // with one segment the results themselves [m][k]
  float *val;       // (may be null)
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
  for (int64_t i = q0 + wave; i < q1; i += 4)
    if (lane < k) lkeys[(i - q0) * k + lane] = ~0ull;
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
      const uint64_t hits = __ballot(key < thr);
      if (hits) {
        list_insert(lk, lvals + (i - q0) * k, k, lane, key, s, hits, thr);
        sg_wsync();
      }
    }
  }
  for (int64_t i = q0 + wave; i < q1; i += 4) {
    if (lane >= k) continue;
    const uint64_t key = lkeys[(i - q0) * k + lane];
    const float val = lvals[(i - q0) * k + lane];
    if (A.ncb == 1) {   // k <= n: every entry is a column
      A.idx[i * k + lane] = (int32_t)(uint32_t)key;
      if (A.val) A.val[i * k + lane] = val;
    } else {   // a short last segment leaves sentinels; their values are never read
      const int64_t o = (sgm * A.m + i) * k + lane;
      A.ckey[o] = key;
      A.cval[o] = val;
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
  A.ckey = (uint64_t *)((char *)workspace + S.q_bytes);
  A.cval = (float *)(A.ckey + S.cand);
  A.idx = idx_out;
  A.val = val_out;
  grid_dispatch_ns(grid_dp(P) / 4, [&](auto ns) {
    hipLaunchKernelGGL(sg_search_kernel<decltype(ns)::value>, dim3((unsigned)S.blocks),
                       dim3(256), S.lds, st, A);
  });
  if (S.nseg > 1)
    hipLaunchKernelGGL(sg_search_merge_kernel, dim3((unsigned)m), dim3(64), 0, st, A.ckey,
                       A.cval, m, (int)S.nseg, (int)k, idx_out, val_out);
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

}  // extern "C"
