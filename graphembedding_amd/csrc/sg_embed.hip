// sg_embed.hip — embed-once retrieval (include/siamese_embed.h): the NTN score grid over
// graph-level embeddings (sg_embed: sg_embed_nodes.hip) as a batched small-k GEMM on
// v_mfma_f32_16x16x4_f32, and per-row top-k selection.
//
// The NTN head (layers.py:282-310) of (query i as graph 1, database j as graph 2) is
//   m_k = e_i^T W[:,:,k] e_j + V[k] · [e_i, e_j] + bias[k]  =  [e_j, 1] · Q_i[:, k]
// with the per-query table  Q_i[b][k] = Σ_a e_i[a] W[a][b][k] + V[k][D + b]  (b < D) and
// Q_i[D][k] = Σ_a V[k][a] e_i[a] + bias[k]: 2 (D + 1) K FLOP per pair after O(m + n) work.
// Inference mode: no dropout anywhere (the header states the deviation, quirk A4).
#include "../../include/siamese_embed.h"
#include "sg_embed_plan.h"
#include "sg_mfma.h"

namespace {

using sgk::f4;

constexpr int kTopkMax = 64;

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
struct GridArgs : GridCommon {
  int64_t ld;
  int apply_final;
  float *out;
};

template <int NS>
__global__ void __launch_bounds__(256) sg_grid_kernel(GridArgs A) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int64_t cb = (int64_t)blockIdx.x % A.ncb, qc = (int64_t)blockIdx.x / A.ncb;
  const int64_t j0 = cb * 64;
  float a[4][NS];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int s = 0; s < NS; ++s) a[t][s] = grid_aug(A, j0 + 16 * t + c, 4 * s + g);
  const float usum = grid_usum(A);
  const GridCol col = grid_col(A, c, usum);   // column k = c of C
  const bool kmask = col.mask;
  const float wk = col.w;
  const int64_t q1 = (qc + 1) * A.qb < A.m ? (qc + 1) * A.qb : A.m;
  const int64_t jst = j0 + 16 * (c >> 2) + 4 * g + (c & 3);   // the column this lane stores
  for (int64_t i = qc * A.qb + wave; i < q1; i += 4) {
    float b[NS];
    grid_load_q<NS>(A, i, lane, b);
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

// ---------------------------------------------------------------------------
// Top-k of each row: one wavefront per row, k selection rounds.  Every element maps to a
// 64-bit key (rank of the value, column) whose unsigned order is the documented total
// order; a round scans the row for the smallest key strictly above the previous round's,
// then reduces over the wavefront (topk_key: sg_embed_plan.h).  The input is only read.
// ---------------------------------------------------------------------------
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
  // enough workgroups to fill the device
  const GridSplit split = grid_split(m, n, (int64_t)sg_num_cus() * 8);
  if (split.blocks > 0x7FFFFFFF) return SG_ERR_UNSUPPORTED;
  float *Q = (float *)workspace;
  launch_grid_q(P, emb_q, m, params, Q, st);
  GridArgs A;
  fill_grid_common(A, P, Q, emb_db, params, m, n, split);
  A.ld = ld_out;
  A.apply_final = apply_final ? 1 : 0;
  A.out = out;
  grid_dispatch_ns(grid_dp(P) / 4, [&](auto ns) {
    hipLaunchKernelGGL(sg_grid_kernel<decltype(ns)::value>, dim3((unsigned)split.blocks),
                       dim3(256), 0, st, A);
  });
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
