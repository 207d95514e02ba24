// sg_web_grid.h — what the two translation units of embed-once retrieval for graph-store
// (Web) models share (sg_web_grid.hip: the m x n score grid, include/siamese_web_embed.h;
// sg_web_search.hip: the grid fused with a per-query top-k, include/siamese_web_search.h):
// the per-query tables Q_i and their kernel, and the arithmetic of one score: the
// A operands of a 16-row database tile, the staging of a table through LDS, the MFMA
// k-steps and the epilogue.  The contract of the search is bitwise equality with the grid,
// so both kernels run these functions and neither has a copy.
// Internal linkage throughout: each unit compiles its own copy.
#pragma once
#include "sg_embed_plan.h"
#include "sg_mfma.h"

namespace {

using sgk::f4;
using sgk::mfma4;

// Dq: D + 1 rounded up to the MFMA k-step of 4, the rows of a table Q_i [Dq][16]
int web_dq(int D) { return (D + 1 + 3) & ~3; }

// ---------------------------------------------------------------------------
// Table kernel: Q [m][Dq][16]; rows b > D and columns k >= K are zero.
// A workgroup stages 32 queries (two 16-row MFMA tiles) transposed in LDS, sE[h][a][16], so
// that the A operand of k-step s of tile h is the linear read sE[h][64 s + lane] (lane
// (g, c): query c of the tile, a = 4 s + g), and owns a chunk of table rows b.  A wavefront
// takes four rows b at a time: the B operand of row b is W[4 s + g][b][c] (row D: V[c][4 s +
// g]), so the wavefront's loads of one k-step cover W[a][b .. b + 3][0 .. K), contiguous per
// a, and feed eight independent accumulators (4 rows x 2 query tiles).  The accumulators
// start from the V / bias term; C holds query 4 g + r in register r, column k = c.
// W is read once per 32 queries.
// ---------------------------------------------------------------------------
struct WebQArgs {
  const float *eq;
  int64_t ld_q, m;
  const float *prm;
  int oW, oV, obn;
  int D, K, Dq, Da;   // Da: D rounded up to 4 (k-steps of the contraction over a)
  int nbc, bch;       // row chunks per query tile pair, rows b per chunk (a multiple of 16)
  float *Q;
};

__global__ void __launch_bounds__(256) web_grid_q_kernel(WebQArgs A) {
  extern __shared__ __attribute__((aligned(16))) float sE[];   // [2][Da][16]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int D = A.D, K = A.K, Dq = A.Dq, Da = A.Da;
  const int64_t i0 = ((int64_t)blockIdx.x / A.nbc) * 32;
  const int bc = (int)((int64_t)blockIdx.x % A.nbc);
  for (int x = tid; x < 2 * Da * 16; x += 256) {
    const int h = x / (Da * 16), y = x - h * Da * 16;
    const int a = y >> 4;
    const int64_t qi = i0 + 16 * h + (y & 15);
    sE[x] = (qi < A.m && a < D) ? A.eq[qi * A.ld_q + a] : 0.f;
  }
  __syncthreads();
  const bool two = i0 + 16 < A.m;   // the second query tile exists
  const bool kc = c < K;
  const float *__restrict__ Wt = A.prm + A.oW;
  const float *__restrict__ Vt = A.prm + A.oV;
  const float *sE1 = sE + Da * 16;
  const int ns = Da >> 2;
  const int bend = (bc + 1) * A.bch < Dq ? (bc + 1) * A.bch : Dq;
  for (int bb = bc * A.bch + 4 * wave; bb < bend; bb += 16) {   // rows bb .. bb + 3 (Dq % 4 == 0)
    f4 acc[2][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int b = bb + j;
      float init = 0.f;
      if (kc && b < D) init = Vt[c * 2 * D + D + b];
      if (kc && b == D && A.obn >= 0) init = A.prm[A.obn + c];
      acc[0][j] = acc[1][j] = f4{init, init, init, init};
    }
    for (int s = 0; s < ns; ++s) {
      const int a = 4 * s + g;
      const bool in = kc && a < D;
      float bv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int b = bb + j;
        bv[j] = 0.f;
        if (in && b < D) bv[j] = Wt[((size_t)a * D + b) * K + c];
        if (in && b == D) bv[j] = Vt[c * 2 * D + a];
      }
      const float a0 = sE[s * 64 + lane];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[0][j] = mfma4(a0, bv[j], acc[0][j]);
      if (two) {
        const float a1 = sE1[s * 64 + lane];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[1][j] = mfma4(a1, bv[j], acc[1][j]);
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t qi = i0 + 16 * h + 4 * g + r;
        if (qi < A.m)
#pragma unroll
          for (int j = 0; j < 4; ++j) A.Q[(qi * Dq + bb + j) * 16 + c] = acc[h][j][r];
      }
  }
}

// the tables start at the first 16-byte boundary of the workspace (float4 staging)
float *web_grid_tables(void *workspace) {
  return (float *)(((uintptr_t)workspace + 15u) & ~(uintptr_t)15u);
}

// The tables of m queries into Q: enough row chunks to fill the device, at most 128 rows b
// per staged tile pair
void web_grid_launch_q(const SgWebHead &H, const float *emb_q, int64_t ld_q, int64_t m,
                       const float *params, float *Q, int cus, hipStream_t st) {
  const int D = H.D, Dq = web_dq(D), Da = (D + 3) & ~3;
  WebQArgs T;
  T.eq = emb_q; T.ld_q = ld_q; T.m = m;
  T.prm = params; T.oW = H.oW; T.oV = H.oV; T.obn = H.obn;
  T.D = D; T.K = H.K; T.Dq = Dq; T.Da = Da;
  T.Q = Q;
  const int64_t mt = (m + 31) / 32;
  const int nb16 = (Dq + 15) / 16;
  int64_t R = mt * nb16 / (2 * (int64_t)cus);
  R = R < 1 ? 1 : (R > 8 ? 8 : R);
  T.bch = 16 * (int)R;
  T.nbc = (Dq + T.bch - 1) / T.bch;
  const size_t qlds = (size_t)2 * Da * 16 * 4u;
  sg_allow_lds((const void *)web_grid_q_kernel, qlds);
  hipLaunchKernelGGL(web_grid_q_kernel, dim3((unsigned)(mt * T.nbc)), dim3(256), qlds, st, T);
}

// The head's options into the arguments every kernel over the tables takes (ncb and qb are
// the caller's: each kernel cuts the database its own way)
void web_fill_grid_common(GridCommon &A, const SgWebHead &H, const float *Q, const float *emb_db,
                          const float *params, int64_t m, int64_t n) {
  A.Q = Q;
  A.edb = emb_db;
  A.U = params + H.oU;
  A.m = m;
  A.n = n;
  A.D = H.D;
  A.K = H.K;
  A.act = SG_ACT_RELU;   // the only inner activation path 3 admits
  A.ntn_mode = H.ntn_mode;
  A.final_act = H.final_act;
  A.yeta = H.yeta;
}

// f(std::integral_constant<int, NSMAX>) for the A-operand array that holds ns k-steps:
// D <= 64, 128, 256, 384, 512
template <class F>
void web_dispatch_nsmax(int ns, F &&f) {
  if (ns <= 17) f(std::integral_constant<int, 17>{});
  else if (ns <= 33) f(std::integral_constant<int, 33>{});
  else if (ns <= 65) f(std::integral_constant<int, 65>{});
  else if (ns <= 97) f(std::integral_constant<int, 97>{});
  else f(std::integral_constant<int, 129>{});
}

// ---------------------------------------------------------------------------
// One score of the grid, as a wavefront computes sixteen of them (16 database rows against
// one query).  A wavefront keeps the augmented rows [e_j, 1, 0…] of its 16-row tile as MFMA
// A operands, one register per k-step (lane (g, c): row c, component 4 s + g; NSMAX >= ns =
// Dq / 4 is the register array's size, the loops stop at ns).  Q_i (ns x 256 B, contiguous)
// is staged in LDS once for the workgroup's four wavefronts: web_q_load takes a thread's
// float4s of a table into registers, web_q_store writes them to an LDS buffer.  The B
// operand of k-step s is the linear LDS read cur[64 s + lane]; even and odd k-steps
// accumulate in two independent chains (the instruction issues in 32 cycles with 40 of
// dependent latency), summed at the end.  Epilogue as sg_grid_kernel: relu, column weights
// and the k < K mask, the 16-lane row sum; lanes c < 4 of group g then hold the scores of
// rows 4 g + c of the tile.  web_score is web_mk (the k-steps) followed by web_score_mk (the
// epilogue); the training grid (sg_web_train.hip) calls the two halves and keeps the m_k.
// ---------------------------------------------------------------------------
template <int NSMAX>
__device__ __forceinline__ void web_load_a(const float *edb, int64_t ld_db, int64_t n, int D,
                                           int64_t j, int g, float (&a)[NSMAX]) {
  const bool jin = j < n;
  const float *__restrict__ er = edb + (jin ? j : 0) * ld_db;
#pragma unroll
  for (int s = 0; s < NSMAX; ++s) {
    const int b = 4 * s + g;
    a[s] = 0.f;
    if (jin && b < D) a[s] = er[b];
    if (jin && b == D) a[s] = 1.f;
  }
}

// the pipeline's first table, straight into its LDS buffer
template <int NST>
__device__ __forceinline__ void web_q_stage(float *dst, const float *Qi, int tid, int nf4) {
#pragma unroll
  for (int t = 0; t < NST; ++t) {
    const int x = tid + 256 * t;
    if (x < nf4) ((float4 *)dst)[x] = ((const float4 *)Qi)[x];
  }
}

template <int NST>
__device__ __forceinline__ void web_q_load(const float *Qi, int tid, int nf4, float4 (&st)[NST]) {
#pragma unroll
  for (int t = 0; t < NST; ++t) {
    const int x = tid + 256 * t;
    st[t] = x < nf4 ? ((const float4 *)Qi)[x] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

template <int NST>
__device__ __forceinline__ void web_q_store(float *dst, int tid, int nf4,
                                            const float4 (&st)[NST]) {
#pragma unroll
  for (int t = 0; t < NST; ++t) {
    const int x = tid + 256 * t;
    if (x < nf4) ((float4 *)dst)[x] = st[t];
  }
}

// the k-steps: m_k of the tile against the staged table, register r = row 4 g + r of the tile,
// column k = c
template <int NSMAX>
__device__ __forceinline__ void web_mk(const float (&a)[NSMAX], const float *cur, int ns,
                                       int lane, float (&x)[4]) {
  f4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < NSMAX; ++s) {   // (no break: the loop must unroll, a[] stays in registers)
    if (s < ns) {
      const float b = cur[s * 64 + lane];
      if (s & 1) acc1 = mfma4(a[s], b, acc1);
      else acc0 = mfma4(a[s], b, acc0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) x[r] = acc0[r] + acc1[r];
}

// the epilogue: the score of row 4 g + c from the m_k of web_mk, in lanes c < 4
__device__ __forceinline__ float web_score_mk(const float (&x)[4], int c, bool kmask, float wk,
                                              float usum, int act, int apply_final,
                                              int final_act, float yeta) {
  float v[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = kmask ? sg_act(act, x[r]) * wk : 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = sgk::row_sum16(v[r]);
  float sc = v[0];
#pragma unroll
  for (int x = 1; x < 4; ++x) sc = c == x ? v[x] : sc;
  sc *= usum;
  if (apply_final) sc = sg_final(final_act, yeta, sc);
  return sc;
}

template <int NSMAX>
__device__ __forceinline__ float web_score(const float (&a)[NSMAX], const float *cur, int ns,
                                           int lane, int c, bool kmask, float wk, float usum,
                                           int act, int apply_final, int final_act,
                                           float yeta) {
  float x[4];
  web_mk<NSMAX>(a, cur, ns, lane, x);
  return web_score_mk(x, c, kmask, wk, usum, act, apply_final, final_act, yeta);
}

}  // namespace
