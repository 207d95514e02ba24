// sg_web_grid.hip — the NTN score grid of embed-once retrieval for graph-store (Web)
// models (include/siamese_web_embed.h; the embeddings come from sg_web_embed, sg_web.hip),
// on v_mfma_f32_16x16x4_f32 at Padding / NTN widths D in [32, 512].
//
// The NTN head (layers.py:282-310) of (query i as graph 1, database j as graph 2) is
//   m_k = e_i^T W[:,:,k] e_j + V[k] · [e_i, e_j] + bias[k]  =  [e_j, 1] · Q_i[:, k]
// with the per-query table  Q_i[b][k] = Σ_a e_i[a] W[a][b][k] + V[k][D + b]  (b < D) and
// Q_i[D][k] = Σ_a V[k][a] e_i[a] + bias[k].  sg_embed.hip does the same at D <= 31 with a
// tile's whole contraction in registers and one thread per table entry; here the table is
// a GEMM [m x D]·[D x (D K)] that reads W once per 32 queries, and the grid walks the
// contraction over b in Dq / 4 MFMA k-steps with the tables staged through LDS.
// Exact f32, fixed summation orders: bitwise reproducible, independent of the launch shape.
#include "../../include/siamese_web_embed.h"
#include "sg_web_grid.h"

namespace {

// ---------------------------------------------------------------------------
// Grid kernel over the tables.  A workgroup owns 64 database rows and a chunk of queries
// (grid_split); each of its four wavefronts keeps the augmented rows [e_j, 1, 0…] of its own
// 16-row tile as MFMA A operands, one register per k-step (lane (g, c): row c, component
// 4 s + g; NSMAX >= ns = Dq / 4 is the register array's size, the loops stop at ns).  The
// workgroup walks the chunk's queries: Q_i (ns x 256 B, contiguous) is staged in LDS once
// for the four wavefronts, double-buffered, the next query's loads issued before this
// query's MFMAs and written to LDS after them, one barrier per query.  The B operand of
// k-step s is the linear LDS read sQ[64 s + lane]; even and odd k-steps accumulate in two
// independent chains (the instruction issues in 32 cycles with 40 of dependent latency),
// summed at the end.  Epilogue as sg_grid_kernel: relu, column weights and the k < K mask,
// the 16-lane row sum; lanes c < 4 of group g then hold the scores of rows 4 g + c, and the
// wavefront stores 16 consecutive columns of row i of `out`.
// ---------------------------------------------------------------------------
struct WebGridArgs : GridCommon {
  int64_t ld_db, ld_out;
  int ns;
  int apply_final;
  float *out;
};

template <int NSMAX>
__global__ void __launch_bounds__(256) web_grid_kernel(WebGridArgs A) {
  extern __shared__ __attribute__((aligned(16))) float sQ[];   // [2][ns * 64]
  constexpr int NST = (NSMAX + 15) / 16;   // float4 of a table per thread
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int ns = A.ns, qw = ns * 64, nf4 = ns * 16;
  const int64_t cb = (int64_t)blockIdx.x % A.ncb, qc = (int64_t)blockIdx.x / A.ncb;
  const int64_t j0 = cb * 64 + 16 * wave;
  const int D = A.D;
  float a[NSMAX];
  web_load_a<NSMAX>(A.edb, A.ld_db, A.n, D, j0 + c, g, a);
  const float usum = grid_usum(A);
  const GridCol col = grid_col(A, c, usum);   // column k = c of C
  const bool kmask = col.mask;
  const float wk = col.w;
  const int64_t qa = qc * A.qb;
  const int64_t qe = qa + A.qb < A.m ? qa + A.qb : A.m;
  const int64_t jst = j0 + 4 * g + c;   // the column lanes c < 4 store
  const float *__restrict__ Qg = A.Q;
  float4 st[NST];
  web_q_stage<NST>(sQ, Qg + qa * qw, tid, nf4);
  __syncthreads();
  for (int64_t i = qa; i < qe; ++i) {
    const float *cur = sQ + ((i - qa) & 1) * qw;
    float *nxt = sQ + (((i - qa) & 1) ^ 1) * qw;
    const bool more = i + 1 < qe;
    if (more) web_q_load<NST>(Qg + (i + 1) * qw, tid, nf4, st);
    const float sc = web_score<NSMAX>(a, cur, ns, lane, c, kmask, wk, usum, A.act, A.apply_final,
                                      A.final_act, A.yeta);
    if (c < 4 && jst < A.n) A.out[i * A.ld_out + jst] = sc;
    if (more) web_q_store<NST>(nxt, tid, nf4, st);
    __syncthreads();
  }
}

template <int NSMAX>
void web_grid_launch(const WebGridArgs &A, unsigned blocks, hipStream_t st) {
  const size_t lds = (size_t)2 * A.ns * 64 * 4u;
  sg_allow_lds((const void *)web_grid_kernel<NSMAX>, lds);
  hipLaunchKernelGGL(web_grid_kernel<NSMAX>, dim3(blocks), dim3(256), lds, st, A);
}

}  // namespace

extern "C" {

int64_t sg_web_score_grid_workspace_bytes(const sg_model_t *model, int64_t m) {
  SgWebHead H;
  if (m < 0 || m > kMaxRows || sg_web_head_plan(model, &H) != SG_OK) return -1;
  return m * web_dq(H.D) * 16 * 4 + 256;
}

int32_t sg_web_score_grid(const sg_model_t *model, const float *emb_q, int64_t ld_q,
                          const float *emb_db, int64_t ld_db, int64_t m, int64_t n,
                          const float *params, int32_t apply_final, float *out, int64_t ld_out,
                          void *workspace, sg_stream_t stream) {
  if (!model || m < 0 || n < 0) return SG_ERR_ARG;
  SgWebHead H;
  const int rc = sg_web_head_plan(model, &H);
  if (rc != SG_OK) return rc;
  if (H.K > kGridMaxK) return SG_ERR_UNSUPPORTED;
  if (m > kMaxRows || n > kMaxRows) return SG_ERR_UNSUPPORTED;
  if (m == 0 || n == 0) return SG_OK;
  if (!emb_q || !emb_db || !params || !out || !workspace || ld_q < H.D || ld_db < H.D ||
      ld_out < n)
    return SG_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  (void)hipGetLastError();   // report only this call's launch errors
  const int ns = web_dq(H.D) / 4;
  const int cus = sg_num_cus();
  float *Q = web_grid_tables(workspace);
  web_grid_launch_q(H, emb_q, ld_q, m, params, Q, cus, st);

  // grid: two workgroups per CU hold the device (2 x 66 KB of LDS at D = 512); past that,
  // as many queries as possible per load of a workgroup's database rows
  const GridSplit split = grid_split(m, n, (int64_t)cus * 2);
  if (split.blocks > 0x7FFFFFFF) return SG_ERR_UNSUPPORTED;
  WebGridArgs A;
  web_fill_grid_common(A, H, Q, emb_db, params, m, n);
  A.ncb = split.ncb;
  A.qb = (int)split.qb;
  A.ld_db = ld_db;
  A.ld_out = ld_out;
  A.ns = ns;
  A.apply_final = apply_final ? 1 : 0;
  A.out = out;
  const unsigned blocks = (unsigned)split.blocks;
  web_dispatch_nsmax(ns, [&](auto nsmax) {
    web_grid_launch<decltype(nsmax)::value>(A, blocks, st);
  });
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

}  // extern "C"
