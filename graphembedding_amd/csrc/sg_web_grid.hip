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
  {
    const int64_t j = j0 + c;
    const bool jin = j < A.n;
    const float *__restrict__ er = A.edb + (jin ? j : 0) * A.ld_db;
#pragma unroll
    for (int s = 0; s < NSMAX; ++s) {
      const int b = 4 * s + g;
      a[s] = 0.f;
      if (jin && b < D) a[s] = er[b];
      if (jin && b == D) a[s] = 1.f;
    }
  }
  const float usum = grid_usum(A);
  const GridCol col = grid_col(A, c, usum);   // column k = c of C
  const bool kmask = col.mask;
  const float wk = col.w;
  const int64_t qa = qc * A.qb;
  const int64_t qe = qa + A.qb < A.m ? qa + A.qb : A.m;
  const int64_t jst = j0 + 4 * g + c;   // the column lanes c < 4 store
  const float *__restrict__ Qg = A.Q;
  float4 st[NST];
#pragma unroll
  for (int t = 0; t < NST; ++t) {
    const int x = tid + 256 * t;
    if (x < nf4) ((float4 *)sQ)[x] = ((const float4 *)(Qg + qa * qw))[x];
  }
  __syncthreads();
  for (int64_t i = qa; i < qe; ++i) {
    const float *cur = sQ + ((i - qa) & 1) * qw;
    float *nxt = sQ + (((i - qa) & 1) ^ 1) * qw;
    const bool more = i + 1 < qe;
    if (more) {
#pragma unroll
      for (int t = 0; t < NST; ++t) {
        const int x = tid + 256 * t;
        st[t] = x < nf4 ? ((const float4 *)(Qg + (i + 1) * qw))[x] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    f4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NSMAX; ++s) {   // (no break: the loop must unroll, a[] stays in registers)
      if (s < ns) {
        const float b = cur[s * 64 + lane];
        if (s & 1) acc1 = mfma4(a[s], b, acc1);
        else acc0 = mfma4(a[s], b, acc0);
      }
    }
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float x = acc0[r] + acc1[r];
      v[r] = kmask ? sg_act(A.act, x) * wk : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = sgk::row_sum16(v[r]);
    float sc = v[0];
#pragma unroll
    for (int x = 1; x < 4; ++x) sc = c == x ? v[x] : sc;
    sc *= usum;
    if (A.apply_final) sc = sg_final(A.final_act, A.yeta, sc);
    if (c < 4 && jst < A.n) A.out[i * A.ld_out + jst] = sc;
    if (more) {
#pragma unroll
      for (int t = 0; t < NST; ++t) {
        const int x = tid + 256 * t;
        if (x < nf4) ((float4 *)nxt)[x] = st[t];
      }
    }
    __syncthreads();
  }
}

// the tables start at the first 16-byte boundary of the workspace (float4 staging)
float *web_grid_tables(void *workspace) {
  return (float *)(((uintptr_t)workspace + 15u) & ~(uintptr_t)15u);
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
  const int D = H.D, Dq = web_dq(D), Da = (D + 3) & ~3, ns = Dq / 4;
  const int cus = sg_num_cus();
  float *Q = web_grid_tables(workspace);

  // tables: enough row chunks to fill the device, at most 128 rows b per staged tile pair
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

  // grid: two workgroups per CU hold the device (2 x 66 KB of LDS at D = 512); past that,
  // as many queries as possible per load of a workgroup's database rows
  const GridSplit split = grid_split(m, n, (int64_t)cus * 2);
  if (split.blocks > 0x7FFFFFFF) return SG_ERR_UNSUPPORTED;
  WebGridArgs A;
  A.Q = Q;
  A.edb = emb_db;
  A.U = params + H.oU;
  A.m = m;
  A.n = n;
  A.ncb = split.ncb;
  A.D = D;
  A.K = H.K;
  A.qb = (int)split.qb;
  A.act = SG_ACT_RELU;   // the only inner activation path 3 admits
  A.ntn_mode = H.ntn_mode;
  A.final_act = H.final_act;
  A.yeta = H.yeta;
  A.ld_db = ld_db;
  A.ld_out = ld_out;
  A.ns = ns;
  A.apply_final = apply_final ? 1 : 0;
  A.out = out;
  const unsigned blocks = (unsigned)split.blocks;
  // the A-operand array of the kernel: D <= 64, 128, 256, 384, 512
  if (ns <= 17) web_grid_launch<17>(A, blocks, st);
  else if (ns <= 33) web_grid_launch<33>(A, blocks, st);
  else if (ns <= 65) web_grid_launch<65>(A, blocks, st);
  else if (ns <= 97) web_grid_launch<97>(A, blocks, st);
  else web_grid_launch<129>(A, blocks, st);
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

}  // extern "C"
