// sg_web_train.hip — embed-once training for graph-store (Web) models
// (include/siamese_web_embed_train.h): forward, loss and adjoint of the m x n NTN score grid
// at Padding / NTN widths D in [32, 512], on v_mfma_f32_16x16x4_f32.  (The backward of the
// node stack, sg_web_embed_bwd: sg_web.hip.)
//
// The head (layers.py:282-310) of (query i, database j) is  m_k = [e_j, 1] · Q_i[:, k]  with
// the per-query tables Q [m][Dq][16] of sg_web_grid.h, r_k = relu(m_k), s = ΣU · Σ_k r_k
// (reference, quirk A1) or Σ_k U_k r_k (intended), ŷ = final(s).  Its adjoint per pair:
//   gs = gy · final'(s),   gm_k = relu'(m_k) · gs · (ΣU or U_k),
//   gU_k += gs · Σr (reference) or gs · r_k (intended),
// and four contractions:
//   g_emb_db[j][b] = Σ_i Σ_k Q_i[b][k] · gm_k(i, j)          (over k and over queries)
//   gQ_i[b][k]     = Σ_j [e_j, 1][b] · gm_k(i, j)            (over database rows)
//   gW[a][b][k] = Σ_i e_i[a] gQ_i[b][k], gV[k][D+b] = Σ_i gQ_i[b][k],
//   gV[k][a] = Σ_i e_i[a] gQ_i[D][k], gbias[k] = Σ_i gQ_i[D][k]   (one augmented GEMM)
//   g_emb_q[i][a] = Σ_{b<D,k} W[a][b][k] gQ_i[b][k] + Σ_k V[k][a] gQ_i[D][k].
// sg_grid_bwd_kernel (sg_embed_train.hip, D <= 31) keeps a tile's contraction, g_emb_dbᵀ and
// a transposed operand in registers and writes one gQ partial per column block; at D = 512
// that is ~400 registers and m·n·Dq bytes.  Here the grid is staged: the queries run in
// chunks of qc, a forward kernel (the score arithmetic of sg_web_grid.h, so s_out is bitwise
// sg_web_score_grid's) writes GM [qc][n64][16] = gm_k, and two GEMM kernels contract it,
// into g_emb_db (accumulated chunk after chunk in stream order, one owner per element) and
// into the chunk's gQ_i.  The table adjoint runs once over all gQ.  Every sum has one owner
// and a fixed order; no float atomics; the launch shapes depend on (m, n, D, K) only.
// Exact f32 MFMA, as the Web grid: the split-bf16 product (b3_mma6) would need GM and gQ
// split on the fly in four kernels for a head that is O(D K) per pair; not tried.
#include <stdlib.h>

#include "../../include/siamese_web_embed_train.h"
#include "sg_web_grid.h"

namespace {

constexpr int64_t kGmCapFloats = (int64_t)1 << 23;   // 32 MiB of GM per query chunk
constexpr int64_t kQcMax = 256;                      // queries per chunk at most
constexpr int64_t kFwdBlocks = 512;                  // workgroups the forward kernel aims for
constexpr int kBlkStride = 32;                       // floats per workgroup partial: gU[16], loss
constexpr int kTableCus = 256;   // web_grid_launch_q's row chunking: fixed, not the device's

int64_t up64(int64_t x) { return (x + 63) & ~(int64_t)63; }

// any layer the path reads dropout from (web_plan: 0, 1, 2 and the head) would drop
bool web_train_drops(const sg_model_t *m) {
  if (sg_keep_threshold(m->keep_prob) == 65536u) return false;
  return m->layers[0].dropout || m->layers[1].dropout || m->layers[2].dropout ||
         m->layers[4].dropout;
}

// The model checks of both the workspace query and the call: sg_web_score_grid's, then the
// dropout refusal
int web_train_plan(const sg_model_t *model, SgWebHead *H) {
  if (!model) return SG_ERR_ARG;
  const int rc = sg_web_head_plan(model, H);
  if (rc != SG_OK) return rc;
  if (H->K > kGridMaxK) return SG_ERR_UNSUPPORTED;
  if (web_train_drops(model)) return SG_ERR_UNSUPPORTED;
  return SG_OK;
}

// Launch geometry and workspace layout (host; a function of m, n, D only)
struct WebTrainGeo {
  int Dq;
  int64_t n64, ncb;
  int64_t qc;            // queries per chunk
  int64_t qb, nqs;       // queries per forward workgroup, workgroups per column block (full chunk)
  int64_t oQ, ogQ, oGM, oblk, floats;   // workspace offsets in floats
};

void web_train_geo(const SgWebHead &H, int64_t m, int64_t n, int64_t qc_override,
                   WebTrainGeo *G) {
  G->Dq = web_dq(H.D);
  G->n64 = (n + 63) & ~(int64_t)63;
  G->ncb = G->n64 / 64;
  const int64_t row = G->n64 * 16 > 0 ? G->n64 * 16 : 16;   // GM floats of one query
  int64_t qc = kGmCapFloats / row;
  qc = qc < 1 ? 1 : (qc > kQcMax ? kQcMax : qc);
  if (qc > m) qc = m > 0 ? m : 1;
  if (qc_override > 0 && qc_override < qc) qc = qc_override;   // tests: small chunks
  G->qc = qc;
  const GridSplit s = grid_split(qc, n, kFwdBlocks);
  G->qb = s.qb;
  G->nqs = s.nqc;
  const int64_t mq = m < kQcMax ? m : kQcMax;
  int64_t gm = mq * G->n64 * 16;
  const int64_t cap = kGmCapFloats > G->n64 * 16 ? kGmCapFloats : G->n64 * 16;
  if (gm > cap) gm = cap;
  int64_t o = 0;
  G->oQ = o;   o += up64(m * G->Dq * 16);
  G->ogQ = o;  o += up64(m * G->Dq * 16);
  G->oGM = o;  o += up64(gm);
  G->oblk = o; o += up64((G->ncb + kFwdBlocks) * kBlkStride);
  G->floats = o;
}

// ---------------------------------------------------------------------------
// Forward + loss + GM of one query chunk [i0, i1).  The workgroup shape is web_grid_kernel's
// (sg_web_grid.hip): 64 database rows, one 16-row tile per wavefront held as MFMA A operands,
// the queries' tables double-buffered through LDS.  Per query: the score of web_score (lanes
// c < 4 of group g: row 4 g + c), ŷ, the loss term and gs in those lanes; gs of row 4 g + r
// goes to every lane of the group (four ds_bpermute), and with m_k in the accumulator layout
// (register r: row 4 g + r, column k = c) the lane stores GM[i - i0][row][k] and adds to its
// column's gU.  Rows j >= n hold zero operands: gs = 0 there and GM is written as zeros up
// to n64, so the GEMMs below read no garbage.  One partial row {gU[16], loss} per workgroup,
// added to the row of the same workgroup of the previous chunks (stream order).
// ---------------------------------------------------------------------------
struct WebTrainFwdArgs : GridCommon {
  int64_t ld_db, ld_lab, ld_s, n64, i0, i1;
  int ns, loss_mode, first;
  float inv_batch;
  const float *labels, *y_stats;
  float *s_out, *GM, *blkp;
};

template <int NSMAX>
__global__ void __launch_bounds__(256) web_train_fwd_kernel(WebTrainFwdArgs A) {
  extern __shared__ __attribute__((aligned(16))) float sQ[];   // [2][ns * 64]
  __shared__ float bred[4][20];
  constexpr int NST = (NSMAX + 15) / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int ns = A.ns, qw = ns * 64, nf4 = ns * 16;
  const int64_t cb = (int64_t)blockIdx.x % A.ncb, qs = (int64_t)blockIdx.x / A.ncb;
  const int64_t j0 = cb * 64 + 16 * wave;
  float a[NSMAX];
  web_load_a<NSMAX>(A.edb, A.ld_db, A.n, A.D, j0 + c, g, a);
  const float usum = grid_usum(A);
  const GridCol col = grid_col(A, c, usum);
  const bool kmask = col.mask;
  const float wk = col.w, uw = col.uw;
  const bool broadcast = A.loss_mode == SG_LOSS_BROADCAST;
  const float ybar = broadcast ? A.y_stats[0] : 0.f;
  const int64_t qa = A.i0 + qs * A.qb;
  const int64_t qe = qa + A.qb < A.i1 ? qa + A.qb : A.i1;
  const int64_t jr = j0 + 4 * g + (c & 3);   // the row whose score lanes c < 4 hold
  const bool valid = c < 4 && jr < A.n;
  const float *__restrict__ Qg = A.Q;
  float uacc = 0.f, loss_acc = 0.f;
  float4 st[NST];
  web_q_stage<NST>(sQ, Qg + qa * qw, tid, nf4);
  __syncthreads();
  for (int64_t i = qa; i < qe; ++i) {
    const float *cur = sQ + ((i - qa) & 1) * qw;
    float *nxt = sQ + (((i - qa) & 1) ^ 1) * qw;
    const bool more = i + 1 < qe;
    if (more) web_q_load<NST>(Qg + (i + 1) * qw, tid, nf4, st);
    float x[4];   // web_score's two halves (sg_web_grid.h): the m_k stay
    web_mk<NSMAX>(a, cur, ns, lane, x);
    const float sc = web_score_mk(x, c, kmask, wk, usum, A.act, 0, A.final_act, A.yeta);
    if (valid && A.s_out) A.s_out[i * A.ld_s + jr] = sc;
    const float yhat = sg_final(A.final_act, A.yeta, sc);
    float gy, l;
    if (broadcast) {
      gy = yhat - ybar;
      l = 0.5f * gy * gy;
    } else {
      const float dlt = yhat - (valid ? A.labels[i * A.ld_lab + jr] : 0.f);
      gy = dlt * A.inv_batch;
      l = 0.5f * dlt * dlt * A.inv_batch;
    }
    const float gsv = valid ? gy * sg_final_grad(A.final_act, A.yeta, sc, yhat) : 0.f;
    loss_acc += valid ? l : 0.f;
    float *__restrict__ gmr = A.GM + ((i - A.i0) * A.n64 + j0 + 4 * g) * 16 + c;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float gs = __shfl(gsv, (lane & 48) | r, 64);
      const float rr = kmask ? sg_act(A.act, x[r]) : 0.f;
      uacc = fmaf(gs, rr, uacc);
      gmr[r * 16] = kmask ? sg_act_grad(A.act, x[r], rr, gs * uw) : 0.f;
    }
    if (more) web_q_store<NST>(nxt, tid, nf4, st);
    __syncthreads();
  }
  const float u = sgk::xsum32(sgk::xsum16(uacc));   // column c over the four row groups
  if (g == 0) bred[wave][c] = u;
  const float lsum = sg_wave_sum(loss_acc);
  if (lane == 0) bred[wave][16] = lsum;
  __syncthreads();
  if (tid < 17) {
    const float v = ((bred[0][tid] + bred[1][tid]) + bred[2][tid]) + bred[3][tid];
    float *dst = A.blkp + (int64_t)blockIdx.x * kBlkStride + tid;
    *dst = A.first ? v : *dst + v;
  }
}

// ---------------------------------------------------------------------------
// g_emb_db[j][b] (+)= Σ_il Σ_k GM[il][j][k] · Q_{i0 + il}[b][k]: [n64 x 16 qcn]·[16 qcn x D].
// A workgroup owns 64 rows j x 32 columns b, a wavefront one 16-row tile and both 16-column
// tiles.  Per query a lane loads GM[il][j0 + c][4 g ..+3] and Q[b0 + c][4 g ..+3] (16 bytes
// each, a tile's 1 KB contiguous): MFMA k-step t contracts k = 4 g + t.  Queries in order,
// one owner per element: the first chunk stores, the later ones add.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) web_train_gdb_kernel(const float *__restrict__ GM,
                                                            const float *__restrict__ Q,
                                                            int64_t n, int64_t n64, int D, int Dq,
                                                            int64_t i0, int64_t qcn, int first,
                                                            float *__restrict__ g_emb_db,
                                                            int64_t ld_gdb) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int64_t j0 = (int64_t)blockIdx.x * 64 + 16 * wave;
  const int b0 = (int)blockIdx.y * 32;
  f4 acc[2] = {f4{0.f, 0.f, 0.f, 0.f}, f4{0.f, 0.f, 0.f, 0.f}};
  const float *__restrict__ gmp = GM + (j0 + c) * 16 + 4 * g;
  const float *__restrict__ qp = Q + i0 * Dq * 16 + 4 * g;
  const bool bin0 = b0 + c < Dq, bin1 = b0 + 16 + c < Dq;
  for (int64_t il = 0; il < qcn; ++il) {
    const f4 av = *(const f4 *)(gmp + il * n64 * 16);
    const float *__restrict__ Qi = qp + il * Dq * 16;
    const f4 z = {0.f, 0.f, 0.f, 0.f};
    const f4 bv0 = bin0 ? *(const f4 *)(Qi + (b0 + c) * 16) : z;
    const f4 bv1 = bin1 ? *(const f4 *)(Qi + (b0 + 16 + c) * 16) : z;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      acc[0] = mfma4(av[t], bv0[t], acc[0]);
      acc[1] = mfma4(av[t], bv1[t], acc[1]);
    }
  }
#pragma unroll
  for (int bt = 0; bt < 2; ++bt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t j = j0 + 4 * g + r;
      const int b = b0 + 16 * bt + c;
      if (j < n && b < D) {
        float *dst = g_emb_db + j * ld_gdb + b;
        *dst = first ? acc[bt][r] : *dst + acc[bt][r];
      }
    }
}

// ---------------------------------------------------------------------------
// gQ_i[b][k] = Σ_j [e_j, 1][b] · GM[il][j][k]: per query [Dq x n64]·[n64 x 16].  Workgroup
// (query, 256 rows b); a wavefront owns four 16-row tiles of b.  MFMA k-step t contracts rows
// j = 4 t + g: the B operand is the linear read GM[il][64 t + lane], the A operands are
// [e_j, 1][b0 + c] (64 contiguous bytes of four rows), reused over the chunk's queries from L2.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) web_train_gq_kernel(const float *__restrict__ GM,
                                                           const float *__restrict__ edb,
                                                           int64_t ld_db, int64_t n, int64_t n64,
                                                           int D, int Dq, int64_t i0,
                                                           float *__restrict__ gQ) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int64_t il = blockIdx.x;
  const int b0 = (int)blockIdx.y * 256 + 64 * wave;
  if (b0 >= Dq) return;   // (no barrier below)
  int nbt = (Dq - b0 + 15) / 16;
  nbt = nbt > 4 ? 4 : nbt;
  f4 acc[4];
#pragma unroll
  for (int bt = 0; bt < 4; ++bt) acc[bt] = f4{0.f, 0.f, 0.f, 0.f};
  const float *__restrict__ GMi = GM + il * n64 * 16;
  for (int64_t t = 0; t < n64 / 4; ++t) {
    const float bop = GMi[t * 64 + lane];
    const int64_t j = 4 * t + g;
    const bool jin = j < n;
    const float *__restrict__ er = edb + (jin ? j : 0) * ld_db;
#pragma unroll
    for (int bt = 0; bt < 4; ++bt) {
      if (bt < nbt) {
        const int b = b0 + 16 * bt + c;
        float aop = 0.f;
        if (jin && b < D) aop = er[b];
        if (jin && b == D) aop = 1.f;
        acc[bt] = mfma4(aop, bop, acc[bt]);
      }
    }
  }
  float *__restrict__ gQi = gQ + (i0 + il) * Dq * 16;
#pragma unroll
  for (int bt = 0; bt < 4; ++bt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = b0 + 16 * bt + 4 * g + r;
      if (b < Dq) gQi[b * 16 + c] = acc[bt][r];
    }
}

// ---------------------------------------------------------------------------
// Table adjoint, parameters: out[a][b][k] = Σ_i [e_i, 1][a] · gQ_i[b][k] for a, b in [0, D]:
// (a < D, b < D) is gW, (D, b) gV[k][D + b], (a, D) gV[k][a], (D, D) gbias.  A wavefront
// owns 32 rows a x 4 rows b x 16 columns k and walks all m queries, four per MFMA k-step
// (A: [e_i, 1][a0 + c] of query 4 t + g, B: gQ_i[b][c]); a workgroup takes 16 rows b.
// ---------------------------------------------------------------------------
struct WebTrainTabArgs {
  const float *eq, *gQ;
  int64_t ld_q, m;
  int D, K, Dq, oW, oV, obn;
  float *grad;
};

__global__ void __launch_bounds__(256) web_train_tab_kernel(WebTrainTabArgs A) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int D = A.D, K = A.K, Dq = A.Dq;
  const int b0 = (int)blockIdx.x * 16 + 4 * wave;
  const int a0 = (int)blockIdx.y * 32;
  if (b0 > D) return;   // (no barrier below; Dq % 4 == 0, so b0 + 3 < Dq)
  f4 acc[2][4];
#pragma unroll
  for (int at = 0; at < 2; ++at)
#pragma unroll
    for (int bj = 0; bj < 4; ++bj) acc[at][bj] = f4{0.f, 0.f, 0.f, 0.f};
  const float *__restrict__ eq = A.eq;
  const float *__restrict__ gQ = A.gQ;
  for (int64_t i4 = 0; i4 < A.m; i4 += 4) {
    const int64_t i = i4 + g;
    const bool iin = i < A.m;
    const float *__restrict__ er = eq + (iin ? i : 0) * A.ld_q;
    const float *__restrict__ gq = gQ + ((iin ? i : 0) * Dq + b0) * 16 + c;
    float aop[2], bop[4];
#pragma unroll
    for (int at = 0; at < 2; ++at) {
      const int a = a0 + 16 * at + c;
      aop[at] = 0.f;
      if (iin && a < D) aop[at] = er[a];
      if (iin && a == D) aop[at] = 1.f;
    }
#pragma unroll
    for (int bj = 0; bj < 4; ++bj) bop[bj] = iin ? gq[bj * 16] : 0.f;
#pragma unroll
    for (int at = 0; at < 2; ++at)
#pragma unroll
      for (int bj = 0; bj < 4; ++bj) acc[at][bj] = mfma4(aop[at], bop[bj], acc[at][bj]);
  }
  if (c >= K) return;
  const int k = c;
#pragma unroll
  for (int at = 0; at < 2; ++at)
#pragma unroll
    for (int bj = 0; bj < 4; ++bj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int a = a0 + 16 * at + 4 * g + r, b = b0 + bj;
        const float v = acc[at][bj][r];
        if (a < D && b < D) A.grad[A.oW + ((size_t)a * D + b) * K + k] = v;
        else if (a == D && b < D) A.grad[A.oV + k * 2 * D + D + b] = v;
        else if (a < D && b == D) A.grad[A.oV + k * 2 * D + a] = v;
        else if (a == D && b == D && A.obn >= 0) A.grad[A.obn + k] = v;
      }
}

// ---------------------------------------------------------------------------
// Table adjoint, embeddings: g_emb_q[i][a] = Σ_{b<D} Σ_k gQ_i[b][k] W[a][b][k] + Σ_k
// gQ_i[D][k] V[k][a]: [m x (D+1) 16]·[(D+1) 16 x D].  A wavefront owns 64 queries x 16
// columns a, a workgroup 64 columns; per row b a lane loads gQ_i[b][4 g ..+3] of its four
// query tiles and W[a0 + c][b][4 g ..+3] (k >= K: zero), MFMA k-step t contracts k = 4 g + t.
// ---------------------------------------------------------------------------
struct WebTrainGeqArgs {
  const float *gQ, *prm;
  int64_t m, ld_gq;
  int D, K, Dq, oW, oV;
  float *g_emb_q;
};

__global__ void __launch_bounds__(256) web_train_geq_kernel(WebTrainGeqArgs A) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int D = A.D, K = A.K, Dq = A.Dq;
  const int64_t i0 = (int64_t)blockIdx.x * 64;
  const int at0 = (int)blockIdx.y * 64 + 16 * wave;
  if (at0 >= D) return;   // (no barrier below)
  const int a = at0 + c;
  const bool ain = a < D;
  f4 acc[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) acc[it] = f4{0.f, 0.f, 0.f, 0.f};
  const float *__restrict__ Wa = A.prm + A.oW + (size_t)(ain ? a : 0) * D * K;
  const float *__restrict__ Va = A.prm + A.oV + (ain ? a : 0);
  const float *gqp[4];
  bool iin[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int64_t i = i0 + 16 * it + c;
    iin[it] = i < A.m;
    gqp[it] = A.gQ + (iin[it] ? i : 0) * Dq * 16 + 4 * g;
  }
  for (int b = 0; b <= D; ++b) {
    float bv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int k = 4 * g + t;
      bv[t] = 0.f;
      if (ain && k < K) bv[t] = b < D ? Wa[b * K + k] : Va[k * 2 * D];
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const f4 z = {0.f, 0.f, 0.f, 0.f};
      const f4 av = iin[it] ? *(const f4 *)(gqp[it] + b * 16) : z;
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[it] = mfma4(av[t], bv[t], acc[it]);
    }
  }
#pragma unroll
  for (int it = 0; it < 4; ++it)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t i = i0 + 16 * it + 4 * g + r;
      if (i < A.m && ain) A.g_emb_q[i * A.ld_gq + a] = acc[it][r];
    }
}

// ---------------------------------------------------------------------------
// gU and the loss: the forward kernel's partial rows summed in a fixed order (thread t takes
// column t & 31 of rows (t >> 5) + 8 i, the eight strands are added in order), as
// sg_grid_head_kernel does.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) web_train_head_kernel(const float *__restrict__ blkp,
                                                             int64_t nblk, int K, int intended,
                                                             int add_label,
                                                             const float *__restrict__ y_stats,
                                                             float *__restrict__ gU,
                                                             float *__restrict__ loss) {
  __shared__ float strand[8][kBlkStride];
  __shared__ float cs[kBlkStride];
  const int x = threadIdx.x & 31, st = threadIdx.x >> 5;
  float acc = 0.f;
  if (x < 17)
    for (int64_t bk = st; bk < nblk; bk += 8) acc += blkp[bk * kBlkStride + x];
  strand[st][x] = acc;
  __syncthreads();
  if (threadIdx.x < kBlkStride) {
    float v = 0.f;
    for (int s = 0; s < 8; ++s) v += strand[s][threadIdx.x];
    cs[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x < K) {   // weights_U (reference, quirk A1: every U_k sees Σ_k r_k)
    float v = cs[threadIdx.x];
    if (!intended) {
      v = 0.f;
      for (int k = 0; k < 16; ++k) v += cs[k];
    }
    gU[threadIdx.x] = v;
  }
  if (threadIdx.x == 16 && loss) loss[0] = cs[16] + (add_label ? y_stats[1] : 0.f);
}

template <int NSMAX>
void web_train_fwd_launch(const WebTrainFwdArgs &A, unsigned blocks, hipStream_t st) {
  const size_t lds = (size_t)2 * A.ns * 64 * 4u;
  sg_allow_lds((const void *)web_train_fwd_kernel<NSMAX>, lds);
  hipLaunchKernelGGL(web_train_fwd_kernel<NSMAX>, dim3(blocks), dim3(256), lds, st, A);
}

// SG_WEB_TRAIN_QC=n: at most n queries per chunk (tests reach several chunks on a small
// grid; read per call).  It can only shrink the chunk, so the workspace of the query serves.
int64_t web_train_qc_override() {
  const char *e = getenv("SG_WEB_TRAIN_QC");
  return e ? atoll(e) : 0;
}

}  // namespace

extern "C" {

int64_t sg_web_score_grid_bwd_workspace_bytes(const sg_model_t *model, int64_t m, int64_t n) {
  SgWebHead H;
  if (m < 0 || n < 0 || m > kMaxRows || n > kMaxRows || web_train_plan(model, &H) != SG_OK)
    return -1;
  WebTrainGeo G;
  web_train_geo(H, m, n, 0, &G);
  return G.floats * 4 + 256;
}

int32_t sg_web_score_grid_fwd_bwd(const sg_model_t *model, const float *emb_q, int64_t ld_q,
                                  const float *emb_db, int64_t ld_db, int64_t m, int64_t n,
                                  const float *params, const float *labels, int64_t ld_labels,
                                  int64_t batch_total, const float *y_stats,
                                  int32_t add_label_term, float *s_out, int64_t ld_s,
                                  float *g_emb_q, int64_t ld_gq, float *g_emb_db,
                                  int64_t ld_gdb, float *grad_out, float *loss_out,
                                  void *workspace, sg_stream_t stream) {
  if (!model || m < 0 || n < 0) return SG_ERR_ARG;
  SgWebHead H;
  const int rc = web_train_plan(model, &H);
  if (rc != SG_OK) return rc;
  if (m > kMaxRows || n > kMaxRows) return SG_ERR_UNSUPPORTED;
  if (m == 0 || n == 0) return SG_OK;
  const int D = H.D, K = H.K;
  if (!emb_q || !emb_db || !params || !g_emb_q || !g_emb_db || !grad_out || !workspace ||
      ld_q < D || ld_db < D || ld_gq < D || ld_gdb < D || (s_out && ld_s < n))
    return SG_ERR_ARG;
  const bool broadcast = model->loss_mode == SG_LOSS_BROADCAST;
  if (broadcast && !y_stats) return SG_ERR_ARG;
  if (!broadcast && (!labels || ld_labels < n || batch_total <= 0)) return SG_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  (void)hipGetLastError();   // report only this call's launch errors
  WebTrainGeo G;
  web_train_geo(H, m, n, web_train_qc_override(), &G);
  const int Dq = G.Dq, ns = Dq / 4;
  float *ws = web_grid_tables(workspace);
  float *Q = ws + G.oQ, *gQ = ws + G.ogQ, *GM = ws + G.oGM, *blkp = ws + G.oblk;
  web_grid_launch_q(H, emb_q, ld_q, m, params, Q, kTableCus, st);

  WebTrainFwdArgs A;
  web_fill_grid_common(A, H, Q, emb_db, params, m, n);
  A.ncb = G.ncb;
  A.qb = (int)G.qb;
  A.ld_db = ld_db;
  A.ld_lab = ld_labels;
  A.ld_s = ld_s;
  A.n64 = G.n64;
  A.ns = ns;
  A.loss_mode = model->loss_mode;
  A.inv_batch = batch_total > 0 ? 1.f / (float)batch_total : 0.f;
  A.labels = labels;
  A.y_stats = y_stats;
  A.s_out = s_out;
  A.GM = GM;
  A.blkp = blkp;
  for (int64_t i0 = 0; i0 < m; i0 += G.qc) {
    const int64_t qcn = m - i0 < G.qc ? m - i0 : G.qc;
    const int first = i0 == 0 ? 1 : 0;
    A.i0 = i0;
    A.i1 = i0 + qcn;
    A.first = first;
    const unsigned blocks = (unsigned)(G.ncb * ((qcn + G.qb - 1) / G.qb));
    web_dispatch_nsmax(ns, [&](auto nsmax) {
      web_train_fwd_launch<decltype(nsmax)::value>(A, blocks, st);
    });
    hipLaunchKernelGGL(web_train_gdb_kernel, dim3((unsigned)G.ncb, (unsigned)((D + 31) / 32)),
                       dim3(256), 0, st, (const float *)GM, (const float *)Q, n, G.n64, D, Dq, i0,
                       qcn, first, g_emb_db, ld_gdb);
    hipLaunchKernelGGL(web_train_gq_kernel, dim3((unsigned)qcn, (unsigned)((Dq + 255) / 256)),
                       dim3(256), 0, st, (const float *)GM, emb_db, ld_db, n, G.n64, D, Dq, i0,
                       gQ);
  }
  WebTrainTabArgs T;
  T.eq = emb_q; T.gQ = gQ; T.ld_q = ld_q; T.m = m;
  T.D = D; T.K = K; T.Dq = Dq; T.oW = H.oW; T.oV = H.oV; T.obn = H.obn;
  T.grad = grad_out;
  hipLaunchKernelGGL(web_train_tab_kernel, dim3((unsigned)((Dq + 15) / 16), (unsigned)(D / 32 + 1)),
                     dim3(256), 0, st, T);
  WebTrainGeqArgs E;
  E.gQ = gQ; E.prm = params; E.m = m; E.ld_gq = ld_gq;
  E.D = D; E.K = K; E.Dq = Dq; E.oW = H.oW; E.oV = H.oV;
  E.g_emb_q = g_emb_q;
  hipLaunchKernelGGL(web_train_geq_kernel, dim3((unsigned)((m + 63) / 64), (unsigned)((D + 63) / 64)),
                     dim3(256), 0, st, E);
  hipLaunchKernelGGL(web_train_head_kernel, dim3(1), dim3(256), 0, st, (const float *)blkp,
                     G.ncb * G.nqs, K, H.ntn_mode == SG_NTN_INTENDED ? 1 : 0,
                     (broadcast && add_label_term && y_stats) ? 1 : 0, y_stats, grad_out + H.oU,
                     loss_out);
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

}  // extern "C"
