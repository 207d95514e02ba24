// sg_embed_train.hip — embed-once training (include/siamese_embed_train.h): forward, loss
// and adjoint of the m x n NTN score grid on v_mfma_f32_16x16x4_f32, the table adjoint
// that turns the query tables' gradients into the head's parameter gradients and the query
// embeddings' gradients.  (The backward of the node stack, sg_embed_bwd: sg_embed_nodes.hip.)
//
// The head (layers.py:282-310) of (query i, database j) is  m_k = [e_j, 1] · Q_i[:, k]
// (sg_embed_plan.h), r_k = act(m_k), s = ΣU · Σ_k r_k (reference, quirk A1) or Σ_k U_k r_k
// (intended), ŷ = final(s).  Its adjoint per pair:
//   gs = gy · final'(s),   gm_k = act'(m_k) · gs · (ΣU or U_k),
//   gU_k += gs · Σr (reference) or gs · r_k (intended),
//   gQ_i[b][k]     = Σ_j [e_j, 1][b] · gm_k(i, j)            (contraction over database rows)
//   g_emb_db[j][b] = Σ_i Σ_k Q_i[b][k] · gm_k(i, j)          (over k and over queries)
// and, O(m), the table adjoint
//   gW[a][b][k] = Σ_i e_i[a] gQ_i[b][k],   gV[k][D+b] = Σ_i gQ_i[b][k],
//   gV[k][a] = Σ_i e_i[a] gQ_i[D][k],      gbias[k] = Σ_i gQ_i[D][k],
//   g_emb_q[i][a] = Σ_{b<D,k} W[a][b][k] gQ_i[b][k] + Σ_k V[k][a] gQ_i[D][k].
// Dropout 0 only: the header states why, train_plan (sg_embed_plan.h) refuses everything else.
#include "../../include/siamese_embed_train.h"
#include "sg_embed_bwd.h"
#include "sg_mfma.h"

namespace {

using sgk::f4;

constexpr int64_t kTrainGridBlocks = 1024;   // workgroups the grid kernel aims for
constexpr int kBlkStride = 32;               // floats per workgroup partial: gU[16], loss

// ---------------------------------------------------------------------------
// Launch geometry and workspace layout of the grid call (host; independent of the device,
// so the workspace query and the launch agree everywhere)
// ---------------------------------------------------------------------------
struct TrainGeo {
  GridSplit split;                // for kTrainGridBlocks workgroups, whatever the device
  int64_t chunk, nch;             // queries per table-adjoint chunk, chunks
  int64_t nT;                     // table-adjoint columns: W, V, bias
  int64_t oQ, ogQ, ogQp, ogdbp, oblk, otab, floats;   // workspace offsets in floats
};

int64_t up64(int64_t x) { return (x + 63) & ~(int64_t)63; }

bool train_geo(const SgGenPlan &P, int64_t m, int64_t n, TrainGeo *G) {
  const int64_t Dp = grid_dp(P), D = P.D, K = P.K;
  G->split = grid_split(m, n, kTrainGridBlocks);
  const GridSplit &s = G->split;
  G->chunk = (m + 1023) / 1024 > 64 ? (m + 1023) / 1024 : 64;
  G->nch = (m + G->chunk - 1) / G->chunk;
  G->nT = D * D * K + 2 * D * K + K;
  // the partials of the query tables' gradients dominate: refuse what overflows int64
  const double est = (double)s.ncb * (double)m * (double)(Dp * 16) +
                     (double)s.nqc * (double)n * (double)D + 2.0 * (double)m * (double)(Dp * 16) +
                     (double)s.blocks * kBlkStride + (double)G->nch * (double)G->nT;
  if (est > 1.0e18 || s.blocks > 0x7FFFFFFF) return false;
  int64_t o = 0;
  G->oQ = o;    o += up64(m * Dp * 16);
  G->ogQ = o;   o += up64(m * Dp * 16);
  G->ogQp = o;  o += up64(s.ncb * m * Dp * 16);
  G->ogdbp = o; o += up64(s.nqc * n * D);
  G->oblk = o;  o += up64(s.blocks * kBlkStride);
  G->otab = o;  o += up64(G->nch * G->nT);
  G->floats = o;
  return true;
}

// ---------------------------------------------------------------------------
// Grid forward + adjoint.  The workgroup shape is sg_grid_kernel's (sg_embed.hip): 64
// database rows (four 16-row tiles) and a range of queries, each of four wavefronts walks
// every fourth query.  MFMA layouts (lane l: g = l >> 4, c = l & 15): an A operand holds
// A[row c][k-slot g], a B operand B[k-slot g][column c], the accumulator register r holds
// C[row 4 g + r][column c].
//   a[t][s]       = [e_j, 1][b = 4 s + g] of row j = 16 t + c          (forward operand)
//   aT[t][r][bt]  = [e_j, 1][b = 16 bt + c] of row j = 16 t + 4 g + r  (A operand of gQ)
// Per query, with b[s] = Q_i[4 s + g][c]:
//   MT[t] = Σ_s mfma(b[s], a[t][s])   = Mᵀ[k = 4 g + r][j = 16 t + c]  (operands swapped)
//   M[t]  = Σ_s mfma(a[t][s], b[s])   = M [j = 16 t + 4 g + r][k = c]
// MT gives the scores (the sum over k is a sum over registers and over g: two permlane
// swaps), each lane's four gs of rows j = 16 t + c, and GMᵀ as the B operand of the
// contraction over k:  g_emb_dbᵀ[b][j] += Σ_k Q_i[b][k] GMᵀ[k][j], accumulated in registers
// over the wavefront's queries.  gs crosses to the other layout through 64 floats of LDS
// per wavefront (lane l writes row l's; a 16-byte read returns rows 16 t + 4 g + 0..3), M is
// recomputed rather than transposed, and GM[j][k] is the B operand of the contraction over
// j:  gQ_i[b][k] = Σ_j [e_j, 1][b] GM[j][k], sixteen k-steps of four rows.
// Across workgroups: gQ_i partials per column block and g_emb_db partials per query chunk
// go to the workspace and are summed in a fixed order (sg_sum_rows); gU and the loss go
// to one partial row per workgroup.  No float atomics.
// ---------------------------------------------------------------------------
struct TrainGridArgs : GridCommon {
  const float *labels, *y_stats;
  int64_t ld_lab, ld_s;
  int loss_mode;
  float inv_batch;
  float *s_out, *gQp, *gdbp, *blkp;
};

template <int NS>
__global__ void __launch_bounds__(256) sg_grid_bwd_kernel(TrainGridArgs A) {
  constexpr int NB = NS > 4 ? 2 : 1;      // 16-row tiles of b = 0 .. Dp - 1
  constexpr int Dp = 4 * NS;
  __shared__ __attribute__((aligned(16))) float gsl[4][64];
  __shared__ float red[4][64][16 * NB + 1];
  __shared__ float bred[4][20];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int64_t cb = (int64_t)blockIdx.x % A.ncb, qc = (int64_t)blockIdx.x / A.ncb;
  const int64_t j0 = cb * 64;
  const int D = A.D;
  float a[4][NS], aT[4][4][NB];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int s = 0; s < NS; ++s) a[t][s] = grid_aug(A, j0 + 16 * t + c, 4 * s + g);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int bt = 0; bt < NB; ++bt)
        aT[t][r][bt] = grid_aug(A, j0 + 16 * t + 4 * g + r, 16 * bt + c);
  }
  // column weights (grid_col) in both layouts: k = c (M) and k = 4 g + r (MT)
  const float usum = grid_usum(A);
  const GridCol col = grid_col(A, c, usum);
  const bool kmask = col.mask;
  const float uw = col.uw;
  bool kmT[4];
  float wT[4], uwT[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const GridCol cT = grid_col(A, 4 * g + r, usum);
    kmT[r] = cT.mask;
    wT[r] = cT.w;
    uwT[r] = cT.uw;
  }
  const bool broadcast = A.loss_mode == SG_LOSS_BROADCAST;
  const float ybar = broadcast ? A.y_stats[0] : 0.f;
  f4 gdb[4][NB];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int bt = 0; bt < NB; ++bt) gdb[t][bt] = f4{0.f, 0.f, 0.f, 0.f};
  float uacc[4] = {0.f, 0.f, 0.f, 0.f}, loss_acc = 0.f;
  const int64_t q1 = (qc + 1) * A.qb < A.m ? (qc + 1) * A.qb : A.m;
  for (int64_t i = qc * A.qb + wave; i < q1; i += 4) {
    float b[NS];
    const float *__restrict__ Qi = grid_load_q<NS>(A, i, lane, b);
    f4 qT[NB];   // Q_i[b = 16 bt + c][k = 4 g + 0..3]
#pragma unroll
    for (int bt = 0; bt < NB; ++bt) {
      const int row = 16 * bt + c;
      qT[bt] = row < Dp ? *(const f4 *)(Qi + row * 16 + 4 * g) : f4{0.f, 0.f, 0.f, 0.f};
    }
    // ---- transposed forward: scores, loss, gs ----
    f4 MT[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) MT[t] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int t = 0; t < 4; ++t) MT[t] = sgk::mfma4(b[s], a[t][s], MT[t]);
    float RT[4][4], gs[4];
    float s_mine = 0.f, l_mine = 0.f, gs_mine = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float p = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        RT[t][r] = kmT[r] ? sg_act(A.act, MT[t][r]) : 0.f;
        p = fmaf(RT[t][r], wT[r], p);
      }
      const float s = sgk::xsum32(sgk::xsum16(p)) * usum;
      const int64_t j = j0 + 16 * t + c;
      const bool valid = j < A.n;
      const float yhat = sg_final(A.final_act, A.yeta, s);
      float gy, l;
      if (broadcast) {
        gy = yhat - ybar;
        l = 0.5f * gy * gy;
      } else {
        const float dlt = yhat - (valid ? A.labels[i * A.ld_lab + j] : 0.f);
        gy = dlt * A.inv_batch;
        l = 0.5f * dlt * dlt * A.inv_batch;
      }
      gs[t] = valid ? gy * sg_final_grad(A.final_act, A.yeta, s, yhat) : 0.f;
      if (t == g) {   // each row j once: by the lane whose g is its tile
        s_mine = s;
        l_mine = valid ? l : 0.f;
        gs_mine = gs[t];
      }
    }
    loss_acc += l_mine;
    const int64_t jm = j0 + lane;   // = 16 g + c: the row this lane reports
    if (A.s_out && jm < A.n) A.s_out[i * A.ld_s + jm] = s_mine;
    gsl[wave][lane] = gs_mine;
    sg_wsync();
    // ---- GMᵀ and the contraction over k ----
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        uacc[r] = fmaf(gs[t], RT[t][r], uacc[r]);
        MT[t][r] = kmT[r] ? sg_act_grad(A.act, MT[t][r], RT[t][r], gs[t] * uwT[r]) : 0.f;
      }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int bt = 0; bt < NB; ++bt) gdb[t][bt] = sgk::mfma4(qT[bt][r], MT[t][r], gdb[t][bt]);
    // ---- M again in the forward layout, GM and the contraction over j ----
    f4 M[4], gsn[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      M[t] = f4{0.f, 0.f, 0.f, 0.f};
      gsn[t] = *(const f4 *)&gsl[wave][16 * t + 4 * g];
    }
    sg_wsync();   // the next query overwrites gsl
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int t = 0; t < 4; ++t) M[t] = sgk::mfma4(a[t][s], b[s], M[t]);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float mv = M[t][r];
        M[t][r] = kmask ? sg_act_grad(A.act, mv, sg_act(A.act, mv), gsn[t][r] * uw) : 0.f;
      }
    f4 gq[NB];
#pragma unroll
    for (int bt = 0; bt < NB; ++bt) gq[bt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int bt = 0; bt < NB; ++bt) gq[bt] = sgk::mfma4(aT[t][r][bt], M[t][r], gq[bt]);
    float *__restrict__ gQi = A.gQp + (cb * A.m + i) * (NS * 64);
#pragma unroll
    for (int bt = 0; bt < NB; ++bt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * bt + 4 * g + r;
        if (row < Dp) gQi[row * 16 + c] = gq[bt][r];
      }
  }
  // ---- workgroup partials: g_emb_db of the 64 rows, gU[16], loss ----
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int bt = 0; bt < NB; ++bt)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][16 * t + c][16 * bt + 4 * g + r] = gdb[t][bt][r];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float u = sgk::row_sum16(uacc[r]);
    if (c == 0) bred[wave][4 * g + r] = u;
  }
  const float lsum = sgk::xsum32(sgk::xsum16(sgk::row_sum16(loss_acc)));
  if (lane == 0) bred[wave][16] = lsum;
  __syncthreads();
  for (int e = threadIdx.x; e < 64 * D; e += 256) {
    const int j = e / D, bb = e - j * D;
    if (j0 + j < A.n)
      A.gdbp[(qc * A.n + j0 + j) * D + bb] =
          ((red[0][j][bb] + red[1][j][bb]) + red[2][j][bb]) + red[3][j][bb];
  }
  if (threadIdx.x < 17)
    A.blkp[(int64_t)blockIdx.x * kBlkStride + threadIdx.x] =
        ((bred[0][threadIdx.x] + bred[1][threadIdx.x]) + bred[2][threadIdx.x]) +
        bred[3][threadIdx.x];
}

// ---------------------------------------------------------------------------
// Table adjoint.  tab: one partial row [nT] = {gW, gV, gbias} per chunk of queries; gq:
// g_emb_q; head: the fixed-order sums into grad_out's head range and loss_out.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) sg_grid_tab_kernel(const float *__restrict__ eq,
                                                          const float *__restrict__ gQ, int64_t m,
                                                          int D, int K, int Dp, int64_t chunk,
                                                          int nT, int neb,
                                                          float *__restrict__ tabp) {
  const int64_t ch = (int64_t)blockIdx.x / neb;
  const int e = (int)((int64_t)blockIdx.x % neb) * 256 + threadIdx.x;
  if (e >= nT) return;
  const int nW = D * D * K, nV = 2 * D * K;
  int ea = -1, gb = D, k;   // Σ_i (ea >= 0 ? e_i[ea] : 1) · gQ_i[gb][k]
  if (e < nW) {
    ea = e / (D * K);
    gb = (e / K) % D;
    k = e % K;
  } else if (e < nW + nV) {
    const int x = e - nW, y = x % (2 * D);
    k = x / (2 * D);
    if (y < D) ea = y; else gb = y - D;
  } else {
    k = e - nW - nV;
  }
  const int64_t i0 = ch * chunk, i1 = i0 + chunk < m ? i0 + chunk : m;
  float acc = 0.f;
  for (int64_t i = i0; i < i1; ++i)
    acc = fmaf(ea >= 0 ? eq[i * D + ea] : 1.f, gQ[(i * Dp + gb) * 16 + k], acc);
  tabp[ch * nT + e] = acc;
}

__global__ void __launch_bounds__(256) sg_grid_gq_kernel(const float *__restrict__ gQ, int64_t m,
                                                         int D, int K, int Dp,
                                                         const float *__restrict__ prm, int offW,
                                                         int offV, float *__restrict__ g_emb_q) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= m * D) return;
  const int64_t i = t / D;
  const int a = (int)(t - i * D);
  const float *__restrict__ gq = gQ + i * Dp * 16;
  float acc = 0.f;
  for (int b = 0; b < D; ++b)
    for (int k = 0; k < K; ++k) acc = fmaf(prm[offW + (a * D + b) * K + k], gq[b * 16 + k], acc);
  for (int k = 0; k < K; ++k) acc = fmaf(prm[offV + k * 2 * D + a], gq[D * 16 + k], acc);
  g_emb_q[t] = acc;
}

struct HeadArgs {
  const float *tabp, *blkp, *y_stats;
  int64_t nch, nblk;
  int nT, nWV, K, has_bias, intended, add_label;
  float *grad_head, *loss;   // grad_out + offW
};

// The last workgroup sums the grid kernel's partial rows {gU[16], loss}: thread t takes
// column t & 31 of rows (t >> 5) + 8 i, the eight strands are added in order.  The others
// sum the table adjoint's chunk rows, one thread per W / V / bias element.
__global__ void __launch_bounds__(256) sg_grid_head_kernel(HeadArgs A) {
  __shared__ float strand[8][kBlkStride];
  __shared__ float cs[kBlkStride];
  if (blockIdx.x == gridDim.x - 1) {
    const int x = threadIdx.x & 31, st = threadIdx.x >> 5;
    float acc = 0.f;
    if (x < 17)
      for (int64_t bk = st; bk < A.nblk; bk += 8) acc += A.blkp[bk * kBlkStride + x];
    strand[st][x] = acc;
    __syncthreads();
    if (threadIdx.x < kBlkStride) {
      float v = 0.f;
      for (int s = 0; s < 8; ++s) v += strand[s][threadIdx.x];
      cs[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x < A.K) {   // weights_U (reference, quirk A1: every U_k sees Σ_k r_k)
      float v = cs[threadIdx.x];
      if (!A.intended) {
        v = 0.f;
        for (int k = 0; k < 16; ++k) v += cs[k];
      }
      A.grad_head[A.nWV + threadIdx.x] = v;
    }
    if (threadIdx.x == 16 && A.loss) A.loss[0] = cs[16] + (A.add_label ? A.y_stats[1] : 0.f);
    return;
  }
  const int e = blockIdx.x * 256 + threadIdx.x;   // column of the table adjoint's rows
  if (e >= A.nWV + (A.has_bias ? A.K : 0)) return;
  float acc = 0.f;
  for (int64_t ch = 0; ch < A.nch; ++ch) acc += A.tabp[ch * A.nT + e];
  A.grad_head[e < A.nWV ? e : e + A.K] = acc;   // bias follows U in the parameter vector
}

}  // namespace

extern "C" {

int64_t sg_score_grid_bwd_workspace_bytes(const sg_model_t *model, int64_t m, int64_t n) {
  SgGenPlan P;
  if (m < 0 || n < 0 || m > kMaxRows || n > kMaxRows || train_plan(model, &P, true) != SG_OK)
    return -1;
  TrainGeo G;
  if (!train_geo(P, m, n, &G)) return -1;
  return G.floats * 4 + 256;
}

int32_t sg_score_grid_fwd_bwd(const sg_model_t *model, const float *emb_q, const float *emb_db,
                              int64_t m, int64_t n, const float *params, const float *labels,
                              int64_t ld_labels, int64_t batch_total, const float *y_stats,
                              int32_t add_label_term, float *s_out, int64_t ld_s,
                              float *g_emb_q, float *g_emb_db, float *grad_out,
                              float *loss_out, void *workspace, sg_stream_t stream) {
  if (!model || m < 0 || n < 0) return SG_ERR_ARG;
  SgGenPlan P;
  const int rc = train_plan(model, &P, true);
  if (rc != SG_OK) return rc;
  if (m > kMaxRows || n > kMaxRows) return SG_ERR_UNSUPPORTED;
  if (m == 0 || n == 0) return SG_OK;
  if (!emb_q || !emb_db || !params || !g_emb_q || !g_emb_db || !grad_out || !workspace)
    return SG_ERR_ARG;
  if (ld_labels < n || (s_out && ld_s < n)) return SG_ERR_ARG;
  const bool broadcast = P.loss_mode == SG_LOSS_BROADCAST;
  if (broadcast && !y_stats) return SG_ERR_ARG;
  if (!broadcast && (!labels || batch_total <= 0)) return SG_ERR_ARG;
  if (((uintptr_t)workspace & 15u) != 0) return SG_ERR_ARG;   // 16-byte table reads
  TrainGeo G;
  if (!train_geo(P, m, n, &G)) return SG_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int Dp = grid_dp(P), D = P.D, K = P.K;
  float *ws = (float *)workspace;
  float *Q = ws + G.oQ, *gQ = ws + G.ogQ, *gQp = ws + G.ogQp, *gdbp = ws + G.ogdbp;
  float *blkp = ws + G.oblk, *tabp = ws + G.otab;
  const int64_t qelems = m * Dp * 16;
  launch_grid_q(P, emb_q, m, params, Q, st);
  TrainGridArgs A;
  fill_grid_common(A, P, Q, emb_db, params, m, n, G.split);
  A.labels = labels;
  A.y_stats = y_stats;
  A.ld_lab = ld_labels;
  A.ld_s = ld_s;
  A.loss_mode = P.loss_mode;
  A.inv_batch = batch_total > 0 ? 1.f / (float)batch_total : 0.f;
  A.s_out = s_out;
  A.gQp = gQp;
  A.gdbp = gdbp;
  A.blkp = blkp;
  grid_dispatch_ns(Dp / 4, [&](auto ns) {
    hipLaunchKernelGGL(sg_grid_bwd_kernel<decltype(ns)::value>, dim3((unsigned)G.split.blocks),
                       dim3(256), 0, st, A);
  });
  // fixed-order sums of the partials: gQ over column blocks, g_emb_db over query chunks
  hipLaunchKernelGGL(sg_sum_rows, dim3((unsigned)((qelems + 255) / 256)), dim3(256), 0, st,
                     (const float *)gQp, G.split.ncb, qelems, gQ);
  const int64_t dbelems = n * D;
  hipLaunchKernelGGL(sg_sum_rows, dim3((unsigned)((dbelems + 255) / 256)), dim3(256), 0, st,
                     (const float *)gdbp, G.split.nqc, dbelems, g_emb_db);
  // table adjoint
  const int nT = (int)G.nT, neb = (nT + 255) / 256;
  hipLaunchKernelGGL(sg_grid_tab_kernel, dim3((unsigned)(G.nch * neb)), dim3(256), 0, st, emb_q,
                     (const float *)gQ, m, D, K, Dp, G.chunk, nT, neb, tabp);
  hipLaunchKernelGGL(sg_grid_gq_kernel, dim3((unsigned)((m * D + 255) / 256)), dim3(256), 0, st,
                     (const float *)gQ, m, D, K, Dp, params, P.offW, P.offV, g_emb_q);
  HeadArgs H;
  H.tabp = tabp;
  H.blkp = blkp;
  H.y_stats = y_stats;
  H.nch = G.nch;
  H.nblk = G.split.blocks;
  H.nT = nT;
  H.nWV = D * D * K + 2 * D * K;
  H.K = K;
  H.has_bias = P.head_bias;
  H.intended = P.ntn_mode == SG_NTN_INTENDED ? 1 : 0;
  H.add_label = (broadcast && add_label_term && y_stats) ? 1 : 0;
  H.grad_head = grad_out + P.offW;
  H.loss = loss_out;
  const int ntab = H.nWV + (P.head_bias ? K : 0);
  hipLaunchKernelGGL(sg_grid_head_kernel, dim3((unsigned)((ntab + 255) / 256 + 1)), dim3(256), 0,
                     st, H);
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

}  // extern "C"
