// sg_dot_grid.hip — embed-once retrieval, search and training for the Dot head
// (include/siamese_dot_embed.h): the score grid E_q · E_dbᵀ on v_mfma_f32_16x16x4_f32, the
// same grid fused with the per-query running top-k of sg_search.hip (sg_search_lists.h), and
// the grid's forward + loss + adjoint (GS staged in the workspace, then GS · E_db and
// GSᵀ · E_q as two fixed-order products).
//
// One score is one accumulator chain (dot_tile): every kernel that produces a score calls that
// function, so the grid, the search and the training call agree bit for bit.
#include "../../include/siamese_dot_embed.h"
#include "sg_embed_bwd.h"
#include "sg_mfma.h"
#include "sg_search_lists.h"

namespace {

using sgk::f4;

constexpr int kDotMaxE = 512;
constexpr int kDotListLds = 32768;      // LDS for the lists of a workgroup's queries
constexpr int kTileLd = 68;             // floats per row of a wavefront's 16 x 64 score tile:
                                        // rows 4 g + r of the four lane groups 16 banks apart
constexpr int kTileFloats = 16 * kTileLd;
constexpr int64_t kAdjChunk = 512;      // contraction rows per partial product of the adjoint

// embed_plan with the Dot head this unit serves, or an SG_ERR_* code
int dot_plan(const sg_model_t *model, SgGenPlan *P) {
  const int rc = embed_plan(model, P);
  if (rc != SG_OK) return rc;
  if (P->head_kind != SG_DOT || plan_embed_dim(*P) < 1 || plan_embed_dim(*P) > kDotMaxE)
    return SG_ERR_UNSUPPORTED;
  return SG_OK;
}

// ---------------------------------------------------------------------------
// The chain.  MFMA layouts (lane l: g = l >> 4, c = l & 15): an A operand holds A[row c]
// [k-slot g], a B operand B[k-slot g][column c], accumulator register r holds C[row 4 g + r]
// [column c].  Queries are A, database rows are B:
//   acc[t][r] = s(i0 + 4 g + r, j0 + 16 t + c),  t = 0 .. 3
// k-step s takes components a = 4 s + g; rows >= m, >= n and components >= E are zeros (the
// address is clamped to one that exists, the value is selected afterwards).
// ---------------------------------------------------------------------------
struct DotOps {
  const float *q, *db;
  int64_t ld_q, ld_db, m, n;
  int E;
};

__device__ __forceinline__ void dot_tile(const DotOps &A, int64_t i0, int64_t j0, int g, int c,
                                         f4 (&acc)[4]) {
  const int64_t i = i0 + c;
  const bool qv = i < A.m;
  const float *__restrict__ qr = A.q + (qv ? i : 0) * A.ld_q;
  const float *__restrict__ dr[4];
  bool dv[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int64_t j = j0 + 16 * t + c;
    dv[t] = j < A.n;
    dr[t] = A.db + (dv[t] ? j : 0) * A.ld_db;
    acc[t] = f4{0.f, 0.f, 0.f, 0.f};
  }
  // full k-steps, the next step's operands loaded before this step's MFMAs (the last step
  // reloads its own)
  const int nfull = A.E >> 2;
  float qn = 0.f, dn[4] = {0.f, 0.f, 0.f, 0.f};
  if (nfull > 0) {
    qn = qr[g];
#pragma unroll
    for (int t = 0; t < 4; ++t) dn[t] = dr[t][g];
  }
  for (int s = 0; s < nfull; ++s) {
    const float a = qv ? qn : 0.f;
    float b[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) b[t] = dv[t] ? dn[t] : 0.f;
    const int k = 4 * (s + 1 < nfull ? s + 1 : s) + g;
    qn = qr[k];
#pragma unroll
    for (int t = 0; t < 4; ++t) dn[t] = dr[t][k];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = sgk::mfma4(a, b[t], acc[t]);
  }
  if (A.E & 3) {   // the zero-padded tail k-step
    const int k = 4 * nfull + g;
    const bool kv = k < A.E;
    const float qa = qr[kv ? k : 0];
    const float a = (qv && kv) ? qa : 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float db = dr[t][kv ? k : 0];
      acc[t] = sgk::mfma4(a, (dv[t] && kv) ? db : 0.f, acc[t]);
    }
  }
}

// ---------------------------------------------------------------------------
// Score grid: a workgroup owns a 64 x 64 tile of `out`, each of its four wavefronts 16
// queries of it.  The launch is ceil(n / 64) · ceil(m / 64) workgroups on every device.
// ---------------------------------------------------------------------------
struct DotGridArgs {
  DotOps O;
  int64_t ncb, ld;
  int apply_final, final_act;
  float yeta;
  float *out;
};

__global__ void __launch_bounds__(256) dot_grid_kernel(DotGridArgs A) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int64_t cb = (int64_t)blockIdx.x % A.ncb, qb = (int64_t)blockIdx.x / A.ncb;
  const int64_t j0 = cb * 64, i0 = qb * 64 + 16 * wave;
  if (i0 >= A.O.m) return;   // the whole wavefront; the kernel has no barrier
  f4 acc[4];
  dot_tile(A.O, i0, j0, g, c, acc);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t i = i0 + 4 * g + r;
    if (i >= A.O.m) continue;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int64_t j = j0 + 16 * t + c;
      float s = acc[t][r];
      if (A.apply_final) s = sg_final(A.final_act, A.yeta, s);
      if (j < A.O.n) A.out[i * A.ld + j] = s;
    }
  }
}

// ---------------------------------------------------------------------------
// Search.  How a call is cut (search_split, sg_search_split.h): S segments of seg database
// columns times nqc chunks of qb queries (a multiple of 16), one workgroup each; wavefront w of
// a workgroup takes the chunk's groups of 16 queries w, w + nw, …  For each 64-column block of
// the segment it computes the group's 16 x 64 scores (dot_tile), turns them through its own LDS tile so that
// lane l holds column j0 + l of one query, and meets that query's running list exactly as
// sg_search_kernel does (list_insert).  A query's list belongs to one wavefront: no barrier.
// ---------------------------------------------------------------------------
struct DotSearchPlan : SearchSplit {   // the workspace is the candidates alone: cand_bytes
  int waves;
  size_t lds;
};

// Every host check that needs no pointer, in the header's order
int dot_search_plan(const sg_model_t *model, int64_t m, int64_t n, int32_t k, int64_t seg_cols,
                    SgGenPlan *P, DotSearchPlan *S) {
  if (!model || m < 0 || n < 0) return SG_ERR_ARG;
  int rc = dot_plan(model, P);
  if (rc != SG_OK) return rc;
  // 8 workgroups per CU fill the device
  rc = search_split(SearchUnit{(int64_t)sg_num_cus() * 8, 16, kDotListLds}, m, n, k, seg_cols, S);
  if (rc != SG_OK) return rc;
  S->waves = S->qb / 16 > 4 ? 4 : (int)(S->qb / 16);
  S->lds = (size_t)S->qb * k * kListBytes + (size_t)S->waves * kTileFloats * 4;
  return SG_OK;
}

struct DotSearchArgs {
  DotOps O;
  int64_t seg, nseg;
  int qb, k, apply_final, largest, final_act;
  float yeta;
  ListOut out;
};

__global__ void __launch_bounds__(256) dot_search_kernel(DotSearchArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int g = lane >> 4, c = lane & 15, k = A.k;
  const int64_t sgm = (int64_t)blockIdx.x % A.nseg, qc = (int64_t)blockIdx.x / A.nseg;
  const int64_t q0 = qc * A.qb;
  const int64_t q1 = q0 + A.qb < A.O.m ? q0 + A.qb : A.O.m;
  const int64_t c0 = sgm * A.seg;
  const int64_t c1 = c0 + A.seg < A.O.n ? c0 + A.seg : A.O.n;
  uint64_t *lkeys = (uint64_t *)smem;                          // [qb][k]
  float *lvals = (float *)(lkeys + (size_t)A.qb * k);           // [qb][k]
  float *tile = lvals + (size_t)A.qb * k + wave * kTileFloats;   // [16][kTileLd], this wave's
  for (int64_t i0 = q0 + 16 * wave; i0 < q1; i0 += 16 * nw)
    for (int R = 0; R < 16 && i0 + R < q1; ++R) list_reset(lkeys + (i0 + R - q0) * k, k, lane);
  sg_wsync();
  for (int64_t i0 = q0 + 16 * wave; i0 < q1; i0 += 16 * nw) {
    for (int64_t j0 = c0; j0 < c1; j0 += 64) {
      f4 acc[4];
      dot_tile(A.O, i0, j0, g, c, acc);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) tile[(4 * g + r) * kTileLd + 16 * t + c] = acc[t][r];
      sg_wsync();
      const int64_t jst = j0 + lane;   // the column whose score this lane reads
      for (int R = 0; R < 16 && i0 + R < q1; ++R) {
        float s = tile[R * kTileLd + lane];
        if (A.apply_final) s = sg_final(A.final_act, A.yeta, s);
        uint64_t *lk = lkeys + (i0 + R - q0) * k;
        const uint64_t thr = lk[k - 1];
        const uint64_t key = jst < A.O.n ? topk_key(s, (uint32_t)jst, A.largest) : ~0ull;
        list_offer(lk, lvals + (i0 + R - q0) * k, k, lane, key, s, thr);
      }
      sg_wsync();   // the next block overwrites the tile
    }
  }
  for (int64_t i0 = q0 + 16 * wave; i0 < q1; i0 += 16 * nw)
    for (int R = 0; R < 16 && i0 + R < q1; ++R) {
      if (lane >= k) continue;
      const int64_t i = i0 + R;
      const uint64_t key = lkeys[(i - q0) * k + lane];
      const float val = lvals[(i - q0) * k + lane];
      if (A.nseg == 1) {   // k <= n: every entry is a column
        A.out.idx[i * k + lane] = (int32_t)(uint32_t)key;
        if (A.out.val) A.out.val[i * k + lane] = val;
      } else {   // a short last segment leaves sentinels; their values are never read
        const int64_t o = (sgm * A.O.m + i) * k + lane;
        A.out.ckey[o] = key;
        A.out.cval[o] = val;
      }
    }
}

// ---------------------------------------------------------------------------
// Training.  Launch geometry and workspace layout (host; a function of m, n and E alone, so
// the workspace query and the launch agree everywhere).
// ---------------------------------------------------------------------------
struct DotTrainGeo {
  int64_t ncb, nqb, blocks;        // 64 x 64 tiles of the grid
  int64_t nchq, nchdb;             // partial products of g_emb_q (over n) and g_emb_db (over m)
  int64_t oGS, oblk, opq, opdb, floats;   // workspace offsets in floats
};

int64_t up64(int64_t x) { return (x + 63) & ~(int64_t)63; }

bool dot_train_geo(int64_t m, int64_t n, int64_t E, DotTrainGeo *G) {
  G->ncb = (n + 63) / 64;
  G->nqb = (m + 63) / 64;
  G->blocks = G->ncb * G->nqb;
  G->nchq = (n + kAdjChunk - 1) / kAdjChunk;
  G->nchdb = (m + kAdjChunk - 1) / kAdjChunk;
  // GS dominates: refuse what overflows the launch index or a sane byte count
  const double est = (double)m * (double)n + (double)G->blocks +
                     (double)G->nchq * (double)m * (double)E +
                     (double)G->nchdb * (double)n * (double)E;
  if (est > 2.8e17 || G->blocks > 0x7FFFFFFF) return false;   // 2^60 bytes
  const int64_t ncolb = (E + 63) / 64;   // workgroups of the two adjoint launches
  if (G->nqb * ncolb * G->nchq > 0x7FFFFFFF || G->ncb * ncolb * G->nchdb > 0x7FFFFFFF)
    return false;
  int64_t o = 0;
  G->oGS = o;  o += up64(m * n);
  G->oblk = o; o += up64(G->blocks);
  G->opq = o;  o += up64(G->nchq * m * E);
  G->opdb = o; o += up64(G->nchdb * n * E);
  G->floats = o;
  return true;
}

// Forward + loss + GS: the score grid's tiles, each lane's sixteen scores turned into ŷ, the
// loss term and gs = gy · final'(s).  The loss of a tile is summed lane by lane (r outer, t
// inner), over the wavefront by DPP / permlane sums and over the four wavefronts in order.
struct DotTrainArgs {
  DotOps O;
  int64_t ncb, ld_lab, ld_s;
  const float *labels, *y_stats;
  int final_act, loss_mode;
  float yeta, inv_batch;
  float *s_out, *GS, *blkp;
};

__global__ void __launch_bounds__(256) dot_train_fwd_kernel(DotTrainArgs A) {
  __shared__ float wsum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int64_t cb = (int64_t)blockIdx.x % A.ncb, qb = (int64_t)blockIdx.x / A.ncb;
  const int64_t j0 = cb * 64, i0 = qb * 64 + 16 * wave;
  const bool broadcast = A.loss_mode == SG_LOSS_BROADCAST;
  const float ybar = broadcast ? A.y_stats[0] : 0.f;
  float loss_acc = 0.f;
  if (i0 < A.O.m) {   // wave-uniform
    f4 acc[4];
    dot_tile(A.O, i0, j0, g, c, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t i = i0 + 4 * g + r;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int64_t j = j0 + 16 * t + c;
        if (i >= A.O.m || j >= A.O.n) continue;
        const float s = acc[t][r];
        const float yhat = sg_final(A.final_act, A.yeta, s);
        float gy, l;
        if (broadcast) {
          gy = yhat - ybar;
          l = 0.5f * gy * gy;
        } else {
          const float dlt = yhat - A.labels[i * A.ld_lab + j];
          gy = dlt * A.inv_batch;
          l = 0.5f * dlt * dlt * A.inv_batch;
        }
        loss_acc += l;
        if (A.s_out) A.s_out[i * A.ld_s + j] = s;
        A.GS[i * A.O.n + j] = gy * sg_final_grad(A.final_act, A.yeta, s, yhat);
      }
    }
  }
  const float lsum = sgk::xsum32(sgk::xsum16(sgk::row_sum16(loss_acc)));
  if (lane == 0) wsum[wave] = lsum;
  __syncthreads();
  if (threadIdx.x == 0) A.blkp[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// One partial product of an adjoint:  part[ch][row][a] = Σ_{kk in chunk ch} G(row, kk) ·
// X[kk][a], G(row, kk) = G[row · rs + kk · ks] (rs = n, ks = 1: GS for g_emb_q; rs = 1,
// ks = n: GSᵀ for g_emb_db), one MFMA chain over kk ascending, four rows per k-step, rows past
// the chunk's end as zeros.  A workgroup owns 64 rows x 64 columns a of one chunk, each
// wavefront 16 rows; column tiles at or past E are skipped (wave-uniform).
struct DotAdjArgs {
  const float *G, *X;
  int64_t rs, ks, R, K, ldx, nrb;
  int E, ncolb;
  float *part;   // [nch][R][E]
};

__global__ void __launch_bounds__(256) dot_adj_kernel(DotAdjArgs A) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int64_t rb = (int64_t)blockIdx.x % A.nrb, rest = (int64_t)blockIdx.x / A.nrb;
  const int ab = (int)(rest % A.ncolb);
  const int64_t ch = rest / A.ncolb;
  const int64_t r0 = rb * 64 + 16 * wave;
  if (r0 >= A.R) return;   // the whole wavefront; the kernel has no barrier
  const int a0 = ab * 64;
  const int64_t k0 = ch * kAdjChunk;
  const int64_t k1 = k0 + kAdjChunk < A.K ? k0 + kAdjChunk : A.K;
  const int64_t row = r0 + c;
  const bool rv = row < A.R;
  const float *__restrict__ gr = A.G + (rv ? row : 0) * A.rs;
  bool cv[4];
  int col[4];
  f4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    cv[t] = a0 + 16 * t + c < A.E;
    col[t] = cv[t] ? a0 + 16 * t + c : 0;
    acc[t] = f4{0.f, 0.f, 0.f, 0.f};
  }
  for (int64_t kb = k0; kb < k1; kb += 4) {
    const int64_t kk = kb + g;
    const bool kv = kk < k1;
    const int64_t ks = kv ? kk : k0;
    const float ga = gr[ks * A.ks];
    const float a = (rv && kv) ? ga : 0.f;
    const float *__restrict__ xr = A.X + ks * A.ldx;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (a0 + 16 * t >= A.E) continue;   // wave-uniform
      const float x = xr[col[t]];
      acc[t] = sgk::mfma4(a, (cv[t] && kv) ? x : 0.f, acc[t]);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t ro = r0 + 4 * g + r;
    if (ro >= A.R) continue;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (cv[t]) A.part[(ch * A.R + ro) * A.E + a0 + 16 * t + c] = acc[t][r];
  }
}

// loss_out[0] = Σ blkp (+ y_stats[1]): thread t sums tiles t, t + 256, …, the 256 strands are
// added by a fixed tree.
__global__ void __launch_bounds__(256) dot_loss_kernel(const float *__restrict__ blkp,
                                                       int64_t nblk,
                                                       const float *__restrict__ y_stats,
                                                       int add_label, float *__restrict__ loss) {
  __shared__ float strand[256];
  float acc = 0.f;
  for (int64_t b = threadIdx.x; b < nblk; b += 256) acc += blkp[b];
  strand[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) strand[threadIdx.x] += strand[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = strand[0] + (add_label ? y_stats[1] : 0.f);
}

// the model checks of the training call: dot_plan, then no effective dropout (train_plan's rule)
int dot_train_plan(const sg_model_t *model, SgGenPlan *P) {
  const int rc = dot_plan(model, P);
  return rc != SG_OK ? rc : plan_no_dropout(model);
}

void dot_adj_launch(const float *G, int64_t rs, int64_t ks, int64_t R, int64_t K, const float *X,
                    int64_t ldx, int E, int64_t nch, float *part, float *out, hipStream_t st) {
  DotAdjArgs A;
  A.G = G;
  A.X = X;
  A.rs = rs;
  A.ks = ks;
  A.R = R;
  A.K = K;
  A.ldx = ldx;
  A.nrb = (R + 63) / 64;
  A.E = E;
  A.ncolb = (E + 63) / 64;
  A.part = part;
  hipLaunchKernelGGL(dot_adj_kernel, dim3((unsigned)(A.nrb * A.ncolb * nch)), dim3(256), 0, st,
                     A);
  const int64_t elems = R * E;
  hipLaunchKernelGGL(sg_sum_rows, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st,
                     (const float *)part, nch, elems, out);
}

}  // namespace

extern "C" {

int32_t sg_dot_score_grid(const sg_model_t *model, const float *emb_q, int64_t ld_q,
                          const float *emb_db, int64_t ld_db, int64_t m, int64_t n,
                          int32_t apply_final, float *out, int64_t ld_out, sg_stream_t stream) {
  if (!model || m < 0 || n < 0) return SG_ERR_ARG;
  SgGenPlan P;
  const int rc = dot_plan(model, &P);
  if (rc != SG_OK) return rc;
  if (m > kMaxRows || n > kMaxRows) return SG_ERR_UNSUPPORTED;
  if (m == 0 || n == 0) return SG_OK;
  const int E = plan_embed_dim(P);
  if (!emb_q || !emb_db || !out || ld_q < E || ld_db < E || ld_out < n) return SG_ERR_ARG;
  DotGridArgs A;
  A.O = DotOps{emb_q, emb_db, ld_q, ld_db, m, n, E};
  A.ncb = (n + 63) / 64;
  const int64_t blocks = A.ncb * ((m + 63) / 64);
  if (blocks > 0x7FFFFFFF) return SG_ERR_UNSUPPORTED;
  A.ld = ld_out;
  A.apply_final = apply_final ? 1 : 0;
  A.final_act = P.final_act;
  A.yeta = P.yeta;
  A.out = out;
  (void)hipGetLastError();   // report only this call's launch errors
  hipLaunchKernelGGL(dot_grid_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     A);
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

int64_t sg_dot_search_topk_workspace_bytes(const sg_model_t *model, int64_t m, int64_t n,
                                           int32_t k, int64_t seg_cols) {
  SgGenPlan P;
  DotSearchPlan S;
  if (dot_search_plan(model, m, n, k, seg_cols, &P, &S) != SG_OK) return -1;
  return S.cand_bytes;
}

int32_t sg_dot_search_topk(const sg_model_t *model, const float *emb_q, int64_t ld_q,
                           const float *emb_db, int64_t ld_db, int64_t m, int64_t n,
                           int32_t apply_final, int32_t k, int32_t largest, int64_t seg_cols,
                           int32_t *idx_out, float *val_out, void *workspace,
                           sg_stream_t stream) {
  SgGenPlan P;
  DotSearchPlan S;
  const int rc = dot_search_plan(model, m, n, k, seg_cols, &P, &S);
  if (rc != SG_OK) return rc;
  if (m == 0) return SG_OK;
  const int E = plan_embed_dim(P);
  if (!emb_q || !emb_db || !idx_out || !workspace || ((uintptr_t)workspace & 7u) != 0 ||
      ld_q < E || ld_db < E)
    return SG_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  DotSearchArgs A;
  A.O = DotOps{emb_q, emb_db, ld_q, ld_db, m, n, E};
  A.seg = S.seg;
  A.nseg = S.nseg;
  A.qb = (int)S.qb;
  A.k = k;
  A.apply_final = apply_final ? 1 : 0;
  A.largest = largest ? 1 : 0;
  A.final_act = P.final_act;
  A.yeta = P.yeta;
  A.out = list_out(workspace, S, idx_out, val_out);
  (void)hipGetLastError();   // report only this call's launch errors
  hipLaunchKernelGGL(dot_search_kernel, dim3((unsigned)S.blocks), dim3(64 * S.waves), S.lds, st,
                     A);
  launch_search_merge(A.out, S, m, k, st);
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

int64_t sg_dot_score_grid_bwd_workspace_bytes(const sg_model_t *model, int64_t m, int64_t n) {
  SgGenPlan P;
  if (!model || m < 0 || n < 0 || dot_train_plan(model, &P) != SG_OK) return -1;
  if (m > kMaxRows || n > kMaxRows) return -1;
  DotTrainGeo G;
  if (!dot_train_geo(m, n, plan_embed_dim(P), &G)) return -1;
  return G.floats * 4 + 256;
}

int32_t sg_dot_score_grid_fwd_bwd(const sg_model_t *model, const float *emb_q, int64_t ld_q,
                                  const float *emb_db, int64_t ld_db, int64_t m, int64_t n,
                                  const float *labels, int64_t ld_labels, int64_t batch_total,
                                  const float *y_stats, int32_t add_label_term, float *s_out,
                                  int64_t ld_s, float *g_emb_q, float *g_emb_db,
                                  float *loss_out, void *workspace, sg_stream_t stream) {
  if (!model || m < 0 || n < 0) return SG_ERR_ARG;
  SgGenPlan P;
  const int rc = dot_train_plan(model, &P);
  if (rc != SG_OK) return rc;
  if (m > kMaxRows || n > kMaxRows) return SG_ERR_UNSUPPORTED;
  const int E = plan_embed_dim(P);
  DotTrainGeo G;
  if (!dot_train_geo(m, n, E, &G)) return SG_ERR_UNSUPPORTED;
  if (m == 0 || n == 0) return SG_OK;
  if (!emb_q || !emb_db || !g_emb_q || !g_emb_db || !workspace ||
      ((uintptr_t)workspace & 15u) != 0 || ld_q < E || ld_db < E)
    return SG_ERR_ARG;
  if (ld_labels < n || (s_out && ld_s < n)) return SG_ERR_ARG;
  const bool broadcast = P.loss_mode == SG_LOSS_BROADCAST;
  if (broadcast && !y_stats) return SG_ERR_ARG;
  if (!broadcast && (!labels || batch_total <= 0)) return SG_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  float *ws = (float *)workspace;
  float *GS = ws + G.oGS, *blkp = ws + G.oblk;
  DotTrainArgs A;
  A.O = DotOps{emb_q, emb_db, ld_q, ld_db, m, n, E};
  A.ncb = G.ncb;
  A.ld_lab = ld_labels;
  A.ld_s = ld_s;
  A.labels = labels;
  A.y_stats = y_stats;
  A.final_act = P.final_act;
  A.loss_mode = P.loss_mode;
  A.yeta = P.yeta;
  A.inv_batch = batch_total > 0 ? 1.f / (float)batch_total : 0.f;
  A.s_out = s_out;
  A.GS = GS;
  A.blkp = blkp;
  (void)hipGetLastError();   // report only this call's launch errors
  hipLaunchKernelGGL(dot_train_fwd_kernel, dim3((unsigned)G.blocks), dim3(256), 0, st, A);
  // g_emb_q = GS · E_db (contraction over the n database rows), g_emb_db = GSᵀ · E_q (over m)
  dot_adj_launch(GS, n, 1, m, n, emb_db, ld_db, E, G.nchq, ws + G.opq, g_emb_q, st);
  dot_adj_launch(GS, 1, n, n, m, emb_q, ld_q, E, G.nchdb, ws + G.opdb, g_emb_db, st);
  if (loss_out)
    hipLaunchKernelGGL(dot_loss_kernel, dim3(1), dim3(256), 0, st, (const float *)blkp, G.blocks,
                       y_stats, (broadcast && add_label_term && y_stats) ? 1 : 0, loss_out);
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

}  // extern "C"
