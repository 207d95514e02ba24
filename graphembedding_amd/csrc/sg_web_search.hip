// sg_web_search.hip — embed-once search for graph-store (Web) models
// (include/siamese_web_search.h): the NTN score grid of sg_web_grid.hip at D in [32, 512]
// fused with a per-query running top-k, so the m x n scores never reach memory.  The
// arithmetic of one score is web_grid_kernel's, the same functions of sg_web_grid.h (the
// contract is bitwise equality with sg_web_score_grid + sg_topk_rows); the lists and their
// merge are sg_search.hip's (sg_search_lists.h).  What is new is how the two meet: the
// scores of a query come out of four wavefronts, sixteen each, and go into one list.
#include "../../include/siamese_web_search.h"
#include "sg_search_lists.h"
#include "sg_web_grid.h"

namespace {

// LDS for the lists of a workgroup's queries.  At D = 512 the two table buffers take
// 66048 B and the hand-over slots 1536 B; with 12288 B of lists a workgroup asks for
// 79872 B, so two workgroups share a CU's 160 KB at every k (k = 64: 16 queries).
constexpr int kWebListLds = 12288;
constexpr int kWebSlotBytes = 2 * 64 * kListBytes;   // two hand-over slots of 64 entries

// ---------------------------------------------------------------------------
// How a call is cut (search_split, sg_search_split.h) and its workspace
// [Q tables | candidate keys | candidate values].
// ---------------------------------------------------------------------------
struct WebSearchPlan : SearchSplit {
  int64_t q_bytes, ws_bytes;
  size_t lds;
};

// Every host check that needs no pointer: sg_web_score_grid's for the model, then
// search_split's for k, seg_cols, m and n.
int web_search_plan(const sg_model_t *model, int64_t m, int64_t n, int32_t k, int64_t seg_cols,
                    SgWebHead *H, WebSearchPlan *S) {
  if (!model || m < 0 || n < 0) return SG_ERR_ARG;
  int rc = sg_web_head_plan(model, H);
  if (rc != SG_OK) return rc;
  if (H->K > kGridMaxK) return SG_ERR_UNSUPPORTED;
  // two workgroups per CU hold the device, as for the grid (2 x 78 KB of LDS at D = 512)
  rc = search_split(SearchUnit{(int64_t)sg_num_cus() * 2, 4, kWebListLds}, m, n, k, seg_cols, S);
  if (rc != SG_OK) return rc;
  const int ns = web_dq(H->D) / 4;
  S->lds = (size_t)2 * ns * 256u + (size_t)S->qb * k * kListBytes + kWebSlotBytes;
  S->q_bytes = (m * web_dq(H->D) * 16 * 4 + 255) & ~(int64_t)255;
  S->ws_bytes = S->q_bytes + S->cand_bytes;
  return SG_OK;
}

// ---------------------------------------------------------------------------
// A workgroup owns one segment of the database and one chunk of qb queries.  For each
// 64-column block of the segment its four wavefronts load the augmented rows of their
// 16-row tiles as MFMA A operands (web_load_a) and the workgroup walks the chunk's queries
// exactly as web_grid_kernel does: Q_i staged in LDS, double-buffered, the next table's
// loads issued before this query's MFMAs and written after them, one barrier per query.
// The pipeline runs on across block boundaries (the table after a block's last query is the
// next block's first), so the buffer of a step is its parity, not the query's; only the
// A-operand reload at the top of a block waits for memory, once per block and wavefront,
// while the CU's other workgroup computes.
//
// What happens to a score: lanes c < 4 of group g of wavefront w hold the scores of columns
// j0 + 16 w + 4 g + c.  Each wavefront writes its 16 (key, value) pairs into the 64-entry
// hand-over slot of the step's parity; after the step's barrier, at the top of the next
// step, wavefront (i - q0) & 3 reads the slot, one entry per lane, and inserts the keys
// below the threshold into the list of query i (list_insert).  qb is a multiple of 4, so a
// query's list is handled by the same wavefront in every block and needs no barrier of its
// own; the slot of a parity is rewritten two steps later, after the barrier of the step
// that read it.  A tail step takes the last query's slot.  Keys of columns >= n are the
// all-ones sentinel and never enter a list.
// ---------------------------------------------------------------------------
struct WebSearchArgs : GridCommon {   // ncb counts segments here
  int64_t ld_db, seg;
  int ns;
  int apply_final, k, largest;
  ListOut out;
};

// the slot of parity p into the list of local query qi, by the wavefront that owns it
__device__ __forceinline__ void web_search_take(const uint64_t *skey, const float *sval, int p,
                                                uint64_t *lkeys, float *lvals, int64_t qi, int k,
                                                int lane) {
  const uint64_t key = skey[p * 64 + lane];
  const float s = sval[p * 64 + lane];
  uint64_t *lk = lkeys + qi * k;
  list_offer(lk, lvals + qi * k, k, lane, key, s, lk[k - 1]);
}

template <int NSMAX>
__global__ void __launch_bounds__(256) web_search_kernel(WebSearchArgs A) {
  extern __shared__ __attribute__((aligned(16))) float sQ[];   // [2][ns * 64], then the lists
  constexpr int NST = (NSMAX + 15) / 16;   // float4 of a table per thread
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15, k = A.k;
  const int ns = A.ns, qw = ns * 64, nf4 = ns * 16;
  const int64_t sgm = (int64_t)blockIdx.x % A.ncb, qc = (int64_t)blockIdx.x / A.ncb;
  const int64_t q0 = qc * A.qb;
  const int64_t q1 = q0 + A.qb < A.m ? q0 + A.qb : A.m;
  const int64_t c0 = sgm * A.seg;
  const int64_t c1 = c0 + A.seg < A.n ? c0 + A.seg : A.n;
  const int D = A.D;
  // LDS past the tables: list keys [qb][k], slot keys [2][64], list values [qb][k], slot
  // values [2][64] (qb % 4 == 0: every array starts on a multiple of 16 bytes)
  uint64_t *lkeys = (uint64_t *)(sQ + 2 * qw);
  uint64_t *skey = lkeys + (size_t)A.qb * k;
  float *lvals = (float *)(skey + 2 * 64);
  float *sval = lvals + (size_t)A.qb * k;
  for (int64_t qi = wave; qi < q1 - q0; qi += 4) list_reset(lkeys + qi * k, k, lane);
  const float usum = grid_usum(A);
  const GridCol col = grid_col(A, c, usum);   // column k = c of C
  const bool kmask = col.mask;
  const float wk = col.w;
  const float *__restrict__ Qg = A.Q;
  float4 st[NST];
  web_q_stage<NST>(sQ, Qg + q0 * qw, tid, nf4);
  __syncthreads();
  uint32_t step = 0;     // (block, query) pairs done; its parity picks the buffers and slots
  int64_t prev = -1;     // the local query whose scores wait in slot (step - 1) & 1
  for (int64_t j0 = c0; j0 < c1; j0 += 64) {
    float a[NSMAX];
    web_load_a<NSMAX>(A.edb, A.ld_db, A.n, D, j0 + 16 * wave + c, g, a);
    const int64_t jst = j0 + 16 * wave + 4 * g + c;   // the column lanes c < 4 hand over
    const bool last_blk = j0 + 64 >= c1;
    for (int64_t i = q0; i < q1; ++i, ++step) {
      const int p = step & 1;
      const float *cur = sQ + p * qw;
      float *nxt = sQ + (p ^ 1) * qw;
      const bool more = i + 1 < q1 || !last_blk;
      if (more) web_q_load<NST>(Qg + (i + 1 < q1 ? i + 1 : q0) * qw, tid, nf4, st);
      if (prev >= 0 && wave == (int)(prev & 3))
        web_search_take(skey, sval, p ^ 1, lkeys, lvals, prev, k, lane);
      const float sc = web_score<NSMAX>(a, cur, ns, lane, c, kmask, wk, usum, A.act,
                                        A.apply_final, A.final_act, A.yeta);
      if (c < 4) {
        const int e = p * 64 + 16 * wave + 4 * g + c;
        skey[e] = jst < A.n ? topk_key(sc, (uint32_t)jst, A.largest) : ~0ull;
        sval[e] = sc;
      }
      prev = i - q0;
      if (more) web_q_store<NST>(nxt, tid, nf4, st);
      __syncthreads();
    }
  }
  if (prev >= 0 && wave == (int)(prev & 3))   // c0 < c1: at least one step ran
    web_search_take(skey, sval, (step - 1) & 1, lkeys, lvals, prev, k, lane);
  // every wavefront writes the lists it kept
  for (int64_t qi = wave; qi < q1 - q0; qi += 4) {
    if (lane >= k) continue;
    const int64_t i = q0 + qi;
    const uint64_t key = lkeys[qi * k + lane];
    const float val = lvals[qi * k + lane];
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

template <int NSMAX>
void web_search_launch(const WebSearchArgs &A, const WebSearchPlan &S, hipStream_t st) {
  sg_allow_lds((const void *)web_search_kernel<NSMAX>, S.lds);
  hipLaunchKernelGGL(web_search_kernel<NSMAX>, dim3((unsigned)S.blocks), dim3(256), S.lds, st, A);
}

}  // namespace

extern "C" {

int64_t sg_web_search_topk_workspace_bytes(const sg_model_t *model, int64_t m, int64_t n,
                                           int32_t k, int64_t seg_cols) {
  SgWebHead H;
  WebSearchPlan S;
  if (web_search_plan(model, m, n, k, seg_cols, &H, &S) != SG_OK) return -1;
  return S.ws_bytes;
}

int32_t sg_web_search_topk(const sg_model_t *model, const float *emb_q, int64_t ld_q,
                           const float *emb_db, int64_t ld_db, int64_t m, int64_t n,
                           const float *params, int32_t apply_final, int32_t k, int32_t largest,
                           int64_t seg_cols, int32_t *idx_out, float *val_out,
                           void *workspace, sg_stream_t stream) {
  SgWebHead H;
  WebSearchPlan S;
  const int rc = web_search_plan(model, m, n, k, seg_cols, &H, &S);
  if (rc != SG_OK) return rc;
  if (m == 0) return SG_OK;
  if (!emb_q || !emb_db || !params || !idx_out || !workspace || ld_q < H.D || ld_db < H.D)
    return SG_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  (void)hipGetLastError();   // report only this call's launch errors
  float *Q = web_grid_tables(workspace);
  web_grid_launch_q(H, emb_q, ld_q, m, params, Q, sg_num_cus(), st);
  WebSearchArgs A;
  web_fill_grid_common(A, H, Q, emb_db, params, m, n);
  A.ncb = S.nseg;
  A.qb = (int)S.qb;
  A.ld_db = ld_db;
  A.seg = S.seg;
  A.ns = web_dq(H.D) / 4;
  A.apply_final = apply_final ? 1 : 0;
  A.k = k;
  A.largest = largest ? 1 : 0;
  A.out = list_out((char *)Q + S.q_bytes, S, idx_out, val_out);   // 16-byte aligned, as Q is
  web_dispatch_nsmax(A.ns, [&](auto nsmax) {
    web_search_launch<decltype(nsmax)::value>(A, S, st);
  });
  launch_search_merge(A.out, S, m, k, st);
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

}  // extern "C"
